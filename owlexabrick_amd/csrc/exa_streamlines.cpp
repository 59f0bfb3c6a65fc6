// exa_streamlines.cpp — exa_hip_streamlines: field lines of three channels integrated from seeds on the device and kept as
// packed polylines (kernels in exa_stream_kernels.h; include/exa_hip.h states the contract).  Count, then emit: the
// integration runs twice, the first time storing only how many vertices every direction appends and why it ended; the
// counts are scanned on the host (the call is synchronous), and the second run stores every vertex at its packed position.
#include "exa_renderer.h"

#include <cmath>
#include <cstring>
#include <new>

static void streamRelease(ExaHipRenderer *r)
{
  r->streamVertices.release(); r->streamVelocities.release(); r->streamOffsets.release();
  r->streamSeedVertex.release(); r->streamReasons.release();
  r->streamSeeds = 0; r->streamNumVertices = 0;
  r->haveStreamlines = false;
}

namespace {
struct StreamEvents {
  hipEvent_t ev[4] = { nullptr, nullptr, nullptr, nullptr };
  hipError_t create() { for (auto &e : ev) { hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; } return hipSuccess; }
  ~StreamEvents() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
};
} // namespace

// all lanes of a, at most 2^24 per launch
static hipError_t launchAll(ExaHipRenderer *r, StreamArgs &a, bool emit, hipStream_t s)
{
  for (a.laneBase = 0; a.laneBase < a.numLanes; a.laneBase += 1ull << 24) {
    const hipError_t e = EXA_FORM(r, launchStreamlines)(a, emit, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

extern "C" {

int exa_hip_streamlines(ExaHipRenderer *h, const float *seeds, uint64_t n, const int32_t channels[3], float step,
                        int32_t maxSteps, int32_t flags, uint64_t *numVertices, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_streamlines";
  if (numVertices) *numVertices = 0;
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  streamRelease(r);                      // also a failed extraction drops the previous lines
  r->streamKernelMs = 0.f;
  const int32_t known = EXA_STREAM_FORWARD | EXA_STREAM_BACKWARD | EXA_STREAM_NORMALIZE | EXA_STREAM_VELOCITIES;
  if (flags & ~known) { h->fail(std::string(fn) + ": unknown flag bits"); return 1; }
  if (!(flags & (EXA_STREAM_FORWARD | EXA_STREAM_BACKWARD))) { h->fail(std::string(fn) + ": no direction (EXA_STREAM_FORWARD, EXA_STREAM_BACKWARD or both)"); return 1; }
  if (!(std::isfinite(step) && step > 0.f)) { h->fail(std::string(fn) + ": step must be finite and > 0"); return 1; }
  if (maxSteps < 1 || maxSteps > EXA_STREAM_MAX_STEPS) { h->fail(std::string(fn) + ": maxSteps must be in 1.." + std::to_string(EXA_STREAM_MAX_STEPS)); return 1; }
  if (!channels) { h->fail(std::string(fn) + ": null channels"); return 1; }
  for (int c = 0; c < 3; c++)
    if (channels[c] < 0 || channels[c] >= h->numFields) { h->fail(std::string(fn) + ": channel out of range"); return 1; }
  hipStream_t s = (hipStream_t)hipStream;
  StreamArgs a;
  std::memset(&a, 0, sizeof(a));
  if (probeSetup(h, r, fn, false, s, a.s)) return 1;
  if (n == 0) {
    // no lines: offsets = {0}
    const unsigned long long zero = 0;
    HIP_TRY(h, r->streamOffsets.upload(&zero, 1));
    r->haveStreamlines = true;
    return 0;
  }
  if (!seeds) { h->fail(std::string(fn) + ": null seeds"); return 1; }
  // every line has a vertex at the least
  if (n > uint64_t(INT32_MAX)) { h->fail(std::string(fn) + ": more than INT32_MAX vertices (one per seed at the least): extract in parts"); return 1; }
  auto fail = [&](hipError_t e, const char *what) {
    (void)hipGetLastError();
    streamRelease(r);
    h->fail(std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
    return 1;
  };
  // past this point a failed HIP call drops what the call has allocated, like every other failure
#define STREAM_TRY(call) do { const hipError_t e_ = (call); if (e_ != hipSuccess) return fail(e_, #call); } while (0)
  const bool both = (flags & EXA_STREAM_FORWARD) && (flags & EXA_STREAM_BACKWARD);
  a.s.numChannels = 3;
  for (int c = 0; c < 3; c++) a.s.fieldOffset[c] = r->sc.channelOffset[channels[c]];
  a.numSeeds = n;
  a.numLanes = both ? 2 * n : n;
  a.step = step;
  a.maxSteps = maxSteps;
  a.flags = flags;

  DevBuf<float> devSeeds;
  DevBuf<uint32_t> counts;
  hipError_t e = devSeeds.alloc(3 * size_t(n));
  if (e == hipSuccess) e = counts.alloc(2 * size_t(n));
  if (e == hipSuccess) e = r->streamReasons.alloc(2 * size_t(n));
  if (e == hipSuccess) e = r->streamOffsets.alloc(size_t(n) + 1);
  if (e == hipSuccess) e = r->streamSeedVertex.alloc(size_t(n));
  if (e != hipSuccess) return fail(e, "no device memory for the seeds and the per-line arrays (40 bytes per seed)");
  a.seeds = devSeeds.p;
  a.counts = counts.p;
  a.reasons = r->streamReasons.p;
  StreamEvents t;
  STREAM_TRY(t.create());
  STREAM_TRY(hipMemcpyAsync(devSeeds.p, seeds, 12 * size_t(n), hipMemcpyHostToDevice, s));
  // a direction that is not requested: count 0, EXA_STREAM_END_NONE
  STREAM_TRY(hipMemsetAsync(counts.p, 0, 8 * size_t(n), s));
  STREAM_TRY(hipMemsetAsync(r->streamReasons.p, 0, 8 * size_t(n), s));
  STREAM_TRY(hipEventRecord(t.ev[0], s));
  if ((e = launchAll(r, a, false, s)) != hipSuccess) return fail(e, "the counting launch");
  STREAM_TRY(hipEventRecord(t.ev[1], s));
  // the host side of the scan: 20 bytes per seed
  std::vector<uint32_t> hostCounts, seedVertex;
  std::vector<unsigned long long> offsets;
  try {
    hostCounts.resize(2 * size_t(n));
    seedVertex.resize(size_t(n));
    offsets.resize(size_t(n) + 1);
  } catch (const std::bad_alloc &) {
    streamRelease(r);
    h->fail(std::string(fn) + ": no host memory for the scan of the counts (20 bytes per seed)");
    return 1;
  }
  STREAM_TRY(hipMemcpyAsync(hostCounts.data(), counts.p, 8 * size_t(n), hipMemcpyDeviceToHost, s));
  STREAM_TRY(hipStreamSynchronize(s));
  if (int rc = checkLoopGuard(h, r, fn, kDescentGuard)) { streamRelease(r); return rc; }
  // the scan: line i = backward vertices, the seed, forward vertices
  unsigned long long total = 0;
  for (uint64_t i = 0; i < n; i++) {
    offsets[i] = total;
    seedVertex[i] = hostCounts[2 * i];
    total += 1ull + hostCounts[2 * i] + hostCounts[2 * i + 1];
  }
  offsets[n] = total;
  if (total > uint64_t(INT32_MAX)) {
    streamRelease(r);
    h->fail(std::string(fn) + ": the lines have " + std::to_string(total) + " vertices: more than INT32_MAX (extract in parts)");
    return 1;
  }
  e = r->streamVertices.alloc(3 * size_t(total));
  if (e == hipSuccess && (flags & EXA_STREAM_VELOCITIES)) e = r->streamVelocities.alloc(3 * size_t(total));
  if (e != hipSuccess) return fail(e, "no device memory for the lines");
  STREAM_TRY(hipMemcpyAsync(r->streamOffsets.p, offsets.data(), 8 * (size_t(n) + 1), hipMemcpyHostToDevice, s));
  STREAM_TRY(hipMemcpyAsync(r->streamSeedVertex.p, seedVertex.data(), 4 * size_t(n), hipMemcpyHostToDevice, s));
  a.offsets = r->streamOffsets.p;
  a.seedVertex = r->streamSeedVertex.p;
  a.vertices = r->streamVertices.p;
  a.velocities = (flags & EXA_STREAM_VELOCITIES) ? r->streamVelocities.p : nullptr;
  STREAM_TRY(hipEventRecord(t.ev[2], s));
  if ((e = launchAll(r, a, true, s)) != hipSuccess) return fail(e, "the emitting launch");
  STREAM_TRY(hipEventRecord(t.ev[3], s));
  STREAM_TRY(hipStreamSynchronize(s));
  if (int rc = checkLoopGuard(h, r, fn, kDescentGuard)) { streamRelease(r); return rc; }
  float ms0 = 0.f, ms1 = 0.f;
  STREAM_TRY(hipEventElapsedTime(&ms0, t.ev[0], t.ev[1]));
  STREAM_TRY(hipEventElapsedTime(&ms1, t.ev[2], t.ev[3]));
#undef STREAM_TRY
  r->streamKernelMs = ms0 + ms1;
  r->streamSeeds = n;
  r->streamNumVertices = total;
  r->haveStreamlines = true;
  if (numVertices) *numVertices = total;
  return 0;
}

int exa_hip_streamlines_read(ExaHipRenderer *h, float *vertices, float *velocities, uint64_t *offsets, uint32_t *seedVertex,
                             int32_t *reasons, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_streamlines_read";
  ExaHipRenderer *r = firstChild(h);
  if (!r->haveStreamlines) { h->fail(std::string(fn) + ": no lines (exa_hip_streamlines comes first; a release or a failed extraction drops them)"); return 1; }
  if (velocities && r->streamNumVertices && !r->streamVelocities.n) { h->fail(std::string(fn) + ": the lines were extracted without EXA_STREAM_VELOCITIES"); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  const hipMemcpyKind kind = pointersAreDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t n = size_t(r->streamSeeds), nv = size_t(r->streamNumVertices);
  if (vertices && nv) HIP_TRY(h, hipMemcpyAsync(vertices, r->streamVertices.p, 12 * nv, kind, s));
  if (velocities && nv) HIP_TRY(h, hipMemcpyAsync(velocities, r->streamVelocities.p, 12 * nv, kind, s));
  if (offsets) HIP_TRY(h, hipMemcpyAsync(offsets, r->streamOffsets.p, 8 * (n + 1), kind, s));
  if (seedVertex && n) HIP_TRY(h, hipMemcpyAsync(seedVertex, r->streamSeedVertex.p, 4 * n, kind, s));
  if (reasons && n) HIP_TRY(h, hipMemcpyAsync(reasons, r->streamReasons.p, 8 * n, kind, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return 0;
}

int exa_hip_streamlines_release(ExaHipRenderer *h)
{
  if (!h) return 1;
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  streamRelease(r);
  return 0;
}

int exa_hip_streamlines_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->streamKernelMs;
  return 0;
}

} // extern "C"
