// exa_streamlines.cpp — exa_hip_streamlines: field lines of three channels integrated from seeds on the device and kept as
// packed polylines (kernels in exa_stream_kernels.h; include/exa_hip.h states the contract).  Count, then emit: the
// integration runs twice, the first time storing only how many vertices every direction appends and why it ended; the
// counts are scanned on the host (the call is synchronous), and the second run stores every vertex at its packed position.
// Behind it exa_hip_lic, the dense sibling on a plane lattice (kernel in exa_lic_kernels.h, in the same units): one launch,
// nothing counted first and nothing emitted but the image; and exa_hip_flowmap, the same integration from every point of a
// lattice with only the end state kept (kernel in exa_flowmap_kernels.h), and the stretch stencil over it.
#include "exa_renderer.h"
#include "exa_isomesh.h"

#include <cmath>
#include <cstring>
#include <new>

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
  r->lines.release();                    // also a failed extraction drops the previous lines
  r->lines.kernelMs = 0.f;
  if (!checkFlags(h, fn, flags, EXA_STREAM_FORWARD | EXA_STREAM_BACKWARD | EXA_STREAM_NORMALIZE | EXA_STREAM_VELOCITIES, "")) return 1;
  if (!(flags & (EXA_STREAM_FORWARD | EXA_STREAM_BACKWARD))) { h->fail(std::string(fn) + ": no direction (EXA_STREAM_FORWARD, EXA_STREAM_BACKWARD or both)"); return 1; }
  if (!(std::isfinite(step) && step > 0.f)) { h->fail(std::string(fn) + ": step must be finite and > 0"); return 1; }
  if (maxSteps < 1 || maxSteps > EXA_STREAM_MAX_STEPS) { h->fail(std::string(fn) + ": maxSteps must be in 1.." + std::to_string(EXA_STREAM_MAX_STEPS)); return 1; }
  if (!channels) { h->fail(std::string(fn) + ": null channels"); return 1; }
  for (int c = 0; c < 3; c++)
    if (!checkChannel(h, fn, channels[c])) return 1;
  hipStream_t s = (hipStream_t)hipStream;
  StreamArgs a;
  std::memset(&a, 0, sizeof(a));
  if (probeSetup(h, r, fn, false, s, a.s)) return 1;
  if (n == 0) {
    // no lines: offsets = {0}
    const unsigned long long zero = 0;
    HIP_TRY(h, r->lines.offsets.upload(&zero, 1));
    r->lines.have = true;
    return 0;
  }
  if (!seeds) { h->fail(std::string(fn) + ": null seeds"); return 1; }
  // every line has a vertex at the least
  if (n > uint64_t(INT32_MAX)) { h->fail(std::string(fn) + ": more than INT32_MAX vertices (one per seed at the least): extract in parts"); return 1; }
  // past this point whatever fails drops what the call has allocated
  DropUnlessCommitted<ExaHipRenderer::Streamlines> lines(r->lines);
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
  if (e == hipSuccess) e = r->lines.reasons.alloc(2 * size_t(n));
  if (e == hipSuccess) e = r->lines.offsets.alloc(size_t(n) + 1);
  if (e == hipSuccess) e = r->lines.seedVertex.alloc(size_t(n));
  if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the seeds and the per-line arrays (40 bytes per seed)", e);
  a.seeds = devSeeds.p;
  a.counts = counts.p;
  a.reasons = r->lines.reasons.p;
  TimingEvents<4> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipMemcpyAsync(devSeeds.p, seeds, 12 * size_t(n), hipMemcpyHostToDevice, s));
  // a direction that is not requested: count 0, EXA_STREAM_END_NONE
  HIP_TRY(h, hipMemsetAsync(counts.p, 0, 8 * size_t(n), s));
  HIP_TRY(h, hipMemsetAsync(r->lines.reasons.p, 0, 8 * size_t(n), s));
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  HIP_TRY(h, launchAll(r, a, false, s));
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  // the host side of the scan: 20 bytes per seed
  std::vector<uint32_t> hostCounts, seedVertex;
  std::vector<unsigned long long> offsets;
  try {
    hostCounts.resize(2 * size_t(n));
    seedVertex.resize(size_t(n));
    offsets.resize(size_t(n) + 1);
  } catch (const std::bad_alloc &) {
    h->fail(std::string(fn) + ": no host memory for the scan of the counts (20 bytes per seed)");
    return 1;
  }
  HIP_TRY(h, hipMemcpyAsync(hostCounts.data(), counts.p, 8 * size_t(n), hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (int rc = checkLoopGuard(h, r, fn, kDescentGuard)) return rc;
  // the scan: line i = backward vertices, the seed, forward vertices
  unsigned long long total = 0;
  for (uint64_t i = 0; i < n; i++) {
    offsets[i] = total;
    seedVertex[i] = hostCounts[2 * i];
    total += 1ull + hostCounts[2 * i] + hostCounts[2 * i + 1];
  }
  offsets[n] = total;
  if (total > uint64_t(INT32_MAX)) {
    h->fail(std::string(fn) + ": the lines have " + std::to_string(total) + " vertices: more than INT32_MAX (extract in parts)");
    return 1;
  }
  e = r->lines.vertices.alloc(3 * size_t(total));
  if (e == hipSuccess && (flags & EXA_STREAM_VELOCITIES)) e = r->lines.velocities.alloc(3 * size_t(total));
  if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the lines", e);
  HIP_TRY(h, hipMemcpyAsync(r->lines.offsets.p, offsets.data(), 8 * (size_t(n) + 1), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemcpyAsync(r->lines.seedVertex.p, seedVertex.data(), 4 * size_t(n), hipMemcpyHostToDevice, s));
  a.offsets = r->lines.offsets.p;
  a.seedVertex = r->lines.seedVertex.p;
  a.vertices = r->lines.vertices.p;
  a.velocities = (flags & EXA_STREAM_VELOCITIES) ? r->lines.velocities.p : nullptr;
  HIP_TRY(h, hipEventRecord(t.ev[2], s));
  HIP_TRY(h, launchAll(r, a, true, s));
  HIP_TRY(h, hipEventRecord(t.ev[3], s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (int rc = checkLoopGuard(h, r, fn, kDescentGuard)) return rc;
  float ms0 = 0.f, ms1 = 0.f;
  HIP_TRY(h, t.elapsed(0, 1, &ms0));
  HIP_TRY(h, t.elapsed(2, 3, &ms1));
  r->lines.kernelMs = ms0 + ms1;
  r->lines.seeds = n;
  r->lines.numVertices = total;
  r->lines.have = true;
  lines.commit();
  if (numVertices) *numVertices = total;
  return 0;
}

int exa_hip_streamlines_read(ExaHipRenderer *h, float *vertices, float *velocities, uint64_t *offsets, uint32_t *seedVertex,
                             int32_t *reasons, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_streamlines_read";
  ExaHipRenderer *r = firstChild(h);
  if (!r->lines.have) { h->fail(std::string(fn) + ": no lines (exa_hip_streamlines comes first; a release or a failed extraction drops them)"); return 1; }
  if (velocities && r->lines.numVertices && !r->lines.velocities.n) { h->fail(std::string(fn) + ": the lines were extracted without EXA_STREAM_VELOCITIES"); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  const hipMemcpyKind kind = pointersAreDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  const size_t n = size_t(r->lines.seeds), nv = size_t(r->lines.numVertices);
  if (vertices && nv) HIP_TRY(h, hipMemcpyAsync(vertices, r->lines.vertices.p, 12 * nv, kind, s));
  if (velocities && nv) HIP_TRY(h, hipMemcpyAsync(velocities, r->lines.velocities.p, 12 * nv, kind, s));
  if (offsets) HIP_TRY(h, hipMemcpyAsync(offsets, r->lines.offsets.p, 8 * (n + 1), kind, s));
  if (seedVertex && n) HIP_TRY(h, hipMemcpyAsync(seedVertex, r->lines.seedVertex.p, 4 * n, kind, s));
  if (reasons && n) HIP_TRY(h, hipMemcpyAsync(reasons, r->lines.reasons.p, 8 * n, kind, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return 0;
}

int exa_hip_streamlines_release(ExaHipRenderer *h)
{
  if (!h) return 1;
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  r->lines.release();
  return 0;
}

int exa_hip_streamlines_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->lines.kernelMs;
  return 0;
}

// ---- line integral convolution on a plane lattice (streamlinesKernelLic, exa_lic_kernels.h) ----
// One launch per 2^18 patches (2^24 lanes).  Host arrays pass through one device buffer of the call, {lic | sum | count |
// speed | reasons | noise}: every part a multiple of 4 bytes in front of the noise, so each is aligned to its element; a
// line crosses the whole image, so the image is not cut into tiles.
int exa_hip_lic(ExaHipRenderer *h, const ExaHipPlane *plane, const int32_t channels[3], float step, int32_t halfLength,
                const uint8_t *noise, uint32_t seed, int32_t flags, float fill, float *lic, uint32_t *sum, uint32_t *count,
                float *speed, int32_t *reasons, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_lic";
  ExaHipRenderer *r = firstChild(h);
  r->lic.kernelMs = 0.f;
  if (!plane || !channels) { h->fail(std::string(fn) + ": null argument (the plane or the channels)"); return 1; }
  for (int k = 0; k < 3; k++)
    if (!(std::isfinite(plane->origin[k]) && std::isfinite(plane->du[k]) && std::isfinite(plane->dv[k]))) {
      h->fail(std::string(fn) + ": the plane's origin, du and dv must be finite");
      return 1;
    }
  if (plane->nu < 1 || plane->nv < 1) { h->fail(std::string(fn) + ": nu and nv must be >= 1"); return 1; }
  const uint64_t n = uint64_t(plane->nu) * uint64_t(plane->nv);
  if (n > uint64_t(INT32_MAX)) { h->fail(std::string(fn) + ": an image of more than 2^31 - 1 points"); return 1; }
  // the plane's metric, every operation rounded separately
  const float *du = plane->du, *dv = plane->dv;
  const float g11 = (du[0] * du[0] + du[1] * du[1]) + du[2] * du[2];
  const float g12 = (du[0] * dv[0] + du[1] * dv[1]) + du[2] * dv[2];
  const float g22 = (dv[0] * dv[0] + dv[1] * dv[1]) + dv[2] * dv[2];
  const float p1 = g11 * g22, p2 = g12 * g12, det = p1 - p2;
  if (!std::isfinite(det) || !(det > 0.f)) {
    h->fail(std::string(fn) + ": du and dv do not span a plane (G11*G22 - G12*G12 must be finite and > 0 in float32)");
    return 1;
  }
  for (int c = 0; c < 3; c++)
    if (!checkChannel(h, fn, channels[c])) return 1;
  if (!(std::isfinite(step) && step > 0.f)) { h->fail(std::string(fn) + ": step must be finite and > 0"); return 1; }
  if (halfLength < 1 || halfLength > EXA_LIC_MAX_STEPS) { h->fail(std::string(fn) + ": halfLength must be in 1.." + std::to_string(EXA_LIC_MAX_STEPS)); return 1; }
  if (!checkFlags(h, fn, flags, 0, " (none is defined)")) return 1;
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  LicArgs a;
  std::memset(&a, 0, sizeof(a));
  if (probeSetup(h, r, fn, false, s, a.s)) return 1;
  a.s.numChannels = 3;
  for (int c = 0; c < 3; c++) a.s.fieldOffset[c] = r->sc.channelOffset[channels[c]];
  for (int k = 0; k < 3; k++) { a.origin[k] = plane->origin[k]; a.du[k] = du[k]; a.dv[k] = dv[k]; }
  a.nu = uint32_t(plane->nu); a.nv = uint32_t(plane->nv);
  a.g11 = g11; a.g12 = g12; a.g22 = g22; a.det = det;
  a.step = step;
  a.halfLength = halfLength;
  a.seed = seed;
  a.fill = fill;
  a.lanesPerPixel = r->lic.lanes;
  const uint32_t perWave = 64u / uint32_t(a.lanesPerPixel);
  a.patchShift = r->lic.patch ? 3 : (a.lanesPerPixel == 2 ? 5 : 6);
  const uint64_t pw = 1ull << a.patchShift, ph = perWave >> a.patchShift;
  a.patchesX = uint32_t((a.nu + pw - 1) / pw);
  a.numWaves = uint64_t(a.patchesX) * ((a.nv + ph - 1) / ph);

  const bool staged = !pointersAreDevice;
  DevBuf<char> stage;
  if (staged) {
    const size_t bytes = (lic ? 4 * n : 0) + (sum ? 4 * n : 0) + (count ? 4 * n : 0) + (speed ? 4 * n : 0) + (reasons ? 8 * n : 0) + (noise ? n : 0);
    const hipError_t e = stage.alloc(bytes);
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the image's arrays (up to 25 bytes per pixel with host pointers)", e);
    char *cut = stage.p;
    auto carve = [&](const void *user, size_t size) { char *part = user ? cut : nullptr; if (user) cut += size; return part; };
    a.lic = reinterpret_cast<float *>(carve(lic, 4 * n));
    a.sum = reinterpret_cast<uint32_t *>(carve(sum, 4 * n));
    a.count = reinterpret_cast<uint32_t *>(carve(count, 4 * n));
    a.speed = reinterpret_cast<float *>(carve(speed, 4 * n));
    a.reasons = reinterpret_cast<int32_t *>(carve(reasons, 8 * n));
    a.noise = reinterpret_cast<const uint8_t *>(carve(noise, n));
    if (noise) HIP_TRY(h, hipMemcpyAsync(const_cast<uint8_t *>(a.noise), noise, n, hipMemcpyHostToDevice, s));
  } else {
    a.lic = lic; a.sum = sum; a.count = count; a.speed = speed; a.reasons = reasons; a.noise = noise;
  }
  TimingEvents<2> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  for (a.waveBase = 0; a.waveBase < a.numWaves; a.waveBase += 1ull << 18) HIP_TRY(h, EXA_FORM(r, launchLic)(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  if (staged) {
    if (lic) HIP_TRY(h, hipMemcpyAsync(lic, a.lic, 4 * n, hipMemcpyDeviceToHost, s));
    if (sum) HIP_TRY(h, hipMemcpyAsync(sum, a.sum, 4 * n, hipMemcpyDeviceToHost, s));
    if (count) HIP_TRY(h, hipMemcpyAsync(count, a.count, 4 * n, hipMemcpyDeviceToHost, s));
    if (speed) HIP_TRY(h, hipMemcpyAsync(speed, a.speed, 4 * n, hipMemcpyDeviceToHost, s));
    if (reasons) HIP_TRY(h, hipMemcpyAsync(reasons, a.reasons, 8 * n, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(h, hipStreamSynchronize(s));
  if (int rc = checkLoopGuard(h, r, fn, kDescentGuard)) return rc;
  HIP_TRY(h, t.elapsed(0, 1, &r->lic.kernelMs));
  return 0;
}

int exa_hip_lic_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->lic.kernelMs;
  return 0;
}

// ---- the flow map of a lattice and its stretch (streamlinesKernelFlowmap, exa_flowmap_kernels.h; isoLatticeStretchKernel,
// exa_isomesh.hip) ----
// The extents 2^shift[a] of a wave's patch of 64 lattice points.  patch 0: 64 along x.  patch 1: 4 x 4 x 4; an axis shorter
// than 4 gets the largest power of two it holds, and what it frees goes to x, y and z in turn, wherever the lattice is longer
// than the patch (to x when it is nowhere).
static void flowmapPatch(int patch, const int32_t dims[3], uint32_t shift[3])
{
  shift[0] = 6; shift[1] = shift[2] = 0;
  if (!patch) return;
  int spare = 0;
  for (int k = 0; k < 3; k++) {
    shift[k] = dims[k] >= 4 ? 2 : (dims[k] >= 2 ? 1 : 0);
    spare += 2 - int(shift[k]);
  }
  for (int turn = 0; spare > 0 && turn < 18; turn++) {
    const int k = turn % 3;
    if (int64_t(dims[k]) > (int64_t(1) << shift[k])) { shift[k]++; spare--; }
  }
  shift[0] += uint32_t(spare);
}

int exa_hip_flowmap(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t channels[3],
                    float step, int32_t numSteps, int32_t flags, float fill, float *end, uint32_t *steps, int32_t *reasons,
                    float *stretch, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_flowmap";
  ExaHipRenderer *r = firstChild(h);
  r->flowmap.ms[0] = r->flowmap.ms[1] = 0.f;
  if (!lo || !hi || !dims || !channels) { h->fail(std::string(fn) + ": null argument (lo, hi, dims or channels)"); return 1; }
  for (int k = 0; k < 3; k++) {
    if (!(std::isfinite(lo[k]) && std::isfinite(hi[k]) && hi[k] > lo[k])) { h->fail(std::string(fn) + ": the box needs finite lo < hi on every axis"); return 1; }
    if (dims[k] < 1) { h->fail(std::string(fn) + ": dims must be >= 1 on every axis"); return 1; }
  }
  const uint64_t n = uint64_t(dims[0]) * uint64_t(dims[1]) * uint64_t(dims[2]);       // each < 2^31: the product of two fits
  if (uint64_t(dims[0]) * uint64_t(dims[1]) > uint64_t(INT32_MAX) || n > uint64_t(INT32_MAX)) {
    h->fail(std::string(fn) + ": a lattice of more than 2^31 - 1 points");
    return 1;
  }
  for (int c = 0; c < 3; c++)
    if (!checkChannel(h, fn, channels[c])) return 1;
  if (!(std::isfinite(step) && step > 0.f)) { h->fail(std::string(fn) + ": step must be finite and > 0"); return 1; }
  if (numSteps < 1 || numSteps > EXA_STREAM_MAX_STEPS) { h->fail(std::string(fn) + ": numSteps must be in 1.." + std::to_string(EXA_STREAM_MAX_STEPS)); return 1; }
  if (!checkFlags(h, fn, flags, EXA_FLOWMAP_FORWARD | EXA_FLOWMAP_BACKWARD, "")) return 1;
  if (flags != EXA_FLOWMAP_FORWARD && flags != EXA_FLOWMAP_BACKWARD) {
    h->fail(std::string(fn) + ": exactly one direction (EXA_FLOWMAP_FORWARD or EXA_FLOWMAP_BACKWARD)");
    return 1;
  }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  FlowmapArgs a;
  std::memset(&a, 0, sizeof(a));
  if (probeSetup(h, r, fn, false, s, a.s)) return 1;
  a.s.numChannels = 3;
  for (int c = 0; c < 3; c++) a.s.fieldOffset[c] = r->sc.channelOffset[channels[c]];
  for (int k = 0; k < 3; k++) { a.lo[k] = lo[k]; a.cell[k] = (hi[k] - lo[k]) / float(dims[k]); }
  a.nx = uint32_t(dims[0]); a.ny = uint32_t(dims[1]); a.nz = uint32_t(dims[2]);
  a.hs = flags == EXA_FLOWMAP_FORWARD ? step : -step;
  a.numSteps = numSteps;
  flowmapPatch(r->flowmap.patch, dims, a.shift);
  auto patches = [&](int k) { return (uint64_t(dims[k]) + (1ull << a.shift[k]) - 1) >> a.shift[k]; };
  a.patchesX = uint32_t(patches(0));
  a.patchesY = uint32_t(patches(1));
  a.numWaves = patches(0) * patches(1) * patches(2);

  // One device buffer of the call, {end | steps | reasons | stretch}: with host pointers every array the caller asks for,
  // with device pointers none of them; in both cases the flow map the stretch reads (end, reasons) where the caller does
  // not ask for it.
  const bool staged = !pointersAreDevice;
  auto own = [&](const void *user, bool needed) { return user ? staged : needed; };
  const bool ownEnd = own(end, stretch != nullptr), ownSteps = own(steps, false), ownReasons = own(reasons, stretch != nullptr),
             ownStretch = own(stretch, false);
  DevBuf<char> work;
  const size_t bytes = (ownEnd ? 12 * n : 0) + (ownSteps ? 4 * n : 0) + (ownReasons ? 4 * n : 0) + (ownStretch ? 4 * n : 0);
  if (bytes) {
    const hipError_t e = work.alloc(bytes);
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the flow map (up to 24 bytes per point with host pointers, up to 16 with device pointers)", e);
  }
  char *cut = work.p;
  auto carve = [&](bool mine, void *user, size_t size) { char *part = mine ? cut : static_cast<char *>(user); if (mine) cut += size; return part; };
  a.end = reinterpret_cast<float *>(carve(ownEnd, end, 12 * n));
  a.steps = reinterpret_cast<uint32_t *>(carve(ownSteps, steps, 4 * n));
  a.reasons = reinterpret_cast<int32_t *>(carve(ownReasons, reasons, 4 * n));
  IsoStretchArgs st;
  std::memset(&st, 0, sizeof(st));
  st.stretch = reinterpret_cast<float *>(carve(ownStretch, stretch, 4 * n));
  st.end = a.end; st.reasons = a.reasons;
  st.numPoints = uint32_t(n);
  st.nx = a.nx; st.ny = a.ny; st.nz = a.nz;
  for (int k = 0; k < 3; k++) { st.lo[k] = a.lo[k]; st.cell[k] = a.cell[k]; }
  st.fill = fill;

  TimingEvents<3> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  if (a.end || a.steps || a.reasons)
    for (a.waveBase = 0; a.waveBase < a.numWaves; a.waveBase += 1ull << 18) HIP_TRY(h, EXA_FORM(r, launchFlowmap)(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  if (st.stretch) HIP_TRY(h, launchIsoLatticeStretch(st, s));
  HIP_TRY(h, hipEventRecord(t.ev[2], s));
  if (staged) {
    if (end) HIP_TRY(h, hipMemcpyAsync(end, a.end, 12 * n, hipMemcpyDeviceToHost, s));
    if (steps) HIP_TRY(h, hipMemcpyAsync(steps, a.steps, 4 * n, hipMemcpyDeviceToHost, s));
    if (reasons) HIP_TRY(h, hipMemcpyAsync(reasons, a.reasons, 4 * n, hipMemcpyDeviceToHost, s));
    if (stretch) HIP_TRY(h, hipMemcpyAsync(stretch, st.stretch, 4 * n, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(h, hipStreamSynchronize(s));
  if (int rc = checkLoopGuard(h, r, fn, kDescentGuard)) return rc;
  float ms0 = 0.f, ms1 = 0.f;
  HIP_TRY(h, t.elapsed(0, 1, &ms0));
  HIP_TRY(h, t.elapsed(1, 2, &ms1));
  r->flowmap.ms[0] = ms0;
  r->flowmap.ms[1] = ms1;
  return 0;
}

int exa_hip_flowmap_ms(ExaHipRenderer *h, float ms[2])
{
  if (!h || !ms) return 1;
  ms[0] = firstChild(h)->flowmap.ms[0];
  ms[1] = firstChild(h)->flowmap.ms[1];
  return 0;
}

} // extern "C"
