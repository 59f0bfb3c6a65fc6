// exa_probe.cpp — reading the reconstructed field outside a frame: the point probes (exa_hip_sample_points,
// exa_hip_resample; kernels in exa_sample_kernels.h), the quantities derived from three channels' velocity gradient tensor
// (exa_hip_sample_derived, exa_hip_resample_derived), the projections along rays (exa_hip_project) and the iso-crossings along
// the same rays (exa_hip_raycast_iso) in the same file, the field on the triangles of a mesh (exa_hip_sample_triangles), and
// the iso-surface extraction on a sampled lattice (exa_hip_isosurface, exa_hip_isosurface_derived; exa_isomesh.hip) with the
// contour lines on a plane lattice beside it (exa_hip_isolines, exa_hip_isolines_derived; the same unit) and the connected
// regions of field >= iso on the lattice (exa_hip_regions, exa_hip_regions_derived; the same unit), its basins, one per peak
// (exa_hip_basins, exa_hip_basins_derived; the same unit), the critical points of a flow on it (exa_hip_critical_points;
// the same unit), the profiles and phase plots of fields on it (exa_hip_profile; the same unit), and the distance transform
// of a set of its points (exa_hip_distance, exa_hip_distance_derived, exa_hip_distance_mask; the same unit).
#include "exa_renderer.h"
#include "exa_isomesh.h"

#include <cmath>
#include <cstring>
#include <functional>

// after a synchronous probe: the descent's loop guard (checkLoopGuard)
const char *const kDescentGuard = ": the kd descent's loop guard tripped (malformed kd-tree?)";

// what the probes (and exa_streamlines.cpp) share: the renderer that runs them (a multi-device handle: the one of devices[0]),
// the checks, a pending brick order applied (render does the same: the probes read `begin` through the march headers the
// permutation patches)
int probeSetup(ExaHipRenderer *h, ExaHipRenderer *r, const char *fn, bool world, hipStream_t s, SampleArgs &a)
{
  if (!r->haveKd) {
    h->fail(std::string(fn) + ": the scene has no region kd-tree (ExaHipScene.kdNodes): the probes locate a point's region with it "
            "(the LBVH is refit to the region activity and cannot)");
    return 1;
  }
  if (world && !r->haveFs) { h->fail(std::string(fn) + ": world space needs a frame state (the voxelSpaceTransform of exa_hip_set_frame_state)"); return 1; }
  if (r->applyBrickOrder(s)) { h->fail(r->err); return 1; }
  std::memset(&a, 0, sizeof(a));
  a.leafHdr = r->leafHdr.p;
  a.scalars = r->scalars.p;
  a.kdNodes = r->kdNodes.p;
  a.regionRec = r->regionRec.p;
  a.kdRoot = r->kdRoot;
  a.maxSteps = (int32_t)std::min<uint64_t>(r->kdNodes.n + 1, INT32_MAX);
  for (int k = 0; k < 3; k++) { a.kdLo[k] = r->kdLo[k]; a.kdHi[k] = r->kdHi[k]; }
  a.errorFlag = r->errorFlag.p;
  a.world = world ? 1 : 0;
  if (world) a.fs = r->fs;
  return 0;
}

extern "C" {

// ---- point probes ----
// Host arrays pass through the handle's staging buffer in chunks of at most kProbeStageBytes; a launch covers at most
// kProbeLaunch points (a grid patch holds one point at the least: 64 x that many lanes stay below 2^32).
static const uint64_t kProbeStageBytes = 64ull << 20, kProbeLaunch = 1ull << 24;

// the next `bytes` of the staging buffer for a part of a chunk, nullptr for a part the call does not have; the parts come in
// an order that leaves each aligned to its element
static char *carve(char *&at, bool wanted, uint64_t bytes)
{
  if (!wanted) return nullptr;
  char *part = at;
  at += bytes;
  return part;
}

int exa_hip_sample_points(ExaHipRenderer *h, const float *points, uint64_t n, const int32_t *channels, int32_t numChannels,
                          int32_t flags, float fill, float *values, float *gradients, int32_t *status,
                          int32_t pointersAreDevice, void *hipStream, int32_t async)
{
  if (!h) return 1;
  const char *fn = "exa_hip_sample_points";
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED, "")) return 1;
  const bool grad = (flags & EXA_SAMPLE_GRADIENT) != 0;
  if ((flags & EXA_SAMPLE_GRADIENT_NORMALIZED) && !grad) { h->fail(std::string(fn) + ": EXA_SAMPLE_GRADIENT_NORMALIZED needs EXA_SAMPLE_GRADIENT"); return 1; }
  if (!channels || numChannels < 1 || numChannels > EXA_MAX_CHANNELS) { h->fail(std::string(fn) + ": 1..10 channels required"); return 1; }
  for (int c = 0; c < numChannels; c++)
    if (!checkChannel(h, fn, channels[c])) return 1;
  if (n == 0) return 0;
  if (!points || !values || (grad && !gradients)) { h->fail(std::string(fn) + ": null array (points, values, or gradients with EXA_SAMPLE_GRADIENT)"); return 1; }
  if (n > (UINT64_MAX / 12) / uint64_t(numChannels)) { h->fail(std::string(fn) + ": too many points"); return 1; }
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  SampleArgs a;
  if (probeSetup(h, r, fn, (flags & EXA_SAMPLE_WORLD_SPACE) != 0, s, a)) return 1;
  a.fill = fill;
  a.normalized = (flags & EXA_SAMPLE_GRADIENT_NORMALIZED) ? 1 : 0;
  a.numChannels = numChannels;
  for (int c = 0; c < numChannels; c++) a.fieldOffset[c] = r->sc.channelOffset[channels[c]];
  const uint64_t nch = uint64_t(numChannels);
  if (pointersAreDevice) {
    for (uint64_t at = 0; at < n; at += kProbeLaunch) {
      a.count = std::min(kProbeLaunch, n - at);
      a.points = points + 3 * at;
      a.values = values + at * nch;
      a.gradients = grad ? gradients + 3 * at * nch : nullptr;
      a.status = status ? status + at * nch : nullptr;
      HIP_TRY(h, EXA_FORM(r, launchSamplePoints)(a, grad, s));
    }
    if (async) return 0;
    HIP_TRY(h, hipStreamSynchronize(s));
    return checkLoopGuard(h, r, fn, kDescentGuard);
  }
  // host arrays: chunk by chunk through the staging buffer {points | values | gradients | status}
  const uint64_t perPoint = 12 + nch * 4 * (1 + (grad ? 3 : 0) + (status ? 1 : 0));
  const uint64_t chunk = std::max<uint64_t>(1, std::min(kProbeLaunch, kProbeStageBytes / perPoint));
  const uint64_t need = std::min(n, chunk) * perPoint;
  if (r->probes.stage.n < need) HIP_TRY(h, r->probes.stage.alloc(need));
  for (uint64_t at = 0; at < n; at += chunk) {
    const uint64_t m = std::min(chunk, n - at);
    char *cut = r->probes.stage.p;
    a.count = m;
    a.points = reinterpret_cast<const float *>(carve(cut, true, 12 * m));
    a.values = reinterpret_cast<float *>(carve(cut, true, 4 * m * nch));
    a.gradients = reinterpret_cast<float *>(carve(cut, grad, 12 * m * nch));
    a.status = reinterpret_cast<int32_t *>(carve(cut, status != nullptr, 4 * m * nch));
    HIP_TRY(h, hipMemcpyAsync(r->probes.stage.p, points + 3 * at, 12 * m, hipMemcpyHostToDevice, s));
    HIP_TRY(h, EXA_FORM(r, launchSamplePoints)(a, grad, s));
    HIP_TRY(h, hipMemcpyAsync(values + at * nch, a.values, 4 * m * nch, hipMemcpyDeviceToHost, s));
    if (grad) HIP_TRY(h, hipMemcpyAsync(gradients + 3 * at * nch, a.gradients, 12 * m * nch, hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, hipMemcpyAsync(status + at * nch, a.status, 4 * m * nch, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
  }
  return checkLoopGuard(h, r, fn, kDescentGuard);
}

// ---- derived quantities (sampleDerivedPointsKernel, sampleDerivedGridKernel) ----
// the number of components of a quantity of three channels, 0 after h->fail for an unknown quantity or a bad channel
static int derivedComponents(ExaHipRenderer *h, const char *fn, const int32_t *channels, int32_t quantity)
{
  if (quantity < 0 || quantity >= EXA_DERIVED_QUANTITIES) { h->fail(std::string(fn) + ": unknown quantity (EXA_DERIVED_*)"); return 0; }
  if (!channels) { h->fail(std::string(fn) + ": null channels (three are required)"); return 0; }
  for (int c = 0; c < 3; c++)
    if (!checkChannel(h, fn, channels[c])) return 0;
  return quantity == EXA_DERIVED_VORTICITY ? 3 : 1;
}

// the same for a call that needs a one-component quantity: false after h->fail, for three components in the caller's words
// ("a surface needs", "regions need")
static bool oneComponent(ExaHipRenderer *h, const char *fn, const int32_t *channels, int32_t quantity, const char *needs)
{
  const int comps = derivedComponents(h, fn, channels, quantity);
  if (comps > 1) h->fail(std::string(fn) + ": " + needs + " a one-component quantity (EXA_DERIVED_VORTICITY has three)");
  return comps == 1;
}

static void derivedArgs(SampleArgs &a, const ExaHipRenderer *r, const int32_t *channels, int32_t quantity, int components)
{
  a.numChannels = 3;
  for (int c = 0; c < 3; c++) a.fieldOffset[c] = r->sc.channelOffset[channels[c]];
  a.quantity = quantity;
  a.components = components;
}

int exa_hip_sample_derived(ExaHipRenderer *h, const float *points, uint64_t n, const int32_t channels[3], int32_t quantity,
                           int32_t flags, float fill, float *out, int32_t *status, int32_t pointersAreDevice, void *hipStream,
                           int32_t async)
{
  if (!h) return 1;
  const char *fn = "exa_hip_sample_derived";
  ExaHipRenderer *r = firstChild(h);
  r->derived.kernelMs = 0.f;
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE, " (only EXA_SAMPLE_WORLD_SPACE applies)")) return 1;
  const int comps = derivedComponents(h, fn, channels, quantity);
  if (!comps) return 1;
  if (n == 0) return 0;
  if (!points || !out) { h->fail(std::string(fn) + ": null array (points or out)"); return 1; }
  if (n > UINT64_MAX / 12) { h->fail(std::string(fn) + ": too many points"); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  SampleArgs a;
  if (probeSetup(h, r, fn, (flags & EXA_SAMPLE_WORLD_SPACE) != 0, s, a)) return 1;
  a.fill = fill;
  derivedArgs(a, r, channels, quantity, comps);
  const uint64_t nc = uint64_t(comps);
  TimingEvents<2> t;
  HIP_TRY(h, t.create());
  if (pointersAreDevice) {
    if (!async) HIP_TRY(h, hipEventRecord(t.ev[0], s));
    for (uint64_t at = 0; at < n; at += kProbeLaunch) {
      a.count = std::min(kProbeLaunch, n - at);
      a.points = points + 3 * at;
      a.values = out + at * nc;
      a.status = status ? status + at : nullptr;
      HIP_TRY(h, EXA_FORM(r, launchSampleDerivedPoints)(a, s));
    }
    if (async) return 0;
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, t.elapsed(0, 1, &r->derived.kernelMs));
    return checkLoopGuard(h, r, fn, kDescentGuard);
  }
  // host arrays: chunk by chunk through the staging buffer {points | out | status}
  const uint64_t perPoint = 12 + 4 * nc + (status ? 4 : 0);
  const uint64_t chunk = std::max<uint64_t>(1, std::min(kProbeLaunch, kProbeStageBytes / perPoint));
  const uint64_t need = std::min(n, chunk) * perPoint;
  if (r->probes.stage.n < need) HIP_TRY(h, r->probes.stage.alloc(need));
  float total = 0.f;
  for (uint64_t at = 0; at < n; at += chunk) {
    const uint64_t m = std::min(chunk, n - at);
    char *cut = r->probes.stage.p;
    a.count = m;
    a.points = reinterpret_cast<const float *>(carve(cut, true, 12 * m));
    a.values = reinterpret_cast<float *>(carve(cut, true, 4 * m * nc));
    a.status = reinterpret_cast<int32_t *>(carve(cut, status != nullptr, 4 * m));
    HIP_TRY(h, hipMemcpyAsync(r->probes.stage.p, points + 3 * at, 12 * m, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(t.ev[0], s));
    HIP_TRY(h, EXA_FORM(r, launchSampleDerivedPoints)(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(out + at * nc, a.values, 4 * m * nc, hipMemcpyDeviceToHost, s));
    if (status) HIP_TRY(h, hipMemcpyAsync(status + at, a.status, 4 * m, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(h, t.elapsed(0, 1, &ms));
    total += ms;
  }
  r->derived.kernelMs = total;
  return checkLoopGuard(h, r, fn, kDescentGuard);
}

// exa_hip_resample (quantity < 0: the one channel channels[0]) and exa_hip_resample_derived: the checks, the lattice and its
// boxes are the same; the derived call stores `components` floats per lattice point and times its kernels
static int resampleLattice(ExaHipRenderer *h, const char *fn, const float lo[3], const float hi[3], const int32_t dims[3],
                           const int32_t *channels, int32_t quantity, int32_t flags, float fill, float *out, int32_t dstIsDevice,
                           void *hipStream, int32_t async)
{
  const bool derived = quantity >= 0;
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE, " (only EXA_SAMPLE_WORLD_SPACE applies)")) return 1;
  if (!lo || !hi || !dims || !out) { h->fail(std::string(fn) + ": null argument"); return 1; }
  for (int k = 0; k < 3; k++) {
    if (!(std::isfinite(lo[k]) && std::isfinite(hi[k]) && hi[k] > lo[k])) { h->fail(std::string(fn) + ": the box needs finite lo < hi on every axis"); return 1; }
    if (dims[k] < 1) { h->fail(std::string(fn) + ": dims must be >= 1 on every axis"); return 1; }
  }
  int comps = 1;
  if (derived) {
    comps = derivedComponents(h, fn, channels, quantity);
    if (!comps) return 1;
  } else if (!checkChannel(h, fn, channels[0])) return 1;
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  SampleArgs a;
  if (probeSetup(h, r, fn, (flags & EXA_SAMPLE_WORLD_SPACE) != 0, s, a)) return 1;
  a.fill = fill;
  if (derived) derivedArgs(a, r, channels, quantity, comps);
  else { a.numChannels = 1; a.fieldOffset[0] = r->sc.channelOffset[channels[0]]; }
  for (int k = 0; k < 3; k++) { a.lo[k] = lo[k]; a.step[k] = (hi[k] - lo[k]) / float(dims[k]); }
  static const int kShape[kSamplePatchShapes][3] = { { 64, 1, 1 }, { 16, 4, 1 }, { 8, 8, 1 }, { 4, 4, 4 } };
  const int *ps = kShape[r->probes.patch];
  const uint64_t nx = uint64_t(dims[0]), ny = uint64_t(dims[1]), nz = uint64_t(dims[2]), nc = uint64_t(comps);
  // boxes of at most kProbeLaunch points (a host destination: at most what kProbeStageBytes hold): whole slabs of z, else
  // rows of one slice, else pieces of one row — each one contiguous in the output, so a host destination takes one copy per box
  const uint64_t cap = dstIsDevice ? kProbeLaunch : std::min(kProbeLaunch, kProbeStageBytes / (4 * nc));
  const uint64_t bx = std::min(nx, cap), by = std::min(ny, std::max<uint64_t>(1, cap / bx)),
                 bz = std::min(nz, std::max<uint64_t>(1, cap / (bx * by)));
  if (!dstIsDevice && r->probes.stage.n < bx * by * bz * nc * 4) HIP_TRY(h, r->probes.stage.alloc(bx * by * bz * nc * 4));
  // the derived call's kernel time: a host destination synchronises box by box, a device destination once behind the last box
  const bool timed = derived && !(dstIsDevice && async);
  TimingEvents<2> t;
  if (timed) HIP_TRY(h, t.create());
  float total = 0.f, ms = 0.f;
  if (timed && dstIsDevice) HIP_TRY(h, hipEventRecord(t.ev[0], s));
  for (uint64_t z0 = 0; z0 < nz; z0 += bz)
    for (uint64_t y0 = 0; y0 < ny; y0 += by)
      for (uint64_t x0 = 0; x0 < nx; x0 += bx) {
        const uint64_t ex = std::min(bx, nx - x0), ey = std::min(by, ny - y0), ez = std::min(bz, nz - z0);
        a.box0[0] = int32_t(x0); a.box0[1] = int32_t(y0); a.box0[2] = int32_t(z0);
        a.box1[0] = int32_t(x0 + ex); a.box1[1] = int32_t(y0 + ey); a.box1[2] = int32_t(z0 + ez);
        a.patchesX = (ex + ps[0] - 1) / ps[0];
        a.patchesY = (ey + ps[1] - 1) / ps[1];
        a.numPatches = a.patchesX * a.patchesY * ((ez + ps[2] - 1) / ps[2]);
        const uint64_t first = ((z0 * ny + y0) * nx + x0) * nc;
        if (dstIsDevice) {
          a.out = out + first; a.strideY = nx; a.strideZ = nx * ny;
        } else {
          a.out = reinterpret_cast<float *>(r->probes.stage.p); a.strideY = ex; a.strideZ = ex * ey;
        }
        if (timed && !dstIsDevice) HIP_TRY(h, hipEventRecord(t.ev[0], s));
        if (derived) HIP_TRY(h, EXA_FORM(r, launchSampleDerivedGrid)(a, r->probes.patch, r->probes.uniform != 0, s));
        else HIP_TRY(h, EXA_FORM(r, launchSampleGrid)(a, r->probes.patch, r->probes.uniform != 0, s));
        if (!dstIsDevice) {
          if (timed) HIP_TRY(h, hipEventRecord(t.ev[1], s));
          HIP_TRY(h, hipMemcpyAsync(out + first, a.out, ex * ey * ez * nc * sizeof(float), hipMemcpyDeviceToHost, s));
          HIP_TRY(h, hipStreamSynchronize(s));
          if (timed) { HIP_TRY(h, t.elapsed(0, 1, &ms)); total += ms; }
        }
      }
  if (dstIsDevice && async) return 0;
  if (timed && dstIsDevice) HIP_TRY(h, hipEventRecord(t.ev[1], s));
  HIP_TRY(h, hipStreamSynchronize(s));
  if (timed && dstIsDevice) HIP_TRY(h, t.elapsed(0, 1, &total));
  if (derived) r->derived.kernelMs = total;
  return checkLoopGuard(h, r, fn, kDescentGuard);
}

int exa_hip_resample(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel,
                     int32_t flags, float fill, float *out, int32_t dstIsDevice, void *hipStream, int32_t async)
{
  if (!h) return 1;
  return resampleLattice(h, "exa_hip_resample", lo, hi, dims, &channel, -1, flags, fill, out, dstIsDevice, hipStream, async);
}

int exa_hip_resample_derived(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t channels[3],
                             int32_t quantity, int32_t flags, float fill, float *out, int32_t dstIsDevice, void *hipStream,
                             int32_t async)
{
  if (!h) return 1;
  firstChild(h)->derived.kernelMs = 0.f;
  // a quantity below 0 would mean exa_hip_resample's one channel to resampleLattice
  if (quantity < 0) { h->fail("exa_hip_resample_derived: unknown quantity (EXA_DERIVED_*)"); return 1; }
  return resampleLattice(h, "exa_hip_resample_derived", lo, hi, dims, channels, quantity, flags, fill, out, dstIsDevice, hipStream, async);
}

int exa_hip_derived_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->derived.kernelMs;
  return 0;
}

// ---- rays: the projections (sampleRaysKernel) and the iso-crossings (sampleCrossingsKernel) ----
// what both calls refuse of their flags, rays and channel
static int checkRays(ExaHipRenderer *h, const char *fn, const ExaHipRays *rays, int32_t channel, int32_t flags)
{
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_PROJECT_NORMALIZE, " (EXA_SAMPLE_WORLD_SPACE and EXA_PROJECT_NORMALIZE apply)")) return 1;
  if (!rays) { h->fail(std::string(fn) + ": null rays"); return 1; }
  const float *vec[6] = { rays->org, rays->orgDu, rays->orgDv, rays->dir, rays->dirDu, rays->dirDv };
  bool finite = std::isfinite(rays->tmin) && std::isfinite(rays->dt);
  for (const float *v : vec)
    for (int k = 0; k < 3; k++) finite = finite && std::isfinite(v[k]);
  if (!finite) { h->fail(std::string(fn) + ": a float of the rays is not finite"); return 1; }
  if (!(rays->dt > 0.f)) { h->fail(std::string(fn) + ": dt must be > 0"); return 1; }
  if (rays->numSamples < 1 || rays->numSamples > EXA_PROJECT_MAX_SAMPLES) { h->fail(std::string(fn) + ": numSamples must be in 1.." + std::to_string(EXA_PROJECT_MAX_SAMPLES)); return 1; }
  const float tEnd = rays->tmin + float(rays->numSamples) * rays->dt;
  if (!std::isfinite(tEnd)) { h->fail(std::string(fn) + ": tmin + numSamples * dt is not finite in float32"); return 1; }
  if (rays->width < 1 || rays->height < 1 || uint64_t(rays->width) * uint64_t(rays->height) > uint64_t(INT32_MAX)) {
    h->fail(std::string(fn) + ": width and height must be >= 1 and width * height <= 2^31 - 1");
    return 1;
  }
  if (!checkChannel(h, fn, channel)) return 1;
  return 0;
}

// after checkRays, on r's device: probeSetup and the rays' part of the kernels' arguments (the tile: rayTiles)
static int rayArgs(ExaHipRenderer *h, ExaHipRenderer *r, const char *fn, const ExaHipRays *rays, int32_t channel, int32_t flags,
                   hipStream_t s, RayArgs &a)
{
  std::memset(&a, 0, sizeof(a));
  if (probeSetup(h, r, fn, (flags & EXA_SAMPLE_WORLD_SPACE) != 0, s, a.s)) return 1;
  a.s.numChannels = 1;
  a.s.fieldOffset[0] = r->sc.channelOffset[channel];
  a.rays = *rays;
  a.normalize = (flags & EXA_PROJECT_NORMALIZE) ? 1 : 0;
  return 0;
}

// an optional output of one element per pixel: the caller's array (NULL: skipped), the element's size and where the kernel
// stores the current tile
struct RayOutput { char *user; uint64_t size; char *dev; };

// The image goes tile by tile: a tile is at most kProjectTileWidth pixels wide and holds at most kProbeLaunch pixels — host
// outputs: at most what kProbeStageBytes of the staging buffer hold —, whole 8 x 8 patches except at the image's edges.
// Per tile: a's tile and every outs[k].dev set — a staged tile carves the staging buffer in the order of outs, which must
// leave every part aligned to its element —, launchTile() between two events, a staged tile's copies, the synchronisation.
// kernelMs: the device time between the events, summed.
static const uint64_t kProjectTileWidth = 4096;

static int rayTiles(ExaHipRenderer *h, ExaHipRenderer *r, RayArgs &a, RayOutput *outs, int numOuts, bool pointersAreDevice,
                    hipStream_t s, float &kernelMs, const std::function<hipError_t()> &launchTile)
{
  const uint64_t W = uint64_t(a.rays.width), H = uint64_t(a.rays.height);
  RayOutput *const outsEnd = outs + numOuts;
  uint64_t perPixel = 0;
  for (const RayOutput *o = outs; o != outsEnd; o++) perPixel += o->user ? o->size : 0;
  const bool staged = !pointersAreDevice && perPixel > 0;
  const uint64_t cap = staged ? std::min(kProbeLaunch, kProbeStageBytes / perPixel) : kProbeLaunch;
  const uint64_t tw = std::min(W, kProjectTileWidth), th = std::min(H, std::max<uint64_t>(8, (cap / tw) & ~uint64_t(7)));
  if (staged && r->probes.stage.n < tw * th * perPixel) HIP_TRY(h, r->probes.stage.alloc(tw * th * perPixel));
  TimingEvents<2> t;
  HIP_TRY(h, t.create());
  float total = 0.f;
  for (uint64_t y0 = 0; y0 < H; y0 += th)
    for (uint64_t x0 = 0; x0 < W; x0 += tw) {
      const uint64_t ex = std::min(tw, W - x0), ey = std::min(th, H - y0), first = y0 * W + x0;
      a.x0 = int32_t(x0); a.y0 = int32_t(y0); a.x1 = int32_t(x0 + ex); a.y1 = int32_t(y0 + ey);
      a.patchesX = uint32_t((ex + 7) / 8);
      a.numPatches = uint64_t(a.patchesX) * ((ey + 7) / 8);
      // a staged tile: rows of ex pixels in the staging buffer; else straight into the caller's device arrays
      char *cut = r->probes.stage.p;
      a.strideY = staged ? ex : W;
      for (RayOutput *o = outs; o != outsEnd; o++)
        o->dev = staged ? carve(cut, o->user != nullptr, o->size * ex * ey) : (o->user ? o->user + o->size * first : nullptr);
      HIP_TRY(h, hipEventRecord(t.ev[0], s));
      HIP_TRY(h, launchTile());
      HIP_TRY(h, hipEventRecord(t.ev[1], s));
      if (staged)
        for (const RayOutput *o = outs; o != outsEnd; o++)
          if (o->user) HIP_TRY(h, hipMemcpy2DAsync(o->user + o->size * first, W * o->size, o->dev, ex * o->size, ex * o->size, ey, hipMemcpyDeviceToHost, s));
      HIP_TRY(h, hipStreamSynchronize(s));
      float ms = 0.f;
      HIP_TRY(h, t.elapsed(0, 1, &ms));
      total += ms;
    }
  kernelMs = total;
  return 0;
}

int exa_hip_project(ExaHipRenderer *h, const ExaHipRays *rays, int32_t channel, int32_t flags, double *sum, uint32_t *count,
                    float *vmax, float *vmin, int32_t *maxIndex, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_project";
  ExaHipRenderer *r = firstChild(h);
  r->project.kernelMs = 0.f;
  if (checkRays(h, fn, rays, channel, flags)) return 1;
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  RayArgs a;
  if (rayArgs(h, r, fn, rays, channel, flags, s, a)) return 1;
  // the doubles first, so that every part of the staging buffer {sum | count | vmax | vmin | maxIndex} is aligned
  RayOutput outs[5] = { { reinterpret_cast<char *>(sum), 8, nullptr }, { reinterpret_cast<char *>(count), 4, nullptr },
                        { reinterpret_cast<char *>(vmax), 4, nullptr }, { reinterpret_cast<char *>(vmin), 4, nullptr },
                        { reinterpret_cast<char *>(maxIndex), 4, nullptr } };
  const int rc = rayTiles(h, r, a, outs, 5, pointersAreDevice != 0, s, r->project.kernelMs, [&]() {
    a.sum = reinterpret_cast<double *>(outs[0].dev);
    a.count = reinterpret_cast<uint32_t *>(outs[1].dev);
    a.vmax = reinterpret_cast<float *>(outs[2].dev);
    a.vmin = reinterpret_cast<float *>(outs[3].dev);
    a.maxIndex = reinterpret_cast<int32_t *>(outs[4].dev);
    return EXA_FORM(r, launchSampleRays)(a, r->probes.uniform != 0, s);
  });
  return rc ? rc : checkLoopGuard(h, r, fn, kDescentGuard);
}

int exa_hip_project_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->project.kernelMs;
  return 0;
}

// ---- the field on a triangle mesh (the sampleTriangles* kernels) ----
// The triangles go in chunks of at most kProbeLaunch (with staged parts: at most what kProbeStageBytes hold) through the
// staging buffer {the two list counters, 16 bytes | sum | list | triangles | count | areaNormal | subdiv}: the doubles in
// front, so that every part is aligned to its element.  The list is always there; the triangles only for a host mesh, the
// outputs only for host outputs (the mesh of the handle with host outputs: the one without the other).
int exa_hip_sample_triangles(ExaHipRenderer *h, const float *vertices, uint64_t numVertices, const int32_t *triangles,
                             uint64_t numTriangles, const int32_t *channels, int32_t numChannels, float spacing, int32_t maxN,
                             int32_t flags, double *sum, uint32_t *count, float *areaNormal, int32_t *subdiv,
                             int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_sample_triangles";
  ExaHipRenderer *r = firstChild(h);
  r->surface.kernelMs = 0.f;
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_SURFACE_FROM_ISOSURFACE, " (EXA_SAMPLE_WORLD_SPACE and EXA_SURFACE_FROM_ISOSURFACE apply)")) return 1;
  if (!channels || numChannels < 1 || numChannels > EXA_SURFACE_MAX_CHANNELS) { h->fail(std::string(fn) + ": 1..4 channels required"); return 1; }
  for (int c = 0; c < numChannels; c++)
    if (!checkChannel(h, fn, channels[c])) return 1;
  if (maxN < 1 || maxN > EXA_SURFACE_MAX_N) { h->fail(std::string(fn) + ": maxN must be in 1.." + std::to_string(EXA_SURFACE_MAX_N)); return 1; }
  if (!std::isfinite(spacing) || spacing < 0.f) { h->fail(std::string(fn) + ": the spacing must be finite and >= 0"); return 1; }
  const bool fromIso = (flags & EXA_SURFACE_FROM_ISOSURFACE) != 0;
  if (fromIso) {
    if (vertices || triangles) { h->fail(std::string(fn) + ": vertices and triangles must be NULL with EXA_SURFACE_FROM_ISOSURFACE"); return 1; }
    if (!r->isoMesh.have) { h->fail(std::string(fn) + ": no mesh (exa_hip_isosurface comes first; a release or a failed extraction drops it)"); return 1; }
    vertices = r->isoMesh.vertices.p;
    triangles = r->isoMesh.triangles.p;
    numVertices = r->isoMesh.vertices.n / 3;
    numTriangles = r->isoMesh.triangles.n / 3;
  } else {
    if (numVertices > uint64_t(INT32_MAX) || numTriangles > uint64_t(INT32_MAX)) { h->fail(std::string(fn) + ": more than INT32_MAX vertices or triangles"); return 1; }
    if (numTriangles && (!vertices || !triangles)) { h->fail(std::string(fn) + ": null vertices or triangles (without EXA_SURFACE_FROM_ISOSURFACE)"); return 1; }
  }
  if (numTriangles == 0) return 0;
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  TriArgs a;
  std::memset(&a, 0, sizeof(a));
  if (probeSetup(h, r, fn, (flags & EXA_SAMPLE_WORLD_SPACE) != 0, s, a.s)) return 1;
  a.s.numChannels = numChannels;
  for (int c = 0; c < numChannels; c++) a.s.fieldOffset[c] = r->sc.channelOffset[channels[c]];
  a.spacing = spacing;
  a.maxN = maxN;
  a.pack = r->surface.pack;
  const bool meshDev = fromIso || pointersAreDevice, outDev = pointersAreDevice != 0;
  DevBuf<float> vbuf;                      // a host mesh: its vertices, for the duration of the call
  if (!meshDev) {
    const hipError_t e = vbuf.upload(vertices, 3 * size_t(numVertices));
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the vertices (12 bytes each)", e);
    vertices = vbuf.p;
  }
  a.vertices = vertices;
  a.numVertices = numVertices;
  const uint64_t nch = uint64_t(numChannels);
  const uint64_t perTri = 4 + (meshDev ? 0 : 12) + (outDev ? 0 : (sum ? 8 * nch : 0) + (count ? 4 * nch : 0) + (areaNormal ? 12 : 0) + (subdiv ? 4 : 0));
  const uint64_t chunk = std::max<uint64_t>(1, std::min(kProbeLaunch, (kProbeStageBytes - 16) / perTri));
  const uint64_t need = 16 + std::min(numTriangles, chunk) * perTri;
  if (r->probes.stage.n < need) HIP_TRY(h, r->probes.stage.alloc(need));
  TimingEvents<2> t;
  HIP_TRY(h, t.create());
  float total = 0.f;
  for (uint64_t at = 0; at < numTriangles; at += chunk) {
    const uint64_t m = std::min(chunk, numTriangles - at);
    char *cut = r->probes.stage.p;
    a.numTriangles = uint32_t(m);
    a.listCount = reinterpret_cast<uint32_t *>(carve(cut, true, 16));
    double *dSum = reinterpret_cast<double *>(carve(cut, !outDev && sum, 8 * m * nch));
    a.list = reinterpret_cast<int32_t *>(carve(cut, true, 4 * m));
    int32_t *dTri = reinterpret_cast<int32_t *>(carve(cut, !meshDev, 12 * m));
    uint32_t *dCount = reinterpret_cast<uint32_t *>(carve(cut, !outDev && count, 4 * m * nch));
    float *dNormal = reinterpret_cast<float *>(carve(cut, !outDev && areaNormal, 12 * m));
    int32_t *dSubdiv = reinterpret_cast<int32_t *>(carve(cut, !outDev && subdiv, 4 * m));
    a.triangles = meshDev ? triangles + 3 * at : dTri;
    a.sum = outDev ? (sum ? sum + at * nch : nullptr) : dSum;
    a.count = outDev ? (count ? count + at * nch : nullptr) : dCount;
    a.areaNormal = outDev ? (areaNormal ? areaNormal + 3 * at : nullptr) : dNormal;
    a.subdiv = outDev ? (subdiv ? subdiv + at : nullptr) : dSubdiv;
    if (!meshDev) HIP_TRY(h, hipMemcpyAsync(dTri, triangles + 3 * at, 12 * m, hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipMemsetAsync(a.listCount, 0, 16, s));
    HIP_TRY(h, hipEventRecord(t.ev[0], s));
    HIP_TRY(h, EXA_FORM(r, launchSampleTriangles)(a, r->probes.uniform != 0, s));
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    if (dSum) HIP_TRY(h, hipMemcpyAsync(sum + at * nch, dSum, 8 * m * nch, hipMemcpyDeviceToHost, s));
    if (dCount) HIP_TRY(h, hipMemcpyAsync(count + at * nch, dCount, 4 * m * nch, hipMemcpyDeviceToHost, s));
    if (dNormal) HIP_TRY(h, hipMemcpyAsync(areaNormal + 3 * at, dNormal, 12 * m, hipMemcpyDeviceToHost, s));
    if (dSubdiv) HIP_TRY(h, hipMemcpyAsync(subdiv + at, dSubdiv, 4 * m, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    float ms = 0.f;
    HIP_TRY(h, t.elapsed(0, 1, &ms));
    total += ms;
  }
  r->surface.kernelMs = total;
  return checkLoopGuard(h, r, fn, kDescentGuard);
}

int exa_hip_sample_triangles_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->surface.kernelMs;
  return 0;
}

int exa_hip_raycast_iso(ExaHipRenderer *h, const ExaHipRays *rays, int32_t channel, float iso, int32_t refine, int32_t flags,
                        float fill, float *t, float *position, float *value, float *gradient, int32_t *index, int32_t *side,
                        uint32_t *crossings, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_raycast_iso";
  ExaHipRenderer *r = firstChild(h);
  r->raycast.kernelMs = 0.f;
  if (checkRays(h, fn, rays, channel, flags)) return 1;
  if (!std::isfinite(iso)) { h->fail(std::string(fn) + ": the iso value must be finite"); return 1; }
  if (refine < 0 || refine > EXA_CROSS_MAX_REFINE) { h->fail(std::string(fn) + ": refine must be in 0.." + std::to_string(EXA_CROSS_MAX_REFINE)); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  CrossArgs a;
  std::memset(&a, 0, sizeof(a));
  if (rayArgs(h, r, fn, rays, channel, flags, s, a.r)) return 1;
  a.r.s.fill = fill;
  a.iso = iso;
  a.refine = refine;
  // every element a multiple of 4 bytes: any order leaves the parts of the staging buffer aligned
  RayOutput outs[7] = { { reinterpret_cast<char *>(t), 4, nullptr }, { reinterpret_cast<char *>(position), 12, nullptr },
                        { reinterpret_cast<char *>(value), 4, nullptr }, { reinterpret_cast<char *>(gradient), 12, nullptr },
                        { reinterpret_cast<char *>(index), 4, nullptr }, { reinterpret_cast<char *>(side), 4, nullptr },
                        { reinterpret_cast<char *>(crossings), 4, nullptr } };
  const int rc = rayTiles(h, r, a.r, outs, 7, pointersAreDevice != 0, s, r->raycast.kernelMs, [&]() {
    a.t = reinterpret_cast<float *>(outs[0].dev);
    a.position = reinterpret_cast<float *>(outs[1].dev);
    a.value = reinterpret_cast<float *>(outs[2].dev);
    a.gradient = reinterpret_cast<float *>(outs[3].dev);
    a.index = reinterpret_cast<int32_t *>(outs[4].dev);
    a.side = reinterpret_cast<int32_t *>(outs[5].dev);
    a.crossings = reinterpret_cast<uint32_t *>(outs[6].dev);
    return EXA_FORM(r, launchSampleCrossings)(a, r->probes.uniform != 0, s);
  });
  return rc ? rc : checkLoopGuard(h, r, fn, kDescentGuard);
}

int exa_hip_raycast_iso_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->raycast.kernelMs;
  return 0;
}

} // extern "C"

// ---- what the extractions on a lattice share (exa_isomesh.hip); outside the extern "C" block for the templates ----
// a call of another entry point on behalf of fn failed with rc: its message with fn in front
static int failedIn(ExaHipRenderer *h, const char *fn, int rc)
{
  h->fail(std::string(fn) + ": " + h->err);
  return rc;
}

// The number of points of the lattice `dims`, 0 after h has failed with one of the caller's texts, axis by axis: boxText
// where lo or hi is not finite or, with `ordered`, hi <= lo (nullptr: the box is left to the resampling call), then
// dimsText where the axis has fewer than minDim points
static uint64_t latticePoints(ExaHipRenderer *h, const char *fn, const float lo[3], const float hi[3], const int32_t dims[3],
                              int32_t minDim, const char *dimsText, const char *boxText, bool ordered)
{
  for (int k = 0; k < 3; k++) {
    if (boxText && !(std::isfinite(lo[k]) && std::isfinite(hi[k]) && (!ordered || hi[k] > lo[k]))) { h->fail(std::string(fn) + ": " + boxText); return 0; }
    if (dims[k] < minDim) { h->fail(std::string(fn) + ": " + dimsText); return 0; }
  }
  const uint64_t n = uint64_t(dims[0]) * uint64_t(dims[1]) * uint64_t(dims[2]);     // each < 2^31: no overflow of the first product
  if (uint64_t(dims[0]) * uint64_t(dims[1]) > uint64_t(INT32_MAX) || n > uint64_t(INT32_MAX)) {
    h->fail(std::string(fn) + ": a lattice of more than 2^31 - 1 points");
    return 0;
  }
  return n;
}

// The blocks and chunks of n lattice points and the scans' work space for `counts` block counts, carved out of `work`
// (freed when the call returns; every part aligned to its element): chunkBase | totals | extra64 more 64-bit words |
// blockCount | blockBase | tailBytes more.  The six fields go to two places: `scan` is what launchIsoScans takes, and the
// family's own kernels read the same fields out of their own arguments `a`, whose layout stays as it is.  The extra words
// begin at scan.totals + counts, the tail at scan.blockBase + counts * scan.numBlocks.
template <typename A>
static hipError_t allocScans(DevBuf<char> &work, uint64_t n, int counts, size_t extra64, size_t tailBytes, A &a, IsoScanArgs &scan)
{
  scan.numBlocks = uint32_t((n + kIsoBlock - 1) / kIsoBlock);
  scan.numChunks = (scan.numBlocks + kIsoChunk - 1) / kIsoChunk;
  const size_t n64 = size_t(counts) * (size_t(scan.numChunks) + 1) + extra64, n32 = 2 * size_t(counts) * scan.numBlocks;
  const hipError_t e = work.alloc(n64 * 8 + n32 * 4 + tailBytes);
  if (e != hipSuccess) return e;
  scan.chunkBase = reinterpret_cast<uint64_t *>(work.p);
  scan.totals = scan.chunkBase + size_t(counts) * scan.numChunks;
  scan.blockCount = reinterpret_cast<uint32_t *>(work.p + n64 * 8);
  scan.blockBase = scan.blockCount + size_t(counts) * scan.numBlocks;
  a.numBlocks = scan.numBlocks; a.numChunks = scan.numChunks;
  a.blockCount = scan.blockCount; a.blockBase = scan.blockBase; a.chunkBase = scan.chunkBase; a.totals = scan.totals;
  return hipSuccess;
}

// The lattice: exa_hip_resample of channels[0] or (quantity >= 0) exa_hip_resample_derived of channels[0..2], with a NaN
// fill into the device buffer (its checks of the box, the channels, the quantity, the kd tree and the frame state apply;
// synchronous, with the descent's loop guard checked)
static int fillLattice(ExaHipRenderer *h, const char *fn, const float lo[3], const float hi[3], const int32_t dims[3],
                       const int32_t *channels, int32_t quantity, int32_t worldFlag, float *values, void *hipStream)
{
  const int rc = quantity < 0 ? exa_hip_resample(h, lo, hi, dims, channels[0], worldFlag, NAN, values, 1, hipStream, 0)
                              : exa_hip_resample_derived(h, lo, hi, dims, channels, quantity, worldFlag, NAN, values, 1, hipStream, 0);
  return rc ? failedIn(h, fn, rc) : 0;
}

// a small read-back that steers the call: the stream is idle behind it
static int readBack(ExaHipRenderer *h, void *dst, const void *src, size_t bytes, hipStream_t s)
{
  HIP_TRY(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return 0;
}

// the exponent of the fixed-point sums of the regions and basins out of their totals: .., inside points, bits of max |V|
static int32_t sumExponentOf(const uint64_t totals[3])
{
  const uint32_t maxBits = uint32_t(totals[2]);
  float maxAbs;
  std::memcpy(&maxAbs, &maxBits, sizeof(maxAbs));
  if (!totals[1] || maxAbs == 0.f) return 0;
  int ex = 0;
  (void)std::frexp(maxAbs, &ex);
  return 30 - ex;
}

// What regionsExtract and basinsExtract do alike in front of their passes (A: IsoRegionArgs or IsoBasinArgs): the common
// fields of the kernels' arguments, the result's values and labels, and the scans' work space with extra64 words behind
// the three totals ...
template <typename A, typename R>
static int labelledSetup(ExaHipRenderer *h, const char *fn, const int32_t dims[3], float iso, int32_t flags, size_t extra64,
                         LabelledLattice<R> &res, DevBuf<char> &work, A &a, IsoScanArgs &scan)
{
  const size_t n = size_t(dims[0]) * size_t(dims[1]) * size_t(dims[2]);       // checked by the caller (latticePoints)
  std::memset(&a, 0, sizeof(a));
  a.numPoints = uint32_t(n);
  a.nx = uint32_t(dims[0]); a.ny = uint32_t(dims[1]); a.nz = uint32_t(dims[2]);
  a.iso = iso;
  a.below = (flags & EXA_REGIONS_BELOW) ? 1 : 0;
  a.faces = (flags & EXA_REGIONS_FACES) ? 1 : 0;
  a.errorFlag = firstChild(h)->errorFlag.p;
  hipError_t e = res.values.alloc(n);
  if (e == hipSuccess) e = res.labels.alloc(n);
  if (e == hipSuccess) e = allocScans(work, n, 1, 2 + extra64, 0, a, scan);
  if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the lattice (4 bytes per point) and the labels (4 more)", e);
  a.values = res.values.p;
  return 0;
}

// ... and behind them: the values kept or dropped, the result committed, the out-parameters that both have
template <typename R>
static void labelledCommit(LabelledLattice<R> &res, DropUnlessCommitted<LabelledLattice<R>> &guard, int32_t flags,
                           const uint64_t totals[3], int32_t exponent, uint64_t *numInside, int32_t *sumExponent)
{
  res.keptValues = (flags & EXA_REGIONS_KEEP_VALUES) != 0;
  if (!res.keptValues) res.values.release();
  res.have = true;
  guard.commit();
  if (numInside) *numInside = totals[1];
  if (sumExponent) *sumExponent = exponent;
}

// exa_hip_regions_read and exa_hip_basins_read, each with its own two texts
template <typename R>
static int labelledRead(ExaHipRenderer *h, const char *fn, LabelledLattice<R> ExaHipRenderer::*which, const char *noneText,
                        const char *noValuesText, int32_t *labels, R *table, float *values, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  ExaHipRenderer *r = firstChild(h);
  const LabelledLattice<R> &res = r->*which;
  if (!res.have) { h->fail(std::string(fn) + ": " + noneText); return 1; }
  if (values && !res.keptValues) { h->fail(std::string(fn) + ": " + noValuesText); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  const hipMemcpyKind kind = pointersAreDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(h, copyOut(labels, res.labels, kind, s));
  HIP_TRY(h, copyOut(table, res.table, kind, s));
  HIP_TRY(h, copyOut(values, res.values, kind, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return 0;
}

extern "C" {

// ---- iso-surface extraction (exa_isomesh.hip) ----
// exa_hip_isosurface (quantity < 0: the lattice holds the one channel channels[0]) and exa_hip_isosurface_derived (it holds
// the quantity of channels[0..2]; no gradients: the caller has refused the flag).  Filling the lattice is the one step in
// which they differ; every later stage only ever looks at lattice values.  The flags are checked by the caller.
static int isoExtract(ExaHipRenderer *h, const char *fn, const float lo[3], const float hi[3], const int32_t dims[3],
                      const int32_t *channels, int32_t quantity, float iso, int32_t flags, uint64_t *numVertices,
                      uint64_t *numTriangles, void *hipStream)
{
  if (!lo || !hi || !dims) { h->fail(std::string(fn) + ": null argument"); return 1; }
  if (!std::isfinite(iso)) { h->fail(std::string(fn) + ": the iso value must be finite"); return 1; }
  const uint64_t n = latticePoints(h, fn, lo, hi, dims, 2, "dims must be >= 2 on every axis (a lattice of cubes)", nullptr, false);
  if (!n) return 1;
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  r->isoMesh.release();
  DropUnlessCommitted<ExaHipRenderer::IsoMesh> mesh(r->isoMesh);     // whatever fails from here on leaves no mesh
  for (float &ms : r->isoMesh.stageMs) ms = 0.f;
  const bool world = (flags & EXA_SAMPLE_WORLD_SPACE) != 0, grad = (flags & EXA_SAMPLE_GRADIENT) != 0;

  IsoMeshArgs a;
  std::memset(&a, 0, sizeof(a));
  a.numPoints = uint32_t(n);
  a.nx = uint32_t(dims[0]); a.ny = uint32_t(dims[1]); a.nz = uint32_t(dims[2]);
  a.iso = iso;
  for (int k = 0; k < 3; k++) { a.lo[k] = lo[k]; a.step[k] = (hi[k] - lo[k]) / float(dims[k]); }
  // the work space of one extraction: the scans' for the two counts (vertices, triangles) | rel | cubeInfo, mask
  DevBuf<float> values;
  DevBuf<char> work;
  IsoScanArgs scan;
  const size_t n16 = n + (n & 1);
  hipError_t e = values.alloc(n);
  if (e == hipSuccess) e = allocScans(work, n, 2, 0, n16 * 2 + 2 * n, a, scan);
  if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the lattice (4 bytes per point) and the work space (4 more)", e);
  a.values = values.p;
  a.rel = reinterpret_cast<uint16_t *>(scan.blockBase + 2 * size_t(scan.numBlocks));
  a.cubeInfo = reinterpret_cast<uint8_t *>(a.rel + n16);
  a.mask = a.cubeInfo + n;

  TimingEvents<7> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  if (int rc = fillLattice(h, fn, lo, hi, dims, channels, quantity, world ? EXA_SAMPLE_WORLD_SPACE : 0, values.p, hipStream)) return rc;
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  HIP_TRY(h, launchIsoCubePass(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[2], s));
  HIP_TRY(h, launchIsoPointPass(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[3], s));
  HIP_TRY(h, launchIsoScans(scan, 2, s));
  HIP_TRY(h, hipEventRecord(t.ev[4], s));
  uint64_t totals[2] = { 0, 0 };                 // vertices, triangles
  if (readBack(h, totals, a.totals, sizeof(totals), s)) return 1;
  if (totals[0] > uint64_t(INT32_MAX) || totals[1] > uint64_t(INT32_MAX)) {
    h->fail(std::string(fn) + ": the surface has " + std::to_string(totals[0]) + " vertices and " + std::to_string(totals[1]) +
            " triangles: more than INT32_MAX, the indices are int32 (extract it in parts)");
    return 1;
  }
  if (totals[0] && totals[1]) {
    e = r->isoMesh.vertices.alloc(3 * size_t(totals[0]));
    if (e == hipSuccess) e = r->isoMesh.triangles.alloc(3 * size_t(totals[1]));
    if (e == hipSuccess && grad) e = r->isoMesh.gradients.alloc(3 * size_t(totals[0]));
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the mesh", e);
    a.vertices = r->isoMesh.vertices.p;
    a.triangles = r->isoMesh.triangles.p;
    HIP_TRY(h, launchIsoEmit(a, s));
  }
  HIP_TRY(h, hipEventRecord(t.ev[5], s));
  if (grad && totals[0]) {
    // the existing points kernel on the device vertex buffer; its values go into the lattice buffer, which is done with
    // (a vertex sits on an edge between two lattice points: fewer than 7 per point, but the buffer holds only n floats)
    DevBuf<float> scratch;
    float *vals = values.p;
    if (totals[0] > n) {
      e = scratch.alloc(size_t(totals[0]));
      if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the gradients", e);
      vals = scratch.p;
    }
    const int32_t pf = (world ? EXA_SAMPLE_WORLD_SPACE : 0) | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED;
    if (int rc = exa_hip_sample_points(h, r->isoMesh.vertices.p, totals[0], channels, 1, pf, NAN, vals, r->isoMesh.gradients.p, nullptr, 1, hipStream, 0))
      return failedIn(h, fn, rc);
  }
  HIP_TRY(h, hipEventRecord(t.ev[6], s));
  HIP_TRY(h, hipStreamSynchronize(s));
  for (int k = 0; k < 6; k++) HIP_TRY(h, t.elapsed(k, k + 1, &r->isoMesh.stageMs[k]));
  r->isoMesh.have = true;
  mesh.commit();
  if (numVertices) *numVertices = totals[0];
  if (numTriangles) *numTriangles = totals[1];
  return 0;
}

int exa_hip_isosurface(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel, float iso,
                       int32_t flags, uint64_t *numVertices, uint64_t *numTriangles, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_isosurface";
  if (numVertices) *numVertices = 0;
  if (numTriangles) *numTriangles = 0;
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_SAMPLE_GRADIENT, " (EXA_SAMPLE_WORLD_SPACE and EXA_SAMPLE_GRADIENT apply)")) return 1;
  return isoExtract(h, fn, lo, hi, dims, &channel, -1, iso, flags, numVertices, numTriangles, hipStream);
}

int exa_hip_isosurface_derived(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t channels[3],
                               int32_t quantity, float iso, int32_t flags, uint64_t *numVertices, uint64_t *numTriangles,
                               void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_isosurface_derived";
  if (numVertices) *numVertices = 0;
  if (numTriangles) *numTriangles = 0;
  if (flags & EXA_SAMPLE_GRADIENT) {
    h->fail(std::string(fn) + ": EXA_SAMPLE_GRADIENT does not apply (a normal of a derived surface would need second derivatives)");
    return 1;
  }
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE, " (only EXA_SAMPLE_WORLD_SPACE applies)")) return 1;
  if (!oneComponent(h, fn, channels, quantity, "a surface needs")) return 1;
  return isoExtract(h, fn, lo, hi, dims, channels, quantity, iso, flags, numVertices, numTriangles, hipStream);
}

int exa_hip_isosurface_read(ExaHipRenderer *h, float *vertices, float *gradients, int32_t *triangles, int32_t pointersAreDevice,
                            void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_isosurface_read";
  ExaHipRenderer *r = firstChild(h);
  const ExaHipRenderer::IsoMesh &res = r->isoMesh;
  if (!res.have) { h->fail(std::string(fn) + ": no mesh (exa_hip_isosurface comes first; a release or a failed extraction drops it)"); return 1; }
  if (gradients && res.vertices.n && !res.gradients.n) { h->fail(std::string(fn) + ": the mesh was extracted without EXA_SAMPLE_GRADIENT"); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  const hipMemcpyKind kind = pointersAreDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(h, copyOut(vertices, res.vertices, kind, s));
  HIP_TRY(h, copyOut(gradients, res.gradients, kind, s));
  HIP_TRY(h, copyOut(triangles, res.triangles, kind, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return 0;
}

int exa_hip_isosurface_release(ExaHipRenderer *h) { return releaseResult(h, &ExaHipRenderer::isoMesh); }
int exa_hip_isosurface_stage_ms(ExaHipRenderer *h, float ms[6]) { return readStageMs(h, &ExaHipRenderer::isoMesh, ms); }

// ---- contour lines on a plane lattice (exa_isomesh.hip) ----
// exa_hip_isolines (quantity < 0: the lattice holds the one channel channels[0]) and exa_hip_isolines_derived (it holds the
// quantity of channels[0..2]; no gradients: the caller has refused the flag).  The levels share the lattice values and the
// work space of one level: a first round counts every level (square pass, point pass, scans), the packed arrays are
// allocated for the sum, and a second round repeats the passes level by level and emits at the level's offsets — from the
// last level to the first, so that the last one, whose passes the work space still holds, is not repeated.  The flags, the
// channels and the quantity are checked by the caller.
static int isolinesExtract(ExaHipRenderer *h, const char *fn, const ExaHipPlane *plane, const int32_t *channels, int32_t quantity,
                           const float *isos, int32_t numIsos, int32_t flags, uint64_t *numVertices, uint64_t *numSegments,
                           void *hipStream)
{
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  r->isolines.release();
  DropUnlessCommitted<ExaHipRenderer::Isolines> lines(r->isolines);     // whatever fails from here on leaves no result
  ExaHipRenderer::Isolines &res = r->isolines;
  for (float &ms : res.stageMs) ms = 0.f;
  if (!plane || !isos) { h->fail(std::string(fn) + ": null argument (the plane or the levels)"); return 1; }
  for (int k = 0; k < 3; k++)
    if (!(std::isfinite(plane->origin[k]) && std::isfinite(plane->du[k]) && std::isfinite(plane->dv[k]))) {
      h->fail(std::string(fn) + ": the plane's origin, du and dv must be finite");
      return 1;
    }
  if (plane->nu < 2 || plane->nv < 2) { h->fail(std::string(fn) + ": nu and nv must be >= 2 (a lattice of squares)"); return 1; }
  const uint64_t n = uint64_t(plane->nu) * uint64_t(plane->nv);
  if (n > uint64_t(INT32_MAX)) { h->fail(std::string(fn) + ": a lattice of more than 2^31 - 1 points"); return 1; }
  if (numIsos < 1 || numIsos > EXA_ISOLINES_MAX_LEVELS) { h->fail(std::string(fn) + ": 1..256 levels required (EXA_ISOLINES_MAX_LEVELS)"); return 1; }
  for (int32_t l = 0; l < numIsos; l++)
    if (!std::isfinite(isos[l])) { h->fail(std::string(fn) + ": every level must be finite"); return 1; }
  hipStream_t s = (hipStream_t)hipStream;
  const bool world = (flags & EXA_SAMPLE_WORLD_SPACE) != 0, grad = (flags & EXA_SAMPLE_GRADIENT) != 0;
  const int32_t wf = world ? EXA_SAMPLE_WORLD_SPACE : 0;

  IsoLineArgs a;
  std::memset(&a, 0, sizeof(a));
  a.numPoints = uint32_t(n);
  a.nu = uint32_t(plane->nu); a.nv = uint32_t(plane->nv);
  for (int k = 0; k < 3; k++) { a.origin[k] = plane->origin[k]; a.du[k] = plane->du[k]; a.dv[k] = plane->dv[k]; }
  a.numBlocks = uint32_t((n + kIsoBlock - 1) / kIsoBlock);      // for the positions; once more with the work space

  TimingEvents<5> t;
  HIP_TRY(h, t.create());
  float ms = 0.f;
  // the values: the positions into a device buffer, then exa_hip_sample_points, or exa_hip_sample_derived, with a NaN fill
  // on it (their checks of the kd tree and the frame state apply; synchronous, with the loop guard's check).  The positions
  // are freed before the work space is allocated.
  hipError_t e = res.values.alloc(n);
  {
    DevBuf<float> positions;
    if (e == hipSuccess) e = positions.alloc(3 * size_t(n));
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the lattice (4 bytes per point) and its positions (12 more)", e);
    a.positions = positions.p;
    HIP_TRY(h, hipEventRecord(t.ev[0], s));
    HIP_TRY(h, launchIsolinePositions(a, s));
    if (int rc = quantity < 0 ? exa_hip_sample_points(h, positions.p, n, channels, 1, wf, NAN, res.values.p, nullptr, nullptr, 1, hipStream, 0)
                              : exa_hip_sample_derived(h, positions.p, n, channels, quantity, wf, NAN, res.values.p, nullptr, 1, hipStream, 0))
      return failedIn(h, fn, rc);
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, t.elapsed(0, 1, &res.stageMs[0]));
    a.positions = nullptr;
  }
  a.values = res.values.p;
  // the work space of one level: the scans' for the two counts (vertices, segments) | rel | squareInfo, mask
  DevBuf<char> work;
  IsoScanArgs scan;
  const size_t n16 = n + (n & 1);
  e = allocScans(work, n, 2, 0, n16 * 2 + 2 * n, a, scan);
  if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the work space (4 bytes per lattice point)", e);
  a.rel = reinterpret_cast<uint16_t *>(scan.blockBase + 2 * size_t(scan.numBlocks));
  a.squareInfo = reinterpret_cast<uint8_t *>(a.rel + n16);
  a.mask = a.squareInfo + n;

  // square pass, point pass and scans of the level a.iso, timed into stages 1..3; the level's totals {vertices, segments}
  auto countLevel = [&](uint64_t totals[2]) -> int {
    HIP_TRY(h, hipEventRecord(t.ev[0], s));
    HIP_TRY(h, launchIsolineSquarePass(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    HIP_TRY(h, launchIsolinePointPass(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[2], s));
    HIP_TRY(h, launchIsoScans(scan, 2, s));
    HIP_TRY(h, hipEventRecord(t.ev[3], s));
    if (readBack(h, totals, a.totals, 2 * sizeof(uint64_t), s)) return 1;
    for (int k = 0; k < 3; k++) { HIP_TRY(h, t.elapsed(k, k + 1, &ms)); res.stageMs[1 + k] += ms; }
    return 0;
  };
  res.vertexOffsets.assign(size_t(numIsos) + 1, 0);
  res.segmentOffsets.assign(size_t(numIsos) + 1, 0);
  for (int32_t l = 0; l < numIsos; l++) {
    uint64_t totals[2] = { 0, 0 };
    a.iso = isos[l];
    if (countLevel(totals)) return 1;
    res.vertexOffsets[l + 1] = res.vertexOffsets[l] + totals[0];
    res.segmentOffsets[l + 1] = res.segmentOffsets[l] + totals[1];
    if (res.vertexOffsets[l + 1] > uint64_t(INT32_MAX) || res.segmentOffsets[l + 1] > uint64_t(INT32_MAX)) {
      h->fail(std::string(fn) + ": more than INT32_MAX vertices or segments at level " + std::to_string(l) +
              ", the indices are int32 (extract the levels in parts)");
      return 1;
    }
  }
  const uint64_t nv = res.vertexOffsets[numIsos], ns = res.segmentOffsets[numIsos];
  if (nv && ns) {
    e = res.vertices.alloc(3 * size_t(nv));
    if (e == hipSuccess) e = res.uv.alloc(2 * size_t(nv));
    if (e == hipSuccess) e = res.segments.alloc(2 * size_t(ns));
    if (e == hipSuccess && grad) e = res.gradients.alloc(3 * size_t(nv));
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the lines", e);
    for (int32_t l = numIsos - 1; l >= 0; l--) {
      if (res.vertexOffsets[l + 1] == res.vertexOffsets[l]) continue;          // no vertices: no segments either
      a.iso = isos[l];
      uint64_t totals[2] = { 0, 0 };
      if (l != numIsos - 1 && countLevel(totals)) return 1;
      a.vertexBase = uint32_t(res.vertexOffsets[l]);
      a.vertices = res.vertices.p + 3 * size_t(res.vertexOffsets[l]);
      a.uv = res.uv.p + 2 * size_t(res.vertexOffsets[l]);
      a.segments = res.segments.p + 2 * size_t(res.segmentOffsets[l]);
      HIP_TRY(h, hipEventRecord(t.ev[3], s));
      HIP_TRY(h, launchIsolineEmit(a, s));
      HIP_TRY(h, hipEventRecord(t.ev[4], s));
      HIP_TRY(h, hipStreamSynchronize(s));
      HIP_TRY(h, t.elapsed(3, 4, &ms));
      res.stageMs[4] += ms;
    }
  }
  if (grad && nv) {
    // the existing points kernel on the device vertex buffer; its values go into the lattice buffer where that is done
    // with and large enough (a lattice point owns up to three vertices per level)
    DevBuf<float> scratch;
    float *vals = res.values.p;
    if (nv > n || (flags & EXA_ISOLINES_KEEP_VALUES)) {
      e = scratch.alloc(size_t(nv));
      if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the gradients", e);
      vals = scratch.p;
    }
    HIP_TRY(h, hipEventRecord(t.ev[0], s));
    const int32_t pf = wf | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED;
    if (int rc = exa_hip_sample_points(h, res.vertices.p, nv, channels, 1, pf, NAN, vals, res.gradients.p, nullptr, 1, hipStream, 0))
      return failedIn(h, fn, rc);
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, t.elapsed(0, 1, &res.stageMs[5]));
  }
  res.keptValues = (flags & EXA_ISOLINES_KEEP_VALUES) != 0;
  if (!res.keptValues) res.values.release();
  res.withGradients = grad;
  res.have = true;
  lines.commit();
  if (numVertices) *numVertices = nv;
  if (numSegments) *numSegments = ns;
  return 0;
}

int exa_hip_isolines(ExaHipRenderer *h, const ExaHipPlane *plane, int32_t channel, const float *isos, int32_t numIsos, int32_t flags,
                     uint64_t *numVertices, uint64_t *numSegments, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_isolines";
  if (numVertices) *numVertices = 0;
  if (numSegments) *numSegments = 0;
  int rc = 1;
  if (checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_SAMPLE_GRADIENT | EXA_ISOLINES_KEEP_VALUES,
                 " (EXA_SAMPLE_WORLD_SPACE, EXA_SAMPLE_GRADIENT and EXA_ISOLINES_KEEP_VALUES apply)") &&
      checkChannel(h, fn, channel))
    rc = isolinesExtract(h, fn, plane, &channel, -1, isos, numIsos, flags, numVertices, numSegments, hipStream);
  if (rc) (void)exa_hip_isolines_release(h);            // a failed extraction leaves no result, whichever check refused it
  return rc;
}

int exa_hip_isolines_derived(ExaHipRenderer *h, const ExaHipPlane *plane, const int32_t channels[3], int32_t quantity,
                             const float *isos, int32_t numIsos, int32_t flags, uint64_t *numVertices, uint64_t *numSegments,
                             void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_isolines_derived";
  if (numVertices) *numVertices = 0;
  if (numSegments) *numSegments = 0;
  int rc = 1;
  if (flags & EXA_SAMPLE_GRADIENT)
    h->fail(std::string(fn) + ": EXA_SAMPLE_GRADIENT does not apply (a gradient of a derived quantity would need second derivatives)");
  else if (checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_ISOLINES_KEEP_VALUES,
                      " (EXA_SAMPLE_WORLD_SPACE and EXA_ISOLINES_KEEP_VALUES apply)") &&
           oneComponent(h, fn, channels, quantity, "contour lines need"))
    rc = isolinesExtract(h, fn, plane, channels, quantity, isos, numIsos, flags, numVertices, numSegments, hipStream);
  if (rc) (void)exa_hip_isolines_release(h);
  return rc;
}

int exa_hip_isolines_read(ExaHipRenderer *h, float *vertices, float *uv, float *gradients, int32_t *segments, uint64_t *vertexOffsets,
                          uint64_t *segmentOffsets, float *values, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_isolines_read";
  ExaHipRenderer *r = firstChild(h);
  const ExaHipRenderer::Isolines &res = r->isolines;
  if (!res.have) { h->fail(std::string(fn) + ": no lines (exa_hip_isolines comes first; a release or a failed extraction drops them)"); return 1; }
  if (gradients && !res.withGradients) { h->fail(std::string(fn) + ": the lines were extracted without EXA_SAMPLE_GRADIENT"); return 1; }
  if (values && !res.keptValues) { h->fail(std::string(fn) + ": the lines were extracted without EXA_ISOLINES_KEEP_VALUES"); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  const hipMemcpyKind kind = pointersAreDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(h, copyOut(vertices, res.vertices, kind, s));
  HIP_TRY(h, copyOut(uv, res.uv, kind, s));
  HIP_TRY(h, copyOut(gradients, res.gradients, kind, s));
  HIP_TRY(h, copyOut(segments, res.segments, kind, s));
  HIP_TRY(h, copyOut(values, res.values, kind, s));
  // the offsets live on the host
  const size_t offBytes = res.vertexOffsets.size() * sizeof(uint64_t);
  if (pointersAreDevice) {
    if (vertexOffsets) HIP_TRY(h, hipMemcpyAsync(vertexOffsets, res.vertexOffsets.data(), offBytes, hipMemcpyHostToDevice, s));
    if (segmentOffsets) HIP_TRY(h, hipMemcpyAsync(segmentOffsets, res.segmentOffsets.data(), offBytes, hipMemcpyHostToDevice, s));
  } else {
    if (vertexOffsets) std::memcpy(vertexOffsets, res.vertexOffsets.data(), offBytes);
    if (segmentOffsets) std::memcpy(segmentOffsets, res.segmentOffsets.data(), offBytes);
  }
  HIP_TRY(h, hipStreamSynchronize(s));
  return 0;
}

int exa_hip_isolines_release(ExaHipRenderer *h) { return releaseResult(h, &ExaHipRenderer::isolines); }
int exa_hip_isolines_stage_ms(ExaHipRenderer *h, float ms[6]) { return readStageMs(h, &ExaHipRenderer::isolines, ms); }

// ---- connected regions of the inside set on a lattice (exa_isomesh.hip) ----
const char *const kRegionGuard = ": the union-find's loop guard tripped (a parent link that does not descend)";

// exa_hip_regions (quantity < 0: the lattice holds the one channel channels[0]) and exa_hip_regions_derived (it holds the
// quantity of channels[0..2]).  The flags, the channels and the quantity are checked by the caller.  The labels array of the
// result is the union-find's forest until the stats pass; two small read-backs: the counts (regions, inside points, max
// |V|) behind the scans, which size the table and give the sum's exponent, and the loop guard at the end.
static int regionsExtract(ExaHipRenderer *h, const char *fn, const float lo[3], const float hi[3], const int32_t dims[3],
                          const int32_t *channels, int32_t quantity, float iso, int32_t flags, uint64_t *numRegions,
                          uint64_t *numInside, int32_t *sumExponent, void *hipStream)
{
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  LabelledLattice<ExaHipRegion> &res = r->isoRegions;
  res.release();
  DropUnlessCommitted<LabelledLattice<ExaHipRegion>> regions(res);     // whatever fails from here on leaves no result
  for (float &ms : res.stageMs) ms = 0.f;
  if (!lo || !hi || !dims) { h->fail(std::string(fn) + ": null argument (lo, hi or dims)"); return 1; }
  if (!std::isfinite(iso)) { h->fail(std::string(fn) + ": the iso value must be finite"); return 1; }
  const uint64_t n = latticePoints(h, fn, lo, hi, dims, 1, "dims must be >= 1 on every axis", "the box must be finite", false);
  if (!n) return 1;
  hipStream_t s = (hipStream_t)hipStream;

  // the work space: the scans' with totals[3]; and the keys further down
  IsoRegionArgs a;
  DevBuf<char> work;
  IsoScanArgs scan;
  if (labelledSetup(h, fn, dims, iso, flags, 0, res, work, a, scan)) return 1;
  a.parent = reinterpret_cast<uint32_t *>(res.labels.p);

  TimingEvents<9> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  if (int rc = fillLattice(h, fn, lo, hi, dims, channels, quantity, flags & EXA_SAMPLE_WORLD_SPACE, res.values.p, hipStream)) return rc;
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  HIP_TRY(h, hipMemsetAsync(a.totals, 0, 3 * sizeof(uint64_t), s));
  HIP_TRY(h, launchIsoRegionInit(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[2], s));
  HIP_TRY(h, launchIsoRegionMerge(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[3], s));
  HIP_TRY(h, launchIsoRegionFlatten(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[4], s));
  HIP_TRY(h, launchIsoScans(scan, 1, s));
  HIP_TRY(h, hipEventRecord(t.ev[5], s));
  uint64_t totals[3] = { 0, 0, 0 };              // regions, inside points, bits of max |V|
  if (readBack(h, totals, a.totals, sizeof(totals), s)) return 1;
  const int32_t exponent = sumExponentOf(totals);
  a.scale = std::ldexp(1.0, exponent);
  a.numRegions = uint32_t(totals[0]);            // <= n
  float rankMs = 0.f;
  if (totals[0]) {
    DevBuf<uint64_t> keys;
    hipError_t e = res.table.alloc(size_t(totals[0]));
    if (e == hipSuccess) e = keys.alloc(2 * size_t(totals[0]));
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the table of regions (88 bytes each, and 16 while the call runs)", e);
    a.regions = res.table.p;
    a.keys = keys.p;
    HIP_TRY(h, hipEventRecord(t.ev[6], s));
    HIP_TRY(h, launchIsoRegionRank(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[7], s));
    HIP_TRY(h, launchIsoRegionStats(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[8], s));
    HIP_TRY(h, hipStreamSynchronize(s));         // the keys are freed behind it
    HIP_TRY(h, t.elapsed(6, 7, &rankMs));
    HIP_TRY(h, t.elapsed(7, 8, &res.stageMs[5]));
  }                                              // no region: every label is the outside mark, which is -1
  for (int k = 0; k < 5; k++) HIP_TRY(h, t.elapsed(k, k + 1, &res.stageMs[k]));
  res.stageMs[4] += rankMs;
  if (int rc = checkLoopGuard(h, r, fn, kRegionGuard)) return rc;
  labelledCommit(res, regions, flags, totals, exponent, numInside, sumExponent);
  if (numRegions) *numRegions = totals[0];
  return 0;
}

static const int32_t kRegionFlags = EXA_SAMPLE_WORLD_SPACE | EXA_REGIONS_KEEP_VALUES | EXA_REGIONS_BELOW | EXA_REGIONS_FACES;
static const char *const kRegionFlagsHint = " (EXA_SAMPLE_WORLD_SPACE, EXA_REGIONS_KEEP_VALUES, EXA_REGIONS_BELOW and EXA_REGIONS_FACES apply)";

int exa_hip_regions(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel, float iso,
                    int32_t flags, uint64_t *numRegions, uint64_t *numInside, int32_t *sumExponent, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_regions";
  if (numRegions) *numRegions = 0;
  if (numInside) *numInside = 0;
  if (sumExponent) *sumExponent = 0;
  int rc = 1;
  if (checkFlags(h, fn, flags, kRegionFlags, kRegionFlagsHint) && checkChannel(h, fn, channel))
    rc = regionsExtract(h, fn, lo, hi, dims, &channel, -1, iso, flags, numRegions, numInside, sumExponent, hipStream);
  if (rc) (void)exa_hip_regions_release(h);            // a failed call leaves no result, whichever check refused it
  return rc;
}

int exa_hip_regions_derived(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t channels[3],
                            int32_t quantity, float iso, int32_t flags, uint64_t *numRegions, uint64_t *numInside,
                            int32_t *sumExponent, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_regions_derived";
  if (numRegions) *numRegions = 0;
  if (numInside) *numInside = 0;
  if (sumExponent) *sumExponent = 0;
  int rc = 1;
  if (checkFlags(h, fn, flags, kRegionFlags, kRegionFlagsHint) && oneComponent(h, fn, channels, quantity, "regions need"))
    rc = regionsExtract(h, fn, lo, hi, dims, channels, quantity, iso, flags, numRegions, numInside, sumExponent, hipStream);
  if (rc) (void)exa_hip_regions_release(h);
  return rc;
}

int exa_hip_regions_read(ExaHipRenderer *h, int32_t *labels, ExaHipRegion *regions, float *values, int32_t pointersAreDevice,
                         void *hipStream)
{
  return labelledRead(h, "exa_hip_regions_read", &ExaHipRenderer::isoRegions,
                      "no regions (exa_hip_regions comes first; a release or a failed call drops them)",
                      "the regions were extracted without EXA_REGIONS_KEEP_VALUES", labels, regions, values, pointersAreDevice, hipStream);
}

int exa_hip_regions_release(ExaHipRenderer *h) { return releaseResult(h, &ExaHipRenderer::isoRegions); }
int exa_hip_regions_stage_ms(ExaHipRenderer *h, float ms[6]) { return readStageMs(h, &ExaHipRenderer::isoRegions, ms); }

// ---- basins of the inside set on a lattice: one per peak, shallow ones merged in rounds (exa_isomesh.hip) ----
const char *const kBasinGuard = ": a loop guard of the basins tripped (a chain of links longer than the lattice, or more rounds than raw basins)";

// exa_hip_basins (quantity < 0: the lattice holds the one channel channels[0]) and exa_hip_basins_derived.  The flags, the
// channels and the quantity are checked by the caller.  The labels array of the result holds the up links, then the
// components, until the stats pass.  Small read-backs steer the call: 4 bytes per pass of pointer doubling and per round
// (the links it made), the counts behind the two numberings (peaks, then components), the loop guard at the end.
static int basinsExtract(ExaHipRenderer *h, const char *fn, const float lo[3], const float hi[3], const int32_t dims[3],
                         const int32_t *channels, int32_t quantity, float iso, float minDepth, int32_t flags, uint64_t *numBasins,
                         uint64_t *numRawBasins, uint64_t *numInside, int32_t *sumExponent, int32_t *rounds, void *hipStream)
{
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  LabelledLattice<ExaHipBasin> &res = r->isoBasins;
  res.release();
  DropUnlessCommitted<LabelledLattice<ExaHipBasin>> basins(res);       // whatever fails from here on leaves no result
  for (float &ms : res.stageMs) ms = 0.f;
  if (!lo || !hi || !dims) { h->fail(std::string(fn) + ": null argument (lo, hi or dims)"); return 1; }
  if (!std::isfinite(iso)) { h->fail(std::string(fn) + ": the iso value must be finite"); return 1; }
  if (!(minDepth >= 0.f)) { h->fail(std::string(fn) + ": minDepth must be >= 0 (+INFINITY is allowed, NaN is not)"); return 1; }
  const uint64_t n = latticePoints(h, fn, lo, hi, dims, 1, "dims must be >= 1 on every axis", "the box must be finite", false);
  if (!n) return 1;
  hipStream_t s = (hipStream_t)hipStream;

  // the work space: the scans' with totals[3] and the jump count; the raw basins' arrays and the keys further down
  IsoBasinArgs a;
  DevBuf<char> work;
  IsoScanArgs scan;
  if (labelledSetup(h, fn, dims, iso, flags, 1, res, work, a, scan)) return 1;
  a.minDepth = minDepth;
  a.comp = reinterpret_cast<uint32_t *>(res.labels.p);
  a.jumpCount = reinterpret_cast<uint32_t *>(a.totals + 3);

  TimingEvents<3> t;
  HIP_TRY(h, t.create());
  // what lies between two events, added to a stage; the stream is idle behind it
  auto lap = [&](int from, int stage) -> int {
    float ms = 0.f;
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, t.elapsed(from, from + 1, &ms));
    res.stageMs[stage] += ms;
    return 0;
  };
  // pointer doubling over array[0, size) to its end: a chain shrinks to a fifth per pass, so 2^31 links need 14 passes
  auto resolve = [&](uint32_t *array, uint32_t size) -> int {
    for (int pass = 0;; pass++) {
      uint32_t left = 0;
      HIP_TRY(h, hipMemsetAsync(a.jumpCount, 0, sizeof(uint32_t), s));
      HIP_TRY(h, launchIsoBasinJump(a, array, size, s));
      if (readBack(h, &left, a.jumpCount, sizeof(left), s)) return 1;
      if (!left) return 0;
      if (pass >= 32) {
        if (int rc = checkLoopGuard(h, r, fn, kBasinGuard)) return rc;
        h->fail(std::string(fn) + kBasinGuard);
        return 3;
      }
    }
  };
  // the fixed points of array[0, size), which are fewer than the lattice's points, counted per block and scanned: their
  // number into totals[0]
  auto count = [&](uint32_t *array, uint32_t size) -> int {
    IsoScanArgs part = scan;
    part.numBlocks = (size + kIsoBlock - 1) / kIsoBlock;
    part.numChunks = (part.numBlocks + kIsoChunk - 1) / kIsoChunk;
    HIP_TRY(h, launchIsoBasinCount(a, array, size, s));
    HIP_TRY(h, launchIsoScans(part, 1, s));
    return 0;
  };

  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  if (int rc = fillLattice(h, fn, lo, hi, dims, channels, quantity, flags & EXA_SAMPLE_WORLD_SPACE, res.values.p, hipStream)) return rc;
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  if (int rc = lap(0, 0)) return rc;

  // the ascent: inside test and counts, the up links, their resolution
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  HIP_TRY(h, hipMemsetAsync(a.totals, 0, 3 * sizeof(uint64_t), s));
  HIP_TRY(h, launchIsoBasinInit(a, s));
  HIP_TRY(h, launchIsoBasinUp(a, s));
  if (int rc = resolve(a.comp, a.numPoints)) return rc;
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  if (int rc = lap(0, 1)) return rc;

  // the peaks, counted and numbered
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  if (int rc = count(a.comp, a.numPoints)) return rc;
  uint64_t totals[3] = { 0, 0, 0 };              // raw basins, inside points, bits of max |V|
  if (readBack(h, totals, a.totals, sizeof(totals), s)) return 1;
  const int32_t exponent = sumExponentOf(totals);
  a.scale = std::ldexp(1.0, exponent);
  a.numRaw = uint32_t(totals[0]);                // <= n
  uint64_t numFinal = 0;
  int32_t numRounds = 0;
  if (a.numRaw) {
    // per raw basin: the word of its pass | its peak, its link, its final number
    DevBuf<char> raw;
    DevBuf<uint64_t> keys;
    hipError_t e = raw.alloc(size_t(a.numRaw) * 20);
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the raw basins (20 bytes each)", e);
    a.pass = reinterpret_cast<uint64_t *>(raw.p);
    a.peakOf = reinterpret_cast<uint32_t *>(raw.p + size_t(a.numRaw) * 8);
    a.link = a.peakOf + a.numRaw;
    a.finalOf = a.link + a.numRaw;
    HIP_TRY(h, launchIsoBasinRank(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    if (int rc = lap(0, 4)) return rc;

    // the rounds; the last one makes no link and leaves every component's word for the table
    for (;;) {
      uint32_t links = 0;
      HIP_TRY(h, hipEventRecord(t.ev[0], s));
      HIP_TRY(h, hipMemsetAsync(a.pass, 0, size_t(a.numRaw) * 8, s));
      HIP_TRY(h, launchIsoBasinPass(a, s));
      HIP_TRY(h, hipEventRecord(t.ev[1], s));
      HIP_TRY(h, hipMemsetAsync(a.jumpCount, 0, sizeof(uint32_t), s));
      HIP_TRY(h, launchIsoBasinLink(a, s));
      if (readBack(h, &links, a.jumpCount, sizeof(links), s)) return 1;
      if (links) {
        if (uint32_t(numRounds) >= a.numRaw) {   // every round but the last removes a component
          if (int rc = checkLoopGuard(h, r, fn, kBasinGuard)) return rc;
          h->fail(std::string(fn) + kBasinGuard);
          return 3;
        }
        numRounds++;
        if (int rc = resolve(a.link, a.numRaw)) return rc;
        HIP_TRY(h, launchIsoBasinMerge(a, s));
      }
      HIP_TRY(h, hipEventRecord(t.ev[2], s));
      if (int rc = lap(0, 2)) return rc;
      if (int rc = lap(1, 3)) return rc;
      if (!links) break;
    }

    // the components, counted and numbered; the table
    HIP_TRY(h, hipEventRecord(t.ev[0], s));
    if (int rc = count(a.link, a.numRaw)) return rc;
    if (readBack(h, &numFinal, a.totals, sizeof(numFinal), s)) return 1;
    a.numBasins = uint32_t(numFinal);            // 1 <= numBasins <= numRaw
    e = res.table.alloc(size_t(numFinal));
    if (e == hipSuccess) e = keys.alloc(2 * size_t(numFinal));
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the table of basins (96 bytes each, and 16 while the call runs)", e);
    a.basins = res.table.p;
    a.keys = keys.p;
    HIP_TRY(h, launchIsoBasinFinal(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    HIP_TRY(h, launchIsoBasinStats(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[2], s));
    if (int rc = lap(0, 4)) return rc;           // the raw basins' arrays and the keys are freed behind it
    if (int rc = lap(1, 5)) return rc;
  } else {                                       // no basin: every label is the outside mark, which is -1
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    if (int rc = lap(0, 4)) return rc;
  }
  if (int rc = checkLoopGuard(h, r, fn, kBasinGuard)) return rc;
  labelledCommit(res, basins, flags, totals, exponent, numInside, sumExponent);
  if (numBasins) *numBasins = numFinal;
  if (numRawBasins) *numRawBasins = totals[0];
  if (rounds) *rounds = numRounds;
  return 0;
}

static void basinsZero(uint64_t *numBasins, uint64_t *numRawBasins, uint64_t *numInside, int32_t *sumExponent, int32_t *rounds)
{
  if (numBasins) *numBasins = 0;
  if (numRawBasins) *numRawBasins = 0;
  if (numInside) *numInside = 0;
  if (sumExponent) *sumExponent = 0;
  if (rounds) *rounds = 0;
}

int exa_hip_basins(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel, float iso,
                   float minDepth, int32_t flags, uint64_t *numBasins, uint64_t *numRawBasins, uint64_t *numInside,
                   int32_t *sumExponent, int32_t *rounds, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_basins";
  basinsZero(numBasins, numRawBasins, numInside, sumExponent, rounds);
  int rc = 1;
  if (checkFlags(h, fn, flags, kRegionFlags, kRegionFlagsHint) && checkChannel(h, fn, channel))
    rc = basinsExtract(h, fn, lo, hi, dims, &channel, -1, iso, minDepth, flags, numBasins, numRawBasins, numInside, sumExponent, rounds,
                       hipStream);
  if (rc) (void)exa_hip_basins_release(h);             // a failed call leaves no result, whichever check refused it
  return rc;
}

int exa_hip_basins_derived(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t channels[3],
                           int32_t quantity, float iso, float minDepth, int32_t flags, uint64_t *numBasins, uint64_t *numRawBasins,
                           uint64_t *numInside, int32_t *sumExponent, int32_t *rounds, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_basins_derived";
  basinsZero(numBasins, numRawBasins, numInside, sumExponent, rounds);
  int rc = 1;
  if (checkFlags(h, fn, flags, kRegionFlags, kRegionFlagsHint) && oneComponent(h, fn, channels, quantity, "basins need"))
    rc = basinsExtract(h, fn, lo, hi, dims, channels, quantity, iso, minDepth, flags, numBasins, numRawBasins, numInside, sumExponent,
                       rounds, hipStream);
  if (rc) (void)exa_hip_basins_release(h);
  return rc;
}

int exa_hip_basins_read(ExaHipRenderer *h, int32_t *labels, ExaHipBasin *basins, float *values, int32_t pointersAreDevice,
                        void *hipStream)
{
  return labelledRead(h, "exa_hip_basins_read", &ExaHipRenderer::isoBasins,
                      "no basins (exa_hip_basins comes first; a release or a failed call drops them)",
                      "the basins were extracted without EXA_REGIONS_KEEP_VALUES", labels, basins, values, pointersAreDevice, hipStream);
}

int exa_hip_basins_release(ExaHipRenderer *h) { return releaseResult(h, &ExaHipRenderer::isoBasins); }
int exa_hip_basins_stage_ms(ExaHipRenderer *h, float ms[6]) { return readStageMs(h, &ExaHipRenderer::isoBasins, ms); }

// ---- critical points of a vector field on a lattice (exa_isomesh.hip) ----
// The three lattices are three exa_hip_resample calls into one device buffer.  Two small read-backs size what follows: the
// number of candidates behind the first scans (the candidate list and the iteration's state), the number of found points
// behind the second (the records).  The timing events are recorded stage by stage also where a stage has nothing to do.
int exa_hip_critical_points(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t channels[3],
                            int32_t iterations, float tolerance, int32_t flags, uint64_t *numPoints, ExaHipCriticalStats *stats,
                            void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_critical_points";
  if (numPoints) *numPoints = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  r->isoCritical.release();
  DropUnlessCommitted<ExaHipRenderer::IsoCritical> result(r->isoCritical);     // whatever fails from here on leaves no result
  ExaHipRenderer::IsoCritical &res = r->isoCritical;
  for (float &ms : res.stageMs) ms = 0.f;
  if (!lo || !hi || !dims || !channels) { h->fail(std::string(fn) + ": null argument (lo, hi, dims or channels)"); return 1; }
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_CRITICAL_PROBE, " (EXA_SAMPLE_WORLD_SPACE and EXA_CRITICAL_PROBE apply)")) return 1;
  for (int c = 0; c < 3; c++)
    if (!checkChannel(h, fn, channels[c])) return 1;
  if (iterations < 1 || iterations > EXA_CRITICAL_MAX_ITERATIONS) { h->fail(std::string(fn) + ": iterations must be 1 .. EXA_CRITICAL_MAX_ITERATIONS (32)"); return 1; }
  if (!(std::isfinite(tolerance) && tolerance > 0.f && tolerance <= 1.f)) { h->fail(std::string(fn) + ": the tolerance must be finite and in (0, 1]"); return 1; }
  const uint64_t n = latticePoints(h, fn, lo, hi, dims, 2, "dims must be >= 2 on every axis (a lattice of cells)",
                                   "the box needs finite lo < hi on every axis", true);
  if (!n) return 1;
  hipStream_t s = (hipStream_t)hipStream;
  const int32_t wf = flags & EXA_SAMPLE_WORLD_SPACE;
  const bool probe = (flags & EXA_CRITICAL_PROBE) != 0;

  IsoCriticalArgs a;
  std::memset(&a, 0, sizeof(a));
  a.numPoints = uint32_t(n);
  a.nx = uint32_t(dims[0]); a.ny = uint32_t(dims[1]); a.nz = uint32_t(dims[2]);
  for (int k = 0; k < 3; k++) { a.lo[k] = lo[k]; a.step[k] = (hi[k] - lo[k]) / float(dims[k]); }
  a.iterations = iterations;
  a.tolerance = tolerance;
  // the work space of the lattice: the scans' with totals[2] (candidates, found), then the counters and the marks
  DevBuf<float> values;
  DevBuf<char> work;
  IsoScanArgs scan;
  const size_t waves = size_t((n + kIsoBlock - 1) / kIsoBlock) * (kIsoBlock / 64);
  hipError_t e = values.alloc(3 * size_t(n));
  if (e == hipSuccess) e = allocScans(work, n, 1, 1 + 7 + waves, 0, a, scan);
  if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the three lattices (12 bytes per point) and the work space", e);
  a.values = values.p;
  a.counters = reinterpret_cast<unsigned long long *>(a.totals + 2);
  a.marks = a.counters + 7;

  TimingEvents<8> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  for (int c = 0; c < 3; c++)
    if (int rc = fillLattice(h, fn, lo, hi, dims, channels + c, -1, wf, values.p + size_t(c) * n, hipStream)) return rc;
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  HIP_TRY(h, hipMemsetAsync(a.totals, 0, 9 * sizeof(uint64_t), s));
  HIP_TRY(h, launchIsoCriticalCells(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[2], s));
  HIP_TRY(h, launchIsoScans(scan, 1, s));
  uint64_t totals[2] = { 0, 0 };                 // candidates, found
  if (readBack(h, totals, a.totals, sizeof(uint64_t), s)) return 1;
  a.numCandidates = uint32_t(totals[0]);         // <= n
  a.numCandBlocks = uint32_t((totals[0] + kIsoBlock - 1) / kIsoBlock);
  a.numCandChunks = (a.numCandBlocks + kIsoChunk - 1) / kIsoChunk;
  // the work space of the candidates: candChunkBase | candidates, result, candCount, candBase | state
  DevBuf<char> candWork;
  DevBuf<float> positions, probeValues, probeGradients;
  if (a.numCandidates) {
    const size_t nc = a.numCandidates, c32 = 2 * nc + 2 * size_t(a.numCandBlocks);
    e = candWork.alloc(size_t(a.numCandChunks) * 8 + c32 * 4 + 4 * nc * 4);
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the candidates (24 bytes each)", e);
    a.candChunkBase = reinterpret_cast<uint64_t *>(candWork.p);
    a.candidates = reinterpret_cast<uint32_t *>(candWork.p + size_t(a.numCandChunks) * 8);
    a.result = reinterpret_cast<int32_t *>(a.candidates + nc);
    a.candCount = reinterpret_cast<uint32_t *>(a.result + nc);
    a.candBase = a.candCount + a.numCandBlocks;
    a.state = reinterpret_cast<float *>(a.candBase + a.numCandBlocks);
    HIP_TRY(h, launchIsoCriticalCompact(a, s));
  }
  HIP_TRY(h, hipEventRecord(t.ev[3], s));
  if (a.numCandidates) HIP_TRY(h, launchIsoCriticalRefine(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[4], s));
  if (a.numCandidates) {
    // the found points per block of candidates, scanned: their number into totals[1]
    const IsoScanArgs found = { a.numCandBlocks, a.numCandChunks, a.candCount, a.candBase, a.candChunkBase, a.totals + 1 };
    HIP_TRY(h, launchIsoScans(found, 1, s));
    if (readBack(h, totals + 1, a.totals + 1, sizeof(uint64_t), s)) return 1;
  }
  HIP_TRY(h, hipEventRecord(t.ev[5], s));
  a.numFound = uint32_t(totals[1]);              // <= the candidates
  if (a.numFound) {
    const size_t nf = a.numFound;
    e = res.points.alloc(nf);
    if (e == hipSuccess && probe) e = positions.alloc(3 * nf);
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the points (104 bytes each)", e);
    a.points = res.points.p;
    a.positions = positions.p;
    HIP_TRY(h, launchIsoCriticalEmit(a, s));
  }
  HIP_TRY(h, hipEventRecord(t.ev[6], s));
  if (probe && a.numFound) {
    // the existing points kernel on the device positions, then its two arrays interleaved into the contract's one
    const size_t nf = a.numFound;
    e = probeValues.alloc(3 * nf);
    if (e == hipSuccess) e = probeGradients.alloc(9 * nf);
    if (e == hipSuccess) e = res.probe.alloc(12 * nf);
    if (e == hipSuccess) e = res.probeStatus.alloc(3 * nf);
    if (e != hipSuccess) return failNoMemory(h, fn, "no device memory for the probe (120 bytes per point)", e);
    const int32_t pf = wf | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED;
    if (int rc = exa_hip_sample_points(h, positions.p, nf, channels, 3, pf, NAN, probeValues.p, probeGradients.p, res.probeStatus.p, 1, hipStream, 0))
      return failedIn(h, fn, rc);
    a.probeValues = probeValues.p;
    a.probeGradients = probeGradients.p;
    a.probe = res.probe.p;
    HIP_TRY(h, launchIsoCriticalPack(a, s));
  }
  HIP_TRY(h, hipEventRecord(t.ev[7], s));
  uint64_t counters[7] = { 0, 0, 0, 0, 0, 0, 0 };
  if (readBack(h, counters, a.counters, sizeof(counters), s)) return 1;      // the work spaces are freed behind it
  float ms[7];
  for (int k = 0; k < 7; k++) HIP_TRY(h, t.elapsed(k, k + 1, &ms[k]));
  res.stageMs[0] = ms[0]; res.stageMs[1] = ms[1]; res.stageMs[2] = ms[2] + ms[4];
  res.stageMs[3] = ms[3]; res.stageMs[4] = ms[5]; res.stageMs[5] = probe && a.numFound ? ms[6] : 0.f;
  res.probed = probe;
  res.have = true;
  result.commit();
  if (numPoints) *numPoints = totals[1];
  if (stats) {
    stats->cells = counters[0]; stats->invalidCells = counters[1];
    stats->candidates = totals[0]; stats->found = totals[1];
    stats->nonFinite = counters[4]; stats->leftCell = counters[5]; stats->notConverged = counters[6];
  }
  return 0;
}

int exa_hip_critical_points_read(ExaHipRenderer *h, ExaHipCriticalPoint *points, float *probe, int32_t *probeStatus,
                                 int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_critical_points_read";
  ExaHipRenderer *r = firstChild(h);
  const ExaHipRenderer::IsoCritical &res = r->isoCritical;
  if (!res.have) { h->fail(std::string(fn) + ": no points (exa_hip_critical_points comes first; a release or a failed call drops them)"); return 1; }
  if ((probe || probeStatus) && !res.probed) { h->fail(std::string(fn) + ": the points were extracted without EXA_CRITICAL_PROBE"); return 1; }
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  const hipMemcpyKind kind = pointersAreDevice ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
  HIP_TRY(h, copyOut(points, res.points, kind, s));
  HIP_TRY(h, copyOut(probe, res.probe, kind, s));
  HIP_TRY(h, copyOut(probeStatus, res.probeStatus, kind, s));
  HIP_TRY(h, hipStreamSynchronize(s));
  return 0;
}

int exa_hip_critical_points_release(ExaHipRenderer *h) { return releaseResult(h, &ExaHipRenderer::isoCritical); }
int exa_hip_critical_points_stage_ms(ExaHipRenderer *h, float ms[6]) { return readStageMs(h, &ExaHipRenderer::isoCritical, ms); }

} // extern "C"

// ---- profiles and phase plots on a lattice (exa_isomesh.hip) ----
// the lattices the call's channel / derived sources need, each once, and where every such source reads
struct ProfileLattices {
  struct Lattice { int32_t channels[3]; int32_t quantity; };      // quantity < 0: the one channel channels[0]
  std::vector<Lattice> distinct;
  std::vector<std::pair<int, size_t>> users;                      // the slot of IsoProfileArgs::sources, the lattice
};

// One source of the call into slot `slot` of the kernels' arguments, false after h->fail.  A channel / derived source is
// noted in `lat`: its values pointer follows once the lattices are allocated.
static bool profileSourceOf(ExaHipRenderer *h, const char *fn, const ExaHipSource &src, ProfileLattices &lat, IsoProfileArgs &a, int slot)
{
  IsoProfileSource &out = a.sources[slot];
  a.kinds |= uint32_t(src.kind == EXA_SOURCE_DERIVED ? kIsoProfileMemoryKind : src.kind) << (4 * slot);
  static_assert(EXA_SOURCE_CHANNEL == kIsoProfileMemoryKind, "a channel's lattice is a lattice in memory");
  switch (src.kind) {
  case EXA_SOURCE_CHANNEL:
  case EXA_SOURCE_DERIVED: {
    ProfileLattices::Lattice want = { { src.channels[0], 0, 0 }, -1 };
    if (src.kind == EXA_SOURCE_CHANNEL) {
      if (!checkChannel(h, fn, src.channels[0])) return false;
    } else {
      if (!oneComponent(h, fn, src.channels, src.quantity, "a source needs")) return false;
      want = { { src.channels[0], src.channels[1], src.channels[2] }, src.quantity };
    }
    size_t at = 0;
    while (at < lat.distinct.size() && std::memcmp(&lat.distinct[at], &want, sizeof(want)) != 0) at++;
    if (at == lat.distinct.size()) lat.distinct.push_back(want);
    lat.users.push_back({ slot, at });
    return true;
  }
  case EXA_SOURCE_RADIUS:
    for (int k = 0; k < 3; k++) {
      if (!std::isfinite(src.centre[k])) { h->fail(std::string(fn) + ": the centre of a radius source must be finite"); return false; }
      out.centre[k] = src.centre[k];
    }
    a.needPosition = 1;
    return true;
  case EXA_SOURCE_COORDINATE:
    if (src.channels[0] < 0 || src.channels[0] > 2) { h->fail(std::string(fn) + ": a coordinate source needs its axis 0..2 in channels[0]"); return false; }
    out.axis = src.channels[0];
    a.needPosition = 1;
    return true;
  default:
    h->fail(std::string(fn) + ": unknown source kind (EXA_SOURCE_*)");
    return false;
  }
}

// the exponent of a series out of the number of binned points and the bits of its max |term|: the regions' rule
static int32_t profileExponent(uint64_t binned, uint32_t maxBits)
{
  const uint64_t totals[3] = { 0, binned, maxBits };
  return sumExponentOf(totals);
}

extern "C" {

int exa_hip_profile(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], int32_t flags,
                    const ExaHipProfileAxis *axes, int32_t numAxes, const ExaHipSource *values, int32_t numValues,
                    const ExaHipSource *weight, uint64_t *count, int64_t *sumWeight, int64_t *sums, float *mins, float *maxs,
                    ExaHipProfileStats *stats, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_profile";
  ExaHipRenderer *r = firstChild(h);
  for (float &ms : r->profile.stageMs) ms = 0.f;
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_PROFILE_LABELS_DEVICE, " (EXA_SAMPLE_WORLD_SPACE and EXA_PROFILE_LABELS_DEVICE apply)")) return 1;
  if (!lo || !hi || !dims || !axes || !count) { h->fail(std::string(fn) + ": null argument (lo, hi, dims, axes or count)"); return 1; }
  if (numAxes != 1 && numAxes != 2) { h->fail(std::string(fn) + ": numAxes must be 1 or 2"); return 1; }
  if (numAxes == 2 && axes[1].labels) { h->fail(std::string(fn) + ": labels on the second axis (only the first axis takes labels)"); return 1; }
  if (numValues < 0 || numValues > EXA_PROFILE_MAX_VALUES) { h->fail(std::string(fn) + ": numValues must be 0..4"); return 1; }
  if (numValues > 0 && (!values || !sums)) { h->fail(std::string(fn) + ": null values or sums with numValues > 0"); return 1; }
  if ((weight != nullptr) != (sumWeight != nullptr)) { h->fail(std::string(fn) + ": sumWeight needs a weight, and a weight needs sumWeight"); return 1; }
  if ((mins != nullptr) != (maxs != nullptr)) { h->fail(std::string(fn) + ": mins and maxs come together (both or neither)"); return 1; }
  const uint64_t n = latticePoints(h, fn, lo, hi, dims, 1, "dims must be >= 1 on every axis", "the box must be finite with lo < hi on every axis", true);
  if (!n) return 1;

  // the sources and the axes
  IsoProfileArgs a;
  std::memset(&a, 0, sizeof(a));
  ProfileLattices lat;
  std::vector<float> edges;                                   // both axes' one behind the other
  size_t edgesAt[2] = { 0, 0 };
  uint64_t bins = 1;
  for (int ax = 0; ax < numAxes; ax++) {
    const ExaHipProfileAxis &in = axes[ax];
    IsoProfileKey &key = a.axes[ax];
    if (in.numBins < 1) { h->fail(std::string(fn) + ": numBins must be >= 1 on every axis"); return 1; }
    key.numBins = in.numBins;
    bins *= uint64_t(in.numBins);                              // two factors below 2^31
    if (in.labels) { key.mode = kIsoProfileLabels; continue; }
    if (!profileSourceOf(h, fn, in.source, lat, a, ax)) return 1;
    if (in.edges) {
      if (bins > uint64_t(EXA_PROFILE_MAX_BINS)) break;        // refused below, before the edges are read
      for (int32_t b = 0; b <= in.numBins; b++)
        if (!std::isfinite(in.edges[b]) || (b && !(in.edges[b] > in.edges[b - 1]))) { h->fail(std::string(fn) + ": edges must be finite and strictly ascending"); return 1; }
      key.mode = kIsoProfileEdges;
      key.lo = in.edges[0]; key.hi = in.edges[in.numBins];
      edgesAt[ax] = edges.size();
      edges.insert(edges.end(), in.edges, in.edges + in.numBins + 1);
    } else {
      if (!(std::isfinite(in.lo) && std::isfinite(in.hi) && in.lo < in.hi)) { h->fail(std::string(fn) + ": the range needs finite lo < hi"); return 1; }
      const float width = in.hi - in.lo;
      key.mode = kIsoProfileUniform;
      key.lo = in.lo; key.hi = in.hi; key.scale = float(in.numBins) / width;
      if (!std::isfinite(width) || !std::isfinite(key.scale)) { h->fail(std::string(fn) + ": hi - lo and numBins / (hi - lo) must be finite in float32"); return 1; }
    }
  }
  if (bins > uint64_t(EXA_PROFILE_MAX_BINS)) { h->fail(std::string(fn) + ": the number of bins must be 1 .. 2^24"); return 1; }
  for (int f = 0; f < numValues; f++)
    if (!profileSourceOf(h, fn, values[f], lat, a, kIsoProfileValueSlot + f)) return 1;
  if (weight && !profileSourceOf(h, fn, *weight, lat, a, kIsoProfileWeightSlot)) return 1;
  const size_t B = size_t(bins), nv = size_t(numValues), ns = nv + (weight ? 1 : 0);
  const bool minMax = mins != nullptr && nv > 0;
  a.numPoints = uint32_t(n);
  a.nx = uint32_t(dims[0]); a.ny = uint32_t(dims[1]);
  for (int k = 0; k < 3; k++) { a.lo[k] = lo[k]; a.step[k] = (hi[k] - lo[k]) / float(dims[k]); }
  a.numAxes = uint32_t(numAxes); a.numValues = uint32_t(numValues); a.hasWeight = weight ? 1 : 0; a.minMax = minMax ? 1 : 0;
  a.numBlocks = uint32_t((n + kIsoBlock - 1) / kIsoBlock);
  a.numBins = uint32_t(B);

  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  if (r->applyBrickOrder(s)) { h->fail(r->err); return 1; }

  // the work space: the lattices, the bin indices, labels that come from the host, the edges, the counters, the table
  // (sums | count | max keys | min keys: what starts as zeros, then what starts as ones)
  const bool hostLabels = axes[0].labels && !(flags & EXA_PROFILE_LABELS_DEVICE);
  const size_t counterWords = kIsoProfileCounters + (kIsoProfileSeries + 1) / 2, zeroWords = (ns + 1) * B + (minMax ? (nv * B + 1) / 2 : 0),
               tableWords = zeroWords + (minMax ? (nv * B + 1) / 2 : 0);
  DevBuf<float> lattices, devEdges;
  DevBuf<uint32_t> binOf;
  DevBuf<int32_t> devLabels;
  DevBuf<unsigned long long> counters, table;
  hipError_t e = lattices.alloc(lat.distinct.size() * size_t(n));
  if (e == hipSuccess) e = binOf.alloc(size_t(n));
  if (e == hipSuccess && hostLabels) e = devLabels.alloc(size_t(n));
  if (e == hipSuccess) e = devEdges.alloc(edges.size());
  if (e == hipSuccess) e = counters.alloc(counterWords);
  if (e == hipSuccess) e = table.alloc(tableWords);
  if (e != hipSuccess)
    return failNoMemory(h, fn, "no device memory for the lattices (4 bytes per point and distinct source), the bin indices (4 more) and the table (8 bytes per bin and series, 8 for the count, 8 per value with min / max)", e);
  for (auto &user : lat.users) a.sources[user.first].values = lattices.p + user.second * size_t(n);
  for (int ax = 0; ax < numAxes; ax++) a.axes[ax].edges = a.axes[ax].mode == kIsoProfileEdges ? devEdges.p + edgesAt[ax] : nullptr;
  a.labels = hostLabels ? devLabels.p : axes[0].labels;
  a.bins = binOf.p;
  a.counters = counters.p;
  a.sums = table.p;
  a.count = table.p + ns * B;
  a.keyMax = reinterpret_cast<uint32_t *>(table.p + (ns + 1) * B);
  a.keyMin = reinterpret_cast<uint32_t *>(table.p + zeroWords);

  TimingEvents<6> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  for (size_t k = 0; k < lat.distinct.size(); k++)
    if (int rc = fillLattice(h, fn, lo, hi, dims, lat.distinct[k].channels, lat.distinct[k].quantity, flags & EXA_SAMPLE_WORLD_SPACE,
                             lattices.p + k * size_t(n), hipStream)) return rc;
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  unsigned long long start[kIsoProfileCounters + (kIsoProfileSeries + 1) / 2] = {};
  start[kIsoProfileBadLabel] = ~0ull;
  HIP_TRY(h, hipMemcpyAsync(counters.p, start, sizeof(start), hipMemcpyHostToDevice, s));
  if (hostLabels) HIP_TRY(h, hipMemcpyAsync(devLabels.p, axes[0].labels, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, s));
  if (!edges.empty()) HIP_TRY(h, hipMemcpyAsync(devEdges.p, edges.data(), edges.size() * sizeof(float), hipMemcpyHostToDevice, s));
  HIP_TRY(h, hipMemsetAsync(table.p, 0, zeroWords * 8, s));
  if (tableWords > zeroWords) HIP_TRY(h, hipMemsetAsync(table.p + zeroWords, 0xff, (tableWords - zeroWords) * 8, s));
  HIP_TRY(h, launchIsoProfileClassify(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[2], s));
  unsigned long long got[kIsoProfileCounters + (kIsoProfileSeries + 1) / 2];
  if (readBack(h, got, counters.p, sizeof(got), s)) return 1;
  if (got[kIsoProfileBadLabel] != ~0ull) {
    h->fail(std::string(fn) + ": a label >= numBins, first at L = " + std::to_string(got[kIsoProfileBadLabel]));
    return 1;
  }
  uint32_t magnitudes[kIsoProfileSeries];
  std::memcpy(magnitudes, got + kIsoProfileCounters, sizeof(magnitudes));
  int32_t exponent[kIsoProfileSeries] = {};
  for (int q = 0; q < kIsoProfileSeries; q++) {
    const bool have = q == 0 ? weight != nullptr : q - 1 < numValues;
    exponent[q] = have ? profileExponent(got[kIsoProfileBinned], magnitudes[q]) : 0;
    a.exponent[q] = exponent[q];
  }
  HIP_TRY(h, hipEventRecord(t.ev[3], s));
  if (got[kIsoProfileBinned]) HIP_TRY(h, launchIsoProfileAccumulate(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[4], s));
  if (minMax) HIP_TRY(h, launchIsoProfileFinish(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[5], s));
  HIP_TRY(h, hipMemcpyAsync(count, a.count, B * 8, hipMemcpyDeviceToHost, s));
  if (weight) HIP_TRY(h, hipMemcpyAsync(sumWeight, a.sums, B * 8, hipMemcpyDeviceToHost, s));
  if (nv) HIP_TRY(h, hipMemcpyAsync(sums, a.sums + (ns - nv) * B, nv * B * 8, hipMemcpyDeviceToHost, s));
  if (minMax) {
    HIP_TRY(h, hipMemcpyAsync(mins, a.keyMin, nv * B * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipMemcpyAsync(maxs, a.keyMax, nv * B * 4, hipMemcpyDeviceToHost, s));
  }
  HIP_TRY(h, hipStreamSynchronize(s));                  // the work space is freed behind it
  float *ms = r->profile.stageMs;
  HIP_TRY(h, t.elapsed(0, 1, &ms[0]));
  HIP_TRY(h, t.elapsed(1, 2, &ms[1]));
  HIP_TRY(h, t.elapsed(3, 4, &ms[2]));
  HIP_TRY(h, t.elapsed(4, 5, &ms[3]));
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->points = n;
    stats->outside = got[kIsoProfileOutside]; stats->invalid = got[kIsoProfileInvalid];
    for (int ax = 0; ax < 2; ax++) { stats->under[ax] = got[kIsoProfileUnder + ax]; stats->over[ax] = got[kIsoProfileOver + ax]; }
    stats->binned = got[kIsoProfileBinned];
    stats->weightExponent = exponent[0];
    for (int f = 0; f < EXA_PROFILE_MAX_VALUES; f++) stats->valueExponent[f] = exponent[1 + f];
    stats->ldsTable = isoProfileLdsTable(B, numValues) ? 1 : 0;
  }
  return 0;
}

int exa_hip_profile_stage_ms(ExaHipRenderer *h, float ms[4])
{
  if (!h || !ms) return 1;
  for (int k = 0; k < 4; k++) ms[k] = firstChild(h)->profile.stageMs[k];
  return 0;
}

} // extern "C"

// ---- exact Euclidean distance transform on a lattice (exa_isomesh.hip) ----
// exa_hip_distance (quantity < 0: the lattice holds the one channel channels[0]), exa_hip_distance_derived (it holds the
// quantity of channels[0..2]) and exa_hip_distance_mask (channels == nullptr: inside by `labels` and `label`).  The flags,
// the channels and the quantity are checked by the caller.  One run of the passes per target set, two with
// EXA_DISTANCE_SIGNED, each with a finish pass that writes its share of the outputs; one read-back, the three counters.
static int distanceTransform(ExaHipRenderer *h, const char *fn, const float lo[3], const float hi[3], const int32_t dims[3],
                             const int32_t *channels, int32_t quantity, float iso, const int32_t *labels, int32_t label,
                             float maxDistance, int32_t flags, float *dist, int32_t *nearest, ExaHipDistanceStats *stats,
                             int32_t pointersAreDevice, void *hipStream)
{
  ExaHipRenderer *r = firstChild(h);
  for (float &ms : r->distance.stageMs) ms = 0.f;
  const bool mask = channels == nullptr;
  if (!lo || !hi || !dims || !dist) { h->fail(std::string(fn) + ": null argument (lo, hi, dims or dist)"); return 1; }
  if (mask && !labels) { h->fail(std::string(fn) + ": null labels"); return 1; }
  if (mask && label < -1) { h->fail(std::string(fn) + ": label must be >= -1 (-1: every label >= 0)"); return 1; }
  if (!mask && !std::isfinite(iso)) { h->fail(std::string(fn) + ": the iso value must be finite"); return 1; }
  if (!(maxDistance > 0.f)) { h->fail(std::string(fn) + ": maxDistance must be > 0 (+INF for no limit)"); return 1; }
  if ((flags & EXA_DISTANCE_SIGNED) && (flags & EXA_DISTANCE_TO_OUTSIDE)) {
    h->fail(std::string(fn) + ": EXA_DISTANCE_SIGNED excludes EXA_DISTANCE_TO_OUTSIDE");
    return 1;
  }
  const uint64_t n = latticePoints(h, fn, lo, hi, dims, 1, "dims must be >= 1 on every axis", "the box must be finite", false);
  if (!n) return 1;

  IsoDistanceArgs a;
  std::memset(&a, 0, sizeof(a));
  a.numPoints = uint32_t(n);
  a.nx = uint32_t(dims[0]); a.ny = uint32_t(dims[1]); a.nz = uint32_t(dims[2]);
  a.numBlocks = uint32_t((n + kIsoBlock - 1) / kIsoBlock);
  for (int k = 0; k < 3; k++) {
    a.h[k] = (hi[k] - lo[k]) / float(dims[k]);
    if (!std::isfinite(a.h[k])) { h->fail(std::string(fn) + ": the spacing (hi - lo) / dims must be finite in float32"); return 1; }
  }
  a.limit = maxDistance * maxDistance;
  a.iso = iso;
  a.label = label;
  a.byLabel = mask ? 1 : 0;
  a.below = (flags & EXA_DISTANCE_BELOW) ? 1 : 0;

  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  if (!mask && r->applyBrickOrder(s)) { h->fail(r->err); return 1; }

  // the work space: a | b | c | gy | d2 | dist and nearest for host pointers | the inside bytes | and the counters
  const bool staged = !pointersAreDevice, hostLabels = mask && !(flags & EXA_DISTANCE_LABELS_DEVICE);
  const size_t N = size_t(n), words = 5 + (staged ? 1 + (nearest ? 1 : 0) : 0);
  DevBuf<char> work;
  DevBuf<unsigned long long> counters;
  hipError_t e = work.alloc(words * 4 * N + N);
  if (e == hipSuccess) e = counters.alloc(kIsoDistanceCounters);
  if (e != hipSuccess)
    return failNoMemory(h, fn, "no device memory for the passes (21 bytes per point, and 4 each for dist and nearest with host pointers)", e);
  int32_t *ints = reinterpret_cast<int32_t *>(work.p);
  a.a = ints; a.b = ints + N; a.c = ints + 2 * N;
  a.gy = reinterpret_cast<float *>(ints + 3 * N); a.d2 = reinterpret_cast<float *>(ints + 4 * N);
  a.dist = staged ? reinterpret_cast<float *>(ints + 5 * N) : dist;
  a.nearest = !nearest ? nullptr : staged ? ints + 6 * N : nearest;
  a.inside = reinterpret_cast<uint8_t *>(ints + words * N);
  a.counters = counters.p;
  a.values = a.d2;                                      // read by the inside pass only, d2 is written behind it
  a.labels = hostLabels ? a.c : labels;                 // likewise

  TimingEvents<8> t;
  HIP_TRY(h, t.create());
  HIP_TRY(h, hipEventRecord(t.ev[0], s));
  if (!mask) {
    if (int rc = fillLattice(h, fn, lo, hi, dims, channels, quantity, flags & EXA_SAMPLE_WORLD_SPACE, a.d2, hipStream)) return rc;
  } else if (hostLabels) {
    HIP_TRY(h, hipMemcpyAsync(a.c, labels, N * sizeof(int32_t), hipMemcpyHostToDevice, s));
  }
  HIP_TRY(h, hipMemsetAsync(counters.p, 0, kIsoDistanceCounters * sizeof(unsigned long long), s));
  HIP_TRY(h, launchIsoDistanceInside(a, s));
  HIP_TRY(h, hipEventRecord(t.ev[1], s));
  const bool isSigned = (flags & EXA_DISTANCE_SIGNED) != 0;
  const int runs = isSigned ? 2 : 1;
  for (int run = 0; run < runs; run++) {
    a.toOutside = isSigned ? run : (flags & EXA_DISTANCE_TO_OUTSIDE) ? 1 : 0;
    a.negative = isSigned && run == 1 ? 1 : 0;
    a.onlyOthers = isSigned ? 1 : 0;
    HIP_TRY(h, launchIsoDistanceRows(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[2 + 3 * run], s));
    HIP_TRY(h, launchIsoDistanceColumns(a, 1, s));
    HIP_TRY(h, launchIsoDistanceColumns(a, 2, s));
    HIP_TRY(h, hipEventRecord(t.ev[3 + 3 * run], s));
    HIP_TRY(h, launchIsoDistanceFinish(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[4 + 3 * run], s));
  }
  if (staged) {
    HIP_TRY(h, hipMemcpyAsync(dist, a.dist, N * sizeof(float), hipMemcpyDeviceToHost, s));
    if (nearest) HIP_TRY(h, hipMemcpyAsync(nearest, a.nearest, N * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  }
  unsigned long long got[kIsoDistanceCounters] = {};
  if (readBack(h, got, counters.p, sizeof(got), s)) return 1;         // the work space is freed behind it
  float *ms = r->distance.stageMs;
  HIP_TRY(h, t.elapsed(0, 1, &ms[0]));
  for (int run = 0; run < runs; run++)
    for (int k = 0; k < 3; k++) {
      float part = 0.f;
      HIP_TRY(h, t.elapsed(1 + 3 * run + k, 2 + 3 * run + k, &part));
      ms[1 + k] += part;
    }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->points = n;
    stats->inside = got[kIsoDistanceInside];
    stats->reached = got[kIsoDistanceReached];
    const uint32_t bits = uint32_t(got[kIsoDistanceMaxBits]);
    std::memcpy(&stats->maxDistance, &bits, sizeof(bits));
  }
  return 0;
}

static const int32_t kDistanceFieldFlags = EXA_SAMPLE_WORLD_SPACE | EXA_DISTANCE_BELOW | EXA_DISTANCE_TO_OUTSIDE | EXA_DISTANCE_SIGNED;
static const char *const kDistanceFieldHint = " (EXA_SAMPLE_WORLD_SPACE, EXA_DISTANCE_BELOW, EXA_DISTANCE_TO_OUTSIDE and EXA_DISTANCE_SIGNED apply)";

extern "C" {

int exa_hip_distance(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel, float iso,
                     float maxDistance, int32_t flags, float *dist, int32_t *nearest, ExaHipDistanceStats *stats,
                     int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_distance";
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!checkFlags(h, fn, flags, kDistanceFieldFlags, kDistanceFieldHint) || !checkChannel(h, fn, channel)) return 1;
  return distanceTransform(h, fn, lo, hi, dims, &channel, -1, iso, nullptr, 0, maxDistance, flags, dist, nearest, stats,
                           pointersAreDevice, hipStream);
}

int exa_hip_distance_derived(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t channels[3],
                             int32_t quantity, float iso, float maxDistance, int32_t flags, float *dist, int32_t *nearest,
                             ExaHipDistanceStats *stats, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_distance_derived";
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!checkFlags(h, fn, flags, kDistanceFieldFlags, kDistanceFieldHint)) return 1;
  if (!channels) { h->fail(std::string(fn) + ": null argument (channels)"); return 1; }
  if (!oneComponent(h, fn, channels, quantity, "the distance needs")) return 1;
  return distanceTransform(h, fn, lo, hi, dims, channels, quantity, iso, nullptr, 0, maxDistance, flags, dist, nearest, stats,
                           pointersAreDevice, hipStream);
}

int exa_hip_distance_mask(ExaHipRenderer *h, const float lo[3], const float hi[3], const int32_t dims[3], const int32_t *labels,
                          int32_t label, float maxDistance, int32_t flags, float *dist, int32_t *nearest,
                          ExaHipDistanceStats *stats, int32_t pointersAreDevice, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_distance_mask";
  if (stats) std::memset(stats, 0, sizeof(*stats));
  if (!checkFlags(h, fn, flags, EXA_SAMPLE_WORLD_SPACE | EXA_DISTANCE_TO_OUTSIDE | EXA_DISTANCE_SIGNED | EXA_DISTANCE_LABELS_DEVICE,
                  " (EXA_DISTANCE_TO_OUTSIDE, EXA_DISTANCE_SIGNED and EXA_DISTANCE_LABELS_DEVICE apply)")) return 1;
  return distanceTransform(h, fn, lo, hi, dims, nullptr, -1, 0.f, labels, label, maxDistance, flags, dist, nearest, stats,
                           pointersAreDevice, hipStream);
}

int exa_hip_distance_stage_ms(ExaHipRenderer *h, float ms[4])
{
  if (!h || !ms) return 1;
  for (int k = 0; k < 4; k++) ms[k] = firstChild(h)->distance.stageMs[k];
  return 0;
}

} // extern "C"
