// exa_module.cpp — the setters, options and read-backs of the exa_hip_* C ABI; see include/exa_hip.h for the
// per-entry citations.  Creation is in exa_create.cpp, the frame in exa_frame.cpp, probes and iso-surfaces in exa_probe.cpp.
#include "exa_renderer.h"
#include "exa_hostbvh.h"

#include <cmath>
#include <cstring>

namespace {

bool isMulti(const ExaHipRenderer *h) { return h && !h->children.empty(); }

// a call on one renderer of a multi-device handle: the child's error becomes the handle's
template <typename Call>
int onChild(ExaHipRenderer *h, ExaHipRenderer *c, Call call)
{
  const int rc = call(c);
  if (rc) h->fail(c->err);
  return rc;
}

// multi-device handle: the same call on every device's renderer, up to the first that fails
template <typename Call>
int onEveryChild(ExaHipRenderer *h, Call call)
{
  for (ExaHipRenderer *c : h->children)
    if (int rc = onChild(h, c, call)) return rc;
  return 0;
}

} // namespace

extern "C" {

const char *exa_hip_last_error(const ExaHipRenderer *h) { return h ? h->err.c_str() : g_createError.c_str(); }

int exa_hip_resize(ExaHipRenderer *h, int32_t width, int32_t height)
{
  if (!h) return 1;
  if (width <= 0 || height <= 0 || int64_t(width) * height > (int64_t(1) << 30)) { h->fail("exa_hip_resize: bad size"); return 1; }
  if (isMulti(h)) {
    if (int rc = onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_resize(c, width, height); })) return rc;
    h->W = width; h->H = height;
    EXA_ON_DEVICE(h);                         // the root device holds the frame a host destination is copied from
    HIP_TRY(h, h->color.alloc(size_t(width) * height));
    return 0;
  }
  EXA_ON_DEVICE(h);
  h->W = width; h->H = height;
  h->layoutDirty = true;
  return h->rebuildLayout();
}

int exa_hip_set_frame_state(ExaHipRenderer *h, const ExaHipFrameState *fs)
{
  if (isMulti(h)) return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_set_frame_state(c, fs); });
  if (!h || !fs) return 1;
  if (!h->haveFs || std::memcmp(h->fs.xfDomain, fs->xfDomain, sizeof(fs->xfDomain)) != 0
      || h->fs.xfOpacityScale != fs->xfOpacityScale) h->volDirty = true;
  if (!h->haveFs || std::memcmp(h->fs.iso, fs->iso, sizeof(fs->iso)) != 0) h->isoDirty = true;
  if (h->haveFs) {
    // anything but the frame id changes which tiles are expensive
    ExaHipFrameState a = h->fs, b = *fs;
    a.frameID = b.frameID = 0;
    if (std::memcmp(&a, &b, sizeof(a)) != 0) h->costPhase = 1;
  }
  h->fs = *fs;
  h->haveFs = true;
  return 0;
}

int exa_hip_set_xf(ExaHipRenderer *h, int32_t chan, const float *rgba128)
{
  if (isMulti(h)) return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_set_xf(c, chan, rgba128); });
  if (!h || !rgba128) return 1;
  if (chan < 0 || chan >= EXA_MAX_CHANNELS) { h->fail("exa_hip_set_xf: bad channel"); return 1; }
  std::memcpy(h->xfHost[chan], rgba128, sizeof(h->xfHost[chan]));
  h->xfDirty = true;
  h->volDirty = true;                      // needVolumeBVHRebuild = true (OptixRenderer.cpp:403)
  h->costPhase = 1;
  return 0;
}

int exa_hip_set_triangles(ExaHipRenderer *h, const float *vertices, uint64_t numVertices,
                          const int32_t *triangles, uint64_t numTris)
{
  if (isMulti(h)) return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_set_triangles(c, vertices, numVertices, triangles, numTris); });
  if (!h) return 1;
  EXA_ON_DEVICE(h);
  HIP_TRY(h, hipDeviceSynchronize());
  h->numTris = 0;
  h->meshNodes.release(); h->meshVerts.release(); h->meshTris.release();
  if (numTris == 0) return 0;
  if (!vertices || !triangles || numTris > 0x3fffffffull) { h->fail("exa_hip_set_triangles: bad arguments"); return 1; }
  for (uint64_t i = 0; i < 3 * numTris; i++)
    if (triangles[i] < 0 || uint64_t(triangles[i]) >= numVertices) { h->fail("broken triangle model"); return 1; }   // TriangleMesh.cpp:43-52
  // boxes, slightly padded so that axis-aligned triangles keep a non-degenerate slab interval
  std::vector<float> boxes(6 * numTris);
  for (uint64_t t = 0; t < numTris; t++)
    for (int k = 0; k < 3; k++) {
      const float a = vertices[3 * triangles[3 * t] + k], b = vertices[3 * triangles[3 * t + 1] + k], c = vertices[3 * triangles[3 * t + 2] + k];
      const float lo = std::fmin(a, std::fmin(b, c)), hi = std::fmax(a, std::fmax(b, c));
      const float pad = 1e-5f * std::fmax(std::fmax(std::fabs(lo), std::fabs(hi)), hi - lo) + 1e-30f;
      boxes[6 * t + k] = lo - pad; boxes[6 * t + 3 + k] = hi + pad;
    }
  LbvhTopology topo;
  topo.build(boxes.data(), numTris);
  const std::vector<BvhNode> nodes = fillBoxes(topo, boxes, [](size_t t) { return t; });   // leaf = triangle index
  HIP_TRY(h, h->meshNodes.upload(nodes.data(), nodes.size()));
  HIP_TRY(h, h->meshVerts.upload(vertices, 3 * numVertices));
  HIP_TRY(h, h->meshTris.upload(triangles, 3 * numTris));
  h->numTris = (int)numTris;
  return 0;
}

int exa_hip_reset_tracer(ExaHipRenderer *h, const ExaHipTracer *t, const float *seeds)
{
  if (isMulti(h)) return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_reset_tracer(c, t, seeds); });
  if (!h || !t || !seeds) return 1;
  if (t->numTraces < 0 || t->numTimesteps < 2 || (long long)t->numTraces * t->numTimesteps > (1ll << 28)) { h->fail("exa_hip_reset_tracer: bad trace counts"); return 1; }
  for (int k = 0; k < 3; k++)
    if (t->channels[k] < 0 || t->channels[k] >= h->numFields) { h->fail("exa_hip_reset_tracer: tracer channel out of range"); return 1; }
  EXA_ON_DEVICE(h);
  HIP_TRY(h, hipDeviceSynchronize());
  h->tracer = *t;
  h->haveTracer = true;
  std::vector<float> host(size_t(t->numTraces) * t->numTimesteps * 3, 0.f);
  for (int i = 0; i < t->numTraces; i++) std::memcpy(&host[size_t(i) * t->numTimesteps * 3], &seeds[3 * i], 3 * sizeof(float));
  HIP_TRY(h, h->traces.upload(host.data(), host.size()));
  h->timestep = 0;
  h->streamDirty = true;                     // needStreamlineBVHRebuild = true (:461)
  return 0;
}

int exa_hip_set_tracer_enabled(ExaHipRenderer *h, int32_t enabled)
{
  if (isMulti(h)) return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_set_tracer_enabled(c, enabled); });
  if (!h) return 1;
  h->tracer.enabled = enabled;
  return 0;
}

int exa_hip_advance_tracer(ExaHipRenderer *h, int32_t *rebuild)
{
  if (isMulti(h))                              // every device advances; the caller sees the rebuild flag of the first
    return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_advance_tracer(c, c == firstChild(h) ? rebuild : nullptr); });
  if (!h) return 1;
  if (rebuild) *rebuild = 0;
  if (!h->haveTracer || !h->tracer.enabled) return 0;
  h->timestep++;
  if (h->timestep <= h->tracer.numTimesteps) h->streamDirty = true;
  if (rebuild) *rebuild = h->streamDirty;
  return 0;
}

int exa_hip_read_traces(ExaHipRenderer *h, float *dst)
{
  if (isMulti(h))                              // every device holds the same traces
    return onChild(h, firstChild(h), [&](ExaHipRenderer *c) { return exa_hip_read_traces(c, dst); });
  if (!h || !dst || !h->haveTracer) return 1;
  EXA_ON_DEVICE(h);
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipMemcpy(dst, h->traces.p, h->traces.n * sizeof(float), hipMemcpyDeviceToHost));
  return 0;
}

int exa_hip_set_params(ExaHipRenderer *h, const ExaHipParams *p)
{
  if (isMulti(h)) return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_set_params(c, p); });
  if (!h || !p) return 1;
  if (!(p->dt > 0.f)) { h->fail("exa_hip_set_params: dt must be > 0"); return 1; }
  if (!h->haveParams || h->p.numChannels != p->numChannels || h->p.spaceSkippingEnabled != p->spaceSkippingEnabled)
    h->volDirty = true;
  if (!h->haveParams || std::memcmp(&h->p, p, sizeof(*p)) != 0) h->costPhase = 1;
  h->p = *p;
  h->haveParams = true;
  return 0;
}

int exa_hip_set_shard(ExaHipRenderer *h, int32_t rank, int32_t worldSize)
{
  if (isMulti(h)) { h->fail("exa_hip_set_shard: a multi-device handle shards the frame internally"); return 1; }
  if (!h) return 1;
  if (worldSize < 1 || rank < 0 || rank >= worldSize) { h->fail("exa_hip_set_shard: bad rank/world"); return 1; }
  h->rank = rank; h->world = worldSize;
  h->layoutDirty = true;
  if (h->W > 0) { EXA_ON_DEVICE(h); return h->rebuildLayout(); }
  return 0;
}

int exa_hip_set_option(ExaHipRenderer *h, const char *key, int32_t value)
{
  if (isMulti(h)) return onEveryChild(h, [&](ExaHipRenderer *c) { return exa_hip_set_option(c, key, value); });
  if (!h || !key) return 1;
  if (!std::strcmp(key, "tile_order")) { h->tileOrder = value; h->layoutDirty = true; return 0; }
  if (!std::strcmp(key, "tile_feedback")) { h->feedback = value; h->layoutDirty = true; return 0; }
  if (!std::strcmp(key, "wide_march")) {
    if (value != 0 && value != 1 && value != 2 && value != 4) { h->fail("exa_hip_set_option: wide_march is 0, 1, 2 or 4"); return 1; }
    h->wideMode = value; h->layoutDirty = true; return 0;
  }
  if (!std::strcmp(key, "stats_mode")) {
    if (value != 1 && value != 2) { h->fail("exa_hip_set_option: stats_mode is 1 or 2"); return 1; }
    h->statsMode = value; return 0;
  }
  if (!std::strcmp(key, "ao_defer")) {
    if (value < 0 || value > 2) { h->fail("exa_hip_set_option: ao_defer is 0, 1 or 2"); return 1; }
    h->aoDefer = value; return 0;
  }
  if (!std::strcmp(key, "prepass_split")) { h->prepassSplit = value != 0; h->costPhase = 1; return 0; }
  if (!std::strcmp(key, "ao_overlap")) { h->aoOverlap = value != 0; return 0; }
  if (!std::strcmp(key, "walk_probe")) { h->walkProbeOn = value != 0; return 0; }
  if (!std::strcmp(key, "debug_pixel")) { h->debugPixel = value; return 0; }
  if (!std::strcmp(key, "profile_marker")) {            // an empty kernel on the null stream, visible in a profiler's dispatch list
    EXA_ON_DEVICE(h);
    if (launchProfileMarker(value, nullptr) != hipSuccess) { h->fail("exa_hip_set_option: profile_marker launch failed"); return 1; }
    return 0;
  }
  if (!std::strcmp(key, "accel")) { h->accel = value; return 0; }
  if (!std::strcmp(key, "walk")) {
    if (value < 0 || value > 2) { h->fail("exa_hip_set_option: walk is 0 (chosen per frame), 1 (stack walk) or 2 (rope walk)"); return 1; }
    h->walkMode = value; return 0;
  }
  if (!std::strcmp(key, "lbvh_build")) {              // 0 = on the device (default), 1 = on the host; before the first LBVH frame
    if (h->lbvhBuilt && value != h->lbvhOnHost) { h->fail("exa_hip_set_option: lbvh_build must be set before the LBVH is first used"); return 1; }
    h->lbvhOnHost = value; return 0;
  }
  if (!std::strcmp(key, "fast_math")) { h->fastMath = value; return 0; }
  if (!std::strcmp(key, "fast_sampler")) { h->fastSampler = value; return 0; }
  if (!std::strcmp(key, "basis_form")) {
    if (value != 0 && value != 1) { h->fail("exa_hip_set_option: basis_form is 0 or 1"); return 1; }
    if (value && h->emptyCells) {
      h->fail("exa_hip_set_option: a scene with empty cells keeps basis_form 0 (an empty cell is a per-corner property, the per-axis association needs per-axis ones)");
      return 1;
    }
    h->basisForm = value; return 0;
  }
  if (!std::strcmp(key, "sample_patch")) {
    if (value < 0 || value >= kSamplePatchShapes) { h->fail("exa_hip_set_option: sample_patch is 0 (64x1x1), 1 (16x4x1), 2 (8x8x1) or 3 (4x4x4)"); return 1; }
    h->probes.patch = value; return 0;
  }
  if (!std::strcmp(key, "sample_uniform")) { h->probes.uniform = value != 0; return 0; }
  if (!std::strcmp(key, "surface_pack")) { h->surface.pack = value != 0; return 0; }
  if (!std::strcmp(key, "lic_lanes")) {
    if (value != 1 && value != 2) { h->fail("exa_hip_set_option: lic_lanes is 1 (a lane per pixel) or 2 (a lane per pixel and direction)"); return 1; }
    h->lic.lanes = value; return 0;
  }
  if (!std::strcmp(key, "lic_patch")) { h->lic.patch = value != 0; return 0; }
  if (!std::strcmp(key, "flowmap_patch")) { h->flowmap.patch = value != 0; return 0; }
  if (!std::strcmp(key, "interleave")) { h->interleave = value != 0; return 0; }
  if (!std::strcmp(key, "addr64")) { h->addr64 = value != 0; return 0; }
  if (!std::strcmp(key, "pack_records")) { h->packRecords = value != 0; return 0; }
  if (!std::strcmp(key, "cube_records")) { h->cubeRecords = value != 0; return 0; }
  if (!std::strcmp(key, "brick_order")) {
    if (value && !h->brickOrderPossible) {
      h->fail("exa_hip_set_option: brick_order 1 needs channel offsets f * totalCells and brick begins that partition [0, totalCells)");
      return 1;
    }
    h->brickOrderWanted = value != 0; return 0;
  }
  if (!std::strcmp(key, "tf_filter")) {
    if (value != 0 && value != 1) { h->fail("exa_hip_set_option: tf_filter is 0 or 1"); return 1; }
    if (value != h->tfFilter) { h->tfFilter = value; h->volDirty = true; }     // region activity goes through the TF lookup
    return 0;
  }
  h->fail(std::string("exa_hip_set_option: unknown key ") + key);
  return 1;
}

int exa_hip_read_activity(ExaHipRenderer *h, int32_t which, uint8_t *dst)
{
  if (isMulti(h)) return onChild(h, firstChild(h), [&](ExaHipRenderer *c) { return exa_hip_read_activity(c, which, dst); });
  if (!h || !dst) return 1;
  EXA_ON_DEVICE(h);
  if (h->prepareFrame(nullptr)) return 1;
  if (which == 1 && !h->isoEnabled()) {     // evaluate on demand
    HIP_TRY(h, launchIsoActivity(h->sc, h->fs, h->isoActive.p, nullptr));
  }
  HIP_TRY(h, hipDeviceSynchronize());
  HIP_TRY(h, hipMemcpy(dst, which ? h->isoActive.p : h->volActive.p, h->sc.numRegions, hipMemcpyDeviceToHost));
  return 0;
}

} // extern "C"
