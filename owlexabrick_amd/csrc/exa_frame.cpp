// exa_frame.cpp — a frame of the exa_hip_* module: tile layout and launch-order feedback, wide-march assignment, LBVH
// build, activity and refit, streamline BVH, rope links, the launch plans, and the render / stats / accumulation
// entries.  Host side of what OptixRenderer::render does through OWL/OptiX.
#include "exa_renderer.h"
#include "exa_hostbvh.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

// calibration of the wide-march assignment (assignWide), overridable for A/B builds
#ifndef EXA_WIDE_SPEED2
#define EXA_WIDE_SPEED2 1.63
#endif
#ifndef EXA_WIDE_WORK2
#define EXA_WIDE_WORK2 1.49
#endif
#ifndef EXA_WIDE_WORK4
#define EXA_WIDE_WORK4 1.88
#endif

int ExaHipRenderer::applyBrickOrder(hipStream_t s)
{
  if (brickOrderWanted == brickOrder) return 0;
  const std::vector<uint32_t> &from = brickOrder ? beginMorton : beginUploaded, &to = brickOrderWanted ? beginMorton : beginUploaded;
  HIP_TRY(this, hipStreamSynchronize(s));
  HIP_TRY(this, hipDeviceSynchronize());                 // frames in flight on other streams read the old layout
  DevBuf<uint32_t> dFrom, dTo;
  DevBuf<float> moved;
  HIP_TRY(this, dFrom.upload(from.data(), from.size()));
  HIP_TRY(this, dTo.upload(to.data(), to.size()));
  HIP_TRY(this, moved.alloc(scalars.n));
  HIP_TRY(this, launchPermuteBricks(scalars.p, moved.p, dFrom.p, dTo.p, bricks.p, numBricks, leafHdr.p, leafList.p, leafListSize,
                                    totalCells, numFields, s));
  if (leafHdrCube.p) HIP_TRY(this, launchPatchCubeRecords(leafHdrCube.p, leafList.p, leafListSize, dTo.p, cubeLog2, s));
  HIP_TRY(this, hipStreamSynchronize(s));
  std::swap(scalars.p, moved.p);                         // `moved` now owns the old array and frees it
  sc.scalars = scalars.p;
  brickOrder = brickOrderWanted;
  ilChannels = 0; cellsIl.release();                     // the interleaved copy follows the new order
  return 0;
}

// worldSpaceBounds = rcp(voxelSpaceTransform) applied to the voxel bounds (OptixRenderer.cpp:330-332);
// rcp(affine3f) = inverse of the linear part by adjoint/determinant, p' = -(L^-1 p)
void ExaHipRenderer::worldBounds(float lo[3], float hi[3]) const
{
  auto cross = [](const float *a, const float *b, float *o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; };
  float c0[3], c1[3], c2[3];
  cross(fs.xfm_vy, fs.xfm_vz, c0); cross(fs.xfm_vz, fs.xfm_vx, c1); cross(fs.xfm_vx, fs.xfm_vy, c2);
  const float det = fs.xfm_vx[0] * c0[0] + fs.xfm_vx[1] * c0[1] + fs.xfm_vx[2] * c0[2];
  const float ix[3] = { c0[0] / det, c1[0] / det, c2[0] / det }, iy[3] = { c0[1] / det, c1[1] / det, c2[1] / det },
              iz[3] = { c0[2] / det, c1[2] / det, c2[2] / det };
  float ip[3];
  for (int k = 0; k < 3; k++) ip[k] = -(fs.xfm_p[0] * ix[k] + (fs.xfm_p[1] * iy[k] + fs.xfm_p[2] * iz[k]));
  for (int k = 0; k < 3; k++) {
    lo[k] = voxLo[0] * ix[k] + (voxLo[1] * iy[k] + (voxLo[2] * iz[k] + ip[k]));
    hi[k] = voxHi[0] * ix[k] + (voxHi[1] * iy[k] + (voxHi[2] * iz[k] + ip[k]));
  }
}

int ExaHipRenderer::rebuildLayout()
{
  tilesX = (W + kTile - 1) / kTile;
  tilesY = (H + kTile - 1) / kTile;
  numBlocks = numBlocksFor();
  const size_t px = world <= 1 ? size_t(W) * H : size_t(numBlocks) * kTilePixels;
  HIP_TRY(this, accum.alloc(px));
  if (px) HIP_TRY(this, hipMemset(accum.p, 0, px * sizeof(float4)));
  HIP_TRY(this, color.alloc(px));
  surf.release(); surfRnd.release();       // allocated by the first frame that has surfaces
  std::vector<int32_t> map;
  map.reserve(numBlocks);
  for (int t = rank; t < tilesX * tilesY; t += world) map.push_back(t);
  if (tileOrder == 1 && world == 1 && tilesX % 8 == 0 && tilesY % 8 == 0 && ((tilesX / 8) * (tilesY / 8)) % 8 == 0) {
    // XCD-aware order: workgroups are dealt round-robin over the 8 XCDs, so block b
    // lands on XCD b%8.  Give each XCD whole 8x8-tile supertiles (128x128 px) so the
    // rays sharing bricks also share one L2.
    const int stx = tilesX / 8;
    for (int b = 0; b < numBlocks; b++) {
      const int xcd = b % 8, j = b / 8;
      const int super = (j / 64) * 8 + xcd, in = j % 64;
      const int sx = super % stx, sy = super / stx;
      map[b] = (sy * 8 + in / 8) * tilesX + sx * 8 + in % 8;
    }
  }
  if (tileOrder == 2) {          // fixed pseudo-random permutation (load-balance experiment)
    uint64_t st = 0x9E3779B97F4A7C15ull;
    for (size_t i = map.size(); i > 1; i--) {
      st = st * 6364136223846793005ull + 1442695040888963407ull;
      std::swap(map[i - 1], map[size_t((st >> 33) % i)]);
    }
  } else if (tileOrder == 3) {   // centre-out: tiles nearest the image centre first
    const float cx = 0.5f * tilesX, cy = 0.5f * tilesY;
    std::stable_sort(map.begin(), map.end(), [&](int32_t a, int32_t b) {
      const float ax = a % tilesX + 0.5f - cx, ay = a / tilesX + 0.5f - cy, bx = b % tilesX + 0.5f - cx, by = b / tilesX + 0.5f - cy;
      return ax * ax + ay * ay < bx * bx + by * by;
    });
  }
  if (tileOrder >= 4) {          // Z-order: tiles in flight form a compact 2-d patch of the image
    auto part = [](uint32_t v) { v &= 0xffff; v = (v | v << 8) & 0x00ff00ff; v = (v | v << 4) & 0x0f0f0f0f; v = (v | v << 2) & 0x33333333; v = (v | v << 1) & 0x55555555; return v; };
    std::stable_sort(map.begin(), map.end(), [&](int32_t a, int32_t b) {
      return (part(a % tilesX) | part(a / tilesX) << 1) < (part(b % tilesX) | part(b / tilesX) << 1);
    });
    // 5..7: deal chunks of 16/64/256 Z-consecutive tiles to the 8 XCDs (block b runs on XCD b%8)
    const int chunk = tileOrder == 5 ? 16 : (tileOrder == 6 ? 64 : (tileOrder == 7 ? 256 : 0));
    if (chunk && map.size() % size_t(8 * chunk) == 0) {
      std::vector<int32_t> z(map);
      for (size_t b = 0; b < map.size(); b++) {
        const size_t xcd = b % 8, j = b / 8;
        map[b] = z[((j / chunk) * 8 + xcd) * chunk + j % chunk];
      }
    }
  }
  HIP_TRY(this, tileMap.upload(map.data(), map.size()));
  HIP_TRY(this, tileCost.alloc(size_t(tilesX) * tilesY));
  HIP_TRY(this, tileCostPre.alloc(size_t(tilesX) * tilesY));
  nPreCheap = nPreHeavy = 0;
  baseMap = map; curMap = map;
  costPhase = 1;
  nNormal = nWide4 = nWide2 = 0;
  if (assignWide(nullptr)) return 1;
  layoutDirty = false;
  return 0;
}

// Launch-order feedback.  A frame's critical path is its longest rays (a wave runs until its
// slowest lane is done); launched late they drain alone on an empty GPU — worst on a multi-GPU
// shard, where a rank holds little more than one GPU-full of waves.  The frame after a change of
// view/TF/layout records each tile's longest wave (march iterations); from then on the heaviest
// tiles are launched first (coarse cost classes, the static order inside a class so that the
// tiles in flight still share bricks).  Pixels do not depend on the launch order.
int ExaHipRenderer::reorderFromCosts()
{
  costPhase = 0;
  const size_t n = curMap.size();
  if (n < 2) return 0;
  std::vector<uint32_t> costOfTile(size_t(tilesX) * tilesY, 0);
  HIP_TRY(this, hipMemcpy(costOfTile.data(), tileCost.p, costOfTile.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
  uint32_t maxC = 0;
  for (size_t b = 0; b < n; b++) maxC = std::max(maxC, costOfTile[curMap[b]]);
  // cost classes: heaviest first between classes, the static (Z-order) sequence inside a class, so that the tiles in
  // flight still share bricks.  Measured on C4 (EXA_COST_CLASSES = 1 / 2 / 4 / 8 / 16 / 32 / 64 / 256 / 1024 / 4096):
  // 24.29 / 24.11 / 23.36 / 22.76 / 22.56 / 22.37 / 22.33 / 22.26 / 22.30 / 22.24 ms — the frame's tail matters more than
  // the locality of the tiles in flight
  int kClasses = 256;
  if (const char *e = std::getenv("EXA_COST_CLASSES")) kClasses = std::max(1, std::min(4096, std::atoi(e)));
  std::vector<std::vector<int32_t>> cls(kClasses);
  for (size_t b = 0; b < n; b++) {
    const int32_t t = baseMap[b];
    const int c = kClasses - 1 - int(uint64_t(costOfTile[t]) * kClasses / (uint64_t(maxC) + 1));
    cls[c].push_back(t);
  }
  if (std::getenv("EXA_HIP_VERBOSE")) {
    uint64_t sum = 0;
    for (size_t b = 0; b < n; b++) sum += costOfTile[curMap[b]];
    std::fprintf(stderr, "[exa_hip] tile costs: %zu tiles, max %u iterations, sum %llu, per class (heaviest first):", n, maxC,
                 (unsigned long long)sum);
    for (int c = 0; c < kClasses; c++) std::fprintf(stderr, " %zu", cls[c].size());
    std::fprintf(stderr, "\n");
  }
  std::vector<int32_t> order;
  order.reserve(n);
  for (int c = 0; c < kClasses; c++) order.insert(order.end(), cls[c].begin(), cls[c].end());
  if (order != curMap) {
    HIP_TRY(this, hipMemcpy(tileMap.p, order.data(), n * sizeof(int32_t), hipMemcpyHostToDevice));
    curMap.swap(order);
  }
  nPreCheap = nPreHeavy = 0;
  if (preMeasured && prepassSplit) {
    std::vector<uint32_t> pre(size_t(tilesX) * tilesY, 0);
    HIP_TRY(this, hipMemcpy(pre.data(), tileCostPre.p, pre.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    uint32_t maxP = 0;
    for (size_t b = 0; b < n; b++) maxP = std::max(maxP, pre[curMap[b]]);
    // heavy: a longest iso march above 1/32 of the frame's longest (and long enough to matter at all)
    // (C3 / C5 with the threshold at max/8 | >= 64 steps: 16.81 / 1444 ms, max/32 | 16: 16.61 / 1444, every tile with any iso
    // step: 16.59 / 1444 — on C5 only 9 % of the tiles have any; profiles/r03_prepass_split_threshold.txt)
    uint32_t div = 32, minSteps = 16;
    if (const char *e = std::getenv("EXA_PREPASS_SPLIT_DIV")) div = (uint32_t)std::max(1, std::atoi(e));          // calibration runs
    if (const char *e = std::getenv("EXA_PREPASS_SPLIT_MIN")) minSteps = (uint32_t)std::max(0, std::atoi(e));
    const uint32_t thr = std::max<uint32_t>(minSteps, maxP / div);
    std::vector<int32_t> cheap, heavy;
    for (size_t b = 0; b < n; b++) (pre[curMap[b]] > thr ? heavy : cheap).push_back(curMap[b]);
    if (!heavy.empty() && !cheap.empty()) {
      // the heavy pipeline starts with its longest pre-pass rays
      std::stable_sort(heavy.begin(), heavy.end(), [&](int32_t x, int32_t y) { return pre[x] > pre[y]; });
      std::vector<int32_t> both(cheap);
      both.insert(both.end(), heavy.begin(), heavy.end());
      HIP_TRY(this, splitMap.refill(both.data(), both.size()));
      nPreCheap = (int)cheap.size(); nPreHeavy = (int)heavy.size();
    }
    if (std::getenv("EXA_HIP_VERBOSE"))
      std::fprintf(stderr, "[exa_hip] pre-pass costs: longest iso march %u steps; %d tiles in the heavy pipeline, %d in the other\n", maxP, nPreHeavy, nPreCheap);
  }
  return assignWide(&costOfTile);
}

// Which tiles march with 2 or 4 lanes per ray.  In units of one wave's march iterations on an idle
// GPU: a tile's critical path is cost / speedup(L); the time the GPU needs for everything else is
// the work (4 waves per tile, x L / speedup(L) for a wide tile) over the waves it holds, at the pace
// of a loaded GPU.  Heaviest tiles first, each gets the smallest L that brings its path below the
// fill time; on one GPU nothing qualifies, on a shard of 8 the few hundred longest tiles do.
int ExaHipRenderer::assignWide(const std::vector<uint32_t> *costOfTile)
{
  const size_t n = curMap.size();
  std::vector<int32_t> normal, w4, w2;
  const int lanesTop = 4;
  if (wideMode == 2 || wideMode == 4) {
    (wideMode >= 4 ? w4 : w2) = curMap;
  } else if (wideMode == 1 && costOfTile) {
    // Model constants: a critical tile finishes kSpeed2 (2 lanes) times sooner and costs kWork2 / kWork4
    // times the work; a loaded GPU steps a wave 1.3x slower.  Measured with the round-1 kernels (probe 6.0 -> 3.7 ->
    // 2.5 ms).  With the round-2 kernels the probe (tests/gpu_wide_probe.py) gives 4.78 -> 3.39 -> 2.52 ms (8 lanes:
    // 3.00 ms, not instantiated) and every tile of a rank forced wide costs x1.9 / x2.4 the time (tests/gpu_shard_modes.py);
    // variations of the constants around these values move the shard of 8 by +-0.2 ms (4.46 .. 4.95 ms), the set below
    // stays within 0.05 ms of the best one tried.
    // NOTE: the module owns exactly three side streams.  A fourth (tried for an 8-lane class) made two of the
    // streams that carry one frame's launches share a hardware queue, and the shard of 8 went from 4.6 to 7.0 ms.
    double kSpeed2 = EXA_WIDE_SPEED2;
    const double kWork2 = EXA_WIDE_WORK2, kLoaded = 1.3;
    double kWork4 = EXA_WIDE_WORK4;
    if (const char *e = std::getenv("EXA_WIDE_WORK_TOP")) kWork4 = std::atof(e);          // calibration runs
    if (const char *e = std::getenv("EXA_WIDE_SPEED2")) kSpeed2 = std::atof(e);
    double fill = 0;
    for (size_t b = 0; b < n; b++) fill += 4.0 * (*costOfTile)[curMap[b]];
    fill *= kLoaded / numSimdWaves;
    // curMap is ordered by descending cost class; inside a class the decision only depends on the tile's own cost
    for (size_t b = 0; b < n; b++) {
      const int32_t t = curMap[b];
      const double c = (*costOfTile)[t];
      int L = 1;
      if (c > fill) L = (c / kSpeed2 > fill) ? 4 : 2;
      if (L == 1) { normal.push_back(t); continue; }
      fill += 4.0 * c * ((L == 4 ? kWork4 : kWork2) - 1.0) * kLoaded / numSimdWaves;
      (L == 4 ? w4 : w2).push_back(t);
    }
  } else {
    normal = curMap;
  }
  {
    // leaf lists: 16 B x kWideSegCap per window walker = 8 KiB per lane; keep them within 8 GiB by handing the
    // lightest wide tiles back to the one-lane march (forced modes on large frames)
    const size_t perTile4 = size_t(kTilePixels) * segsPerRay(lanesTop) * sizeof(float4), perTile2 = size_t(kTilePixels) * segsPerRay(2) * sizeof(float4);
    const size_t budget = size_t(std::getenv("EXA_WIDE_BUDGET_GB") ? std::atoi(std::getenv("EXA_WIDE_BUDGET_GB")) : 8) << 30;
    while (w4.size() * perTile4 + w2.size() * perTile2 > budget) {
      if (!w2.empty()) { normal.push_back(w2.back()); w2.pop_back(); }
      else { normal.push_back(w4.back()); w4.pop_back(); }
    }
  }
  if (w4.empty() && w2.empty()) { nNormal = (int)n; nWide4 = nWide2 = 0; return 0; }
  std::vector<int32_t> wide(w4);
  wide.insert(wide.end(), w2.begin(), w2.end());
  {
    const size_t need = (w4.size() * segsPerRay(lanesTop) + w2.size() * segsPerRay(2)) * size_t(kTilePixels);
    if (need > wideSegs.n && wideSegs.alloc(need) != hipSuccess) {
      // no room for the leaf lists: the frame simply keeps the one-lane march
      (void)hipGetLastError();
      wideSegs.release();
      nNormal = (int)n; nWide4 = nWide2 = 0;
      return 0;
    }
  }
  HIP_TRY(this, normalMap.refill(normal.data(), normal.size()));
  HIP_TRY(this, wideMap.refill(wide.data(), wide.size()));
  nNormal = (int)normal.size(); nWide4 = (int)w4.size(); nWide2 = (int)w2.size();
  lanesTopInUse = lanesTop;
  if (std::getenv("EXA_HIP_VERBOSE"))
    std::fprintf(stderr, "[exa_hip] wide march: %d tiles x%d lanes, %d x2, %d one lane per ray\n", nWide4, lanesTop, nWide2, nNormal);
  return 0;
}

int ExaHipRenderer::kdRefit(const uint8_t *active, int which, hipStream_t s)
{
  for (size_t h = 0; h + 1 < kdLevelBegin.size(); h++)
    HIP_TRY(this, launchKdRefit(kdNodes.p, kdMarchNodes.p, kdLevelIds.p + kdLevelBegin[h], kdLevelBegin[h + 1] - kdLevelBegin[h],
                                active, which, s));
  return 0;
}

int ExaHipRenderer::ensureLbvh()
{
  if (lbvhBuilt) return 0;
  const size_t nr = domain.n / 6;
  levelRanges.clear();
  const auto tBuild0 = std::chrono::steady_clock::now();
  if (nr < 2 || lbvhOnHost) {
    std::vector<float> boxes(domain.n);
    HIP_TRY(this, hipMemcpy(boxes.data(), domain.p, domain.n * sizeof(float), hipMemcpyDeviceToHost));
    LbvhTopology topo;
    topo.build(boxes.data(), nr);
    boxes.clear(); boxes.shrink_to_fit();
    const size_t ni = topo.child0.size();
    std::vector<BvhNode> tmpl(ni);
    for (size_t i = 0; i < ni; i++) {
      BvhNode &n = tmpl[i];
      n.q0 = make_float4(FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX);
      n.q1 = make_float4(-FLT_MAX, -FLT_MAX, FLT_MAX, FLT_MAX);
      n.q2 = make_float4(FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX);
      n.child0 = topo.child0[i]; n.child1 = topo.child1[i]; n.pad0 = n.pad1 = 0;
    }
    HIP_TRY(this, topoNodes.upload(tmpl.data(), ni));
    std::vector<int32_t> ids;
    std::vector<int> begin;
    orderByHeight(topo.height, ids, begin);
    for (size_t hh = 1; hh < begin.size(); hh++) levelRanges.push_back({ begin[hh - 1], begin[hh] - begin[hh - 1] });   // by height, leaves' parents first
    HIP_TRY(this, levelIds.upload(ids.data(), ids.size()));
    sc.numInternal = (uint32_t)ni;
  } else {
    const size_t ni = nr - 1;
    HIP_TRY(this, topoNodes.alloc(ni));
    HIP_TRY(this, levelIds.alloc(ni));
    std::vector<uint32_t> perDepth;
    HIP_TRY(this, buildLbvhTopologyDevice(domain.p, (uint32_t)nr, topoNodes.p, levelIds.p, perDepth, nullptr));
    int at = 0;
    std::vector<std::pair<int, int>> byDepth;
    for (uint32_t c : perDepth) { byDepth.push_back({ at, (int)c }); at += (int)c; }
    levelRanges.assign(byDepth.rbegin(), byDepth.rend());            // deepest level first
    sc.numInternal = (uint32_t)ni;
  }
  HIP_TRY(this, volNodes.alloc(topoNodes.n));
  HIP_TRY(this, hipMemcpy(volNodes.p, topoNodes.p, topoNodes.n * sizeof(BvhNode), hipMemcpyDeviceToDevice));
  lbvhBuilt = true;
  volDirty = isoDirty = true;          // boxes of both LBVHs come from the next refit
  if (std::getenv("EXA_HIP_VERBOSE")) {
    (void)hipDeviceSynchronize();
    std::fprintf(stderr, "[exa_hip] LBVH over %zu regions built on the %s in %.1f ms (%zu refit launches)\n", nr,
                 (nr < 2 || lbvhOnHost) ? "host" : "device",
                 std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tBuild0).count(), levelRanges.size());
  }
  return 0;
}

int ExaHipRenderer::refit(DevBuf<BvhNode> &nodes, const uint8_t *active, hipStream_t s)
{
  for (const auto &r : levelRanges)
    HIP_TRY(this, launchRefit(nodes.p, levelIds.p + r.first, r.second, domain.p, active, s));
  return 0;
}

int ExaHipRenderer::prepareFrame(hipStream_t s)
{
  if (!haveFs || !haveParams) { fail("exa_hip_render: frame state / params not set"); return 1; }
  if (W <= 0 || H <= 0) { fail("exa_hip_render: framebuffer not sized"); return 1; }
  if (p.numPrimaryChannels < 1 || p.numPrimaryChannels > numFields || p.numChannels > numFields
      || p.colormapChannel < 0 || p.colormapChannel >= numFields) {
    fail("exa_hip_render: channel counts exceed the scene's scalar fields"); return 1;
  }
  if (layoutDirty && rebuildLayout()) return 1;
  if (xfDirty) {
    HIP_TRY(this, hipMemcpyAsync(xf.p, xfHost, sizeof(xfHost), hipMemcpyHostToDevice, s));
    xfDirty = false;
  }
  if (needLbvh() && ensureLbvh()) return 1;
  if (applyBrickOrder(s)) return 1;
  {
    int want = (useKd() && interleave && !emptyCells && p.numPrimaryChannels >= 2 && p.numPrimaryChannels <= 4) ? p.numPrimaryChannels : 0;
    if (want == ilNoMemory) want = 0;                    // this many channels did not fit before: field by field
    if (want != ilChannels) {
      HIP_TRY(this, hipStreamSynchronize(s));            // frames in flight may still read the old copy
      cellsIl.release();
      ilChannels = 0;
      if (want && cellsIl.alloc(size_t(totalCells) * want + 2 * size_t(want)) != hipSuccess) {      // a pair load may reach one cell past the end
        // the copy is an optimisation (want x one field of extra memory): without it the march reads the fields one after
        // the other, same pixels
        (void)hipGetLastError();
        cellsIl.release();
        if (std::getenv("EXA_HIP_VERBOSE"))
          std::fprintf(stderr, "[exa_hip] no memory for the channel-interleaved copy of %d fields: field-by-field march\n", want);
        ilNoMemory = want;
        want = 0;
      }
      if (want) {
        HIP_TRY(this, hipMemsetAsync(cellsIl.p + size_t(totalCells) * want, 0, 2 * size_t(want) * sizeof(float), s));
        HIP_TRY(this, launchInterleave(sc, totalCells, want, cellsIl.p, s));
        ilChannels = want;
      }
    }
  }
  const bool needIso = isoEnabled();
  if (volDirty || (needIso && isoDirty)) {
    HIP_TRY(this, hipEventRecord(ev2, s));
    const bool volChanged = volDirty;
    if (volDirty) {                       // needVolumeBVHRebuild (OptixRenderer.cpp:533-537)
      HIP_TRY(this, launchVolumeActivity(sc, fs, p, xf.p, volActive.p, tfFracMagic(), s));
      if (lbvhBuilt && refit(volNodes, volActive.p, s)) return 1;
      if (haveKd && kdRefit(volActive.p, 0, s)) return 1;
      volDirty = false;
    }
    if (needIso && isoDirty) {            // needIsoBVHRebuild (OptixRenderer.cpp:539-543)
      if (lbvhBuilt && !isoNodes.p && topoNodes.n) {
        HIP_TRY(this, isoNodes.alloc(topoNodes.n));
        HIP_TRY(this, hipMemcpyAsync(isoNodes.p, topoNodes.p, topoNodes.n * sizeof(BvhNode), hipMemcpyDeviceToDevice, s));
      }
      HIP_TRY(this, launchIsoActivity(sc, fs, isoActive.p, s));
      if (lbvhBuilt && refit(isoNodes, isoActive.p, s)) return 1;
      if (haveKd && kdRefit(isoActive.p, 1, s)) return 1;
      isoDirty = false;
    }
    if (haveKd && volChanged) {
      // how many regions the volume march finds active: what the automatic choice of the walk looks at
      if (!activeCountBuf.p) HIP_TRY(this, activeCountBuf.alloc(1));
      HIP_TRY(this, hipMemsetAsync(activeCountBuf.p, 0, sizeof(uint32_t), s));
      HIP_TRY(this, launchRopeActivity(ropeBuilt ? ropeLeaves.p : nullptr, sc.numRegions, volActive.p, 0, activeCountBuf.p, s));
      ropeFlagsStale = !ropeBuilt;
    }
    HIP_TRY(this, hipEventRecord(ev1, s));
    HIP_TRY(this, hipEventSynchronize(ev1));
    HIP_TRY(this, hipEventElapsedTime(&last.rebuild_ms, ev2, ev1));
    if (haveKd && volChanged) HIP_TRY(this, hipMemcpy(&activeRegions, activeCountBuf.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (haveKd && kdRoot < 0 && kdRoot != EXA_KD_EMPTY) {        // the kd tree is a single leaf: its activity lives here
      uint8_t f[2] = {1, 1};
      HIP_TRY(this, hipMemcpy(&f[0], volActive.p + ~kdRoot, 1, hipMemcpyDeviceToHost));
      if (needIso) HIP_TRY(this, hipMemcpy(&f[1], isoActive.p + ~kdRoot, 1, hipMemcpyDeviceToHost));
      rootLeafVolActive = f[0] != 0;
      rootLeafIsoActive = f[1] != 0;
    }
  }
  // which walk this frame's DVR march takes
  const bool ropeBefore = ropeThisFrame;
  ropeThisFrame = ropeWanted();
  if (ropeThisFrame != ropeBefore && std::getenv("EXA_HIP_VERBOSE"))
    std::fprintf(stderr, "[exa_hip] %u of %u regions active for the volume march: %s walk (option walk = %d)\n", activeRegions, sc.numRegions,
                 ropeThisFrame ? "rope" : "stack", walkMode);
  if (ropeThisFrame && !ropeBuilt) {
    HIP_TRY(this, hipStreamSynchronize(s));
    if (buildRopes()) return 1;
    ropeThisFrame = ropeBuilt;
  }
  if (ropeThisFrame && ropeFlagsStale) {
    HIP_TRY(this, launchRopeActivity(ropeLeaves.p, sc.numRegions, volActive.p, 0, nullptr, s));
    ropeFlagsStale = false;
  }
  return 0;
}

// needStreamlineBVHRebuild (OptixRenderer.cpp:545-549): BVH over the segments the Streamline bounds
// program leaves visible (exabrick.cu:541-570), built on the host from the current traces
int ExaHipRenderer::rebuildStreamlines(hipStream_t s)
{
  streamDirty = false;
  numStreamPrims = 0;
  if (!haveTracer) return 0;
  const int NT = tracer.numTimesteps;
  const long long nprims = (long long)tracer.numTraces * (NT - 1);
  // the device copy of the timestep stops at numTimesteps (advanceTracer uploads it only while <= numTimesteps)
  const int timestep = std::min(this->timestep, NT);
  if (timestep < 2 || nprims <= 0) return 0;
  HIP_TRY(this, hipStreamSynchronize(s));
  std::vector<float> host(traces.n);
  HIP_TRY(this, hipMemcpy(host.data(), traces.p, traces.n * sizeof(float), hipMemcpyDeviceToHost));
  std::vector<float> boxes;
  std::vector<int32_t> prim;
  for (long long p = 0; p < nprims; p++) {
    if (int(p % NT) >= timestep - 1) continue;
    const float *pa = &host[3 * p], *pb = &host[3 * (p + 1)];
    if (!(pa[0] < 2e10f && pb[0] < 2e10f)) continue;
    for (int k = 0; k < 3; k++) boxes.push_back(std::fmin(pa[k] - 2.f, pb[k] - 2.f));
    for (int k = 0; k < 3; k++) boxes.push_back(std::fmax(pa[k] + 2.f, pb[k] + 2.f));
    prim.push_back((int32_t)p);
  }
  if (prim.empty()) return 0;
  LbvhTopology topo;
  topo.build(boxes.data(), prim.size());
  const std::vector<BvhNode> nodes = fillBoxes(topo, boxes, [&](size_t i) { return prim[i]; });   // leaf = flat segment index
  HIP_TRY(this, streamNodes.upload(nodes.data(), nodes.size()));
  numStreamPrims = (int)prim.size();
  return 0;
}

// ---- a frame's launches ----
// What every kernel of the frame takes (RenderArgs), from the renderer's state; clears the buffers the instrumented and
// the cost-measuring frame count into.
int ExaHipRenderer::fillRenderArgs(RenderArgs &a, uint32_t *dstDevice, bool stats, hipStream_t s)
{
  a.sc = sc;
  a.volNodes = volNodes.p;
  a.isoNodes = isoNodes.p;
  a.fs = fs;
  a.p = p;
  a.xf = xf.p;
  a.tfFracMagic = tfFracMagic();
  a.fastSampler = fastSampler;
  a.mul24 = mul24; a.addr32 = addr64 ? 0 : addr32;
  a.cellsIl = ilChannels == p.numPrimaryChannels ? cellsIl.p : nullptr;
  a.il32 = (uint64_t(totalCells) + 2) * uint64_t(ilChannels > 0 ? ilChannels : 1) * sizeof(float) <= (1ull << 32) && !addr64 ? 1 : 0;
  {
    // launch.dt a power of two (the reference's default 0.5 is): 1/dt is exact and x/dt == x*(1/dt)
    int e = 0;
    const float mant = std::frexp(p.dt, &e);
    a.invDtPow2 = (mant == 0.5f && e > -100 && e < 100) ? 1.f / p.dt : 0.f;
  }
  a.numXfChannels = numFields;
  a.W = W; a.H = H; a.tilesX = tilesX; a.tilesY = tilesY;
  a.rank = rank; a.world = world;
  a.tileMap = tileMap.p;
  a.color = dstDevice;
  a.colorRowMajor = colorRowMajor ? 1 : 0;
  a.accum = accum.p;
  a.surf = surf.p;
  a.surfRnd = surfRnd.p;
  a.stats = statsBuf.p;
  a.errorFlag = errorFlag.p;
  a.debugPixel = debugPixel;
  a.walkProbe = nullptr;
  if (stats && statsMode == 1 && walkProbeOn && useKd()) {
    const size_t need = size_t(numBlocks) * (256 / 64) * kWalkProbeSize;
    if (walkProbe.n != need) HIP_TRY(this, walkProbe.alloc(need));
    HIP_TRY(this, hipMemsetAsync(walkProbe.p, 0, need * sizeof(uint32_t), s));
    a.walkProbe = walkProbe.p;
  }
  a.tileCost = nullptr;
  a.tileCostPre = nullptr;
  if (feedback && costPhase == 1 && useKd() && measureCosts) {
    HIP_TRY(this, hipMemsetAsync(tileCost.p, 0, tileCost.n * sizeof(uint32_t), s));
    a.tileCost = tileCost.p;
    preMeasured = surfacesEnabled();
    if (preMeasured) {
      HIP_TRY(this, hipMemsetAsync(tileCostPre.p, 0, tileCostPre.n * sizeof(uint32_t), s));
      a.tileCostPre = tileCostPre.p;
    }
  }
  a.kdNodes = kdNodes.p;
  // the instrumented counters re-check every leaf against its region record, so they walk the tree with region ids
  const bool packed = packRecords && kdMarchNodes.p != nullptr && !(stats && statsMode == 1);
  a.kdMarchNodes = packed ? kdMarchNodes.p : kdNodes.p;
  a.kdMarchRoot = packed ? kdMarchRoot : kdRoot;
  // A tree that is one leaf (a one-region scene) has no node to carry the activity bits: the walks start at
  // "done" when that region is inactive (the reference's BVHs hold no primitive then)
  if (!rootLeafVolActive) a.kdMarchRoot = EXA_KD_EMPTY + 1;
  a.leafBeginBits = packed ? leafBeginBits : 0;
  a.leafSizeBits = packed ? leafSizeBits : 0;
  a.regionRec = regionRec.p;
  // cube scene: the one-channel 32-bit rope march may read the cube records (launchRenderKdT decides)
  a.leafHdrCube = (cubeRecords && cubeLog2) ? leafHdrCube.p : nullptr;
  a.cubeLog2 = cubeLog2;
  a.ropeLeaves = (ropeThisFrame && ropeBuilt) ? ropeLeaves.p : nullptr;
  a.ropeNodes = ropeNodes.p;
  a.ropeRoot = ropeRoot;
  a.ropeFastDiv = ropeFastDiv;
  a.ropeAddr32 = addr64 ? 0 : ropeAddr32;
  a.kdRoot = kdRoot;
  a.kdIsoRoot = rootLeafIsoActive ? kdRoot : EXA_KD_EMPTY + 1;
  for (int k = 0; k < 3; k++) { a.kdLo[k] = kdLo[k]; a.kdHi[k] = kdHi[k]; }
  worldBounds(a.worldLo, a.worldHi);
  a.meshNodes = meshNodes.p; a.meshVerts = meshVerts.p; a.meshTris = meshTris.p; a.numTris = numTris;
  a.streamNodes = streamNodes.p; a.traces = traces.p; a.numStreamPrims = numStreamPrims;
  for (int k = 0; k < 3; k++) a.tracerChannels[k] = tracer.channels[k];
  a.numTraces = tracer.numTraces; a.numTimesteps = tracer.numTimesteps; a.timestep = std::min(timestep, tracer.numTimesteps); a.steplen = tracer.steplen;
  return 0;
}

// The surfaces' buffers, allocated by the first frame that has surfaces, and the lists of the deferred AO rays
int ExaHipRenderer::prepareSurfaceLists(RenderArgs &a, bool stats, hipStream_t s)
{
  if (useKd() && surfacesEnabled() && surf.n != accum.n) {
    HIP_TRY(this, surf.alloc(accum.n));
    HIP_TRY(this, surfRnd.alloc(accum.n));
    a.surf = surf.p; a.surfRnd = surfRnd.p;
  }
  a.aoRecs = nullptr; a.aoCount = nullptr; a.aoKeys = nullptr; a.aoHist = nullptr; a.aoOrder = nullptr; a.aoHit = nullptr; a.aoBins = 0;
  if (!(useKd() && surfacesEnabled() && fs.ao.enabled && aoDefer && !stats)) return 0;
  // one record per pixel of every launched tile, the padding pixels of partial edge tiles included: the heavy
  // pipeline's list starts behind nPreCheap WHOLE tiles (accum.n = W * H on one GPU is smaller when W or H is not a
  // multiple of the tile)
  const size_t recs = size_t(numBlocks) * kTilePixels;
  if (aoRecs.n != recs && aoRecs.alloc(recs) != hipSuccess) {
    // the list is an optimisation (64 B per pixel): without it the AO rays are traced inline behind each pixel's primary ray
    (void)hipGetLastError();
    aoRecs.release();
    if (std::getenv("EXA_HIP_VERBOSE")) std::fprintf(stderr, "[exa_hip] no memory for the list of deferred AO rays (%zu records): traced inline\n", recs);
    return 0;
  }
  if (!aoCount.p) HIP_TRY(this, aoCount.alloc(8));        // per pipeline: [0] listed hits, [2] the AO kernel's chunk counter
  HIP_TRY(this, hipMemsetAsync(aoCount.p, 0, 8 * sizeof(uint32_t), s));
  a.aoRecs = aoRecs.p; a.aoCount = aoCount.p;
  if (aoDefer == 2) {
    // bins: (32x32-pixel blocks of the frame, or groups of four of this shard's tiles) x 24 direction classes
    const uint32_t cells = world <= 1 ? uint32_t((W + 31) / 32) * uint32_t((H + 31) / 32) : uint32_t((numBlocks + 3) / 4);
    const uint32_t bins = std::max(1u, cells) * 24u;
    if (aoKeys.n != 2 * recs) { HIP_TRY(this, aoKeys.alloc(2 * recs)); HIP_TRY(this, aoOrder.alloc(2 * recs)); HIP_TRY(this, aoHit.alloc(2 * recs)); }
    if (aoBins != bins) { HIP_TRY(this, aoHist.alloc(2 * size_t(bins))); aoBins = bins; }
    a.aoKeys = aoKeys.p; a.aoOrder = aoOrder.p; a.aoHit = aoHit.p; a.aoHist = aoHist.p; a.aoBins = bins;
  }
  return 0;
}

// the one-lane DVR march on the walk chosen for this frame
hipError_t ExaHipRenderer::march(const RenderArgs &a, int n, bool surfArg, int statsArg, hipStream_t s)
{
  return (ropeThisFrame && ropeBuilt) ? EXA_FORM(this, launchRenderKdRope)(a, n, p.gradientShadingDVR != 0, fastMath != 0, surfArg, statsArg, s)
                                      : EXA_FORM(this, launchRenderKd)(a, n, p.gradientShadingDVR != 0, fastMath != 0, surfArg, statsArg, s);
}

// the surfaces pre-pass of the whole frame and, unless the frame counts, its deferred AO rays behind it
int ExaHipRenderer::launchSurfaces(const RenderArgs &a, bool surfOn, bool stats, hipStream_t s)
{
  if (surfOn) HIP_TRY(this, EXA_FORM(this, launchSurfacePrepassKd)(a, numBlocks, stats, s));
  if (surfOn && !stats) HIP_TRY(this, EXA_FORM(this, launchAoRaysKd)(a, numBlocks, s));
  return 0;
}

// plain plan: everything on the caller's stream
int ExaHipRenderer::launchPlain(const RenderArgs &a, bool surfOn, bool stats, hipStream_t s)
{
  if (launchSurfaces(a, surfOn, stats, s)) return 1;
  HIP_TRY(this, march(a, numBlocks, surfOn, stats ? statsMode : 0, s));
  return 0;
}

// pre-pass split: two pipelines side by side (see prepassSplit), pre-pass + march of the heavy tiles, pre-pass + march of
// the rest; with `overlap` the AO rays of both beside their marches (see aoOverlap)
int ExaHipRenderer::launchSplit(const RenderArgs &a, bool overlap, hipStream_t s)
{
  HIP_TRY(this, hipEventRecord(evFork, s));
  RenderArgs ah = a, ac = a;
  ac.tileMap = splitMap.p;
  ah.tileMap = splitMap.p + nPreCheap;
  if (a.aoRecs) {                                   // each pipeline appends to its own list
    ah.aoRecs = a.aoRecs + size_t(nPreCheap) * kTilePixels;
    ah.aoCount = a.aoCount + 4;
    if (a.aoKeys) {
      const size_t off = 2 * size_t(nPreCheap) * kTilePixels;
      ah.aoKeys = a.aoKeys + off; ah.aoOrder = a.aoOrder + off; ah.aoHit = a.aoHit + off; ah.aoHist = a.aoHist + a.aoBins;
    }
  }
  HIP_TRY(this, hipStreamWaitEvent(side2, evFork, 0));
  HIP_TRY(this, EXA_FORM(this, launchSurfacePrepassKd)(ah, nPreHeavy, false, side2));
  HIP_TRY(this, hipStreamWaitEvent(sideN, evFork, 0));
  HIP_TRY(this, EXA_FORM(this, launchSurfacePrepassKd)(ac, nPreCheap, false, sideN));
  if (overlap) {
    // both pipelines' AO rays on the third side stream, each behind its pre-pass; the marches start at once
    HIP_TRY(this, hipEventRecord(evPre2, side2));
    HIP_TRY(this, hipEventRecord(evPre, sideN));
    HIP_TRY(this, hipStreamWaitEvent(side4, evPre2, 0));
    HIP_TRY(this, EXA_FORM(this, launchAoRaysKd)(ah, nPreHeavy, side4));
    HIP_TRY(this, hipEventRecord(evAo2, side4));
    HIP_TRY(this, hipStreamWaitEvent(side4, evPre, 0));
    HIP_TRY(this, EXA_FORM(this, launchAoRaysKd)(ac, nPreCheap, side4));
    HIP_TRY(this, hipEventRecord(evAo, side4));
  } else {
    HIP_TRY(this, EXA_FORM(this, launchAoRaysKd)(ah, nPreHeavy, side2));
    HIP_TRY(this, EXA_FORM(this, launchAoRaysKd)(ac, nPreCheap, sideN));
  }
  HIP_TRY(this, march(ac, nPreCheap, true, 0, sideN));
  if (overlap) {
    HIP_TRY(this, hipStreamWaitEvent(sideN, evAo, 0));
    HIP_TRY(this, EXA_FORM(this, launchCompositeKd)(ac, nPreCheap, sideN));
  }
  HIP_TRY(this, hipEventRecord(evJoinN, sideN));
  HIP_TRY(this, march(ah, nPreHeavy, true, 0, side2));
  if (overlap) {
    HIP_TRY(this, hipStreamWaitEvent(side2, evAo2, 0));
    HIP_TRY(this, EXA_FORM(this, launchCompositeKd)(ah, nPreHeavy, side2));
  }
  HIP_TRY(this, hipEventRecord(evJoin2, side2));
  HIP_TRY(this, hipStreamWaitEvent(s, evJoin2, 0));
  HIP_TRY(this, hipStreamWaitEvent(s, evJoinN, 0));
  return 0;
}

// AO overlap on an unsplit frame: the deferred AO rays on a side stream beside the march, then the finishing pass
int ExaHipRenderer::launchOverlap(const RenderArgs &a, hipStream_t s)
{
  HIP_TRY(this, EXA_FORM(this, launchSurfacePrepassKd)(a, numBlocks, false, s));
  HIP_TRY(this, hipEventRecord(evPre, s));
  HIP_TRY(this, hipStreamWaitEvent(side4, evPre, 0));
  HIP_TRY(this, EXA_FORM(this, launchAoRaysKd)(a, numBlocks, side4));
  HIP_TRY(this, hipEventRecord(evAo, side4));
  HIP_TRY(this, march(a, numBlocks, true, 0, s));
  HIP_TRY(this, hipStreamWaitEvent(s, evAo, 0));
  HIP_TRY(this, EXA_FORM(this, launchCompositeKd)(a, numBlocks, s));
  return 0;
}

// wide plan: the critical tiles on side streams so that they start together with the rest of the frame
int ExaHipRenderer::launchWide(const RenderArgs &a, bool surfOn, hipStream_t s)
{
  if (launchSurfaces(a, surfOn, false, s)) return 1;
  HIP_TRY(this, hipEventRecord(evFork, s));
  RenderArgs aw = a;
  if (nWide4) {
    HIP_TRY(this, hipStreamWaitEvent(side4, evFork, 0));
    aw.wideTileMap = wideMap.p;
    aw.wideSegs = wideSegs.p;
    HIP_TRY(this, EXA_FORM(this, launchRenderKdWide)(aw, nWide4, lanesTopInUse, p.gradientShadingDVR != 0, fastMath != 0, surfOn, side4));
    HIP_TRY(this, hipEventRecord(evJoin4, side4));
  }
  if (nWide2) {
    HIP_TRY(this, hipStreamWaitEvent(side2, evFork, 0));
    aw.wideTileMap = wideMap.p + nWide4;
    aw.wideSegs = wideSegs.p + size_t(nWide4) * segsPerRay(lanesTopInUse) * kTilePixels;
    HIP_TRY(this, EXA_FORM(this, launchRenderKdWide)(aw, nWide2, 2, p.gradientShadingDVR != 0, fastMath != 0, surfOn, side2));
    HIP_TRY(this, hipEventRecord(evJoin2, side2));
  }
  // the rest of the frame on a stream of its own as well: launched on the caller's stream it would not
  // overlap the side streams when that stream is the (synchronising) null stream
  RenderArgs an = a;
  an.tileMap = normalMap.p;
  HIP_TRY(this, hipStreamWaitEvent(sideN, evFork, 0));
  HIP_TRY(this, march(an, nNormal, surfOn, 0, sideN));
  HIP_TRY(this, hipEventRecord(evJoinN, sideN));
  if (nWide4) HIP_TRY(this, hipStreamWaitEvent(s, evJoin4, 0));
  if (nWide2) HIP_TRY(this, hipStreamWaitEvent(s, evJoin2, 0));
  HIP_TRY(this, hipStreamWaitEvent(s, evJoinN, 0));
  return 0;
}

int ExaHipRenderer::launch(uint32_t *dstDevice, bool stats, hipStream_t s)
{
  if (streamDirty && rebuildStreamlines(s)) return 1;
  RenderArgs a{};
  if (fillRenderArgs(a, dstDevice, stats, s)) return 1;
  if (haveTracer && tracer.enabled && timestep < tracer.numTimesteps && timestep >= 1) {
    // computeTraces: the threads with pixelIdx < numTraces (exabrick.cu:1539)
    const long long px = (long long)W * H;
    HIP_TRY(this, EXA_FORM(this, launchComputeTraces)(a, traces.p, (int)std::min<long long>(tracer.numTraces, px), s));
  }
  if (prepareSurfaceLists(a, stats, s)) return 1;
  HIP_TRY(this, hipEventRecord(ev0, s));
  if (useKd()) {
    const bool surfOn = surfacesEnabled();
    const bool wide = !stats && !emptyCells && nWide4 + nWide2 > 0 && p.numPrimaryChannels == 1 && a.debugPixel < 0;
    const bool split = surfOn && !stats && !wide && costPhase == 0 && !a.tileCost && nPreHeavy > 0 && nPreCheap > 0
                       && nPreHeavy + nPreCheap == numBlocks && a.debugPixel < 0;
    // the deferred AO rays beside the march (see aoOverlap); the viewer's clock heat map times the march kernel itself and
    // keeps the plain sequence
    const bool overlap = aoOverlap && a.aoRecs && fs.ao.enabled && !wide && !(fs.clockScale > 0.f);
    if (overlap) {
      if (pixBuf.n != accum.n) HIP_TRY(this, pixBuf.alloc(accum.n));
      a.pixOut = pixBuf.p;
    }
    if (split) { if (launchSplit(a, overlap, s)) return 1; }
    else if (overlap) { if (launchOverlap(a, s)) return 1; }
    else if (wide) { if (launchWide(a, surfOn, s)) return 1; }
    else if (launchPlain(a, surfOn, stats, s)) return 1;
  } else {
    HIP_TRY(this, EXA_FORM(this, launchRender)(a, numBlocks, p.gradientShadingDVR != 0, surfacesEnabled(), stats, s));
  }
  last.node_bytes = useKd() ? sizeof(KdNodeDev) : sizeof(BvhNode);
  HIP_TRY(this, hipEventRecord(ev1, s));
  return 0;
}

// Leaves and neighbour links of the rope walk (exa_ropes.h), from the region kd-tree and the regions' domains as the device
// holds them; this adds what the march needs of a region (its packed record) and uploads the result.
int ExaHipRenderer::buildRopes()
{
  const auto tBuild0 = std::chrono::steady_clock::now();
  const size_t nk = kdNodes.n, nr = sc.numRegions;
  static_assert(sizeof(KdNodeDev) == sizeof(ExaKdNode), "the device's kd node is the ABI's with activity bits in the axis word");
  std::vector<ExaKdNode> kd(nk);
  std::vector<float> dom(6 * nr);
  std::vector<RegionInfo> ri(nr);
  if (nk) HIP_TRY(this, hipMemcpy(kd.data(), kdNodes.p, nk * sizeof(KdNodeDev), hipMemcpyDeviceToHost));
  HIP_TRY(this, hipMemcpy(dom.data(), domain.p, dom.size() * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(this, hipMemcpy(ri.data(), regionInfo.p, nr * sizeof(RegionInfo), hipMemcpyDeviceToHost));
  const unsigned nthreads = std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
  RopeBuild rb;
  buildRopesHost(kd.data(), nk, kdRoot, dom.data(), nr, kdLo, kdHi, nthreads, rb);
  if (rb.leaves.size() >= 0x7ffffff0ull) { ropeFailed = true; return 0; }
  if (!rb.boxesMatch) {
    // a tree whose planes do not reproduce the regions' domains (a caller's own kd-tree): the stack walk stays
    if (std::getenv("EXA_HIP_VERBOSE")) std::fprintf(stderr, "[exa_hip] rope walk: the kd-tree's planes do not reproduce the region domains; stack walk kept\n");
    ropeFailed = true;
    return 0;
  }
  std::vector<RopeLeaf> leaves(rb.leaves.size());
  const uint32_t bb = leafBeginBits, sb = leafSizeBits;
  for (size_t id = 0; id < leaves.size(); id++) {
    const RopeLeafHost &H = rb.leaves[id];
    RopeLeaf &L = leaves[id];
    L.lo[0] = H.lo[0]; L.lo[1] = H.lo[1]; L.lo[2] = H.lo[2];
    L.hi0 = H.hi[0]; L.hi1 = H.hi[1]; L.hi2 = H.hi[2];
    for (int f = 0; f < 6; f++) L.rope[f] = H.rope[f];
    L.flags = 0; L.pad = 0;
    L.region = H.region;
    L.rec = H.region >= 0 ? (uint32_t)H.region : 0u;
    if (H.region >= 0 && bb) L.rec = packLeafRec(ri[id].listBegin, ri[id].listSize, ri[id].finestLevelCellWidth, bb, sb);
  }
  static_assert(sizeof(ExaKdNode) == 16, "kd node = one 16-byte load");
  if (ropeLeaves.upload(leaves.data(), leaves.size()) != hipSuccess
      || ropeNodes.upload(reinterpret_cast<const KdNodeDev *>(rb.nodes.data()), rb.nodes.size()) != hipSuccess) {
    // the links are an optimisation (64 B per leaf + 16 B per node of extra memory): without them the stack walk
    (void)hipGetLastError();
    ropeLeaves.release(); ropeNodes.release();
    ropeFailed = true;
    return 0;
  }
  ropeRoot = kdRoot;
  ropeFastDiv = rb.planesOnGrid ? 1 : 0;
  ropeAddr32 = (leaves.size() * sizeof(RopeLeaf) < (1ull << 32) && rb.nodes.size() * sizeof(KdNodeDev) < (1ull << 32)) ? 1 : 0;
  ropeBuilt = true;
  ropeFlagsStale = true;
  if (std::getenv("EXA_HIP_VERBOSE"))
    std::fprintf(stderr, "[exa_hip] rope walk: %zu leaves (%zu gaps), %zu nodes linked on %u threads in %.1f ms; short division %s\n", leaves.size(), rb.gaps,
                 rb.nodes.size(), nthreads, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tBuild0).count(), rb.planesOnGrid ? "on" : "off");
  return 0;
}

int checkLoopGuard(ExaHipRenderer *h, ExaHipRenderer *r, const char *fn, const char *what)
{
  int32_t flag = 0;
  HIP_TRY(h, hipMemcpy(&flag, r->errorFlag.p, sizeof(flag), hipMemcpyDeviceToHost));
  if (flag) {
    (void)hipMemset(r->errorFlag.p, 0, sizeof(int32_t));
    h->fail(std::string(fn) + what);
    return 3;
  }
  return 0;
}

static const char *const kMarchGuard = ": a ray-march loop guard tripped (step size too small for the ray length?)";

// the work counters of r's instrumented frame (statsBuf) added to `st`: every field of ExaHipStats but node_bytes, pixels
// and the two times
static int addCounters(ExaHipRenderer *h, ExaHipRenderer *r, ExaHipStats &st)
{
  unsigned long long k[ST_COUNT];
  HIP_TRY(h, hipMemcpy(k, r->statsBuf.p, sizeof(k), hipMemcpyDeviceToHost));
  st.segments += k[ST_SEGMENTS]; st.sample_evals += k[ST_SAMPLE_EVALS]; st.samples += k[ST_SAMPLES];
  st.brick_visits += k[ST_BRICK_VISITS]; st.corner_loads += k[ST_CORNER_LOADS];
  st.iso_segments += k[ST_ISO_SEGMENTS]; st.iso_evals += k[ST_ISO_EVALS]; st.nodes_visited += k[ST_NODES];
  for (int i = 0; i < 9; i++) st.diag[i] += k[ST_W_BRICK + i];
  for (int i = 0; i < 5; i++) st.phase_cycles[i] += k[ST_T_BRICK + i];
  st.walk_restarts += k[ST_RESTARTS]; st.walk_union_nodes += k[ST_UNION]; st.walk_probe_overflow += k[ST_PROBE_OVERFLOW];
  st.wave_iters += k[ST_WAVE_ITERS]; st.tile_iters += k[ST_TILE_ITERS]; st.walk_leaf_visits += k[ST_ROPE_LEAVES];
  return 0;
}

// A frame of a multi-device handle: every device marches its tiles into the same destination frame on its own stream;
// the caller's stream waits for all of them (async) or the host does (synchronous).
static int renderMulti(ExaHipRenderer *h, uint32_t *rgba8, int32_t dstIsDevice, hipStream_t s, bool async, bool stats)
{
  if (h->W <= 0) { h->fail("exa_hip_render: framebuffer not sized"); return 1; }
  uint32_t *dst = dstIsDevice && rgba8 ? rgba8 : h->color.p;
  const bool willSync = !(async && dstIsDevice && !stats);
  {
    EXA_ON_DEVICE(h);
    HIP_TRY(h, hipEventRecord(h->evCall, s));           // what the caller queued before (e.g. the copy-out of this buffer)
  }
  for (ExaHipRenderer *c : h->children) {
    DeviceGuard g(c->device);
    if (g.err != hipSuccess) { h->fail("hipSetDevice failed"); return 1; }
    HIP_TRY(h, hipStreamWaitEvent(c->ownStream, h->evCall, 0));
    if (c->prepareFrame(c->ownStream)) { h->fail(c->err); return 1; }
    if (stats) HIP_TRY(h, hipMemsetAsync(c->statsBuf.p, 0, ST_COUNT * sizeof(unsigned long long), c->ownStream));
    c->measureCosts = willSync && !stats;
    if (c->launch(dst, stats, c->ownStream)) { h->fail(c->err); return 1; }
  }
  if (!willSync) {
    EXA_ON_DEVICE(h);
    for (ExaHipRenderer *c : h->children) HIP_TRY(h, hipStreamWaitEvent(s, c->ev1, 0));
    return 0;
  }
  // a frame without counters keeps those of the last counted frame, as a single-device handle does
  ExaHipStats sum = stats ? ExaHipStats{} : h->last;
  sum.kernel_ms = sum.rebuild_ms = 0.f;
  for (ExaHipRenderer *c : h->children) {
    DeviceGuard g(c->device);
    HIP_TRY(h, hipEventSynchronize(c->ev1));
    HIP_TRY(h, hipEventElapsedTime(&c->last.kernel_ms, c->ev0, c->ev1));
    if (c->measureCosts && c->feedback && c->costPhase == 1 && c->useKd() && c->reorderFromCosts()) { h->fail(c->err); return 1; }
    if (int rc = checkLoopGuard(h, c, "exa_hip_render", kMarchGuard)) return rc;
    sum.kernel_ms = std::max(sum.kernel_ms, c->last.kernel_ms);
    sum.rebuild_ms = std::max(sum.rebuild_ms, c->last.rebuild_ms);
    sum.node_bytes = c->last.node_bytes;
    if (stats && addCounters(h, c, sum)) return 1;
  }
  sum.pixels = uint64_t(h->W) * h->H;
  h->last = sum;
  if (!dstIsDevice && rgba8) {
    EXA_ON_DEVICE(h);
    HIP_TRY(h, hipMemcpy(rgba8, h->color.p, size_t(h->W) * h->H * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  return 0;
}

static int renderImpl(ExaHipRenderer *h, uint32_t *rgba8, int32_t dstIsDevice, hipStream_t s, bool async, bool stats)
{
  if (!h) return 1;
  if (!h->children.empty()) return renderMulti(h, rgba8, dstIsDevice, s, async, stats);
  EXA_ON_DEVICE(h);
  if (h->prepareFrame(s)) return 1;
  uint32_t *dst = dstIsDevice && rgba8 ? rgba8 : h->color.p;
  if (stats) HIP_TRY(h, hipMemsetAsync(h->statsBuf.p, 0, ST_COUNT * sizeof(unsigned long long), s));
  const bool willSync = !(async && dstIsDevice && !stats);
  h->measureCosts = willSync && !stats;
  if (h->launch(dst, stats, s)) return 1;
  if (!willSync) return 0;
  HIP_TRY(h, hipEventSynchronize(h->ev1));
  HIP_TRY(h, hipEventElapsedTime(&h->last.kernel_ms, h->ev0, h->ev1));
  if (h->measureCosts && h->feedback && h->costPhase == 1 && h->useKd() && h->reorderFromCosts()) return 1;
  const size_t px = (size_t)exa_hip_output_pixels(h);
  if (!dstIsDevice && rgba8) HIP_TRY(h, hipMemcpy(rgba8, h->color.p, px * sizeof(uint32_t), hipMemcpyDeviceToHost));
  if (int rc = checkLoopGuard(h, h, "exa_hip_render", kMarchGuard)) return rc;
  if (stats) {
    ExaHipStats counted{};
    if (addCounters(h, h, counted)) return 1;
    counted.node_bytes = h->last.node_bytes; counted.kernel_ms = h->last.kernel_ms; counted.rebuild_ms = h->last.rebuild_ms;
    h->last = counted;
    h->walkProbe.release();
  }
  h->last.pixels = px;
  return 0;
}

// row-major frame <-> the tile-major shards of a multi-device handle's children (host side)
static int multiAccum(ExaHipRenderer *h, float *frame4, bool read)
{
  const int n = (int)h->children.size(), W = h->W, H = h->H;
  const int tilesX = (W + kTile - 1) / kTile, tilesY = (H + kTile - 1) / kTile;
  for (int i = 0; i < n; i++) {
    ExaHipRenderer *c = h->children[i];
    if (c->accum.n == 0) continue;                 // more devices than tiles: this one owns nothing
    std::vector<float> shard(c->accum.n * 4);
    if (exa_hip_read_accum(c, shard.data())) { h->fail(c->err); return 1; }   // a write keeps the padding pixels of ragged tiles
    for (int t = i; t < tilesX * tilesY; t += n) {
      const int tx = t % tilesX, ty = t / tilesX;
      for (int y = 0; y < kTile && ty * kTile + y < H; y++)
        for (int x = 0; x < kTile && tx * kTile + x < W; x++) {
          float *f = frame4 + 4 * (size_t(tx * kTile + x) + size_t(W) * (ty * kTile + y));
          float *s = shard.data() + 4 * (size_t(t / n) * kTilePixels + size_t(y) * kTile + x);
          for (int k = 0; k < 4; k++) { if (read) f[k] = s[k]; else s[k] = f[k]; }
        }
    }
    if (!read && exa_hip_write_accum(c, shard.data())) { h->fail(c->err); return 1; }
  }
  return 0;
}

extern "C" {

uint64_t exa_hip_output_pixels(const ExaHipRenderer *h)
{
  if (!h || h->W <= 0) return 0;
  if (!h->children.empty()) return uint64_t(h->W) * h->H;
  return h->world <= 1 ? uint64_t(h->W) * h->H : h->outputPixels();
}

int exa_hip_render(ExaHipRenderer *h, uint32_t *rgba8, int32_t dstIsDevice, void *hipStream, int32_t async)
{ return renderImpl(h, rgba8, dstIsDevice, (hipStream_t)hipStream, async != 0, false); }

int exa_hip_render_stats(ExaHipRenderer *h, uint32_t *rgba8, int32_t dstIsDevice, ExaHipStats *out)
{
  const int rc = renderImpl(h, rgba8, dstIsDevice, nullptr, false, true);
  if (rc == 0 && out) *out = h->last;
  return rc;
}

int exa_hip_get_stats(ExaHipRenderer *h, ExaHipStats *out)
{
  if (!h || !out) return 1;
  if (!h->children.empty()) {                  // kernel time of the slowest device (refreshed if an async frame has completed)
    float ms = 0.f;
    for (ExaHipRenderer *c : h->children) { ExaHipStats s; exa_hip_get_stats(c, &s); ms = std::max(ms, s.kernel_ms); }
    h->last.kernel_ms = ms;
    *out = h->last;
    return 0;
  }
  // refresh the kernel time of an async launch if it has completed
  if (h->ev0 && hipEventQuery(h->ev1) == hipSuccess) (void)hipEventElapsedTime(&h->last.kernel_ms, h->ev0, h->ev1);
  *out = h->last;
  return 0;
}

int exa_hip_untile(ExaHipRenderer *h, const uint32_t *gathered, uint64_t shardStridePixels,
                   int32_t worldSize, uint32_t *rgba8_out, void *hipStream)
{
  if (!h || !gathered || !rgba8_out || worldSize < 1) return 1;
  EXA_ON_DEVICE(h);
  HIP_TRY(h, launchUntile(gathered, shardStridePixels, worldSize, h->W, h->H, rgba8_out, (hipStream_t)hipStream));
  return 0;
}

int exa_hip_read_accum(ExaHipRenderer *h, float *dst4)
{
  if (!h || !dst4) return 1;
  if (!h->children.empty()) return multiAccum(h, dst4, true);
  EXA_ON_DEVICE(h);
  HIP_TRY(h, hipMemcpy(dst4, h->accum.p, h->accum.n * sizeof(float4), hipMemcpyDeviceToHost));
  return 0;
}

int exa_hip_write_accum(ExaHipRenderer *h, const float *src4)
{
  if (!h || !src4) return 1;
  if (!h->children.empty()) return multiAccum(h, const_cast<float *>(src4), false);
  EXA_ON_DEVICE(h);
  HIP_TRY(h, hipMemcpy(h->accum.p, src4, h->accum.n * sizeof(float4), hipMemcpyHostToDevice));
  return 0;
}

} // extern "C"
