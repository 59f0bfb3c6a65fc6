// exa_create.cpp — exa_hip_create / _create_multi / _destroy: scene validation, the tables derived from the scene
// (brick orders, march headers, address forms, kd level order, packed march tree) and their upload.  Host side of what
// the constructor of exa/OptixRenderer.cpp does through OWL/OptiX; see include/exa_hip.h for the per-entry citations.
#include "exa_renderer.h"
#include "exa_hostbvh.h"
#include "exa_coords.h"
#include "exa_cube.h"

#include <cmath>
#include <cstdlib>
#include <cstring>

thread_local std::string g_createError;

namespace {

// The renderer's events and side streams, created and destroyed through these tables.  ev0..ev2 time a frame's launches
// and the activity + refit pass; the others only order streams.
struct EventSlot { hipEvent_t ExaHipRenderer::*ev; bool timing; };
const EventSlot kEvents[] = {
  { &ExaHipRenderer::ev0, true },      { &ExaHipRenderer::ev1, true },      { &ExaHipRenderer::ev2, true },
  { &ExaHipRenderer::evFork, false },  { &ExaHipRenderer::evJoin4, false }, { &ExaHipRenderer::evJoin2, false },
  { &ExaHipRenderer::evJoinN, false }, { &ExaHipRenderer::evPre, false },   { &ExaHipRenderer::evPre2, false },
  { &ExaHipRenderer::evAo, false },    { &ExaHipRenderer::evAo2, false },
};
hipStream_t ExaHipRenderer::*const kSideStreams[] = { &ExaHipRenderer::side4, &ExaHipRenderer::side2, &ExaHipRenderer::sideN };

uint64_t volumeOf(const ExaBrick &B) { return uint64_t(B.size[0]) * uint64_t(B.size[1]) * uint64_t(B.size[2]); }

// Brick orders: as uploaded, and along a Morton curve of the brick centres (21 bits per axis over the voxel bounds;
// equal codes keep the uploaded order), with a running `begin` as the reference assigns it (OptixRenderer.cpp:71-93)
void buildBrickOrders(ExaHipRenderer *h, const ExaHipScene *scene)
{
  const uint64_t nb = scene->numBricks;
  h->beginUploaded.resize(nb);
  std::vector<std::pair<uint64_t, uint32_t>> keyed(nb);
  for (uint64_t b = 0; b < nb; b++) {
    const ExaBrick &B = scene->bricks[b];
    h->beginUploaded[b] = B.begin;
    double c[3];
    for (int k = 0; k < 3; k++) {
      const double cw = double(1u << B.level);
      c[k] = double(B.lower[k]) + 0.5 * cw * double(B.size[k]);
    }
    keyed[b] = { mortonKey(c, scene->voxelBounds_lo, scene->voxelBounds_hi), uint32_t(b) };
  }
  std::sort(keyed.begin(), keyed.end());
  h->beginMorton.resize(nb);
  uint64_t at = 0;
  for (uint64_t i = 0; i < nb; i++) {
    h->beginMorton[keyed[i].second] = uint32_t(at);
    at += volumeOf(scene->bricks[keyed[i].second]);
  }
  // The permutation moves field f at f * totalCells and brick b's cells as one block [begin, begin + volume): it needs the
  // layout the reference's constructor produces (OptixRenderer.cpp:71-110) — channel offsets f * totalCells and the
  // uploaded begins a partition of [0, totalCells) into the bricks' volumes.  Anything else keeps the uploaded order.
  bool partition = at == scene->totalCells;
  for (int f = 0; f < scene->numFields && partition; f++) partition = scene->channelOffset[f] == uint64_t(f) * scene->totalCells;
  if (partition) {
    std::vector<std::pair<uint32_t, uint64_t>> spans(nb);                  // (begin, volume), sorted by begin
    for (uint64_t b = 0; b < nb; b++) spans[b] = { scene->bricks[b].begin, volumeOf(scene->bricks[b]) };
    std::sort(spans.begin(), spans.end());
    uint64_t run = 0;
    for (uint64_t b = 0; b < nb && partition; b++) { partition = spans[b].first == run; run += spans[b].second; }
  }
  h->brickOrderPossible = partition;
  if (!partition) h->beginMorton = h->beginUploaded;
  if (const char *e = std::getenv("EXA_BRICK_ORDER")) h->brickOrderWanted = std::atoi(e) != 0 && h->brickOrderPossible;
}

// March headers along the leaf list (the kd march reads the record at listBegin + child, no id indirection).
// What a brick visit needs, ready to use — float(lower) (the conversion the reference's
// `vec3f(brick.lower)` performs, exabrick.cu:623), 2^-level, the sizes and the first cell's offset
std::vector<ExaBrick> buildMarchHeaders(const ExaHipScene *scene)
{
  std::vector<ExaBrick> hdr(scene->leafListSize);
  for (uint64_t i = 0; i < scene->leafListSize; i++) {
    const ExaBrick &B = scene->bricks[scene->leafList[i]];
    const float lowerF[3] = { float(B.lower[0]), float(B.lower[1]), float(B.lower[2]) };
    const float invCw = std::ldexp(1.f, -B.level);
    ExaBrick &o = hdr[i];
    std::memcpy(&o.lower[0], lowerF, sizeof(lowerF));
    std::memcpy(&o.size[0], &invCw, sizeof(float));
    o.size[1] = B.size[0]; o.size[2] = B.size[1]; o.level = B.size[2]; o.begin = B.begin;
  }
  return hdr;
}

// 24-bit multiplies in the cell address need every factor below 2^24 and every product below 2^32; 32-bit byte
// offsets need a field below 4 GiB (the pair load reads one float past a row's last cell at most)
void chooseAddressForms(ExaHipRenderer *h, const ExaHipScene *scene)
{
  h->mul24 = 1;
  for (uint64_t b = 0; b < scene->numBricks; b++) {
    const ExaBrick &B = scene->bricks[b];
    if (uint64_t(B.size[0]) * uint64_t(B.size[1]) >= (1ull << 24) || B.size[0] >= (1 << 24) || B.size[1] >= (1 << 24) || B.size[2] >= (1 << 24))
      h->mul24 = 0;
  }
  if (scene->totalCells >= (1ull << 32)) h->mul24 = 0;
  h->addr32 = ((scene->totalCells + 2) * sizeof(float) <= (1ull << 32)              // cell scalars of one field
               && scene->leafListSize * 32ull < (1ull << 32)                          // march headers
               && scene->numKdNodes * sizeof(KdNodeDev) < (1ull << 32)) ? 1 : 0;      // kd nodes
}

bool kdTreeWellFormed(const ExaHipScene *scene)
{
  const uint64_t nk = scene->numKdNodes;
  auto refOk = [&](int32_t ref) {
    if (ref == EXA_KD_EMPTY) return true;
    return ref >= 0 ? uint64_t(ref) < nk : uint64_t(~ref) < scene->numRegions;
  };
  bool ok = refOk(scene->kdRoot) && scene->kdRoot != EXA_KD_EMPTY && nk < 0x7fffffffull;
  for (uint64_t i = 0; ok && i < nk; i++) {
    const ExaKdNode &n = scene->kdNodes[i];
    // children must come later in the array (preorder), which also rules out cycles
    ok = n.axis >= 0 && n.axis <= 2 && refOk(n.left) && refOk(n.right)
         && (n.left < 0 || uint64_t(n.left) > i) && (n.right < 0 || uint64_t(n.right) > i);
  }
  return ok;
}

// the kd nodes by height, for the refit of their activity bits level by level (kdRefit)
void buildKdLevelOrder(const ExaHipScene *scene, std::vector<int32_t> &ids, std::vector<int> &levelBegin)
{
  const uint64_t nk = scene->numKdNodes;
  std::vector<int32_t> kh(nk, 1);
  for (uint64_t ii = nk; ii-- > 0;) {            // children have larger indices: one backward sweep
    const ExaKdNode &n = scene->kdNodes[ii];
    int hh = 0;
    if (n.left >= 0) hh = std::max(hh, kh[n.left]);
    if (n.right >= 0) hh = std::max(hh, kh[n.right]);
    kh[ii] = hh + 1;
  }
  orderByHeight(kh, ids, levelBegin);
}

// March tree: the same nodes with every leaf reference replaced by the region's record
// {listBegin | listSize-1 | log2(finestLevelCellWidth)}, when the scene's ranges fit 31 bits, so that a segment
// start needs no region-info load (one dependent HBM/L2 round trip less per segment).  False: no such tree (the
// march then takes region ids); mk, root, bb and sb are set otherwise.
bool buildMarchTree(const ExaHipScene *scene, const std::vector<KdNodeDev> &kd, std::vector<KdNodeDev> &mk, int32_t &root,
                    uint32_t &bb, uint32_t &sb)
{
  auto bitsFor = [](uint64_t maxValue) { uint32_t b = 0; while (b < 63 && (1ull << b) <= maxValue) b++; return b; };
  uint64_t maxSize = 1; int maxLevel = 0; bool pow2 = true;
  for (uint64_t r = 0; r < scene->numRegions; r++) {
    const ExaBrickRegion &R = scene->regions[r];
    maxSize = std::max<uint64_t>(maxSize, (uint64_t)R.leafListSize);
    const int lv = levelOfWidth(R.finestLevelCellWidth);
    if (float(1 << lv) != R.finestLevelCellWidth) pow2 = false;
    maxLevel = std::max(maxLevel, lv);
  }
  bb = std::max(1u, bitsFor(scene->leafListSize ? scene->leafListSize - 1 : 0));
  sb = bitsFor(maxSize - 1);
  const uint32_t lb = bitsFor((uint64_t)maxLevel);
  if (!pow2 || bb + sb + lb > 31) return false;
  auto pack = [&](int32_t ref) -> int32_t {
    if (ref >= 0 || ref == EXA_KD_EMPTY) return ref;
    const ExaBrickRegion &R = scene->regions[~ref];
    return ~int32_t(packLeafRec(R.leafListBegin, R.leafListSize, R.finestLevelCellWidth, bb, sb));
  };
  mk = kd;
  bool clash = false;
  for (auto &n : mk) {
    n.left = pack(n.left); n.right = pack(n.right);
    // ~d must not collide with the walk's two sentinels (INT32_MIN, INT32_MIN + 1)
    clash = clash || (n.left < 0 && n.left != EXA_KD_EMPTY && n.left <= INT32_MIN + 1) || (n.right < 0 && n.right != EXA_KD_EMPTY && n.right <= INT32_MIN + 1);
  }
  root = pack(scene->kdRoot);
  clash = clash || (root < 0 && root <= INT32_MIN + 1);
  if (clash) return false;
  if (mk.empty()) mk.resize(1);              // single-region scene: the root is the leaf
  return true;
}

} // namespace

extern "C" {

int exa_hip_create(const ExaHipScene *scene, int32_t device, ExaHipRenderer **out)
{
  if (!out || !scene) { g_createError = "exa_hip_create: null argument"; return 1; }
  *out = nullptr;
  if (scene->allowEmptyCells != 0 && scene->allowEmptyCells != 1) {
    g_createError = "exa_hip_create: ExaHipScene.allowEmptyCells is 0 or 1 (was the struct zero-initialised before it was filled?)";
    return 1;
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    g_createError = std::string("exa_hip_create: no HIP device available (") + hipGetErrorString(e)
                  + "); this module has no CPU fallback";
    return 2;
  }
  if (device < 0 || device >= ndev) { g_createError = "exa_hip_create: bad device index"; return 1; }
  if (scene->numFields < 1 || scene->numFields > EXA_MAX_CHANNELS) { g_createError = "exa_hip_create: 1..10 scalar fields required"; return 1; }
  if (scene->numRegions == 0 || scene->numBricks == 0) { g_createError = "exa_hip_create: empty scene"; return 1; }
  if (scene->numRegions > 0x7fffffffull) { g_createError = "exa_hip_create: too many regions"; return 1; }
  ExaHipRenderer *h = new ExaHipRenderer;
  h->device = device;
  auto bail = [&]() { g_createError = h->err; delete h; return 1; };
#define CREATE_TRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { h->fail(std::string(#call) + ": " + hipGetErrorString(e_)); return bail(); } } while (0)
  DeviceGuard guard_(device);
  CREATE_TRY(guard_.err);

  // validate indices on the host before anything can fault on the device
  for (uint64_t i = 0; i < scene->leafListSize; i++)
    if (scene->leafList[i] < 0 || uint64_t(scene->leafList[i]) >= scene->numBricks) { h->fail("exa_hip_create: leaf list entry out of range"); return bail(); }
  for (uint64_t b = 0; b < scene->numBricks; b++) {
    const ExaBrick &B = scene->bricks[b];
    if (B.size[0] <= 0 || B.size[1] <= 0 || B.size[2] <= 0 || B.level < 0 || B.level > 30
        || uint64_t(B.begin) + volumeOf(B) > scene->totalCells) { h->fail("exa_hip_create: brick record out of range"); return bail(); }
    int axis = 0;
    double plane = 0.0;
    // (next to the kd-tree's check below: a table that does not describe the scene is refused, not rendered)
    if (!exa::brickPlanesAreFloats(B, &axis, &plane)) { h->fail(exa::brickPlaneMessage("exa_hip_create", b, B, axis, plane)); return bail(); }
  }
  for (int f = 0; f < scene->numFields; f++)
    if (scene->channelOffset[f] + scene->totalCells > uint64_t(scene->numFields) * scene->totalCells) { h->fail("exa_hip_create: channel offset out of range"); return bail(); }

  h->numFields = scene->numFields;
  h->emptyCells = scene->allowEmptyCells != 0;
  if (h->emptyCells) h->basisForm = 0;
  h->totalCells = scene->totalCells;
  h->numBricks = scene->numBricks; h->leafListSize = scene->leafListSize;
  buildBrickOrders(h, scene);
  if (const char *e = std::getenv("EXA_BASIS_FORM")) h->basisForm = std::atoi(e) != 0 && !h->emptyCells;    // initial value of option basis_form
  for (int k = 0; k < 3; k++) { h->voxLo[k] = scene->voxelBounds_lo[k]; h->voxHi[k] = scene->voxelBounds_hi[k]; }
  static_assert(sizeof(ExaBrick) == 2 * sizeof(int4), "brick = two int4");
  CREATE_TRY(h->bricks.upload(reinterpret_cast<const int4 *>(scene->bricks), scene->numBricks * 2));
  CREATE_TRY(h->leafList.upload(scene->leafList, scene->leafListSize));
  {
    const std::vector<ExaBrick> hdr = buildMarchHeaders(scene);
    CREATE_TRY(h->leafHdr.upload(reinterpret_cast<const int4 *>(hdr.data()), hdr.size() * 2));
  }
  chooseAddressForms(h, scene);
  CREATE_TRY(h->scalars.upload(scene->scalars, size_t(scene->numFields) * scene->totalCells));
  // cube records beside the march headers, where the scene has only cubes of one power-of-two edge: 16 B per leaf-list
  // entry (half the headers' size, so below 4 GiB wherever the 32-bit march runs).  They are an optimisation: without the
  // memory for them the scene renders from the march headers.
  h->cubeLog2 = exa::cubeSceneLog2(scene->bricks, scene->numBricks, h->beginMorton.data());
  if (h->cubeLog2) {
    std::vector<int32_t> rec(scene->leafListSize * 4);
    exa::buildCubeRecords(scene->bricks, scene->leafList, scene->leafListSize, h->cubeLog2, rec.data());
    if (h->leafHdrCube.upload(reinterpret_cast<const int4 *>(rec.data()), scene->leafListSize) != hipSuccess) {
      (void)hipGetLastError();
      h->leafHdrCube.release();
      h->cubeLog2 = 0;
    }
  }
  std::vector<RegionInfo> ri(scene->numRegions);
  std::vector<float2> vr(scene->numRegions);
  std::vector<float> dom(scene->numRegions * 6);
  for (uint64_t r = 0; r < scene->numRegions; r++) {
    const ExaBrickRegion &R = scene->regions[r];
    if (R.leafListSize < 1 || R.leafListBegin < 0 || uint64_t(R.leafListBegin) + uint64_t(R.leafListSize) > scene->leafListSize) {
      h->fail("exa_hip_create: region leaf list out of range"); return bail();
    }
    // finestLevelCellWidth = 2^(min level) (exa/Regions.cpp:293-299): the kernels rely on an integer-valued width >= 1
    // and on a power of two (the reference only ever writes 1 << finestLevel): the march forms 1/(dt*width) from the
    // width's exponent bits
    {
      int ex = 0;
      const float mant = std::frexp(R.finestLevelCellWidth, &ex);
      if (!(R.finestLevelCellWidth >= 1.f && R.finestLevelCellWidth <= 1073741824.f) || mant != 0.5f) {
        h->fail("exa_hip_create: region finestLevelCellWidth is not a power of two >= 1"); return bail();
      }
    }
    ri[r].listBegin = R.leafListBegin;
    ri[r].listSize = R.leafListSize;
    ri[r].finestLevelCellWidth = R.finestLevelCellWidth;
    ri[r].firstBrick = scene->leafList[R.leafListBegin];
    vr[r] = make_float2(R.valueRange_lo, R.valueRange_hi);
    for (int k = 0; k < 3; k++) { dom[6 * r + k] = R.domain_lo[k]; dom[6 * r + 3 + k] = R.domain_hi[k]; }
  }
  CREATE_TRY(h->regionInfo.upload(ri.data(), ri.size()));
  CREATE_TRY(h->valueRange.upload(vr.data(), vr.size()));
  CREATE_TRY(h->domain.upload(dom.data(), dom.size()));

  // ---- optional region kd-tree: validate, order by height for the refit, upload ----
  for (int k = 0; k < 3; k++) { h->kdLo[k] = INFINITY; h->kdHi[k] = -INFINITY; }
  for (uint64_t r = 0; r < scene->numRegions; r++)
    for (int k = 0; k < 3; k++) {
      h->kdLo[k] = std::fmin(h->kdLo[k], scene->regions[r].domain_lo[k]);
      h->kdHi[k] = std::fmax(h->kdHi[k], scene->regions[r].domain_hi[k]);
    }
  if (scene->kdNodes != nullptr || (scene->numKdNodes == 0 && scene->numRegions == 1 && scene->kdRoot == ~int32_t(0))) {
    const uint64_t nk = scene->numKdNodes;
    if (!kdTreeWellFormed(scene)) { h->fail("exa_hip_create: malformed kd-tree"); return bail(); }
    std::vector<int32_t> kids;
    buildKdLevelOrder(scene, kids, h->kdLevelBegin);
    std::vector<KdNodeDev> kd(nk);
    for (uint64_t i = 0; i < nk; i++) {
      kd[i].split = scene->kdNodes[i].split;
      kd[i].word = (uint32_t)scene->kdNodes[i].axis;
      kd[i].left = scene->kdNodes[i].left;
      kd[i].right = scene->kdNodes[i].right;
    }
    std::vector<RegionRec> rec(scene->numRegions);
    for (uint64_t r = 0; r < scene->numRegions; r++) {
      const ExaBrickRegion &R = scene->regions[r];
      RegionRec &q = rec[r];
      q.lo[0] = R.domain_lo[0]; q.lo[1] = R.domain_lo[1]; q.lo[2] = R.domain_lo[2];
      q.hi0 = R.domain_hi[0]; q.hi1 = R.domain_hi[1]; q.hi2 = R.domain_hi[2];
      q.finestLevelCellWidth = R.finestLevelCellWidth;
      q.firstBrick = scene->leafList[R.leafListBegin];
      q.listBegin = R.leafListBegin; q.listSize = R.leafListSize; q.pad0 = q.pad1 = 0;
    }
    CREATE_TRY(h->kdNodes.upload(kd.data(), kd.size()));
    {
      std::vector<KdNodeDev> mk;
      int32_t root = 0;
      uint32_t bb = 0, sb = 0;
      if (buildMarchTree(scene, kd, mk, root, bb, sb)) {
        CREATE_TRY(h->kdMarchNodes.upload(mk.data(), mk.size()));
        h->kdMarchRoot = root;
        h->leafBeginBits = bb; h->leafSizeBits = sb;
      }
    }
    CREATE_TRY(h->kdLevelIds.upload(kids.data(), kids.size()));
    CREATE_TRY(h->regionRec.upload(rec.data(), rec.size()));
    h->kdRoot = scene->kdRoot;
    h->haveKd = true;
  }
  CREATE_TRY(h->volActive.alloc(scene->numRegions));
  CREATE_TRY(h->isoActive.alloc(scene->numRegions));
  CREATE_TRY(h->xf.alloc(size_t(EXA_MAX_CHANNELS) * EXA_NUM_XF_VALUES));
  std::memset(h->xfHost, 0, sizeof(h->xfHost));
  CREATE_TRY(h->statsBuf.alloc(ST_COUNT));
  CREATE_TRY(h->errorFlag.alloc(1));
  CREATE_TRY(hipMemset(h->errorFlag.p, 0, sizeof(int32_t)));
  for (const EventSlot &slot : kEvents)
    CREATE_TRY(hipEventCreateWithFlags(&(h->*slot.ev), slot.timing ? hipEventDefault : hipEventDisableTiming));
  for (auto stream : kSideStreams) CREATE_TRY(hipStreamCreateWithFlags(&(h->*stream), hipStreamNonBlocking));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
      h->numSimdWaves = prop.multiProcessorCount * 4 * 6;
  }

  h->sc.bricks = h->bricks.p;
  h->sc.leafList = h->leafList.p;
  h->sc.leafHdr = h->leafHdr.p;
  h->sc.scalars = h->scalars.p;
  h->sc.regionInfo = h->regionInfo.p;
  h->sc.valueRange = h->valueRange.p;
  h->sc.domain = h->domain.p;
  for (int f = 0; f < EXA_MAX_CHANNELS; f++) h->sc.channelOffset[f] = f < scene->numFields ? scene->channelOffset[f] : 0;
  h->sc.numRegions = (uint32_t)scene->numRegions;
  h->sc.numInternal = 0;                     // set when the LBVH is built (ensureLbvh)
#undef CREATE_TRY
  *out = h;
  return 0;
}

// One handle, several devices: the scene is replicated, device i renders the 16x16 tiles t with t % n == i and stores
// them straight into the destination frame on the first device of the list (peer-mapped when it is another device), so
// there is no gather and no untile step.  Entries of `devices` may repeat (several renderers sharing one GPU: rehearsal).
int exa_hip_create_multi(const ExaHipScene *scene, const int32_t *devices, int32_t numDevices, ExaHipRenderer **out)
{
  if (!out || !scene || !devices || numDevices < 1 || numDevices > 64) { g_createError = "exa_hip_create_multi: bad arguments"; return 1; }
  *out = nullptr;
  ExaHipRenderer *h = new ExaHipRenderer;
  h->device = devices[0];
  auto bail = [&](const std::string &msg) { g_createError = msg; exa_hip_destroy(h); return 1; };
  for (int i = 0; i < numDevices; i++) {
    ExaHipRenderer *c = nullptr;
    if (int rc = exa_hip_create(scene, devices[i], &c)) { exa_hip_destroy(h); return rc; }    // g_createError is set
    h->children.push_back(c);
    c->colorRowMajor = true;
    c->rank = i; c->world = numDevices; c->layoutDirty = true;
    DeviceGuard g(devices[i]);
    if (g.err != hipSuccess || hipStreamCreateWithFlags(&c->ownStream, hipStreamNonBlocking) != hipSuccess)
      return bail("exa_hip_create_multi: cannot create a stream on device " + std::to_string(devices[i]));
    if (devices[i] != devices[0]) {
      int can = 0;
      if (hipDeviceCanAccessPeer(&can, devices[i], devices[0]) != hipSuccess || !can)
        return bail("exa_hip_create_multi: device " + std::to_string(devices[i]) + " cannot access device " + std::to_string(devices[0]));
      const hipError_t e = hipDeviceEnablePeerAccess(devices[0], 0);
      if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return bail(std::string("hipDeviceEnablePeerAccess: ") + hipGetErrorString(e));
      (void)hipGetLastError();
    }
  }
  {
    DeviceGuard g(devices[0]);
    if (g.err != hipSuccess || hipEventCreateWithFlags(&h->evCall, hipEventDisableTiming) != hipSuccess) return bail("exa_hip_create_multi: hipEventCreate failed");
  }
  h->numFields = h->children[0]->numFields;
  *out = h;
  return 0;
}

int exa_hip_destroy(ExaHipRenderer *h)
{
  if (!h) return 0;
  for (ExaHipRenderer *c : h->children) exa_hip_destroy(c);
  h->children.clear();
  DeviceGuard guard_(h->device);
  if (h->ownStream) (void)hipStreamDestroy(h->ownStream);
  if (h->evCall) (void)hipEventDestroy(h->evCall);
  (void)hipDeviceSynchronize();
  for (const EventSlot &slot : kEvents) if (h->*slot.ev) (void)hipEventDestroy(h->*slot.ev);
  for (auto stream : kSideStreams) if (h->*stream) (void)hipStreamDestroy(h->*stream);
  delete h;
  return 0;
}

} // extern "C"
