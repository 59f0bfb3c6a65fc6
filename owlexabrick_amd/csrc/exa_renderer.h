// exa_renderer.h — internal to the exa_hip_* module (not installed): the renderer behind the opaque ExaHipRenderer handle
// of include/exa_hip.h and the helpers its translation units share.  exa_create.cpp builds and destroys a renderer,
// exa_frame.cpp prepares and launches a frame, exa_probe.cpp holds the point probes, the projections along rays and the
// iso-surface extraction, exa_streamlines.cpp the streamline extraction and, on its evaluation, the line integral
// convolution and the flow map, exa_stats.cpp the histogram and value range of
// the cells, exa_module.cpp the setters, options and read-backs.  What the calls outside a frame keep on the handle is
// one struct per call (ExaHipRenderer::probes, isoMesh, isolines, isoRegions, isoCritical, isoBasins, hist, lines, project, surface); TimingEvents, DropUnlessCommitted and the
// argument checks below the renderer are what their host code shares.
#pragma once
#include "exa_device.h"
#include "exa_ropes.h"

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

using namespace exa;

// the launchers of the sampling kernels exist once per association of the basis sums (exa_device.h); r: the renderer
#define EXA_FORM(r, fn) ((r)->emptyCells ? form0e::fn : ((r)->basisForm ? form1::fn : form0::fn))

#define HIP_TRY(h, call)                                                                   \
  do {                                                                                     \
    hipError_t e_ = (call);                                                                \
    if (e_ != hipSuccess) {                                                                \
      (h)->fail(std::string(#call) + ": " + hipGetErrorString(e_));                        \
      return 1;                                                                            \
    }                                                                                      \
  } while (0)

// what exa_hip_last_error(nullptr) reports: the failure of the calling thread's last create (defined in exa_create.cpp)
extern thread_local std::string g_createError;

// The ABI calls run on the handle's device and leave the caller's current device as they found it.
struct DeviceGuard {
  int prev = -1;
  hipError_t err;
  explicit DeviceGuard(int device)
  {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    err = hipSetDevice(device);
  }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define EXA_ON_DEVICE(h) EXA_ON_DEVICE_OF(h, h)
// ... on the device of r, a failure reported by h (r: the renderer of a multi-device handle h that runs the call)
#define EXA_ON_DEVICE_OF(h, r) DeviceGuard guard_((r)->device); HIP_TRY(h, guard_.err)

template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  // a failed allocation leaves the buffer empty, {nullptr, 0, 0}: a guard `if (buf.n < need)` asks again the next time
  hipError_t alloc(size_t count)
  {
    release();
    if (count == 0) return hipSuccess;
    // 16 spare bytes: the pair load of a one-cell-wide row reads one float past the last brick
    const hipError_t e = hipMalloc((void **)&p, count * sizeof(T) + 16);
    if (e == hipSuccess) n = count; else p = nullptr;
    return e;
  }
  hipError_t upload(const T *src, size_t count)
  {
    hipError_t e = alloc(count);
    if (e != hipSuccess || count == 0) return e;
    return hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
  }
  // like upload, but keeps the allocation when it is large enough (per-frame tables)
  hipError_t refill(const T *src, size_t count)
  {
    if (count > cap || !p) {
      hipError_t e = alloc(std::max(count, size_t(1)));
      if (e != hipSuccess) return e;
      cap = std::max(count, size_t(1));
    }
    n = count;
    return count ? hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice) : hipSuccess;
  }
  size_t cap = 0;
  void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; cap = 0; }
  ~DevBuf() { release(); }
};

// the events around the timed stages of a synchronous call, destroyed when it returns
template <int N>
struct TimingEvents {
  hipEvent_t ev[N] = {};
  hipError_t create() { for (auto &e : ev) { hipError_t r = hipEventCreate(&e); if (r != hipSuccess) return r; } return hipSuccess; }
  hipError_t elapsed(int i, int j, float *ms) const { return hipEventElapsedTime(ms, ev[i], ev[j]); }
  ~TimingEvents() { for (auto &e : ev) if (e) (void)hipEventDestroy(e); }
};

// A result that a call builds on the handle piece by piece (ExaHipRenderer::isoMesh, lines): whatever way the call
// leaves, release() drops the pieces unless it got as far as commit().  Declared behind the call's DeviceGuard, so that
// the buffers are freed on the handle's device.
template <typename T>
struct DropUnlessCommitted {
  T &result;
  bool committed = false;
  explicit DropUnlessCommitted(T &r) : result(r) {}
  ~DropUnlessCommitted() { if (!committed) result.release(); }
  void commit() { committed = true; }
  DropUnlessCommitted(const DropUnlessCommitted &) = delete;
  DropUnlessCommitted &operator=(const DropUnlessCommitted &) = delete;
};

// What exa_hip_regions and exa_hip_basins keep on the handle: a label per lattice point, the table of records the labels
// number, and the lattice values where EXA_REGIONS_KEEP_VALUES kept them
template <typename Record>
struct LabelledLattice {
  DevBuf<int32_t> labels;
  DevBuf<Record> table;
  DevBuf<float> values;
  bool have = false, keptValues = false;
  float stageMs[6] = { 0, 0, 0, 0, 0, 0 };
  void release() { labels.release(); table.release(); values.release(); have = keptValues = false; }
};

struct ExaHipRenderer {
  int device = 0;
  std::string err;
  void fail(const std::string &m) { err = m; }

  // multi-device handle (exa_hip_create_multi): this object only fans out to `children`, one complete renderer per
  // entry of the device list, each owning the tiles t with t % n == i and storing them straight into the root
  // device's row-major frame (peer-mapped pointer)
  std::vector<ExaHipRenderer *> children;
  bool colorRowMajor = false;          // a child: colour goes row-major into the destination frame
  hipStream_t ownStream = nullptr;     // a child's launch stream
  hipEvent_t evCall = nullptr;         // multi handle: the caller's stream position at the start of a frame

  // scene
  DevBuf<int4> bricks;
  DevBuf<int32_t> leafList;
  DevBuf<int4> leafHdr;
  // Cube records (exa_cube.h): one int4 per leaf-list entry beside leafHdr, built when every brick is a cube of one edge
  // 2^cubeLog2 (0: no cube scene, nothing built); the one-channel 32-bit rope march reads them instead of the march headers
  DevBuf<int4> leafHdrCube;
  int cubeLog2 = 0;
  int cubeRecords = 1;               // option "cube_records": 0 = the march headers also in a cube scene
  DevBuf<float> scalars;
  // channel-interleaved copy of the primary channels, float[cell][ilChannels], for the multi-channel march (built on the
  // device by the first frame that marches 2..4 channels; the field-major arrays of the ABI stay for everything else)
  DevBuf<float> cellsIl;
  int ilChannels = 0;
  int ilNoMemory = 0;                // channel count whose interleaved copy could not be allocated (not tried again)
  int interleave = 1;                // option "interleave"
  bool emptyCells = false;           // the scene is marked allowEmptyCells (the reference's ALLOW_EMPTY_CELLS build): source-order kernels with the poison test
  int basisForm = 1;                 // option "basis_form": 1 (default) = the eight-corner basis sums per axis with fused multiply-adds, 0 = in the reference's source order
  int addr64 = 0;                    // option "addr64": the general 64-bit address form even where 32-bit offsets would do (tests)
  int packRecords = 1;               // option "pack_records": 0 = the march takes region ids and loads the region records, as in scenes
                                     // whose records {first brick, brick count, level} do not fit the 32 bits of a leaf reference (tests)
  uint64_t totalCells = 0;
  // Order of the bricks' cells in memory (option brick_order): 0 = as uploaded (the running `begin` of
  // OptixRenderer.cpp:71-93), 1 = along a Morton curve of the brick centres.  Cells are only ever found through their
  // brick's `begin`, so the module may move them; switching re-lays the fields on the device.
  std::vector<uint32_t> beginUploaded, beginMorton;   // per brick
  int brickOrder = 0, brickOrderWanted = 0;
  bool brickOrderPossible = true;   // the scene has the reference's layout (fields at f * totalCells, begins a partition): cells may be moved
  uint64_t numBricks = 0, leafListSize = 0;
  int applyBrickOrder(hipStream_t s);
  DevBuf<RegionInfo> regionInfo;
  DevBuf<float2> valueRange;
  DevBuf<float> domain;
  DeviceScene sc{};
  int numFields = 0;

  // region kd-tree (optional; exact front-to-back walk)
  DevBuf<KdNodeDev> kdNodes;
  DevBuf<KdNodeDev> kdMarchNodes;       // copy of kdNodes whose leaf references are packed region records (may be empty)
  int32_t kdMarchRoot = 0;
  uint32_t leafBeginBits = 0, leafSizeBits = 0;
  DevBuf<RegionRec> regionRec;
  DevBuf<int32_t> kdLevelIds;
  std::vector<int> kdLevelBegin;
  int32_t kdRoot = EXA_KD_EMPTY;
  bool rootLeafVolActive = true, rootLeafIsoActive = true;   // activity of the only region when the kd tree is one leaf
  bool haveKd = false;
  int accel = 1;                     // 1 = kd walk when available, 0 = LBVH
  float kdLo[3], kdHi[3];

  // Rope walk of the DVR march (option "walk": 0 = chosen per frame, 1 = the stack walk, 2 = the rope walk).  The leaves of
  // the kd-tree with their boxes and neighbour links are built on the host at the first frame that wants them (buildRopes);
  // the stack walk skips inactive subtrees, the rope walk passes through every leaf on the ray, so the automatic choice
  // takes the rope walk when at least kRopeActiveFraction of the regions are active for the volume march.
  DevBuf<RopeLeaf> ropeLeaves;
  DevBuf<KdNodeDev> ropeNodes;
  DevBuf<uint32_t> activeCountBuf;
  int32_t ropeRoot = EXA_KD_EMPTY + 1;
  bool ropeBuilt = false, ropeFailed = false, ropeFlagsStale = true, ropeThisFrame = false;
  int ropeFastDiv = 0, ropeAddr32 = 0;
  int walkMode = 0;
  uint32_t activeRegions = 0;        // regions active for the volume march (refreshed with the activity)
  // (C4 scene, kernel ms stack / rope by active fraction: 0.16 3.82 / 5.35, 0.23 5.45 / 7.22, 0.33 6.96 / 7.88, 0.50 1.91 / 1.65,
  //  0.62 1.98 / 1.66, 0.79 2.01 / 1.68, 1.0 19.84 / 17.31; profiles/r05_experiments.txt 5)
  static constexpr double kRopeActiveFraction = 0.4;
  bool ropeWanted() const
  {
    if (!useKd() || ropeFailed || walkMode == 1) return false;
    if (walkMode == 2) return true;
    return double(activeRegions) >= kRopeActiveFraction * double(sc.numRegions);
  }
  int buildRopes();

  // triangle surfaces
  DevBuf<BvhNode> meshNodes;
  DevBuf<float> meshVerts;
  DevBuf<int32_t> meshTris;
  int numTris = 0;

  // streamline tracer
  ExaHipTracer tracer{};
  bool haveTracer = false;
  DevBuf<float> traces;
  DevBuf<BvhNode> streamNodes;
  int numStreamPrims = 0, timestep = 0;
  bool streamDirty = false;
  int rebuildStreamlines(hipStream_t s);

  // LBVH
  DevBuf<BvhNode> volNodes, isoNodes;
  DevBuf<int32_t> levelIds;
  DevBuf<uint8_t> volActive, isoActive;
  bool volDirty = true, isoDirty = true;

  // state
  DevBuf<float4> xf;
  float xfHost[EXA_MAX_CHANNELS][EXA_NUM_XF_VALUES][4];
  bool xfDirty = true;
  ExaHipFrameState fs{};
  ExaHipParams p{};
  bool haveFs = false, haveParams = false;

  // framebuffer / shard
  int W = 0, H = 0, tilesX = 0, tilesY = 0;
  int rank = 0, world = 1;
  int tileOrder = 4;                 // Z-order launch sequence (measured best on C4)
  int debugPixel = -1;
  int fastMath = 1;                  // hardware exp2/log2 for the opacity correction (kd kernel)
  int mul24 = 0, addr32 = 0;         // address arithmetic the scene's sizes allow (set at creation)
  int fastSampler = 1;               // option fast_sampler (surfaces pre-pass; 0 = the literal addBasisFunctions)
  int tfFilter = 1;                  // TF filter weight in 1.8 fixed point as CUDA's tex1D (0: full precision)
  float tfFracMagic() const { return tfFilter ? 32768.f : 0.f; }
  DevBuf<float4> accum;
  DevBuf<float4> surf;
  DevBuf<uint32_t> tileCost;            // launch-order feedback, one entry per tile of the image
  // Launch plan of a frame with surfaces (option prepass_split, default 1).  The surfaces pre-pass is bound by the LATENCY
  // of its longest iso marches (C3: 0.3 G vector instructions in 3.6 ms), the march behind it by throughput.  The frame
  // that measures tile costs also records every tile's longest iso march; afterwards the few tiles with long pre-pass
  // rays ("heavy") get their own pre-pass + march pipeline on a side stream, which runs beside the pre-pass + march of
  // all other tiles instead of in front of it.  Same launches per tile, same pixels.
  DevBuf<uint32_t> tileCostPre;
  DevBuf<int32_t> splitMap;             // cheap tiles in launch order, then the heavy ones
  int nPreCheap = 0, nPreHeavy = 0;
  int prepassSplit = 1;
  bool preMeasured = false;             // the cost frame had surfaces (tileCostPre is valid)
  std::vector<int32_t> baseMap, curMap; // static launch order (tile_order) / the order in use
  int feedback = 1;                     // option tile_feedback
  int statsMode = 1;                    // option stats_mode: what exa_hip_render_stats collects (1 work counters, 2 wave time by phase)
  int costPhase = 0;                    // 1: the next synchronous frame measures tile costs, then the tiles are re-ordered
  // wide march (L lanes per ray) for the tiles on the frame's critical path
  int wideMode = 1;                     // option wide_march: 0 off, 1 by cost, 2 / 4 every tile with that many lanes (tests)
  // listed leaves per ray of a wide tile: kWideSegCap per window
  static size_t segsPerRay(int lanes) { return size_t(lanes) * kWideSegCap; }
  int numSimdWaves = 256 * 4 * 6;       // waves the device holds at the march kernel's occupancy
  DevBuf<int32_t> normalMap, wideMap;   // one-lane tiles in launch order; wide tiles, the 4-lane ones first
  DevBuf<float4> wideSegs;              // leaf lists of the wide march's window walkers (grown on demand)
  int nNormal = 0, nWide4 = 0, nWide2 = 0;
  int lanesTopInUse = 4;                // lanes per ray of the nWide4 tiles of the current plan
  hipStream_t side4 = nullptr, side2 = nullptr, sideN = nullptr;
  hipEvent_t evFork = nullptr, evJoin4 = nullptr, evJoin2 = nullptr, evJoinN = nullptr;
  DevBuf<uint32_t> surfRnd;
  // option ao_overlap (default 0): 1 = the deferred AO rays run BESIDE the march instead of in front of it.  The march needs the
  // surfaces' hit distance up front but their colour only for its very last operation, and the AO launch — as long as its
  // longest rays, with few waves busy — writes nothing but that colour: the march stores its pixel colour (pixBuf) and a small
  // kernel finishes the pixels once both are done.  Same operations per pixel, same order.  Measured on C5: -0.6 % beside the
  // six-wave march (1079.9 -> 1073.5 ms), +1.4 % beside the seven-wave march with four frames in flight (1052 -> 1067 ms; a
  // lone frame: 1049 / 1050) — the march now fills the GPU on its own and the finishing pass is extra traffic —, hence off.
  DevBuf<float4> pixBuf;
  int aoOverlap = 0;
  hipEvent_t evPre = nullptr, evPre2 = nullptr, evAo = nullptr, evAo2 = nullptr;
  DevBuf<AoRecord> aoRecs;              // deferred AO rays: one record per shaded hit and pixel slot at most
  DevBuf<uint32_t> aoCount;             // [0..3] the frame's list (or the cheap pipeline's), [4..7] the heavy pipeline's
  DevBuf<uint32_t> aoKeys, aoOrder, aoHist;   // ao_defer = 2: bin of every listed ray, ray indices in bin order, 2 x aoBins counters (one set per pipeline)
  DevBuf<uint8_t> aoHit;                // ... and the rays' hit flags
  uint32_t aoBins = 0;
  int aoDefer = 1;                      // option ao_defer: 1 (default since round 4: C5 1317 vs 1329 ms per 16-sample frame, C3 + iso + AO 15.8 vs 16.4 ms), 0 inline, 2 sorted
  DevBuf<uint32_t> color;
  DevBuf<int32_t> tileMap;
  int numBlocks = 0;
  bool layoutDirty = true;

  DevBuf<unsigned long long> statsBuf;
  int walkProbeOn = 0;                  // option walk_probe
  DevBuf<uint32_t> walkProbe;
  DevBuf<int32_t> errorFlag;
  // point probes (exa_hip_sample_points / exa_hip_resample): the device copy of a chunk of host arrays (bounded, grown on
  // demand), and the grid kernel's patch shape / wave-uniform path (options sample_patch, sample_uniform)
  struct Probes {
    DevBuf<char> stage;
    int patch = 3, uniform = 1;
  } probes;
  // the mesh of the last exa_hip_isosurface (on a multi-device handle: in the renderer of devices[0]) and the time its
  // stages took (lattice values, cube pass, point pass, scans, emit, gradients)
  struct IsoMesh {
    DevBuf<float> vertices, gradients;
    DevBuf<int32_t> triangles;
    bool have = false;
    float stageMs[6] = { 0, 0, 0, 0, 0, 0 };
    void release() { vertices.release(); gradients.release(); triangles.release(); have = false; }
  } isoMesh;
  // the contour lines of the last exa_hip_isolines (in the renderer of devices[0] as well), independent of the mesh: the
  // packed vertices with their plane coordinates, the segments, where each level's begin (numIsos + 1 entries each), the
  // lattice values where EXA_ISOLINES_KEEP_VALUES kept them, and the time of the stages summed over the levels (positions
  // and values, square pass, point pass, scans, emit, gradients)
  struct Isolines {
    DevBuf<float> vertices, uv, gradients, values;
    DevBuf<int32_t> segments;
    std::vector<uint64_t> vertexOffsets, segmentOffsets;
    bool have = false, withGradients = false, keptValues = false;
    float stageMs[6] = { 0, 0, 0, 0, 0, 0 };
    void release()
    {
      vertices.release(); uv.release(); gradients.release(); values.release(); segments.release();
      vertexOffsets.clear(); segmentOffsets.clear();
      have = withGradients = keptValues = false;
    }
  } isolines;
  // the regions of the last exa_hip_regions (in the renderer of devices[0] as well), independent of the mesh and of the
  // lines: the labels (the union-find's parent links while the call runs), the table, the lattice values where
  // EXA_REGIONS_KEEP_VALUES kept them, and the time of the stages (values, init, merge, flatten, rank, stats)
  LabelledLattice<ExaHipRegion> isoRegions;
  // the critical points of the last exa_hip_critical_points (in the renderer of devices[0] as well), independent of the mesh,
  // the lines and the regions: the records, the probe's arrays where EXA_CRITICAL_PROBE asked for them, and the time of the
  // stages (values, cells, scans, refine, emit, probe)
  struct IsoCritical {
    DevBuf<ExaHipCriticalPoint> points;
    DevBuf<float> probe;
    DevBuf<int32_t> probeStatus;
    bool have = false, probed = false;
    float stageMs[6] = { 0, 0, 0, 0, 0, 0 };
    void release() { points.release(); probe.release(); probeStatus.release(); have = probed = false; }
  } isoCritical;
  // the basins of the last exa_hip_basins (in the renderer of devices[0] as well), independent of the mesh, the lines, the
  // regions and the critical points: the labels (the up links, then the components while the call runs), the table, the
  // lattice values where EXA_REGIONS_KEEP_VALUES kept them, and the time of the stages (values, ascent, passes, links, rank,
  // stats)
  LabelledLattice<ExaHipBasin> isoBasins;
  // exa_hip_histogram (on a multi-device handle: in the renderer of devices[0]): the work list of the pass — segments
  // {brick, first cell} by level and the offsets of the runs, built by the first call (exa_stats.cpp) —, whether the scene's
  // volume-weighted cell count fits 64 bits, the device copy of a call's result and the device time of its kernel
  struct Histogram {
    DevBuf<uint4> segs;
    DevBuf<uint32_t> runs;
    uint32_t numRuns = 0;
    bool planBuilt = false, volumeFits = true;
    DevBuf<unsigned long long> result;
    float kernelMs = 0.f;
  } hist;
  // the lines of the last exa_hip_streamlines (on a multi-device handle: in the renderer of devices[0]), packed, and the
  // device time of its two kernels
  struct Streamlines {
    DevBuf<float> vertices, velocities;
    DevBuf<unsigned long long> offsets;
    DevBuf<uint32_t> seedVertex;
    DevBuf<int32_t> reasons;
    uint64_t seeds = 0, numVertices = 0;
    bool have = false;
    float kernelMs = 0.f;
    void release()
    {
      vertices.release(); velocities.release(); offsets.release(); seedVertex.release(); reasons.release();
      seeds = 0; numVertices = 0;
      have = false;
    }
  } lines;
  // exa_hip_lic (in the renderer of devices[0] as well): the device time of the last call's kernels, summed, and how the
  // lanes are laid out — options "lic_lanes" (lanes per pixel, 1 or 2) and "lic_patch" (0 = a wave's pixels in a row,
  // 1 = in a patch 8 pixels wide); the bytes are the same in every layout
  struct Lic {
    float kernelMs = 0.f;
    int lanes = 1, patch = 1;
  } lic;
  // exa_hip_flowmap (in the renderer of devices[0] as well): the device time of the last call's two stages (integrate,
  // stretch), and which 64 lattice points a wave takes — option "flowmap_patch" (0 = 64 along x, 1 = a 4 x 4 x 4 patch); the
  // bytes are the same either way
  struct Flowmap {
    float ms[2] = { 0.f, 0.f };
    int patch = 1;
  } flowmap;
  // the device time of the last exa_hip_project's kernel launches, summed (in the renderer of devices[0])
  struct Projection {
    float kernelMs = 0.f;
  } project;
  // the same of the last exa_hip_sample_triangles, and whether it packs small triangles into shared waves (option surface_pack)
  struct Surface {
    float kernelMs = 0.f;
    int pack = 1;
  } surface;
  // the same of the last exa_hip_raycast_iso
  struct Raycast {
    float kernelMs = 0.f;
  } raycast;
  // the device time of the kernels of the last exa_hip_sample_derived / exa_hip_resample_derived
  struct Derived {
    float kernelMs = 0.f;
  } derived;
  // the device time of the stages of the last exa_hip_profile (in the renderer of devices[0]): values, classify,
  // accumulate, finish; the call keeps nothing else
  struct Profile {
    float stageMs[4] = { 0.f, 0.f, 0.f, 0.f };
  } profile;
  // the device time of the stages of the last exa_hip_distance[_derived|_mask] (in the renderer of devices[0]): values,
  // rows, columns, finish; the call keeps nothing else
  struct Distance {
    float stageMs[4] = { 0.f, 0.f, 0.f, 0.f };
  } distance;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
  ExaHipStats last{};

  bool isoEnabled() const
  {
    for (int i = 0; i < EXA_MAX_ISO_SURFACES; i++) if (fs.iso[i].enabled) return true;
    return false;
  }
  bool contourEnabled() const
  {
    for (int i = 0; i < EXA_MAX_CONTOUR_PLANES; i++) if (fs.contour[i].enabled) return true;
    return false;
  }
  bool surfacesEnabled() const { return isoEnabled() || contourEnabled() || numTris > 0 || numStreamPrims > 0; }
  float voxLo[3], voxHi[3];
  void worldBounds(float lo[3], float hi[3]) const;
  uint64_t outputPixels() const { return uint64_t(numBlocksFor()) * kTilePixels; }
  int numBlocksFor() const
  {
    const int tiles = tilesX * tilesY;
    if (world <= 1) return tiles;
    return tiles > rank ? (tiles - rank + world - 1) / world : 0;
  }

  // tile layout, launch order and wide-march assignment (exa_frame.cpp)
  int rebuildLayout();
  int reorderFromCosts();
  int assignWide(const std::vector<uint32_t> *costOfTile);

  int kdRefit(const uint8_t *active, int which, hipStream_t s);
  bool useKd() const { return haveKd && accel == 1; }

  // The LBVH over the regions (north_star's structure; accel=0, scenes without a kd-tree, and the
  // streamline tracer's point queries) is built on first use, on the device (exa_lbvh.hip): Morton codes, radix
  // sort, topology level by level; boxes are filled by the refit.  Option lbvh_build = 1 builds the same tree on
  // the host instead (LbvhTopology, exa_hostbvh.h; the two are identical node for node, tests compare them).
  bool lbvhBuilt = false;
  int lbvhOnHost = 0;
  std::vector<std::pair<int, int>> levelRanges;   // (offset into levelIds, count) per refit launch, children before parents
  DevBuf<BvhNode> topoNodes;                       // children filled, boxes empty: the template of volNodes / isoNodes
  int ensureLbvh();
  bool needLbvh() const { return !useKd() || (haveTracer && tracer.enabled); }
  int refit(DevBuf<BvhNode> &nodes, const uint8_t *active, hipStream_t s);

  int prepareFrame(hipStream_t s);

  // a frame's launches (exa_frame.cpp): launch() fills the kernels' arguments and the deferred-AO lists, then issues one
  // of the plans
  bool measureCosts = false;            // set by renderImpl for synchronous frames
  int launch(uint32_t *dstDevice, bool stats, hipStream_t s);
  int fillRenderArgs(RenderArgs &a, uint32_t *dstDevice, bool stats, hipStream_t s);
  int prepareSurfaceLists(RenderArgs &a, bool stats, hipStream_t s);
  hipError_t march(const RenderArgs &a, int n, bool surfArg, int statsArg, hipStream_t s);
  int launchSurfaces(const RenderArgs &a, bool surfOn, bool stats, hipStream_t s);
  int launchPlain(const RenderArgs &a, bool surfOn, bool stats, hipStream_t s);
  int launchSplit(const RenderArgs &a, bool overlap, hipStream_t s);
  int launchOverlap(const RenderArgs &a, hipStream_t s);
  int launchWide(const RenderArgs &a, bool surfOn, hipStream_t s);
};

// the renderer that holds what every device has a copy of (traces, activity) and that runs the probes
inline ExaHipRenderer *firstChild(ExaHipRenderer *h) { return h->children.empty() ? h : h->children[0]; }

// The packed region record a leaf reference of the march tree carries, {listBegin | listSize-1 << bb | level << (bb+sb)},
// level = log2(finestLevelCellWidth) (a power of two in [1, 2^30], checked at creation)
inline int levelOfWidth(float w) { int lv = 0; while (lv < 31 && float(1 << lv) < w) lv++; return lv; }
inline uint32_t packLeafRec(int32_t listBegin, int32_t listSize, float width, uint32_t bb, uint32_t sb)
{
  return uint32_t(listBegin) | (uint32_t(listSize - 1) << bb) | (uint32_t(levelOfWidth(width)) << (bb + sb));
}

// Argument checks that three or more calls state, each with one wording: false after h has failed with it
inline bool checkChannel(ExaHipRenderer *h, const char *fn, int32_t channel)
{
  if (channel >= 0 && channel < h->numFields) return true;
  h->fail(std::string(fn) + ": channel out of range");
  return false;
}
// hint: the call's own words in parentheses on what applies, or ""
inline bool checkFlags(ExaHipRenderer *h, const char *fn, int32_t flags, int32_t known, const char *hint)
{
  if (!(flags & ~known)) return true;
  h->fail(std::string(fn) + ": unknown flag bits" + hint);
  return false;
}
// an allocation of a call failed with e: clears the runtime's sticky error, h fails with "fn: what: <e>"; returns 1
inline int failNoMemory(ExaHipRenderer *h, const char *fn, const char *what, hipError_t e)
{
  (void)hipGetLastError();
  h->fail(std::string(fn) + ": " + what + ": " + hipGetErrorString(e));
  return 1;
}

// What the _read, _release and _stage_ms calls of the results on the handle share (`which`: the result's member of the
// renderer, of devices[0] on a multi-device handle).  An array the caller does not ask for, or that is empty, is not copied.
template <typename T>
hipError_t copyOut(T *dst, const DevBuf<T> &src, hipMemcpyKind kind, hipStream_t s)
{
  return dst && src.n ? hipMemcpyAsync(dst, src.p, src.n * sizeof(T), kind, s) : hipSuccess;
}
template <typename T>
int releaseResult(ExaHipRenderer *h, T ExaHipRenderer::*which)
{
  if (!h) return 1;
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  (r->*which).release();
  return 0;
}
template <typename T>
int readStageMs(ExaHipRenderer *h, T ExaHipRenderer::*which, float ms[6])
{
  if (!h || !ms) return 1;
  for (int k = 0; k < 6; k++) ms[k] = (firstChild(h)->*which).stageMs[k];
  return 0;
}

// Reads and clears the loop guard of r's kernels; when it tripped, h (r or its multi-device handle) fails with fn + what
// and the ABI's return code 3 comes back
int checkLoopGuard(ExaHipRenderer *h, ExaHipRenderer *r, const char *fn, const char *what);

// What the probes and the streamline integrator share (exa_probe.cpp): the checks (a kd tree; a frame state for world
// space), a pending brick order applied, and the lookup / field part of the kernels' arguments; the message of the kd
// descent's loop guard (checkLoopGuard)
int probeSetup(ExaHipRenderer *h, ExaHipRenderer *r, const char *fn, bool world, hipStream_t s, SampleArgs &a);
extern const char *const kDescentGuard;
