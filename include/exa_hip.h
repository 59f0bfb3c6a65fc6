/* exa_hip.h — C ABI of the MI355X-native ExaBrick render module (libexa_hip.so).
 *
 * This is the drop-in boundary for the reference's `exa::OptixRenderer`
 * (exa/OptixRenderer.h:32-97) and the device programs it launches
 * (programs/exabrick.cu).  Plain pointers and sizes only; no C++/torch types.
 * The C++ facade `exa::Renderer` (owlexabrick_amd/host/exa_host.h) keeps the
 * OptixRenderer method names on top of these entry points; INTEGRATION.md shows
 * the binding a maintainer of the reference would add.
 *
 * Two groups:
 *   exa_prep_*  host-side data preparation the OptixRenderer constructor does
 *               (brick flattening, scalar gather, same-bricks regions)
 *   exa_hip_*   the device module (upload, LBVH, activity, render, readback)
 *
 * All functions return 0 on success, non-zero on error; the message is
 * available from exa_hip_last_error()/exa_prep_last_error().  Nothing here
 * falls back to a CPU renderer: without a HIP device exa_hip_create fails.
 */
#ifndef EXA_HIP_H
#define EXA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EXA_NUM_XF_VALUES      128 /* exa/common.h:41 */
#define EXA_MAX_CHANNELS       10  /* exa/common.h:42 */
#define EXA_MAX_ISO_SURFACES   2   /* exa/common.h:43 */
#define EXA_MAX_CONTOUR_PLANES 3   /* exa/common.h:44 */

/* ---- POD mirrors of the reference's shared host/device structs ---- */

/* programs/Brick.h:31-71
 *
 * Coordinates are signed: a scene may lie anywhere, the origin inside it or far from it.  What bounds them is that every
 * table derived from the bricks is float32.  With cw = 2^level, each of the planes
 *     lower,  lower +- cw/2,  lower + size cw,  lower + (size +- 1/2) cw        (per axis)
 * must be exactly representable in float32: for level-0 bricks that is |coordinate| < 2^23.  exa_prep_create[_ex] and
 * exa_hip_create[_multi] refuse a scene that breaks this and name the brick and the plane.  exa_prep_create[_ex]
 * furthermore refuses a scene in which the float32 arithmetic that chooses the regions' split planes (midpoints and
 * distances of such planes, as the reference computes them) rounds so that another plane is chosen than exact
 * arithmetic would choose: level-0 bricks beyond |coordinate| = 2^22.  Inside these limits the prepared tables of a scene
 * moved by an integer vector are the tables of the scene, moved. */
typedef struct ExaBrick {
  int32_t  lower[3];
  int32_t  size[3];
  int32_t  level;
  uint32_t begin;   /* offset of the brick's first cell in the gathered scalar arrays */
} ExaBrick;

/* exa/Regions.h:31-41 (ExaBrickRegions::BrickRegion == SameBricksRegion) */
typedef struct ExaBrickRegion {
  float   domain_lo[3], domain_hi[3];
  float   valueRange_lo, valueRange_hi;
  int32_t leafListBegin;
  int32_t leafListSize;
  float   finestLevelCellWidth;
} ExaBrickRegion;

/* programs/FrameState.h:29-71.  The per-channel cudaTextureObject_t handles are
 * replaced by exa_hip_set_xf(); bools are int32. */
typedef struct ExaHipFrameState {
  float cam_pos[3], cam_dir00[3], cam_dirDu[3], cam_dirDv[3];
  struct { int32_t enabled; float value; int32_t channel; } iso[EXA_MAX_ISO_SURFACES];
  struct { int32_t enabled; float normal[3]; int32_t channel; float offset; } contour[EXA_MAX_CONTOUR_PLANES];
  struct { float lo[3], hi[3]; int32_t enabled; } clipBox;
  struct { float length; int32_t enabled; } ao;
  float   clockScale;
  float   xfm_vx[3], xfm_vy[3], xfm_vz[3], xfm_p[3]; /* affine3f voxelSpaceTransform */
  int32_t frameID;
  float   xfDomain[EXA_MAX_CHANNELS][2];
  float   xfOpacityScale;
} ExaHipFrameState;

/* the scalar launch parameters of programs/LaunchParams.h:26-80 the path reads,
 * plus VolumeData.numChannels / spaceSkippingEnabled (programs/VolumeData.h:24-31) */
typedef struct ExaHipParams {
  float   dt;                   /* OptixRenderer::updateDt            (OptixRenderer.cpp:413-416) */
  int32_t numPrimaryChannels;   /* multiFieldDvr ? #fields : 1        (OptixRenderer.cpp:284)     */
  int32_t colormapChannel;      /*                                    (OptixRenderer.cpp:278-283) */
  int32_t gradientShadingDVR;   /* setGradientShadingDVR              (OptixRenderer.cpp:434-437) */
  int32_t gradientShadingISO;   /* setGradientShadingISO              (OptixRenderer.cpp:439-442) */
  int32_t numChannels;          /* VolumeData.numChannels             (OptixRenderer.cpp:650)     */
  int32_t spaceSkippingEnabled; /* !contourPlanesActive && doSpaceSkipping (OptixRenderer.cpp:418-432) */
} ExaHipParams;

/* The recursion of ExaBrickRegions::buildRec (exa/Regions.cpp:73-179) is a kd-tree
 * whose leaves are the regions; exa_prep keeps it.  A child reference is >= 0 for a
 * node index, < 0 for a leaf (region id = ~ref), EXA_KD_EMPTY for an empty side.
 * Optional input of exa_hip_create: with it the module walks the regions in exact
 * front-to-back order; without it (regions built elsewhere) it uses its LBVH. */
#define EXA_KD_EMPTY INT32_MIN
typedef struct ExaKdNode {
  float   split;   /* plane position on `axis`                         */
  int32_t axis;    /* 0,1,2                                            */
  int32_t left;    /* child on the lower side of the plane             */
  int32_t right;   /* child on the upper side                          */
} ExaKdNode;

/* what the OptixRenderer constructor uploads (OptixRenderer.cpp:95-98,133-141,160-168) */
typedef struct ExaHipScene {
  const ExaBrick       *bricks;        uint64_t numBricks;
  const ExaBrickRegion *regions;       uint64_t numRegions;
  const int32_t        *leafList;      uint64_t leafListSize;
  const float          *scalars;       /* numFields * totalCells floats, brick order    */
  const uint64_t       *channelOffset; /* numFields entries (reference: 32-bit unsigned) */
  uint64_t              totalCells;
  int32_t               numFields;
  float                 voxelBounds_lo[3], voxelBounds_hi[3];
  const ExaKdNode      *kdNodes;       /* optional (may be NULL) */
  uint64_t              numKdNodes;
  int32_t               kdRoot;        /* reference of the root (a leaf ref for a one-region scene) */
  /* (added in round 4, at the end: a caller that fills the struct by hand zero-initialises it first; exa_hip_create refuses
     any value other than 0 and 1, so that a struct filled field by field without this one is caught, not misread) */
  int32_t               allowEmptyCells; /* the reference's compile-time option ALLOW_EMPTY_CELLS (CMakeLists.txt:70-73, default
                                          OFF) as a property of the scene: scalars equal to EXA_EMPTY_CELL_POISON_VALUE are
                                          "no cell here" and addBasisFunctions skips them (programs/exabrick.cu:614-618) */
} ExaHipScene;

/* programs/FrameState.h:27 */
#define EXA_EMPTY_CELL_POISON_VALUE (-1e20f)
/* exa_prep_create_ex flags */
#define EXA_PREP_ALLOW_EMPTY_CELLS 1   /* a negative cell id = no cell: its slot holds the poison value (exa/OptixRenderer.cpp:116-118) */

/* work counters of one frame (instrumented kernel variant); the basis of the
 * algorithmic-bytes figure in DESIGN.md */
typedef struct ExaHipStats {
  uint64_t segments;      /* traceVolumeRay hits                                  */
  uint64_t sample_evals;  /* samplePoint[WithDerivative] calls in the DVR march    */
  uint64_t samples;       /* ...of which valid                                     */
  uint64_t brick_visits;  /* addBasisFunctions calls, all paths                    */
  uint64_t corner_loads;  /* cell scalars read, all paths                          */
  uint64_t iso_segments;  /* iso-BVH hits                                          */
  uint64_t iso_evals;     /* sample calls of the iso march (+ re-samples)          */
  uint64_t nodes_visited; /* acceleration-structure nodes fetched: 64-B LBVH nodes or
                             16-B kd nodes, see node_bytes                         */
  uint64_t node_bytes;    /* bytes per node of the structure that was walked       */
  uint64_t pixels;        /* pixels rendered by this handle (its tile shard)       */
  uint64_t diag[9];       /* kd kernel diagnostics: {waves,lanes} x {brick visit, sample epilogue,
                             kd node step, leaf accept}, then kd-interval/slab-test mismatches */
  uint64_t phase_cycles[5]; /* kd kernel: shader-clock cycles of its waves, summed, by phase: brick visit, sample
                             epilogue, kd walk, segment pop, other (ray set-up, output) */
  float    kernel_ms;     /* hipEvent time of the last render launch               */
  float    rebuild_ms;    /* hipEvent time of the last activity+refit pass         */
  uint64_t walk_restarts;     /* kd walk: restarts from the root after the 4-entry short stack dropped an entry */
  uint64_t walk_union_nodes;  /* option walk_probe: kd nodes visited, counted once per WAVE (the union over its 64 rays):
                                 what a wave-coherent (packet) walk would have to step through at least */
  uint64_t walk_probe_overflow; /* ... lanes that found their wave's probe table full (0 in a valid measurement) */
  uint64_t wave_iters;        /* kd march: march iterations of every wave's longest ray, summed over the waves ...       */
  uint64_t tile_iters;        /* ... and 4 x the slowest wave's per workgroup, summed: wave_iters / tile_iters = how evenly
                                 the four waves of a workgroup finish (its LDS is held until the slowest one does)        */
  uint64_t walk_leaf_visits;  /* rope walk (option "walk"): leaves fetched, 64 B each — counted as four 16-byte nodes in
                                 nodes_visited, so nodes_visited - 4 * walk_leaf_visits inner nodes were stepped through;
                                 0 for the stack walk, whose leaves are references inside their parent node              */
} ExaHipStats;

typedef struct ExaHipRenderer ExaHipRenderer;
typedef struct ExaPrep ExaPrep;

/* ------------------------------------------------------------------ */
/* host data preparation                                               */
/* ------------------------------------------------------------------ */

/* OptixRenderer::OptixRenderer data prep (exa/OptixRenderer.cpp:71-141):
 * brick flattening with running `begin`, index-vector concat, per-field gather
 * scalar[i] = field[cellID[i]]; then ExaBrickRegions::buildFrom
 * (exa/Regions.cpp:242-320) over the first numRegionFields fields.
 * bricks7 = numBricks x {size.xyz, lower.xyz, level}, the `.bricks` record
 * header order (exa/ExaBricks.cpp:27-33).  Errors mirror the reference's
 * std::runtime_error texts. */
int exa_prep_create(const int32_t *bricks7, uint64_t numBricks,
                    const int32_t *cellIDs, uint64_t numCellIDs,
                    const float *const *fields, const uint64_t *fieldLen,
                    int32_t numFields, int32_t numRegionFields, int32_t numThreads,
                    ExaPrep **out);
/* as exa_prep_create with `flags` (EXA_PREP_*).  EXA_PREP_ALLOW_EMPTY_CELLS = the reference built with
 * -DALLOW_EMPTY_CELLS=1: every negative cell id is "no cell", as in the renderer (exa/OptixRenderer.cpp:116-118; that only -1
 * occurs is an assert of the loader, exa/ExaBricks.cpp:46-49, compiled out of a release build); the regions' value ranges include the poison
 * value, as the reference's computeValueRange (exa/Regions.cpp:182-240) does; the scene is marked allowEmptyCells */
int exa_prep_create_ex(const int32_t *bricks7, uint64_t numBricks,
                       const int32_t *cellIDs, uint64_t numCellIDs,
                       const float *const *fields, const uint64_t *fieldLen,
                       int32_t numFields, int32_t numRegionFields, int32_t numThreads, int32_t flags,
                       ExaPrep **out);
void exa_prep_destroy(ExaPrep *);
/* fills an ExaHipScene whose pointers stay valid until exa_prep_destroy */
int  exa_prep_scene(const ExaPrep *, ExaHipScene *out);
const char *exa_prep_last_error(void);
/* diagnostic: the leaves and neighbour links exa_hip builds for its rope walk (option "walk") from this scene's kd-tree, on the
 * host (owlexabrick_amd/csrc/exa_ropes.h).  Call with leafBoxes == NULL for the counts, then with arrays of that size:
 * leafBoxes numLeaves x 6 floats (lo, hi), leafLinks numLeaves x 6 (-x +x -y +y -z +z: inner node >= 0, leaf ~index, outside
 * the root box = EXA_KD_EMPTY + 1), leafRegion numLeaves (region id; -1: a gap = an empty child slot of the tree), nodes
 * numNodes (the tree behind the links: no empty slots).  *flags: bit 0 = every region leaf's box is its domain, bit 1 = the
 * planes are in the range of the walk's short exact division. */
int exa_prep_ropes(const ExaPrep *, uint64_t *numLeaves, uint64_t *numNodes, float *leafBoxes, int32_t *leafLinks,
                   int32_t *leafRegion, ExaKdNode *nodes, int32_t *flags);
/* diagnostic: the 16-byte cube records exa_hip_create builds beside the march headers (option "cube_records") for a scene
 * whose bricks are all cubes of one edge 2^k, 1 <= k <= 7, with every `begin` a multiple of the cube's cell count, begin /
 * 8^k < 2^23 and levels 0..30 (owlexabrick_amd/csrc/exa_cube.h).  *log2Edge = k, or 0 when the scene is no cube scene (then
 * nothing is built).  beginAlt (may be NULL): numBricks `begin` values of the other brick order, held to the same conditions.
 * records (may be NULL): leafListSize x 4 words {float(lower.xyz) as float bits, ((begin >> 3k) << 9) | (127 - level)}. */
int exa_prep_cube_records(const ExaBrick *bricks, uint64_t numBricks, const int32_t *leafList, uint64_t leafListSize,
                          const uint32_t *beginAlt, int32_t *log2Edge, int32_t *records);
/* diagnostic: replaces the prep's region kd-tree by a caller's own (what a caller may hand exa_hip_create in
 * ExaHipScene.kdNodes); exa_prep_scene and exa_prep_ropes then see that tree.  Checked as exa_hip_create checks it: axis 0..2,
 * references in range, children after their parent. */
int exa_prep_set_kd_tree(ExaPrep *, const ExaKdNode *nodes, uint64_t numNodes, int32_t root);

/* ------------------------------------------------------------------ */
/* device module                                                       */
/* ------------------------------------------------------------------ */

/* replaces the upload + accel half of OptixRenderer::OptixRenderer
 * (exa/OptixRenderer.cpp:95-98,133-141,160-168,305-316): copies the scene to HBM
 * on `device`, builds the LBVH over the regions.  The caller's arrays are not
 * referenced after return. */
int exa_hip_create(const ExaHipScene *scene, int32_t device, ExaHipRenderer **out);
/* One handle that drives several GPUs of one node (SURVEY 8(b) threading row, 8(e)); new relative to the reference,
 * whose raygen program never reads LaunchParams.deviceIndex/deviceCount (programs/LaunchParams.h:31-32).  The scene is
 * replicated on every device of the list; device i renders the 16x16 tiles t with t % numDevices == i on a stream of
 * its own and stores them straight into the destination frame, which lives on devices[0] (the other devices write it
 * through a peer mapping over xGMI): no gather, no untile.  Every other entry point takes the handle unchanged
 * (exa_hip_set_shard is refused).  A device destination passed to exa_hip_render must be memory of devices[0]; with
 * async != 0 the call returns once the work is queued and `hipStream` (a stream of devices[0]) waits for all
 * devices, so the caller can queue the frame's copy-out behind it and start the next frame into another buffer.
 * Entries of `devices` may repeat (several renderers on one GPU: rehearsal on a one-GPU box). */
int exa_hip_create_multi(const ExaHipScene *scene, const int32_t *devices, int32_t numDevices, ExaHipRenderer **out);
int exa_hip_destroy(ExaHipRenderer *);

/* OptixRenderer::resizeFrameBuffer (exa/OptixRenderer.cpp:341-355): (re)allocates
 * the float4 accumulation buffer; the colour destination is passed per render. */
int exa_hip_resize(ExaHipRenderer *, int32_t width, int32_t height);

/* whole-struct upload as every OptixRenderer setter does (updateCamera,
 * updateFrameID, updateIsoValues, setVoxelSpaceTransform ...;
 * exa/OptixRenderer.cpp:322-339,357-368,406-411,489-502).  A change of
 * xfDomain/xfOpacityScale marks the volume LBVH dirty, a change of iso[] marks
 * the iso LBVH dirty (needVolumeBVHRebuild / needIsoBVHRebuild). */
int exa_hip_set_frame_state(ExaHipRenderer *, const ExaHipFrameState *);

/* OptixRenderer::updateXF texture upload (exa/OptixRenderer.cpp:385-402):
 * 128 x (r,g,b,a) for channel `chan`; marks the volume LBVH dirty. */
int exa_hip_set_xf(ExaHipRenderer *, int32_t chan, const float *rgba128);

/* the triangle surfaces of the OptixRenderer constructor (createSurfaces, exa/OptixRenderer.cpp:554-612;
 * closest-hit shading programs/exabrick.cu:420-433): all meshes concatenated, world space,
 * vertices 3 floats each, triangles 3 vertex indices each.  numTris = 0 removes them. */
int exa_hip_set_triangles(ExaHipRenderer *, const float *vertices, uint64_t numVertices,
                          const int32_t *triangles, uint64_t numTris);

/* streamline tracer (OptixRenderer::traces, exa/OptixRenderer.h:160-170) */
typedef struct ExaHipTracer {
  int32_t enabled;          /* setTracerEnabled                                   */
  int32_t channels[3];      /* the three scalar fields read as a velocity          */
  int32_t numTraces, numTimesteps;
  float   steplen;
} ExaHipTracer;
/* resetTracer (exa/OptixRenderer.cpp:450-472): seeds (numTraces x 3, the caller draws them) become
 * timestep 0 of every trace, the rest is cleared, the current timestep returns to 0 */
int exa_hip_reset_tracer(ExaHipRenderer *, const ExaHipTracer *, const float *seeds);
int exa_hip_set_tracer_enabled(ExaHipRenderer *, int32_t enabled);
/* advanceTracer (:474-487): next timestep; *rebuild = needStreamlineBVHRebuild */
int exa_hip_advance_tracer(ExaHipRenderer *, int32_t *rebuild);
/* numTraces * numTimesteps * 3 floats */
int exa_hip_read_traces(ExaHipRenderer *, float *dst);

/* updateDt / setSpaceSkipping / setGradientShading* (exa/OptixRenderer.cpp:413-442) */
int exa_hip_set_params(ExaHipRenderer *, const ExaHipParams *);

/* image-space sharding for multi-GPU: this handle renders the 16x16-pixel tiles
 * t with t % worldSize == rank (row-major tile order) and writes them compactly,
 * tile-major, 256 pixels per tile.  rank 0 / worldSize 1 = whole frame in the
 * normal row-major layout.  New relative to the reference (it never shards). */
int exa_hip_set_shard(ExaHipRenderer *, int32_t rank, int32_t worldSize);
/* number of uint32 pixels exa_hip_render writes for the current size/shard */
uint64_t exa_hip_output_pixels(const ExaHipRenderer *);
/* root side of the gather: `gathered` holds worldSize shards back to back, each
 * padded to shardStridePixels; writes the row-major W*H image.  Device pointers. */
int exa_hip_untile(ExaHipRenderer *, const uint32_t *gathered, uint64_t shardStridePixels,
                   int32_t worldSize, uint32_t *rgba8_out, void *hipStream);

/* OptixRenderer::render (exa/OptixRenderer.cpp:531-552): re-evaluates region
 * activity and refits the dirty LBVH(s), then launches the frame.
 * rgba8 is the caller-owned colour buffer (resizeFrameBuffer's fbPointer):
 * a device pointer if dstIsDevice, else host memory (copied back synchronously).
 * hipStream: a hipStream_t or NULL for the default stream.  Synchronous unless
 * dstIsDevice and async != 0. */
int exa_hip_render(ExaHipRenderer *, uint32_t *rgba8, int32_t dstIsDevice,
                   void *hipStream, int32_t async);

/* same frame through the instrumented kernel variant; fills counters */
int exa_hip_render_stats(ExaHipRenderer *, uint32_t *rgba8, int32_t dstIsDevice, ExaHipStats *out);
int exa_hip_get_stats(ExaHipRenderer *, ExaHipStats *out);

/* accumulation buffer (float4 per pixel, row-major, this shard's layout) */
int exa_hip_read_accum(ExaHipRenderer *, float *dst4);
int exa_hip_write_accum(ExaHipRenderer *, const float *src4);

/* region activity as the VolumeBVH / IsoSurface bounds programs see it
 * (programs/exabrick.cu:285-312, 373-402), one byte per region; for tests */
int exa_hip_read_activity(ExaHipRenderer *, int32_t which /*0 volume, 1 iso*/, uint8_t *dst);

/* ---- point probes: the reconstructed field at arbitrary points and on uniform grids (new relative to the reference,
 * whose samplePoint / samplePointWithDerivative, programs/exabrick.cu:781-806,883-928, only run inside its programs) ----
 *
 * Spaces.  Positions are in voxel space (the bricks' coordinates) unless EXA_SAMPLE_WORLD_SPACE is given: then they are
 * mapped with the voxelSpaceTransform of the last exa_hip_set_frame_state, in xfmPoint's operation order
 * x*vx + (y*vy + (z*vz + p)), nothing contracted; world space before any frame state is an error.
 *
 * Region lookup.  A result depends only on the scene, the position, the option basis_form and (world space) the
 * transform — not on the transfer function, region activity, iso values, the camera or any other option:
 *   - outside the closed root box [kdLo, kdHi] of the region kd-tree (the union of the region domains), or with a NaN or
 *     infinite coordinate: status -1;
 *   - else descend from the root: at an inner node `right` if p[axis] >= split, else `left` (activity bits ignored).  So a
 *     point belongs to the half-open kd cell [lo, hi) on every axis, except on the upper faces of the root box, which are
 *     closed: a point on a face between a region and a gap above it gets -1 (the region's hat basis ends on that face;
 *     there is no backtracking);
 *   - EXA_KD_EMPTY: -1; a leaf: region ~ref if p lies in that region's closed domain, else -1 (a caller's own tree,
 *     exa_prep_set_kd_tree, stays honest);
 *   - the descent is bounded; a tripped bound sets the module's loop-guard flag, and a synchronous call fails with 3.
 * A scene without a kd tree (ExaHipScene.kdNodes == NULL, more than one region) is refused: its LBVH is refit to the region
 * activity and cannot answer an activity-free lookup.
 *
 * Value.  samplePoint through the march headers in the handle's current basis_form (a scene marked allowEmptyCells: the
 * form-0 sums with the poison test).  sumW <= 1e-20 gives status -2 (the reference's samplePoint returns false).  Status
 * is per point AND channel: in an empty-cells scene the poison test skips corners channel by channel
 * (exabrick.cu:614-618), so one channel can vanish where another does not.
 *
 * Gradient (EXA_SAMPLE_GRADIENT): the reference's numerator sumW*sumD - sumWV*sumDC (exabrick.cu:916-921), bit for bit as
 * samplePointWithDerivative returns it.  The derivative weights in it are taken per brick in that brick's own cell units
 * (the reference compiles INV_CELL_WIDTH == 1, exabrick.cu:640-641): in a region whose bricks are at level L it is
 * sumW*sumW * 2^L times the gradient, and in a region with bricks of several levels (every coarse-fine boundary) it is
 * no voxel-space vector at all.  It is what the reference shades with, nothing more.
 * With EXA_SAMPLE_GRADIENT_NORMALIZED as well the result is the gradient of the reconstruction sumWV/sumW with respect to
 * VOXEL-space coordinates (also for world-space positions): every brick's derivative weights carry its 2^-level, and the
 * numerator formed from those sums is divided by sumW*sumW on the device.  The value and the status are the same with
 * and without the flag.
 *
 * Fill.  Where status < 0, value and gradient components of that point and channel are `fill`.
 *
 * Arrays.  n == 0 does nothing.  Host arrays go through a device buffer of bounded size (64 MiB), in chunks.  Synchronous
 * unless the pointers are device pointers and async != 0 (as exa_hip_render); hipStream: a hipStream_t or NULL.  A handle
 * of exa_hip_create_multi runs the call on devices[0], and device pointers are memory of that device.  A pending
 * brick_order change is applied first, as render does.  Unknown flag bits are an error. */
#define EXA_SAMPLE_WORLD_SPACE          1
#define EXA_SAMPLE_GRADIENT             2
#define EXA_SAMPLE_GRADIENT_NORMALIZED  4   /* with EXA_SAMPLE_GRADIENT only */
/* channels: numChannels (1..EXA_MAX_CHANNELS) entries in [0, numFields), repeats allowed; values n x numChannels;
 * gradients n x numChannels x 3 (read only with EXA_SAMPLE_GRADIENT, may be NULL otherwise); status n x numChannels:
 * region id, -1 (no region), -2 (sumW <= 1e-20), or NULL */
int exa_hip_sample_points(ExaHipRenderer *, const float *points /* n x 3 */, uint64_t n,
                          const int32_t *channels, int32_t numChannels, int32_t flags, float fill,
                          float *values, float *gradients, int32_t *status,
                          int32_t pointersAreDevice, void *hipStream, int32_t async);
/* the field on a uniform grid of dims[0] x dims[1] x dims[2] cell centres of the box [lo, hi] (finite, hi > lo and
 * dims >= 1 on every axis): per axis p = lo + (float(i) + 0.5f) * ((hi - lo) / float(n)) in float32, nothing contracted,
 * then the world mapping if flags = EXA_SAMPLE_WORLD_SPACE (the only flag).  out[(z*ny + y)*nx + x] (64-bit index, x
 * fastest), fill where the status would be < 0: bit for bit what exa_hip_sample_points gives at those positions. */
int exa_hip_resample(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                     int32_t channel, int32_t flags, float fill,
                     float *out /* dims[0]*dims[1]*dims[2] floats */, int32_t dstIsDevice, void *hipStream, int32_t async);

/* ---- iso-surface extraction: the surface field == iso of one channel on a caller-chosen uniform lattice, as an indexed
 * triangle mesh without duplicate vertices, consistently oriented, in a fixed order (two runs give the same bytes).  New
 * relative to the reference, which only renders iso-surfaces implicitly.  Marching tetrahedra on the six-tetrahedra (Kuhn)
 * split of every lattice cube along the diagonal (0,0,0)-(1,1,1): no ambiguous cases, and the split is translation
 * invariant, so neighbouring cubes agree on every shared face diagonal and the surface is watertight by construction. ----
 *
 * Lattice.  lo, hi, dims (each >= 2 here) and flags as for exa_hip_resample: lattice point (i,j,k) lies at
 * P = lo + (float(i) + 0.5f) * ((hi - lo) / float(n)) per axis, and its value V is exactly what
 * exa_hip_resample(lo, hi, dims, channel, flags & EXA_SAMPLE_WORLD_SPACE, fill = NaN) returns there in the handle's current
 * basis_form.  Linear index L = (k*ny + j)*nx + i.  At most 2^31 - 1 lattice points.
 *
 * Valid cubes.  Cube (i,j,k), i < nx-1, j < ny-1, k < nz-1, is valid if all 8 corner values are finite; an invalid cube
 * emits nothing.  inside(v) = V(v) >= iso; iso must be finite.
 *
 * Tetrahedra.  Six per valid cube, one per permutation (a,b,c) of the axes in lexicographic order 012, 021, 102, 120, 201,
 * 210, with the vertices v0 = cube origin, v1 = v0 + e_a, v2 = v1 + e_b, v3 = v2 + e_c.  Parity = inversions mod 2.
 *
 * Vertices.  Every tet edge joins lattice points p and q = p + d, d in {0,1}^3 \ {0}: seven edge kinds per lattice point,
 * coded dx + 2*dy + 4*dz.  An edge crosses if inside(p) != inside(q).  Exactly one vertex per crossing edge that belongs to
 * at least one valid cube, no others: t = (iso - V(p)) / (V(q) - V(p)), pos = P(p) + t * (P(q) - P(p)) per component in
 * float32, every operation rounded separately.  Positions are in the caller's space (the space of lo / hi), never put
 * through the world transform.  Order: ascending L(p), then ascending edge code.
 *
 * Triangles (tet-vertex indices 0..3; "x-y" = the vertex on the edge between tet vertices x and y).
 *   - one inside vertex s, or one outside vertex s: the triangle (s-o0, s-o1, s-o2), the other three vertices ascending,
 *     reversed iff parity(s,o0,o1,o2) XOR parity(perm) XOR (three inside);
 *   - two inside (a < b), two outside (c < d): the quad q = [a-c, a-d, b-d, b-c], reversed iff parity(a,b,c,d) XOR
 *     parity(perm), then the triangles (q0,q1,q2) and (q0,q2,q3).
 * Every geometric normal (B-A)x(C-A) then points toward the lower-value side.  Order: ascending L of the cube origin, then
 * the tet order, then the order above.  Zero-area triangles (a lattice value equal to iso) are kept.  Indices are int32.
 *
 * Gradients.  With EXA_SAMPLE_GRADIENT the module also keeps, per vertex, the gradient that exa_hip_sample_points(pos,
 * flags = world? | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED, fill = NaN) returns there, bit for bit (the same
 * kernel on the device vertex buffer).  The shading normal is -grad/|grad|; the normalisation is the caller's.
 *
 * Independence.  The result depends only on the scene, the lattice, channel, iso, basis_form and (world space) the
 * transform — not on the transfer function, region activity, the camera, walk, accel, brick_order, sample_patch or
 * sample_uniform.  A scene without a kd tree is refused, as the probes refuse it.  A multi-device handle runs on devices[0].
 *
 * Calls.  exa_hip_isosurface extracts synchronously on hipStream and returns the counts; the mesh stays in module-owned
 * device memory until the next extraction (also a failed one), exa_hip_isosurface_release or exa_hip_destroy.  An empty
 * surface returns 0 with zero counts.  The call needs 8 bytes of device memory per lattice point while it runs.  A lattice
 * of more than 2^31 - 1 points, more than INT32_MAX vertices or triangles, a failed allocation, a NaN or infinite iso, a
 * dim < 2, a bad channel and flag bits other than EXA_SAMPLE_WORLD_SPACE | EXA_SAMPLE_GRADIENT are errors with a message.
 * exa_hip_isosurface_read copies the mesh out: vertices numVertices x 3 floats, gradients numVertices x 3 floats (only after
 * an extraction with EXA_SAMPLE_GRADIENT), triangles numTriangles x 3 int32; a NULL pointer skips that array; host arrays,
 * or memory of the handle's first device with pointersAreDevice; an error before any extraction.
 * exa_hip_isosurface_stage_ms: the device time of the last extraction's stages in ms — lattice values, cube pass (validity
 * and triangle count per cube), point pass (mask of owned crossing edges per lattice point), scans, emit, gradients. */
int exa_hip_isosurface(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel,
                       float iso, int32_t flags, uint64_t *numVertices, uint64_t *numTriangles, void *hipStream);
int exa_hip_isosurface_read(ExaHipRenderer *, float *vertices, float *gradients, int32_t *triangles,
                            int32_t pointersAreDevice, void *hipStream);
int exa_hip_isosurface_release(ExaHipRenderer *);
int exa_hip_isosurface_stage_ms(ExaHipRenderer *, float ms[6]);

/* ---- derived flow quantities: speed, divergence, vorticity, its magnitude, the Q-criterion and helicity of the vector field
 * formed by three channels, at points, on uniform grids and as iso-surfaces.  New relative to the reference.  Formed on the
 * device from what exa_hip_sample_points returns, so that a scalar leaves the device instead of 12 floats per point. ----
 *
 * Inputs.  channels[3], each in [0, numFields), repeats allowed, and a quantity.  For a position p the region lookup is the
 * probes' lookup, done once.  For c = 0..2, v[c] is the value and J[c][k] component k of the gradient that
 * exa_hip_sample_points(p, channels, 3, world? | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED) returns for channel
 * c, bit for bit, in the handle's current basis_form (a scene marked allowEmptyCells: the form-0 sums with the poison test).
 *
 * Voxel space.  J is the Jacobian with respect to VOXEL-space coordinates, also for world-space positions, exactly as
 * EXA_SAMPLE_GRADIENT_NORMALIZED states: every quantity below is a voxel-space quantity (bringing it into world
 * space through the transform is the caller's).
 *
 * Status per point: -1 no region; -2 if any of the three channels has status -2; otherwise the region id.  Where status < 0
 * every component of the output is `fill`.
 *
 * Quantities.  All arithmetic is float32, every operation rounded separately, nothing contracted, associated exactly as
 * written; sqrtf and `/` are correctly rounded.  NaN and infinities propagate by these formulas, nothing is special-cased.
 * With w = (J21 - J12, J02 - J20, J10 - J01):
 *   EXA_DERIVED_SPEED               1 component   sqrtf((v0*v0 + v1*v1) + v2*v2)
 *   EXA_DERIVED_DIVERGENCE          1             (J00 + J11) + J22
 *   EXA_DERIVED_VORTICITY           3             w
 *   EXA_DERIVED_VORTICITY_MAGNITUDE 1             sqrtf((w.x*w.x + w.y*w.y) + w.z*w.z)
 *   EXA_DERIVED_Q                   1             d = (J00*J00 + J11*J11) + J22*J22; o = (J01*J10 + J02*J20) + J12*J21;
 *                                                 Q = -0.5f*d - o     (= -1/2 tr(J^2) = 1/2 (|Omega|^2 - |S|^2))
 *   EXA_DERIVED_HELICITY            1             (v0*w.x + v1*w.y) + v2*w.z
 *
 * Independence.  As for the probes: the result depends on the scene, the positions or the lattice, the channels and the
 * quantity, basis_form and (world space) the transform, and on nothing a frame sets; sample_patch and sample_uniform never
 * change a bit.
 *
 * exa_hip_sample_derived: out n x components, status n or NULL.  Arrays, the chunks of host arrays, the async rule,
 * multi-device handles, the refusal of a scene without a kd tree, a pending brick_order change and the loop guard's return
 * code 3 are those of exa_hip_sample_points; n == 0 does nothing.  The only flag is EXA_SAMPLE_WORLD_SPACE (the gradient
 * flags are errors here).
 * exa_hip_resample_derived: the lattice, its positions and the checks of the box and dims are those of exa_hip_resample;
 * out[((z*ny + y)*nx + x) * components + c], bit for bit what exa_hip_sample_derived gives at those positions.
 * exa_hip_isosurface_derived: the contract of exa_hip_isosurface with the lattice value V = what
 * exa_hip_resample_derived(lo, hi, dims, channels, quantity, flags, fill = NaN) returns.  One-component quantities only;
 * EXA_SAMPLE_GRADIENT is refused (a normal of a derived surface would need second derivatives).  The mesh replaces any
 * earlier mesh of either call and is read, released and timed with exa_hip_isosurface_read / _release / _stage_ms.
 * exa_hip_derived_ms: the device time of the kernels of the last exa_hip_sample_derived / exa_hip_resample_derived call,
 * summed; 0 before any call, after a refused one and after an asynchronous one.
 * Errors with a message that starts with the function's name, after which the handle stays usable: an unknown quantity, a
 * bad channel, null arrays, unknown flag bits, world space before a frame state, the box and dims errors of
 * exa_hip_resample, the lattice and size errors of exa_hip_isosurface, a non-finite iso. */
#define EXA_DERIVED_SPEED               0
#define EXA_DERIVED_DIVERGENCE          1
#define EXA_DERIVED_VORTICITY           2
#define EXA_DERIVED_VORTICITY_MAGNITUDE 3
#define EXA_DERIVED_Q                   4
#define EXA_DERIVED_HELICITY            5
#define EXA_DERIVED_QUANTITIES          6
int exa_hip_sample_derived(ExaHipRenderer *, const float *points /* n x 3 */, uint64_t n, const int32_t channels[3],
                           int32_t quantity, int32_t flags, float fill, float *out /* n x components */,
                           int32_t *status /* n, or NULL */, int32_t pointersAreDevice, void *hipStream, int32_t async);
int exa_hip_resample_derived(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                             const int32_t channels[3], int32_t quantity, int32_t flags, float fill,
                             float *out /* dims[0]*dims[1]*dims[2]*components floats */, int32_t dstIsDevice,
                             void *hipStream, int32_t async);
int exa_hip_isosurface_derived(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                               const int32_t channels[3], int32_t quantity, float iso, int32_t flags,
                               uint64_t *numVertices, uint64_t *numTriangles, void *hipStream);
int exa_hip_derived_ms(ExaHipRenderer *, float *ms);

/* ---- contour lines: the lines field == iso of one channel, or of a derived quantity, on a caller-chosen plane lattice that
 * may be oblique, for several levels at once, as indexed segments without duplicate vertices, consistently oriented, in a
 * fixed order (two runs give the same bytes).  The 2D sibling of exa_hip_isosurface; new relative to the reference, whose
 * contour planes (ExaHipFrameState.contour) exist only as shaded pixels.  Marching triangles on the split of every lattice
 * square along the diagonal (0,0)-(1,1): no ambiguous cases, and the split is translation invariant, so neighbouring
 * squares agree on every shared edge.  All arithmetic is float32, every operation rounded separately, nothing contracted. ----
 *
 * Lattice.  nu, nv >= 2, nu*nv <= 2^31 - 1, every float of the plane finite.  Lattice point (i,j) lies at
 * P = (origin + (float(i) + 0.5f) * du) + (float(j) + 0.5f) * dv per component (the association of ExaHipRays' origin);
 * linear index L = j*nu + i.  du and dv are not checked for independence: a degenerate plane gives coincident points.
 * Without EXA_SAMPLE_WORLD_SPACE the plane is in voxel space, with it in world space: the positions then go through the frame
 * state's transform exactly as the probes do it.
 *
 * Values.  V(L) is exactly what exa_hip_sample_points(P, {channel}, 1, flags & EXA_SAMPLE_WORLD_SPACE, fill = NaN) returns;
 * for exa_hip_isolines_derived what exa_hip_sample_derived(P, channels, quantity, the same flag, fill = NaN) returns
 * (one-component quantities only; EXA_SAMPLE_GRADIENT is refused, as by exa_hip_isosurface_derived).  Both in the handle's
 * current basis_form.
 *
 * Levels.  isos[0 .. numIsos), 1 <= numIsos <= EXA_ISOLINES_MAX_LEVELS, each finite, in any order, repeats allowed; each
 * level is contoured independently.  inside(v) = v >= iso.
 *
 * Valid squares.  Square (i,j), i < nu-1, j < nv-1, is valid if its four corner values are finite; an invalid square emits
 * nothing.
 *
 * Triangles.  Two per valid square, in this order: T0, the permutation (u,v): v0 = p, v1 = p + e_u, v2 = p + e_u + e_v,
 * parity 0; T1, the permutation (v,u): v0 = p, v1 = p + e_v, v2 = p + e_u + e_v, parity 1.
 *
 * Vertices.  Every triangle edge joins lattice points p and q = p + d, d in {(1,0), (0,1), (1,1)}, coded dx + 2*dy.  An edge
 * crosses if inside(V(p)) != inside(V(q)).  Exactly one vertex per crossing edge that belongs to at least one valid square,
 * no others: t = (iso - V(p)) / (V(q) - V(p)), pos = P(p) + t * (P(q) - P(p)) per component,
 * uv = ((float(i) + 0.5f) + t * float(dx), (float(j) + 0.5f) + t * float(dy)).  Positions are in the caller's space, never put
 * through the transform.  Order within a level: ascending L(p), then ascending edge code.
 *
 * Segments (triangle-vertex indices 0..2; "x-y" = the vertex on the edge between triangle vertices x and y).  A triangle
 * whose vertex s lies alone on its side emits the segment (s-o0, s-o1), o0 < o1 the other two, reversed iff
 * parity(s,o0,o1) XOR parity(triangle) XOR (s is outside).  With u pointing right and v up the >= iso side then lies to the
 * left of every segment.  Order within a level: ascending L of the square's origin, then T0 before T1.  Zero-length segments
 * (a lattice value equal to iso) are kept.  Indices are int32 and global (they address the packed vertex array).
 *
 * Levels in the output.  Level l's vertices are vertexOffsets[l] .. vertexOffsets[l+1], its segments
 * segmentOffsets[l] .. segmentOffsets[l+1]; the levels appear in the order given.  More than INT32_MAX vertices or segments
 * in all is an error.
 *
 * Gradients.  With EXA_SAMPLE_GRADIENT (exa_hip_isolines only) the module also keeps, per vertex, the gradient that
 * exa_hip_sample_points(pos, world? | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED, fill = NaN) returns there, bit
 * for bit (the same kernel on the device vertex buffer).
 *
 * Values kept.  With EXA_ISOLINES_KEEP_VALUES the nu*nv lattice values stay with the result and exa_hip_isolines_read
 * returns them: the slice image under the contours.  Without the flag a non-NULL `values` there is an error.
 *
 * Independence.  The result depends only on the scene, the plane, the channel(s) and the quantity, the levels, the flags,
 * basis_form and (world space) the transform — on nothing a frame sets, nor on walk, accel, brick_order, sample_patch or
 * sample_uniform.  Two calls give the same bytes.  A pending brick_order change is applied first.  A scene without a kd tree
 * is refused.  A multi-device handle runs on devices[0].
 *
 * Calls.  Synchronous on hipStream.  The result lives in module-owned device memory until the next extraction (also a
 * failed one), exa_hip_isolines_release or exa_hip_destroy; it is independent of the mesh of exa_hip_isosurface, neither
 * call drops the other's result.  An empty result returns 0 with zero counts.  exa_hip_isolines_read: vertices V x 3, uv
 * V x 2, gradients V x 3 (only after EXA_SAMPLE_GRADIENT), segments S x 2, both offset arrays numIsos + 1, values nu*nv
 * (values[j*nu + i]); a NULL pointer skips that array; host arrays, or memory of the handle's first device with
 * pointersAreDevice; an error before any extraction.  Errors carry a message that starts with the function's name and
 * leave the handle usable: a NULL plane or NULL levels, a non-finite float, nu or nv < 2, too many lattice points, numIsos
 * out of range, a bad channel or quantity, unknown flag bits, world space before a frame state, a failed allocation.  The
 * descent's loop guard returns 3.
 * exa_hip_isolines_stage_ms: the device time of the last extraction's stages in ms, summed over the levels — positions and
 * values, square pass (validity and segment count per square), point pass (mask of owned crossing edges per lattice point),
 * scans, emit, gradients.
 *
 * Memory.  While the values are formed: 4 bytes per lattice point for the values and 12 for the positions (the peak, 16);
 * afterwards the values and a work space of 4 bytes per point, plus the packed result.  Nothing grows with nu*nv*numIsos:
 * the levels run one after another over the shared values — a first round counts every level, a second repeats the passes
 * and emits at the level's offsets (a single level is not repeated). */
#define EXA_ISOLINES_KEEP_VALUES 16   /* flag: keep the lattice values for exa_hip_isolines_read */
#define EXA_ISOLINES_MAX_LEVELS  256
typedef struct ExaHipPlane { float origin[3], du[3], dv[3]; int32_t nu, nv; } ExaHipPlane;
int exa_hip_isolines(ExaHipRenderer *, const ExaHipPlane *, int32_t channel, const float *isos, int32_t numIsos,
                     int32_t flags, uint64_t *numVertices, uint64_t *numSegments, void *hipStream);
int exa_hip_isolines_derived(ExaHipRenderer *, const ExaHipPlane *, const int32_t channels[3], int32_t quantity,
                             const float *isos, int32_t numIsos, int32_t flags,
                             uint64_t *numVertices, uint64_t *numSegments, void *hipStream);
int exa_hip_isolines_read(ExaHipRenderer *, float *vertices /* V x 3 */, float *uv /* V x 2 */, float *gradients /* V x 3 */,
                          int32_t *segments /* S x 2 */, uint64_t *vertexOffsets /* numIsos+1 */,
                          uint64_t *segmentOffsets /* numIsos+1 */, float *values /* nu*nv */,
                          int32_t pointersAreDevice, void *hipStream);
int exa_hip_isolines_release(ExaHipRenderer *);
int exa_hip_isolines_stage_ms(ExaHipRenderer *, float ms[6]);

/* ---- connected regions: the connected components of the set field >= iso (or < iso) on the lattice the other extractions
 * use, numbered, with exact measurements per region — how many blobs (vortices of Q > threshold, clumps, voids) there are,
 * how large each is, where it lies, where its extreme values sit and what the field sums to over it.  New relative to the
 * reference.  Every output is an integer or a float bit pattern that depends on no schedule: two runs give the same bytes. ----
 *
 * Lattice and values.  lo, hi, dims and EXA_SAMPLE_WORLD_SPACE as for exa_hip_resample; dims >= 1 per axis (no cubes are
 * needed: a line or a plane of points is a lattice), nx*ny*nz <= 2^31 - 1.  Linear index L = (k*ny + j)*nx + i.  V(L) is
 * exactly what exa_hip_resample(lo, hi, dims, channel, the same flag, fill = NaN) returns in the handle's current basis_form,
 * for exa_hip_regions_derived what exa_hip_resample_derived(channels, quantity, ...) returns (one-component quantities only).
 *
 * Inside.  inside(L) = V(L) is finite and V(L) >= iso; with EXA_REGIONS_BELOW: finite and V(L) < iso.  NaN, +-Inf and
 * filled points are never inside.  iso must be finite.
 *
 * Edges.  Two inside points p and q are joined if q = p + d, d in {0,1}^3 \ {0}: the seven kinds of tetrahedron edge of the
 * Kuhn split exa_hip_isosurface uses (three axis edges, three face diagonals, the cube diagonal), a neighbourhood of 14
 * points, +-d.  With EXA_REGIONS_FACES only d in {e_x, e_y, e_z}, the 6 neighbours.  Kuhn is the default because it is the
 * connectivity of the surface: where all cubes are valid, the regions are exactly the connected pieces of
 * {interpolant >= iso} of the piecewise-linear interpolant whose level set exa_hip_isosurface emits (on a tetrahedron a
 * linear function is >= iso on a convex set that holds the tetrahedron's inside vertices, so pieces meet exactly along
 * tetrahedron edges with two inside ends) — regions and shells agree.  An edge needs no valid cube here, only two inside ends.
 *
 * Regions and labels.  A region is a connected component of that graph.  `first` is its smallest L; regions are numbered
 * 0, 1, ... by ascending `first`.  labels[L] = the number of L's region, -1 outside.
 *
 * Sum.  M = max |V| over the inside points of the call.  sumExponent s = 0 if there is no inside point or M == 0, else
 * s = 30 - e with M = f * 2^e, f in [0.5, 1) (frexpf).  q(v) = (double)v * 2^s rounded to the nearest integer, ties to even
 * (the scaling is exact in double; |q| <= 2^30).  sumFixed = the sum of q over the region in 64-bit integers, which cannot
 * overflow below 2^31 points.  The region's value sum is sumFixed * 2^-s, its integral that times the volume of a lattice
 * cell.  Per point the quantisation is at most 2^-(s+1) < 2^-31 M.  Fixed point because integer adds commute: the sum is
 * exact and the same in every reduction order, which no float atomic gives.
 *
 * min, max, argMin, argMax.  By the total order of exa_hip_histogram's value range (the ordered 32-bit key of the float
 * bits: -0.0 < +0.0); argMin / argMax = the smallest L among the region's points that hold min / max.
 * sumIndex = the sums of i, of j and of k: the centroid in lattice indices is sumIndex / points, exactly.  lo, hi: the
 * inclusive bounding box in lattice indices.
 *
 * Independence.  As for the mesh: the result depends only on the scene, the lattice, the channel(s) and the quantity, iso,
 * the flags, basis_form and (world space) the transform — on nothing a frame sets, nor on walk, accel, brick_order,
 * interleave, sample_patch or sample_uniform.  A scene without a kd tree is refused.  A multi-device handle runs on
 * devices[0].
 *
 * Calls.  Synchronous on hipStream.  The result lives in module-owned device memory until the next exa_hip_regions[_derived]
 * (also a failed one), exa_hip_regions_release or exa_hip_destroy; it is independent of the mesh of exa_hip_isosurface and
 * of the lines of exa_hip_isolines, none of the three calls drops another's result.  Zero regions is not an error.
 * exa_hip_regions_read: labels numPoints, regions numRegions, values numPoints (only after EXA_REGIONS_KEEP_VALUES; without
 * the flag a non-NULL `values` is an error); a NULL pointer skips that array; host arrays, or memory of the handle's first
 * device with pointersAreDevice; an error before any extraction.  Errors carry a message that starts with the function's
 * name and leave the handle usable: a NULL lo, hi, dims or channels, a non-finite iso or box float, dims < 1, too many
 * points, a bad channel or quantity, a quantity of more than one component, unknown flag bits, world space before a frame
 * state, a failed allocation.  A loop guard (the kd descent's, the union-find's) returns 3.
 * exa_hip_regions_stage_ms: device ms of the last call's stages — values, init (inside test, count, M), merge (the unions),
 * flatten (every point to its root, roots counted), rank (scans, numbering), stats (labels and measurements).
 *
 * Memory.  While the call runs: 4 bytes per lattice point for the values and 4 for the labels, which hold the union-find's
 * parent links until the numbering replaces them in place (a root's number passes through the root's own slot, no second
 * array), 8 bytes per block of 256 points for the scans, and 16 bytes per region for the min / max keys.  Afterwards: the
 * labels, 88 bytes per region, and the values if kept. */
#define EXA_REGIONS_KEEP_VALUES 16   /* flag: keep the lattice values for exa_hip_regions_read */
#define EXA_REGIONS_BELOW       32   /* flag: inside(v) = v < iso instead of v >= iso */
#define EXA_REGIONS_FACES       64   /* flag: join along the three axis edges only (6 neighbours) instead of the Kuhn edges (14) */
typedef struct ExaHipRegion {
  uint64_t points;            /* lattice points of the region */
  int64_t  sumFixed;          /* sum of q(V) over the region, see Sum */
  uint64_t sumIndex[3];       /* sum of i, of j, of k */
  int32_t  lo[3], hi[3];      /* inclusive bounding box in lattice indices */
  uint32_t first;             /* smallest linear index L of the region */
  uint32_t argMin, argMax;    /* smallest L among the points that hold min / max */
  float    min, max;
} ExaHipRegion;               /* 88 bytes */
int exa_hip_regions(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel,
                    float iso, int32_t flags, uint64_t *numRegions, uint64_t *numInside, int32_t *sumExponent, void *hipStream);
int exa_hip_regions_derived(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                            const int32_t channels[3], int32_t quantity, float iso, int32_t flags,
                            uint64_t *numRegions, uint64_t *numInside, int32_t *sumExponent, void *hipStream);
int exa_hip_regions_read(ExaHipRenderer *, int32_t *labels /* numPoints */, ExaHipRegion *regions /* numRegions */,
                         float *values /* numPoints */, int32_t pointersAreDevice, void *hipStream);
int exa_hip_regions_release(ExaHipRenderer *);
int exa_hip_regions_stage_ms(ExaHipRenderer *, float ms[6]);

/* ---- basins: one feature per local maximum of the set field >= iso (or per minimum of field < iso), shallow ones merged
 * away — a watershed segmentation with prominence merging.  Where one threshold leaves every vortex (clump, halo) in one
 * connected region, the basins split that region peak by peak; minDepth says how far a peak must stand out of the highest
 * pass to a neighbour to count as a feature of its own.  New relative to the reference.  Every output is an integer or a
 * float bit pattern that depends on no schedule: two runs give the same bytes. ----
 *
 * Lattice, values, inside, edges.  Exactly as for exa_hip_regions, with its flags (EXA_SAMPLE_WORLD_SPACE,
 * EXA_REGIONS_KEEP_VALUES, EXA_REGIONS_BELOW, EXA_REGIONS_FACES): L = (k*ny + j)*nx + i, V(L) what exa_hip_resample (or
 * exa_hip_resample_derived for a one-component quantity) returns with fill = NaN, inside(L) = V finite and V >= iso (BELOW:
 * V < iso), iso finite; edges join inside points p and p +- d, d in {0,1}^3 \ {0} (FACES: the 6 axis neighbours).
 *
 * Height and order.  h(L) = the ordered 32-bit key of V(L): bits ^ (sign ? 0xffffffff : 0x80000000); with EXA_REGIONS_BELOW
 * its complement, so that the call finds basins of minima and everything below reads the same.  p > q ("p is greater") iff
 * h(p) > h(q), or h(p) == h(q) and L(p) < L(q): a strict total order on the points.
 *
 * Ascent.  up(p) = the greatest among p and its inside neighbours.  A point with up(p) == p is a peak; peak(p) is the fixed
 * point of up from p (links rise strictly: no cycles).  A raw basin is the set of inside points with one peak.  On a plateau
 * the tie-break makes several raw basins of depth 0, which any minDepth > 0 merges.
 *
 * Merging, in rounds.  minDepth >= 0, not NaN; +INFINITY is allowed.  Components start as the raw basins; peak(C) is the
 * greatest point of C.  In a round, every edge (p, q) whose ends lie in different components has the height
 * hs = min(h(p), h(q)); each component A with such an edge takes the neighbour component B with the greatest 64-bit word
 * hs << 32 | (0xffffffff - L(peak(B))) — the highest pass, ties to the smaller peak index.  saddle(A) = the float whose key
 * is that hs; depth(A) = float32(V(peak A) - saddle), with BELOW float32(saddle - V(peak A)): one float32 subtraction,
 * always >= 0.  A links to B iff depth(A) < minDepth and peak(B) > peak(A).  All links of a round are made at once and
 * chains are followed to their end (links rise strictly: no cycles); the components of the next round are the unions.
 * Rounds repeat until one makes no link; `rounds` counts those that made one.  With minDepth == 0 none does.  At the end
 * every component that still has a neighbour has depth >= minDepth.  With minDepth = +INFINITY the components are exactly
 * the regions of exa_hip_regions with the same flags (unless a depth overflows to +Inf, which is not < +INFINITY).
 *
 * Numbering and table.  Basins are numbered 0, 1, ... by ascending L of their peak; labels[L] = the number, -1 outside.
 * points, sumFixed (with the sumExponent rule of the regions: M over all inside points of the call), sumIndex, lo, hi, argMin,
 * argMax, min, max as in ExaHipRegion; the peak is argMax, with BELOW argMin.  first = the smallest L of the basin.
 * neighbour = the number of the basin across the highest pass after the last round, -1 if there is none; saddle = that
 * pass, NaN without a neighbour; depth = the depth at that pass, +INFINITY without a neighbour.
 * numRawBasins = the number of peaks, numBasins = the number of components at the end.
 *
 * Calls, independence, errors.  As for the regions (synchronous; the result lives until the next exa_hip_basins[_derived],
 * also a failed one, exa_hip_basins_release or exa_hip_destroy; a multi-device handle runs on devices[0]; a scene without a
 * kd tree is refused): the mesh, the lines, the regions, the critical points and the basins never drop one another's
 * result.  Zero basins is not an error.  Errors carry a message that starts with the function's name and leave the handle
 * usable: those of the regions, and a NaN or negative minDepth.  A loop guard returns 3: the kd descent's, a chain of links
 * longer than numPoints, more rounds than numRawBasins (every round but the last removes a component).
 * exa_hip_basins_stage_ms: device ms of the last call's stages — values, ascent (inside test, up links and their
 * resolution), passes (all rounds' pass kernels), links (all rounds' link, jump and merge kernels), rank (the scans and
 * numberings of the peaks and of the basins), stats (labels and measurements).
 *
 * Memory.  While the call runs: 4 bytes per lattice point for the values and 4 for the labels, which hold the up links,
 * then the peak, then the component of every point until the numbering replaces it in place; 8 bytes per block of 256
 * points for the scans; 20 bytes per raw basin (its peak, its link, its final number, the 64-bit word of its pass) and 16
 * bytes per basin for the min / max keys.  Afterwards: the labels, 96 bytes per basin, and the values if kept. */
typedef struct ExaHipBasin {
  uint64_t points;            /* lattice points of the basin */
  int64_t  sumFixed;          /* sum of q(V) over the basin, see Sum of the regions */
  uint64_t sumIndex[3];       /* sum of i, of j, of k */
  int32_t  lo[3], hi[3];      /* inclusive bounding box in lattice indices */
  uint32_t first;             /* smallest linear index L of the basin */
  uint32_t argMin, argMax;    /* smallest L among the points that hold min / max */
  float    min, max;
  int32_t  neighbour;         /* the basin across the highest pass, -1 if none */
  float    saddle;            /* the value of that pass, NaN if none */
  float    depth;             /* |V(peak) - saddle|, +INFINITY if none */
} ExaHipBasin;                /* 96 bytes, no padding */
int exa_hip_basins(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel, float iso,
                   float minDepth, int32_t flags, uint64_t *numBasins, uint64_t *numRawBasins, uint64_t *numInside,
                   int32_t *sumExponent, int32_t *rounds, void *hipStream);
int exa_hip_basins_derived(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                           const int32_t channels[3], int32_t quantity, float iso, float minDepth, int32_t flags,
                           uint64_t *numBasins, uint64_t *numRawBasins, uint64_t *numInside, int32_t *sumExponent,
                           int32_t *rounds, void *hipStream);
int exa_hip_basins_read(ExaHipRenderer *, int32_t *labels /* numPoints */, ExaHipBasin *basins /* numBasins */,
                        float *values /* numPoints */, int32_t pointersAreDevice, void *hipStream);
int exa_hip_basins_release(ExaHipRenderer *);
int exa_hip_basins_stage_ms(ExaHipRenderer *, float ms[6]);

/* ---- histogram and value range of one channel's cells: the exact histogram of the cell values by cell count and by
 * volume, the value range, the cell counts per level and the NaN / empty / out-of-range counts, optionally inside an integer
 * voxel box.  New relative to the reference, whose viewer left the hook unbuilt (exa/viewer.cpp:1274-1276, setValueRange /
 * setHistogram(computeHistogram(scalarField)) commented out).  One streaming pass over the channel on the device. ----
 *
 * Cell slots.  The call considers every slot (b, i) of every brick b of the scene, i < size.x*size.y*size.z, x fastest; the
 * slot's value is scalars[channelOffset[channel] + begin_b + i], addressed in 64 bits.  Every brick slot is counted: a scene
 * whose bricks share cells counts them once per brick.
 *
 * Box.  box = lo.xyz, hi.xyz in voxel coordinates, NULL = everything.  A slot is considered if its cell centre lies in the
 * half-open box: per axis 2*box_lo <= 2*(lower + idx*2^level) + 2^level < 2*box_hi, in 64-bit integers.  box_lo == box_hi on
 * an axis is an empty box: all zeros, no error.  box_lo > box_hi is an error.
 *
 * Classes, in this order.  empty: the scene is marked allowEmptyCells and the value equals EXA_EMPTY_CELL_POISON_VALUE;
 * nan: the value is NaN; under: v < lo; over: v > hi; binned: everything else, with
 * t = (v - lo) * (float(numBins) / (hi - lo)) in float32, every operation rounded separately, bin = min(numBins - 1, (int)t).
 * +-Inf are under / over and count for min / max.  The call adds 1 to cells[bin] and, with volume != NULL, 8^level to
 * volume[bin] (a level-L cell is 8^L finest voxels).  Counts are integers: the result is exact.
 *
 * Arguments.  Errors with a message: lo or hi not finite, lo >= hi; hi - lo or float(numBins) / (hi - lo) not finite in
 * float32; numBins > EXA_HIST_MAX_BINS or < 0; cells == NULL with numBins > 0; a bad channel; a brick level outside 0..31.
 * With volume != NULL the call is refused if the sum over all bricks of cells * 8^level does not fit 64 bits.
 *
 * Range only.  With numBins == 0, lo / hi / cells / volume are ignored, under = over = 0 and every non-empty non-NaN slot is
 * binned: the pass a caller runs first to choose lo and hi.
 *
 * min / max.  Over the considered, non-empty, non-NaN values (under and over included), under the total order in which
 * -0.0 < +0.0 (the sign-flip map of the bit pattern to an ordered uint32): the returned bits do not depend on the order in
 * which the values arrive.  +INFINITY / -INFINITY if there is no such value.
 *
 * Independence.  The result depends only on the scene, channel, lo, hi, numBins and the box — not on the transfer function,
 * region activity, the frame state, basis_form, brick_order, interleave or any other option; two calls give the same bytes.
 * A pending brick_order change is applied first, as render and the probes do.  The call never looks at regions and works on
 * scenes without a kd tree.  A multi-device handle runs it on devices[0].  Synchronous on hipStream; all outputs are host
 * memory.  A failed call leaves the handle usable. */
#define EXA_HIST_MAX_BINS   4096
#define EXA_HIST_MAX_LEVELS 32
typedef struct ExaHipFieldStats {
  uint64_t slots;                     /* cell slots considered: = empty + nan + under + over + binned */
  uint64_t empty, nan, under, over, binned;
  uint64_t levelCells[EXA_HIST_MAX_LEVELS]; /* non-empty considered slots (NaN included) by brick level */
  float    min, max;                  /* over considered, non-empty, non-NaN values; +INFINITY / -INFINITY if there is none */
} ExaHipFieldStats;
int exa_hip_histogram(ExaHipRenderer *, int32_t channel, float lo, float hi, int32_t numBins,
                      const int32_t box[6] /* lo.xyz, hi.xyz in voxel coordinates; NULL = everything */,
                      uint64_t *cells /* numBins */, uint64_t *volume /* numBins, or NULL */,
                      ExaHipFieldStats *stats /* or NULL */, void *hipStream);
/* the device time of the last exa_hip_histogram's kernel in ms (0 after a call with an empty box, or before any) */
int exa_hip_histogram_ms(ExaHipRenderer *, float *ms);

/* ---- profiles and phase plots: the points of a lattice binned by one or two keys (a field, a derived quantity, the radius
 * about a centre, a coordinate, or the labels of exa_hip_regions / exa_hip_basins), with the count, the exact sums and the
 * min / max of up to four other quantities per bin, optionally weighted — the mean pressure inside every vortex, the fall-off
 * of a field with radius, the joint distribution of two quantities, the mean of one field binned by another, as a table of
 * a few kilobytes instead of a lattice per quantity.  New relative to the reference.  Every output is an integer or a float
 * bit pattern that depends on no schedule: two runs give the same bytes. ----
 *
 * Lattice and positions.  lo, hi, dims (each >= 1, nx*ny*nz <= 2^31 - 1) and EXA_SAMPLE_WORLD_SPACE as for exa_hip_resample.
 * Linear index L = (k*ny + j)*nx + i.  P(L) is the lattice position in the caller's space, per axis
 * lo + (float(i) + 0.5f) * ((hi - lo) / float(n)) in float32, nothing contracted: what exa_hip_resample forms before any world
 * mapping.
 *
 * Sources.  EXA_SOURCE_CHANNEL: V(L) = what exa_hip_resample(lo, hi, dims, channels[0], the same flag, fill = NaN) returns,
 * bit for bit, in the handle's current basis_form.  EXA_SOURCE_DERIVED: what exa_hip_resample_derived(channels, quantity, ...)
 * returns (one-component quantities only).  EXA_SOURCE_RADIUS: d = P - centre per component, sqrtf((d.x*d.x + d.y*d.y) +
 * d.z*d.z), every operation rounded separately.  EXA_SOURCE_COORDINATE: P[channels[0]], channels[0] in 0..2.  The last two
 * are formed in the kernels from (i, j, k) and take no memory.  The fields a kind does not name are ignored.  Identical
 * channel / derived sources are evaluated once.
 *
 * Bins.  B = axes[0].numBins (x axes[1].numBins), bin index b1 * axes[0].numBins + b0, 1 <= B <= EXA_PROFILE_MAX_BINS.
 * Uniform axis (edges == NULL, labels == NULL): exa_hip_histogram's rule, t = (v - lo) * (float(numBins) / (hi - lo)) in
 * float32, every operation rounded separately, bin = min(numBins - 1, (int)t); under: v < lo, over: v > hi; lo and hi finite,
 * lo < hi, hi - lo and float(numBins) / (hi - lo) finite in float32.  Edges axis: numBins + 1 strictly ascending finite
 * floats; bin b holds edges[b] <= v < edges[b+1], the last bin also v == edges[numBins]; under: v < edges[0], over:
 * v > edges[numBins] — logarithmic or any other spacing, exactly; no transcendental function is evaluated on the device.
 * Label axis (labels != NULL, the first axis only; the axis' source is ignored): bin = labels[L], numBins = the number of
 * labels, a label < 0 puts the point outside.  A label >= numBins is an error, found on the device: the call fails with a
 * message that names the smallest such L and returns no result.  labels is host memory, or with EXA_PROFILE_LABELS_DEVICE
 * memory of the handle's first device (what exa_hip_regions_read hands out with pointersAreDevice).
 *
 * Classes, tested in this order per lattice point.  outside: the label is < 0.  invalid: a key value is NaN, or the weight,
 * a value or a term (below) is not finite.  under / over: the first axis, in axis order, on which the key is out of range
 * takes the count; +-Inf keys are under / over.  binned: everything else.  points = the sum of all of them.
 *
 * Per bin.  count.  With a weight w the terms are w and float32(w * v_f), one float32 product, nothing contracted: sumWeight
 * accumulates q(w), sums[f] q(w * v_f).  Without a weight the term is v_f and sums[f] accumulates q(v_f).  A point whose
 * product overflows float32 is invalid (w and v_f are finite, their term is not).  mins[f] / maxs[f] over the unweighted v_f
 * by the ordered 32-bit key of exa_hip_histogram's value range (-0.0 < +0.0); +INFINITY / -INFINITY in an empty bin.
 * q is the Sum rule of exa_hip_regions, per series (the weight's, then each value's): M = max |term| over the binned points of
 * the call; exponent s = 0 if there is no binned point or M == 0, else s = 30 - e with M = f * 2^e, f in [0.5, 1);
 * q(v) = (double)v * 2^s rounded to the nearest integer, ties to even, summed in 64-bit integers.  A series' sum is
 * fixed * 2^-s; stats.weightExponent and stats.valueExponent[f] are the s (0 for a series the call does not have).
 *
 * Outputs.  Host memory: count B, sumWeight B, sums numValues x B, mins / maxs numValues x B (both or neither; neither skips
 * the keys).  sumWeight is given exactly when there is a weight.  stats.ldsTable says which variant of the accumulate pass
 * ran (1: the table privatised in LDS per workgroup; 0: atomics to the table in HBM); the choice hangs on B and numValues
 * alone and does not change a byte of the result.
 *
 * Independence.  The result depends only on the scene, the lattice, the axes, values and weight, basis_form and (world space)
 * the transform — on nothing a frame sets, nor on walk, accel, brick_order, interleave, sample_patch or sample_uniform.
 *
 * Calls.  Synchronous on hipStream.  A multi-device handle runs on devices[0]; a pending brick_order change is applied
 * first.  Whatever exa_hip_resample[_derived] refuses for a channel / derived source (no kd tree, world space before a frame
 * state, a bad channel or quantity) is refused here with this function's name in front.  Further errors, each with a message
 * that starts with the function's name and leaves the handle usable: a NULL lo, hi, dims, axes or count; a box that is not
 * finite with lo < hi; dims < 1; too many points; numAxes not 1 or 2; labels on the second axis; numValues outside
 * 0..EXA_PROFILE_MAX_VALUES or NULL values / sums with numValues > 0; an unknown source kind, a coordinate axis outside 0..2,
 * a centre that is not finite; a quantity of more than one component; numBins < 1, the range errors of exa_hip_histogram,
 * edges that are not finite or not strictly ascending; B out of range; sumWeight without a weight or a weight without it;
 * only one of mins / maxs; unknown flag bits; a label >= numBins; a failed allocation.  The kd descent's loop guard returns 3.
 * exa_hip_profile_stage_ms: device ms of the last call's stages — values (the resampled sources), classify, accumulate,
 * finish.
 *
 * Memory.  While the call runs: 4 bytes per lattice point and distinct channel / derived source, 4 per point for the bin
 * indices, 4 per point for labels that came from the host; per bin 8 for the count, 8 per series (weight, values) and 8 per
 * value with mins / maxs; 4 per edge.  Nothing is kept afterwards. */
#define EXA_SOURCE_CHANNEL    0  /* V = exa_hip_resample(lo, hi, dims, channels[0], world?, fill = NaN)            */
#define EXA_SOURCE_DERIVED    1  /* V = exa_hip_resample_derived(channels, quantity, ...); one-component only      */
#define EXA_SOURCE_RADIUS     2  /* d = P - centre per component; sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z)              */
#define EXA_SOURCE_COORDINATE 3  /* P[channels[0]], channels[0] in 0..2                                            */
typedef struct ExaHipSource { int32_t kind; int32_t channels[3]; int32_t quantity; float centre[3]; } ExaHipSource;

typedef struct ExaHipProfileAxis {
  ExaHipSource   source;     /* ignored when labels != NULL */
  int32_t        numBins;
  float          lo, hi;     /* uniform bins, used when edges == NULL && labels == NULL */
  const float   *edges;      /* numBins + 1 strictly ascending finite floats, or NULL (host memory) */
  const int32_t *labels;     /* numPoints labels, or NULL; first axis only */
} ExaHipProfileAxis;

typedef struct ExaHipProfileStats {
  uint64_t points, outside, invalid, under[2], over[2], binned;  /* points = the sum of the others */
  int32_t  weightExponent, valueExponent[4];                     /* the regions' sumExponent rule, per series */
  int32_t  ldsTable;                                             /* 1: the accumulate pass kept the table in LDS */
} ExaHipProfileStats;

#define EXA_PROFILE_LABELS_DEVICE 16   /* flag: axes[0].labels is memory of the handle's first device */
#define EXA_PROFILE_MAX_VALUES    4
#define EXA_PROFILE_MAX_BINS      (1 << 24)

int exa_hip_profile(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3], int32_t flags,
                    const ExaHipProfileAxis *axes, int32_t numAxes /* 1 or 2 */,
                    const ExaHipSource *values, int32_t numValues /* 0..4 */, const ExaHipSource *weight /* or NULL */,
                    uint64_t *count /* B */, int64_t *sumWeight /* B; NULL iff weight == NULL */,
                    int64_t *sums /* numValues x B */, float *mins, float *maxs /* numValues x B, or both NULL */,
                    ExaHipProfileStats *stats /* or NULL */, void *hipStream);
int exa_hip_profile_stage_ms(ExaHipRenderer *, float ms[4]);   /* values, classify, accumulate, finish */

/* ---- distance transform: per point of the lattice the exact Euclidean distance to the nearest point of a set — the points
 * where a field is >= iso (or < iso), the points that are not, or the points that carry a label — and which point that is.
 * Wall distance (the distance to the nearest point without data), the distance from a surface field == iso for shell and
 * boundary-layer profiles (exa_hip_profile takes labels), thickness and clearance of the blobs of exa_hip_regions /
 * exa_hip_basins, the Voronoi partition labels[nearest].  New relative to the reference.  Every output is an integer or a
 * float bit pattern that depends on no schedule: two runs give the same bytes. ----
 *
 * Lattice and values.  lo, hi, dims, EXA_SAMPLE_WORLD_SPACE, L = (k*ny + j)*nx + i and the limit of 2^31 - 1 points as for
 * exa_hip_regions.  V(L) is exactly what exa_hip_resample(lo, hi, dims, channel, the same flag, fill = NaN) returns, for
 * exa_hip_distance_derived what exa_hip_resample_derived(channels, quantity, ...) returns (one-component quantities only).
 * inside(L) is the regions' rule: V(L) is finite and V(L) >= iso, with EXA_DISTANCE_BELOW finite and V(L) < iso.  NaN, +-Inf
 * and filled points are never inside; iso must be finite.  So iso = -FLT_MAX with EXA_DISTANCE_TO_OUTSIDE gives the distance
 * to the nearest point without data (every point with a finite value is inside, the targets are the others).
 * exa_hip_distance_mask: inside(L) = (labels[L] == label), with label == -1 (labels[L] >= 0).  It reads no field, needs no kd
 * tree and ignores EXA_SAMPLE_WORLD_SPACE; lo, hi and dims give only the spacing.
 *
 * Targets.  The target set T is the inside points, with EXA_DISTANCE_TO_OUTSIDE the points that are not inside.
 * EXA_DISTANCE_SIGNED does both: a point that is not inside gets + its distance to the inside set, an inside point gets
 * - its distance to the set of the others (nearest likewise); it excludes EXA_DISTANCE_TO_OUTSIDE.  Points beyond the lattice
 * do not exist and are never targets.
 *
 * Spacing and terms.  h_a = (hi_a - lo_a) / float(n_a) as exa_hip_resample forms it, so distances are in the caller's space
 * (also with EXA_SAMPLE_WORLD_SPACE).  term_a(d) = o*o with o = h_a * float(|d|).  Everything is float32, every operation is
 * rounded separately, nothing is contracted.
 *
 * Passes (the contract).  X: a(i,j,k) is the target i' of row (j,k) with the least |i - i'|, of two the smaller i', -1 if the
 * row holds none; gx = term_x(i - a), +INF without one.  Y: b(i,j,k) is the j' that minimises gx(i,j',k) + term_y(j - j'), of
 * several the smallest j'; gy is that minimum.  Z: c is the k' that minimises gy(i,j,k') + term_z(k - k'), of several the
 * smallest k'; d2 is that minimum.  nearest(L) is the linear index of (a(i, b(i,j,c), c), b(i,j,c), c).  A minimum of +INF
 * (no target in reach of the pass, or a sum that overflows) has no index.
 *
 * Theorem.  d2 equals the minimum over all targets (i',j',k') of (term_x(i-i') + term_y(j-j')) + term_z(k-k') in float32:
 * rounding is monotone, so x -> fl(x + c) is non-decreasing and commutes with min, pass by pass.  The separable result is the
 * global brute-force minimum bit for bit.
 *
 * Reach.  maxDistance must be > 0 and may be +INF; limit = maxDistance*maxDistance, one float32 product.  A point with
 * d2 > limit, or with no target at all (d2 = +INF), has dist = +INF (-INF on the inside branch of EXA_DISTANCE_SIGNED) and
 * nearest = -1.  A target's own dist is +0.0 and its nearest is itself.  A finite maxDistance bounds the work: a pass stops
 * looking once its term alone exceeds the limit.
 *
 * Outputs.  dist = sqrtf(d2), correctly rounded (with the sign above); nothing transcendental runs on the device.  nearest is
 * a linear index L or -1.  stats: points = nx*ny*nz; inside = the number of inside points; reached = the number of points
 * with a finite dist; maxDistance = the largest finite |dist|, 0 if there is none (an integer max on the bits of a
 * non-negative float, so two runs give the same bytes).
 *
 * Independence.  The bytes depend only on the scene, the lattice, the channel(s) and the quantity (or the labels and the
 * label), iso, maxDistance, the flags, basis_form and (world space) the transform — on nothing a frame sets, nor on walk,
 * accel, brick_order, interleave, sample_patch or sample_uniform, nor on whether the arrays are host or device memory.
 *
 * Calls.  Synchronous on hipStream; a pending brick_order change is applied first; a multi-device handle runs on devices[0].
 * dist and nearest are host memory, or memory of the handle's first device with pointersAreDevice; a NULL nearest skips that
 * array and its gathers.  labels is host memory, or memory of the handle's first device with EXA_DISTANCE_LABELS_DEVICE.
 * Whatever exa_hip_resample[_derived] refuses (no kd tree, world space before a frame state, a bad channel or quantity) the
 * field calls refuse with their own name in front; the mask call needs none of that.  Further errors, each with a message
 * that starts with the function's name and leaves the handle usable: a NULL lo, hi, dims, channels or dist; NULL labels; a
 * box float that is not finite or a spacing that is not; dims < 1; too many points; a non-finite iso; a quantity of more than
 * one component; maxDistance NaN or <= 0; EXA_DISTANCE_SIGNED together with EXA_DISTANCE_TO_OUTSIDE; unknown flag bits
 * (EXA_DISTANCE_LABELS_DEVICE applies to the mask call only, EXA_DISTANCE_BELOW to the field calls only); label < -1; a failed
 * allocation.  The kd descent's loop guard returns 3.
 * exa_hip_distance_stage_ms: device ms of the last call's stages — values (the resampled field or the labels, and the inside
 * test), rows, columns (y and z), finish; with EXA_DISTANCE_SIGNED the sums over both target sets.
 *
 * Memory.  While the call runs: 21 bytes per lattice point (a, b, c, gy and d2 of 4 bytes each and the inside byte; the
 * values share d2's room and labels from the host share c's), and with host pointers 4 more for dist and 4 for nearest.
 * Nothing is kept afterwards. */
#define EXA_DISTANCE_BELOW          32   /* inside(v) = finite and v <  iso (default: finite and v >= iso; the regions' rule) */
#define EXA_DISTANCE_TO_OUTSIDE     64   /* targets = the points that are NOT inside (default: the inside points) */
#define EXA_DISTANCE_SIGNED        128   /* both: + distance to the inside set at non-inside points, - distance to the
                                            non-inside set at inside points; excludes EXA_DISTANCE_TO_OUTSIDE */
#define EXA_DISTANCE_LABELS_DEVICE 256   /* exa_hip_distance_mask: labels is memory of the handle's first device */
typedef struct ExaHipDistanceStats { uint64_t points, inside, reached; float maxDistance; int32_t pad; } ExaHipDistanceStats;

int exa_hip_distance(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3], int32_t channel,
                     float iso, float maxDistance, int32_t flags, float *dist /* n */, int32_t *nearest /* n, or NULL */,
                     ExaHipDistanceStats *stats /* or NULL */, int32_t pointersAreDevice, void *hipStream);
int exa_hip_distance_derived(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                             const int32_t channels[3], int32_t quantity, float iso, float maxDistance, int32_t flags,
                             float *dist /* n */, int32_t *nearest /* n, or NULL */, ExaHipDistanceStats *stats /* or NULL */,
                             int32_t pointersAreDevice, void *hipStream);
int exa_hip_distance_mask(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                          const int32_t *labels /* n */, int32_t label, float maxDistance, int32_t flags,
                          float *dist /* n */, int32_t *nearest /* n, or NULL */, ExaHipDistanceStats *stats /* or NULL */,
                          int32_t pointersAreDevice, void *hipStream);
int exa_hip_distance_stage_ms(ExaHipRenderer *, float ms[4]);   /* values, rows, columns (y and z), finish */

/* ---- streamlines: field lines of the vector field formed by three channels, integrated from seed points with classical
 * RK4 at a fixed step and handed out as packed polylines.  An extraction, not the viewer's animation: the reference's tracer
 * (exa_hip_reset_tracer / exa_hip_advance_tracer) takes one step per rendered frame, forward only, at a trace count and
 * length fixed at reset, and finds a position's region with a ray through the volume BVH, which is refit to the transfer
 * function — its traces end where the volume is merely invisible.  Here a whole line is integrated on the device in one
 * call, in either or both directions, and nothing a frame sets changes it. ----
 *
 * Space.  Voxel space only.  World-space seeds are not offered: the components of a vector field have no defined mapping
 * under the voxelSpaceTransform.
 *
 * Evaluation E(q).  Exactly what exa_hip_sample_points(q, channels, 3, flags = 0) returns: one region lookup by the rules of
 * the probes' block (closed root box, `>= split` goes right, no backtracking, closed-domain test at the leaf), then the three
 * channels in the order given, in the handle's current basis_form (a scene marked allowEmptyCells: the form-0 sums with the
 * poison test).  The outcome is LEFT if the lookup gives -1 (outside, a gap, a NaN or infinite coordinate); otherwise NOVALUE
 * if any channel has status -2; otherwise the velocity v = (v0, v1, v2).  With EXA_STREAM_NORMALIZE,
 * s = sqrtf((v0*v0 + v1*v1) + v2*v2), every operation rounded separately and the square root correctly rounded; if !(s > 0)
 * or s is not finite the outcome is STAGNANT, otherwise the direction is d = v / s per component by true division.  Without
 * the flag d = v.
 *
 * One direction from the seed p0.  hs = +step forward, -step backward.  The seed is vertex 0 of its direction.  E(p0) failing
 * ends the direction with that reason and no further vertices.  Otherwise, up to maxSteps times, in float32 with nothing
 * contracted:
 *     k1 = hs*d(p)   k2 = hs*d(p + .5f*k1)   k3 = hs*d(p + .5f*k2)   k4 = hs*d(p + k3)
 *     pn = p + (1/6.f) * (((k1 + 2.f*k2) + 2.f*k3) + k4)
 * (the reference's step, exabrick.cu:1531-1574).  A failing stage ends the direction with that stage's reason: the stage order
 * decides, within a stage the order is lookup, channels, speed.  pn bit-equal to p in all three components ends it STAGNANT.
 * Then E(pn): a failure ends the direction with that reason and pn is NOT appended; otherwise pn is appended and its d is the
 * next step's k1.  After maxSteps appended vertices the reason is MAXSTEPS.  So every vertex other than a failed seed has a
 * value in all three channels.
 *
 * A line.  The backward direction's vertices in reverse (farthest first), the seed once, the forward direction's vertices.
 * seedVertex[i] = number of backward vertices; line i is vertices offsets[i] .. offsets[i+1]; offsets[n] = numVertices.  A
 * seed whose own evaluation fails is a one-vertex line (the seed as given) with that reason in every requested direction.
 * reasons[2*i] is the backward, reasons[2*i+1] the forward direction's; EXA_STREAM_END_NONE for a direction not requested.
 * velocities (only after an extraction with EXA_STREAM_VELOCITIES) holds the raw v, never normalised, of every vertex; NaN
 * for a failed seed.
 *
 * Independence.  The bytes depend only on the scene, the seeds, channels, step, maxSteps, flags and basis_form — not on the
 * transfer function, region activity, the frame state, walk, accel, brick_order, interleave, the number of seeds in the call
 * or their order: line i of a batch equals the one-seed call.  A pending brick_order change is applied first.  A multi-device
 * handle runs on devices[0].  A scene without a kd tree is refused, as the probes refuse it.
 *
 * Calls.  exa_hip_streamlines extracts synchronously on hipStream; seeds are host memory.  The lines stay in module-owned
 * device memory until the next extraction (also a failed one), exa_hip_streamlines_release or exa_hip_destroy.  n == 0
 * returns 0 with zero vertices.  Errors with a message, after which the handle stays usable: step not finite or <= 0;
 * maxSteps < 1 or > EXA_STREAM_MAX_STEPS; no direction flag; unknown flag bits; a channel outside [0, numFields); more than
 * INT32_MAX vertices in all; a failed allocation; the descent's loop guard (return code 3, as the probes).
 * exa_hip_streamlines_read copies the last extraction out (host arrays, or memory of the handle's first device with
 * pointersAreDevice); a NULL pointer skips that array; an error before any extraction, after a release, and for velocities
 * without EXA_STREAM_VELOCITIES.  exa_hip_streamlines_ms: the device time of the last extraction's two kernels, summed.
 *
 * Memory.  Count, then emit: the integration is deterministic, so it runs twice — once storing per direction only the
 * number of vertices and the reason, then, after a scan of the counts on the host, again storing every vertex at its packed
 * position.  Peak device memory: the packed result (12 bytes per vertex, 24 with velocities, and 28 bytes per seed for
 * offsets, seedVertex, reasons and counts) plus 12 bytes per seed for the seeds while the call runs; nothing grows with
 * n * maxSteps. */
#define EXA_STREAM_FORWARD     1
#define EXA_STREAM_BACKWARD    2   /* both: one polyline through the seed */
#define EXA_STREAM_NORMALIZE   4   /* step along v/|v|: `step` is an arc length in voxel units */
#define EXA_STREAM_VELOCITIES  8   /* also keep v at every vertex */
#define EXA_STREAM_MAX_STEPS   1048576   /* the cap of maxSteps (per direction) */
/* why a direction ended */
#define EXA_STREAM_END_NONE     0  /* direction not requested */
#define EXA_STREAM_END_MAXSTEPS 1
#define EXA_STREAM_END_LEFT     2  /* a position with probe status -1 (outside, a gap, NaN / infinite) */
#define EXA_STREAM_END_NOVALUE  3  /* probe status -2 in one of the three channels */
#define EXA_STREAM_END_STAGNANT 4
int exa_hip_streamlines(ExaHipRenderer *, const float *seeds /* n x 3, voxel space, host */, uint64_t n,
                        const int32_t channels[3], float step, int32_t maxSteps, int32_t flags,
                        uint64_t *numVertices, void *hipStream);
int exa_hip_streamlines_read(ExaHipRenderer *, float *vertices /* numVertices x 3 */, float *velocities /* same, or NULL */,
                             uint64_t *offsets /* n + 1 */, uint32_t *seedVertex /* n */, int32_t *reasons /* n x 2: backward, forward */,
                             int32_t pointersAreDevice, void *hipStream);
int exa_hip_streamlines_release(ExaHipRenderer *);
int exa_hip_streamlines_ms(ExaHipRenderer *, float *ms);   /* device time of the last extraction's kernels, summed */

/* ---- line integral convolution (LIC): the dense picture of where a vector field goes on a cut plane.  Per pixel of the
 * plane lattice of exa_hip_isolines the field line of the in-plane part of three channels is followed backward and forward
 * from the pixel's centre, and the noise of the pixels it passes is averaged (box filter).  The dense sibling of
 * exa_hip_streamlines: one launch integrates and reduces in registers, nothing of size pixels x steps is stored. ----
 *
 * Space.  Voxel space only, for the reason exa_hip_streamlines states.  All float arithmetic is float32, every operation
 * rounded separately, nothing contracted; sqrtf and `/` are correctly rounded.
 *
 * Lattice coordinates.  A position is c = (a, b) in pixel units; pixel (i, j) has its centre at (float(i) + 0.5f,
 * float(j) + 0.5f); p(c) = (origin + a*du) + b*dv per component, the association of exa_hip_isolines' lattice points, so a
 * centre is that lattice's point.  Output index j*nu + i; nu, nv >= 1, nu*nv <= 2^31 - 1.
 *
 * Plane metric, formed once: G11 = (du.x*du.x + du.y*du.y) + du.z*du.z, G12 (du.dv) and G22 (dv.dv) likewise,
 * det = G11*G22 - G12*G12.  A plane with a non-finite float, or with det not finite or !(det > 0), is refused.
 *
 * Evaluation E2(c).  E(p(c)) is the E(q) of exa_hip_streamlines without EXA_STREAM_NORMALIZE: LEFT, NOVALUE, or v.  Then
 * r1 = (v0*du.x + v1*du.y) + v2*du.z, r2 the same with dv; va = (G22*r1 - G12*r2) / det, vb = (G11*r2 - G12*r1) / det;
 * s = sqrtf(va*va + vb*vb).  If !(s > 0) or s is not finite the outcome is STAGNANT (a field normal to the plane
 * stagnates); otherwise d = (va/s, vb/s).  The lines are the field lines of the in-plane component; `step` is an arc length
 * in pixels.
 *
 * One direction from the centre c0.  hs = +step forward, -step backward.  If E2(c0) fails, both directions end with that
 * reason.  Otherwise, up to halfLength times:
 *     k1 = hs*d(c)   k2 = hs*d(c + .5f*k1)   k3 = hs*d(c + .5f*k2)   k4 = hs*d(c + k3)
 *     cn = c + (1/6.f) * (((k1 + 2.f*k2) + 2.f*k3) + k4)
 * per component (the streamlines' step); a failing stage ends the direction with its reason.  cn bit-equal to c ends it
 * STAGNANT.  !(cn.a >= 0.f && cn.a < float(nu) && cn.b >= 0.f && cn.b < float(nv)) ends it EXA_LIC_END_IMAGE.  Then E2(cn):
 * a failure ends the direction with that reason and cn is not counted; otherwise the sample N((int)cn.a, (int)cn.b) is
 * added, the direction's count goes up by one and d(cn) is the next k1.  After halfLength samples the reason is MAXSTEPS.
 *
 * Noise.  N(ix, iy) = noise[iy*nu + ix], or with noise == NULL the built-in hash, in uint32 arithmetic:
 *     h = ix*0x9E3779B1 + iy*0x85EBCA77 + seed*0xC2B2AE3D
 *     h ^= h>>16; h *= 0x7FEB352D; h ^= h>>15; h *= 0x846CA68B; h ^= h>>16; N = h>>24
 * ((ix, iy, seed) = (1,0,0) -> 109, (0,1,0) -> 196, (3,5,7) -> 178, (66,44,1) -> 71).
 *
 * Outputs per pixel (a NULL pointer skips that array).  The centre's E fails (LEFT / NOVALUE): sum 0, count 0, lic = speed =
 * fill, both reasons that reason.  The centre stagnates: sum = N(i, j), count 1, both reasons STAGNANT.  Otherwise sum =
 * N(i, j) + the forward samples + the backward samples, count = 1 + both directions' counts, one reason per direction
 * (reasons[2*k] backward, reasons[2*k+1] forward).  In the last two cases lic = float(sum) / float(count), one true division,
 * and speed = sqrtf((v0*v0 + v1*v1) + v2*v2) at the centre.  The sums are integers of at most 8193 * 255: exact in uint32 and
 * in float32 whatever the order they are added in.
 *
 * Independence.  The bytes depend only on the scene, the plane, channels, step, halfLength, the noise or the seed, fill and
 * basis_form — not on anything a frame sets, nor on walk, accel, brick_order, interleave, lic_lanes, lic_patch or the other
 * options, nor on whether the arrays are host or device memory.
 *
 * Calls.  Synchronous on hipStream; a pending brick_order change is applied first; a scene without a kd tree is refused; a
 * multi-device handle runs on devices[0].  The arrays, the noise included, are host memory, or memory of the handle's first
 * device with pointersAreDevice; host arrays pass through one device buffer of the call (up to 25 bytes per pixel).  Errors
 * with a message that starts with "exa_hip_lic: ", after which the handle stays usable: a NULL plane or NULL channels; a
 * non-finite plane float, the det rule, nu or nv < 1, more than 2^31 - 1 points; a channel outside [0, numFields); step not
 * finite or <= 0; halfLength outside 1 .. EXA_LIC_MAX_STEPS; any flag bit (a non-finite fill is allowed); a failed
 * allocation; the descent's loop guard (return code 3, as the probes).  exa_hip_lic_ms: the device time of the last call's
 * kernels, summed; 0 before any call and after a refused one. */
#define EXA_LIC_MAX_STEPS 4096     /* the cap of halfLength (per direction) */
#define EXA_LIC_END_IMAGE 5        /* a direction ended because the line left the image; the other reasons are EXA_STREAM_END_* */
int exa_hip_lic(ExaHipRenderer *, const ExaHipPlane *, const int32_t channels[3], float step, int32_t halfLength,
                const uint8_t *noise /* nu*nv, or NULL: the built-in hash */, uint32_t seed, int32_t flags /* 0 */, float fill,
                float *lic /* nu*nv */, uint32_t *sum, uint32_t *count, float *speed, int32_t *reasons /* nu*nv x 2: backward, forward */,
                int32_t pointersAreDevice, void *hipStream);
int exa_hip_lic_ms(ExaHipRenderer *, float *ms);

/* ---- flow map and stretch: the Lagrangian view of a vector field.  From every point of a lattice a particle is carried along
 * the field of three channels for the time T = numSteps * step; the flow map is where it ends, and the stretch is the largest
 * eigenvalue of the Cauchy-Green tensor of the map's differences, from which the finite-time Lyapunov exponent (FTLE) follows:
 * the ridges of that field are the separatrices, the separation (forward) and attachment (backward) lines and the edges of
 * vortices.  One launch integrates with only the end state kept in registers, a second one runs the stencil; nothing of size
 * points x numSteps is stored. ----
 *
 * Space.  Voxel space only, for the reason exa_hip_streamlines states.  All float arithmetic is float32, every operation
 * rounded separately, nothing contracted; `/` and sqrtf are correctly rounded; no transcendental function runs on the device.
 *
 * Lattice.  lo, hi, dims as for exa_hip_resample, dims >= 1 per axis, nx*ny*nz <= 2^31 - 1: point (i,j,k) lies at
 * P = lo + (float(i) + 0.5f) * ((hi - lo) / float(n)) per axis.  Linear index L = (k*ny + j)*nx + i, n = nx*ny*nz points.
 *
 * Flow map.  end(L), steps(L), reasons(L) are taken from the line that exa_hip_streamlines(seeds = {P(L)}, channels, step,
 * maxSteps = numSteps, flags = the one direction) returns — its "One direction" paragraph, without EXA_STREAM_NORMALIZE, so
 * `step` is a time: end(L) is the last vertex of that line bit for bit, steps(L) its vertex count minus one, reasons(L) that
 * direction's reason.  A seed whose own evaluation fails gives end = P(L), steps = 0 and its reason.
 *
 * Validity.  valid(L) = reasons(L) is EXA_STREAM_END_MAXSTEPS or EXA_STREAM_END_STAGNANT: a particle that stagnates stays where
 * it is for the rest of the time.
 *
 * Stencil.  Per axis a with n_a >= 2, m_a is the neighbour of L at index max(i_a - 1, 0) and p_a the one at min(i_a + 1, n_a - 1):
 * central differences inside, one-sided ones on the lattice's faces.  Column a of the deformation gradient is
 *     F[c][a] = (end_c(p_a) - end_c(m_a)) / (P_a(p_a) - P_a(m_a))          c = 0, 1, 2
 * and the column of an axis with n_a == 1 is zero: a plane or a line of points gives the 2-D / 1-D stretch of the 3-D
 * displacement.  stretch(L) = fill unless L and every stencil point of L are valid.
 *
 * Tensor.  C_ab = (F[0][a]*F[0][b] + F[1][a]*F[1][b]) + F[2][a]*F[2][b] for the six entries ab = 00, 11, 22, 01, 02, 12.
 *
 * Largest eigenvalue.  Five sweeps of cyclic Jacobi on the symmetric a = C, each sweep the rotations (p,q) = (0,1), (0,2),
 * (1,2), r the third index.  A rotation is skipped if and only if a_pq == 0.0f; otherwise, in this order,
 *     theta = (a_qq - a_pp) / (2.f*a_pq)
 *     t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta*theta + 1.f))
 *     c = 1.f / sqrtf(t*t + 1.f)        s = t*c
 *     a_pp' = a_pp - t*a_pq             a_qq' = a_qq + t*a_pq
 *     a_rp' = c*a_rp - s*a_rq           a_rq' = s*a_rp + c*a_rq          a_pq' = 0
 * (t*a_pq is one product, used twice).  Then m = a_00; if (a_11 > m) m = a_11; if (a_22 > m) m = a_22; stretch(L) = m.  NaN and
 * infinities propagate by these formulas, nothing is special-cased.
 *
 * FTLE.  Never formed on the device (logf is not correctly rounded, and the outputs here are byte-exact).
 * FTLE = log(stretch) / (2 * |T|), T = numSteps * step, formed in double and rounded to float; fill where stretch is fill.  The
 * binding, the host library and exaRender form it so.
 *
 * Independence.  As the streamlines: the bytes depend only on the scene, the lattice, channels, step, numSteps, the direction,
 * fill and basis_form — not on anything a frame sets, nor on walk, accel, brick_order, interleave, flowmap_patch or the other
 * options, nor on whether the arrays are host or device memory; end, steps and reasons of point L equal the one-point call.
 *
 * Calls.  Synchronous on hipStream; a pending brick_order change is applied first; a scene without a kd tree is refused; a
 * multi-device handle runs on devices[0]; a NULL output pointer skips that array.  The arrays are host memory, or memory of the
 * handle's first device with pointersAreDevice.  Errors with a message that starts with "exa_hip_flowmap: ", after which the
 * handle stays usable: NULL lo, hi, dims or channels; the box and dims errors of exa_hip_resample, more than 2^31 - 1 points; a
 * channel outside [0, numFields); step not finite or <= 0; numSteps outside 1 .. EXA_STREAM_MAX_STEPS; neither or both
 * direction flags, unknown flag bits (a non-finite fill is allowed); a failed allocation; the descent's loop guard (return
 * code 3, as the probes).
 *
 * Memory.  One device buffer of the call: with host pointers every array asked for, and end and reasons also when only the
 * stretch is asked for (at most 24 bytes per point); with device pointers only what the stretch reads and the caller did not
 * ask for (end 12, reasons 4: at most 16 bytes per point, nothing when end and reasons are given or stretch is NULL).
 * exa_hip_flowmap_ms: the device time of the last call's two stages, integrate and stretch; both 0 before any call and after a
 * refused one. */
#define EXA_FLOWMAP_FORWARD  1      /* exactly one of the two */
#define EXA_FLOWMAP_BACKWARD 2
int exa_hip_flowmap(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                    const int32_t channels[3], float step, int32_t numSteps, int32_t flags, float fill,
                    float *end /* n x 3 */, uint32_t *steps /* n */, int32_t *reasons /* n */, float *stretch /* n */,
                    int32_t pointersAreDevice, void *hipStream);
int exa_hip_flowmap_ms(ExaHipRenderer *, float ms[2]);   /* integrate, stretch */

/* ---- critical points: the topology of a vector field.  Where the flow of three channels, sampled on the lattice the other
 * extractions use, stagnates, and what kind of point each zero is: source, sink, one of the two saddles, each plain or
 * spiralling.  The points seed separatrices (exa_hip_streamlines), explain a LIC image and find stagnation and attachment
 * points.  New relative to the reference.  Every output is an integer or a float / double bit pattern that depends on no
 * schedule: placement is by prefix sums, the counters are integer sums, two runs give the same bytes. ----
 *
 * Arithmetic.  All arithmetic float32 unless stated, every operation rounded separately, nothing contracted; `/` is correctly
 * rounded; every expression below is written in the association the kernels use; sums written "x = x + y" over the corners
 * m = 0..7 run in ascending m from x = 0.0f.  NaN and infinities propagate by the formulas, nothing is special-cased or clamped.
 *
 * Lattice and values.  lo, hi, dims and EXA_SAMPLE_WORLD_SPACE as for exa_hip_resample; dims >= 2 per axis (cells are
 * needed), nx*ny*nz <= 2^31 - 1.  step[a] = (hi[a] - lo[a]) / float(dims[a]).  Linear index L = (k*ny + j)*nx + i.
 * V_c(L), c = 0, 1, 2, is exactly what exa_hip_resample(lo, hi, dims, channels[c], the same flag, fill = NaN) returns in the
 * handle's current basis_form.  Channels may repeat.
 *
 * Cells.  Cell (i,j,k) exists for i < nx-1, j < ny-1, k < nz-1; its number is the linear index L of its origin (i,j,k).  Its
 * corner m = dx + 2 dy + 4 dz is the lattice point (i+dx, j+dy, k+dz), with values V_c(m).  A cell is valid if all 24 corner
 * floats are finite.  stats.cells = (nx-1)(ny-1)(nz-1), stats.invalidCells = the cells that are not valid.
 *
 * Candidates.  A valid cell is a candidate if for each component c the minimum lo_c and the maximum hi_c of V_c over the 8
 * corners satisfy  lo_c <= 0 && 0 <= hi_c && lo_c < hi_c.  A cell in which a component is constant is never a candidate (the
 * all-zero interior of a body).  stats.candidates counts them.
 *
 * Trilinear interpolant.  For s = (s0, s1, s2):  u_a[0] = 1.f - s_a, u_a[1] = s_a.  Per corner m = (dx,dy,dz):
 *     wxy = u_0[dx] * u_1[dy]        wxz = u_0[dx] * u_2[dz]        wyz = u_1[dy] * u_2[dz]        w = wxy * u_2[dz]
 * and per component c, over the corners in ascending m,
 *     F_c    = F_c    + w * V_c(m)
 *     J_c0   = J_c0   + (dx ? wyz * V_c(m) : -(wyz * V_c(m)))
 *     J_c1   = J_c1   + (dy ? wxz * V_c(m) : -(wxz * V_c(m)))
 *     J_c2   = J_c2   + (dz ? wxy * V_c(m) : -(wxy * V_c(m)))
 * F = T(s) and J = dT/ds (J_ca = dT_c/ds_a), accumulated corner by corner.
 *
 * Newton iteration.  s = (0.5, 0.5, 0.5); exactly `iterations` steps (1 .. EXA_CRITICAL_MAX_ITERATIONS), no early exit.  A
 * step forms F and J at s, then solves J delta = -F by Cramer's rule with the cofactors
 *     A00 = J11*J22 - J12*J21      A01 = J02*J21 - J01*J22      A02 = J01*J12 - J02*J11
 *     A10 = J12*J20 - J10*J22      A11 = J00*J22 - J02*J20      A12 = J02*J10 - J00*J12
 *     A20 = J10*J21 - J11*J20      A21 = J01*J20 - J00*J21      A22 = J00*J11 - J01*J10
 *     det = (A00*J00 + A01*J10) + A02*J20
 *     delta_a = -(((Aa0*F0 + Aa1*F1) + Aa2*F2) / det)              s_a = s_a + delta_a
 * A singular matrix divides by zero and gives infinities or NaN.  det is the first row of the cofactors times the first column
 * of J, the expansion the numerator of delta_0 has: in a cell whose corners with dx = 0 are all zero (the layer around a body
 * of zeros below x0) the first step has F_c = 0.5 * J_c0 exactly, so delta_0 = -0.5 and s_0 = 0 exactly, where the second step
 * finds F = 0 and det = 0: 0/0, nonFinite.
 *
 * Acceptance.  With the final s and the delta of the last step, tested in this order:
 *     nonFinite     some s_a or delta_a is not finite
 *     leftCell      not (0 <= s_a < 1) on some axis a; in the last cell of an axis (i_a == n_a - 2) s_a <= 1 is allowed.  A
 *                   root on a face between two cells so belongs to one of them by rule
 *     notConverged  lastStep = max(max(|delta_0|, |delta_1|), |delta_2|) > tolerance (tolerance finite, in (0, 1])
 * A rejected candidate is counted in exactly one of stats.nonFinite, leftCell, notConverged; the others are found.  At most
 * one point per cell is found: a cell that holds several zeros gives the one the iteration runs to, or none.  Duplicates
 * are not merged: the interpolants of two cells differ outside their shared face, so both may accept a root close to it.
 *
 * Output.  One ExaHipCriticalPoint per found candidate, in ascending cell number:
 *     local = s                  position[a] = lo[a] + ((float(i_a) + 0.5f) + s_a) * step[a]   (the lattice's space)
 *     lastStep as above          jacobian[c*3 + a] = J_ca / step[a], J formed once more at the final s
 * Classification in double from the float32 `jacobian`, j = (double)jacobian:
 *     P = -((j[0] + j[4]) + j[8])
 *     Q = ((j[0]*j[4] - j[1]*j[3]) + (j[0]*j[8] - j[2]*j[6])) + (j[4]*j[8] - j[5]*j[7])
 *     R = -((j[0]*(j[4]*j[8] - j[5]*j[7]) - j[1]*(j[3]*j[8] - j[5]*j[6])) + j[2]*(j[3]*j[7] - j[4]*j[6]))
 *     D = (27.0*(R*R) + (4.0*((P*P)*P) - 18.0*(P*Q))*R) + (4.0*((Q*Q)*Q) - (P*P)*(Q*Q))
 * invariants = (P, Q, R) of the characteristic polynomial lambda^3 + P lambda^2 + Q lambda + R; discriminant = D, the negative
 * of the cubic's discriminant.  The Routh column is e = (1, P, (P*Q - R)/P, R); an entry counts as positive iff it is > 0 (a NaN
 * is not); n+ = the number of k in 0..2 at which e_k and e_k+1 differ in that.  type = n+ (bits 0-1: the eigenvalues with a
 * positive real part: 0 sink, 3 source, 1 and 2 the two saddles) | EXA_CRITICAL_SPIRAL if D > 0 (a complex pair) |
 * EXA_CRITICAL_DEGENERATE if P == 0, P*Q - R == 0, R == 0 or one of P, (P*Q - R)/P, R is not finite; n+ is then still what the
 * rule gives.
 *
 * Probe (EXA_CRITICAL_PROBE).  The point probe runs on the positions while they are on the device: probe[(p*3 + c)*4 + 0] is
 * the value, [.. + 1..3] the gradient and probeStatus[p*3 + c] the status of channel channels[c] at position(p), bit for bit
 * what exa_hip_sample_points(positions, channels, 3, the world flag | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED,
 * fill = NaN) returns: the residual of the real field at the lattice's root and the real field's voxel-space Jacobian.
 *
 * Independence.  As for the regions: the result depends only on the scene, the lattice, the channels, iterations,
 * tolerance, the flags, basis_form and (world space) the transform — on nothing a frame sets, nor on walk, accel,
 * brick_order, interleave, sample_patch or sample_uniform.  A scene without a kd tree is refused.  A multi-device handle runs
 * on devices[0].
 *
 * Calls.  Synchronous on hipStream.  The result lives in module-owned device memory until the next exa_hip_critical_points
 * (also a failed one), exa_hip_critical_points_release or exa_hip_destroy; it is independent of the mesh, the lines and the
 * regions: none of the four calls drops another's result.  Zero points is not an error.  numPoints and stats (or NULL) are
 * written by a call that succeeds, and zeroed by one that fails.  exa_hip_critical_points_read: points numPoints records,
 * probe numPoints x 12 floats, probeStatus numPoints x 3 (both only after EXA_CRITICAL_PROBE; without the flag a non-NULL
 * pointer is an error); a NULL pointer skips that array; host arrays, or memory of the handle's first device with
 * pointersAreDevice; an error before any extraction.  Errors carry a message that starts with the function's name and leave
 * the handle usable: a NULL lo, hi, dims or channels, the box and dims errors of exa_hip_resample, dims < 2, too many points,
 * a bad channel, iterations outside 1 .. EXA_CRITICAL_MAX_ITERATIONS, a tolerance that is not finite or outside (0, 1],
 * unknown flag bits, world space before a frame state, a failed allocation.  The kd descent's loop guard returns 3.
 * exa_hip_critical_points_stage_ms: device ms of the last call's stages — values (three lattices), cells (validity,
 * candidates, counts), scans (both rounds, with the compaction of the candidate list), refine (the iteration), emit (records
 * and classification), probe.
 *
 * Memory.  While the call runs: 12 bytes per lattice point for the three lattices, 1 bit per lattice point for the candidate
 * marks and 8 bytes per block of 256 points for the scans; 24 bytes per candidate (its cell 4, s and lastStep 16, its class 4)
 * and 8 bytes per block of 256 candidates.  Afterwards: 104 bytes per found point, and with the probe 60 more (48 + 12), and
 * another 60 while the probe runs (the positions 12, the probe's own values 12 and gradients 36). */
#define EXA_CRITICAL_MAX_ITERATIONS 32
#define EXA_CRITICAL_SPIRAL         4    /* type: a complex pair of eigenvalues (D > 0) */
#define EXA_CRITICAL_DEGENERATE     8    /* type: an entry of the Routh column is zero or not finite */
#define EXA_CRITICAL_PROBE          16   /* flag: probe the real field at the found positions */
typedef struct ExaHipCriticalPoint {
  uint32_t cell;              /* linear index L of the cell's origin */
  int32_t  type;              /* n+ | EXA_CRITICAL_SPIRAL | EXA_CRITICAL_DEGENERATE */
  float    local[3];          /* s */
  float    position[3];       /* lo[a] + ((float(i_a) + 0.5f) + s[a]) * step[a], the lattice's space */
  float    lastStep;          /* max |delta| of the last iteration */
  float    jacobian[9];       /* [c*3 + a] = (dT_c/ds_a) / step[a]: per unit of the lattice's space */
  double   invariants[3];     /* P, Q, R of lambda^3 + P lambda^2 + Q lambda + R */
  double   discriminant;      /* D */
} ExaHipCriticalPoint;        /* 104 bytes */
typedef struct ExaHipCriticalStats {
  uint64_t cells, invalidCells, candidates, found, nonFinite, leftCell, notConverged;
} ExaHipCriticalStats;
int exa_hip_critical_points(ExaHipRenderer *, const float lo[3], const float hi[3], const int32_t dims[3],
                            const int32_t channels[3], int32_t iterations, float tolerance, int32_t flags,
                            uint64_t *numPoints, ExaHipCriticalStats *stats /* or NULL */, void *hipStream);
int exa_hip_critical_points_read(ExaHipRenderer *, ExaHipCriticalPoint *points, float *probe /* n x 12, or NULL */,
                                 int32_t *probeStatus /* n x 3, or NULL */, int32_t pointersAreDevice, void *hipStream);
int exa_hip_critical_points_release(ExaHipRenderer *);
int exa_hip_critical_points_stage_ms(ExaHipRenderer *, float ms[6]);   /* values, cells, scans, refine, emit, probe */

/* ---- projections: the field itself reduced along lines of sight — per pixel the sum, the number, the maximum and the
 * minimum of the samples of one channel along a ray, as plain arrays: column density (sum*dt), the mean along the ray
 * (sum/count), maximum- and minimum-intensity images.  New relative to the reference, whose only images are RGBA8 pictures
 * through a transfer function.  One kernel forms the positions and reduces in registers; nothing of size pixels x samples
 * exists. ----
 *
 * Spaces.  Without EXA_SAMPLE_WORLD_SPACE the rays are in voxel space.  With it they are in world space: every sample
 * position goes through the voxelSpaceTransform of the frame state (xfmPoint) exactly as exa_hip_sample_points does it, and
 * tmin / dt are world-space lengths.  A frame state must have been set.
 *
 * Positions.  Pixel (x, y), x < width, y < height; all arithmetic in float32, every operation rounded separately, nothing
 * contracted, in exactly this association:
 *     sx = float(x) + 0.5f                       sy = float(y) + 0.5f
 *     o  = (org + sx*orgDu) + sy*orgDv           d  = (dir + sx*dirDu) + sy*dirDv          per component
 *     with EXA_PROJECT_NORMALIZE: s = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z), correctly rounded, then d = d / s per component
 *         by true division; a pixel with !(s > 0) or a non-finite s has no samples
 *     t_i = tmin + (float(i) + 0.5f) * dt        for i = 0 .. numSamples-1
 *     p_i = o + t_i * d                          per component
 * One struct covers orthographic cameras (dirDu = dirDv = 0), pinhole cameras (orgDu = orgDv = 0) and anything affine in
 * between.  Without the flag t and dt are multiples of |d|; with it they are arc lengths.
 *
 * Sample.  Sample i of a pixel is exactly what exa_hip_sample_points(p_i, {channel}, 1, flags & EXA_SAMPLE_WORLD_SPACE)
 * returns, in the handle's current basis_form (a scene marked allowEmptyCells: the form-0 sums with the poison test): the
 * same lookup and the same sums, bit for bit.  A sample is valid when its status is >= 0.
 *
 * Reduction.  Per pixel over the valid samples in ascending i: count = their number; sum = a double started at 0.0 with
 * sum += (double)v per valid sample — invalid samples are skipped, not added as zero; the caller forms sum*dt and sum/count.
 * vmax starts at -INFINITY, vmin at +INFINITY, maxIndex at -1, and per valid sample
 *     if (v > vmax) { vmax = v; maxIndex = i; }        if (v < vmin) vmin = v;
 * so a NaN value counts, poisons sum and never becomes max or min; of equal maxima the first wins (+0.0 does not replace
 * -0.0).  Output index y*width + x; a NULL output pointer skips that array.
 *
 * Independence.  The bytes depend only on the scene, the ExaHipRays struct, the channel, the flags, basis_form and (world
 * space) the transform — not on the transfer function, region activity, the camera of the frame state, walk, accel,
 * brick_order, interleave, sample_patch or sample_uniform (which here, too, only selects whether a wave descends the tree
 * and reads a shared region's headers together); two calls give the same bytes.  A pending brick_order change is applied
 * first.  A scene without a kd tree is refused, as the probes refuse it.  A multi-device handle runs on devices[0].
 *
 * Calls.  Synchronous on hipStream.  Outputs are host arrays, which pass through the handle's bounded staging buffer tile
 * by tile of the image, or with pointersAreDevice memory of the handle's first device.  Errors with a message, after which
 * the handle stays usable: a NULL struct; a non-finite float in it; dt <= 0; numSamples < 1 or > EXA_PROJECT_MAX_SAMPLES;
 * tmin + float(numSamples) * dt not finite in float32; width < 1, height < 1 or width*height > 2^31 - 1; a bad channel; flag
 * bits other than EXA_SAMPLE_WORLD_SPACE | EXA_PROJECT_NORMALIZE; world space before any frame state; the descent's loop
 * guard (return code 3, as the probes).  exa_hip_project_ms: the device time of the last call's kernel launches, summed
 * (0 before any call and after a refused one). */
#define EXA_PROJECT_NORMALIZE    4        /* rays run along d/|d|: t and dt are arc lengths */
#define EXA_PROJECT_MAX_SAMPLES  1048576  /* cap of numSamples */
typedef struct ExaHipRays {
  float   org[3], orgDu[3], orgDv[3];   /* origin of pixel (x,y) */
  float   dir[3], dirDu[3], dirDv[3];   /* direction of pixel (x,y) */
  int32_t width, height;
  float   tmin, dt;
  int32_t numSamples;
} ExaHipRays;
int exa_hip_project(ExaHipRenderer *, const ExaHipRays *, int32_t channel, int32_t flags,
                    double *sum, uint32_t *count, float *vmax, float *vmin, int32_t *maxIndex,
                    int32_t pointersAreDevice, void *hipStream);
int exa_hip_project_ms(ExaHipRenderer *, float *ms);   /* device time of the last call's kernel(s) */

/* ---- iso-crossings along rays: where along each ray of an image the field of one channel first crosses a value — the
 * depth t, the position, the value and the gradient there, and the number of crossings of the whole ray, as plain arrays:
 * picking, depth images to composite rasterised geometry with, position and normal images without a lattice and a mesh.
 * New relative to the reference, whose implicit iso hit goes straight into an RGBA8 pixel and depends on the transfer
 * function and the region activity.  One kernel marches the ray, refines the first crossing and samples the hit in
 * registers; nothing of size pixels x samples exists. ----
 *
 * Positions.  The rays, o, d, t_i and p_i of a pixel are exactly those of exa_hip_project: the same struct, the same
 * float32 association, EXA_PROJECT_NORMALIZE and its pixels without samples (!(s > 0) or a non-finite s), and
 * EXA_SAMPLE_WORLD_SPACE as there.  These two are the only flag bits.
 *
 * Samples.  S_i is exactly what exa_hip_sample_points(p_i, {channel}, 1, flags & EXA_SAMPLE_WORLD_SPACE) returns in the
 * handle's current basis_form (a scene marked allowEmptyCells: the form-0 sums with the poison test).  A sample is usable if
 * its status is >= 0 and its value v_i is not NaN.  inside(v) = v >= iso, as in exa_hip_isosurface; iso must be finite.
 *
 * Crossings.  Index i in 1 .. numSamples-1 is a crossing if S_{i-1} and S_i are both usable and inside(v_{i-1}) !=
 * inside(v_i).  A pair separated by an unusable sample never forms a crossing, and where the volume begins no cap is
 * invented: a ray that enters the volume, or comes out of a gap or of NaN cells, already on the `>= iso` side has no crossing
 * there.  This is deliberate: the call reports where the field crosses the value, not where the data begin.
 *
 * Per pixel, for the whole ray.  crossings = the number of crossing indices; index = the smallest one, -1 if there is none;
 * side = +1 if v_{index-1} < iso (the ray enters the `>= iso` side), -1 otherwise, 0 without a crossing.
 *
 * Refinement of the first crossing.  From (ta, va) = (t_{index-1}, v_{index-1}) and (tb, vb) = (t_index, v_index), at most
 * `refine` rounds (0 .. EXA_CROSS_MAX_REFINE), float32 with every operation rounded separately:
 *     tm = 0.5f * (ta + tb);   if (tm == ta || tm == tb) stop
 *     pm = o + tm * d          per component;   the sample at pm (as S_i);   if it is not usable, stop
 *     if (inside(vm) == inside(va)) (ta, va) = (tm, vm);   else (tb, vb) = (tm, vm)
 * and after the rounds
 *     s = (iso - va) / (vb - va)        t = ta + s * (tb - ta)        position = o + t * d   per component
 * in exactly this association, as exa_hip_isosurface interpolates along an edge.  position is in the caller's space (world
 * space with the flag) and is never put through the transform.  Infinite samples propagate by these formulas (a NaN t and
 * position where inf - inf or inf / inf arises); nothing is special-cased.
 *
 * Value and gradient at the hit.  value and gradient are what exa_hip_sample_points(position, {channel}, 1, (flags &
 * EXA_SAMPLE_WORLD_SPACE) | EXA_SAMPLE_GRADIENT | EXA_SAMPLE_GRADIENT_NORMALIZED, fill) returns there: the voxel-space gradient
 * of the field; a shading normal -g/|g| is the caller's.  A pixel without a crossing has `fill` in t, position, value and
 * gradient.
 *
 * Outputs.  Index y*width + x (position, gradient: three floats there); a NULL pointer skips that array.  With
 * crossings == NULL a ray may stop at its first crossing; every other array holds the same bytes either way.
 *
 * Independence, calls and errors as exa_hip_project: the bytes depend only on the scene, the struct, the channel, iso,
 * refine, the flags, fill, basis_form and (world space) the transform — not on the transfer function, region activity, the
 * camera of the frame state, walk, accel, brick_order, interleave, sample_patch or sample_uniform; a pending brick_order
 * change is applied first; a scene without a kd tree is refused; a multi-device handle runs on devices[0].  Synchronous on
 * hipStream; host outputs pass through the staging buffer tile by tile, or with pointersAreDevice memory of the handle's
 * first device.  Refused with a message, after which the handle stays usable: everything exa_hip_project refuses of its
 * rays, channel and flags, world space before any frame state, a non-finite iso, refine outside 0 .. EXA_CROSS_MAX_REFINE; the
 * descent's loop guard returns 3.  exa_hip_raycast_iso_ms: the device time of the last call's kernel launches, summed
 * (0 before any call and after a refused one). */
#define EXA_CROSS_MAX_REFINE 32
int exa_hip_raycast_iso(ExaHipRenderer *, const ExaHipRays *, int32_t channel, float iso, int32_t refine, int32_t flags,
                        float fill,
                        float *t /* w*h */, float *position /* w*h*3 */, float *value /* w*h */, float *gradient /* w*h*3 */,
                        int32_t *index /* w*h */, int32_t *side /* w*h */, uint32_t *crossings /* w*h */,
                        int32_t pointersAreDevice, void *hipStream);
int exa_hip_raycast_iso_ms(ExaHipRenderer *, float *ms);

/* ---- the field on a surface: per triangle of a mesh the sum and the number of the samples of up to four channels at
 * quadrature points spread evenly over it, and its area-weighted normal — surface pressure on loaded geometry, force
 * (the integral of p n dA), flux through an iso-surface or a cut, the area of an iso-surface, a second channel on the mesh
 * that exa_hip_isosurface just left in device memory.  New relative to the reference.  The kernels form the positions and
 * reduce in registers; nothing of size triangles x samples exists. ----
 *
 * All arithmetic below is float32 with every operation rounded separately and nothing contracted, unless it says double.
 *
 * Mesh.  Vertices are in the caller's space: voxel space, or world space with EXA_SAMPLE_WORLD_SPACE (every sample position
 * then goes through the voxelSpaceTransform of the frame state exactly as exa_hip_sample_points does it).  Triangles are
 * vertex indices.  With EXA_SURFACE_FROM_ISOSURFACE `vertices` and `triangles` must be NULL, the two counts are ignored and
 * the mesh is the one of the last exa_hip_isosurface[_derived] of this handle, read where it lies and never copied to the
 * host; without such a mesh the call is an error; the caller passes the same space flag the extraction had.
 * numTriangles == 0 (and an empty mesh of the handle) does nothing and returns 0.
 *
 * Per triangle, with v0, v1, v2 its vertices, e1 = v1 - v0 and e2 = v2 - v0 per component:
 *     areaNormal = 0.5f * (e1.y*e2.z - e1.z*e2.y, e1.z*e2.x - e1.x*e2.z, e1.x*e2.y - e1.y*e2.x)
 * whose length is the area and whose direction is the geometric normal (B-A)x(C-A) of the iso-surface contract; non-finite
 * input propagates.  The edge lengths are sqrtf((dx*dx + dy*dy) + dz*dz), correctly rounded, of v1-v0, v2-v1 and v0-v2; L is
 * their maximum, NaN if one of them is.  A triangle is valid if its three indices lie in [0, numVertices) and L is finite.
 * One that is not has subdiv = 0, no samples, sum = +0.0 and count = 0, and areaNormal by the formula, or three NaN where an
 * index is out of range.  The subdivision n of a valid triangle: spacing == 0: n = maxN; otherwise q = L / spacing (true
 * division) and n = maxN if q >= float(maxN), else max(1, (int)ceilf(q)).  subdiv = n.
 *
 * Samples.  A valid triangle has n*n samples of equal weight, the centroids of its n*n congruent sub-triangles.  For
 * sample k = 0 .. n*n-1, with a = k / n and b = k % n as integers:
 *     a + b <  n :  fa = float(a) + T1          fb = float(b) + T1            T1 = 1.0f/3.0f (bits 0x3eaaaaab)
 *     a + b >= n :  fa = float(n-1-a) + T2      fb = float(n-1-b) + T2        T2 = 2.0f/3.0f (bits 0x3f2aaaab)
 *     b1 = fa / float(n)    b2 = fb / float(n)          (true division)
 *     p_k = (v0 + b1*e1) + b2*e2                         per component
 * Sample k of channel c is exactly what exa_hip_sample_points(p_k, channels, numChannels, flags & EXA_SAMPLE_WORLD_SPACE)
 * returns for that channel, in the handle's current basis_form (a scene marked allowEmptyCells: the form-0 sums with the
 * poison test), with one region lookup for all channels.  A sample is valid where its status is >= 0.
 *
 * Reduction, per triangle and channel; its shape is fixed, so that a wave can form it and any implementation gives the
 * same bytes.  count = the number of valid samples.  Slot l = k % 64 holds a double P_l, started at +0.0; the valid samples
 * with k % 64 == l are added to it in ascending k, P_l += (double)v_k, invalid ones are skipped.  Then, for o = 32, 16, 8, 4, 2,
 * 1 in this order, P_l = P_l + P_{l+o} for every l < o; sum = P_0.  (So a lone -0.0 gives +0.0.)  A NaN value makes a NaN
 * sum, whose payload and sign are not part of the contract.  The caller forms the mean sum/count, the integral
 * mean*|areaNormal|, the force mean*areaNormal and the flux mean_c . areaNormal.
 *
 * Outputs.  sum and count: index triangle*numChannels + c; areaNormal: three floats per triangle; subdiv: one int.  A NULL
 * output pointer skips that array.
 *
 * Independence.  The bytes depend only on the scene, the mesh, the channels, spacing, maxN, the space flag, basis_form and
 * (world space) the transform — not on anything a frame sets, nor on sample_uniform or surface_pack; two calls give the same
 * bytes.  A pending brick_order change is applied first.  A scene without a kd tree is refused.  A multi-device handle runs
 * on devices[0].
 *
 * Calls.  Synchronous on hipStream.  A host mesh: the vertices are uploaded whole for the duration of the call (12 bytes of
 * device memory per vertex); triangles and outputs pass through the handle's bounded staging buffer in chunks.  With
 * pointersAreDevice all arrays are memory of the handle's first device.  Refused with a message that starts with
 * "exa_hip_sample_triangles: ", after which the handle stays usable: numChannels outside 1 .. EXA_SURFACE_MAX_CHANNELS or a
 * bad channel; maxN outside 1 .. EXA_SURFACE_MAX_N; a spacing that is negative or not finite; flag bits other than
 * EXA_SAMPLE_WORLD_SPACE | EXA_SURFACE_FROM_ISOSURFACE; world space before any frame state; NULL mesh pointers without
 * EXA_SURFACE_FROM_ISOSURFACE or non-NULL ones with it; the flag without a mesh; counts above INT32_MAX.  The descent's loop
 * guard returns 3.  exa_hip_sample_triangles_ms: the device time of the last call's kernels, summed (0 before any call and
 * after a refused one). */
#define EXA_SURFACE_FROM_ISOSURFACE 8     /* flag: the mesh of the last exa_hip_isosurface[_derived] of this handle */
#define EXA_SURFACE_MAX_N           64    /* cap of maxN: at most 4096 samples per triangle */
#define EXA_SURFACE_MAX_CHANNELS    4
int exa_hip_sample_triangles(ExaHipRenderer *, const float *vertices /* nV x 3 */, uint64_t numVertices,
                             const int32_t *triangles /* nT x 3 */, uint64_t numTriangles,
                             const int32_t *channels, int32_t numChannels, float spacing, int32_t maxN, int32_t flags,
                             double *sum /* nT x C */, uint32_t *count /* nT x C */, float *areaNormal /* nT x 3 */,
                             int32_t *subdiv /* nT */, int32_t pointersAreDevice, void *hipStream);
int exa_hip_sample_triangles_ms(ExaHipRenderer *, float *ms);

/* tuning knobs that never change results: "tile_order" = launch sequence of the 16x16 tiles:
 * 0 row-major, 1 row-major 8x8 supertiles per XCD, 2 pseudo-random, 3 centre-out, 4 Z-order
 * (default), 5/6/7 Z-order dealt to the XCDs in chunks of 16/64/256 tiles; "accel" 0 = LBVH with restart per segment,
 * 1 = region kd-tree walked front to back (default when the scene carries one); "lbvh_build" 0 (default) = that LBVH
 * is built on the device (Morton codes, radix sort, topology level by level), 1 = the same tree built on the host;
 * "fast_sampler" 1 (default) = the surfaces pre-pass of the kd path samples through the march headers with the
 * masked-weight basis evaluation, 0 = with the literal addBasisFunctions (same sums bit for bit); "interleave" 1 (default) =
 * a DVR march of 2..4 primary channels reads a channel-interleaved copy float[cell][channel] of those fields (built on
 * the device at the first such frame) and evaluates all channels per brick visit, 0 = field by field from the arrays
 * as uploaded; "addr64" 1 = the march forms 64-bit cell / header / node addresses even where a scene is small enough for
 * 32-bit offsets from a uniform base (default 0: chosen per scene; "pack_records" 0 = the march takes region ids from the walk and loads the region
 * records, as it does in scenes whose records {first brick, brick count, level} do not fit the 32 bits of a leaf reference (default 1:
 * packed where they fit; tests); tests); "cube_records" 1 (default) = in a scene whose bricks are all cubes of one power-of-two
 * edge (exa_prep_cube_records says which) the one-channel 32-bit rope march reads 16-byte brick records with the edge as a
 * kernel argument instead of the 32-byte march headers (16 bytes of device memory per leaf-list entry, built by exa_hip_create;
 * bit-identical frames), 0 = the march headers, as in every other scene. "brick_order" 0 = the bricks' cells lie in
 * memory in the order of the brick list (the running `begin` of OptixRenderer.cpp:71-93), 1 = along a Morton curve of the
 * brick centres (re-laid on the device at the next frame; cells are only found through their brick's `begin`, so pixels
 * cannot change; environment EXA_BRICK_ORDER sets the initial value); "tile_feedback" 1 (default) = after a
 * change of view / TF / layout the next synchronous frame records every tile's longest ray and later frames launch
 * the heaviest tiles first (a frame's critical path is its longest rays), 0 = keep the static order; "wide_march" 1
 * (default) = tiles whose longest ray would outlast the rest of the frame (multi-GPU shards) march with 2 or 4 lanes
 * per ray — the walk split into depth windows, consecutive samples evaluated side by side and composited in order,
 * bit-identical pixels; up to 8 GiB of device memory for the walkers' leaf lists — 0 = never,
 * 2 / 4 = every tile with that many lanes (tests); "prepass_split" 1 (default) = in a frame with surfaces the tiles whose iso marches are
 * long (measured by the same frame that measures the tile costs) get their own pre-pass + march pipeline on a side stream,
 * beside the pre-pass + march of the other tiles (the pre-pass is bound by the latency of its longest rays, the march by
 * throughput), 0 = the whole pre-pass in front of the whole march; "ao_defer" 1 (default) = the ambient-occlusion rays of the shaded hits are traced by a launch of their own,
 * one ray per lane over a compact list of the hits, 2 = as 1 with the listed rays sorted on the device by (32x32-pixel block of the
 * hit | direction class: octant x dominant axis) before they are traced, so that a wave's 64 rays start close together and head
 * the same way (counting sort: histogram, scan, scatter; hit flags combined per hit by a last kernel), 0 = inline behind each pixel's primary ray (1 is the default); "ao_overlap" 1 = the deferred AO rays run on a side
 * stream BESIDE the march instead of in front of it: the march needs the surfaces' hit distance up front but their colour only for
 * its last operation, so it stores its pixel colour and a small kernel finishes the pixels (over the surfaces' colour, accumulation,
 * sRGB, pack: the same operations in the same order) once both are done, 0 (default: the faster one with several frames in flight) = pre-pass, AO rays, march one after the other; "stats_mode" = what exa_hip_render_stats collects: 1 (default) the
 * work counters, 2 only phase_cycles, from the shipped code plus a clock read at every phase change; "walk_probe" 1 = the
 * counting variant also records every wave's SET of visited kd nodes (128 KiB of device memory per wave) and reports its
 * size summed over the waves as walk_union_nodes (a diagnostic of how coherent the 64 walks of a wave are);
 * "sample_patch" / "sample_uniform" = the patch shape of exa_hip_resample's grid kernel (0 64x1x1, 1 16x4x1, 2 8x8x1,
 * 3 4x4x4 (default) grid points per wave) and whether its waves descend the kd tree and read a shared region's brick headers together
 * (1, default) or lane by lane (0): same values bit for bit either way;
 * "surface_pack" 1 (default) = exa_hip_sample_triangles packs triangles of at most 16 samples into shared waves (groups of
 * 1, 4 or 16 lanes per triangle), 0 = every triangle gets a wave of its own: same bytes either way;
 * "lic_lanes" 1 (default) = exa_hip_lic gives a pixel one lane, which integrates backward, then forward, 2 = a lane per pixel
 * and direction, the pair's integer sums added by a lane exchange; "lic_patch" 1 (default) = a wave's pixels form a patch 8
 * pixels wide (8 x 8, or 8 x 4 with two lanes per pixel), 0 = a row (64 x 1 / 32 x 1): same bytes in every layout;
 * "flowmap_patch" 1 (default) = a wave of exa_hip_flowmap takes a 4 x 4 x 4 patch of lattice points (an axis shorter than 4
 * gives its share to the others: 8 x 8 x 1 on a plane), 0 = 64 points along x: same bytes either way;
 * "profile_marker" N = launch an empty kernel (profileMarkerKernel) on the null stream now: a bracket in a profiler's
 * dispatch list, no effect on any frame.
 * "walk" selects how the DVR march of the kd path finds its segments: 1 = the ordered walk of the region kd-tree with a
 * 4-entry short stack in LDS (restart from the root when an entry was dropped), which skips subtrees without an active
 * region; 2 = the rope walk: every leaf carries its box and one link per face to its neighbour (64 B per leaf, built on
 * the host at the first frame that uses it), the ray goes from leaf to leaf, the reference's slab test is evaluated on
 * each leaf's own box, no stack and no restarts — and the LDS of the stack goes to a segment queue of five 16-byte entries
 * (region record, t1, the first sample's t_i, t0) instead of four 12-byte ones; inactive leaves are passed through one by one; 0 (default) = per frame: the rope walk when at least 40 % of the
 * regions are active for the volume march, else the stack walk.  Same segments, same pixels either way.
 * "basis_form" selects the association of the eight-corner sums of addBasisFunctions (programs/exabrick.cu:620-777):
 * 1 (default) = per axis — x-pairs, then y, then z, weight sums as products of per-axis sums — with fused multiply-adds
 * (49 instead of 116 floating-point operations per brick with derivatives), 0 = the reference's source order with every
 * product and sum rounded separately.  The reference binary computes neither literally (nvcc contracts a*b+c by
 * default and CMakeLists.txt passes no -fmad=false); the CPU oracle restates both operation for operation
 * (or_set_basis_form) and the kernels equal it in either.  Form 1 against form 0: |d accum| <= 1e-3, RGBA8 <= 1 LSB
 * (tests/test_basis_form.py).  Environment EXA_BASIS_FORM sets the initial value.
 * Two knobs move results within the stated float tolerance: "fast_math" 1 (default)
 * evaluates the opacity correction powf as exp2(dt*log2(x)) on the hardware
 * transcendental units (~2 ulp), 0 uses the library powf (<1 ulp); "tf_filter" 1 (default) holds the
 * transfer-function filter weight in 9-bit fixed point with 8 fractional bits, as the CUDA texture unit
 * behind the reference's tex1D<float4> fetch does (programs/exabrick.cu:147, exa/Texture.h:141-147; CUDA C
 * programming guide, "Texture Fetching", linear filtering), 0 keeps the full-precision weight. */
int exa_hip_set_option(ExaHipRenderer *, const char *key, int32_t value);

const char *exa_hip_last_error(const ExaHipRenderer * /* may be NULL: creation errors */);

#ifdef __cplusplus
}
#endif
#endif
