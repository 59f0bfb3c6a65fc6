// exa_host.h — C++ host layer above the C ABI (include/exa_hip.h).
//
// Mirrors the interface the reference's viewer programs against, so a host written
// for `exa::OptixRenderer` recompiles against `exa::Renderer`:
//   exa::ExaBricks / ScalarField / TriangleMesh / Config  (exa/ExaBricks.h, ScalarField.h,
//       TriangleMesh.h, Config.h) — same static load functions, same file formats
//   exa::Renderer   (exa/OptixRenderer.h:32-97) — same public method set and the public
//       members the viewer touches (frameState, fbSize, worldSpaceBounds, scalarFields)
// The math types stand in for the un-vendored owl::common ones (vec3f, box3f,
// interval, affine3f with xfmPoint/xfmVector/rcp).
#pragma once

#include "../../include/exa_hip.h"

#include <cmath>
#include <limits>
#include <memory>
#include <string>
#include <vector>

namespace exa {

struct vec2i { int x = 0, y = 0; vec2i() = default; vec2i(int a, int b) : x(a), y(b) {} explicit vec2i(int a) : x(a), y(a) {} };
struct vec3i { int x = 0, y = 0, z = 0; vec3i() = default; vec3i(int a, int b, int c) : x(a), y(b), z(c) {} };
struct vec3f {
  float x = 0, y = 0, z = 0;
  vec3f() = default;
  explicit vec3f(float s) : x(s), y(s), z(s) {}
  vec3f(float a, float b, float c) : x(a), y(b), z(c) {}
  explicit vec3f(const vec3i &v) : x(float(v.x)), y(float(v.y)), z(float(v.z)) {}
  float &operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
  float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};
inline vec3f operator+(vec3f a, vec3f b) { return { a.x + b.x, a.y + b.y, a.z + b.z }; }
inline vec3f operator-(vec3f a, vec3f b) { return { a.x - b.x, a.y - b.y, a.z - b.z }; }
inline vec3f operator*(vec3f a, vec3f b) { return { a.x * b.x, a.y * b.y, a.z * b.z }; }
inline vec3f operator*(float s, vec3f a) { return { s * a.x, s * a.y, s * a.z }; }
inline vec3f operator*(vec3f a, float s) { return { a.x * s, a.y * s, a.z * s }; }
inline vec3f operator/(vec3f a, float s) { return { a.x / s, a.y / s, a.z / s }; }
inline vec3f operator-(vec3f a) { return { -a.x, -a.y, -a.z }; }
inline bool operator==(vec3f a, vec3f b) { return a.x == b.x && a.y == b.y && a.z == b.z; }
inline bool operator!=(vec3f a, vec3f b) { return !(a == b); }
inline float dot(vec3f a, vec3f b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
inline float length(vec3f a) { return std::sqrt(dot(a, a)); }
inline vec3f normalize(vec3f a) { return (1.f / std::sqrt(dot(a, a))) * a; }
inline vec3f cross(vec3f a, vec3f b) { return { a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x }; }

template <typename T> struct interval {
  T lower = std::numeric_limits<T>::infinity(), upper = -std::numeric_limits<T>::infinity();
  interval() = default;
  interval(T lo, T hi) : lower(lo), upper(hi) {}
  void extend(T v) { lower = std::fmin(lower, v); upper = std::fmax(upper, v); }
};
typedef interval<float> range1f;

struct box3f {
  vec3f lower{ std::numeric_limits<float>::infinity() }, upper{ -std::numeric_limits<float>::infinity() };
  box3f() = default;
  box3f(vec3f lo, vec3f hi) : lower(lo), upper(hi) {}
  void extend(vec3f p)
  {
    lower = { std::fmin(lower.x, p.x), std::fmin(lower.y, p.y), std::fmin(lower.z, p.z) };
    upper = { std::fmax(upper.x, p.x), std::fmax(upper.y, p.y), std::fmax(upper.z, p.z) };
  }
  void extend(const box3f &b) { extend(b.lower); extend(b.upper); }
  vec3f center() const { return 0.5f * (lower + upper); }
  vec3f span() const { return upper - lower; }
};

struct linear3f { vec3f vx{ 1, 0, 0 }, vy{ 0, 1, 0 }, vz{ 0, 0, 1 }; };
struct affine3f {
  linear3f l; vec3f p{ 0, 0, 0 };
  static affine3f translate(vec3f t) { affine3f a; a.p = t; return a; }
  static affine3f scale(vec3f s) { affine3f a; a.l.vx = { s.x, 0, 0 }; a.l.vy = { 0, s.y, 0 }; a.l.vz = { 0, 0, s.z }; return a; }
};
inline vec3f xfmVector(const affine3f &a, vec3f v) { return v.x * a.l.vx + (v.y * a.l.vy + v.z * a.l.vz); }
inline vec3f xfmPoint(const affine3f &a, vec3f v) { return v.x * a.l.vx + (v.y * a.l.vy + (v.z * a.l.vz + a.p)); }
affine3f operator*(const affine3f &a, const affine3f &b);
affine3f rcp(const affine3f &a);

static const int NUM_XF_VALUES = EXA_NUM_XF_VALUES;
static const int MAX_CHANNELS = EXA_MAX_CHANNELS;
static const int MAX_ISO_SURFACES = EXA_MAX_ISO_SURFACES;
static const int MAX_CONTOUR_PLANES = EXA_MAX_CONTOUR_PLANES;

// ---- data model (file formats unchanged) ----
struct ExaBricks {
  typedef std::shared_ptr<ExaBricks> SP;
  // all bricks flat: record i = {size.xyz, lower.xyz, level} (the `.bricks` header order)
  std::vector<int32_t> bricks7;
  std::vector<int32_t> cellIDs;      // concatenated per-brick cell ids
  size_t totalNumCells = 0;
  // the reference's build option ALLOW_EMPTY_CELLS (CMakeLists.txt:70-73), here a property of the loaded bricks: cell id -1
  // = no cell (exa/ExaBricks.cpp:46-49); the renderer then gathers the poison value for it and skips such corners
  bool allowEmptyCells = false;
  size_t numBricks() const { return bricks7.size() / 7; }
  static SP load(const std::string &brickFileName);        // exa/ExaBricks.cpp:21-55
  void save(const std::string &brickFileName) const;       // builder/builder.cpp:895-902
  box3f getBounds() const;                                 // exa/ExaBricks.cpp:57-63
};

struct ScalarField {
  typedef std::shared_ptr<ScalarField> SP;
  static SP load(const std::string &fieldName, const std::string &fileName);              // exa/ScalarField.cpp:22-55
  static SP loadAndComputeMagnitude(const std::string &fieldName, const std::string &fnx,
                                    const std::string &fny, const std::string &fnz);      // :57-98
  static SP createFromExpression(const std::string &fieldName, const std::vector<SP> &fields,
                                 const std::vector<std::string> &tokens);                 // :100-226
  std::string name;
  interval<float> valueRange;
  std::vector<float> value;
};

struct TriangleMesh {
  typedef std::shared_ptr<TriangleMesh> SP;
  std::vector<vec3f> vertex;
  std::vector<vec3i> index;
  static std::vector<SP> load(const std::string &fileName);                               // exa/TriangleMesh.cpp:21-71
  // the same file format written: per mesh int32 nVerts, vec3f[nVerts], int32 nTris, vec3i[nTris] (the reference only reads it)
  static void save(const std::string &fileName, const std::vector<SP> &meshes);
};

struct Config {
  typedef std::shared_ptr<Config> SP;
  static SP parseConfigFile(const std::string &fileName);                                 // exa/Config.cpp:57-180
  void finalize();                                                                        // :23-44
  box3f getBounds();                                                                      // :48-55
  std::vector<TriangleMesh::SP> surfaces;
  struct {
    ExaBricks::SP sp;
    box3f remap_from{ vec3f(0.f), vec3f(1.f) };
    box3f remap_to{ vec3f(0.f), vec3f(1.f) };
    affine3f voxelSpaceTransform;
  } bricks;
  std::vector<ScalarField::SP> scalarFields;
};

// programs/FrameState.h:29-71 with the member names the viewer writes to
struct FrameState {
  struct { vec3f pos, dir00, dirDu, dirDv; } camera;
  struct { bool enabled = false; float value = 0.f; int channel = 0; } isoSurface[MAX_ISO_SURFACES];
  struct { bool enabled = false; vec3f normal{ 1.f, 0.f, 0.f }; int channel = 0; float offset = .5f; } contourPlane[MAX_CONTOUR_PLANES];
  struct { box3f coords; bool enabled = false; } clipBox;
  struct { float length = 1e20f; bool enabled = true; } ao;
  float clockScale = 0.f;
  affine3f voxelSpaceTransform;
  int frameID = 0;
  interval<float> xfDomain[MAX_CHANNELS];
  float xfOpacityScale = 1.f;
};

// an integer voxel box, half open (computeHistogram / fieldStats)
struct box3i { vec3i lower, upper; };

// exa::OptixRenderer's interface (exa/OptixRenderer.h:32-97) over the C ABI
struct Renderer {
  typedef std::shared_ptr<Renderer> SP;
  Renderer(ExaBricks::SP input, std::vector<TriangleMesh::SP> surfaces, std::vector<ScalarField::SP> scalarFields,
           int device = 0);
  // one renderer that drives several GPUs of the node (exa_hip_create_multi): image tiles dealt round-robin, every
  // device stores its tiles straight into the frame on devices[0]
  Renderer(ExaBricks::SP input, std::vector<TriangleMesh::SP> surfaces, std::vector<ScalarField::SP> scalarFields,
           const std::vector<int> &devices);
  ~Renderer();
  Renderer(const Renderer &) = delete;

  void setVoxelSpaceTransform(const affine3f &voxelSpaceTransform);
  void resizeFrameBuffer(void *fbPointer, const vec2i &fbSize);      // fbPointer: host memory, owned by the caller
  void updateIsoValues(const float *isoValues, const int *channels, const int *enabled);
  void updateContourPlanes(const vec3f *normals, const float *offsets, const int *channels, const int *enabled);
  void updateCamera(const vec3f &pos, const vec3f &dir00, const vec3f &dirDu, const vec3f &dirDv);
  void updateXF(int chan, const float *opacities, const std::vector<vec3f> &colorMap, const interval<float> &xfDomain,
                float xfOpacityScale = .1f);
  void updateFrameID(int frameID);
  void updateDt(float dt);
  void setSpaceSkipping(bool enable);
  void setGradientShadingDVR(bool enable);
  void setGradientShadingISO(bool enable);
  void setTracerEnabled(bool enable);
  void resetTracer();
  bool advanceTracer();
  void render();
  // the frame into a DEVICE buffer (memory of the first device), queued on `hipStream` without waiting: the caller
  // orders its copy-out behind it on that stream and may start the next frame into another buffer meanwhile
  void renderAsync(void *deviceColorBuffer, void *hipStream);

  // exa_hip_set_option (include/exa_hip.h): tuning knobs of the module that have no counterpart in the reference's
  // interface (which walk of the region kd-tree the march takes, launch order, AO launch plan ...); none changes a picture
  // beyond the stated float tolerance
  void setOption(const std::string &key, int value);

  // point probes (exa_hip_sample_points / exa_hip_resample; include/exa_hip.h states the contract): the reconstructed field
  // at `n` points (host arrays; values n x numChannels, gradients n x numChannels x 3 or NULL = none, status n x numChannels
  // or NULL) and at the cell centres of a uniform dims.x x dims.y x dims.z grid over `box` (out: x fastest).  Positions in
  // voxel space, or in world space through frameState.voxelSpaceTransform (the frame state is pushed first).  gradients:
  // the reference's numerator sumW*sumD - sumWV*sumDC (derivative weights in each brick's own cell units: what the
  // reference shades with, no voxel-space vector on coarse or mixed-level regions); with normalized = true the gradient of
  // the reconstruction with respect to the voxel-space position.
  void samplePoints(const vec3f *points, size_t n, const int *channels, int numChannels, float *values,
                    float *gradients = nullptr, int *status = nullptr, bool worldSpace = false, bool normalized = false,
                    float fill = NAN);
  void resample(const box3f &box, vec3i dims, int channel, float *out, bool worldSpace = false, float fill = NAN);

  // the iso-surface field == iso of `channel` on the lattice of resample(box, dims) (dims >= 2) as an indexed triangle mesh
  // by marching tetrahedra (exa_hip_isosurface; include/exa_hip.h states the contract): no duplicate vertices, normals
  // (B-A)x(C-A) toward the lower values, positions in the space of `box`.  gradients: per vertex what samplePoints gives there
  // with normalized = true (the shading normal is -grad/|grad|).  The mesh can go back in as a surface, or to a file
  // (TriangleMesh::save).
  // keep: the module keeps its device copy of the mesh (for sampleIsoSurface) until the next extraction.
  TriangleMesh::SP extractIsoSurface(const box3f &box, vec3i dims, int channel, float iso, bool worldSpace = false,
                                     std::vector<vec3f> *gradients = nullptr, bool keep = false);

  // quantities of the velocity gradient tensor of the vector field (channels.x, .y, .z): `quantity` = EXA_DERIVED_SPEED,
  // _DIVERGENCE, _VORTICITY (three components, interleaved), _VORTICITY_MAGNITUDE, _Q or _HELICITY (exa_hip_sample_derived,
  // exa_hip_resample_derived, exa_hip_isosurface_derived; include/exa_hip.h states the contract).  At points (out n x
  // components, status n or NULL), on the lattice of resample(box, dims) (components floats per lattice point) and as the
  // surface quantity == iso on that lattice (one-component quantities).  Voxel-space quantities, also with worldSpace.
  void sampleDerived(const vec3f *points, size_t n, vec3i channels, int quantity, float *out, int *status = nullptr,
                     bool worldSpace = false, float fill = NAN);
  void resampleDerived(const box3f &box, vec3i dims, vec3i channels, int quantity, float *out, bool worldSpace = false,
                       float fill = NAN);
  TriangleMesh::SP extractIsoSurfaceDerived(const box3f &box, vec3i dims, vec3i channels, int quantity, float iso,
                                            bool worldSpace = false, bool keep = false);

  // the contour lines field == iso of `channel`, for every iso of `isos`, on the plane lattice of size.x x size.y points
  // whose point (i,j) lies at origin + (i + 0.5) du + (j + 0.5) dv, by marching triangles (exa_hip_isolines; include/exa_hip.h
  // states the contract): packed vertices without duplicates in the plane's space with their plane coordinates uv, segments
  // of global vertex indices with the >= iso side to their left, level l in [vertexOffsets[l], vertexOffsets[l+1]) and
  // [segmentOffsets[l], segmentOffsets[l+1]).  gradients: per vertex what samplePoints gives there with normalized = true;
  // values: the lattice values, values[j*size.x + i] (the slice under the lines).  isolinesDerived: the same of a
  // one-component quantity of the vector field `channels` (no gradients).
  struct Isolines {
    std::vector<vec3f> vertex, gradient;
    std::vector<float> uv;                       // 2 per vertex
    std::vector<int32_t> segment;                // 2 per segment
    std::vector<uint64_t> vertexOffsets, segmentOffsets;
    std::vector<float> values;
  };
  Isolines isolines(vec3f origin, vec3f du, vec3f dv, vec2i size, const std::vector<float> &isos, int channel,
                    bool worldSpace = false, bool gradients = false, bool values = false);
  Isolines isolinesDerived(vec3f origin, vec3f du, vec3f dv, vec2i size, const std::vector<float> &isos, vec3i channels,
                           int quantity, bool worldSpace = false, bool values = false);

  // the connected regions of field >= iso (below: < iso) of `channel` on the lattice of resample(box, dims), joined along
  // the Kuhn edges of extractIsoSurface's split (faces: along the axes only), numbered by their smallest lattice index, each
  // with its exact measurements (exa_hip_regions; include/exa_hip.h states the contract): labels[(k*dims.y + j)*dims.x + i] =
  // the region's number or -1; a region's value sum is sumFixed * 2^-sumExponent.  values: the lattice as well.
  // regionsDerived: the same of a one-component quantity of the vector field `channels`.
  struct Regions {
    vec3i dims;
    std::vector<int32_t> labels;
    std::vector<ExaHipRegion> regions;
    std::vector<float> values;
    uint64_t numInside = 0;
    int32_t sumExponent = 0;
  };
  Regions regions(const box3f &box, vec3i dims, int channel, float iso, bool worldSpace = false, bool below = false,
                  bool faces = false, bool values = false);
  Regions regionsDerived(const box3f &box, vec3i dims, vec3i channels, int quantity, float iso, bool worldSpace = false,
                         bool below = false, bool faces = false, bool values = false);

  // the basins of field >= iso (below: of minima of < iso) on the same lattice: one per local maximum, those that stand
  // out of their highest pass by less than minDepth merged into the neighbour across it, round by round (exa_hip_basins;
  // include/exa_hip.h states the contract).  Numbered by the lattice index of their peak; labels, values, numInside and
  // sumExponent as for the regions; numRaw = the number of peaks, rounds = the rounds that merged something.
  // basinsDerived: the same of a one-component quantity of the vector field `channels`.
  struct Basins {
    vec3i dims;
    std::vector<int32_t> labels;
    std::vector<ExaHipBasin> basins;
    std::vector<float> values;
    uint64_t numInside = 0, numRaw = 0;
    int32_t sumExponent = 0, rounds = 0;
  };
  Basins basins(const box3f &box, vec3i dims, int channel, float iso, float minDepth, bool worldSpace = false, bool below = false,
                bool faces = false, bool values = false);
  Basins basinsDerived(const box3f &box, vec3i dims, vec3i channels, int quantity, float iso, float minDepth,
                       bool worldSpace = false, bool below = false, bool faces = false, bool values = false);

  // the critical points of the vector field (channels.x, .y, .z) on the lattice of resample(box, dims): the zeros of the
  // trilinear interpolant, at most one per cell, found by `iterations` Newton steps and accepted within `tolerance`, each
  // classified by its Jacobian (exa_hip_critical_points; include/exa_hip.h states the contract): type & 3 = the eigenvalues
  // with a positive real part, EXA_CRITICAL_SPIRAL, EXA_CRITICAL_DEGENERATE.  probe: per point and channel the value and the
  // voxel-space gradient of the real field at the position (4 floats), and the probe's status.
  struct CriticalPoints {
    std::vector<ExaHipCriticalPoint> points;     // in ascending cell number
    ExaHipCriticalStats stats;
    std::vector<float> probe;                    // points x 3 x 4, empty unless asked for
    std::vector<int32_t> probeStatus;            // points x 3
  };
  CriticalPoints criticalPoints(const box3f &box, vec3i dims, vec3i channels, int iterations = 8, float tolerance = 0.0009765625f,
                                bool worldSpace = false, bool probe = false);

  // the points of the lattice of resample(box, dims) binned by one or two axes, with the count, the exact fixed-point sums
  // and the min / max of up to four other quantities per bin, weighted if `weight` is given (exa_hip_profile; include/exa_hip.h
  // states the contract, the sources and the axes).  Bin b1 * axes[0].numBins + b0; a series' sum is fixed * 2^-exponent
  // (stats.weightExponent, stats.valueExponent).  An axis whose `labels` point to device memory: labelsOnDevice.
  struct Profile {
    std::vector<uint64_t> count;         // B
    std::vector<int64_t> sumWeight;      // B, empty without a weight
    std::vector<int64_t> sums;           // numValues x B
    std::vector<float> mins, maxs;       // numValues x B, empty without minMax
    ExaHipProfileStats stats;
  };
  Profile profile(const box3f &box, vec3i dims, const std::vector<ExaHipProfileAxis> &axes, const std::vector<ExaHipSource> &values,
                  const ExaHipSource *weight = nullptr, bool worldSpace = false, bool minMax = true, bool labelsOnDevice = false);

  // per point of the lattice of resample(box, dims) the exact Euclidean distance, in the space of the box, to the nearest
  // point where the field is >= iso and (nearest) that point's linear index (exa_hip_distance; include/exa_hip.h states the
  // contract).  flags: EXA_DISTANCE_BELOW, EXA_DISTANCE_TO_OUTSIDE, EXA_DISTANCE_SIGNED.  distanceMask: the set is
  // labels == label (-1: labels >= 0), host memory, or device memory with EXA_DISTANCE_LABELS_DEVICE; the box and dims give
  // only the spacing.  Beyond maxDistance, or with no target: +INF (-INF on the inside branch of SIGNED) and -1.
  struct Distance {
    vec3i dims;
    std::vector<float> dist;             // numPoints
    std::vector<int32_t> nearest;        // numPoints, empty without `nearest`
    ExaHipDistanceStats stats;
  };
  Distance distance(const box3f &box, vec3i dims, int channel, float iso, float maxDistance = INFINITY, int flags = 0,
                    bool nearest = false, bool worldSpace = false);
  Distance distanceDerived(const box3f &box, vec3i dims, vec3i channels, int quantity, float iso, float maxDistance = INFINITY,
                           int flags = 0, bool nearest = false, bool worldSpace = false);
  Distance distanceMask(const box3f &box, vec3i dims, const int32_t *labels, int label = -1, float maxDistance = INFINITY,
                        int flags = 0, bool nearest = false);

  // the histogram the reference's viewer meant to hand its transfer-function editor (exa/viewer.cpp:1274-1276,
  // setHistogram(computeHistogram(scalarField)), commented out there), computed on the device from the cells of `channel`
  // (exa_hip_histogram; include/exa_hip.h states the contract): cells[b] = cell slots whose value falls into bin b of
  // `range`, volume[b] (or NULL) = the same weighted with 8^level finest voxels per cell, stats (or NULL) = the counts by
  // class and level and the value range; box (or NULL) restricts all of it to the cells whose centre lies in it.
  // fieldStats is the range-only pass: what setValueRange wants, and how a caller chooses `range`.
  void computeHistogram(int channel, const interval<float> &range, int numBins, std::vector<uint64_t> &cells,
                        std::vector<uint64_t> *volume = nullptr, ExaHipFieldStats *stats = nullptr, const box3i *box = nullptr);
  ExaHipFieldStats fieldStats(int channel, const box3i *box = nullptr);

  // field lines of the vector field (channels.x, .y, .z) from `n` seeds in VOXEL space (exa_hip_streamlines; include/exa_hip.h
  // states the contract): fixed-step RK4 on the device, forward, backward or both (one polyline through the seed), along
  // v or, with normalize, along v/|v| (`step` is then an arc length in voxels).  Unlike the tracer above it does not depend
  // on the transfer function, takes whole lines in one call and says why each direction ended.
  struct Streamlines {
    std::vector<vec3f> vertex;           // all lines, packed
    std::vector<vec3f> velocity;         // per vertex the raw v (NaN for a failed seed); empty unless asked for
    std::vector<uint64_t> offset;        // n + 1: line i = vertex[offset[i] .. offset[i+1])
    std::vector<uint32_t> seedVertex;    // n: index of the seed within its line (= number of backward vertices)
    std::vector<int32_t> reason;         // n x 2 EXA_STREAM_END_*: backward, forward
  };
  Streamlines streamlines(const vec3f *seeds, size_t n, vec3i channels, float step, int maxSteps, bool forward = true,
                          bool backward = false, bool normalize = false, bool velocities = false);

  // line integral convolution of the vector field (channels.x, .y, .z) on the plane lattice of isolines, in VOXEL space
  // (exa_hip_lic; include/exa_hip.h states the contract): per pixel the noise — `noise` (size.x * size.y bytes) or, for NULL,
  // the built-in hash of (ix, iy, seed) — along the field line of the in-plane part, halfLength steps of `step` pixels
  // backward and forward, averaged.  Row-major, index j*size.x + i; a pixel whose centre has no value gets `fill`.
  struct Lic {
    std::vector<float> lic, speed;       // sum / count; |v| at the centre
    std::vector<uint32_t> sum, count;
    std::vector<int32_t> reason;         // 2 per pixel: EXA_STREAM_END_* or EXA_LIC_END_IMAGE, backward and forward
  };
  Lic lic(vec3f origin, vec3f du, vec3f dv, vec2i size, vec3i channels, float step, int halfLength,
          const uint8_t *noise = nullptr, uint32_t seed = 0, float fill = NAN);

  // flow map and stretch of the vector field (channels.x, .y, .z) on the lattice of resample, in VOXEL space (exa_hip_flowmap;
  // include/exa_hip.h states the contract): per lattice point where a particle released there is after numSteps RK4 steps of
  // the time `step`, forward or backward; the largest eigenvalue of the Cauchy-Green tensor of the map's differences; and the
  // FTLE = log(stretch) / (2 |T|), T = numSteps * step, formed in double.  Index (k*dims.y + j)*dims.x + i; stretch and ftle are
  // `fill` where the point or one of its stencil neighbours did not last the time.
  struct Flowmap {
    std::vector<vec3f> end;
    std::vector<uint32_t> steps;
    std::vector<int32_t> reason;         // EXA_STREAM_END_*
    std::vector<float> stretch, ftle;
  };
  Flowmap flowmap(vec3f lo, vec3f hi, vec3i dims, vec3i channels, float step, int numSteps, bool backward = false, float fill = NAN);

  // the field of `channel` reduced along one ray per pixel (exa_hip_project; include/exa_hip.h states the contract): pixel
  // (x, y) of the rays.width x rays.height image starts at org + (x+.5)*orgDu + (y+.5)*orgDv, runs along
  // dir + (x+.5)*dirDu + (y+.5)*dirDv (normalize: divided by its length) and is sampled at tmin + (i+.5)*dt, i < numSamples,
  // in voxel space or, with worldSpace, in world space (the frame state is pushed first).  Per pixel, row-major: sum of the
  // valid samples (sum*dt: the line integral, sum/count: the mean), their count, maximum (-inf for none), minimum (+inf)
  // and the sample index of the first maximum (-1).
  struct Projection {
    std::vector<double> sum;
    std::vector<uint32_t> count;
    std::vector<float> max, min;
    std::vector<int32_t> maxIndex;
  };
  Projection project(const ExaHipRays &rays, int channel, bool worldSpace = false, bool normalize = false);
  // where the field of `channel` first crosses `iso` along the same rays (exa_hip_raycast_iso; include/exa_hip.h states the
  // contract), per pixel, row-major: the depth t of the first crossing after `refine` rounds of bisection, the position
  // there (in the rays' space), the point probe's value and voxel-space gradient at it (all four `fill` without a
  // crossing), the sample index behind the crossing (-1), the side (+1 entering the >= iso side, -1 leaving it, 0) and the
  // number of crossings of the whole ray.
  struct IsoHits {
    std::vector<float> t, value;
    std::vector<vec3f> position, gradient;
    std::vector<int32_t> index, side;
    std::vector<uint32_t> crossings;
  };
  IsoHits raycastIso(const ExaHipRays &rays, int channel, float iso, int refine, bool worldSpace = false, bool normalize = false,
                     float fill = NAN);
  // up to four channels of the field on the triangles of a mesh (exa_hip_sample_triangles; include/exa_hip.h states the
  // contract): every triangle is cut into n x n congruent parts, n = its longest edge over `spacing` rounded up, at most maxN
  // (spacing 0: n = maxN), and sampled at their centroids.  Per triangle: subdiv = n (0: a bad index or a non-finite vertex,
  // no samples), areaNormal = half the cross product of its edges, and per channel (index triangle * numChannels + c) the sum
  // of the valid samples and their count.  Vertices in voxel space or, with worldSpace, in world space (the frame state is
  // pushed first).  sampleIsoSurface: the same on the mesh an extraction with keep = true left in the module, read on the
  // device (numTriangles: that mesh's, it sizes the result; worldSpace: as the extraction had it).  surfaceIntegrals forms,
  // in double and in ascending triangle order, what a caller wants of them.
  struct SurfaceSamples {
    int numChannels = 0;
    std::vector<double> sum;
    std::vector<uint32_t> count;
    std::vector<vec3f> areaNormal;
    std::vector<int32_t> subdiv;
  };
  SurfaceSamples sampleTriangles(const TriangleMesh &mesh, const int *channels, int numChannels, float spacing, int maxN,
                                 bool worldSpace = false);
  SurfaceSamples sampleIsoSurface(size_t numTriangles, const int *channels, int numChannels, float spacing, int maxN,
                                  bool worldSpace = false);
  // Per triangle: area = |areaNormal|, and per channel mean = sum / count (NaN where count == 0) and integral = mean * area.
  // Totals over the valid triangles (subdiv > 0; the others are counted in invalidTriangles), per channel: coveredArea and
  // uncoveredArea / uncoveredTriangles (count == 0), integral = the sum of mean * area and force = the sum of mean * areaNormal
  // over the covered ones; with three channels flux = the sum of (mean0 * n.x + mean1 * n.y) + mean2 * n.z over the triangles
  // all three cover (else NaN).
  struct SurfaceIntegrals {
    std::vector<double> area, mean, integral;                   // numTriangles, x numChannels, x numChannels
    std::vector<double> coveredArea, uncoveredArea, totalIntegral;   // numChannels each
    std::vector<uint64_t> uncoveredTriangles;
    std::vector<double> force;                                  // numChannels x 3
    double flux = NAN;
    uint64_t invalidTriangles = 0;
  };
  static SurfaceIntegrals surfaceIntegrals(const SurfaceSamples &S);
  // the rays of the camera set with updateCamera, through the pixel centres of a size.x x size.y image (world space)
  ExaHipRays cameraRays(vec2i size, float tmin, float dt, int numSamples) const;

  ExaHipStats stats() const;
  ExaHipStats renderStats();                // the same frame through the counting variant of the kernels
  size_t numRegions = 0, numLeafEntries = 0; // what Regions::buildFrom produced (exa/Regions.cpp:308-319 prints them)

  std::vector<ScalarField::SP> scalarFields;
  ExaBricks::SP input;
  box3f voxelSpaceBounds, worldSpaceBounds;
  bool multiFieldDvr = true;
  bool gradientShadingDVR = true, gradientShadingISO = true;
  bool doSpaceSkipping = true;
  FrameState frameState;
  vec2i fbSize;
  struct {                                   // exa/OptixRenderer.h:160-170
    int tracerEnabled = false;
    vec3i tracerChannels{ 0, 1, 2 };
    int numTraces = 1000;
    int numTimesteps = 100;
    float steplen = 1e-6f;
    int timestepHost = 0;
    box3f seedRegion{ vec3f(.3f, .3f, .5f), vec3f(.8f, .8f, .5f) };
  } traces;

private:
  void init(std::vector<TriangleMesh::SP> surfaces, const std::vector<int> &devices);
  void pushState();
  ExaPrep *prep = nullptr;
  ExaHipRenderer *handle = nullptr;
  ExaHipParams params{};
  void *fbPointer = nullptr;
};
typedef Renderer OptixRenderer;   // source compatibility for hosts written against the reference

} // namespace exa
