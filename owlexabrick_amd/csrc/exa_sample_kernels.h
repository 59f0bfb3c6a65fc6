// exa_sample_kernels.h — the point probes: exa_hip_sample_points (one lane per point) and exa_hip_resample (one wave per
// compact patch of 64 grid points), and on the same lookup and sums the derived quantities of exa_hip_sample_derived /
// exa_hip_resample_derived (the same two shapes of kernel over three channels) and the projections of exa_hip_project (one
// wave per 8 x 8 rays, reduced in registers), the iso-crossings of exa_hip_raycast_iso along the same rays and the field reduced
// over the triangles of a mesh of exa_hip_sample_triangles (small triangles packed into shared waves, large ones a wave each).  Included by exa_kernels.hip inside namespace exa::EXA_FORM_NS when it is compiled with
// -DEXA_TU_SAMPLE=1 (exa_sample_f0.o, exa_sample_f1.o, exa_sample_f0e.o), after samplePoint and the basis evaluations it
// uses; nothing else of the renderer is compiled there.
//
// Contract (include/exa_hip.h): the region of a position comes from the region kd-tree alone — inside the closed root box,
// `right` where p[axis] >= split, else `left`, down to a leaf, accepted if p lies in that region's closed domain — so a
// result depends on the scene, the position, the basis form and (world space) the transform, never on the transfer
// function, the activity bits or any other knob.  The value is samplePoint on the march headers (the sums of the DVR
// march and of the oracle, bit for bit); status -2 where sumW <= 1e-20 (the reference's samplePoint returns false).
// The gradient is the reference's numerator sumW * sumD - sumWV * sumDC, whose derivative weights are per brick in that
// brick's cell units; EXA_SAMPLE_GRADIENT_NORMALIZED takes them in voxel units instead (addBasisFast<.., VOXEL>: each
// brick's terms times its 2^-level) and divides by sumW^2: the gradient of sumWV / sumW with respect to the position.

#include "exa_sample_locate.h"   // sampleInRoot, sampleKdChild, sampleKdLeaf, sampleKdLeafWave, sampleInDomain

// samplePoint's sums (exabrick.cu:781-806, 883-928) over the region's bricks, through the march headers: the loop of
// samplePoint with fastSampler.  listBegin / listSize wave-uniform -> the headers are read once per wave.
template <bool DERIV, bool VOXEL = false>
__device__ __forceinline__ Basis sampleSums(const SampleArgs &a, int listBegin, int listSize, const float *field, V3 p)
{
  Ctx<0> C;                       // no counters
  Basis B;
  B.sumWV = 0.f; B.sumW = 0.f; B.sumD = mk(0.f, 0.f, 0.f); B.sumDC = mk(0.f, 0.f, 0.f);
  for (int child = 0; child < listSize; child++) {
    const size_t at = 2 * (size_t(listBegin) + size_t(child));
    const int4 h0 = a.leafHdr[at], h1 = a.leafHdr[at + 1];
    addBasisFast<DERIV, 0, false, VOXEL>(C, B, h0, h1, field, p);
  }
  return B;
}

// one channel at p inside the closed domain of the region whose record is R: the value and (DERIV) the gradient of the points
// API — NORM: the voxel-space one (see the head of this file); false, both untouched, where the basis weights vanish (status -2)
template <bool DERIV, bool NORM>
__device__ __forceinline__ bool sampleValueGrad(const SampleArgs &a, const RegionRec &R, const float *field, V3 p, float &value, V3 &grad)
{
  const Basis B = sampleSums<DERIV, NORM>(a, R.listBegin, R.listSize, field, p);
  if (B.sumW <= 1e-20f) return false;
  value = B.sumWV / B.sumW;
  if (DERIV) {
    grad = gradOf(B.sumW, B.sumWV, B.sumD, B.sumDC);
    if (NORM) {
      const float w2 = B.sumW * B.sumW;
      grad = mk(grad.x / w2, grad.y / w2, grad.z / w2);
    }
  }
  return true;
}

// one lane per point, the region located once for all channels
template <bool DERIV, bool NORM>
__device__ __forceinline__ void samplePointsBody(const SampleArgs &a)
{
  const size_t i = size_t(blockIdx.x) * 256u + threadIdx.x;
  if (i >= a.count) return;
  V3 p = mk(a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]);
  if (a.world) p = xfmPoint(a.fs, p);
  bool tripped = false;
  int region = sampleInRoot(a, p) ? sampleKdLeaf(a, a.kdRoot, p, tripped) : -1;
  if (tripped) atomicExch(a.errorFlag, 1);
  RegionRec R;
  R.listBegin = 0; R.listSize = 0;
  if (region >= 0) {
    R = a.regionRec[region];
    if (!sampleInDomain(R, p)) region = -1;
  }
  for (int c = 0; c < a.numChannels; c++) {
    const size_t o = i * size_t(a.numChannels) + size_t(c);
    int st = region;
    float value = a.fill;
    V3 grad = mk(a.fill, a.fill, a.fill);
    if (region >= 0 && !sampleValueGrad<DERIV, NORM>(a, R, a.scalars + a.fieldOffset[c], p, value, grad)) st = -2;
    a.values[o] = value;
    if (DERIV) { a.gradients[3 * o] = grad.x; a.gradients[3 * o + 1] = grad.y; a.gradients[3 * o + 2] = grad.z; }
    if (a.status) a.status[o] = st;
  }
}

template <bool DERIV>
__global__ __launch_bounds__(256) void samplePointsKernel(const SampleArgs a) { samplePointsBody<DERIV, false>(a); }
__global__ __launch_bounds__(256) void samplePointsNormKernel(const SampleArgs a) { samplePointsBody<true, true>(a); }

// a sample whose region record is R: the closed-domain test and the sums of samplePointsBody; false, v untouched, outside the
// domain (status -1) and where the basis weights vanish (status -2).  R by value: the whole record is read up front
__device__ __forceinline__ bool sampleValue(const SampleArgs &a, const RegionRec R, const float *field, V3 p, float &v)
{
  if (!sampleInDomain(R, p)) return false;
  const Basis B = sampleSums<false>(a, R.listBegin, R.listSize, field, p);
  if (B.sumW <= 1e-20f) return false;
  v = B.sumWV / B.sumW;
  return true;
}

// One wave per patch of PX x PY x PZ = 64 grid points (lane -> point x fastest).  UNIFORM: the wave descends the tree
// together while all its lanes (those inside the root box) take the same side of every plane — the node index is
// wave-uniform, one scalar load per node — then each lane on its own from there; when all lanes land in the same region,
// its record and brick headers are read once per wave through a wave-uniform index.  Otherwise (and without UNIFORM) the
// per-lane path of samplePointsKernel.  Both find the same region and add the same bricks in the same order: the grid
// equals the points API bit for bit.
template <int PX, int PY, int PZ, bool UNIFORM>
__global__ __launch_bounds__(256) void sampleGridKernel(const SampleArgs a)
{
  static_assert(PX * PY * PZ == 64, "a patch is one wave");
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long wave = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (wave >= a.numPatches) return;
  const unsigned long long wx = wave % a.patchesX, wyz = wave / a.patchesX;
  const unsigned long long wy = wyz % a.patchesY, wz = wyz / a.patchesY;
  const long long x = a.box0[0] + (long long)(wx * PX + lane % PX);
  const long long y = a.box0[1] + (long long)(wy * PY + (lane / PX) % PY);
  const long long z = a.box0[2] + (long long)(wz * PZ + lane / (PX * PY));
  if (x >= a.box1[0] || y >= a.box1[1] || z >= a.box1[2]) return;
  V3 p = mk(a.lo[0] + (float(x) + 0.5f) * a.step[0], a.lo[1] + (float(y) + 0.5f) * a.step[1], a.lo[2] + (float(z) + 0.5f) * a.step[2]);
  if (a.world) p = xfmPoint(a.fs, p);
  bool tripped = false;
  int region = -1;
  if (sampleInRoot(a, p)) region = sampleKdLeafWave<UNIFORM>(a, p, tripped);
  if (tripped) atomicExch(a.errorFlag, 1);
  const float *field = a.scalars + a.fieldOffset[0];
  const int r0 = __builtin_amdgcn_readfirstlane(region);
  float value = a.fill;
  if (UNIFORM && r0 >= 0 && !anyLane(region != r0)) sampleValue(a, a.regionRec[r0], field, p, value);   // wave-uniform index: one record per wave
  else if (region >= 0) sampleValue(a, a.regionRec[region], field, p, value);
  const size_t o = size_t(x - a.box0[0]) + size_t(y - a.box0[1]) * size_t(a.strideY) + size_t(z - a.box0[2]) * size_t(a.strideZ);
  a.out[o] = value;
}

// ---- exa_hip_sample_derived / exa_hip_resample_derived: quantities of the velocity gradient tensor ----
// The three channels at p in the region whose record is R, one after the other through sampleSums<true, true> — value,
// numerator and quotients exactly as samplePointsBody<true, true> forms them —, of which only v[c] and the three quotients
// J[c] stay live, then the contract's table (include/exa_hip.h) in float32, every operation rounded separately (the unit is
// compiled without contraction) and associated as written there.  Returns the status: `region`, -1 outside R's closed
// domain, -2 where the weights of any channel vanish; q untouched where it is < 0.  a.quantity is wave-uniform.
__device__ __forceinline__ int sampleDerived(const SampleArgs &a, const RegionRec R, int region, V3 p, float q[3])
{
  if (!sampleInDomain(R, p)) return -1;
  float v[3];
  V3 J[3];
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const Basis B = sampleSums<true, true>(a, R.listBegin, R.listSize, a.scalars + a.fieldOffset[c], p);
    if (B.sumW <= 1e-20f) return -2;
    v[c] = B.sumWV / B.sumW;
    const V3 g = gradOf(B.sumW, B.sumWV, B.sumD, B.sumDC);
    const float w2 = B.sumW * B.sumW;
    J[c] = mk(g.x / w2, g.y / w2, g.z / w2);
  }
  // J[c].x, .y, .z = J[c][0], [1], [2]
  const V3 w = mk(J[2].y - J[1].z, J[0].z - J[2].x, J[1].x - J[0].y);
  switch (a.quantity) {
  case EXA_DERIVED_SPEED:
    // sqrtf: the compiler's correctly rounded expansion, as in the streamline integrator
    q[0] = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    break;
  case EXA_DERIVED_DIVERGENCE:
    q[0] = (J[0].x + J[1].y) + J[2].z;
    break;
  case EXA_DERIVED_VORTICITY:
    q[0] = w.x; q[1] = w.y; q[2] = w.z;
    break;
  case EXA_DERIVED_VORTICITY_MAGNITUDE:
    q[0] = sqrtf((w.x * w.x + w.y * w.y) + w.z * w.z);
    break;
  case EXA_DERIVED_Q: {
    const float d = (J[0].x * J[0].x + J[1].y * J[1].y) + J[2].z * J[2].z;
    const float o = (J[0].y * J[1].x + J[0].z * J[2].x) + J[1].z * J[2].y;
    q[0] = -0.5f * d - o;
    break;
  }
  default:   // EXA_DERIVED_HELICITY (the host has checked the quantity)
    q[0] = (v[0] * w.x + v[1] * w.y) + v[2] * w.z;
    break;
  }
  return region;
}

// a.components floats of a point or lattice point: the quantity, or `fill` in every one of them where the status is < 0
__device__ __forceinline__ void storeDerived(const SampleArgs &a, float *at, int st, const float q[3])
{
  at[0] = st >= 0 ? q[0] : a.fill;
  if (a.components == 3) { at[1] = st >= 0 ? q[1] : a.fill; at[2] = st >= 0 ? q[2] : a.fill; }
}

// one lane per point: the lookup of samplePointsBody, once for the three channels
__global__ __launch_bounds__(256) void sampleDerivedPointsKernel(const SampleArgs a)
{
  const size_t i = size_t(blockIdx.x) * 256u + threadIdx.x;
  if (i >= a.count) return;
  V3 p = mk(a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]);
  if (a.world) p = xfmPoint(a.fs, p);
  bool tripped = false;
  const int region = sampleInRoot(a, p) ? sampleKdLeaf(a, a.kdRoot, p, tripped) : -1;
  if (tripped) atomicExch(a.errorFlag, 1);
  float q[3] = { 0.f, 0.f, 0.f };
  const int st = region >= 0 ? sampleDerived(a, a.regionRec[region], region, p, q) : -1;
  storeDerived(a, a.values + i * size_t(a.components), st, q);
  if (a.status) a.status[i] = st;
}

// sampleGridKernel's patches, shared descent and shared region record, with sampleDerived as the body: the lattice equals
// sampleDerivedPointsKernel at its positions bit for bit.  Output index: that of sampleGridKernel times a.components
template <int PX, int PY, int PZ, bool UNIFORM>
__global__ __launch_bounds__(256) void sampleDerivedGridKernel(const SampleArgs a)
{
  static_assert(PX * PY * PZ == 64, "a patch is one wave");
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long wave = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (wave >= a.numPatches) return;
  const unsigned long long wx = wave % a.patchesX, wyz = wave / a.patchesX;
  const unsigned long long wy = wyz % a.patchesY, wz = wyz / a.patchesY;
  const long long x = a.box0[0] + (long long)(wx * PX + lane % PX);
  const long long y = a.box0[1] + (long long)(wy * PY + (lane / PX) % PY);
  const long long z = a.box0[2] + (long long)(wz * PZ + lane / (PX * PY));
  if (x >= a.box1[0] || y >= a.box1[1] || z >= a.box1[2]) return;
  V3 p = mk(a.lo[0] + (float(x) + 0.5f) * a.step[0], a.lo[1] + (float(y) + 0.5f) * a.step[1], a.lo[2] + (float(z) + 0.5f) * a.step[2]);
  if (a.world) p = xfmPoint(a.fs, p);
  bool tripped = false;
  int region = -1;
  if (sampleInRoot(a, p)) region = sampleKdLeafWave<UNIFORM>(a, p, tripped);
  if (tripped) atomicExch(a.errorFlag, 1);
  const int r0 = __builtin_amdgcn_readfirstlane(region);
  float q[3] = { 0.f, 0.f, 0.f };
  int st = -1;
  if (UNIFORM && r0 >= 0 && !anyLane(region != r0)) st = sampleDerived(a, a.regionRec[r0], region, p, q);   // wave-uniform index: one record per wave
  else if (region >= 0) st = sampleDerived(a, a.regionRec[region], region, p, q);
  const size_t o = size_t(x - a.box0[0]) + size_t(y - a.box0[1]) * size_t(a.strideY) + size_t(z - a.box0[2]) * size_t(a.strideZ);
  storeDerived(a, a.out + o * size_t(a.components), st, q);
}

// ---- exa_hip_project: the field reduced along rays ----
// p_i of the contract: t_i = tmin + (float(i) + 0.5f) * dt, p_i = o + t_i * d, every operation rounded separately (the unit
// is compiled without contraction).  The ONE position function of the marches and of the bisections below.
__device__ __forceinline__ float rayTime(const RayArgs &a, int i) { return a.rays.tmin + (float(i) + 0.5f) * a.rays.dt; }
__device__ __forceinline__ V3 rayPos(const RayArgs &a, V3 o, V3 d, int i) { return o + rayTime(a, i) * d; }

// sampleInRoot's six comparisons, dealt by the sign of the direction into the three a ray satisfies from some index on
// (rayEntered) and the three it satisfies up to some index (rayNotLeft): sampleInRoot(p) == rayEntered(p) && rayNotLeft(p)
__device__ __forceinline__ bool rayEntered(const SampleArgs &s, V3 d, V3 p)
{
  return (d.x >= 0.f ? p.x >= s.kdLo[0] : p.x <= s.kdHi[0]) && (d.y >= 0.f ? p.y >= s.kdLo[1] : p.y <= s.kdHi[1])
      && (d.z >= 0.f ? p.z >= s.kdLo[2] : p.z <= s.kdHi[2]);
}
__device__ __forceinline__ bool rayNotLeft(const SampleArgs &s, V3 d, V3 p)
{
  return (d.x >= 0.f ? p.x <= s.kdHi[0] : p.x >= s.kdLo[0]) && (d.y >= 0.f ? p.y <= s.kdHi[1] : p.y >= s.kdLo[1])
      && (d.z >= 0.f ? p.z <= s.kdHi[2] : p.z >= s.kdLo[2]);
}

// the reduction of one pixel, in registers
struct RayAcc { double sum; uint32_t count; float vmax, vmin; int32_t maxIndex; };

// one sample whose lane has a region: where it is valid (sampleValue), the contract's updates
__device__ __forceinline__ void rayAccumulate(const RayArgs &a, const RegionRec &R, const float *field, V3 p, int i, RayAcc &acc)
{
  float v;
  if (!sampleValue(a.s, R, field, p, v)) return;
  acc.count++;
  acc.sum += double(v);
  if (v > acc.vmax) { acc.vmax = v; acc.maxIndex = i; }
  if (v < acc.vmin) acc.vmin = v;
}

// A lane's pixel of the tile, its ray (o, d of the contract) and the sample indices to march: its own [beg, end) and the
// union [wBeg, wEnd) of its wave's (wave-uniform).  One wave per 8 x 8 pixels, every lane one ray.
//
// SKIP (voxel space): indices whose position cannot lie in the root box are not marched.  For a lane with finite o and d
// (any other lane has no position inside the finite root box at all: a non-finite o or d makes every p_i infinite or NaN)
//   - t_i is non-decreasing in i: float(i) + 0.5f is exact below 2^23 and increasing, the product with dt > 0 and the sum
//     with tmin are correctly rounded operations with one operand fixed, which are monotone; every t_i is finite, because
//     |t_i| <= max(|tmin|, |tmin + float(numSamples) * dt|), which the call has checked;
//   - per axis k, p_i.k = o.k + t_i * d.k is, for the same reason, non-decreasing in t_i where d.k >= 0 and non-increasing
//     where d.k < 0 (d.k == +-0: constant; no NaN can arise, o.k being finite: an overflowing product gives o.k +- inf).
// So each comparison of rayEntered is false up to some index and true from it on, hence so is their conjunction; each of
// rayNotLeft is true up to some index and false from it on, hence so is theirs.  A bisection finds the first index `beg`
// with rayEntered and the first index `end` without rayNotLeft exactly (numSamples evaluations of the same rayPos would
// find the same two), and sampleInRoot(p_i) holds precisely for beg <= i < end (for no i if beg >= end).  A skipped index
// is therefore one whose sample is invalid (status -1), which the reduction ignores; the marched ones are tested with
// sampleInRoot itself as ever.  The wave marches the union [min beg, max end) of its lanes' ranges; a lane idles outside
// its own.  In world space the transform mixes the axes and nothing of this holds: every index is marched.
struct RayLane {
  bool live;                  // a dead lane stays (the wave's shuffles and ballots see it) with no samples
  int  x, y;
  V3   o, d;
  int  beg, end, wBeg, wEnd;
};

template <bool SKIP>
__device__ __forceinline__ RayLane rayLane(const RayArgs &a, unsigned long long wave, unsigned lane)
{
  const long long xl = a.x0 + (long long)(wave % a.patchesX) * 8 + (long long)(lane & 7u);
  const long long yl = a.y0 + (long long)(wave / a.patchesX) * 8 + (long long)(lane >> 3);
  const bool live = xl < a.x1 && yl < a.y1;
  const int x = int(xl), y = int(yl);              // a live lane's fit: x1, y1 are int32
  const int n = a.rays.numSamples;
  const float sx = float(x) + 0.5f, sy = float(y) + 0.5f;
  const V3 o = (mk(a.rays.org) + sx * mk(a.rays.orgDu)) + sy * mk(a.rays.orgDv);
  V3 d = (mk(a.rays.dir) + sx * mk(a.rays.dirDu)) + sy * mk(a.rays.dirDv);
  int beg = 0, end = live ? n : 0;
  if (a.normalize) {
    // sqrtf and `/`: the compiler's correctly rounded expansions, as in the streamline integrator
    const float s = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    if (!(s > 0.f) || !(s <= FLT_MAX)) end = 0;
    d = mk(d.x / s, d.y / s, d.z / s);
  }
  if (SKIP) {
    const bool finite = fabsf(o.x) <= FLT_MAX && fabsf(o.y) <= FLT_MAX && fabsf(o.z) <= FLT_MAX
                     && fabsf(d.x) <= FLT_MAX && fabsf(d.y) <= FLT_MAX && fabsf(d.z) <= FLT_MAX;
    if (!finite) end = 0;
    if (end > 0) {
      // the first index with rayEntered, in [0, n]; then the first without rayNotLeft, in [beg, n]
      int lo = 0, hi = n;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rayEntered(a.s, d, rayPos(a, o, d, mid))) hi = mid; else lo = mid + 1;
      }
      beg = lo;
      hi = n;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (rayNotLeft(a.s, d, rayPos(a, o, d, mid))) lo = mid + 1; else hi = mid;
      }
      end = lo;
    }
  }
  if (end <= beg) { beg = n; end = 0; }
  // the union of the wave's ranges
  int wBeg = beg, wEnd = end;
  for (int m = 32; m >= 1; m >>= 1) {
    wBeg = min(wBeg, __shfl_xor(wBeg, m, 64));
    wEnd = max(wEnd, __shfl_xor(wEnd, m, 64));
  }
  RayLane L;
  L.live = live; L.x = x; L.y = y; L.o = o; L.d = d; L.beg = beg; L.end = end;
  L.wBeg = __builtin_amdgcn_readfirstlane(wBeg);
  L.wEnd = __builtin_amdgcn_readfirstlane(wEnd);
  return L;
}

// The lanes step the sample index i together, so that at every i the wave's 64 positions lie in a small patch of space and
// the grid kernel's UNIFORM scheme applies: a shared descent while the lanes (those inside the root box) take the same side
// of every plane, one region record and one stream of brick headers per wave when they land in one region, else lane by
// lane.  Both through sampleInRoot, sampleKdChild, sampleKdLeaf, sampleInDomain and sampleSums<false>, as the points kernel:
// a sample equals exa_hip_sample_points bit for bit.
template <bool UNIFORM, bool SKIP>
__global__ __launch_bounds__(256) void sampleRaysKernel(const RayArgs a)
{
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long wave = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (wave >= a.numPatches) return;
  const RayLane L = rayLane<SKIP>(a, wave, lane);
  const float *field = a.s.scalars + a.s.fieldOffset[0];
  RayAcc acc;
  acc.sum = 0.0; acc.count = 0u; acc.vmax = -INFINITY; acc.vmin = INFINITY; acc.maxIndex = -1;
  bool tripped = false;
  for (int i = L.wBeg; i < L.wEnd; i++) {
    V3 p = rayPos(a, L.o, L.d, i);
    if (a.s.world) p = xfmPoint(a.s.fs, p);
    int region = -1;
    if (i >= L.beg && i < L.end && sampleInRoot(a.s, p)) region = sampleKdLeafWave<UNIFORM>(a.s, p, tripped);
    if (region >= 0) {
      const int r0 = __builtin_amdgcn_readfirstlane(region);           // of the lanes that have a region
      if (UNIFORM && !anyLane(region != r0)) {
        const RegionRec R = a.s.regionRec[r0];                           // wave-uniform index: one record per wave
        rayAccumulate(a, R, field, p, i, acc);
      } else {
        const RegionRec R = a.s.regionRec[region];
        rayAccumulate(a, R, field, p, i, acc);
      }
    }
  }
  if (tripped) atomicExch(a.s.errorFlag, 1);
  if (!L.live) return;
  const size_t at = size_t(L.x - a.x0) + size_t(L.y - a.y0) * size_t(a.strideY);
  if (a.sum) a.sum[at] = acc.sum;
  if (a.count) a.count[at] = acc.count;
  if (a.vmax) a.vmax[at] = acc.vmax;
  if (a.vmin) a.vmin[at] = acc.vmin;
  if (a.maxIndex) a.maxIndex[at] = acc.maxIndex;
}

// ---- exa_hip_raycast_iso: the first crossing of a value along the same rays ----
// the point probe at the caller's position q, lane by lane (the lookup of samplePointsBody, the value of sampleValue): false,
// v untouched, where the sample is not usable — status < 0, or a NaN value
__device__ __forceinline__ bool crossSample(const SampleArgs &s, const float *field, V3 q, bool &tripped, float &v)
{
  const V3 p = s.world ? xfmPoint(s.fs, q) : q;
  if (!sampleInRoot(s, p)) return false;
  const int region = sampleKdLeaf(s, s.kdRoot, p, tripped);
  if (region < 0) return false;
  float u;
  if (!sampleValue(s, s.regionRec[region], field, p, u) || u != u) return false;
  v = u;
  return true;
}

// sampleRaysKernel's rays, patches, lookup and skipped indices — a skipped index is a sample with status -1, which is not
// usable: skipping cannot change a byte — with the contract's crossings in place of the reduction.  The march keeps the
// previous sample (usable, value, t), the bracket of the first crossing and the count in registers; without an array of
// counts (a.crossings == NULL) a lane idles from its first crossing on and the wave stops when no lane is still looking.
// Behind the march, where any lane of the wave has a crossing: that lane's bisection of the bracket, a point probe per
// round on the per-lane lookup (the lanes' brackets have nothing to do with each other any more), the contract's
// interpolation, and the value and voxel-space gradient at the hit as samplePointsNormKernel forms them (sampleValueGrad).
template <bool UNIFORM, bool SKIP>
__global__ __launch_bounds__(256) void sampleCrossingsKernel(const CrossArgs a)
{
  const unsigned lane = threadIdx.x & 63u;
  const unsigned long long wave = (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  const RayArgs &ra = a.r;
  const SampleArgs &s = ra.s;
  if (wave >= ra.numPatches) return;
  const RayLane L = rayLane<SKIP>(ra, wave, lane);
  const float *field = s.scalars + s.fieldOffset[0];
  const float iso = a.iso;
  const bool all = a.crossings != nullptr;
  bool tripped = false, prevOk = false;
  float prevV = 0.f, prevT = 0.f;
  float ta = 0.f, va = 0.f, tb = 0.f, vb = 0.f;   // the bracket of the first crossing
  int index = -1;
  uint32_t count = 0u;
  for (int i = L.wBeg; i < L.wEnd; i++) {
    if (!all && !anyLane(index < 0 && i < L.end)) break;
    const float t = rayTime(ra, i);
    V3 p = L.o + t * L.d;
    if (s.world) p = xfmPoint(s.fs, p);
    int region = -1;
    if (i >= L.beg && i < L.end && (all || index < 0) && sampleInRoot(s, p)) region = sampleKdLeafWave<UNIFORM>(s, p, tripped);
    float v = 0.f;
    bool ok = false;
    if (region >= 0) {
      const int r0 = __builtin_amdgcn_readfirstlane(region);           // of the lanes that have a region
      if (UNIFORM && !anyLane(region != r0)) ok = sampleValue(s, s.regionRec[r0], field, p, v);   // wave-uniform index: one record per wave
      else ok = sampleValue(s, s.regionRec[region], field, p, v);
    }
    ok = ok && v == v;
    if (ok && prevOk && (prevV >= iso) != (v >= iso)) {
      count++;
      if (index < 0) { index = i; ta = prevT; va = prevV; tb = t; vb = v; }
    }
    prevOk = ok; prevV = v; prevT = t;
  }
  const float fill = s.fill;
  float tHit = fill, value = fill;
  V3 pos = mk(fill, fill, fill), grad = mk(fill, fill, fill);
  int side = 0;
  if (anyLane(index >= 0)) {                      // wave-uniform: a wave without a crossing skips the tail
    if (index >= 0) {
      side = va < iso ? 1 : -1;
      for (int round = 0; round < a.refine; round++) {
        const float tm = 0.5f * (ta + tb);
        if (tm == ta || tm == tb) break;
        float vm;
        if (!crossSample(s, field, L.o + tm * L.d, tripped, vm)) break;
        if ((vm >= iso) == (va >= iso)) { ta = tm; va = vm; } else { tb = tm; vb = vm; }
      }
      const float w = (iso - va) / (vb - va);
      tHit = ta + w * (tb - ta);
      pos = L.o + tHit * L.d;
      const V3 p = s.world ? xfmPoint(s.fs, pos) : pos;
      const int region = sampleInRoot(s, p) ? sampleKdLeaf(s, s.kdRoot, p, tripped) : -1;
      if (region >= 0) {
        const RegionRec R = s.regionRec[region];
        if (sampleInDomain(R, p)) sampleValueGrad<true, true>(s, R, field, p, value, grad);
      }
    }
  }
  if (tripped) atomicExch(s.errorFlag, 1);
  if (!L.live) return;
  const size_t at = size_t(L.x - ra.x0) + size_t(L.y - ra.y0) * size_t(ra.strideY);
  if (a.t) a.t[at] = tHit;
  if (a.position) { a.position[3 * at] = pos.x; a.position[3 * at + 1] = pos.y; a.position[3 * at + 2] = pos.z; }
  if (a.value) a.value[at] = value;
  if (a.gradient) { a.gradient[3 * at] = grad.x; a.gradient[3 * at + 1] = grad.y; a.gradient[3 * at + 2] = grad.z; }
  if (a.index) a.index[at] = index;
  if (a.side) a.side[at] = side;
  if (a.crossings) a.crossings[at] = count;
}

// a launcher of a ray kernel K<UNIFORM, SKIP> on the tile of `rays` (the RayArgs of a): one wave per 8 x 8 pixels
#define EXA_RAY_LAUNCHER(NAME, K, ARGS, rays)                                                                            \
  hipError_t NAME(const ARGS &a, bool uniform, hipStream_t s)                                                            \
  {                                                                                                                      \
    if ((rays).numPatches == 0) return hipSuccess;                                                                       \
    const dim3 grid((unsigned)(((rays).numPatches + 3) / 4)), block(256);                                                \
    const bool skip = (rays).s.world == 0;                                                                               \
    if (uniform) { if (skip) hipLaunchKernelGGL((K<true, true>), grid, block, 0, s, a);                                  \
                   else      hipLaunchKernelGGL((K<true, false>), grid, block, 0, s, a); }                               \
    else         { if (skip) hipLaunchKernelGGL((K<false, true>), grid, block, 0, s, a);                                 \
                   else      hipLaunchKernelGGL((K<false, false>), grid, block, 0, s, a); }                              \
    return hipGetLastError();                                                                                            \
  }
EXA_RAY_LAUNCHER(launchSampleRays, sampleRaysKernel, RayArgs, a)
EXA_RAY_LAUNCHER(launchSampleCrossings, sampleCrossingsKernel, CrossArgs, a.r)
#undef EXA_RAY_LAUNCHER

// ---- exa_hip_sample_triangles: the field reduced over the triangles of a mesh ----
// A triangle as the kernels see it: v0, the two edges of the contract and its subdivision n (0: not valid, no samples).
struct TriGeom { V3 v0, e1, e2; int n; };

// n of the contract (include/exa_hip.h): the longest edge over the spacing, rounded up, in 1 .. maxN; 0 where a length is not
// finite (L, the maximum with a NaN propagated, is finite exactly where all three are).  sqrtf, `/`: correctly rounded
__device__ __forceinline__ int sampleTrianglesSubdiv(V3 v0, V3 v1, V3 v2, float spacing, int maxN)
{
  const V3 a = v1 - v0, b = v2 - v1, c = v0 - v2;
  const float la = sqrtf((a.x * a.x + a.y * a.y) + a.z * a.z), lb = sqrtf((b.x * b.x + b.y * b.y) + b.z * b.z),
              lc = sqrtf((c.x * c.x + c.y * c.y) + c.z * c.z);
  if (!(la <= FLT_MAX && lb <= FLT_MAX && lc <= FLT_MAX)) return 0;
  if (spacing == 0.f) return maxN;
  const float q = fmaxf(fmaxf(la, lb), lc) / spacing;
  if (q >= float(maxN)) return maxN;
  return max(1, (int)ceilf(q));
}

// triangle t of the launch, whose indices the first kernel has found in range
__device__ __forceinline__ TriGeom sampleTrianglesGeom(const TriArgs &a, int t)
{
  const int32_t *idx = a.triangles + 3 * size_t(t);
  const V3 v0 = mk(a.vertices + 3 * size_t(idx[0])), v1 = mk(a.vertices + 3 * size_t(idx[1])), v2 = mk(a.vertices + 3 * size_t(idx[2]));
  TriGeom g;
  g.v0 = v0; g.e1 = v1 - v0; g.e2 = v2 - v0;
  g.n = sampleTrianglesSubdiv(v0, v1, v2, a.spacing, a.maxN);
  return g;
}

// p_k of the contract: the centroid of sub-triangle k of n * n, every operation rounded separately
__device__ __forceinline__ V3 sampleTrianglesPos(const TriGeom &g, int k)
{
  const int n = max(g.n, 1), ka = k / n, kb = k - ka * n;
  const bool upright = ka + kb < n;
  const float fa = upright ? float(ka) + 1.0f / 3.0f : float(n - 1 - ka) + 2.0f / 3.0f;
  const float fb = upright ? float(kb) + 1.0f / 3.0f : float(n - 1 - kb) + 2.0f / 3.0f;
  const float b1 = fa / float(n), b2 = fb / float(n);
  return (g.v0 + b1 * g.e1) + b2 * g.e2;
}

// the channels at p inside the region whose record is R, added to the lane's partial sums and counts where valid: the
// closed-domain test and the sums of samplePointsBody
__device__ __forceinline__ void sampleTrianglesAdd(const SampleArgs &s, const RegionRec R, V3 p, double P[EXA_SURFACE_MAX_CHANNELS],
                                                   uint32_t cnt[EXA_SURFACE_MAX_CHANNELS])
{
  if (!sampleInDomain(R, p)) return;
  for (int c = 0; c < s.numChannels; c++) {
    const Basis B = sampleSums<false>(s, R.listBegin, R.listSize, s.scalars + s.fieldOffset[c], p);
    if (B.sumW <= 1e-20f) continue;
    const double v = double(B.sumWV / B.sumW);
#pragma unroll
    for (int k = 0; k < EXA_SURFACE_MAX_CHANNELS; k++)       // registers, not an indexed array
      if (k == c) { P[k] += v; cnt[k]++; }
  }
}

// The voxelSpaceTransform for the sampling kernels below, in LDS: as kernel arguments its twelve floats would stay in scalar
// registers from the first sample to the last, which these kernels do not have to spare (they would spill some); read from
// LDS at each sample they are vector registers for the length of xfmPoint.  Every thread of the block calls this, once
__device__ __forceinline__ void sampleTrianglesStageXfm(const SampleArgs &s, float xfm[12])
{
  if (!s.world) return;                                                 // the same in every thread
  const unsigned i = threadIdx.x;
  if (i < 12u) {
    const float *row = i < 3u ? s.fs.xfm_vx : (i < 6u ? s.fs.xfm_vy : (i < 9u ? s.fs.xfm_vz : s.fs.xfm_p));
    xfm[i] = row[i % 3u];
  }
  __syncthreads();
}

// one sample per lane (`active`: the lane has one) at the caller's position q: the lookup of the grid and ray kernels — a shared
// descent while the wave's lanes agree, one region record per wave where they land in one region, else lane by lane.  World
// space: xfmPoint, operation for operation, on the staged transform
template <bool UNIFORM>
__device__ __forceinline__ void sampleTrianglesAt(const SampleArgs &s, const float xfm[12], bool active, V3 q, bool &tripped,
                                                  double P[EXA_SURFACE_MAX_CHANNELS], uint32_t cnt[EXA_SURFACE_MAX_CHANNELS])
{
  V3 p = q;
  if (s.world) p = q.x * mk(xfm) + (q.y * mk(xfm + 3) + (q.z * mk(xfm + 6) + mk(xfm + 9)));
  int region = -1;
  if (active && sampleInRoot(s, p)) region = sampleKdLeafWave<UNIFORM>(s, p, tripped);
  if (region >= 0) {
    const int r0 = __builtin_amdgcn_readfirstlane(region);             // of the lanes that have a region
    if (UNIFORM && !anyLane(region != r0)) sampleTrianglesAdd(s, s.regionRec[r0], p, P, cnt);   // wave-uniform index: one record per wave
    else sampleTrianglesAdd(s, s.regionRec[region], p, P, cnt);
  }
}

// the steps o = first, first / 2, .. 1 of the contract's tree, P_l = P_l + P_{l+o} for l < o (the lanes from o on hold what
// nobody reads); every lane of the wave takes part
__device__ __forceinline__ void sampleTrianglesTree(int first, double P[EXA_SURFACE_MAX_CHANNELS], uint32_t cnt[EXA_SURFACE_MAX_CHANNELS])
{
  for (int o = first; o >= 1; o >>= 1) {
#pragma unroll
    for (int c = 0; c < EXA_SURFACE_MAX_CHANNELS; c++) {
      P[c] = P[c] + __shfl_down(P[c], o, 64);
      cnt[c] += __shfl_down(cnt[c], o, 64);
    }
  }
}

__device__ __forceinline__ void sampleTrianglesStore(const TriArgs &a, int t, const double P[EXA_SURFACE_MAX_CHANNELS],
                                                     const uint32_t cnt[EXA_SURFACE_MAX_CHANNELS])
{
  const size_t at = size_t(t) * size_t(a.s.numChannels);
#pragma unroll
  for (int c = 0; c < EXA_SURFACE_MAX_CHANNELS; c++)
    if (c < a.s.numChannels) {
      if (a.sum) a.sum[at + c] = P[c];
      if (a.count) a.count[at + c] = cnt[c];
    }
}

// First kernel, one lane per triangle: areaNormal and subdiv, the results of a triangle that is not valid, and the valid ones
// handed to the second kernel through a.list — at most 16 samples (with a.pack): from the front, its packed part; more: from
// the back, its wide part.  A wave appends with one atomic per end; the order of the entries varies from run to
// run and no byte depends on it (every result is stored by triangle).
__global__ __launch_bounds__(256) void sampleTrianglesPrepKernel(const TriArgs a)
{
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t t = blockIdx.x * 256u + threadIdx.x;
  const bool have = t < a.numTriangles;
  int n = 0;
  if (have) {
    const int32_t *idx = a.triangles + 3 * size_t(t);
    const int32_t i0 = idx[0], i1 = idx[1], i2 = idx[2];
    const unsigned long long nv = a.numVertices;
    V3 an = mk(NAN, NAN, NAN);
    if (i0 >= 0 && i1 >= 0 && i2 >= 0 && (unsigned long long)i0 < nv && (unsigned long long)i1 < nv && (unsigned long long)i2 < nv) {
      const V3 v0 = mk(a.vertices + 3 * size_t(i0)), v1 = mk(a.vertices + 3 * size_t(i1)), v2 = mk(a.vertices + 3 * size_t(i2));
      const V3 e1 = v1 - v0, e2 = v2 - v0;
      an = 0.5f * cross(e1, e2);
      n = sampleTrianglesSubdiv(v0, v1, v2, a.spacing, a.maxN);
    }
    if (a.areaNormal) { a.areaNormal[3 * size_t(t)] = an.x; a.areaNormal[3 * size_t(t) + 1] = an.y; a.areaNormal[3 * size_t(t) + 2] = an.z; }
    if (a.subdiv) a.subdiv[t] = n;
    if (n == 0) {
      const double zero[EXA_SURFACE_MAX_CHANNELS] = { 0.0, 0.0, 0.0, 0.0 };
      const uint32_t none[EXA_SURFACE_MAX_CHANNELS] = { 0u, 0u, 0u, 0u };
      sampleTrianglesStore(a, int(t), zero, none);
    }
  }
  const bool packed = n > 0 && a.pack && n <= 4, wide = n > 0 && !packed;
  const unsigned long long mp = __builtin_amdgcn_ballot_w64(packed), mw = __builtin_amdgcn_ballot_w64(wide);
  uint32_t bp = 0u, bw = 0u;
  if (lane == 0u) {
    if (mp) bp = atomicAdd(a.listCount, uint32_t(__popcll(mp)));
    if (mw) bw = atomicAdd(a.listCount + 1, uint32_t(__popcll(mw)));
  }
  bp = __shfl(bp, 0, 64);
  bw = __shfl(bw, 0, 64);
  const unsigned long long below = (1ull << lane) - 1ull;
  if (packed) a.list[bp + uint32_t(__popcll(mp & below))] = int32_t(t);
  if (wide) a.list[a.numTriangles - 1u - (bw + uint32_t(__popcll(mw & below)))] = int32_t(t);
}

// Packed: a wave takes 64 entries from the front of the list, a lane each, and serves them in three rounds by the size G of
// the group of lanes a triangle needs — n = 1: G = 1, every lane its own triangle at once; n = 2: G = 4, sixteen triangles at a
// time; n = 3, 4: G = 16, four at a time —, the owner's triangle handed to its group's lanes by shuffles.  A slot l of the
// contract holds at most one sample here, P_l = +0.0 + v; the tree's steps above G add the +0.0 of the empty slots, which
// changes no P_l (none is -0.0), then its steps below G run inside the group.
template <bool UNIFORM>
__device__ __forceinline__ void sampleTrianglesPacked(const TriArgs &a, const float xfm[12], bool &tripped)
{
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t numPacked = a.listCount[0], waves = gridDim.x * 4u;
  for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); (unsigned long long)w * 64u < numPacked; w += waves) {
    const uint32_t i = w * 64u + lane;
    int t = -1;
    TriGeom g;
    g.v0 = mk(0.f, 0.f, 0.f); g.e1 = g.v0; g.e2 = g.v0; g.n = 0;
    if (i < numPacked) { t = a.list[i]; g = sampleTrianglesGeom(a, t); }
    const int G = g.n == 0 ? 0 : (g.n == 1 ? 1 : (g.n == 2 ? 4 : 16));
    if (anyLane(G == 1)) {
      double P[EXA_SURFACE_MAX_CHANNELS] = { 0.0, 0.0, 0.0, 0.0 };
      uint32_t cnt[EXA_SURFACE_MAX_CHANNELS] = { 0u, 0u, 0u, 0u };
      sampleTrianglesAt<UNIFORM>(a.s, xfm, G == 1, sampleTrianglesPos(g, 0), tripped, P, cnt);
      if (G == 1) sampleTrianglesStore(a, t, P, cnt);
    }
    for (int GG = 4; GG <= 16; GG *= 4) {
      unsigned long long mask = __builtin_amdgcn_ballot_w64(G == GG);
      const int per = 64 / GG, slot = int(lane) / GG, k = int(lane) % GG;
      while (mask) {
        // the owners of this round: the lowest `per` lanes of the mask, in order (wave-uniform arithmetic)
        int owner = -1;
        for (int j = 0; j < per && mask; j++) {
          const int o = __ffsll(mask) - 1;
          mask &= mask - 1ull;
          if (slot == j) owner = o;
        }
        const int src = owner >= 0 ? owner : int(lane);
        TriGeom h;
        h.v0 = mk(__shfl(g.v0.x, src, 64), __shfl(g.v0.y, src, 64), __shfl(g.v0.z, src, 64));
        h.e1 = mk(__shfl(g.e1.x, src, 64), __shfl(g.e1.y, src, 64), __shfl(g.e1.z, src, 64));
        h.e2 = mk(__shfl(g.e2.x, src, 64), __shfl(g.e2.y, src, 64), __shfl(g.e2.z, src, 64));
        h.n = __shfl(g.n, src, 64);
        const int ht = __shfl(t, src, 64);
        double P[EXA_SURFACE_MAX_CHANNELS] = { 0.0, 0.0, 0.0, 0.0 };
        uint32_t cnt[EXA_SURFACE_MAX_CHANNELS] = { 0u, 0u, 0u, 0u };
        sampleTrianglesAt<UNIFORM>(a.s, xfm, owner >= 0 && k < h.n * h.n, sampleTrianglesPos(h, k), tripped, P, cnt);
        sampleTrianglesTree(GG / 2, P, cnt);
        if (owner >= 0 && k == 0) sampleTrianglesStore(a, ht, P, cnt);
      }
    }
  }
}

// Wide: a wave takes one entry from the back of the list and loops over its blocks of 64 samples, lane l holding the
// contract's P_l and its count in registers — sample k = 64 j + l is added in block j, so in ascending k —, then the whole tree.
template <bool UNIFORM>
__device__ __forceinline__ void sampleTrianglesWide(const TriArgs &a, const float xfm[12], bool &tripped)
{
  const unsigned lane = threadIdx.x & 63u;
  const uint32_t numWide = a.listCount[1], waves = gridDim.x * 4u;
  for (uint32_t w = blockIdx.x * 4u + (threadIdx.x >> 6); w < numWide; w += waves) {
    const int t = a.list[a.numTriangles - 1u - w];                     // the same in every lane; held per lane, as its triangle
    const TriGeom g = sampleTrianglesGeom(a, t);
    const int nn = g.n * g.n;
    double P[EXA_SURFACE_MAX_CHANNELS] = { 0.0, 0.0, 0.0, 0.0 };
    uint32_t cnt[EXA_SURFACE_MAX_CHANNELS] = { 0u, 0u, 0u, 0u };
    for (int k0 = 0; k0 < nn; k0 += 64) {
      const int k = k0 + int(lane);
      sampleTrianglesAt<UNIFORM>(a.s, xfm, k < nn, sampleTrianglesPos(g, k), tripped, P, cnt);
    }
    sampleTrianglesTree(32, P, cnt);
    if (lane == 0u) sampleTrianglesStore(a, t, P, cnt);
  }
}

// Second kernel: the waves stride first over the packed part of the list, 64 entries each, then over the wide part, one entry
// each — one launch, so that neither part waits for the other's last waves
template <bool UNIFORM>
__global__ __launch_bounds__(256) void sampleTrianglesKernel(const TriArgs a)
{
  __shared__ float xfm[12];
  sampleTrianglesStageXfm(a.s, xfm);
  bool tripped = false;
  sampleTrianglesPacked<UNIFORM>(a, xfm, tripped);
  sampleTrianglesWide<UNIFORM>(a, xfm, tripped);
  if (tripped) atomicExch(a.s.errorFlag, 1);
}

// the two kernels on the triangles of a, in order; the one that samples runs as at most kSampleTrianglesBlocks blocks whose
// waves stride over the list (the lengths of its two parts are known on the device only)
static const unsigned kSampleTrianglesBlocks = 16384;

hipError_t launchSampleTriangles(const TriArgs &a, bool uniform, hipStream_t s)
{
  const unsigned m = a.numTriangles;
  if (m == 0) return hipSuccess;
  const dim3 block(256), grid(std::min(m / 4u + 1u, kSampleTrianglesBlocks));
  hipLaunchKernelGGL(sampleTrianglesPrepKernel, dim3((m + 255u) / 256u), block, 0, s, a);
  if (uniform) hipLaunchKernelGGL((sampleTrianglesKernel<true>), grid, block, 0, s, a);
  else         hipLaunchKernelGGL((sampleTrianglesKernel<false>), grid, block, 0, s, a);
  return hipGetLastError();
}

hipError_t launchSamplePoints(const SampleArgs &a, bool grad, hipStream_t s)
{
  if (a.count == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.count + 255) / 256)), block(256);
  if (grad && a.normalized) hipLaunchKernelGGL(samplePointsNormKernel, grid, block, 0, s, a);
  else if (grad) hipLaunchKernelGGL((samplePointsKernel<true>), grid, block, 0, s, a);
  else      hipLaunchKernelGGL((samplePointsKernel<false>), grid, block, 0, s, a);
  return hipGetLastError();
}

// a launcher of a grid kernel K<PX, PY, PZ, UNIFORM>: one wave per patch of shape `shape`
#define EXA_GRID_LAUNCHER(NAME, K)                                                                                       \
  hipError_t NAME(const SampleArgs &a, int shape, bool uniform, hipStream_t s)                                           \
  {                                                                                                                      \
    if (a.numPatches == 0) return hipSuccess;                                                                            \
    const dim3 grid((unsigned)((a.numPatches + 3) / 4)), block(256);                                                     \
    switch (shape * 2 + (uniform ? 1 : 0)) {                                                                             \
    case 0: hipLaunchKernelGGL((K<64, 1, 1, false>), grid, block, 0, s, a); break;                                       \
    case 1: hipLaunchKernelGGL((K<64, 1, 1, true>), grid, block, 0, s, a); break;                                        \
    case 2: hipLaunchKernelGGL((K<16, 4, 1, false>), grid, block, 0, s, a); break;                                       \
    case 3: hipLaunchKernelGGL((K<16, 4, 1, true>), grid, block, 0, s, a); break;                                        \
    case 4: hipLaunchKernelGGL((K<8, 8, 1, false>), grid, block, 0, s, a); break;                                        \
    case 5: hipLaunchKernelGGL((K<8, 8, 1, true>), grid, block, 0, s, a); break;                                         \
    case 6: hipLaunchKernelGGL((K<4, 4, 4, false>), grid, block, 0, s, a); break;                                        \
    case 7: hipLaunchKernelGGL((K<4, 4, 4, true>), grid, block, 0, s, a); break;                                         \
    default: return hipErrorInvalidValue;                                                                                \
    }                                                                                                                    \
    return hipGetLastError();                                                                                            \
  }
EXA_GRID_LAUNCHER(launchSampleGrid, sampleGridKernel)
EXA_GRID_LAUNCHER(launchSampleDerivedGrid, sampleDerivedGridKernel)
#undef EXA_GRID_LAUNCHER

hipError_t launchSampleDerivedPoints(const SampleArgs &a, hipStream_t s)
{
  if (a.count == 0) return hipSuccess;
  hipLaunchKernelGGL(sampleDerivedPointsKernel, dim3((unsigned)((a.count + 255) / 256)), dim3(256), 0, s, a);
  return hipGetLastError();
}
