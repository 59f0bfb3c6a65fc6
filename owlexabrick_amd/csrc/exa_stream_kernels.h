// exa_stream_kernels.h — the streamline integrator of exa_hip_streamlines: classical RK4 through three channels of the
// reconstructed field, one lane per (seed, requested direction).  Included by exa_kernels.hip inside namespace
// exa::EXA_FORM_NS when it is compiled with -DEXA_TU_STREAM=1 (exa_stream_f0.o, exa_stream_f1.o, exa_stream_f0e.o), after
// the basis evaluations it uses; nothing else of the renderer is compiled there.
//
// Contract (include/exa_hip.h): an evaluation E(q) is what exa_hip_sample_points(q, channels, 3, flags = 0) returns — the
// probes' lookup (exa_sample_locate.h) and addBasisFast on the march headers, the same calls in the same order, so a stage
// equals the points kernel bit for bit.  The step is the reference's RK4 (exabrick.cu:1531-1574) expression for expression,
// nothing contracted; what differs from computeTracesKernel is the lookup (no ray through the TF-refit volume BVH), the
// whole line in one launch, both directions, the normalised mode and the reasons.
//
// An extraction is two launches of the same integration (it is deterministic): COUNT stores per direction the number of
// vertices appended after the seed and why the direction ended; the host scans the counts; EMIT integrates again and
// stores vertex j of a direction at line offset + seedVertex +- j.  Nothing of size seeds x maxSteps exists.
#include "exa_sample_locate.h"

// E(q): 0 and the velocity v / the direction d, or the reason the evaluation fails.  Order: lookup, channels, speed.
// Brick loop outside, channels inside: the three addBasisFast calls of a brick share its two header loads, its cell
// coordinates, predicates and masked per-axis weights (the same pure expressions of h0, h1 and q: formed once), and each
// channel's sums see the additions of sampleSums on that channel in the same order.
// Args: StreamArgs, or the LicArgs of exa_lic_kernels.h (a.s is all that is read).
template <bool NORM, typename Args>
__device__ __forceinline__ int streamEval(const Args &a, V3 q, V3 &v, V3 &d, bool &tripped)
{
  const int region = sampleInRoot(a.s, q) ? sampleKdLeaf(a.s, a.s.kdRoot, q, tripped) : -1;
  if (region < 0) return EXA_STREAM_END_LEFT;
  const RegionRec R = a.s.regionRec[region];
  if (!sampleInDomain(R, q)) return EXA_STREAM_END_LEFT;
  const float *f0 = a.s.scalars + a.s.fieldOffset[0], *f1 = a.s.scalars + a.s.fieldOffset[1], *f2 = a.s.scalars + a.s.fieldOffset[2];
  Ctx<0> C;                       // no counters
  Basis B0, B1, B2;
  B0.sumWV = 0.f; B0.sumW = 0.f; B0.sumD = mk(0.f, 0.f, 0.f); B0.sumDC = mk(0.f, 0.f, 0.f);
  B1 = B0; B2 = B0;
  for (int child = 0; child < R.listSize; child++) {
    const size_t at = 2 * (size_t(R.listBegin) + size_t(child));
    const int4 h0 = a.s.leafHdr[at], h1 = a.s.leafHdr[at + 1];
    addBasisFast<false, 0, false>(C, B0, h0, h1, f0, q);
    addBasisFast<false, 0, false>(C, B1, h0, h1, f1, q);
    addBasisFast<false, 0, false>(C, B2, h0, h1, f2, q);
  }
  if (B0.sumW <= 1e-20f || B1.sumW <= 1e-20f || B2.sumW <= 1e-20f) return EXA_STREAM_END_NOVALUE;
  v = mk(B0.sumWV / B0.sumW, B1.sumWV / B1.sumW, B2.sumWV / B2.sumW);
  d = v;
  if (NORM) {
    // sqrtf and `/`: the compiler's correctly rounded expansions (__fsqrt_rn is the bare instruction, 1 ulp)
    const float s = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    if (!(s > 0.f) || !(s <= FLT_MAX)) return EXA_STREAM_END_STAGNANT;
    d = mk(v.x / s, v.y / s, v.z / s);
  }
  return 0;
}

__device__ __forceinline__ void streamStore(float *dst, unsigned long long at, V3 x)
{
  dst[3 * at] = x.x; dst[3 * at + 1] = x.y; dst[3 * at + 2] = x.z;
}

// One lane per (seed, direction).  Every evaluation goes through ONE call site: the lane carries which stage of the step
// its next evaluation is (0: the candidate vertex q itself — the seed, or a step's pn —, 1..3: the stages k2..k4), so the
// lanes of a wave evaluate side by side whatever stage each is in, and the body is one copy of the basis code.
template <bool EMIT, bool NORM>
__global__ __launch_bounds__(256) void streamlinesKernel(const StreamArgs a)
{
  const unsigned long long lane = a.laneBase + (unsigned long long)blockIdx.x * 256u + threadIdx.x;
  if (lane >= a.numLanes) return;
  const bool both = (a.flags & (EXA_STREAM_FORWARD | EXA_STREAM_BACKWARD)) == (EXA_STREAM_FORWARD | EXA_STREAM_BACKWARD);
  const unsigned long long seed = both ? lane >> 1 : lane;
  const int slot = both ? int(lane & 1u) : ((a.flags & EXA_STREAM_FORWARD) ? 1 : 0);      // 0 backward, 1 forward
  const float hs = slot ? a.step : -a.step;
  // EMIT: vertex j of this direction goes to base + j (forward) or base - j (backward); the seed (j = 0) is stored by the
  // forward lane, or by the backward lane when it is alone; `limit` = the count of the first launch bounds every store
  unsigned long long base = 0;
  uint32_t limit = 0;
  if (EMIT) {
    base = a.offsets[seed] + a.seedVertex[seed];
    limit = a.counts[2 * seed + slot];
  }
  const bool ownsSeed = slot == 1 || !both;
  V3 p = mk(a.seeds + 3 * seed);
  V3 q = p, acc = mk(0.f, 0.f, 0.f), v = mk(0.f, 0.f, 0.f), d = v;
  if (EMIT && ownsSeed) streamStore(a.vertices, base, p);
  bool tripped = false;
  int stage = 0, reason = EXA_STREAM_END_MAXSTEPS;
  uint32_t appended = 0;           // vertices after the seed
  bool haveSeed = false;
  // at most four evaluations per step and one for the seed (maxSteps <= EXA_STREAM_MAX_STEPS = 2^20)
  for (int e = 0, ne = 4 * a.maxSteps + 1; e < ne; e++) {
    const int r = streamEval<NORM>(a, q, v, d, tripped);
    if (r) { reason = r; break; }
    if (stage == 0) {
      // q holds a value in all three channels: the seed, or the vertex a step appends
      if (haveSeed) {
        appended++;
        if (EMIT && appended <= limit) {
          const unsigned long long at = slot ? base + appended : base - appended;
          streamStore(a.vertices, at, q);
          if (a.velocities) streamStore(a.velocities, at, v);
        }
      } else {
        haveSeed = true;
        if (EMIT && ownsSeed && a.velocities) streamStore(a.velocities, base, v);
      }
      p = q;
      if (appended >= uint32_t(a.maxSteps)) break;                 // MAXSTEPS
      const V3 k1 = hs * d;
      acc = k1;
      q = p + .5f * k1;
      stage = 1;
    } else if (stage == 1) {
      const V3 k2 = hs * d;
      acc = acc + 2.f * k2;
      q = p + .5f * k2;
      stage = 2;
    } else if (stage == 2) {
      const V3 k3 = hs * d;
      acc = acc + 2.f * k3;
      q = p + k3;
      stage = 3;
    } else {
      const V3 k4 = hs * d;
      acc = acc + k4;                                              // ((k1 + 2 k2) + 2 k3) + k4
      q = p + (1 / 6.f) * acc;
      if (__float_as_int(q.x) == __float_as_int(p.x) && __float_as_int(q.y) == __float_as_int(p.y) &&
          __float_as_int(q.z) == __float_as_int(p.z)) { reason = EXA_STREAM_END_STAGNANT; break; }
      stage = 0;
    }
  }
  if (tripped) atomicExch(a.s.errorFlag, 1);
  if (EMIT) {
    // a seed whose own evaluation fails: a one-vertex line without a velocity
    const float nan = __int_as_float(0x7fc00000);
    if (!haveSeed && ownsSeed && a.velocities) streamStore(a.velocities, base, mk(nan, nan, nan));
  } else {
    a.counts[2 * seed + slot] = appended;
    a.reasons[2 * seed + slot] = reason;
  }
}

hipError_t launchStreamlines(const StreamArgs &a, bool emit, hipStream_t s)
{
  if (a.laneBase >= a.numLanes) return hipSuccess;
  const unsigned long long lanes = a.numLanes - a.laneBase < (1ull << 24) ? a.numLanes - a.laneBase : (1ull << 24);
  const dim3 grid((unsigned)((lanes + 255) / 256)), block(256);
  const bool norm = (a.flags & EXA_STREAM_NORMALIZE) != 0;
  if (emit && norm)  hipLaunchKernelGGL((streamlinesKernel<true, true>), grid, block, 0, s, a);
  else if (emit)     hipLaunchKernelGGL((streamlinesKernel<true, false>), grid, block, 0, s, a);
  else if (norm)     hipLaunchKernelGGL((streamlinesKernel<false, true>), grid, block, 0, s, a);
  else               hipLaunchKernelGGL((streamlinesKernel<false, false>), grid, block, 0, s, a);
  return hipGetLastError();
}
