// exa_kernels.hip — hand-written HIP kernels for gfx950 (MI355X, wave64).
//
// One thread per pixel, one wave per 8x8 pixel block, one 256-thread workgroup
// per 16x16 tile.  Replaces the OptiX raygen program `renderFrame` and the
// VolumeBVH / IsoSurface bounds+intersect programs of programs/exabrick.cu.
// Arithmetic order follows the reference expression by expression (cited per
// function); the file is built with -ffp-contract=off so results can be
// compared against the CPU oracle operation for operation.
#include "exa_device.h"
#include <cfloat>
#include <type_traits>

// Instruction trims of the kd march that keep every pixel bit for bit (measured one by one in rounds 2-4,
// profiles/design_history_r01_r03.md, profiles/r04_experiments.txt; the build-time switches they were A/B-timed with are gone):
//   one pop site in the kd step instead of five inlined copies
//   cell loads as uniform base + 32-bit byte offset (global_load saddr form) when a field is < 4 GiB (SMALL)
//   24-bit integer multiplies in the cell address (full rate; v_mul_lo_u32 / v_mad_u64_u32 are quarter rate) (SMALL)
//   the march header carries float(lower) and 2^-level: no conversions / exponent build per visit; the -1 clamp
//   of the cell index is done on the float
//   first sample of a segment: x / dt as x * (1/dt) when dt is a power of two (exact)
//   clamp(l, 0, size-1) as one v_med3_i32
#if EXA_BASIS_FORM == 0 && EXA_EMPTY_CELLS
#define EXA_FORM_NS form0e
#elif EXA_BASIS_FORM == 0
#define EXA_FORM_NS form0
#elif EXA_BASIS_FORM == 1 && EXA_EMPTY_CELLS
#error "empty cells are a per-corner property: the per-axis association (EXA_BASIS_FORM 1) does not apply"
#elif EXA_BASIS_FORM == 1
#define EXA_FORM_NS form1
#else
#error "EXA_BASIS_FORM is 0 (source order) or 1 (per-axis association with fused multiply-adds)"
#endif
// form 1 also fuses the multiply-adds around the basis sums, each mirrored in the oracle (or_set_basis_form): the DVR sample
// position org + t * dir, the cell coordinate (pos - lower) * 2^-level - 0.5, the gradient sumW * sumD - sumWV * sumDC, the
// three dot products of the shading factor and the colour terms of the "over" operator
#define EXA_F1 (EXA_BASIS_FORM == 1)
// The march on the rope walk is compiled in translation units of its own (-DEXA_TU_ROPE=1: exa_kernels_f*r.o hold
// launchRenderKdRope and nothing else), side by side with the others.
#ifndef EXA_TU_ROPE
#define EXA_TU_ROPE 0
#endif
// The point probes likewise (-DEXA_TU_SAMPLE=1: exa_sample_f*.o, the kernels of exa_sample_kernels.h and nothing else).
#ifndef EXA_TU_SAMPLE
#define EXA_TU_SAMPLE 0
#endif
// The streamline integrator likewise (-DEXA_TU_STREAM=1: exa_stream_f*.o, the kernels of exa_stream_kernels.h and nothing else).
#ifndef EXA_TU_STREAM
#define EXA_TU_STREAM 0
#endif
namespace exa {
namespace EXA_FORM_NS {

// ------------------------------------------------------------------------
// small vector helpers (owl::vec3f semantics: componentwise, left-to-right dot)
// ------------------------------------------------------------------------
struct V3 { float x, y, z; };
__device__ __forceinline__ V3 mk(float x, float y, float z) { V3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ V3 mk(const float *p) { return mk(p[0], p[1], p[2]); }
__device__ __forceinline__ V3 operator+(V3 a, V3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ V3 operator-(V3 a, V3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ V3 operator*(float s, V3 a) { return mk(s * a.x, s * a.y, s * a.z); }
__device__ __forceinline__ V3 operator-(V3 a) { return mk(-a.x, -a.y, -a.z); }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// the same sum, left to right, with the two additions fused into their products
__device__ __forceinline__ float dotF(V3 a, V3 b) { return EXA_F1 ? __builtin_fmaf(a.z, b.z, __builtin_fmaf(a.y, b.y, a.x * b.x)) : dot(a, b); }
// exabrick.cu:916-918: sumW * sumD - sumWV * sumDC per component
__device__ __forceinline__ V3 gradOf(float sumW, float sumWV, V3 sumD, V3 sumDC)
{
  return EXA_F1 ? mk(__builtin_fmaf(sumW, sumD.x, -(sumWV * sumDC.x)), __builtin_fmaf(sumW, sumD.y, -(sumWV * sumDC.y)),
                     __builtin_fmaf(sumW, sumD.z, -(sumWV * sumDC.z)))
                : mk(sumW * sumD.x - sumWV * sumDC.x, sumW * sumD.y - sumWV * sumDC.y, sumW * sumD.z - sumWV * sumDC.z);
}
__device__ __forceinline__ V3 rayAt(V3 org, float t, V3 dir)
{ return EXA_F1 ? mk(__builtin_fmaf(t, dir.x, org.x), __builtin_fmaf(t, dir.y, org.y), __builtin_fmaf(t, dir.z, org.z)) : org + t * dir; }
__device__ __forceinline__ float length(V3 a) { return sqrtf(dot(a, a)); }
__device__ __forceinline__ V3 normalize(V3 a) { return (1.f / sqrtf(dot(a, a))) * a; }
__device__ __forceinline__ V3 cross(V3 a, V3 b)
{ return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }

// owl xfmPoint / xfmVector (embree-style madd chains)
__device__ __forceinline__ V3 xfmPoint(const ExaHipFrameState &fs, V3 p)
{ return p.x * mk(fs.xfm_vx) + (p.y * mk(fs.xfm_vy) + (p.z * mk(fs.xfm_vz) + mk(fs.xfm_p))); }
__device__ __forceinline__ V3 xfmVector(const ExaHipFrameState &fs, V3 v)
{ return v.x * mk(fs.xfm_vx) + (v.y * mk(fs.xfm_vy) + v.z * mk(fs.xfm_vz)); }

// owl::common::LCG<16>
struct Lcg {
  uint32_t state;
  __device__ __forceinline__ void init(uint32_t v0, uint32_t v1)
  {
    uint32_t s0 = 0;
#pragma unroll
    for (int n = 0; n < 16; n++) {
      s0 += 0x9e3779b9u;
      v0 += ((v1 << 4) + 0xa341316cu) ^ (v1 + s0) ^ ((v1 >> 5) + 0xc8013ea4u);
      v1 += ((v0 << 4) + 0xad90777du) ^ (v0 + s0) ^ ((v0 >> 5) + 0x7e95761eu);
    }
    state = v0;
  }
  __device__ __forceinline__ float next()
  {
    state = 1664525u * state + 1013904223u;
    return float(state & 0x00FFFFFFu) / float(0x01000000);
  }
};

// FAST (fast_math=1): 1-ulp hardware reciprocal / square root in the per-sample epilogue instead of the
// correctly rounded expansions (~10 instructions each); the walk and the sample positions stay exact
template <bool FAST> __device__ __forceinline__ float fdiv(float a, float b) { return FAST ? a * __builtin_amdgcn_rcpf(b) : a / b; }
// The quotients that decide WHICH transfer-function texels a sample blends and with which 1/256 weight (the cell value
// sumWV/sumW and the two divisions of the TF coordinate) get one correction step on top of the fast form: q = a*y with
// y = rcp(b) is within ~1.5 ulp, the remainder r = a - q*b is exact in an fma, and q + r*y rounds to the correctly
// rounded quotient except at near-ties (none in 2e7 random trials; the plain fast form is off by an ulp in 2 of 3).
// An ulp there is not harmless: the filter weight is quantised, so it can move a sample's opacity by a whole step
// |T[i+1].a - T[i].a| / 256 (seeded random TF tables: accumulation differences of 2e-3).  q is clamped to the finite
// range first, so that an overflowing quotient still saturates the TF coordinate instead of turning into inf - inf.
template <bool FAST> __device__ __forceinline__ float fdivExact(float a, float b, float y /* rcp(b), FAST only */)
{
  if (!FAST) return a / b;
  const float q = __builtin_amdgcn_fmed3f(a * y, -3.402823466e+38f, 3.402823466e+38f);
  return __builtin_fmaf(__builtin_fmaf(-q, b, a), y, q);
}
template <bool FAST> __device__ __forceinline__ float fdivExact(float a, float b) { return fdivExact<FAST>(a, b, FAST ? __builtin_amdgcn_rcpf(b) : 0.f); }
template <bool FAST> __device__ __forceinline__ float fsqrt(float a) { return FAST ? __builtin_amdgcn_sqrtf(a) : sqrtf(a); }

struct Ray { V3 org, dir; float tmin, tmax; };

// LEAN (the variants of the march compiled for seven waves per SIMD: 72 registers): a value the compiler cannot see through, so
// that what is computed from it is computed where it is used instead of once before the march loop and kept in a register across it
__device__ __forceinline__ float opaque(float x) { asm volatile("" : "+v"(x)); return x; }

// "does any active lane want this": the compare's lane mask tested directly (v_cmp + s_cmp); HIP's anyLane() first
// turns the flag into a register value and compares that again
__device__ __forceinline__ bool anyLane(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0ull; }

// exabrick.cu:1588,1703-1707: the viewer's clock heat map — red = clockScale * (cycles this ray's program ran) / 1e6.
// The start stamp is wave-uniform and stays in scalar registers; with a surfaces pre-pass only the march is timed.
__device__ __forceinline__ float clockHeat(float clockScale, unsigned long long clockBegin)
{
  const unsigned long long absClock = clock64() - clockBegin;
  const float relClock = clockScale * (float)absClock / 1000000.f;
  return fminf(relClock, 1.f);
}
struct Color4 { float x, y, z, w; };

// lane -> pixel inside the wave's 8x8 block: along a Morton curve, so that a quad of lanes is a 2x2
// pixel block and 16 lanes a 4x4 block instead of 4x1 / 8x2 strips: the vector memory path handles a wave's gather
// lane group by lane group and merges the lanes of a group that fall into the same cache line, and the march is bound by
// the number of such accesses (TCP_TOTAL_CACHE_ACCESSES = one per clock and CU over the whole frame) —
// closer pixels share more lines.  Pixels do not depend on which lane renders them.
__device__ __forceinline__ int laneX(int lane) { return (lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4); }
__device__ __forceinline__ int laneY(int lane) { return ((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4); }

// per-thread view of the kernel state.  STATS: 0 = the shipped kernel, 1 = work counters (sample for sample the
// oracle's), 2 = wave time by phase only (the shipped code plus a clock read at every phase change)
template <int STATS>
struct Ctx {
  const RenderArgs *a;
  const float4 *xfLds;         // TF tables staged in LDS
  int *stack;                  // this thread's LBVH stack column in LDS (stride 256)
  unsigned long long st[ST_COUNT];
  bool guardTripped;
  bool fastSampler = false;    // samplePoint: masked-weight basis on the march headers (kd kernels) or the literal form
  unsigned isoSteps = 0;       // steps of this lane's iso marches (pre-pass cost of its pixel, for the launch plan)
  uint32_t *probe = nullptr;   // walk probe (counting variant): this wave's set of visited kd nodes
  // adds a node id to the wave's set (open addressing in global memory); new members are counted
  __device__ __forceinline__ void probeNode(int ref)
  {
    if (STATS != 1 || !probe) return;
    const uint32_t key = (uint32_t)ref + 1u;
    uint32_t h = (key * 2654435761u) >> (32 - kWalkProbeBits);
    for (int i = 0; i < kWalkProbeSize; i++) {
      const uint32_t prev = atomicCAS(&probe[h], 0u, key);
      if (prev == 0u) { st[ST_UNION]++; return; }
      if (prev == key) return;
      h = (h + 1u) & (kWalkProbeSize - 1u);
    }
    st[ST_PROBE_OVERFLOW]++;
  }
  __device__ __forceinline__ void count(int slot, unsigned long long n = 1) { if (STATS == 1) st[slot] += n; }
  // wave time by phase (instrumented variant): the cycles since the wave's previous mark go to the phase that
  // mark opened; one lane of the active set keeps the books, the mark itself lives in LDS (per wave)
  unsigned long long *lapMark;   // this wave's record in LDS: [0] time of the last mark, [1] its phase, [2..6] cycles per phase
  __device__ __forceinline__ void lap(int phaseSlot)
  {
    if (STATS == 2) {
      const unsigned long long now = clock64();
      const unsigned long long m = __ballot(1);
      if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) {
        lapMark[2 + lapMark[1]] += now - lapMark[0];
        lapMark[0] = now; lapMark[1] = (unsigned long long)(phaseSlot - ST_T_BRICK);
      }
    }
  }
  // one count per wave execution (first active lane) + one per active lane
  __device__ __forceinline__ void phase(int waveSlot)
  {
    if (STATS == 1) {
      const unsigned long long m = __ballot(1);
      if ((threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) st[waveSlot]++;
      st[waveSlot + 1]++;
    }
  }
};

// ------------------------------------------------------------------------
// exabrick.cu:53-76  sRGB + 8-bit pack
// ------------------------------------------------------------------------
__device__ __forceinline__ float linear_to_srgb(float x)
{
  if (x <= 0.0031308f) return 12.92f * x;
  return 1.055f * powf(x, 1.f / 2.4f) - 0.055f;
}
__device__ __forceinline__ uint32_t make_8bit(float f) { return (uint32_t)min(255, max(0, int(f * 256.f))); }
__device__ __forceinline__ uint32_t make_rgba8(float r, float g, float b)
{ return (make_8bit(r) << 0) + (make_8bit(g) << 8) + (make_8bit(b) << 16) + (0xffu << 24); }

// ------------------------------------------------------------------------
// exabrick.cu:135-150 lookupTransferFunction; the tex1D<float4> fetch (128 texels, linear, clamp,
// normalized coords; exa/Texture.h:141-147) is a software lerp on the LDS-resident table:
// x = u*128-0.5, T[i]*(1-a) + T[i+1]*a.  The CUDA programming guide ("Texture Fetching", linear
// filtering) publishes that the unit holds the weight a in 9-bit fixed point with 8 fractional bits:
// fracMagic = 2^15 rounds a to the nearest 1/256 (a float in [2^15, 2^16) has exactly 8 fractional
// bits), fracMagic = 0 keeps the full-precision weight (option tf_filter).
// ------------------------------------------------------------------------
template <bool FAST = false, bool HAVE_RCP = false>
__device__ __forceinline__ Color4 lookupXF(const float4 *xf, const ExaHipFrameState &fs, float in_scalar, int channel,
                                           const float fracMagic, const float rcpRange = 0.f, const float range = 0.f)
{
  // HAVE_RCP (fast_math only): range / rcpRange are the caller's copies of (hi - lo) + 1e-20f and of its rcp, the values
  // fdiv<true> works out here — wave-uniform and the same for every sample of the frame, formed once by the caller
  const float lo = fs.xfDomain[channel][0], hi = fs.xfDomain[channel][1];
  float scalar = (FAST && HAVE_RCP) ? fdivExact<true>((EXA_NUM_XF_VALUES - 1) * (in_scalar - lo), range, rcpRange)
                                    : fdivExact<FAST>((EXA_NUM_XF_VALUES - 1) * (in_scalar - lo), (hi - lo) + 1e-20f);
  scalar = fminf(EXA_NUM_XF_VALUES - 1.f, fmaxf(0.f, scalar + .5f));
  if (FAST) {        // scalar in [0, 127]: no clamp needed; 1/127 as a constant
    const float q = scalar * (1.f / (EXA_NUM_XF_VALUES - 1.f));
    scalar = __builtin_fmaf(__builtin_fmaf(-q, EXA_NUM_XF_VALUES - 1.f, scalar), 1.f / (EXA_NUM_XF_VALUES - 1.f), q);
  } else {
    scalar = scalar / (EXA_NUM_XF_VALUES - 1.f);
  }
  const float x = scalar * float(EXA_NUM_XF_VALUES) - 0.5f;
  const float fl = floorf(x);
  const float al = ((x - fl) + fracMagic) - fracMagic;
  const int i0 = min(EXA_NUM_XF_VALUES - 1, max(0, int(fl)));
  const int i1 = min(EXA_NUM_XF_VALUES - 1, max(0, int(fl) + 1));
  const float4 T0 = xf[channel * EXA_NUM_XF_VALUES + i0];
  const float4 T1 = xf[channel * EXA_NUM_XF_VALUES + i1];
  const float na = 1.f - al;
  Color4 r;
  r.x = na * T0.x + al * T1.x;
  r.y = na * T0.y + al * T1.y;
  r.z = na * T0.z + al * T1.z;
  r.w = na * T0.w + al * T1.w;
  r.w *= fs.xfOpacityScale;
  return r;
}

// ------------------------------------------------------------------------
// exabrick.cu:197-210 boxTest (true division, NaN-ignoring min/max)
// ------------------------------------------------------------------------
__device__ __forceinline__ bool boxTest(const Ray &ray, V3 lo, V3 hi, float &t0, float &t1)
{
  const float lx = (lo.x - ray.org.x) / ray.dir.x, hx = (hi.x - ray.org.x) / ray.dir.x;
  const float ly = (lo.y - ray.org.y) / ray.dir.y, hy = (hi.y - ray.org.y) / ray.dir.y;
  const float lz = (lo.z - ray.org.z) / ray.dir.z, hz = (hi.z - ray.org.z) / ray.dir.z;
  const float nx = fminf(lx, hx), ny = fminf(ly, hy), nz = fminf(lz, hz);
  const float fx = fmaxf(lx, hx), fy = fmaxf(ly, hy), fz = fmaxf(lz, hz);
  t0 = fmaxf(ray.tmin, fmaxf(fmaxf(nx, ny), nz));
  t1 = fminf(ray.tmax, fminf(fminf(fx, fy), fz));
  return t0 < t1;
}

// ------------------------------------------------------------------------
// Closest active region along the ray: the OptiX trace + VolumeBVH/IsoSurface
// intersect program (exabrick.cu:184-238, 346-371) as a software LBVH walk.
// Result = region with the smallest clamped entry t0 (t0 < t1); equal t0 ->
// lowest region id; t1 clamped to the ray's own tmax only.
// ------------------------------------------------------------------------
struct RegionHit { int leafID; float t0, t1; };

template <int STATS>
__device__ __forceinline__ RegionHit traceRegion(Ctx<STATS> &C, const BvhNode *nodes, const Ray &ray)
{
  RegionHit best; best.leafID = -1; best.t0 = INFINITY; best.t1 = 0.f;
  int *stack = C.stack;
  int sp = 0;
  int node = 0;
  for (;;) {
    const float4 *np = reinterpret_cast<const float4 *>(nodes + node);
    const float4 q0 = np[0], q1 = np[1], q2 = np[2];
    const int4 cc = *reinterpret_cast<const int4 *>(np + 3);
    C.count(ST_NODES);
    float a0, a1, b0, b1;
    bool ha = boxTest(ray, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), a0, a1) && (q0.x <= q0.w);
    bool hb = boxTest(ray, mk(q1.z, q1.w, q2.x), mk(q2.y, q2.z, q2.w), b0, b1) && (q1.z <= q2.y);
    if (ha && cc.x < 0) {
      const int id = ~cc.x;
      if (a0 < best.t0 || (a0 == best.t0 && id < best.leafID)) { best.leafID = id; best.t0 = a0; best.t1 = a1; }
      ha = false;
    }
    if (hb && cc.y < 0) {
      const int id = ~cc.y;
      if (b0 < best.t0 || (b0 == best.t0 && id < best.leafID)) { best.leafID = id; best.t0 = b0; best.t1 = b1; }
      hb = false;
    }
    ha = ha && (a0 <= best.t0);
    hb = hb && (b0 <= best.t0);
    if (ha && hb) {
      const bool aFirst = a0 <= b0;
      stack[sp * 256] = aFirst ? cc.y : cc.x;
      sp++;
      node = aFirst ? cc.x : cc.y;
    } else if (ha) {
      node = cc.x;
    } else if (hb) {
      node = cc.y;
    } else {
      if (sp == 0) break;
      sp--;
      node = stack[sp * 256];
    }
  }
  return best;
}

// ------------------------------------------------------------------------
// exabrick.cu:620-777 addBasisFunctions<NEED_DERIVATIVE>: hat-basis of one brick.
// Branch-free: every corner's address is clamped into the brick and the
// accumulation is selected on the reference's in-brick predicate, so the sums
// see exactly the reference's sequence of additions.
// ------------------------------------------------------------------------
struct Basis { float sumWV, sumW; V3 sumD, sumDC; };

template <bool DERIV, int STATS>
__device__ __forceinline__ void addBasisFunctions(Ctx<STATS> &C, Basis &B, const int4 b0, const int4 b1,
                                                  const float *__restrict__ field, V3 pos)
{
  // b0 = (lower.xyz, size.x)  b1 = (size.y, size.z, level, begin)
  const int sx = b0.w, sy = b1.x, sz = b1.y;
  const float invCw = __int_as_float((127 - b1.z) << 23);   // exact 2^-level: (p/cw) == p*invCw
  const float lpx = (pos.x - float(b0.x)) * invCw - 0.5f;
  const float lpy = (pos.y - float(b0.y)) * invCw - 0.5f;
  const float lpz = (pos.z - float(b0.z)) * invCw - 0.5f;
  const int lx = max(-1, int(floorf(lpx))), ly = max(-1, int(floorf(lpy))), lz = max(-1, int(floorf(lpz)));
  const int hx = lx + 1, hy = ly + 1, hz = lz + 1;
  const float fx = lpx - float(lx), fy = lpy - float(ly), fz = lpz - float(lz);
  const float nx = 1.f - fx, ny = 1.f - fy, nz = 1.f - fz;
  const bool vlx = lx >= 0 && lx < sx, vhx = hx < sx;
  const bool vly = ly >= 0 && ly < sy, vhy = hy < sy;
  const bool vlz = lz >= 0 && lz < sz, vhz = hz < sz;
  // clamped (always in-brick) cell coordinates for the speculative loads
  const int cxl = min(max(lx, 0), sx - 1), cxh = min(hx, sx - 1);
  const int cyl = min(max(ly, 0), sy - 1), cyh = min(hy, sy - 1);
  const int czl = min(max(lz, 0), sz - 1), czh = min(hz, sz - 1);
  const uint32_t base = (uint32_t)b1.w;
  const uint32_t rowLL = base + (uint32_t)(cyl * sx + czl * sx * sy);
  const uint32_t rowHL = base + (uint32_t)(cyh * sx + czl * sx * sy);
  const uint32_t rowLH = base + (uint32_t)(cyl * sx + czh * sx * sy);
  const uint32_t rowHH = base + (uint32_t)(cyh * sx + czh * sx * sy);
  const float s000 = field[rowLL + cxl], s100 = field[rowLL + cxh];
  const float s010 = field[rowHL + cxl], s110 = field[rowHL + cxh];
  const float s001 = field[rowLH + cxl], s101 = field[rowLH + cxh];
  const float s011 = field[rowHH + cxl], s111 = field[rowHH + cxh];
  C.count(ST_BRICK_VISITS);
#define EXA_CORNER(VALID, S, WZ, WY, WX, SGX, SGY, SGZ)                                     \
  {                                                                                          \
    /* EXA_EMPTY_CELLS: notEmptyCell(scalar), exabrick.cu:614-618, 646 ...; the cell is read (and counted) either way */ \
    const bool v_ = (VALID) && (!EXA_EMPTY_CELLS || (S) != EXA_EMPTY_CELL_POISON_VALUE);     \
    if (STATS == 1 && (VALID)) C.st[ST_CORNER_LOADS]++;                                      \
    const float w_ = (WZ) * (WY) * (WX);                                                     \
    if (DERIV) {                                                                             \
      const float dx_ = (WZ) * (WY) * (SGX 1.f);                                             \
      const float dy_ = (WZ) * (WX) * (SGY 1.f);                                             \
      const float dz_ = (WY) * (WX) * (SGZ 1.f);                                             \
      B.sumDC.x = v_ ? B.sumDC.x + dx_ : B.sumDC.x;                                          \
      B.sumDC.y = v_ ? B.sumDC.y + dy_ : B.sumDC.y;                                          \
      B.sumDC.z = v_ ? B.sumDC.z + dz_ : B.sumDC.z;                                          \
      B.sumD.x = v_ ? B.sumD.x + dx_ * (S) : B.sumD.x;                                       \
      B.sumD.y = v_ ? B.sumD.y + dy_ * (S) : B.sumD.y;                                       \
      B.sumD.z = v_ ? B.sumD.z + dz_ * (S) : B.sumD.z;                                       \
    }                                                                                        \
    B.sumW = v_ ? B.sumW + w_ : B.sumW;                                                      \
    B.sumWV = v_ ? B.sumWV + w_ * (S) : B.sumWV;                                             \
  }
  // corner order of the reference: z-lo{y-lo{x-lo,x-hi}, y-hi{..}}, z-hi{..}
  EXA_CORNER(vlz && vly && vlx, s000, nz, ny, nx, -, -, -)   // :644-658
  EXA_CORNER(vlz && vly && vhx, s100, nz, ny, fx, +, -, -)   // :659-673
  EXA_CORNER(vlz && vhy && vlx, s010, nz, fy, nx, -, +, -)   // :676-691
  EXA_CORNER(vlz && vhy && vhx, s110, nz, fy, fx, +, +, -)   // :692-706
  EXA_CORNER(vhz && vly && vlx, s001, fz, ny, nx, -, -, +)   // :712-726
  EXA_CORNER(vhz && vly && vhx, s101, fz, ny, fx, +, -, +)   // :727-741
  EXA_CORNER(vhz && vhy && vlx, s011, fz, fy, nx, -, +, +)   // :744-758
  EXA_CORNER(vhz && vhy && vhx, s111, fz, fy, fx, +, +, +)   // :759-774
#undef EXA_CORNER
}

struct __attribute__((packed, aligned(4))) Pair { float a, b; };
__device__ __forceinline__ Pair loadPair(const float *__restrict__ p) { return *reinterpret_cast<const Pair *>(p); }

// Same sums as addBasisFunctions with fewer instructions: validity is a product of
// per-axis predicates, so the per-axis weights are masked to 0 once (6 selects) instead of
// selecting every accumulator at every corner.  A skipped corner then adds +-0, which
// leaves a sum unchanged (the sums start at +0 and can never become -0), so the
// accumulators see bit-identical values.  The speculative read of an out-of-brick corner
// is clamped onto a cell that an in-brick corner of the same sample reads as well.
//
// VOXEL (the point probes' EXA_SAMPLE_GRADIENT_NORMALIZED only): the derivative weight of a corner is -+2^-level times the
// other two axes' weights, the derivative with respect to the VOXEL-space position, where the reference (and every
// other caller) takes -+1, the derivative with respect to the brick's own cell coordinate (INV_CELL_WIDTH == 1.f,
// exabrick.cu:640-641).  2^-level is a power of two: every product with it is exact, so a brick's terms are the
// reference's times 2^-level bit for bit.  sumW and sumWV do not depend on it.
//
// CUBE (the cube instantiations of the one-channel rope march only, SMALL): every brick of the scene is a cube of edge
// 2^cubeLog2, a wave-uniform kernel argument, and b0 is the brick's cube record (exa_cube.h; b1 is not looked at): the sizes
// are scalar operands of the compares and clamps, the row offsets shifts instead of multiplies, 2^-level is b0.w << 23.  The
// same integers and floats enter every address and every float operation as from the brick's march header.
//
// Two phases around `between`: position, clamps, row offsets and the issue of the four pair loads in front of it; the pick
// out of the pairs, the masked weights and the sums behind it.  A caller puts there what can run while the loads are on their
// way and may change B (the cube march: the previous sample's epilogue); when it returns false the visit is abandoned with
// its loads in flight and B as `between` left it.  The default does nothing and leaves no trace in the code.
struct NothingBetween { __device__ __forceinline__ bool operator()() const { return true; } };
template <bool DERIV, int STATS, bool SMALL, bool VOXEL = false, bool CUBE = false, class Between = NothingBetween>
__device__ __forceinline__ void addBasisFast(Ctx<STATS> &C, Basis &B, const int4 b0, const int4 b1,
                                             const float *__restrict__ field, V3 pos, const int cubeLog2 = 0, Between between = Between())
{
  static_assert(!CUBE || SMALL, "cube records: the 32-bit address form only");
  // march header (exa_module: leafHdr): b0 = (float(lower.xyz), 2^-level) as float bits, b1 = (size.xyz, begin)
  // cube record: b0 = (float(lower.xyz), ((begin >> 3k) << 9) | (127 - level))
  const int sx = CUBE ? (1 << cubeLog2) : b1.x, sy = CUBE ? sx : b1.y, sz = CUBE ? sx : b1.z;
  const uint32_t begin = CUBE ? ((uint32_t)b0.w >> 9) << (3 * cubeLog2) : (uint32_t)b1.w;
  const float invCw = __int_as_float(CUBE ? (int)((uint32_t)b0.w << 23) : b0.w);   // exact 2^-level: (p/cw) == p*invCw
  const float lpx = EXA_F1 ? __builtin_fmaf(pos.x - __int_as_float(b0.x), invCw, -0.5f) : (pos.x - __int_as_float(b0.x)) * invCw - 0.5f;
  const float lpy = EXA_F1 ? __builtin_fmaf(pos.y - __int_as_float(b0.y), invCw, -0.5f) : (pos.y - __int_as_float(b0.y)) * invCw - 0.5f;
  const float lpz = EXA_F1 ? __builtin_fmaf(pos.z - __int_as_float(b0.z), invCw, -0.5f) : (pos.z - __int_as_float(b0.z)) * invCw - 0.5f;
  // idx_lo = max(-1, int(floor(local))) (exabrick.cu:627-629); the clamp on the float is the same value (floor is
  // integral, -1 exact) and saves converting the clamped index back for the fraction
  const float flx = fmaxf(floorf(lpx), -1.f), fly = fmaxf(floorf(lpy), -1.f), flz = fmaxf(floorf(lpz), -1.f);
  const int lx = int(flx), ly = int(fly), lz = int(flz);
  const int hx = lx + 1, hy = ly + 1, hz = lz + 1;
  const float fx = lpx - flx, fy = lpy - fly, fz = lpz - flz;
  // 0 <= l < size as one unsigned compare (l >= -1, sizes > 0)
  const bool vlx = (uint32_t)lx < (uint32_t)sx, vhx = hx < sx;
  const bool vly = (uint32_t)ly < (uint32_t)sy, vhy = hy < sy;
  const bool vlz = (uint32_t)lz < (uint32_t)sz, vhz = hz < sz;
  // clamp(l, 0, size-1) as one v_med3_i32 (sizes >= 1, so 0 <= size-1 and the median IS the clamp); the compiler
  // cannot prove the bound order and emits v_max + v_min (the 0 is the instruction's inline constant: as a "v" operand
  // it occupied a register across the whole march)
  // (CUBE: the bound is wave-uniform, a scalar operand; the edge is >= 2, so size-2 needs no max)
  auto med3 = [](int a, int c) {                                                                                     // clamp(a, 0, c)
    int r;
    if (CUBE) asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(a), "s"(c));
    else asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(a), "v"(c));
    return r;
  };
  const int cxl = med3(lx, sx - 1), cxh = min(hx, sx - 1);
  const int cyl = med3(ly, sy - 1), cyh = min(hy, sy - 1);
  const int czl = med3(lz, sz - 1), czh = min(hz, sz - 1);
  const int bx = med3(lx, CUBE ? sx - 2 : max(sx - 2, 0));
  float s000, s100, s010, s110, s001, s101, s011, s111;
  {
    // (eight 4-byte loads instead of four 8-byte pair loads would save the pair base, two compares and eight
    // selects, ~10 VALU per visit — measured on C4: 26.1 instead of 22.5 ms, the L1 request rate matters too)
    uint32_t rowLL, rowHL, rowLH, rowHH;                      // cell index of the pair's first cell, per (y,z) row
    if (CUBE) {
      // x + (y << k) + (z << 2k) + begin: six v_lshl_add_u32 with scalar shifts and one add, no multiply
      const uint32_t at = begin + (uint32_t)bx;
      const uint32_t zl = ((uint32_t)czl << (2 * cubeLog2)) + at, zh = ((uint32_t)czh << (2 * cubeLog2)) + at;
      rowLL = ((uint32_t)cyl << cubeLog2) + zl; rowHL = ((uint32_t)cyh << cubeLog2) + zl;
      rowLH = ((uint32_t)cyl << cubeLog2) + zh; rowHH = ((uint32_t)cyh << cubeLog2) + zh;
    } else if (SMALL) {
      // SMALL: every factor below 2^24 and every product below 2^32 (checked per scene on the host)
      // (the compiler turns this one __umul24 into the quarter-rate v_mul_lo_u32; forcing v_mul_u32_u24 with inline asm
      // measured 22.25 against 22.19 ms — the asm pins the schedule — so it stays)
      const uint32_t sxy = __umul24((uint32_t)sx, (uint32_t)sy);
      const uint32_t zl = __umul24((uint32_t)czl, sxy) + (begin + (uint32_t)bx);
      const uint32_t zh = __umul24((uint32_t)czh, sxy) + (begin + (uint32_t)bx);
      const uint32_t yl = __umul24((uint32_t)cyl, (uint32_t)sx), yh = __umul24((uint32_t)cyh, (uint32_t)sx);
      rowLL = zl + yl; rowHL = zl + yh; rowLH = zh + yl; rowHH = zh + yh;
    } else {
      const uint32_t sxy = (uint32_t)(sx * sy);
      const uint32_t zl = begin + (uint32_t)czl * sxy + (uint32_t)bx, zh = begin + (uint32_t)czh * sxy + (uint32_t)bx;
      const uint32_t yl = (uint32_t)(cyl * sx), yh = (uint32_t)(cyh * sx);
      rowLL = zl + yl; rowHL = zl + yh; rowLH = zh + yl; rowHH = zh + yh;
    }
    // the two x-neighbours of a row are adjacent in memory: one 8-byte load per row (4-byte
    // aligned), then pick the clamped low/high cell out of the pair
    const bool lFirst = cxl == bx, hFirst = cxh == bx;
    Pair pLL, pHL, pLH, pHH;
    if (SMALL) {
      // SMALL: a field is below 4 GiB: wave-uniform base + 32-bit byte offset per lane (no 64-bit address arithmetic)
      const char *base = reinterpret_cast<const char *>(field);
      pLL = *reinterpret_cast<const Pair *>(base + (rowLL << 2)); pHL = *reinterpret_cast<const Pair *>(base + (rowHL << 2));
      pLH = *reinterpret_cast<const Pair *>(base + (rowLH << 2)); pHH = *reinterpret_cast<const Pair *>(base + (rowHH << 2));
    } else {
      pLL = loadPair(field + rowLL); pHL = loadPair(field + rowHL);
      pLH = loadPair(field + rowLH); pHH = loadPair(field + rowHH);
    }
    if constexpr (!std::is_same<Between, NothingBetween>::value) { if (!between()) return; }
    s000 = lFirst ? pLL.a : pLL.b; s100 = hFirst ? pLL.a : pLL.b;
    s010 = lFirst ? pHL.a : pHL.b; s110 = hFirst ? pHL.a : pHL.b;
    s001 = lFirst ? pLH.a : pLH.b; s101 = hFirst ? pLH.a : pLH.b;
    s011 = lFirst ? pHH.a : pHH.b; s111 = hFirst ? pHH.a : pHH.b;
  }
  C.count(ST_BRICK_VISITS);
  if (STATS == 1) {
    // A NaN position — an iso crossing between two samples that both EQUAL the iso value has 0/0 weights
    // (exabrick.cu:1047-1053) — converts to cell 0 in the reference (float -> int of NaN is 0; cells 0 and 1 are read),
    // where the clamp on the float gives -1 (cell 0 only).  Every sum is NaN either way; the count follows the reference.
    const int nx = lpx != lpx ? (1 + int(1 < sx)) : (int(vlx) + int(vhx));
    const int ny = lpy != lpy ? (1 + int(1 < sy)) : (int(vly) + int(vhy));
    const int nz = lpz != lpz ? (1 + int(1 < sz)) : (int(vlz) + int(vhz));
    C.st[ST_CORNER_LOADS] += (unsigned)(nx * ny * nz);
  }
  // masked per-axis weights: (1-frac) for the low cell, frac for the high cell
  const float wxl = vlx ? 1.f - fx : 0.f, wxh = vhx ? fx : 0.f;
  const float wyl = vly ? 1.f - fy : 0.f, wyh = vhy ? fy : 0.f;
  const float wzl = vlz ? 1.f - fz : 0.f, wzh = vhz ? fz : 0.f;
#if EXA_BASIS_FORM == 1
  // The same sums associated per axis (oracle: add_basis_functions_factored, operation for operation): the weight of
  // a corner is a product of per-axis weights and "inside the brick" a product of per-axis predicates, so the triple
  // sum over the corners factors into x-pairs -> y -> z.  Every fmaf is one v_fma_f32; nothing else is fused.
  {
    const float aLL = __builtin_fmaf(wxh, s100, wxl * s000), aLH = __builtin_fmaf(wxh, s110, wxl * s010);   // [z][y]
    const float aHL = __builtin_fmaf(wxh, s101, wxl * s001), aHH = __builtin_fmaf(wxh, s111, wxl * s011);
    const float Al = __builtin_fmaf(wyh, aLH, wyl * aLL), Ah = __builtin_fmaf(wyh, aHH, wyl * aHL);
    B.sumWV = __builtin_fmaf(wzh, Ah, __builtin_fmaf(wzl, Al, B.sumWV));
    const float Sx = wxl + wxh, Sy = wyl + wyh, Sz = wzl + wzh;
    const float zy = Sz * Sy;
    B.sumW = __builtin_fmaf(zy, Sx, B.sumW);
    if (DERIV) {
      // d w / d x of a corner = -1 (low cell) or +1 (high cell) times the other two axes' weights, 0 outside the brick
      const float dw = VOXEL ? invCw : 1.f;
      const float mxl = vlx ? -dw : 0.f, mxh = vhx ? dw : 0.f;
      const float myl = vly ? -dw : 0.f, myh = vhy ? dw : 0.f;
      const float mzl = vlz ? -dw : 0.f, mzh = vhz ? dw : 0.f;
      const float dLL = __builtin_fmaf(mxh, s100, mxl * s000), dLH = __builtin_fmaf(mxh, s110, mxl * s010);
      const float dHL = __builtin_fmaf(mxh, s101, mxl * s001), dHH = __builtin_fmaf(mxh, s111, mxl * s011);
      const float DXl = __builtin_fmaf(wyh, dLH, wyl * dLL), DXh = __builtin_fmaf(wyh, dHH, wyl * dHL);
      const float DYl = __builtin_fmaf(myh, aLH, myl * aLL), DYh = __builtin_fmaf(myh, aHH, myl * aHL);
      B.sumD.x = __builtin_fmaf(wzh, DXh, __builtin_fmaf(wzl, DXl, B.sumD.x));
      B.sumD.y = __builtin_fmaf(wzh, DYh, __builtin_fmaf(wzl, DYl, B.sumD.y));
      B.sumD.z = __builtin_fmaf(mzh, Ah, __builtin_fmaf(mzl, Al, B.sumD.z));
      const float Mx = mxl + mxh, My = myl + myh, Mz = mzl + mzh;
      B.sumDC.x = __builtin_fmaf(zy, Mx, B.sumDC.x);
      B.sumDC.y = __builtin_fmaf(Sz * Sx, My, B.sumDC.y);
      B.sumDC.z = __builtin_fmaf(Sy * Sx, Mz, B.sumDC.z);
    }
  }
#else
  // (z*y) first, then *x: the reference's association (exabrick.cu:647 etc.)
  const float zyLL = wzl * wyl, zyLH = wzl * wyh, zyHL = wzh * wyl, zyHH = wzh * wyh;
  if (DERIV) {
    // d/dx weight = +-(z*y), d/dy = +-(z*x), d/dz = +-(y*x), zero for an out-of-brick corner
    const float dw = VOXEL ? invCw : 1.f;
    const float mxl = vlx ? -dw : 0.f, mxh = vhx ? dw : 0.f;
    const float myl = vly ? -dw : 0.f, myh = vhy ? dw : 0.f;
    const float mzl = vlz ? -dw : 0.f, mzh = vhz ? dw : 0.f;
    const float zxLL = wzl * wxl, zxLH = wzl * wxh, zxHL = wzh * wxl, zxHH = wzh * wxh;   // [z][x]
    const float yxLL = wyl * wxl, yxLH = wyl * wxh, yxHL = wyh * wxl, yxHH = wyh * wxh;   // [y][x]
    // The derivative weight of a corner is +-(product of the other two axes' weights) or 0: dx_ = zy * mx with
    // mx in {-1, 0, +1}, an EXACT product.  So `sum += dx_` is one fused multiply-add with the same result bit for
    // bit (an fma rounds once, and there is nothing to round in zy * mx), and `sum += dx_ * s` equals
    // fma(zy * s, mx, sum): (+-zy) * s rounds to +-(zy * s), and for mx = 0 both forms add a zero of the sign of s.
    // 13 instructions per corner instead of 16.
    // EXA_EMPTY_CELLS: a corner whose cell holds the poison value is skipped (notEmptyCell, exabrick.cu:614-618): its three
    // pair weights are zeroed, so every term it adds is a zero (the poison value is finite)
#define EXA_ACC(S, ZY0, WX, MX, ZX0, MY, YX0, MZ)                                            \
    {                                                                                        \
      const bool ne_ = !EXA_EMPTY_CELLS || (S) != EXA_EMPTY_CELL_POISON_VALUE;               \
      const float ZY = ne_ ? (ZY0) : 0.f, ZX = ne_ ? (ZX0) : 0.f, YX = ne_ ? (YX0) : 0.f;    \
      B.sumDC.x = __builtin_fmaf((ZY), (MX), B.sumDC.x);                                     \
      B.sumDC.y = __builtin_fmaf((ZX), (MY), B.sumDC.y);                                     \
      B.sumDC.z = __builtin_fmaf((YX), (MZ), B.sumDC.z);                                     \
      B.sumD.x = __builtin_fmaf((ZY) * (S), (MX), B.sumD.x);                                 \
      B.sumD.y = __builtin_fmaf((ZX) * (S), (MY), B.sumD.y);                                 \
      B.sumD.z = __builtin_fmaf((YX) * (S), (MZ), B.sumD.z);                                 \
      const float w_ = (ZY) * (WX);                                                          \
      B.sumW += w_; B.sumWV += w_ * (S);                                                     \
    }
    EXA_ACC(s000, zyLL, wxl, mxl, zxLL, myl, yxLL, mzl)
    EXA_ACC(s100, zyLL, wxh, mxh, zxLH, myl, yxLH, mzl)
    EXA_ACC(s010, zyLH, wxl, mxl, zxLL, myh, yxHL, mzl)
    EXA_ACC(s110, zyLH, wxh, mxh, zxLH, myh, yxHH, mzl)
    EXA_ACC(s001, zyHL, wxl, mxl, zxHL, myl, yxLL, mzh)
    EXA_ACC(s101, zyHL, wxh, mxh, zxHH, myl, yxLH, mzh)
    EXA_ACC(s011, zyHH, wxl, mxl, zxHL, myh, yxHL, mzh)
    EXA_ACC(s111, zyHH, wxh, mxh, zxHH, myh, yxHH, mzh)
#undef EXA_ACC
  } else {
#define EXA_ACC(S, ZY, WX) { const float w_ = (!EXA_EMPTY_CELLS || (S) != EXA_EMPTY_CELL_POISON_VALUE) ? (ZY) * (WX) : 0.f; B.sumW += w_; B.sumWV += w_ * (S); }
    EXA_ACC(s000, zyLL, wxl) EXA_ACC(s100, zyLL, wxh) EXA_ACC(s010, zyLH, wxl) EXA_ACC(s110, zyLH, wxh)
    EXA_ACC(s001, zyHL, wxl) EXA_ACC(s101, zyHL, wxh) EXA_ACC(s011, zyHH, wxl) EXA_ACC(s111, zyHH, wxh)
#undef EXA_ACC
  }
#endif
}

// Channel-interleaved form of addBasisFast for the multi-channel DVR march: the NCH primary channels of a cell lie side
// by side (float[cell][NCH], built by the module from the field-major arrays of the ABI), so the two x-neighbours of a row
// are 2*NCH adjacent floats — one load per row for ALL channels where the field-major layout takes one per row and
// channel, from arrays gigabytes apart.  The cell indices, the six masked weights and the sums that do not depend on the
// cell values (sumW, sumDC) are the same for every channel (same position, same brick) and are evaluated once; per
// channel only sumWV / sumD remain (8 instead of 13 instructions per corner, none of the ~90 of the index arithmetic).
// Each channel's sums see exactly the additions, in exactly the order, of addBasisFast on that channel's field: the
// reference's per-channel samplePoint calls (exabrick.cu:1163-1178) are independent of each other, so evaluating them
// side by side changes no value.  xWV / xD: the sums of channels 1..NCH-1 (channel 0 lives in B).
template <int NCH> struct __attribute__((packed, aligned(4))) PairN { float v[2 * NCH]; };

template <bool DERIV, bool SMALL, int NCH>
__device__ __forceinline__ void addBasisFastIl(Basis &B, float *xWV, V3 *xD, const int4 b0, const int4 b1,
                                               const float *__restrict__ cellsIl, V3 pos)
{
  const int sx = b1.x, sy = b1.y, sz = b1.z;
  const uint32_t begin = (uint32_t)b1.w;
  const float invCw = __int_as_float(b0.w);
  const float lpx = EXA_F1 ? __builtin_fmaf(pos.x - __int_as_float(b0.x), invCw, -0.5f) : (pos.x - __int_as_float(b0.x)) * invCw - 0.5f;
  const float lpy = EXA_F1 ? __builtin_fmaf(pos.y - __int_as_float(b0.y), invCw, -0.5f) : (pos.y - __int_as_float(b0.y)) * invCw - 0.5f;
  const float lpz = EXA_F1 ? __builtin_fmaf(pos.z - __int_as_float(b0.z), invCw, -0.5f) : (pos.z - __int_as_float(b0.z)) * invCw - 0.5f;
  const float flx = fmaxf(floorf(lpx), -1.f), fly = fmaxf(floorf(lpy), -1.f), flz = fmaxf(floorf(lpz), -1.f);
  const int lx = int(flx), ly = int(fly), lz = int(flz);
  const int hx = lx + 1, hy = ly + 1, hz = lz + 1;
  const float fx = lpx - flx, fy = lpy - fly, fz = lpz - flz;
  const bool vlx = (uint32_t)lx < (uint32_t)sx, vhx = hx < sx;
  const bool vly = (uint32_t)ly < (uint32_t)sy, vhy = hy < sy;
  const bool vlz = (uint32_t)lz < (uint32_t)sz, vhz = hz < sz;
  auto med3 = [](int a, int c) { int r; asm("v_med3_i32 %0, %1, 0, %2" : "=v"(r) : "v"(a), "v"(c)); return r; };   // clamp(a, 0, c)
  const int cxl = med3(lx, sx - 1), cxh = min(hx, sx - 1);
  const int cyl = med3(ly, sy - 1), cyh = min(hy, sy - 1);
  const int czl = med3(lz, sz - 1), czh = min(hz, sz - 1);
  const int bx = med3(lx, max(sx - 2, 0));
  uint32_t rowLL, rowHL, rowLH, rowHH;                      // cell index of the pair's first cell, per (y,z) row
  if (SMALL) {
    const uint32_t sxy = __umul24((uint32_t)sx, (uint32_t)sy);
    const uint32_t zl = __umul24((uint32_t)czl, sxy) + (begin + (uint32_t)bx);
    const uint32_t zh = __umul24((uint32_t)czh, sxy) + (begin + (uint32_t)bx);
    const uint32_t yl = __umul24((uint32_t)cyl, (uint32_t)sx), yh = __umul24((uint32_t)cyh, (uint32_t)sx);
    rowLL = zl + yl; rowHL = zl + yh; rowLH = zh + yl; rowHH = zh + yh;
  } else {
    const uint32_t sxy = (uint32_t)(sx * sy);
    const uint32_t zl = begin + (uint32_t)czl * sxy + (uint32_t)bx, zh = begin + (uint32_t)czh * sxy + (uint32_t)bx;
    const uint32_t yl = (uint32_t)(cyl * sx), yh = (uint32_t)(cyh * sx);
    rowLL = zl + yl; rowHL = zl + yh; rowLH = zh + yl; rowHH = zh + yh;
  }
  const bool lFirst = cxl == bx, hFirst = cxh == bx;
  PairN<NCH> pLL, pHL, pLH, pHH;
  if (SMALL) {
    // SMALL: the interleaved array is below 4 GiB: wave-uniform base + 32-bit byte offset per lane
    const char *base = reinterpret_cast<const char *>(cellsIl);
    pLL = *reinterpret_cast<const PairN<NCH> *>(base + rowLL * (uint32_t)(4 * NCH)); pHL = *reinterpret_cast<const PairN<NCH> *>(base + rowHL * (uint32_t)(4 * NCH));
    pLH = *reinterpret_cast<const PairN<NCH> *>(base + rowLH * (uint32_t)(4 * NCH)); pHH = *reinterpret_cast<const PairN<NCH> *>(base + rowHH * (uint32_t)(4 * NCH));
  } else {
    pLL = *reinterpret_cast<const PairN<NCH> *>(cellsIl + size_t(rowLL) * NCH); pHL = *reinterpret_cast<const PairN<NCH> *>(cellsIl + size_t(rowHL) * NCH);
    pLH = *reinterpret_cast<const PairN<NCH> *>(cellsIl + size_t(rowLH) * NCH); pHH = *reinterpret_cast<const PairN<NCH> *>(cellsIl + size_t(rowHH) * NCH);
  }
  const float wxl = vlx ? 1.f - fx : 0.f, wxh = vhx ? fx : 0.f;
  const float wyl = vly ? 1.f - fy : 0.f, wyh = vhy ? fy : 0.f;
  const float wzl = vlz ? 1.f - fz : 0.f, wzh = vhz ? fz : 0.f;
#if EXA_BASIS_FORM == 1
  // per-axis association (see addBasisFast): the sums that do not depend on the cell values once, the value trees per channel
  const float Sx = wxl + wxh, Sy = wyl + wyh, Sz = wzl + wzh;
  const float zy = Sz * Sy;
  B.sumW = __builtin_fmaf(zy, Sx, B.sumW);
  float mxl = 0.f, mxh = 0.f, myl = 0.f, myh = 0.f, mzl = 0.f, mzh = 0.f;
  if (DERIV) {
    mxl = vlx ? -1.f : 0.f; mxh = vhx ? 1.f : 0.f;
    myl = vly ? -1.f : 0.f; myh = vhy ? 1.f : 0.f;
    mzl = vlz ? -1.f : 0.f; mzh = vhz ? 1.f : 0.f;
    const float Mx = mxl + mxh, My = myl + myh, Mz = mzl + mzh;
    B.sumDC.x = __builtin_fmaf(zy, Mx, B.sumDC.x);
    B.sumDC.y = __builtin_fmaf(Sz * Sx, My, B.sumDC.y);
    B.sumDC.z = __builtin_fmaf(Sy * Sx, Mz, B.sumDC.z);
  }
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    float &sumWV = c == 0 ? B.sumWV : xWV[c == 0 ? 0 : c - 1];
    V3 &sumD = c == 0 ? B.sumD : xD[c == 0 ? 0 : c - 1];
    const float s000 = lFirst ? pLL.v[c] : pLL.v[NCH + c], s100 = hFirst ? pLL.v[c] : pLL.v[NCH + c];
    const float s010 = lFirst ? pHL.v[c] : pHL.v[NCH + c], s110 = hFirst ? pHL.v[c] : pHL.v[NCH + c];
    const float s001 = lFirst ? pLH.v[c] : pLH.v[NCH + c], s101 = hFirst ? pLH.v[c] : pLH.v[NCH + c];
    const float s011 = lFirst ? pHH.v[c] : pHH.v[NCH + c], s111 = hFirst ? pHH.v[c] : pHH.v[NCH + c];
    const float aLL = __builtin_fmaf(wxh, s100, wxl * s000), aLH = __builtin_fmaf(wxh, s110, wxl * s010);   // [z][y]
    const float aHL = __builtin_fmaf(wxh, s101, wxl * s001), aHH = __builtin_fmaf(wxh, s111, wxl * s011);
    const float Al = __builtin_fmaf(wyh, aLH, wyl * aLL), Ah = __builtin_fmaf(wyh, aHH, wyl * aHL);
    sumWV = __builtin_fmaf(wzh, Ah, __builtin_fmaf(wzl, Al, sumWV));
    if (DERIV) {
      const float dLL = __builtin_fmaf(mxh, s100, mxl * s000), dLH = __builtin_fmaf(mxh, s110, mxl * s010);
      const float dHL = __builtin_fmaf(mxh, s101, mxl * s001), dHH = __builtin_fmaf(mxh, s111, mxl * s011);
      const float DXl = __builtin_fmaf(wyh, dLH, wyl * dLL), DXh = __builtin_fmaf(wyh, dHH, wyl * dHL);
      const float DYl = __builtin_fmaf(myh, aLH, myl * aLL), DYh = __builtin_fmaf(myh, aHH, myl * aHL);
      sumD.x = __builtin_fmaf(wzh, DXh, __builtin_fmaf(wzl, DXl, sumD.x));
      sumD.y = __builtin_fmaf(wzh, DYh, __builtin_fmaf(wzl, DYl, sumD.y));
      sumD.z = __builtin_fmaf(mzh, Ah, __builtin_fmaf(mzl, Al, sumD.z));
    }
  }
#else
  const float zyLL = wzl * wyl, zyLH = wzl * wyh, zyHL = wzh * wyl, zyHH = wzh * wyh;
  // the eight trilinear weights, in the reference's association (z*y)*x
  const float w000 = zyLL * wxl, w100 = zyLL * wxh, w010 = zyLH * wxl, w110 = zyLH * wxh;
  const float w001 = zyHL * wxl, w101 = zyHL * wxh, w011 = zyHH * wxl, w111 = zyHH * wxh;
  B.sumW += w000; B.sumW += w100; B.sumW += w010; B.sumW += w110;
  B.sumW += w001; B.sumW += w101; B.sumW += w011; B.sumW += w111;
  float mxl = 0.f, mxh = 0.f, myl = 0.f, myh = 0.f, mzl = 0.f, mzh = 0.f;
  float zxLL = 0.f, zxLH = 0.f, zxHL = 0.f, zxHH = 0.f, yxLL = 0.f, yxLH = 0.f, yxHL = 0.f, yxHH = 0.f;
  if (DERIV) {
    mxl = vlx ? -1.f : 0.f; mxh = vhx ? 1.f : 0.f;
    myl = vly ? -1.f : 0.f; myh = vhy ? 1.f : 0.f;
    mzl = vlz ? -1.f : 0.f; mzh = vhz ? 1.f : 0.f;
    zxLL = wzl * wxl; zxLH = wzl * wxh; zxHL = wzh * wxl; zxHH = wzh * wxh;   // [z][x]
    yxLL = wyl * wxl; yxLH = wyl * wxh; yxHL = wyh * wxl; yxHH = wyh * wxh;   // [y][x]
    // sumDC += (+-)(product of the other two axes' weights): exact-product fma, as in addBasisFast
#define EXA_DC(ZY, MX, ZX, MY, YX, MZ)                                                       \
    B.sumDC.x = __builtin_fmaf((ZY), (MX), B.sumDC.x);                                       \
    B.sumDC.y = __builtin_fmaf((ZX), (MY), B.sumDC.y);                                       \
    B.sumDC.z = __builtin_fmaf((YX), (MZ), B.sumDC.z);
    EXA_DC(zyLL, mxl, zxLL, myl, yxLL, mzl) EXA_DC(zyLL, mxh, zxLH, myl, yxLH, mzl)
    EXA_DC(zyLH, mxl, zxLL, myh, yxHL, mzl) EXA_DC(zyLH, mxh, zxLH, myh, yxHH, mzl)
    EXA_DC(zyHL, mxl, zxHL, myl, yxLL, mzh) EXA_DC(zyHL, mxh, zxHH, myl, yxLH, mzh)
    EXA_DC(zyHH, mxl, zxHL, myh, yxHL, mzh) EXA_DC(zyHH, mxh, zxHH, myh, yxHH, mzh)
#undef EXA_DC
  }
#pragma unroll
  for (int c = 0; c < NCH; c++) {
    float &sumWV = c == 0 ? B.sumWV : xWV[c == 0 ? 0 : c - 1];
    V3 &sumD = c == 0 ? B.sumD : xD[c == 0 ? 0 : c - 1];
    const float s000 = lFirst ? pLL.v[c] : pLL.v[NCH + c], s100 = hFirst ? pLL.v[c] : pLL.v[NCH + c];
    const float s010 = lFirst ? pHL.v[c] : pHL.v[NCH + c], s110 = hFirst ? pHL.v[c] : pHL.v[NCH + c];
    const float s001 = lFirst ? pLH.v[c] : pLH.v[NCH + c], s101 = hFirst ? pLH.v[c] : pLH.v[NCH + c];
    const float s011 = lFirst ? pHH.v[c] : pHH.v[NCH + c], s111 = hFirst ? pHH.v[c] : pHH.v[NCH + c];
#define EXA_ACC(S, W, ZY, MX, ZX, MY, YX, MZ)                                                \
    {                                                                                        \
      if (DERIV) {                                                                           \
        sumD.x = __builtin_fmaf((ZY) * (S), (MX), sumD.x);                                   \
        sumD.y = __builtin_fmaf((ZX) * (S), (MY), sumD.y);                                   \
        sumD.z = __builtin_fmaf((YX) * (S), (MZ), sumD.z);                                   \
      }                                                                                      \
      sumWV += (W) * (S);                                                                    \
    }
    EXA_ACC(s000, w000, zyLL, mxl, zxLL, myl, yxLL, mzl)
    EXA_ACC(s100, w100, zyLL, mxh, zxLH, myl, yxLH, mzl)
    EXA_ACC(s010, w010, zyLH, mxl, zxLL, myh, yxHL, mzl)
    EXA_ACC(s110, w110, zyLH, mxh, zxLH, myh, yxHH, mzl)
    EXA_ACC(s001, w001, zyHL, mxl, zxHL, myl, yxLL, mzh)
    EXA_ACC(s101, w101, zyHL, mxh, zxHH, myl, yxLH, mzh)
    EXA_ACC(s011, w011, zyHH, mxl, zxHL, myh, yxHL, mzh)
    EXA_ACC(s111, w111, zyHH, mxh, zxHH, myh, yxHH, mzh)
#undef EXA_ACC
  }
#endif
}

// exabrick.cu:781-806 samplePoint / :883-928 samplePointWithDerivative
template <bool DERIV, int STATS>
__device__ __forceinline__ bool samplePoint(Ctx<STATS> &C, float &value, V3 &derivatives,
                                            const RegionInfo &ri, V3 pos, int channel)
{
  const DeviceScene &sc = C.a->sc;
  const float *field = sc.scalars + sc.channelOffset[channel];
  Basis B;
  B.sumWV = 0.f; B.sumW = 0.f; B.sumD = mk(0.f, 0.f, 0.f); B.sumDC = mk(0.f, 0.f, 0.f);
  if (C.fastSampler) {
    // the kd kernels' surfaces pre-pass: march headers along the leaf list and the masked-weight basis evaluation of
    // the DVR march (bit-identical sums, ~40 % fewer instructions per brick, no brick-id indirection)
    for (int child = 0; child < ri.listSize; child++) {
      const unsigned at = 2u * (unsigned)(ri.listBegin + child);
      const int4 h0 = sc.leafHdr[at], h1 = sc.leafHdr[at + 1u];
      addBasisFast<DERIV, STATS, false>(C, B, h0, h1, field, pos);
    }
  } else {
    // the LBVH kernel keeps the literal form of addBasisFunctions: an independent evaluation of the same sums, which
    // the tests compare with the kd kernels bit for bit
    int brickID = ri.firstBrick;
    for (int child = 0;;) {
      const int4 b0 = sc.bricks[2 * brickID], b1 = sc.bricks[2 * brickID + 1];
#if EXA_BASIS_FORM == 1
      // the per-axis association has one implementation: the brick record is turned into a march header on the fly
      const int4 h0 = make_int4(__float_as_int(float(b0.x)), __float_as_int(float(b0.y)), __float_as_int(float(b0.z)), (127 - b1.z) << 23);
      const int4 h1 = make_int4(b0.w, b1.x, b1.y, b1.w);
      addBasisFast<DERIV, STATS, false>(C, B, h0, h1, field, pos);
#else
      addBasisFunctions<DERIV, STATS>(C, B, b0, b1, field, pos);
#endif
      if (++child >= ri.listSize) break;
      brickID = sc.leafList[ri.listBegin + child];
    }
  }
  if (B.sumW <= 1e-20f) return false;
  value = B.sumWV / B.sumW;
  if (DERIV)
    derivatives = gradOf(B.sumW, B.sumWV, B.sumD, B.sumDC);
  return true;
}

#if EXA_TU_SAMPLE
// the point probes (exa_hip_sample_points / exa_hip_resample) in translation units of their own (-DEXA_TU_SAMPLE=1:
// exa_sample_f*.o hold these kernels and nothing else); everything below is the renderer
#include "exa_sample_kernels.h"
} // namespace EXA_FORM_NS
#elif EXA_TU_STREAM
// the streamline integrator (exa_hip_streamlines) in translation units of its own (-DEXA_TU_STREAM=1: exa_stream_f*.o)
#include "exa_stream_kernels.h"
// ... and the line integral convolution on its evaluation (exa_hip_lic)
#include "exa_lic_kernels.h"
// ... and the flow map of a lattice (exa_hip_flowmap)
#include "exa_flowmap_kernels.h"
} // namespace EXA_FORM_NS
#else

// ------------------------------------------------------------------------
// The dynamic LDS of a workgroup of kKdBlock lanes, described once: the kernels carve theirs by these offsets and the
// launchers ask for `total`, so a carve cannot reach past what its launch reserved.
//   tables        TF tables of EXA_NUM_XF_VALUES float4 each
//   stack walk    per lane a short stack of 12-byte entries (the references, then {tn, tf}) and behind it the segment queue
//                 of 12-byte entries (the regions, then {t0, t1}), each array with a stride of kKdBlock
//   rope walk     no stack: the queue starts where the stack would, in 16-byte entries
//   pad           extra bytes behind everything (occupancy probe)
// ------------------------------------------------------------------------
struct LdsLayout {
  int stackEntries, queueEntries;
  size_t stackRef, stackF, queue, queueT, total;      // byte offsets; the tables are at 0
};
constexpr LdsLayout ldsLayout(int tables, int stackEntries, int queueEntries, bool rope, size_t pad = 0)
{
  const size_t t = size_t(tables) * EXA_NUM_XF_VALUES * sizeof(float4);
  const size_t q = rope ? t : t + size_t(stackEntries) * kKdBlock * 12;
  return { stackEntries, queueEntries, t, t + size_t(stackEntries) * kKdBlock * 4, q, q + size_t(queueEntries) * kKdBlock * 4,
           q + size_t(queueEntries) * kKdBlock * (rope ? 16 : 12) + pad };
}
// the kernels on the stack walk outside the march: surfaces pre-pass, AO rays, wide march (which leaves the queue unused)
constexpr LdsLayout kdLds(int tables) { return ldsLayout(tables, kKdStack, kSegQueue, false); }
// the march: its two-table variant (MULTI == 1) runs with a shorter stack, see renderFrameKdKernel
constexpr LdsLayout marchLds(bool multi1, bool rope, int tables, size_t pad = 0)
{
  return rope ? ldsLayout(tables, 0, multi1 ? kRopeQueueMulti : kRopeQueue, true, pad)
              : ldsLayout(tables, multi1 ? kKdStackMulti : kKdStack, kSegQueue, false, pad);
}
// renderFrameKernel (256 lanes): traceRegion's stack of kStackDepth references per lane (4 bytes each, no floats, no queue)
constexpr LdsLayout lbvhLds(int tables)
{
  const size_t t = ldsLayout(tables, 0, 0, false).total, end = t + size_t(kStackDepth) * 256 * sizeof(int);
  return { kStackDepth, 0, t, end, end, end, end };
}
// do `waves` workgroups (one wave per SIMD each) fit a CU's 160 KB: the occupancy a kernel's launch bounds ask for is only reached then
constexpr bool ldsFits(const LdsLayout &L, int waves) { return L.total * size_t(waves) <= 160 * 1024; }
// this lane's pointers into it (every array has a stride of kKdBlock; queue4: the rope walk's view of the queue)
struct LdsPtrs { float4 *xf; int *stackRef; float *stackF; int *qRegion; float *qT; float4 *queue4; };
__device__ __forceinline__ LdsPtrs carveLds(const LdsLayout &L)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  return { reinterpret_cast<float4 *>(smem), reinterpret_cast<int *>(smem + L.stackRef) + threadIdx.x,
           reinterpret_cast<float *>(smem + L.stackF) + threadIdx.x, reinterpret_cast<int *>(smem + L.queue) + threadIdx.x,
           reinterpret_cast<float *>(smem + L.queueT) + threadIdx.x, reinterpret_cast<float4 *>(smem + L.queue) + threadIdx.x };
}
// the thread's context points at the staged TF tables and at the lane's stack column (an instrumented kernel clears its
// counters itself, behind its clock stamp)
template <int STATS>
__device__ __forceinline__ void initCtx(Ctx<STATS> &C, const RenderArgs &a, const LdsPtrs &lds)
{
  C.a = &a;
  C.xfLds = lds.xf;
  C.stack = lds.stackRef;
  C.guardTripped = false;
}
// The start of a kernel with such a layout: the workgroup stages the TF tables in LDS, then the context is set up
template <int STATS>
__device__ __forceinline__ void kernelPrologue(Ctx<STATS> &C, const RenderArgs &a, const LdsPtrs &lds)
{
  for (int i = threadIdx.x; i < a.numXfChannels * EXA_NUM_XF_VALUES; i += kKdBlock) lds.xf[i] = a.xf[i];
  __syncthreads();
  initCtx(C, a, lds);
}

// framebuffer slot of pixel (px, py) = place (inX, inY) of tile `tile`: row-major for a whole frame, tile-major inside a shard
__device__ __forceinline__ size_t slotOf(const RenderArgs &a, int tile, int inX, int inY, int px, int py)
{ return (a.world == 1) ? size_t(px) + size_t(a.W) * py : size_t(tile / a.world) * kTilePixels + (inY * kTile + inX); }

// ------------------------------------------------------------------------
// exabrick.cu:1591-1594 and Camera.h:27-44: the pixel's random sequence and its jittered camera ray
// ------------------------------------------------------------------------
__device__ __forceinline__ Ray cameraRay(const RenderArgs &a, int px, int py, Lcg &rnd)
{
  const ExaHipFrameState &fs = a.fs;
  rnd.init((uint32_t)(fs.frameID * a.W * a.H) + (uint32_t)px, (uint32_t)py);   // :1591-1592
  const float sx = float(px) + rnd.next();                                      // :1594
  const float sy = float(py) + rnd.next();
  Ray ray;                                                                      // Camera.h:27-44
  ray.org = mk(fs.cam_pos);
  ray.dir = normalize((mk(fs.cam_dir00) + sx * mk(fs.cam_dirDu)) + sy * mk(fs.cam_dirDv));
  ray.tmin = 1e-6f; ray.tmax = 1e8f;
  return ray;
}
// exabrick.cu:1664-1668 (and :1416-1420 of traceIsoRay): the ray in voxel space, its direction normalized; returns dt_scale,
// the length of a world-space unit along it
__device__ __forceinline__ float toVoxelSpace(const ExaHipFrameState &fs, Ray &ray)
{
  ray.org = xfmPoint(fs, ray.org);
  ray.dir = xfmVector(fs, ray.dir);
  const float dt_scale = length(ray.dir);
  ray.dir = normalize(ray.dir);
  return dt_scale;
}
// exabrick.cu:1657-1673: the primary ray ends at the surface hit, is clipped against the clip box (clipRay :1258-1265) and
// goes to voxel space, its interval along with it
__device__ __forceinline__ void clipToVoxelSpace(const ExaHipFrameState &fs, Ray &ray, float surface_t_hit)
{
  ray.tmax = surface_t_hit;                                                     // :1657
  if (fs.clipBox.enabled) {
    float c0, c1;
    boxTest(ray, mk(fs.clipBox.lo), mk(fs.clipBox.hi), c0, c1);
    ray.tmin = c0; ray.tmax = c1;
  }
  const float dt_scale = toVoxelSpace(fs, ray);
  ray.tmin = dt_scale * ray.tmin;                                               // alreadyIntegratedDistance
  ray.tmax = ray.tmax * dt_scale;
}

// the sample's colour after gradient shading and its opacity after the correction; actual_dt != 0
template <bool FAST, int STATS, bool HAVE_RCP = false, bool LEAN = false>
__device__ __forceinline__ Color4 shadeSample(Ctx<STATS> &C, const Ray &ray, float actual_dt, float cellValue, V3 gradient,
                                              float finestLevelCellWidth, int channel, const float rcpRange = 0.f, const float range = 0.f)
{
  Color4 sample = lookupXF<FAST, HAVE_RCP>(C.xfLds, C.a->fs, cellValue, channel, C.a->tfFracMagic, rcpRange, range);
  // the reference compares with `int finestLevelCellWidth` * 1e-6f (exabrick.cu:1124,1001); the width is an
  // integer-valued float (a power of two >= 1, checked at scene creation), so the int round trip is the identity
  if (FAST) {
    // fast_math: transcendental instructions issue at a quarter of the rate, and this block had three of them (sqrt for the
    // threshold, sqrt and rcp for the factor).  The threshold test on the squares and one reciprocal square root keep the
    // shading factor within 2 ulp of the library form (it only scales a colour) at one transcendental
    const float g2 = dotF(gradient, gradient);
    const float thr = finestLevelCellWidth * 1e-6f;
    if (g2 > thr * thr) {
      const V3 lightDir = -ray.dir;
      V3 l2 = lightDir;
      if (LEAN) l2.x = opaque(l2.x);                // |dir|^2 formed here (3 instructions) instead of kept across the march
      const float scale = fabsf(dotF(lightDir, gradient)) * __builtin_amdgcn_rsqf(g2 * dotF(l2, l2));
      sample.x *= scale; sample.y *= scale; sample.z *= scale;
    }
  } else if (fsqrt<FAST>(dotF(gradient, gradient)) > finestLevelCellWidth * 1e-6f) {
    const V3 lightDir = -ray.dir;
    const float scale = fdiv<FAST>(fabsf(dotF(lightDir, gradient)), fsqrt<FAST>(dotF(gradient, gradient) * dotF(lightDir, lightDir)));
    sample.x *= scale; sample.y *= scale; sample.z *= scale;
  }
  // opacity correction 1-(1-a)^dt (exabrick.cu:1011).  FAST: pow as exp2(dt*log2(x)) on the
  // hardware transcendental units — for x in [0,1] and dt of a few voxels within ~2 ulp of a
  // correctly rounded powf (CUDA's own powf is specified to 4 ulp), x==0 -> 0, x==1 -> 1.
  if (FAST) sample.w = 1.f - __builtin_amdgcn_exp2f(actual_dt * __builtin_amdgcn_logf(1.f - sample.w));
  else      sample.w = 1.f - powf(1.f - sample.w, actual_dt);
  return sample;
}

// front-to-back "over" (exabrick.cu:1012-1015)
__device__ __forceinline__ void compositeSample(Color4 &pixelColor, const Color4 &sample)
{
  const float k = (1.f - pixelColor.w) * sample.w;
  if (EXA_F1) {
    pixelColor.x = __builtin_fmaf(k, sample.x, pixelColor.x);
    pixelColor.y = __builtin_fmaf(k, sample.y, pixelColor.y);
    pixelColor.z = __builtin_fmaf(k, sample.z, pixelColor.z);
  } else {
    pixelColor.x += k * sample.x;
    pixelColor.y += k * sample.y;
    pixelColor.z += k * sample.z;
  }
  pixelColor.w += k * 1.f;
}

// exabrick.cu:988-1016 integrateVolume
template <bool FAST, int STATS, bool HAVE_RCP = false, bool LEAN = false>
__device__ __forceinline__ void integrateVolume(Ctx<STATS> &C, const Ray &ray, Color4 &pixelColor, float actual_dt,
                                                float cellValue, V3 gradient, float finestLevelCellWidth, int channel,
                                                const float rcpRange = 0.f, const float range = 0.f)
{
  if (actual_dt == 0.f) return;
  const Color4 sample = shadeSample<FAST, STATS, HAVE_RCP, LEAN>(C, ray, actual_dt, cellValue, gradient, finestLevelCellWidth, channel, rcpRange, range);
  compositeSample(pixelColor, sample);
}

#define EXA_TERMINATION_THRESHOLD 0.98f
#define EXA_MAX_STEPS (1 << 24)

// exabrick.cu:1141-1144
__device__ __forceinline__ float firstSampleT(float t0, float dt, float off)
{
  const int i0 = int(ceilf((t0 - dt * off) / dt));
  float t_i = (off + i0) * dt;
  // the two correction loops almost never run: keep them rolled (unrolled 16x they were 400 instructions), and behind a
  // test of their own — as a plain `for` the first one was compiled with ~15 scalar instructions of loop control that every
  // pop executed (it is the same sequence of subtractions / additions either way)
  if ((t_i - dt) >= t0) {
    int g = 0;
#pragma unroll 1
    do { t_i = t_i - dt; } while (++g < 64 && (t_i - dt) >= t0);
  }
  if (t_i < t0) {
    int g = 0;
#pragma unroll 1
    do { t_i += dt; } while (++g < 64 && t_i < t0);
  }
  return t_i;
}
// the same with x / dt as x * invDt, for a step that is a power of two (invDt = 1/dt exactly, so quotient and product
// are the same real number and round alike)
__device__ __forceinline__ float firstSampleTPow2(float t0, float dt, float invDt, float off)
{
  const int i0 = int(ceilf((t0 - dt * off) * invDt));
  float t_i = (off + i0) * dt;
  if ((t_i - dt) >= t0) {
    int g = 0;
#pragma unroll 1
    do { t_i = t_i - dt; } while (++g < 64 && (t_i - dt) >= t0);
  }
  if (t_i < t0) {
    int g = 0;
#pragma unroll 1
    do { t_i += dt; } while (++g < 64 && t_i < t0);
  }
  return t_i;
}

// exabrick.cu:1116-1185 integrateBrick<GRADIENT_SHADING>
template <bool GRAD, int STATS>
__device__ __forceinline__ void integrateBrick(Ctx<STATS> &C, Color4 &pixelColor, float off, const Ray &ray,
                                               const RegionInfo &ri, float t0, float t1, int numChannels)
{
  const float dt = C.a->p.dt * ri.finestLevelCellWidth;
  const int finestLevelCellWidth = (int)ri.finestLevelCellWidth;
  float t_i = firstSampleT(t0, dt, off);
  float t_last = t0;
  for (int step = 0;; t_i += dt, step++) {
    if (step >= EXA_MAX_STEPS) { C.guardTripped = true; break; }
    const float t_next = fminf(t_i, t1);
    const float t_sample = 0.5f * (fminf(t1, t_next) + t_last);
    const float actual_dt = t_next - t_last;
    t_last = t_next;
    const V3 pos = rayAt(ray.org, t_sample, ray.dir);
    float cellValue = 0.f;
    V3 grad = mk(0.f, 0.f, 0.f);
    for (int c = 0; c < numChannels; ++c) {
      C.count(ST_SAMPLE_EVALS);
      if (samplePoint<GRAD, STATS>(C, cellValue, grad, ri, pos, c)) {
        C.count(ST_SAMPLES);
        integrateVolume<false>(C, ray, pixelColor, actual_dt, cellValue, grad, finestLevelCellWidth, c);
      }
    }
    if (pixelColor.w >= EXA_TERMINATION_THRESHOLD) break;
    if (t_next >= t1) break;
  }
}

// ------------------------------------------------------------------------
// implicit iso-surface path
// ------------------------------------------------------------------------
struct IsoResult { Color4 pixelColor; float t_hit; V3 gradient; };

// exabrick.cu:1018-1114 IsoSurfaceIntegrationFunction::operator()
template <int STATS>
__device__ void isoFunc(Ctx<STATS> &C, const float last_t, const float lastCellValue, const Ray &ray, IsoResult &result,
                        float t_sample, float cellValueIn, const RegionInfo &ri, int channel, const bool hitOnly = false)
{
  const ExaHipFrameState &fs = C.a->fs;
  if (lastCellValue >= -1e35f) {
    for (int i = 0; i < EXA_MAX_ISO_SURFACES; i++) {
      const float isoV = fs.iso[i].value;
      if (fs.iso[i].enabled && fs.iso[i].channel == channel
          && ((lastCellValue <= isoV && cellValueIn >= isoV) || (lastCellValue >= isoV && cellValueIn <= isoV))) {
        const float d1 = fabsf(lastCellValue - isoV);
        const float d2 = fabsf(cellValueIn - isoV);
        const float w1 = 1.f - d1 / (d1 + d2);
        const float w2 = 1.f - d2 / (d1 + d2);
        const float tavg = last_t * w1 + t_sample * w2;
        if (hitOnly && STATS != 1) {
          // An ambient-occlusion ray only asks WHETHER and WHERE it hits (exabrick.cu:1640-1643 reads primID, the trace
          // compares t_hit): colour and normal of the hit — the re-sampling at the crossing point, :1056-1085 — are
          // never read.  What the rest of the march does see is the opacity, which the opaque sample (:1086) brings to
          // (1 - w) * 1 + w whatever its colour, and the hit distance.  (The counting variant keeps the full form.)
          result.pixelColor.w += (1.f - result.pixelColor.w) * 1.f * 1.f;
          result.t_hit = tavg;
          continue;
        }
        float cellValue = 0.f;
        V3 grad = mk(0.f, 0.f, 0.f);
        Color4 sample; sample.x = 1.f; sample.y = 0.f; sample.z = 0.f; sample.w = 1.f;
        const V3 isopt = ray.org + tavg * ray.dir;
        C.count(ST_ISO_EVALS);
        if (C.a->p.gradientShadingISO) {
          if (samplePoint<true, STATS>(C, cellValue, grad, ri, isopt, fs.iso[i].channel)) {
            sample = lookupXF(C.xfLds, fs, cellValue, fs.iso[i].channel, C.a->tfFracMagic);
            grad = normalize(grad);
            if (dot(grad, ray.dir) > 0.f) grad = -grad;
          }
        } else {
          V3 unused;
          if (samplePoint<false, STATS>(C, cellValue, unused, ri, isopt, fs.iso[i].channel))
            sample = lookupXF(C.xfLds, fs, cellValue, fs.iso[i].channel, C.a->tfFracMagic);
        }
        if (C.a->p.colormapChannel != 0) {
          cellValue = 0.f;
          V3 unused;
          C.count(ST_ISO_EVALS);
          if (samplePoint<false, STATS>(C, cellValue, unused, ri, isopt, C.a->p.colormapChannel))
            sample = lookupXF(C.xfLds, fs, cellValue, 0, C.a->tfFracMagic);
        }
        sample.w = 1.f;
        if (!isfinite(grad.x) || !isfinite(grad.y) || !isfinite(grad.z)) grad = mk(0.f, 0.f, 0.f);
        if (length(grad) > .0f) {
          const V3 lightDir = -ray.dir;
          const float scale = .3f + .7f * fabsf(dot(lightDir, grad)) / sqrtf(dot(grad, grad));
          sample.x *= scale; sample.y *= scale; sample.z *= scale;
        }
        const float k = (1.f - result.pixelColor.w) * sample.w;
        result.pixelColor.x += k * sample.x;
        result.pixelColor.y += k * sample.y;
        result.pixelColor.z += k * sample.z;
        result.pixelColor.w += k * 1.f;
        result.t_hit = tavg;
        result.gradient = grad;
      }
    }
  }
  // last_t = t_sample; lastCellValue = cellValueIn (:1112-1113): the caller's IsoLast::set
}

// The functor state of traceIsoRay (IsoSurfaceIntegrationFunction[MAX_CHANNELS], exabrick.cu:1424): per channel the
// previous sample's distance and value.  Only the channels an enabled iso-surface refers to are ever read (the crossing
// test is behind `iso.channel == channel`, :1038), so two slots hold everything that is observable — in registers, where
// an array indexed by the channel lives in scratch memory.
struct IsoLast {
  float t0, v0, t1, v1;
  int ch0, ch1;                     // channel of slot 0 / 1 (-1: unused)
  __device__ __forceinline__ void init(const ExaHipFrameState &fs)
  {
    t0 = t1 = 0.f; v0 = v1 = -1e36f;
    ch0 = fs.iso[0].enabled ? fs.iso[0].channel : -1;
    ch1 = (fs.iso[1].enabled && !(fs.iso[0].enabled && fs.iso[1].channel == fs.iso[0].channel)) ? fs.iso[1].channel : -1;
  }
  __device__ __forceinline__ float lastT(int c) const { return c == ch0 ? t0 : (c == ch1 ? t1 : 0.f); }
  __device__ __forceinline__ float lastV(int c) const { return c == ch0 ? v0 : (c == ch1 ? v1 : -1e36f); }
  __device__ __forceinline__ void set(int c, float t, float v)
  {
    if (c == ch0) { t0 = t; v0 = v; }
    else if (c == ch1) { t1 = t; v1 = v; }
  }
};

struct SurfaceHit { int primID; float t_hit; V3 Ng; float ambient; V3 baseColor; };
#define EXA_PRIMID_ISOSURFACE (-23)

// ------------------------------------------------------------------------
// contour planes (exabrick.cu:1267-1406)
// ------------------------------------------------------------------------
#define EXA_PRIMID_PLANE (-24)

__device__ __forceinline__ float intersectLinePlane(V3 p1, V3 p2, V3 normal, float offset)      // :1267-1284
{
  const float s = dot(normal, normalize(p2 - p1));
  if (s == 0.f) return -1.f;
  const float t = (offset - dot(normal, p1)) / s;
  if (t < 0.f || t > length(p2 - p1)) return -1.f;
  return t;
}

__device__ __forceinline__ float intersectRayTriangle(const Ray &ray, V3 v1, V3 e1, V3 e2)      // :1316-1343
{
  const V3 s1 = cross(ray.dir, e2);
  const float div = dot(s1, e1);
  if (div == 0.f) return -1.f;
  const float invDiv = 1.f / div;
  const V3 d = ray.org - v1;
  const float b1 = dot(d, s1) * invDiv;
  if (b1 < 0.f || b1 > 1.f) return -1.f;
  const V3 s2 = cross(d, e1);
  const float b2 = dot(ray.dir, s2) * invDiv;
  if (b2 < 0.f || b1 + b2 > 1.f) return -1.f;
  return dot(e2, s2) * invDiv;
}

// traceContourRay (:1345-1406).  findRegion(pos) is the degenerate trace of samplePointWithInfRay
// (:818-830: origin pos, direction (1,1,1), [0, 2e-10]) on whichever structure the kernel walks;
// the reference reads region[-1] when it misses, here the sample is skipped (value 0).
template <int STATS, class FindRegion>
__device__ SurfaceHit traceContourRay(Ctx<STATS> &C, const Ray &ray, V3 normal, float offset, int channel, FindRegion findRegion)
{
  SurfaceHit prd;
  prd.primID = -1; prd.t_hit = ray.tmax; prd.Ng = mk(0.f, 0.f, 0.f); prd.ambient = 0.f; prd.baseColor = mk(0.f, 0.f, 0.f);
  V3 pts[6];
  int isectCnt = 0;
  {                                                                 // intersectBoxPlane on the unit box (:1287-1314)
    const int key[4][3] = { {0,0,0}, {1,0,1}, {1,1,0}, {0,1,1} };
    for (int i = 0; i < 4 && isectCnt < 6; ++i)
      for (int j = 0; j < 3 && isectCnt < 6; ++j) {
        const V3 p1 = mk(float(j == 0 ? 1 - key[i][0] : key[i][0]), float(j == 1 ? 1 - key[i][1] : key[i][1]),
                         float(j == 2 ? 1 - key[i][2] : key[i][2]));
        const V3 p2 = mk(float(key[i][0]), float(key[i][1]), float(key[i][2]));
        const float t = intersectLinePlane(p1, p2, normal, offset);
        if (t >= 0.f) pts[isectCnt++] = p1 + t * normalize(p2 - p1);
      }
  }
  const V3 wlo = mk(C.a->worldLo), whi = mk(C.a->worldHi);
  for (int i = 0; i < isectCnt; ++i) {                              // scale to world bounds (:1359-1362)
    const V3 sz = whi - wlo;
    pts[i] = mk(pts[i].x * sz.x, pts[i].y * sz.y, pts[i].z * sz.z) + wlo;
  }
  float t = -1.f;
  for (int i = 0; i < isectCnt - 1; ++i) {                          // cyclical selection sort (:1367-1382)
    int minIdx = i;
    for (int j = i + 1; j < isectCnt; ++j) {
      const V3 v = cross(pts[j] - pts[0], pts[minIdx] - pts[0]);
      if (dot(v, normal) < 0.f) minIdx = j;
    }
    const V3 tmp = pts[i]; pts[i] = pts[minIdx]; pts[minIdx] = tmp;
  }
  for (int i = 2; i < isectCnt; ++i) {                              // triangle fan (:1384-1391)
    const V3 v1 = pts[0], e1 = pts[i - 1] - v1, e2 = pts[i] - v1;
    const float tt = intersectRayTriangle(ray, v1, e1, e2);
    if (tt >= 0.f && (tt < t || t < 0.f)) t = tt;
  }
  if (t < 0.f) return prd;
  const V3 pos = ray.org + t * ray.dir;
  float value = 0.f;
  const int region = findRegion(pos);
  if (region >= 0) {
    V3 unused;
    samplePoint<false, STATS>(C, value, unused, C.a->sc.regionInfo[region], pos, 0);   // :1396, channel 0
  }
  const Color4 sample = lookupXF(C.xfLds, C.a->fs, value, channel, C.a->tfFracMagic);
  prd.primID = EXA_PRIMID_PLANE;
  prd.t_hit = t;
  prd.Ng = normal;
  prd.ambient = 0.f;
  prd.baseColor = mk(sample.x, sample.y, sample.z);
  return prd;
}

// ------------------------------------------------------------------------
// triangle surfaces: the surfaceModel trace of traceSurfaces (exabrick.cu:1483-1486) and its
// closest-hit program (:420-433).  OptiX's built-in triangle test is replaced by the reference's own
// intersectRayTriangle (:1316-1343); closest t in (tmin,tmax), lowest triangle index on a tie.
// ------------------------------------------------------------------------
template <int STATS>
__device__ void traceMeshes(Ctx<STATS> &C, const Ray &ray, SurfaceHit &prd)
{
  const RenderArgs &a = *C.a;
  float best = ray.tmax;
  int hit = -1;
  int stack[kStackDepth];
  int sp = 0, node = 0;
  Ray r = ray;
  for (;;) {
    const float4 *np = reinterpret_cast<const float4 *>(a.meshNodes + node);
    const float4 q0 = np[0], q1 = np[1], q2 = np[2];
    const int4 cc = *reinterpret_cast<const int4 *>(np + 3);
    r.tmax = best;
    float a0, a1, b0, b1;
    boxTest(r, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), a0, a1);
    boxTest(r, mk(q1.z, q1.w, q2.x), mk(q2.y, q2.z, q2.w), b0, b1);
    bool ha = a0 <= a1 && q0.x <= q0.w, hb = b0 <= b1 && q1.z <= q2.y;
    for (int side = 0; side < 2; side++) {
      const int c = side ? cc.y : cc.x;
      if (!(side ? hb : ha) || c >= 0 || c == INT32_MIN) continue;
      const int tri = ~c;
      const int i0 = a.meshTris[3 * tri], i1 = a.meshTris[3 * tri + 1], i2 = a.meshTris[3 * tri + 2];
      const V3 A = mk(a.meshVerts + 3 * i0), B = mk(a.meshVerts + 3 * i1), Cv = mk(a.meshVerts + 3 * i2);
      const float tt = intersectRayTriangle(ray, A, B - A, Cv - A);
      if (tt > ray.tmin && (tt < best || (tt == best && hit >= 0 && tri < hit))) { best = tt; hit = tri; }
    }
    ha = ha && cc.x >= 0; hb = hb && cc.y >= 0;
    if (ha && hb) {
      const bool aFirst = a0 <= b0;
      if (sp < kStackDepth) stack[sp++] = aFirst ? cc.y : cc.x;
      node = aFirst ? cc.x : cc.y;
    } else if (ha) node = cc.x;
    else if (hb) node = cc.y;
    else { if (sp == 0) break; node = stack[--sp]; }
  }
  if (hit >= 0) {
    const int i0 = a.meshTris[3 * hit], i1 = a.meshTris[3 * hit + 1], i2 = a.meshTris[3 * hit + 2];
    const V3 A = mk(a.meshVerts + 3 * i0), B = mk(a.meshVerts + 3 * i1), Cv = mk(a.meshVerts + 3 * i2);
    prd.t_hit = best;
    prd.primID = hit;
    prd.Ng = normalize(cross(B - A, Cv - A));
    prd.ambient = .2f;
    prd.baseColor = mk(.8f, .8f, .8f);
  }
}

// ------------------------------------------------------------------------
// streamlines: rounded-cone segments (exabrick.cu:440-570) under a BVH over the segments the
// Streamline bounds program leaves visible; closest accepted t, lowest primitive id on a tie
// ------------------------------------------------------------------------
#define EXA_PRIMID_STREAMLINE (-25)

__device__ __forceinline__ bool intersectRoundedCone(V3 pa, V3 pb, float ra, float rb, const Ray &ray, float &hit_t, V3 &isec_normal)
{
  V3 ro = ray.org;
  const V3 rd = ray.dir;
  const float minDist = fmaxf(0.f, fminf(length(pa - ro) - ra, length(pb - ro) - rb));
  ro = ro + minDist * rd;
  const V3 ba = pb - pa, oa = ro - pa;
  const float rr = ra - rb;
  const float m0 = dot(ba, ba), m1 = dot(ba, oa), m2 = dot(ba, rd), m3 = dot(rd, oa), m5 = dot(oa, oa);
  const float d2 = m0 - rr * rr;
  const float k2 = d2 - m2 * m2;
  const float k1 = d2 * m3 - m1 * m2 + m2 * rr * ra;
  const float k0 = d2 * m5 - m1 * m1 + m1 * rr * ra * 2.0f - m0 * ra * ra;
  const float h = k1 * k1 - k0 * k2;
  if (h < 0.0f) return false;
  float t = (-sqrtf(h) - k1) / k2;
  const float y = m1 - ra * rr + t * m2;
  if (y > 0.0f && y < d2) {
    hit_t = minDist + t;
    isec_normal = d2 * (oa + t * rd) - y * ba;
    return true;
  }
  const float h1 = m3 * m3 - m5 + ra * ra;                       // caps
  if (h1 > 0.0f) {
    t = -m3 - sqrtf(h1);
    hit_t = minDist + t;
    const V3 q = oa + t * rd;
    isec_normal = mk(q.x / ra, q.y / ra, q.z / ra);
    return true;
  }
  return false;
}

template <int STATS>
__device__ void traceStreamlines(Ctx<STATS> &C, const Ray &ray, SurfaceHit &prd)
{
  const RenderArgs &a = *C.a;
  float best = 2e10f;                                             // streamlinePRD.t_hit (:1507)
  int hit = -1;
  V3 bestN = mk(0.f, 0.f, 0.f);
  int stack[kStackDepth];
  int sp = 0, node = 0;
  Ray r = ray;
  for (;;) {
    const float4 *np = reinterpret_cast<const float4 *>(a.streamNodes + node);
    const float4 q0 = np[0], q1 = np[1], q2 = np[2];
    const int4 cc = *reinterpret_cast<const int4 *>(np + 3);
    r.tmax = fminf(ray.tmax, best);
    float a0, a1, b0, b1;
    boxTest(r, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), a0, a1);
    boxTest(r, mk(q1.z, q1.w, q2.x), mk(q2.y, q2.z, q2.w), b0, b1);
    bool ha = a0 <= a1 && q0.x <= q0.w, hb = b0 <= b1 && q1.z <= q2.y;
    for (int side = 0; side < 2; side++) {
      const int c = side ? cc.y : cc.x;
      if (!(side ? hb : ha) || c >= 0 || c == INT32_MIN) continue;
      const int prim = ~c;
      const V3 pa = mk(a.traces + 3 * size_t(prim)), pb = mk(a.traces + 3 * (size_t(prim) + 1));
      float th; V3 n;
      if (!intersectRoundedCone(pa, pb, 2.f, 2.f, ray, th, n)) continue;
      if (th >= ray.tmin && th <= ray.tmax && (th < best || (th == best && hit >= 0 && prim < hit))) { best = th; hit = prim; bestN = n; }
    }
    ha = ha && cc.x >= 0; hb = hb && cc.y >= 0;
    if (ha && hb) {
      const bool aFirst = a0 <= b0;
      if (sp < kStackDepth) stack[sp++] = aFirst ? cc.y : cc.x;
      node = aFirst ? cc.x : cc.y;
    } else if (ha) node = cc.x;
    else if (hb) node = cc.y;
    else { if (sp == 0) break; node = stack[--sp]; }
  }
  if (hit >= 0 && best < prd.t_hit) {                             // :1510-1511
    prd.primID = EXA_PRIMID_STREAMLINE;
    prd.t_hit = best;
    prd.Ng = normalize(bestN);
    prd.baseColor = mk(.8f, .8f, .8f);
    prd.ambient = 0.f;
  }
}

// exabrick.cu:1187-1256 isoIntegrateBrick
template <int STATS>
__device__ void isoIntegrateBrick(Ctx<STATS> &C, IsoLast &last, IsoResult &ir, float off,
                                  const Ray &ray, const RegionInfo &ri, float t0, float t1, int numChannels, const bool hitOnly = false)
{
  unsigned isoChannelMask = 0;
  for (int i = 0; i < EXA_MAX_ISO_SURFACES; i++)
    if (C.a->fs.iso[i].enabled) isoChannelMask |= 1u << (C.a->fs.iso[i].channel & 31);
  // (keeping a one-brick region's march header in registers across the segment was measured: the eight registers cost
  // the iso-only pre-pass its fourth wave per SIMD — C3 3.6 -> 4.0 ms, C5 10.9 -> 13.9 ms — and spill in the generic one)
  const float dt = C.a->p.dt * ri.finestLevelCellWidth;
  float t_i = firstSampleT(t0, dt, off);
  float t_last = t0;
  for (int step = 0;; t_i += dt, step++) {
    if (step >= EXA_MAX_STEPS) { C.guardTripped = true; break; }
    C.isoSteps++;
    const float t_next = fminf(t_i, t1);
    const float t_sample = 0.5f * (fminf(t1, t_next) + t_last);
    t_last = t_next;
    const V3 pos = ray.org + t_sample * ray.dir;
    for (int c = 0; c < numChannels; ++c) {
      // A channel no enabled iso-surface refers to only feeds last_t/lastCellValue[c], which nothing
      // reads; its sample matters solely through the `break` below once the segment already holds an
      // opaque hit.  Outside that case it is skipped (the instrumented variant keeps the reference's
      // full count of evaluations).
      if (STATS != 1 && !((isoChannelMask >> c) & 1u) && ir.pixelColor.w < EXA_TERMINATION_THRESHOLD) continue;
      float cellValue = 0.f;
      V3 grad = mk(0.f, 0.f, 0.f);
      C.count(ST_ISO_EVALS);
      // The reference samples with the derivative here when gradientShadingISO is on (:1224-1231), but the functor never
      // looks at it (:1019-1110 takes the gradient from its own re-sampling at the crossing point): value and validity
      // are the same sums either way, so the step samples are taken without the derivative sums
      const bool doIntegrate = samplePoint<false, STATS>(C, cellValue, grad, ri, pos, c);
      if (doIntegrate) {
        isoFunc(C, last.lastT(c), last.lastV(c), ray, ir, t_sample, cellValue, ri, c, hitOnly);
        last.set(c, t_sample, cellValue);
        if (ir.pixelColor.w >= EXA_TERMINATION_THRESHOLD) break;   // leaves the channel loop only
      }
    }
    if (t_next >= t1) break;
  }
}

// exabrick.cu:1408-1460 traceIsoRay (LBVH: one closest-region search per segment)
template <int STATS>
__device__ SurfaceHit traceIsoRay(Ctx<STATS> &C, Ray ray, float off)
{
  const ExaHipFrameState &fs = C.a->fs;
  const float dt_scale = toVoxelSpace(fs, ray);                 // :1416-1420
  float alreadyIntegratedDistance = dt_scale * ray.tmin;
  IsoLast last;
  last.init(fs);
  SurfaceHit result;
  result.primID = -1; result.t_hit = ray.tmax; result.Ng = mk(0.f, 0.f, 0.f);
  result.ambient = 0.f; result.baseColor = mk(0.f, 0.f, 0.f);
  for (int seg = 0;; seg++) {
    if (seg >= (1 << 22)) { C.guardTripped = true; break; }
    ray.tmin = alreadyIntegratedDistance;
    ray.tmax = ray.tmax * dt_scale;                       // :1434 (re-applied every iteration)
    const RegionHit prd = traceRegion(C, C.a->isoNodes, ray);
    if (prd.leafID < 0) break;
    C.count(ST_ISO_SEGMENTS);
    const RegionInfo ri = C.a->sc.regionInfo[prd.leafID];
    IsoResult ir;
    ir.pixelColor.x = ir.pixelColor.y = ir.pixelColor.z = ir.pixelColor.w = 0.f;
    ir.t_hit = -1.f; ir.gradient = mk(0.f, 0.f, 0.f);
    isoIntegrateBrick(C, last, ir, off, ray, ri, fmaxf(ray.tmin, prd.t0), fminf(ray.tmax, prd.t1),
                      C.a->p.numPrimaryChannels);
    if (ir.t_hit >= 0.f) {
      result.primID = EXA_PRIMID_ISOSURFACE;
      result.t_hit = ir.t_hit / dt_scale;
      result.Ng = normalize(ir.gradient);
      result.ambient = 0.f;
      result.baseColor = mk(ir.pixelColor.x, ir.pixelColor.y, ir.pixelColor.z);
      return result;
    }
    alreadyIntegratedDistance = prd.t1 * (1.0000001f);
  }
  return result;
}

// exabrick.cu:1475-1529 traceSurfaces: contour planes, then implicit iso-surfaces
template <int STATS>
__device__ __forceinline__ void traceSurfaces(Ctx<STATS> &C, const Ray &ray, SurfaceHit &prd, bool withContourPlanes)
{
  prd.primID = -1;
  prd.t_hit = ray.tmax;
  prd.Ng = mk(0.f, 0.f, 0.f); prd.ambient = 0.f; prd.baseColor = mk(0.f, 0.f, 0.f);
  if (C.a->numTris > 0) traceMeshes(C, ray, prd);                 // ST_MESHES (also for AO rays)
  if (withContourPlanes) {
    for (int i = 0; i < EXA_MAX_CONTOUR_PLANES; ++i)
      if (C.a->fs.contour[i].enabled) {
        auto find = [&](V3 pos) {
          Ray r; r.org = pos; r.dir = mk(1.f, 1.f, 1.f); r.tmin = 0.f; r.tmax = 2e-10f;
          return traceRegion(C, C.a->volNodes, r).leafID;
        };
        const SurfaceHit c = traceContourRay(C, ray, mk(C.a->fs.contour[i].normal), C.a->fs.contour[i].offset,
                                             C.a->fs.contour[i].channel, find);
        if (c.primID == EXA_PRIMID_PLANE && c.t_hit < prd.t_hit) prd = c;
      }
  }
  if (C.a->numStreamPrims > 0) traceStreamlines(C, ray, prd);     // ST_STREAMLINES (:1503-1512)
  bool activeIso = false;
  for (int i = 0; i < EXA_MAX_ISO_SURFACES; i++) activeIso |= (C.a->fs.iso[i].enabled != 0);
  if (activeIso) {
    const SurfaceHit isoPRD = traceIsoRay(C, ray, 0.f);
    if (isoPRD.primID == EXA_PRIMID_ISOSURFACE && isoPRD.t_hit < prd.t_hit) prd = isoPRD;
  }
}

// ------------------------------------------------------------------------
// exabrick.cu:1576-1720 renderFrame
// ------------------------------------------------------------------------
template <bool GRAD, bool ISO, int STATS>
__global__ __launch_bounds__(256) void renderFrameKernel(const RenderArgs a)
{
  const LdsPtrs lds = carveLds(lbvhLds(a.numXfChannels));
  // (kernelPrologue and, below, clipToVoxelSpace and the surface shading stay written out here and in the pre-pass where a
  // function moved a shipped variant's registers or spills: profiles/march_dedup_equivalence.txt)
  for (int i = threadIdx.x; i < a.numXfChannels * EXA_NUM_XF_VALUES; i += 256) lds.xf[i] = a.xf[i];
  __syncthreads();
  Ctx<STATS> C;
  initCtx(C, a, lds);
  const unsigned long long clockBegin = clock64();                              // :1588
  if (STATS) for (int i = 0; i < ST_COUNT; i++) C.st[i] = 0;
  // tile -> pixel: wave w covers the 8x8 block (w&1, w>>1) of the 16x16 tile
  const int tile = a.tileMap[blockIdx.x];
  const int tx = tile % a.tilesX, ty = tile / a.tilesX;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int inX = ((wave & 1) << 3) + laneX(lane), inY = ((wave >> 1) << 3) + laneY(lane);
  const int px = tx * kTile + inX, py = ty * kTile + inY;
  const bool inside = px < a.W && py < a.H && (a.debugPixel < 0 || a.debugPixel == px + a.W * py);

  if (inside) {
    const ExaHipFrameState &fs = a.fs;
    const int frameID = fs.frameID;
    Lcg rnd;
    Ray ray = cameraRay(a, px, py, rnd);

    SurfaceHit surface;
    surface.primID = -1; surface.t_hit = ray.tmax;
    surface.Ng = mk(0.f, 0.f, 0.f); surface.ambient = 0.f; surface.baseColor = mk(0.f, 0.f, 0.f);
    V3 bgColor = mk(0.f, 0.f, 0.f);
    if (ISO) {
      traceSurfaces(C, ray, surface, true);                                       // :1601
      if (surface.primID >= 0 || surface.primID == EXA_PRIMID_ISOSURFACE || surface.primID == EXA_PRIMID_PLANE
          || surface.primID == EXA_PRIMID_STREAMLINE) {   // :1604-1652
        const bool shade = surface.primID >= 0 || surface.primID == EXA_PRIMID_PLANE || surface.primID == EXA_PRIMID_STREAMLINE
                        || (surface.primID == EXA_PRIMID_ISOSURFACE && a.p.gradientShadingISO);
        if (shade && length(surface.Ng) > 0.f) {
          const float AO_Radius = fs.ao.length;
          const int AO_Samples = fs.ao.enabled ? 2 : 0;
          const V3 isect_pos = ray.org + surface.t_hit * ray.dir;
          const V3 w = surface.Ng;
          const V3 v = fabsf(w.x) > fabsf(w.y) ? normalize(mk(-w.z, 0.f, w.x)) : normalize(mk(0.f, w.z, -w.y));
          const V3 u = cross(v, w);
          int hitCnt = 0;
          for (int i = 0; i < AO_Samples; ++i) {
            const float u1 = rnd.next(), u2 = rnd.next();
            const float r = sqrtf(u1);
            const float theta = 2.f * 3.14159265358979323846f * u2;
            const V3 sp = mk(r * cosf(theta), r * sinf(theta), sqrtf(1.f - u1));
            Ray ao_ray;
            ao_ray.org = isect_pos;
            ao_ray.dir = normalize((sp.x * u + sp.y * v) + sp.z * w);
            ao_ray.tmin = 1e-4f; ao_ray.tmax = AO_Radius;
            SurfaceHit ao;
            traceSurfaces(C, ao_ray, ao, false);
            if (ao.primID >= 0 || ao.primID == EXA_PRIMID_ISOSURFACE || ao.primID == EXA_PRIMID_PLANE
                || ao.primID == EXA_PRIMID_STREAMLINE) hitCnt++;
          }
          const float shadow = fs.ao.enabled ? (float)hitCnt / AO_Samples : 0.f;
          const float fd = fabsf(dot(ray.dir, surface.Ng));
          const float ns = 1.f - shadow;
          bgColor = mk(surface.ambient + surface.baseColor.x * fd * ns,
                       surface.ambient + surface.baseColor.y * fd * ns,
                       surface.ambient + surface.baseColor.z * fd * ns);
        } else {
          bgColor = surface.baseColor;
        }
      }
    }

    Color4 pixelColor; pixelColor.x = pixelColor.y = pixelColor.z = pixelColor.w = 0.f;
    const float interleavedSamplingOffset = rnd.next();                           // :1655
    ray.tmax = surface.t_hit;                                                     // :1657
    if (fs.clipBox.enabled) {                                                     // clipRay :1258-1265
      float c0, c1;
      boxTest(ray, mk(fs.clipBox.lo), mk(fs.clipBox.hi), c0, c1);
      ray.tmin = c0; ray.tmax = c1;
    }
    surface.t_hit = ray.tmax;

    ray.org = xfmPoint(fs, ray.org);                                              // :1664-1668
    ray.dir = xfmVector(fs, ray.dir);
    const float dt_scale = length(ray.dir);
    ray.dir = normalize(ray.dir);

    float alreadyIntegratedDistance = dt_scale * ray.tmin;
    for (int seg = 0;; seg++) {                                                   // :1675-1699
      if (seg >= (1 << 22)) { C.guardTripped = true; break; }
      ray.tmin = alreadyIntegratedDistance;
      ray.tmax = surface.t_hit * dt_scale;
      const RegionHit prd = traceRegion(C, a.volNodes, ray);
      if (prd.leafID < 0) break;
      C.count(ST_SEGMENTS);
      const RegionInfo ri = a.sc.regionInfo[prd.leafID];
      integrateBrick<GRAD, STATS>(C, pixelColor, interleavedSamplingOffset, ray, ri, prd.t0, prd.t1,
                                  a.p.numPrimaryChannels);
      if (pixelColor.w >= EXA_TERMINATION_THRESHOLD) {
        pixelColor.x = pixelColor.x * pixelColor.w;                               // :1695
        pixelColor.y = pixelColor.y * pixelColor.w;
        pixelColor.z = pixelColor.z * pixelColor.w;
        pixelColor.w = 1.f;
        break;
      }
      alreadyIntegratedDistance = prd.t1 * (1.0000001f);
    }

    float cr = pixelColor.w * pixelColor.x + (1.f - pixelColor.w) * bgColor.x;    // :1701
    float cg = pixelColor.w * pixelColor.y + (1.f - pixelColor.w) * bgColor.y;
    float cb = pixelColor.w * pixelColor.z + (1.f - pixelColor.w) * bgColor.z;
    if (fs.clockScale > 0.f) cr = clockHeat(fs.clockScale, clockBegin);          // :1703-1707

    const size_t slot = slotOf(a, tile, inX, inY, px, py);
    if (frameID > 0) {                                                            // :1709-1710
      const float4 acc = a.accum[slot];
      cr += acc.x; cg += acc.y; cb += acc.z;
    }
    a.accum[slot] = make_float4(cr, cg, cb, 1.f);                                 // :1712
    const float div = frameID + 1.f;
    cr = cr / div; cg = cg / div; cb = cb / div;
    // colorRowMajor: a device of a multi-device handle stores its tiles straight into the root's row-major frame
    a.color[a.colorRowMajor ? size_t(px) + size_t(a.W) * py : slot] = make_rgba8(linear_to_srgb(cr), linear_to_srgb(cg), linear_to_srgb(cb));
  }

  if (C.guardTripped) atomicExch(a.errorFlag, 1);
  if (STATS) {
    // wave-level reduction, one atomic per wave and counter
    for (int i = 0; i < ST_COUNT; i++) {
      unsigned long long v = inside ? C.st[i] : 0ull;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.stats[i], v);
    }
  }
}

#if !EXA_TU_ROPE
hipError_t launchRender(const RenderArgs &a, int numBlocks, bool grad, bool iso, bool stats, hipStream_t s)
{
  if (numBlocks <= 0) return hipSuccess;
  const size_t lds = lbvhLds(a.numXfChannels).total;
  const dim3 grid(numBlocks), block(256);
#define EXA_LAUNCH(G, I, S) hipLaunchKernelGGL((renderFrameKernel<G, I, S>), grid, block, lds, s, a)
  if (stats) {
    if (grad) { if (iso) EXA_LAUNCH(true, true, true); else EXA_LAUNCH(true, false, true); }
    else      { if (iso) EXA_LAUNCH(false, true, true); else EXA_LAUNCH(false, false, true); }
  } else {
    if (grad) { if (iso) EXA_LAUNCH(true, true, false); else EXA_LAUNCH(true, false, false); }
    else      { if (iso) EXA_LAUNCH(false, true, false); else EXA_LAUNCH(false, false, false); }
  }
#undef EXA_LAUNCH
  return hipGetLastError();
}
#endif // !EXA_TU_ROPE

// ========================================================================
// v2: region kd-tree walked front to back + flattened march.
//
// The recursion of ExaBrickRegions::buildRec is a kd-tree whose leaves are the
// regions, so the regions a ray crosses come out of one ordered walk: no restart
// per segment (exabrick.cu:1675-1699 re-traces the BVH for every region) and one
// 16-byte node + one division per step instead of a 64-byte node + 12 divisions.
// Every visited leaf still gets the reference's exact slab test against its
// domain with the current ray.tmin, so accepted segments [t0,t1] are the ones
// the closest-hit search returns (disjoint boxes: the first accepted leaf in
// front-to-back order is the one with the smallest clamped t0).
//
// The march itself is one loop whose unit of work is ONE brick visit
// (addBasisFunctions).  Lanes of a wave sit in regions with different brick
// counts k and different segment lengths; with nested loops a wave runs at the
// pace of its slowest lane in every loop level, flattened it only idles in the
// short per-sample epilogue.  Per-sample arithmetic and its order are unchanged.
// ========================================================================
// small counters of the walk and the segment queue share one register:
//   bits 0-3 stack head | 4-7 stack count | 8 dropped | 12-15 queue head | 16-19 queue count
struct Packed {
  unsigned v;
  __device__ __forceinline__ int get(int sh) const { return (v >> sh) & 15; }
  __device__ __forceinline__ void set(int sh, int x) { v = (v & ~(15u << sh)) | ((unsigned)x << sh); }
  // cheaper forms for the updates every pop / push / accept makes (same values as get + set):
  __device__ __forceinline__ void inc(int sh) { v += 1u << sh; }                 // field + 1 (caller: no overflow of the 4 bits)
  __device__ __forceinline__ void dec(int sh) { v -= 1u << sh; }                 // field - 1 (caller: field > 0)
  __device__ __forceinline__ void setBit(int sh) { v |= 1u << sh; }              // a 0 / 1 field := 1
  __device__ __forceinline__ void clearField(int sh) { v &= ~(15u << sh); }      // field := 0
  // ring index + 1 modulo N (N a power of two: add and mask in place; else compare and select)
  template <int N> __device__ __forceinline__ void incWrap(int sh)
  {
    if ((N & (N - 1)) == 0) v = (v & ~(15u << sh)) | ((v + (1u << sh)) & ((unsigned)(N - 1) << sh));
    else { const int x = get(sh); set(sh, x == N - 1 ? 0 : x + 1); }
  }
};
enum { PK_SHEAD = 0, PK_SCOUNT = 4, PK_DROPPED = 8, PK_QHEAD = 12, PK_QCOUNT = 16, PK_NEEDHDR = 20 };

struct KdWalk {
  int   ref;            // current subtree reference, or KD_DONE
  float tn, tf;         // its interval along the ray
  float tEnd;           // end of the root interval
  Packed pk;            // short stack head/count/dropped (circular stack in LDS) + queue head/count
};
#define EXA_KD_DONE (EXA_KD_EMPTY + 1)

template <int STATS, int KS = kKdStackEntries, bool SMALL = false>
__device__ __forceinline__ void kdPop(Ctx<STATS> &C, KdWalk &w, const int root, float *stackF, const KdNodeDev *nodes, const Ray &ray)
{
  const int count = w.pk.get(PK_SCOUNT);
  if (count > 0) {
    int head = w.pk.get(PK_SHEAD);
    head = head == 0 ? KS - 1 : head - 1;
    w.pk.set(PK_SHEAD, head);
    w.pk.dec(PK_SCOUNT);
    w.ref = C.stack[head * kKdBlock];
    w.tn = stackF[(2 * head) * kKdBlock];
    w.tf = stackF[(2 * head + 1) * kKdBlock];
  } else if (w.pk.get(PK_DROPPED) && w.tf < w.tEnd) {
    C.count(ST_RESTARTS);
    w.ref = root;                      // short-stack restart: everything before tf is done
    w.tn = w.tf;
    w.tf = w.tEnd;
    w.pk.set(PK_DROPPED, 0);
  } else {
    w.ref = EXA_KD_DONE;
  }
}

// The node stage of a step of the stack walk: one level down from the inner node w.ref.  `shift`: where the node's word holds
// the two activity bits the walk goes by (2 volume, 4 iso).
// There is no pop here: a node that leaves nothing to descend into marks the subtree EMPTY and the pop happens at the start of
// the lane's next call, in front of that call's node stage — the same sequence of subtrees, with one inlined copy of the pop
// instead of five for the wave's divergent lanes to run
template <int KS, bool SMALL, int STATS>
__device__ __forceinline__ void kdNodeStage(Ctx<STATS> &C, KdWalk &w, float *stackF, const Ray &ray, const KdNodeDev *nodes, const int shift)
{
  // SMALL: the node array is below 4 GiB — uniform base + 32-bit byte offset, no 64-bit address per lane
  const int4 n = SMALL ? *reinterpret_cast<const int4 *>(reinterpret_cast<const char *>(nodes) + ((uint32_t)w.ref << 4))
                       : *reinterpret_cast<const int4 *>(nodes + w.ref);
  C.count(ST_NODES);
  C.phase(ST_W_NODE);
  C.probeNode(w.ref);
  const float split = __int_as_float(n.x);
  const int axis = n.y & 3;
  const int bits = (n.y >> shift) & 3;                      // bit0 left active, bit1 right active
  // select on VALUES (copies first): selecting between struct members by address makes the
  // compiler index a scratch copy of the ray
  const float ox = ray.org.x, oy = ray.org.y, oz = ray.org.z, dx = ray.dir.x, dy = ray.dir.y, dz = ray.dir.z;
  float o = axis == 0 ? ox : oy, d = axis == 0 ? dx : dy;
  o = axis == 2 ? oz : o;
  d = axis == 2 ? dz : d;
  if (d == 0.f) {
    // parallel to the plane: only the side that strictly contains the origin can be hit
    // (boxTest turns lo==o / hi==o into a miss, exabrick.cu:201-208 with NaN-ignoring min/max)
    if (o < split && (bits & 1)) w.ref = n.z;
    else if (o > split && (bits & 2)) w.ref = n.w;
    else w.ref = EXA_KD_EMPTY;
    return;
  }
  const float ts = (split - o) / d;                         // same expression as the slab test
  const bool nearIsLeft = d > 0.f;
  const int nearRef = nearIsLeft ? n.z : n.w, farRef = nearIsLeft ? n.w : n.z;
  const bool nearAct = (bits & (nearIsLeft ? 1 : 2)) != 0, farAct = (bits & (nearIsLeft ? 2 : 1)) != 0;
  if (ts >= w.tf) {                                          // plane behind the interval: near side only
    w.ref = nearAct ? nearRef : EXA_KD_EMPTY;
  } else if (ts <= w.tn) {                                   // plane before the interval: far side only
    w.ref = farAct ? farRef : EXA_KD_EMPTY;
  } else if (nearAct) {
    if (farAct) {                                            // push far [ts,tf], go near [tn,ts]
      const int head = w.pk.get(PK_SHEAD), count = w.pk.get(PK_SCOUNT);
      C.stack[head * kKdBlock] = farRef;
      stackF[(2 * head) * kKdBlock] = ts;
      stackF[(2 * head + 1) * kKdBlock] = w.tf;
      w.pk.template incWrap<KS>(PK_SHEAD);
      if (count == KS) w.pk.setBit(PK_DROPPED); else w.pk.inc(PK_SCOUNT);
    }
    w.ref = nearRef;
    w.tf = ts;
  } else if (farAct) {
    w.ref = farRef;
    w.tn = ts;
  } else {
    w.ref = EXA_KD_EMPTY;
  }
}

// Per-lane queue of accepted segments (region, t0, t1) in LDS.  Which segments a ray
// gets depends only on the walk (each accepted leaf advances ray.tmin to t1*1.0000001f,
// exabrick.cu:1698), not on the march, so a lane may walk ahead of its march.  The walk
// therefore runs in wave-wide refill bursts — every lane with a free queue slot steps its
// own walk — instead of one or two lanes at a time whenever a lane's segment ends.

// one step of the walk: pop / descend one level / accept-or-skip a leaf
// ISOWALK: the iso march multiplies ray.tmax by dt_scale before every trace (exabrick.cu:1434), so the
// walk is not clamped at the root; the current tmax clamps t1 at the leaf and ends the walk.
// KS: entries of the lane's short stack (the multi-channel march runs with one fewer, see renderFrameKdKernel)
template <bool ISOWALK, int STATS, bool SMALL = false, int KS = kKdStackEntries>
__device__ __forceinline__ void kdStep(Ctx<STATS> &C, KdWalk &w, float &walkTmin, const RenderArgs &a,
                                       float *stackF, int *qRegion, float *qT, const Ray &ray, const int which,
                                       float &walkTmax, const float dtScale, const KdNodeDev *nodes, const int root)
{
  // A call runs up to three stages in a row — leaf, pop, node — so that a lane that has just
  // queued a leaf also takes the next node in the same call (the wave executes all three
  // stages for its divergent lanes anyway; fewer calls per burst).
  if (ISOWALK && w.ref != EXA_KD_EMPTY && !(w.tn < walkTmax)) { w.ref = EXA_KD_DONE; return; }   // everything left lies beyond tmax
  if (w.ref < 0 && w.ref > EXA_KD_DONE && w.tf > walkTmin) {
    // Leaf.  Its interval [w.tn, w.tf] is max/min over exactly the plane distances the
    // reference's slab test (exabrick.cu:197-210, 213-238) evaluates for this region's domain,
    // (plane-o)/d each: the faces are split planes of the path (or faces of the root box) and
    // the looser planes on the path cannot win a max/min.  No further division is needed; the
    // instrumented variant re-does the slab test and counts mismatches.
    const int region = ~w.ref;
    C.phase(ST_W_LEAF);
    const float t0 = fmaxf(walkTmin, w.tn);
    const float t1 = ISOWALK ? fminf(walkTmax, w.tf) : w.tf;
    const bool hit = t0 < t1;
    if (STATS == 1) {
      const float4 *rp = reinterpret_cast<const float4 *>(a.regionRec + region);
      const float4 r0 = rp[0], r1 = rp[1];
      Ray rr = ray; rr.tmin = walkTmin;
      if (ISOWALK) rr.tmax = walkTmax;
      float s0, s1;
      const bool shit = boxTest(rr, mk(r0.x, r0.y, r0.z), mk(r0.w, r1.x, r1.y), s0, s1);
      if (shit != hit || (hit && (s0 != t0 || s1 != t1))) C.st[ST_KD_MISMATCH]++;
    }
    if (hit) {
      const int qc = w.pk.get(PK_QCOUNT);
      int slot = w.pk.get(PK_QHEAD) + qc;
      slot = slot >= kSegQueue ? slot - kSegQueue : slot;
      qRegion[slot * kKdBlock] = region;
      qT[(2 * slot) * kKdBlock] = t0;
      qT[(2 * slot + 1) * kKdBlock] = t1;
      w.pk.inc(PK_QCOUNT);
      walkTmin = t1 * (1.0000001f);                          // exabrick.cu:1698 / :1457
      if (ISOWALK) walkTmax = walkTmax * dtScale;            // the next trace's tmax (:1434)
    }
    // A region that the trace's tmax cut short is not finished: the reference's intersection program reports the
    // CLAMPED exit (boxTest clamps to the ray's tmax, exabrick.cu:354-369), so the next trace starts just behind it and,
    // its tmax being dt_scale times larger (:1434), finds the rest of the same region.  Only a finite tmax with
    // dt_scale > 1 gets here (AO rays of finite length under a magnifying voxel-space transform); the leaf stays current
    // until a trace reaches its far face or finds nothing (dt_scale <= 1: t0 >= t1 next time).
    if (!(ISOWALK && hit && t1 < w.tf)) w.ref = EXA_KD_EMPTY;
  }
  if (w.ref == EXA_KD_EMPTY || (w.ref != EXA_KD_DONE && !(w.tf > walkTmin))) kdPop<STATS, KS, SMALL>(C, w, root, stackF, nodes, ray);
  // the popped subtree gets its own look at tmin / tmax in the next call
  if (w.ref < 0 || !(w.tf > walkTmin) || (ISOWALK && !(w.tn < walkTmax))) return;
  kdNodeStage<KS, SMALL, STATS>(C, w, stackF, ray, nodes, 2 + 2 * which);
}

// ------------------------------------------------------------------------
// Rope walk: the same ordered sequence of leaves without a stack.  Every leaf of the region kd-tree (and every empty
// child slot, a "gap") carries its box and, per face, a link to what lies across it (RopeLeaf; built by the module).  At a
// leaf the reference's slab test (exabrick.cu:197-210) is evaluated on the leaf's own box — the six (plane - o) / d the
// intersection program computes for this region, so [t0, t1] need no argument about the path — and the walk leaves
// through the face with the smallest exit distance.  A link may name an inner node (the neighbour across the face is
// split further): the walk then descends by the stack walk's own rule — the far child when the plane's distance is
// <= the distance at which the previous leaf was left, else the near child — so it reaches the leaf the stack walk
// pops next.  Space skipping cannot prune subtrees here (an inactive leaf is visited and passed through); the module
// uses this walk for frames in which most regions are active.
//
// The divisions: every quotient must be the correctly rounded (plane - o) / d.  With y = rcp(d) refined by one
// Newton step, q = a * y followed by two fma corrections IS the instruction sequence of the hardware's IEEE division
// (v_div_scale, v_rcp, 2 fma | mul, fma, fma, fma, v_div_fmas, v_div_fixup) minus its scaling and special-case steps;
// those do nothing when 2^-30 <= |d| <= 2 and a is 0 or 2^-60 <= |a| <= 2^60, which the caller establishes per wave
// (`fast`: direction and origin of every lane's ray, and the scene's planes, are in range); otherwise the plain division
// is used.  The counting variant re-does every leaf with the plain division and counts mismatches.
// ------------------------------------------------------------------------
__device__ __forceinline__ float refinedRcp(float d)
{
  const float y = __builtin_amdgcn_rcpf(d);
  return __builtin_fmaf(__builtin_fmaf(-d, y, 1.f), y, y);
}
__device__ __forceinline__ float divByRcp(float a, float d, float y)
{
  float q = a * y;
  float r = __builtin_fmaf(-d, q, a);
  q = __builtin_fmaf(r, y, q);
  r = __builtin_fmaf(-d, q, a);
  return __builtin_fmaf(r, y, q);
}
// is this ray's origin / direction in the range of the short division (see above; planes are checked by the module)
__device__ __forceinline__ bool ropeRayInRange(const Ray &ray)
{
  bool ok = true;
  const float dd[3] = { ray.dir.x, ray.dir.y, ray.dir.z }, oo[3] = { ray.org.x, ray.org.y, ray.org.z };
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const float ad = fabsf(dd[k]), ao = fabsf(oo[k]);
    ok = ok && ad >= 9.31322574615478515625e-10f /* 2^-30 */ && ad <= 2.f
            && (ao == 0.f || (ao >= 9.5367431640625e-07f /* 2^-20 */ && ao <= 1099511627776.f /* 2^40 */));
  }
  return ok;
}

// one step of the rope walk: the leaf stage (slab test, accept, leave through the exit face) and then, for a lane whose
// link names an inner node, one level of the descent — so that a lane that has just taken a link also takes the next node
// in the same call, as kdStep does.  QN: entries of the lane's segment queue.
// (The source forms the refined reciprocals at every step; the compiler hoists them out of the march loop into three registers
// where the register budget allows — the 80-register variants — and LEAN keeps it from doing so.)
template <int STATS, bool SMALL, int QN, bool LEAN, int PACKED_CT /* 1 / 0: known when compiled, -1: a.leafBeginBits says */>
__device__ __forceinline__ void ropeStep(Ctx<STATS> &C, KdWalk &w, float &walkTmin, const RenderArgs &a, float4 *queue,
                                         const Ray &ray, const bool fast, const float samplingOffset)
{
  const float ox = ray.org.x, oy = ray.org.y, oz = ray.org.z, dx = ray.dir.x, dy = ray.dir.y, dz = ray.dir.z;
  const bool PACKED = PACKED_CT < 0 ? a.leafBeginBits != 0 : PACKED_CT != 0;
  if (w.ref < 0 && w.ref != EXA_KD_DONE) {
    C.phase(ST_W_LEAF);
    C.count(ST_NODES, 4);
    C.count(ST_ROPE_LEAVES);
    const uint32_t leaf = (uint32_t)~w.ref;
    const char *lp = SMALL ? reinterpret_cast<const char *>(a.ropeLeaves) + (leaf << 6)
                           : reinterpret_cast<const char *>(a.ropeLeaves + leaf);
    const float4 q0 = *reinterpret_cast<const float4 *>(lp), q1 = *reinterpret_cast<const float4 *>(lp + 16);
    const int4 r2 = *reinterpret_cast<const int4 *>(lp + 32), r3 = *reinterpret_cast<const int4 *>(lp + 48);
    // exabrick.cu:197-210 on this leaf's box (lo = q0.xyz, hi = q0.w, q1.xy)
    float lx, hx, ly, hy, lz, hz;
    if (fast) {
      const V3 rcpDir = LEAN ? mk(refinedRcp(opaque(dx)), refinedRcp(opaque(dy)), refinedRcp(opaque(dz)))
                                 : mk(refinedRcp(dx), refinedRcp(dy), refinedRcp(dz));
      lx = divByRcp(q0.x - ox, dx, rcpDir.x); hx = divByRcp(q0.w - ox, dx, rcpDir.x);
      ly = divByRcp(q0.y - oy, dy, rcpDir.y); hy = divByRcp(q1.x - oy, dy, rcpDir.y);
      lz = divByRcp(q0.z - oz, dz, rcpDir.z); hz = divByRcp(q1.y - oz, dz, rcpDir.z);
    } else {
      lx = (q0.x - ox) / dx; hx = (q0.w - ox) / dx;
      ly = (q0.y - oy) / dy; hy = (q1.x - oy) / dy;
      lz = (q0.z - oz) / dz; hz = (q1.y - oz) / dz;
    }
    const float nx = fminf(lx, hx), ny = fminf(ly, hy), nz = fminf(lz, hz);
    const float fx = fmaxf(lx, hx), fy = fmaxf(ly, hy), fz = fmaxf(lz, hz);
    const float tOut = fminf(fminf(fx, fy), fz);                 // where the ray leaves the box (not clamped)
    const float t0 = fmaxf(walkTmin, fmaxf(fmaxf(nx, ny), nz));
    const float t1 = fminf(w.tEnd, tOut);                        // tEnd = min(ray.tmax, exit of the root box) >= every leaf's clamp
    const bool active = (__float_as_uint(q1.w) & 1u) != 0u;
    const bool hit = active && t0 < t1;
    if (STATS == 1) {
      // the plain slab test of the intersection program with the current ray.tmin (and the plain division)
      Ray rr = ray; rr.tmin = walkTmin;
      float s0, s1;
      const bool slabHit = boxTest(rr, mk(q0.x, q0.y, q0.z), mk(q0.w, q1.x, q1.y), s0, s1);
      if ((slabHit && active) != hit || (hit && (s0 != t0 || s1 != t1))) C.st[ST_KD_MISMATCH]++;
    }
    if (hit) {
      const int qc = w.pk.get(PK_QCOUNT);
      int slot = w.pk.get(PK_QHEAD) + qc;
      slot = slot >= QN ? slot - QN : slot;
      // One 16-byte queue entry: what the march needs of the region — its packed record (the march tree's leaf reference),
      // or the region id when the scene's records do not pack —, the segment [t0, t1], and the first sample's t_i
      // (exabrick.cu:1141-1144), which is worked out HERE, where most lanes of the wave are busy, instead of at the pop,
      // which runs in nearly every march iteration for a handful of lanes
      float t_i = 0.f;
      if (PACKED) {
        const uint32_t level = __float_as_uint(q1.z) >> (a.leafBeginBits + a.leafSizeBits);
        const float flcw = __int_as_float((127 + (int)level) << 23);                       // 2^level
        if (a.invDtPow2 != 0.f) t_i = firstSampleTPow2(t0, a.p.dt * flcw, a.invDtPow2 * __int_as_float((127 - (int)level) << 23), samplingOffset);
        else t_i = firstSampleT(t0, a.p.dt * flcw, samplingOffset);
      }
      queue[slot * kKdBlock] = make_float4(PACKED ? q1.z : __int_as_float(r3.z), t1, t_i, t0);
      w.pk.inc(PK_QCOUNT);
      walkTmin = t1 * (1.0000001f);                              // exabrick.cu:1698
    }
    // leave through the face with the smallest exit distance (the first axis in a tie: the leaf behind a face the ray
    // only touches has an empty interval and is passed through)
    const int linkX = dx > 0.f ? r2.y : r2.x, linkY = dy > 0.f ? r2.w : r2.z, linkZ = dz > 0.f ? r3.y : r3.x;
    const int link = fx == tOut ? linkX : (fy == tOut ? linkY : linkZ);
    w.tn = tOut;
    w.ref = tOut < w.tEnd ? link : EXA_KD_DONE;                  // nothing behind tEnd can be hit (a NaN ray ends here as well)
  }
  if (w.ref >= 0) {
    const int4 n = SMALL ? *reinterpret_cast<const int4 *>(reinterpret_cast<const char *>(a.ropeNodes) + ((uint32_t)w.ref << 4))
                         : *reinterpret_cast<const int4 *>(a.ropeNodes + w.ref);
    C.count(ST_NODES);
    C.phase(ST_W_NODE);
    C.probeNode(w.ref);
    const float split = __int_as_float(n.x);
    const int axis = n.y & 3;
    float o = axis == 0 ? ox : oy, d = axis == 0 ? dx : dy;
    o = axis == 2 ? oz : o;
    d = axis == 2 ? dz : d;
    bool goRight;                                                // right = upper side of the plane
    if (fast) {
      const float ts = divByRcp(split - o, d, refinedRcp(LEAN ? opaque(d) : d));
      goRight = (ts <= w.tn) == (d > 0.f);                       // far child when the plane lies at or before the entry distance
    } else if (d == 0.f) {
      goRight = !(o < split);                                    // parallel to the plane: the side that holds the origin
    } else {
      const float ts = (split - o) / d;
      goRight = (ts <= w.tn) == (d > 0.f);
    }
    w.ref = goRight ? n.w : n.z;
  }
}

// exabrick.cu:1408-1460 traceIsoRay on the kd walk (iso activity bits): segments come out of the
// ordered walk, one lane at a time refills its own queue here (the iso pre-pass is not the
// headline path), the march is isoIntegrateBrick.
template <int STATS>
__device__ SurfaceHit traceIsoRayKd(Ctx<STATS> &C, Ray ray, float off, float *stackF, int *qRegion, float *qT, const bool hitOnly = false)
{
  const RenderArgs &a = *C.a;
  const ExaHipFrameState &fs = a.fs;
  const float dt_scale = toVoxelSpace(fs, ray);                 // :1416-1420
  float walkTmin = dt_scale * ray.tmin;
  float walkTmax = ray.tmax * dt_scale;                      // tmax of the first trace (:1434)
  IsoLast last;
  last.init(fs);
  SurfaceHit result;
  result.primID = -1; result.t_hit = ray.tmax; result.Ng = mk(0.f, 0.f, 0.f);
  result.ambient = 0.f; result.baseColor = mk(0.f, 0.f, 0.f);
  KdWalk w;
  w.pk.v = 0;
  {
    Ray whole = ray; whole.tmin = -INFINITY; whole.tmax = INFINITY;
    float r0, r1;
    const bool hit = boxTest(whole, mk(a.kdLo), mk(a.kdHi), r0, r1);
    w.tn = fmaxf(r0, walkTmin);
    w.tf = r1;
    w.tEnd = r1;
    w.ref = (hit && w.tn < w.tf) ? a.kdIsoRoot : EXA_KD_DONE;
  }
  for (int seg = 0;; seg++) {
    if (seg >= (1 << 22)) { C.guardTripped = true; break; }
    // wave-wide refill burst, as in the DVR loop: when one lane has run dry every lane still in this
    // loop advances its own walk while it has a free queue slot
    if (anyLane(w.pk.get(PK_QCOUNT) == 0 && w.ref != EXA_KD_DONE)) {
      for (int g = 0;; g++) {
        if (g >= (1 << 24)) { C.guardTripped = true; w.ref = EXA_KD_DONE; break; }
        const bool want = w.pk.get(PK_QCOUNT) < kSegQueue && w.ref != EXA_KD_DONE;
        if (want) kdStep<true>(C, w, walkTmin, a, stackF, qRegion, qT, ray, 1, walkTmax, dt_scale, a.kdNodes, a.kdIsoRoot);
        if (!anyLane(w.pk.get(PK_QCOUNT) == 0 && w.ref != EXA_KD_DONE)) break;     // no lane is dry any more
      }
    }
    const int qc = w.pk.get(PK_QCOUNT);
    if (qc == 0) break;
    const int qh = w.pk.get(PK_QHEAD);
    const int region = qRegion[qh * kKdBlock];
    const float t0 = qT[(2 * qh) * kKdBlock], t1 = qT[(2 * qh + 1) * kKdBlock];
    w.pk.template incWrap<kSegQueue>(PK_QHEAD);
    w.pk.dec(PK_QCOUNT);
    C.count(ST_ISO_SEGMENTS);
    const RegionInfo ri = a.sc.regionInfo[region];
    IsoResult ir;
    ir.pixelColor.x = ir.pixelColor.y = ir.pixelColor.z = ir.pixelColor.w = 0.f;
    ir.t_hit = -1.f; ir.gradient = mk(0.f, 0.f, 0.f);
    isoIntegrateBrick(C, last, ir, off, ray, ri, t0, t1, a.p.numPrimaryChannels, hitOnly);
    if (ir.t_hit >= 0.f) {
      result.primID = EXA_PRIMID_ISOSURFACE;
      result.t_hit = ir.t_hit / dt_scale;
      result.Ng = normalize(ir.gradient);
      result.ambient = 0.f;
      result.baseColor = mk(ir.pixelColor.x, ir.pixelColor.y, ir.pixelColor.z);
      return result;
    }
  }
  return result;
}

// samplePointWithInfRay's degenerate trace on the kd walk: first accepted leaf of the ray
// (pos, (1,1,1), [0, 2e-10]) under the volume activity bits
template <int STATS>
__device__ int kdFindRegion(Ctx<STATS> &C, V3 pos, float *stackF, int *qRegion, float *qT)
{
  const RenderArgs &a = *C.a;
  Ray ray; ray.org = pos; ray.dir = mk(1.f, 1.f, 1.f); ray.tmin = 0.f; ray.tmax = 2e-10f;
  KdWalk w;
  w.pk.v = 0;
  Ray whole = ray; whole.tmin = -INFINITY; whole.tmax = INFINITY;
  float r0, r1;
  const bool hit = boxTest(whole, mk(a.kdLo), mk(a.kdHi), r0, r1);
  w.tn = fmaxf(r0, ray.tmin);
  w.tf = fminf(r1, ray.tmax);
  w.tEnd = w.tf;
  w.ref = (hit && w.tn < w.tf) ? a.kdRoot : EXA_KD_DONE;
  float walkTmin = ray.tmin;
  for (int g = 0; w.pk.get(PK_QCOUNT) == 0 && w.ref != EXA_KD_DONE; g++) {
    if (g >= (1 << 24)) { C.guardTripped = true; break; }
    kdStep<false>(C, w, walkTmin, a, stackF, qRegion, qT, ray, 0, walkTmin, 1.f, a.kdNodes, a.kdRoot);
  }
  return w.pk.get(PK_QCOUNT) ? qRegion[w.pk.get(PK_QHEAD) * kKdBlock] : -1;
}

// ISO_ONLY: the frame has no triangle meshes, contour planes or streamlines (the launcher checks): their code is left out
template <int STATS, bool ISO_ONLY>
__device__ __forceinline__ void traceSurfacesKd(Ctx<STATS> &C, const Ray &ray, SurfaceHit &prd, bool withContourPlanes,
                                                float *stackF, int *qRegion, float *qT)
{
  prd.primID = -1;
  prd.t_hit = ray.tmax;
  prd.Ng = mk(0.f, 0.f, 0.f); prd.ambient = 0.f; prd.baseColor = mk(0.f, 0.f, 0.f);
  if (!ISO_ONLY && C.a->numTris > 0) traceMeshes(C, ray, prd);                 // ST_MESHES (also for AO rays)
  if (!ISO_ONLY && withContourPlanes) {
    for (int i = 0; i < EXA_MAX_CONTOUR_PLANES; ++i)
      if (C.a->fs.contour[i].enabled) {
        auto find = [&](V3 pos) { return kdFindRegion(C, pos, stackF, qRegion, qT); };
        const SurfaceHit c = traceContourRay(C, ray, mk(C.a->fs.contour[i].normal), C.a->fs.contour[i].offset,
                                             C.a->fs.contour[i].channel, find);
        if (c.primID == EXA_PRIMID_PLANE && c.t_hit < prd.t_hit) prd = c;
      }
  }
  if (!ISO_ONLY && C.a->numStreamPrims > 0) traceStreamlines(C, ray, prd);     // ST_STREAMLINES (:1503-1512)
  bool activeIso = false;
  for (int i = 0; i < EXA_MAX_ISO_SURFACES; i++) activeIso |= (C.a->fs.iso[i].enabled != 0);
  if (activeIso) {
    // the rays traced without contour planes are the ambient-occlusion rays (:1638): only hit / no hit is read
    const SurfaceHit isoPRD = traceIsoRayKd(C, ray, 0.f, stackF, qRegion, qT, !withContourPlanes);
    if (isoPRD.primID == EXA_PRIMID_ISOSURFACE && isoPRD.t_hit < prd.t_hit) prd = isoPRD;
  }
}

// ------------------------------------------------------------------------
// Surfaces pre-pass (exabrick.cu:1601-1652): triangle meshes, contour planes, streamlines and the
// implicit iso-surface march, shading and AO rays.  Runs as its own launch in front of the volume
// march when a frame has surfaces, and hands {background colour, surface t_hit} and the LCG state
// to it through a[].surf / surfRnd: the generic surface code needs ~130 VGPRs, the march 80, and one
// fused kernel would run the march at half its occupancy.
// ------------------------------------------------------------------------
// AO_DEFER: the ambient-occlusion rays of a shaded hit (:1611-1645) are not traced here, lane by lane behind the primary
// ray with the lanes that hit nothing waiting, but handed to aoRaysKdKernel below as a compact list (one record per shaded
// hit, appended with one atomic per wave): there every lane traces one AO ray.  Same rays, same random numbers, same
// pixel arithmetic; only which lane of which launch traces a ray changes.  (The counting variant keeps them inline.)
template <int STATS, bool ISO_ONLY, bool AO_DEFER>
__global__ __launch_bounds__(kKdBlock, (ISO_ONLY ? EXA_PREPASS_ISO_WAVES : EXA_PREPASS_WAVES)) void surfacePrepassKdKernel(const RenderArgs a)
{
  static_assert(ldsFits(kdLds(1), ISO_ONLY ? EXA_PREPASS_ISO_WAVES : EXA_PREPASS_WAVES), "LDS per workgroup x waves per SIMD exceeds the CU's 160 KB");
  const LdsPtrs lds = carveLds(kdLds(a.numXfChannels));
  Ctx<STATS> C;
  kernelPrologue(C, a, lds);
  float *stackF = lds.stackF, *qT = lds.qT;
  int *qRegion = lds.qRegion;
  // The counting variant keeps the literal sampler: for the NaN positions the iso march produces where a field equals the
  // iso value over a whole step (tavg = 0/0, exabrick.cu:1047-1053; the reference's NaN guard is at :1088) the two
  // forms clamp the cell index differently (int(NaN) = 0 vs max(NaN, -1) = -1), which changes nothing in the sums
  // (NaN either way) but counts other cells as "read".
  C.fastSampler = a.fastSampler != 0 && STATS != 1;
  if (STATS) for (int i = 0; i < ST_COUNT; i++) C.st[i] = 0;
  // a workgroup is kKdBlock/64 waves; each wave renders one 8x8 block of a 16x16 tile
  const int wavesPerBlock = kKdBlock / 64;
  const int gwave = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6);
  const int tile = a.tileMap[gwave >> 2];
  const int tx = tile % a.tilesX, ty = tile / a.tilesX;
  const int wave = gwave & 3, lane = threadIdx.x & 63;
  const int inX = ((wave & 1) << 3) + laneX(lane), inY = ((wave >> 1) << 3) + laneY(lane);
  const int px = tx * kTile + inX, py = ty * kTile + inY;
  const bool inside = px < a.W && py < a.H && (a.debugPixel < 0 || a.debugPixel == px + a.W * py);

  if (inside) {
    const ExaHipFrameState &fs = a.fs;
    Lcg rnd;
    const Ray ray = cameraRay(a, px, py, rnd);
    // ---- surfaces first: implicit iso-surface hit, AO rays, background colour (:1601-1652) ----
    V3 bgColor = mk(0.f, 0.f, 0.f);
    float surface_t_hit = ray.tmax;
    bool deferAo = false;
    AoRecord rec;
    {
      SurfaceHit surface;
      traceSurfacesKd<STATS, ISO_ONLY>(C, ray, surface, true, stackF, qRegion, qT);
      surface_t_hit = surface.t_hit;
      if (surface.primID >= 0 || surface.primID == EXA_PRIMID_ISOSURFACE || surface.primID == EXA_PRIMID_PLANE
          || surface.primID == EXA_PRIMID_STREAMLINE) {
        const bool shade = surface.primID >= 0 || surface.primID == EXA_PRIMID_PLANE || surface.primID == EXA_PRIMID_STREAMLINE
                        || (surface.primID == EXA_PRIMID_ISOSURFACE && a.p.gradientShadingISO);
        if (AO_DEFER && shade && length(surface.Ng) > 0.f && fs.ao.enabled) {
          // record for aoRaysKdKernel: hit point, |cos| of the primary ray, normal, colour, and the LCG state from which
          // the two samples draw (u1, u2 each, :1624-1625); this pixel's state moves past those four draws
          const V3 isect_pos = ray.org + surface.t_hit * ray.dir;
          rec.posFd = make_float4(isect_pos.x, isect_pos.y, isect_pos.z, fabsf(dot(ray.dir, surface.Ng)));
          rec.ngAmb = make_float4(surface.Ng.x, surface.Ng.y, surface.Ng.z, surface.ambient);
          rec.baseRnd = make_float4(surface.baseColor.x, surface.baseColor.y, surface.baseColor.z, __uint_as_float(rnd.state));
          rnd.next(); rnd.next(); rnd.next(); rnd.next();
          deferAo = true;
        } else if (shade && length(surface.Ng) > 0.f) {
          const float AO_Radius = fs.ao.length;
          const int AO_Samples = (!AO_DEFER && fs.ao.enabled) ? 2 : 0;     // AO_DEFER: only hits without AO get here
          const V3 isect_pos = ray.org + surface.t_hit * ray.dir;
          const V3 wN = surface.Ng;
          const V3 vN = fabsf(wN.x) > fabsf(wN.y) ? normalize(mk(-wN.z, 0.f, wN.x)) : normalize(mk(0.f, wN.z, -wN.y));
          const V3 uN = cross(vN, wN);
          int hitCnt = 0;
          for (int i = 0; i < AO_Samples; ++i) {
            const float u1 = rnd.next(), u2 = rnd.next();
            const float r = sqrtf(u1);
            const float theta = 2.f * 3.14159265358979323846f * u2;
            const V3 sp = mk(r * cosf(theta), r * sinf(theta), sqrtf(1.f - u1));
            Ray ao_ray;
            ao_ray.org = isect_pos;
            ao_ray.dir = normalize((sp.x * uN + sp.y * vN) + sp.z * wN);
            ao_ray.tmin = 1e-4f; ao_ray.tmax = AO_Radius;
            SurfaceHit ao;
            traceSurfacesKd<STATS, ISO_ONLY>(C, ao_ray, ao, false, stackF, qRegion, qT);
            if (ao.primID >= 0 || ao.primID == EXA_PRIMID_ISOSURFACE || ao.primID == EXA_PRIMID_PLANE
                || ao.primID == EXA_PRIMID_STREAMLINE) hitCnt++;
          }
          const float shadow = (!AO_DEFER && fs.ao.enabled) ? (float)hitCnt / AO_Samples : 0.f;
          const float fd = fabsf(dot(ray.dir, surface.Ng));
          const float ns = 1.f - shadow;
          bgColor = mk(surface.ambient + surface.baseColor.x * fd * ns,
                       surface.ambient + surface.baseColor.y * fd * ns,
                       surface.ambient + surface.baseColor.z * fd * ns);
        } else {
          bgColor = surface.baseColor;
        }
      }
    }
    const size_t slot = slotOf(a, tile, inX, inY, px, py);
    a.surf[slot] = make_float4(bgColor.x, bgColor.y, bgColor.z, surface_t_hit);
    a.surfRnd[slot] = rnd.state;
    if (AO_DEFER) {
      // append: one atomicAdd per wave (ballot + prefix count), 64 B per record
      const unsigned long long m = __ballot(deferAo);
      if (m) {
        const int lane_ = threadIdx.x & 63;
        const int leader = __ffsll((long long)m) - 1;
        unsigned base = 0;
        if (lane_ == leader) base = atomicAdd(a.aoCount, (unsigned)__popcll(m));
        base = (unsigned)__shfl((int)base, leader, 64);
        if (deferAo) {
          rec.slot = (uint32_t)slot; rec.pad0 = rec.pad1 = rec.pad2 = 0;
          a.aoRecs[base + (unsigned)__popcll(m & ((1ull << lane_) - 1ull))] = rec;
        }
      }
    }
  }

  if (a.tileCostPre) {
    // launch plan: the longest iso march of this tile, in steps (the pre-pass is bound by its longest rays)
    unsigned v = inside ? C.isoSteps : 0u;
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_down((int)v, off, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(&a.tileCostPre[tile], v);
  }
  if (C.guardTripped) atomicExch(a.errorFlag, 1);
  if (STATS) {
    for (int i = 0; i < ST_COUNT; i++) {
      unsigned long long v = inside ? C.st[i] : 0ull;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.stats[i], v);
    }
  }
}

// AO ray j of the deferred list: sample j & 1 of hit j >> 1 — the cosine-distributed direction from the hit's own LCG draws
// (exabrick.cu:85-94, 1624-1633).  One definition for the tracing kernel and for the kernel that sorts the rays.
__device__ __forceinline__ Ray aoRayOf(const ExaHipFrameState &fs, const float4 posFd, const float4 ngAmb, const float4 baseRnd, unsigned j)
{
  Lcg rnd;
  rnd.state = __float_as_uint(baseRnd.w);
  if (j & 1u) { rnd.next(); rnd.next(); }                       // the second sample's draws follow the first's
  const V3 wN = mk(ngAmb.x, ngAmb.y, ngAmb.z);
  const V3 vN = fabsf(wN.x) > fabsf(wN.y) ? normalize(mk(-wN.z, 0.f, wN.x)) : normalize(mk(0.f, wN.z, -wN.y));
  const V3 uN = cross(vN, wN);
  const float u1 = rnd.next(), u2 = rnd.next();
  const float rr = sqrtf(u1);
  const float theta = 2.f * 3.14159265358979323846f * u2;
  const V3 sp = mk(rr * cosf(theta), rr * sinf(theta), sqrtf(1.f - u1));
  Ray ao_ray;
  ao_ray.org = mk(posFd.x, posFd.y, posFd.z);
  ao_ray.dir = normalize((sp.x * uN + sp.y * vN) + sp.z * wN);
  ao_ray.tmin = 1e-4f; ao_ray.tmax = fs.ao.length;
  return ao_ray;
}

// ---- sorting the deferred AO rays (option ao_defer = 2) ----
// The hits are listed in launch order of the pre-pass, two rays per hit in random directions of the hit's hemisphere: the 64
// rays of a wave start close together and fly apart.  A counting sort by (32x32-pixel block of the hit | direction class)
// puts rays that start close together AND head the same way into the same waves: key kernel (histogram) -> scan -> scatter
// of the ray indices; the tracing kernel then takes its chunks from the sorted index list and writes one hit flag per ray,
// and a last kernel combines the two flags of a hit.  Which lane traces a ray does not change the ray: same pixels.
enum { kAoDirClasses = 24, kAoCellShift = 5 };
__device__ __forceinline__ uint32_t aoRayKey(const RenderArgs &a, uint32_t slot, V3 d)
{
  // direction class: octant (3 sign bits) x dominant axis
  const float ax = fabsf(d.x), ay = fabsf(d.y), az = fabsf(d.z);
  const uint32_t dom = (ax >= ay && ax >= az) ? 0u : (ay >= az ? 1u : 2u);
  const uint32_t oct = (d.x < 0.f ? 1u : 0u) | (d.y < 0.f ? 2u : 0u) | (d.z < 0.f ? 4u : 0u);
  // where the hit's pixel lies: 32x32-pixel blocks of the frame (one GPU), or groups of four of this rank's tiles
  uint32_t cell;
  if (a.world == 1) {
    const uint32_t px = slot % (uint32_t)a.W, py = slot / (uint32_t)a.W;
    cell = (py >> kAoCellShift) * (((uint32_t)a.W + 31u) >> kAoCellShift) + (px >> kAoCellShift);
  } else {
    cell = slot >> 10;
  }
  return cell * kAoDirClasses + oct * 3u + dom;
}
#if !EXA_TU_ROPE
__global__ __launch_bounds__(256) void aoKeyKernel(const RenderArgs a)
{
  const unsigned numRays = 2u * a.aoCount[0];
  for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < numRays; j += gridDim.x * 256u) {
    const AoRecord *r = a.aoRecs + (j >> 1);
    const Ray ray = aoRayOf(a.fs, r->posFd, r->ngAmb, r->baseRnd, j);
    const uint32_t key = min(aoRayKey(a, r->slot, ray.dir), a.aoBins - 1u);
    a.aoKeys[j] = key;
    atomicAdd(&a.aoHist[key], 1u);
  }
}
// exclusive prefix sum of the histogram, in place: one workgroup, each thread a contiguous run of bins
__global__ __launch_bounds__(1024) void aoScanKernel(uint32_t *hist, uint32_t numBins)
{
  __shared__ uint32_t part[1024];
  const uint32_t per = (numBins + 1023u) / 1024u;
  const uint32_t b0 = min(threadIdx.x * per, numBins), b1 = min(b0 + per, numBins);
  uint32_t sum = 0;
  for (uint32_t b = b0; b < b1; b++) sum += hist[b];
  part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {
    const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
    __syncthreads();
    part[threadIdx.x] += v;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - sum;                      // exclusive prefix of this thread's run
  for (uint32_t b = b0; b < b1; b++) { const uint32_t c = hist[b]; hist[b] = run; run += c; }
}
__global__ __launch_bounds__(256) void aoScatterKernel(const RenderArgs a)
{
  const unsigned numRays = 2u * a.aoCount[0];
  for (unsigned j = blockIdx.x * 256u + threadIdx.x; j < numRays; j += gridDim.x * 256u)
    a.aoOrder[atomicAdd(&a.aoHist[a.aoKeys[j]], 1u)] = j;       // the scanned histogram doubles as the bins' cursors
}
// shadow term and background colour of every listed hit from its two rays' flags (exabrick.cu:1647-1650)
__global__ __launch_bounds__(256) void aoFinalizeKernel(const RenderArgs a)
{
  const unsigned numHits = a.aoCount[0];
  for (unsigned h = blockIdx.x * 256u + threadIdx.x; h < numHits; h += gridDim.x * 256u) {
    const AoRecord *r = a.aoRecs + h;
    const float4 posFd = r->posFd, ngAmb = r->ngAmb, baseRnd = r->baseRnd;
    const uint32_t slot = r->slot;
    const int hitCnt = (int)a.aoHit[2u * h] + (int)a.aoHit[2u * h + 1u];
    const float shadow = (float)hitCnt / 2;                         // AO_Samples = 2 (:1613)
    const float fd = posFd.w;
    const float ns = 1.f - shadow;
    const float t_hit = a.surf[slot].w;
    a.surf[slot] = make_float4(ngAmb.w + baseRnd.x * fd * ns, ngAmb.w + baseRnd.y * fd * ns, ngAmb.w + baseRnd.z * fd * ns, t_hit);
  }
}

#endif // !EXA_TU_ROPE

// The ambient-occlusion rays of the hits surfacePrepassKdKernel<.., AO_DEFER> listed (exabrick.cu:1611-1652): lane 2h + i
// traces sample i of hit h — the cosine-distributed direction from the hit's own LCG draws (:85-94, :1624-1633), the trace
// through the surfaces without contour planes (:1638), hit or no hit — and the two lanes of a hit combine into the shadow
// term and the hit's background colour (:1647-1650), which replaces the placeholder in a.surf.
// SORTED: the chunks come from the sorted index list a.aoOrder and every ray writes its flag to a.aoHit (aoFinalizeKernel
// combines them); otherwise lanes 2h, 2h + 1 hold the two rays of hit h and combine them with one shuffle.
template <bool ISO_ONLY, bool SORTED>
__global__ __launch_bounds__(kKdBlock, (ISO_ONLY ? EXA_AO_ISO_WAVES : EXA_PREPASS_WAVES)) void aoRaysKdKernel(const RenderArgs a)
{
  static_assert(ldsFits(kdLds(1), ISO_ONLY ? EXA_AO_ISO_WAVES : EXA_PREPASS_WAVES), "LDS per workgroup x waves per SIMD exceeds the CU's 160 KB");
  const LdsPtrs lds = carveLds(kdLds(a.numXfChannels));
  Ctx<0> C;
  kernelPrologue(C, a, lds);
  float *stackF = lds.stackF, *qT = lds.qT;
  int *qRegion = lds.qRegion;
  C.fastSampler = a.fastSampler != 0;
  const ExaHipFrameState &fs = a.fs;
  const unsigned numRays = 2u * a.aoCount[0];
  // The list's length is only known on the device: a grid of resident waves takes chunks of 64 rays from a shared
  // counter (a.aoCount[2], cleared with the list) until the list is used up — rays differ in length by orders of magnitude,
  // a static split leaves most of the grid waiting for its slowest part.  Every wave ends: the counter only grows.
  for (;;) {
    unsigned base = 0;
    if ((threadIdx.x & 63) == 0) base = atomicAdd(&a.aoCount[2], 64u);
    base = (unsigned)__shfl((int)base, 0, 64);
    if (base >= numRays) break;
    const unsigned k = base + (threadIdx.x & 63);
    const bool live = k < numRays;
    const unsigned j = (SORTED && live) ? a.aoOrder[k] : k;
    int hitFlag = 0;
    float4 posFd = make_float4(0.f, 0.f, 0.f, 0.f), ngAmb = posFd, baseRnd = posFd;
    uint32_t slot = 0;
    if (live) {
      const AoRecord *r = a.aoRecs + (j >> 1);
      posFd = r->posFd; ngAmb = r->ngAmb; baseRnd = r->baseRnd; slot = r->slot;
      const Ray ao_ray = aoRayOf(fs, posFd, ngAmb, baseRnd, j);
      SurfaceHit ao;
      traceSurfacesKd<0, ISO_ONLY>(C, ao_ray, ao, false, stackF, qRegion, qT);
      if (ao.primID >= 0 || ao.primID == EXA_PRIMID_ISOSURFACE || ao.primID == EXA_PRIMID_PLANE
          || ao.primID == EXA_PRIMID_STREAMLINE) hitFlag = 1;
      if (SORTED) a.aoHit[j] = (uint8_t)hitFlag;
    }
    if (SORTED) continue;
    const int other = __shfl_xor(hitFlag, 1, 64);                    // the hit's other sample: the neighbouring lane
    if (live && !(j & 1u)) {
      const int hitCnt = hitFlag + other;
      const float shadow = (float)hitCnt / 2;                         // AO_Samples = 2 (:1613)
      const float fd = posFd.w;
      const float ns = 1.f - shadow;
      const float t_hit = a.surf[slot].w;
      a.surf[slot] = make_float4(ngAmb.w + baseRnd.x * fd * ns, ngAmb.w + baseRnd.y * fd * ns, ngAmb.w + baseRnd.z * fd * ns, t_hit);
    }
  }
  if (C.guardTripped) atomicExch(a.errorFlag, 1);
}

// MULTI: 0 = one primary channel; 1 = several, at most two TF tables in LDS (the 6-workgroup layout below); 2 = several, more tables
// NCH: 0 = cell values field by field (the ABI's layout; one channel, or the channels one after the other);
//      2..4 = that many primary channels from the channel-interleaved copy, all of them per brick visit (addBasisFastIl);
//      1 = one primary channel field by field as with 0, in a cube scene: the brick records are the 16-byte cube records
//          (a.leafHdrCube, exa_cube.h; addBasisFast<.., CUBE>) and a lane keeps one int4 of the current record instead of two.
//          MULTI == 0, ROPE, SMALL, not instrumented, form 1.  (A value of this parameter and not a parameter of its own: the
//          variants are known to the profiling tools and the resource tests by this parameter list.)
// ROPE: the walk is the rope walk (ropeStep) instead of the stack walk (kdStep); everything behind the segment queue is the same
// waves per SIMD a variant of the march is compiled for.  Seven for the one-channel rope march (72 registers, no scratch; a
// queue of five entries lets seven workgroups share a CU's LDS): C4 17.28 -> 17.08 ms, inside camera 22.60 -> 22.01, C5 1075 ->
// 1068 ms per 16 samples.  Not for the instrumented variants and the source-order sums (form 0: more values in flight per
// visit — the pixel's colour would live in scratch), nor for fields beyond 4 GiB (SMALL = false: no scratch either, but that
// frame is heavy on HBM traffic already and a seventh wave costs it 2 %: 26.47 -> 27.04 ms).
constexpr int marchWaves(int MULTI, int STATS, bool SMALL, int NCH, bool ROPE)
{
  return NCH > 1 ? (NCH == 2 ? EXA_IL2_WAVES : EXA_IL34_WAVES)
             : (MULTI == 1 ? EXA_MULTI_WAVES
                           : (MULTI ? 5 : ((ROPE && !STATS && SMALL && EXA_BASIS_FORM == 1) ? EXA_ROPE_WAVES : EXA_MARCH_WAVES)));
}

template <bool GRAD, bool FAST, int MULTI, bool SURF, int STATS, bool SMALL, int NCH = 0, bool ROPE = false>
__global__ __launch_bounds__(kKdBlock, marchWaves(MULTI, STATS, SMALL, NCH, ROPE)) void renderFrameKdKernel(const RenderArgs a)
{
  // the template's NCH: 1 = the cube records, one channel; IL = the channels of the interleaved march (0: field by field)
  constexpr bool CUBE = NCH == 1;
  constexpr int IL = CUBE ? 0 : NCH;
  static_assert(!CUBE || (MULTI == 0 && ROPE && SMALL && STATS == 0 && EXA_BASIS_FORM == 1 && !EXA_EMPTY_CELLS),
                "the cube records are a variant of the shipped one-channel 32-bit rope march");
  // The cube variants hold one int4 of the record instead of two, so they have the registers to keep |dir|^2 and the refined
  // reciprocals across the march instead of forming them again (LEAN, which the other seven-wave variants need to stay within
  // 72): C4 15.83 against 16.02 ms with LEAN (profiles/cube_records_bench.txt).  -DEXA_CUBE_LEAN=1 builds them with it.
#ifndef EXA_CUBE_LEAN
#define EXA_CUBE_LEAN 0
#endif
  // The cube variants shade a finished sample one visit late (DEFER): nothing of a sample's epilogue — TF lookup, gradient
  // shading, opacity correction, "over" — enters the next sample's position or addresses, only the end of the ray does, once
  // per ray.  So the epilogue of sample k runs between the issue of the cell loads of sample k+1's first brick and their
  // first use, inside a wait the wave pays anyway, instead of with no load in flight.  Same operations on the same values in
  // the same order per sample: the frames are the same bit for bit (tests/test_gpu_march_defer.py); a ray that the pending
  // sample ends has taken part in one more walk burst, pop or visit's loads (positions it would have sampled, clamped
  // addresses).  -DEXA_MARCH_DEFER=0 builds the cube variants with the epilogue in place (profiles/march_defer_bench.txt).
#ifndef EXA_MARCH_DEFER
#define EXA_MARCH_DEFER 1
#endif
  constexpr bool DEFER = CUBE && EXA_MARCH_DEFER;
  // ... and with gradient shading the deferred epilogue runs with a visit's eight cells and its position in the brick live:
  // LEAN again, or a register is reloaded from scratch in the epilogue behind a wait for all loads (72 VGPRs, no scratch).
  constexpr bool LEAN = marchWaves(MULTI, STATS, SMALL, NCH, ROPE) >= 7 && (!CUBE || EXA_CUBE_LEAN || (DEFER && GRAD));
  // Does the queue hand over the region's packed record (the march tree's leaf reference) or its id?  The 32-bit variants of the
  // rope march are launched only for scenes whose records pack (launchRenderKdT: `small`), its counting variant takes ids: known
  // when the kernel is compiled (no test of a kernel argument in the pop and at the leaf: C4 17.11 -> 17.03 ms).  Everything else
  // finds out from its arguments.
  constexpr int PACKED_CT = !ROPE ? -1 : (STATS == 1 ? 0 : (SMALL ? 1 : -1));
  const bool packedRec = PACKED_CT < 0 ? a.leafBeginBits != 0 : PACKED_CT != 0;
  static_assert(IL == 0 || (MULTI == 2 && STATS == 0), "the interleaved march is a multi-channel variant of the shipped kernel");
  // Entries of the lane's short stack.  The two-table multi-channel march runs with one fewer: a workgroup then needs
  // 25 KB instead of 28 KB of LDS and a sixth workgroup fits a CU (C3: 30.8 -> 29.4 ms; a shorter stack alone costs ~1 %:
  // a dropped entry is re-found by a restart from the root).  With three tables the sixth workgroup does not fit either
  // way and the 80-VGPR build only costs (3 channels on C4: +2 %): MULTI == 2 keeps 4 entries and 5 waves per SIMD.
  constexpr int KS = marchLds(MULTI == 1, false, 0).stackEntries;                 // entries the stack walk keeps per lane
  // entries of the lane's segment queue: the rope walk keeps no stack and gives the queue that LDS as well
  constexpr int QN = marchLds(MULTI == 1, ROPE, 0).queueEntries;
  // the occupancy a variant is compiled for is only reached if that many workgroups' LDS fit a CU (160 KB): the fewest TF
  // tables the variant is launched with (launchRenderKdT: one per primary channel; MULTI == 1: exactly two) + the lane's
  // queue, and for the stack walk its stack
  static_assert(ldsFits(marchLds(MULTI == 1, ROPE, IL ? IL : (MULTI ? 2 : 1)), marchWaves(MULTI, STATS, SMALL, NCH, ROPE)),
                "LDS per workgroup x waves per SIMD exceeds the CU's 160 KB: shorten the queue or lower the occupancy");
  const LdsPtrs lds = carveLds(marchLds(MULTI == 1, ROPE, a.numXfChannels));
  float4 *queue4 = lds.queue4;                                        // rope walk: 16-byte entries, one LDS access each
  float *stackF = lds.stackF, *qT = lds.qT;
  int *qRegion = lds.qRegion;
  // (kernelPrologue, written out: at 72 / 80 registers this kernel's allocation moves with where the compiler lays out the
  // staging loop, and its variants are held to their registers, tests/test_kernel_resources.py)
  for (int i = threadIdx.x; i < a.numXfChannels * EXA_NUM_XF_VALUES; i += kKdBlock) lds.xf[i] = a.xf[i];
  __syncthreads();
  Ctx<STATS> C;
  initCtx(C, a, lds);
  const unsigned long long clockBegin = clock64();                              // :1588
  if (STATS) for (int i = 0; i < ST_COUNT; i++) C.st[i] = 0;
  __shared__ unsigned long long lapMarks[STATS == 2 ? 8 * (kKdBlock / 64) : 1];
  if (STATS == 2) {
    C.lapMark = lapMarks + 8 * (threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 0) {
      C.lapMark[0] = clock64(); C.lapMark[1] = ST_T_OTHER - ST_T_BRICK;
      for (int i = 2; i < 7; i++) C.lapMark[i] = 0;
    }
  }

  const int wavesPerBlock = kKdBlock / 64;
  const int gwave = blockIdx.x * wavesPerBlock + (threadIdx.x >> 6);
  const int tile = a.tileMap[gwave >> 2];
  const int tx = tile % a.tilesX, ty = tile / a.tilesX;
  const int wave = gwave & 3, lane = threadIdx.x & 63;
  const int inX = ((wave & 1) << 3) + laneX(lane), inY = ((wave >> 1) << 3) + laneY(lane);
  const int px = tx * kTile + inX, py = ty * kTile + inY;
  const bool inside = px < a.W && py < a.H && (a.debugPixel < 0 || a.debugPixel == px + a.W * py);

  if (STATS == 1 && a.walkProbe) C.probe = a.walkProbe + size_t(gwave) * kWalkProbeSize;
  unsigned marchIters = 0;
  if (inside) {
    const ExaHipFrameState &fs = a.fs;
    const int frameID = fs.frameID;
    Lcg rnd;
    Ray ray = cameraRay(a, px, py, rnd);
    // ---- surfaces: results of the pre-pass launch (the background colour is fetched after the march) ----
    float surface_t_hit = ray.tmax;
    if (SURF) {
      const size_t slot0 = slotOf(a, tile, inX, inY, px, py);
      surface_t_hit = a.surf[slot0].w;
      rnd.state = a.surfRnd[slot0];
    }
    const float interleavedSamplingOffset = rnd.next();                           // :1655
    clipToVoxelSpace(fs, ray, surface_t_hit);
    // the ray origin is the camera position in voxel space: the same value in every lane, so it lives in scalar registers
    ray.org.x = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ray.org.x)));
    ray.org.y = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ray.org.y)));
    ray.org.z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ray.org.z)));

    Color4 pixelColor; pixelColor.x = pixelColor.y = pixelColor.z = pixelColor.w = 0.f;
    const int numChannels = a.p.numPrimaryChannels;

    // ---- walk set-up: interval of the kd root along the ray ----
    KdWalk w;
    w.pk.v = 0;
    {
      Ray whole = ray; whole.tmin = -INFINITY; whole.tmax = INFINITY;
      float r0, r1;
      const bool hit = boxTest(whole, mk(a.kdLo), mk(a.kdHi), r0, r1);
      w.tn = fmaxf(r0, ray.tmin);
      w.tf = fminf(r1, ray.tmax);
      w.tEnd = w.tf;
      w.ref = (hit && w.tn < w.tf) ? (ROPE ? a.ropeRoot : a.kdMarchRoot) : EXA_KD_DONE;
    }
    // rope walk: the short exact division is valid when every ray of the wave (and the scene's planes) are in its range —
    // one decision per wave, so the walk's code does not diverge on it
    bool ropeFast = false;
    if (ROPE) ropeFast = a.ropeFastDiv != 0 && !anyLane(!ropeRayInRange(ray));

    float walkTmin = ray.tmin;

    // ---- segment / sample state ----
    bool haveSeg = false;
    int listBegin = 0, listSize = 0;
    float flcw = 1.f;                     // region.finestLevelCellWidth; dt = launch.dt * flcw (:1129)
    float t1 = 0.f, t_i = 0.f, t_sample = 0.f, actual_dt = 0.f;   // this step's t_next is fminf(t_i, t1): not kept
    int child = 0, chan = 0;                                     // chan stays 0 (and folds away) unless MULTI
    int4 hb0 = make_int4(0, 0, 0, 1), hb1 = make_int4(1, 1, 1, 0);
    Basis B;
    B.sumWV = 0.f; B.sumW = 0.f; B.sumD = mk(0.f, 0.f, 0.f); B.sumDC = mk(0.f, 0.f, 0.f);
    // interleaved march: value-weighted sums of channels 1..IL-1 (channel 0 and the shared sumW / sumDC live in B)
    float xWV[IL > 1 ? IL - 1 : 1];
    V3 xD[IL > 1 ? IL - 1 : 1];
#pragma unroll
    for (int c = 0; c < (IL > 1 ? IL - 1 : 1); c++) { xWV[c] = 0.f; xD[c] = mk(0.f, 0.f, 0.f); }
    const float *field0 = a.sc.scalars + a.sc.channelOffset[0];   // wave-uniform
    const float *field = field0;
    // fast_math, one channel: the reciprocal of the TF range is the same for every sample of the frame; it is
    // wave-uniform, so it lives in a scalar register (readfirstlane) instead of a vector register
    float xfRcpRange0 = 0.f, xfRange0 = 0.f;
    if (FAST && !MULTI) {
      // (the compiler folds this readfirstlane of a provably uniform value away and keeps the range in a vector register after all;
      // forcing the scalar register with an asm v_readfirstlane measured the same, 17.03-17.11 against 16.98-17.03 ms)
      xfRange0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((fs.xfDomain[0][1] - fs.xfDomain[0][0]) + 1e-20f)));
      xfRcpRange0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(__builtin_amdgcn_rcpf(xfRange0))));
    }
    // ... and with the interleaved march one per channel (a transcendental per channel and sample otherwise)
    float xfRcpRangeN[IL ? IL : 1], xfRangeN[IL ? IL : 1];
#pragma unroll
    for (int c = 0; c < (IL ? IL : 1); c++) {
      xfRangeN[c] = (FAST && IL) ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int((fs.xfDomain[c][1] - fs.xfDomain[c][0]) + 1e-20f))) : 0.f;
      xfRcpRangeN[c] = (FAST && IL) ? __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(__builtin_amdgcn_rcpf(xfRangeN[c])))) : 0.f;
    }

    // DEFER: the finished sample whose sums stand in B has not been shaded yet.  Its step and its region's cell width are
    // carried with it: a pop may have made flcw another region's before its epilogue runs.
    bool pending = false;
    float pendDt = 0.f, pendFlcw = 1.f;
    // the sample epilogue of the one-channel march on the pending sample (:800-806, :910-927), then B at its start values
    auto shadePending = [&]() {
      if (B.sumW > 1e-20f) {
        const float cellValue = fdivExact<FAST>(B.sumWV, B.sumW);
        V3 grad = mk(0.f, 0.f, 0.f);
        if (GRAD) grad = gradOf(B.sumW, B.sumWV, B.sumD, B.sumDC);
        integrateVolume<FAST, STATS, (FAST && !MULTI), LEAN>(C, ray, pixelColor, pendDt, cellValue, grad, pendFlcw, 0, xfRcpRange0, xfRange0);
      }
      B.sumWV = 0.f; B.sumW = 0.f; B.sumD = mk(0.f, 0.f, 0.f); B.sumDC = mk(0.f, 0.f, 0.f);
      pending = false;
    };

    unsigned iter = 0;
    for (;; iter++) {
      if (iter == 0xfffffff0u) { C.guardTripped = true; break; }
      // ---- refill burst: while a lane of the wave is dry (no segment, empty queue, walk not finished), every lane
      //      with a free queue slot advances its own walk; the burst ends as soon as no lane is dry any more —
      //      running it until every queue is full dragged it out with a handful of lanes (C4: 24.1 -> 22.5 ms) ----
      // (starting a burst only once 2 / 4 / 8 lanes are dry, the dry ones sitting iterations out: 23.4 / 23.8 / 25.0 ms)
      if (anyLane(!haveSeg && w.pk.get(PK_QCOUNT) == 0 && w.ref != EXA_KD_DONE)) {
        C.lap(ST_T_WALK);
        do {
          const bool want = w.pk.get(PK_QCOUNT) < QN && w.ref != EXA_KD_DONE;   // top-ups matter: only lanes with <= 2 / 1 / 0 queued: 23.3 / 25.8 / 34.2 ms
          if (want) {
            if (ROPE) ropeStep<STATS, SMALL, QN, LEAN, PACKED_CT>(C, w, walkTmin, a, queue4, ray, ropeFast, interleavedSamplingOffset);
            else kdStep<false, STATS, SMALL, KS>(C, w, walkTmin, a, stackF, qRegion, qT, ray, 0, walkTmin, 1.f, a.kdMarchNodes, a.kdMarchRoot);
          }
        } while (anyLane(!haveSeg && w.pk.get(PK_QCOUNT) == 0 && w.ref != EXA_KD_DONE));
      }
      if (!haveSeg) {
        // ---- next segment from this lane's queue ----
        C.lap(ST_T_SEG);
        const int qc = w.pk.get(PK_QCOUNT);
        if (qc == 0) break;                                                        // walk finished: ray done
        const int qh = w.pk.get(PK_QHEAD);
        int region;
        float t0, tiQueued = 0.f;
        if (ROPE) {
          const float4 e = queue4[qh * kKdBlock];
          region = __float_as_int(e.x); t1 = e.y; tiQueued = e.z; t0 = e.w;
        } else {
          region = qRegion[qh * kKdBlock];
          t0 = qT[(2 * qh) * kKdBlock];
          t1 = qT[(2 * qh + 1) * kKdBlock];
        }
        w.pk.template incWrap<QN>(PK_QHEAD);
        w.pk.dec(PK_QCOUNT);
        if (packedRec) {
          // the leaf reference of the march tree is the region's record itself: no load between the queue and
          // the first brick record
          const unsigned d = (unsigned)region;
          listBegin = (int)(d & ((1u << a.leafBeginBits) - 1u));
          listSize = (int)((d >> a.leafBeginBits) & ((1u << a.leafSizeBits) - 1u)) + 1;
          flcw = __int_as_float((127 + (int)(d >> (a.leafBeginBits + a.leafSizeBits))) << 23);     // 2^level
        } else {
          const RegionInfo ri = a.sc.regionInfo[region];
          listBegin = ri.listBegin; listSize = ri.listSize;
          flcw = ri.finestLevelCellWidth;
        }
        C.count(ST_SEGMENTS);
        haveSeg = true;
        w.pk.setBit(PK_NEEDHDR);
        if (ROPE && packedRec)                                    // the walk has worked it out with the leaf (ropeStep)
          t_i = tiQueued;
        else if (a.invDtPow2 != 0.f)                              // :1141-1144
          t_i = firstSampleTPow2(t0, a.p.dt * flcw, a.invDtPow2 * __int_as_float(0x7f000000 - __float_as_int(flcw)), interleavedSamplingOffset);
        else
          t_i = firstSampleT(t0, a.p.dt * flcw, interleavedSamplingOffset);
        // first step of the segment (:1158-1166)
        {
          const float t_next = fminf(t_i, t1);
          t_sample = 0.5f * (fminf(t1, t_next) + t0);
          actual_dt = t_next - t0;
        }
        // child, chan/field and the basis sums are already at their start values here: the sample
        // epilogue resets them, and a segment only ends there
        C.count(ST_SAMPLE_EVALS);
      }

      // ---- one brick visit ----
      C.lap(ST_T_BRICK);
      C.phase(ST_W_BRICK);
      // brick records are stored along the leaf list (no id indirection); a one-brick region keeps the
      // record it loaded at the start of the segment
      // (requesting the NEXT visit's record here, behind this visit's cell loads — so that a visit in a region of several
      // bricks does not wait for two loads one after the other — was measured: C4 17.35 -> 18.92 ms; profiles/r05_experiments.txt)
      if (listSize > 1 || w.pk.get(PK_NEEDHDR)) {
        if (CUBE) {                                        // the brick's cube record: one 16-byte load, one int4 kept (hb1 is never set)
          hb0 = *reinterpret_cast<const int4 *>(reinterpret_cast<const char *>(a.leafHdrCube) + ((uint32_t)(listBegin + child) << 4));
        } else if (SMALL) {                                // the header array is below 4 GiB
          const char *hp = reinterpret_cast<const char *>(a.sc.leafHdr) + ((uint32_t)(listBegin + child) << 5);
          hb0 = *reinterpret_cast<const int4 *>(hp); hb1 = *reinterpret_cast<const int4 *>(hp + 16);
        } else {
          const unsigned at = 2u * (unsigned)(listBegin + child);
          hb0 = a.sc.leafHdr[at]; hb1 = a.sc.leafHdr[at + 1u];
        }
        w.pk.clearField(PK_NEEDHDR);
      }
      // (two consecutive samples of a one-brick segment per iteration, so that both samples' cell loads are in flight together, was
      // built and measured at 5 and 4 waves per SIMD: C4 17.34 -> 25.05 ms; profiles/r05_experiments.txt 9)
      if (DEFER) {
        // this visit's cell loads go out, the previous sample is shaded while they are on their way, then they are used
        bool ended = false;
        addBasisFast<GRAD, STATS, SMALL, false, CUBE>(C, B, hb0, hb1, field0, rayAt(ray.org, t_sample, ray.dir), a.cubeLog2, [&]() {
          if (pending) {                                     // the first brick of the next sample: B is still the last one's
            shadePending();
            ended = pixelColor.w >= EXA_TERMINATION_THRESHOLD;   // the end of the ray (:1180): the loads in flight are abandoned
          }
          return !ended;
        });
        if (ended) {
          pixelColor.x = pixelColor.x * pixelColor.w;                                // :1694-1696
          pixelColor.y = pixelColor.y * pixelColor.w;
          pixelColor.z = pixelColor.z * pixelColor.w;
          pixelColor.w = 1.f;
          break;
        }
        child++;
        if (child < listSize) continue;
        // all bricks of the region seen: the sample waits in B for the next visit's loads (or the flush behind the loop)
        child = 0;
        pending = true; pendDt = actual_dt; pendFlcw = flcw;
        // ---- end of this step (:1180-1183), without the test of the colour ----
        const float t_last = fminf(t_i, t1);
        if (t_last >= t1) {
          haveSeg = false;
          continue;
        }
        t_i += a.p.dt * flcw;
        {
          const float t_next = fminf(t_i, t1);
          t_sample = 0.5f * (fminf(t1, t_next) + t_last);
          actual_dt = t_next - t_last;
        }
        continue;
      }
      if (IL) addBasisFastIl<GRAD, SMALL, (IL ? IL : 2)>(B, xWV, xD, hb0, hb1, a.cellsIl, rayAt(ray.org, t_sample, ray.dir));
      else if (CUBE) addBasisFast<GRAD, STATS, SMALL, false, CUBE>(C, B, hb0, hb1, field0, rayAt(ray.org, t_sample, ray.dir), a.cubeLog2);
      else addBasisFast<GRAD, STATS, SMALL>(C, B, hb0, hb1, MULTI ? field : field0, rayAt(ray.org, t_sample, ray.dir));   // :1166
      child++;
      if (child < listSize) continue;

      // ---- all bricks of the region seen: finish this channel's sample (:800-806, :910-927) ----
      C.lap(ST_T_FINAL);
      C.phase(ST_W_FINAL);
      if (IL) {
        // every primary channel's sample of this step, in channel order (:1163-1178); valid or not is the same for all
        // of them (sumW does not depend on the cell values)
        if (B.sumW > 1e-20f) {
#pragma unroll
          for (int c = 0; c < IL; c++) {
            const float wv = c == 0 ? B.sumWV : xWV[c == 0 ? 0 : c - 1];
            const V3 sd = c == 0 ? B.sumD : xD[c == 0 ? 0 : c - 1];
            const float cellValue = fdivExact<FAST>(wv, B.sumW);
            V3 grad = mk(0.f, 0.f, 0.f);
            if (GRAD) grad = gradOf(B.sumW, wv, sd, B.sumDC);
            integrateVolume<FAST, STATS, FAST>(C, ray, pixelColor, actual_dt, cellValue, grad, flcw, c, xfRcpRangeN[c], xfRangeN[c]);
          }
        }
#pragma unroll
        for (int c = 0; c < (IL > 1 ? IL - 1 : 1); c++) { xWV[c] = 0.f; xD[c] = mk(0.f, 0.f, 0.f); }
      } else if (B.sumW > 1e-20f) {
        C.count(ST_SAMPLES);
        const float cellValue = fdivExact<FAST>(B.sumWV, B.sumW);
        V3 grad = mk(0.f, 0.f, 0.f);
        if (GRAD) grad = gradOf(B.sumW, B.sumWV, B.sumD, B.sumDC);
        integrateVolume<FAST, STATS, (FAST && !MULTI), LEAN>(C, ray, pixelColor, actual_dt, cellValue, grad, flcw, MULTI ? chan : 0, xfRcpRange0, xfRange0);
      }
      B.sumWV = 0.f; B.sumW = 0.f; B.sumD = mk(0.f, 0.f, 0.f); B.sumDC = mk(0.f, 0.f, 0.f);
      child = 0;
      if (MULTI && !IL) {
        chan++;
        if (chan < numChannels) {
          field = a.sc.scalars + a.sc.channelOffset[chan];
          C.count(ST_SAMPLE_EVALS);
          continue;
        }
        chan = 0; field = field0;
      }
      // ---- end of this step (:1180-1183) ----
      if (pixelColor.w >= EXA_TERMINATION_THRESHOLD) {
        pixelColor.x = pixelColor.x * pixelColor.w;                                // :1694-1696
        pixelColor.y = pixelColor.y * pixelColor.w;
        pixelColor.z = pixelColor.z * pixelColor.w;
        pixelColor.w = 1.f;
        break;
      }
      const float t_last = fminf(t_i, t1);       // this step's t_next (:1158), recomputed instead of kept in a register
      if (t_last >= t1) {                        // segment done (:1182; :1698 is in kdStep)
        haveSeg = false;
        continue;
      }
      t_i += a.p.dt * flcw;
      {
        const float t_next = fminf(t_i, t1);
        t_sample = 0.5f * (fminf(t1, t_next) + t_last);
        actual_dt = t_next - t_last;
      }
      C.count(ST_SAMPLE_EVALS);
    }

    if (DEFER && pending) {
      // the ray's last sample, on every way out of the loop but the one it took itself: shaded, and the end of the ray's test
      shadePending();
      if (pixelColor.w >= EXA_TERMINATION_THRESHOLD) {
        pixelColor.x = pixelColor.x * pixelColor.w;                                  // :1694-1696
        pixelColor.y = pixelColor.y * pixelColor.w;
        pixelColor.z = pixelColor.z * pixelColor.w;
        pixelColor.w = 1.f;
      }
    }
    C.lap(ST_T_OTHER);
    marchIters = iter;
    // The pixel's framebuffer slot is worked out again from the thread id (and, in a shard, the tile number fetched again)
    // instead of being kept in registers across the march (the kernel runs at exactly 80 — the seven-wave variant: 72 —
    // VGPRs; the asm keeps the compiler from re-using the values computed before the loop).
    size_t slot, colorSlot;               // colorSlot: row-major in the root's frame for a device of a multi-device handle
    {
      unsigned tid = threadIdx.x, bid = blockIdx.x;
      asm volatile("" : "+v"(tid));
      asm volatile("" : "+s"(bid));
      const int lane2 = tid & 63, wave2 = (tid >> 6) & 3;
      const int inX2 = ((wave2 & 1) << 3) + laneX(lane2), inY2 = ((wave2 >> 1) << 3) + laneY(lane2);
      slot = (a.world == 1) ? size_t(tx * kTile + inX2) + size_t(a.W) * (ty * kTile + inY2)
                            : size_t(a.tileMap[(bid * wavesPerBlock + (tid >> 6)) >> 2] / a.world) * kTilePixels + (inY2 * kTile + inX2);
      colorSlot = a.colorRowMajor ? size_t(tx * kTile + inX2) + size_t(a.W) * (ty * kTile + inY2) : slot;
    }
    if (SURF && a.pixOut) {
      // The surfaces' colour may still be in the making — the ambient-occlusion rays run BESIDE this march (exa_module:
      // ao_overlap) —, so the pixel is finished by compositeKdKernel once both are done: same operations, same order.
      a.pixOut[slot] = make_float4(pixelColor.x, pixelColor.y, pixelColor.z, pixelColor.w);
    } else {
    float4 bgColor = make_float4(0.f, 0.f, 0.f, 0.f);
    if (SURF) bgColor = a.surf[slot];
    float cr = pixelColor.w * pixelColor.x + (1.f - pixelColor.w) * bgColor.x;     // :1701
    float cg = pixelColor.w * pixelColor.y + (1.f - pixelColor.w) * bgColor.y;
    float cb = pixelColor.w * pixelColor.z + (1.f - pixelColor.w) * bgColor.z;
    if (fs.clockScale > 0.f) cr = clockHeat(fs.clockScale, clockBegin);          // :1703-1707
    if (frameID > 0) {
      const float4 acc = a.accum[slot];
      cr += acc.x; cg += acc.y; cb += acc.z;
    }
    a.accum[slot] = make_float4(cr, cg, cb, 1.f);
    const float div = frameID + 1.f;
    cr = cr / div; cg = cg / div; cb = cb / div;
    a.color[colorSlot] = make_rgba8(linear_to_srgb(cr), linear_to_srgb(cg), linear_to_srgb(cb));
    }
  }

  if (a.tileCost) {
    // launch-order feedback: the longest ray of this tile, in brick visits (= march iterations of its lane)
    unsigned v = marchIters;
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_down((int)v, off, 64));
    // (the tile number is fetched again: the compiler copies the first fetch into a vector register — the index of this access —
    // before the march and carries — at 72 registers: spills — it across)
    unsigned bid = blockIdx.x, tid = threadIdx.x;
    asm volatile("" : "+s"(bid));
    asm volatile("" : "+v"(tid));
    if (lane == 0) atomicMax(&a.tileCost[a.tileMap[(bid * wavesPerBlock + (tid >> 6)) >> 2]], v);
  }
  if (C.guardTripped) atomicExch(a.errorFlag, 1);
  if (STATS == 2) {
    if (lane < 5 && C.lapMark[2 + lane]) atomicAdd(&a.stats[ST_T_BRICK + lane], C.lapMark[2 + lane]);
  }
  if (STATS == 1) {
    for (int i = 0; i < ST_COUNT; i++) {
      unsigned long long v = inside ? C.st[i] : 0ull;
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if ((threadIdx.x & 63) == 0 && v) atomicAdd(&a.stats[i], v);
    }
    // how evenly a workgroup's four waves finish (its LDS stays allocated until the slowest one does): sum of the
    // waves' march iterations against 4 x the slowest wave's, over all workgroups
    __shared__ unsigned wgMaxIters;
    if (threadIdx.x == 0) wgMaxIters = 0;
    __syncthreads();
    unsigned v = marchIters;
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_down((int)v, off, 64));
    if (lane == 0) atomicMax(&wgMaxIters, v);
    __syncthreads();
    if (lane == 0) atomicAdd(&a.stats[ST_WAVE_ITERS], (unsigned long long)v);
    if (threadIdx.x == 0) atomicAdd(&a.stats[ST_TILE_ITERS], 4ull * wgMaxIters);
  }
}

// ------------------------------------------------------------------------
// Wide march: L lanes per ray.  A frame's critical path is its longest rays (one lane marches one
// ray, sample after sample: thousands of dependent iterations of ~2.5 us when the GPU is emptying),
// which bounds a multi-GPU shard long before throughput does.  Everything that is expensive about a
// sample — basis reconstruction, TF lookup, shading, opacity correction — does not depend on the
// colour accumulated so far; only the "over" operator does.  So the L lanes of a ray evaluate L
// consecutive samples of the segment at once and then composite them in order (every lane does the
// same ten operations on the same values, so all copies of the pixel stay identical and no lane has
// to be told about an early termination).  Same samples, same arithmetic, same order as the one-lane
// march: the pixels are bit-identical.  The walk is parallel as well: every lane of the ray lists the leaves of one
// depth window of it in HBM first (kdCollectStep below), then the lists are marched in order.
// Used for the tiles the launch-order feedback marks as critical (exa_module: reorderFromCosts);
// single primary channel only.
// ------------------------------------------------------------------------
// One step of a window walker of the wide march: the kd walk of kdStep (same stages, same order of leaves) that
// records every leaf whose entry distance lies in [winLo, winHi) as {record, tn, tf} in `out` instead of testing it
// against the march's running tmin — that test needs the end of the previous accepted segment, which a walker of a
// later window does not know yet; the march applies it when it consumes the list.  Subtrees that end before the
// window are skipped, the walk ends with the first one that starts behind it.
__device__ __forceinline__ void kdCollectStep(Ctx<0> &C, KdWalk &w, const float winLo, const float winHi, const RenderArgs &a,
                                              float *stackF, const Ray &ray, const KdNodeDev *nodes, const int root,
                                              float4 *out, unsigned &count)
{
  if (w.ref != EXA_KD_EMPTY && !(w.tn < winHi)) { w.ref = EXA_KD_DONE; return; }
  if (w.ref < 0 && w.ref > EXA_KD_DONE) {
    if (w.tn >= winLo && w.tn < w.tf) out[count++] = make_float4(__int_as_float(~w.ref), w.tn, w.tf, 0.f);   // caller: count < cap
    w.ref = EXA_KD_EMPTY;
  }
  if (w.ref == EXA_KD_EMPTY || (w.ref != EXA_KD_DONE && !(w.tf > winLo))) kdPop(C, w, root, stackF, nodes, ray);
  if (w.ref < 0 || !(w.tf > winLo) || !(w.tn < winHi)) return;
  kdNodeStage<kKdStackEntries, false, 0>(C, w, stackF, ray, nodes, 2);   // volume activity
}

template <bool GRAD, bool FAST, bool SURF, int L, bool SMALL>
__global__ __launch_bounds__(kKdBlock, 4) void renderFrameKdWideKernel(const RenderArgs a)
{
  static_assert(ldsFits(kdLds(1), 4), "LDS per workgroup x waves per SIMD exceeds the CU's 160 KB");   // one primary channel
  const LdsPtrs lds = carveLds(kdLds(a.numXfChannels));
  float *stackF = lds.stackF;
  Ctx<false> C;
  kernelPrologue(C, a, lds);
  const unsigned long long clockBegin = clock64();                              // :1588

  // these waves are the frame's critical path: let them issue ahead of the one-lane march they share SIMDs with
  __builtin_amdgcn_s_setprio(3);
  // L workgroups per 16x16 tile; a wave marches 64/L rays
  const int tile = a.wideTileMap[blockIdx.x / L];
  const int part = blockIdx.x % L;
  const int tx = tile % a.tilesX, ty = tile / a.tilesX;
  const int lane = threadIdx.x & 63, sub = lane & (L - 1), lead = lane & ~(L - 1);
  const bool leader = sub == 0;                        // writes the pixel
  const int r = part * (kTilePixels / L) + (threadIdx.x >> 6) * (64 / L) + lane / L;     // ray of the tile
  const int inX = (((r >> 6) & 1) << 3) + (r & 7), inY = ((r >> 7) << 3) + ((r >> 3) & 7);   // 8x8 block order, as the one-lane kernel
  const int px = tx * kTile + inX, py = ty * kTile + inY;
  const bool inside = px < a.W && py < a.H && (a.debugPixel < 0 || a.debugPixel == px + a.W * py);

  unsigned myVisits = 0;
  if (inside) {
    const ExaHipFrameState &fs = a.fs;
    const int frameID = fs.frameID;
    Lcg rnd;
    Ray ray = cameraRay(a, px, py, rnd);
    const size_t slot = slotOf(a, tile, inX, inY, px, py);
    float surface_t_hit = ray.tmax;
    if (SURF) {
      surface_t_hit = a.surf[slot].w;
      rnd.state = a.surfRnd[slot];
    }
    const float interleavedSamplingOffset = rnd.next();                           // :1655
    clipToVoxelSpace(fs, ray, surface_t_hit);

    Color4 pixelColor; pixelColor.x = pixelColor.y = pixelColor.z = pixelColor.w = 0.f;

    // ---- phase 1: every lane of the ray walks one window of it.  The root interval is cut into L windows by
    //      entry distance; lane `sub` lists the leaves that start in window `sub`, whole (a leaf is never split),
    //      in HBM.  All 64 lanes of the wave walk at once, where the one-lane march walks with a quarter of them.
    float4 *const mySegs = a.wideSegs + (size_t(blockIdx.x / L) * kTilePixels * L + size_t(r) * L + sub) * kWideSegCap;
    unsigned myCount = 0;
    KdWalk w;                            // stays alive: a window with more leaves than its list holds is walked in rounds
    w.pk.v = 0;
    float winLo, winHi;
    {
      Ray whole = ray; whole.tmin = -INFINITY; whole.tmax = INFINITY;
      float r0, r1;
      const bool hit = boxTest(whole, mk(a.kdLo), mk(a.kdHi), r0, r1);
      w.tn = fmaxf(r0, ray.tmin);
      w.tf = fminf(r1, ray.tmax);
      w.tEnd = w.tf;
      w.ref = (hit && w.tn < w.tf) ? a.kdMarchRoot : EXA_KD_DONE;
      const float span = w.tf - w.tn;
      winLo = sub == 0 ? -INFINITY : w.tn + span * (float(sub) / float(L));
      winHi = sub == L - 1 ? INFINITY : w.tn + span * (float(sub + 1) / float(L));
      for (unsigned g = 0;; g++) {
        if (g == 0xfffffff0u) { C.guardTripped = true; break; }
        const bool want = w.ref != EXA_KD_DONE && myCount < kWideSegCap;
        if (!anyLane(want)) break;
        if (want) kdCollectStep(C, w, winLo, winHi, a, stackF, ray, a.kdMarchNodes, a.kdMarchRoot, mySegs, myCount);
      }
    }
    // The lists go from the lane that wrote them to the other lanes of the ray through global memory: release here,
    // acquire in front of the reads (wavefront scope — writer and readers are lanes of one wave; no instruction is
    // generated, the fences pin the order the compiler may not change)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // ---- phase 2: the march consumes the lists in order ----
    float walkTmin = ray.tmin;
    int curWin = 0;
    unsigned curIdx = 0, curCount = (unsigned)__shfl((int)myCount, lead, 64);
    const float4 *curSegs = a.wideSegs + (size_t(blockIdx.x / L) * kTilePixels * L + size_t(r) * L) * kWideSegCap;

    bool haveSeg = false, newStep = false, needHdr = false, mine = false;
    int listBegin = 0, listSize = 0;
    float flcw = 1.f, dtSeg = 0.f;
    float t1 = 0.f, tiBase = 0.f, tlBase = 0.f;        // t_i of the step's first sample, t_next of the sample before it
    float t_sample = 0.f, actual_dt = 0.f;
    int child = 0;
    int4 hb0 = make_int4(0, 0, 0, 1), hb1 = make_int4(1, 1, 1, 0);
    Basis B;
    B.sumWV = 0.f; B.sumW = 0.f; B.sumD = mk(0.f, 0.f, 0.f); B.sumDC = mk(0.f, 0.f, 0.f);
    const float *field0 = a.sc.scalars + a.sc.channelOffset[0];

    for (unsigned iter = 0;; iter++) {
      if (iter == 0xfffffff0u) { C.guardTripped = true; break; }
      if (!haveSeg) {
        // ---- next segment: the next listed leaf that passes the reference's test against the running tmin
        //      (t0 = max(tmin, tn) < t1, then tmin = t1 * 1.0000001f: exabrick.cu:197-210, :1698); all lanes of the
        //      ray read the same entry ----
        int region = -1;
        float t0 = 0.f;
        for (;;) {
          if (curIdx >= curCount) {
            // list of window curWin used up.  Its walker may have stopped at a full list: next round for that lane
            // (the other lanes of the ray wait; rare), otherwise on to the next window
            const bool mineIsCur = sub == curWin;
            if (__shfl((int)(w.ref != EXA_KD_DONE), lead + curWin, 64)) {
              if (mineIsCur) {
                myCount = 0;
                for (unsigned g = 0; w.ref != EXA_KD_DONE && myCount < kWideSegCap; g++) {
                  if (g == 0xfffffff0u) { C.guardTripped = true; break; }
                  kdCollectStep(C, w, winLo, winHi, a, stackF, ray, a.kdMarchNodes, a.kdMarchRoot, mySegs, myCount);
                }
              }
              __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");       // refilled list: writer lane -> reader lanes
              __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
              curIdx = 0;
              curCount = (unsigned)__shfl((int)myCount, lead + curWin, 64);
              continue;
            }
            if (++curWin == L) break;
            curIdx = 0;
            curCount = (unsigned)__shfl((int)myCount, lead + min(curWin, L - 1), 64);
            curSegs += kWideSegCap;
            continue;
          }
          const float4 e = curSegs[curIdx++];
          t0 = fmaxf(walkTmin, e.y);
          if (t0 < e.z) {
            region = __float_as_int(e.x);
            t1 = e.z;
            walkTmin = t1 * (1.0000001f);
            break;
          }
        }
        if (curWin == L) break;                                                    // lists exhausted: ray done
        if (a.leafBeginBits) {
          // the leaf reference of the march tree is the region's record itself: no load between the queue and
          // the first brick record
          const unsigned d = (unsigned)region;
          listBegin = (int)(d & ((1u << a.leafBeginBits) - 1u));
          listSize = (int)((d >> a.leafBeginBits) & ((1u << a.leafSizeBits) - 1u)) + 1;
          flcw = __int_as_float((127 + (int)(d >> (a.leafBeginBits + a.leafSizeBits))) << 23);     // 2^level
        } else {
          const RegionInfo ri = a.sc.regionInfo[region];
          listBegin = ri.listBegin; listSize = ri.listSize;
          flcw = ri.finestLevelCellWidth;
        }
        dtSeg = a.p.dt * flcw;
        tiBase = firstSampleT(t0, dtSeg, interleavedSamplingOffset);               // :1141-1144
        tlBase = t0;
        haveSeg = true; newStep = true; needHdr = true;
      }
      if (newStep) {
        // ---- this lane's sample of the step: sample `sub` after the step's first one (:1158-1166) ----
        float ti = tiBase, tl = tlBase, myTn = 0.f, myTl = 0.f;
        bool ex = true;
        mine = false;
#pragma unroll
        for (int s = 0; s < L; s++) {
          const float tn = fminf(ti, t1);
          if (s == sub) { myTn = tn; myTl = tl; mine = ex; }
          ex = ex && tn < t1;                     // the segment ends with the first sample that reaches t1 (:1182)
          tl = tn;
          ti = ti + dtSeg;
        }
        t_sample = 0.5f * (fminf(t1, myTn) + myTl);
        actual_dt = myTn - myTl;
        newStep = false;
      }

      // ---- one brick visit of this lane's sample ----
      if (mine) {
        if (listSize > 1 || needHdr) {
          const unsigned at = 2u * (unsigned)(listBegin + child);
          hb0 = a.sc.leafHdr[at]; hb1 = a.sc.leafHdr[at + 1u];
        }
        addBasisFast<GRAD, 0, SMALL>(C, B, hb0, hb1, field0, rayAt(ray.org, t_sample, ray.dir));   // :1166
        myVisits++;
      }
      needHdr = false;
      child++;
      if (child < listSize) continue;

      // ---- this lane's sample: value, gradient, colour and corrected opacity (:800-806, :910-927, :988-1011) ----
      Color4 smp; smp.x = smp.y = smp.z = smp.w = 0.f;
      int contributes = 0;
      if (mine && B.sumW > 1e-20f && actual_dt != 0.f) {
        const float cellValue = fdivExact<FAST>(B.sumWV, B.sumW);
        V3 grad = mk(0.f, 0.f, 0.f);
        if (GRAD) grad = gradOf(B.sumW, B.sumWV, B.sumD, B.sumDC);
        smp = shadeSample<FAST>(C, ray, actual_dt, cellValue, grad, flcw, 0);
        contributes = 1;
      }
      B.sumWV = 0.f; B.sumW = 0.f; B.sumD = mk(0.f, 0.f, 0.f); B.sumDC = mk(0.f, 0.f, 0.f);
      child = 0;

      // ---- composite the step's samples in order; every lane of the ray keeps the same pixel ----
      bool rayDone = false, segDone = false;
      {
        float ti = tiBase, tl = tlBase;
#pragma unroll
        for (int s = 0; s < L; s++) {
          Color4 o;
          o.x = __shfl(smp.x, lead + s, 64); o.y = __shfl(smp.y, lead + s, 64);
          o.z = __shfl(smp.z, lead + s, 64); o.w = __shfl(smp.w, lead + s, 64);
          const int oc = __shfl(contributes, lead + s, 64);
          if (!rayDone && !segDone) {
            const float tn = fminf(ti, t1);
            if (oc) compositeSample(pixelColor, o);
            if (pixelColor.w >= EXA_TERMINATION_THRESHOLD) rayDone = true;         // :1180
            else if (tn >= t1) segDone = true;                                     // :1182
            tl = tn;
            ti = ti + dtSeg;
          }
        }
        tiBase = ti; tlBase = tl;
      }
      if (rayDone) {
        pixelColor.x = pixelColor.x * pixelColor.w;                                // :1694-1696
        pixelColor.y = pixelColor.y * pixelColor.w;
        pixelColor.z = pixelColor.z * pixelColor.w;
        pixelColor.w = 1.f;
        break;
      }
      if (segDone) haveSeg = false;
      else newStep = true;
    }

    if (leader) {
      float4 bgColor = make_float4(0.f, 0.f, 0.f, 0.f);
      if (SURF) bgColor = a.surf[slot];
      float cr = pixelColor.w * pixelColor.x + (1.f - pixelColor.w) * bgColor.x;     // :1701
      float cg = pixelColor.w * pixelColor.y + (1.f - pixelColor.w) * bgColor.y;
      float cb = pixelColor.w * pixelColor.z + (1.f - pixelColor.w) * bgColor.z;
      if (fs.clockScale > 0.f) cr = clockHeat(fs.clockScale, clockBegin);          // :1703-1707
      if (frameID > 0) {
        const float4 acc = a.accum[slot];
        cr += acc.x; cg += acc.y; cb += acc.z;
      }
      a.accum[slot] = make_float4(cr, cg, cb, 1.f);
      const float div = frameID + 1.f;
      cr = cr / div; cg = cg / div; cb = cb / div;
      a.color[a.colorRowMajor ? size_t(px) + size_t(a.W) * py : slot] = make_rgba8(linear_to_srgb(cr), linear_to_srgb(cg), linear_to_srgb(cb));
    }
  }
  if (a.tileCost) {
    // launch-order feedback in the one-lane kernel's unit: brick visits of the tile's longest ray
    unsigned v = myVisits;
    for (int off = 1; off < L; off <<= 1) v += (unsigned)__shfl_xor((int)v, off, 64);
    for (int off = 32; off > 0; off >>= 1) v = max(v, (unsigned)__shfl_down((int)v, off, 64));
    if (lane == 0) atomicMax(&a.tileCost[tile], v);
  }
  if (C.guardTripped) atomicExch(a.errorFlag, 1);
}

#if !EXA_TU_ROPE
// The end of renderFrame (exabrick.cu:1701-1719) for a march that stored its pixel colour instead of finishing the pixel
// (RenderArgs::pixOut): colour over the surfaces' colour, accumulation, sRGB, pack — the operations of the march kernel's own
// epilogue, in its order, one thread per pixel of the launched tiles.
__global__ __launch_bounds__(256) void compositeKdKernel(const RenderArgs a)
{
  const int tile = a.tileMap[blockIdx.x];
  const int tx = tile % a.tilesX, ty = tile / a.tilesX;
  const int inX = threadIdx.x & 15, inY = threadIdx.x >> 4;
  const int px = tx * kTile + inX, py = ty * kTile + inY;
  if (!(px < a.W && py < a.H) || !(a.debugPixel < 0 || a.debugPixel == px + a.W * py)) return;
  const size_t slot = slotOf(a, tile, inX, inY, px, py);
  const size_t colorSlot = a.colorRowMajor ? size_t(px) + size_t(a.W) * py : slot;
  const float4 pixelColor = a.pixOut[slot];
  const float4 bgColor = a.surf[slot];
  const int frameID = a.fs.frameID;
  float cr = pixelColor.w * pixelColor.x + (1.f - pixelColor.w) * bgColor.x;     // :1701
  float cg = pixelColor.w * pixelColor.y + (1.f - pixelColor.w) * bgColor.y;
  float cb = pixelColor.w * pixelColor.z + (1.f - pixelColor.w) * bgColor.z;
  if (frameID > 0) {
    const float4 acc = a.accum[slot];
    cr += acc.x; cg += acc.y; cb += acc.z;
  }
  a.accum[slot] = make_float4(cr, cg, cb, 1.f);
  const float div = frameID + 1.f;
  cr = cr / div; cg = cg / div; cb = cb / div;
  a.color[colorSlot] = make_rgba8(linear_to_srgb(cr), linear_to_srgb(cg), linear_to_srgb(cb));
}
hipError_t launchCompositeKd(const RenderArgs &a, int numBlocks, hipStream_t s)
{
  if (numBlocks <= 0) return hipSuccess;
  hipLaunchKernelGGL(compositeKdKernel, dim3(numBlocks), dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launchRenderKdWide(const RenderArgs &a, int numTiles, int lanesPerRay, bool grad, bool fast, bool surf, hipStream_t s)
{
  if (numTiles <= 0) return hipSuccess;
#if EXA_EMPTY_CELLS
  return hipErrorNotSupported;       // scenes with empty cells march one lane per ray (the module never asks for more)
#else
  const size_t lds = kdLds(a.numXfChannels).total;
  const dim3 grid(numTiles * lanesPerRay), block(kKdBlock);
  const bool small = a.mul24 && a.addr32;                   // 24-bit address multiplies and 32-bit byte offsets are valid
#define EXA_W4(G, F, S, L) do { if (small) hipLaunchKernelGGL((renderFrameKdWideKernel<G, F, S, L, true>), grid, block, lds, s, a); \
                                else hipLaunchKernelGGL((renderFrameKdWideKernel<G, F, S, L, false>), grid, block, lds, s, a); } while (0)
  // 8 lanes per ray were measured and are not instantiated: on the critical-path probe (tests/gpu_wide_probe.py, C4,
  // rank 0 of 64) 1 / 2 / 4 / 8 lanes take 4.71 / 3.37 / 2.52 / 3.00 ms
#define EXA_W3(G, F, S) do { if (lanesPerRay == 2) EXA_W4(G, F, S, 2); else EXA_W4(G, F, S, 4); } while (0)
#define EXA_W2(G, F) do { if (surf) EXA_W3(G, F, true); else EXA_W3(G, F, false); } while (0)
  if (grad) { if (fast) EXA_W2(true, true); else EXA_W2(true, false); }
  else      { if (fast) EXA_W2(false, true); else EXA_W2(false, false); }
#undef EXA_W4
#undef EXA_W2
#undef EXA_W3
  return hipGetLastError();
#endif
}

// the frame has no triangle meshes, contour planes or streamlines: the pre-pass and the AO rays take their ISO_ONLY variants
// (both launchers must decide alike: the variant sets the wave budget the AO grid is sized by)
static bool isoOnly(const RenderArgs &a)
{
  bool only = a.numTris == 0 && a.numStreamPrims == 0;
  for (int i = 0; i < EXA_MAX_CONTOUR_PLANES; i++) only = only && !a.fs.contour[i].enabled;
  return only;
}

hipError_t launchSurfacePrepassKd(const RenderArgs &a, int numBlocks, bool stats, hipStream_t s)
{
  if (numBlocks <= 0) return hipSuccess;
  const size_t lds = kdLds(a.numXfChannels).total;
  const dim3 grid(numBlocks * (256 / kKdBlock)), block(kKdBlock);
  // the shipped variants hand their AO rays to aoRaysKdKernel (a.aoRecs / a.aoCount, cleared by the caller)
  const bool defer = !stats && a.aoRecs && a.aoCount;
  if (stats)        hipLaunchKernelGGL((surfacePrepassKdKernel<1, false, false>), grid, block, lds, s, a);
  else if (isoOnly(a)) { if (defer) hipLaunchKernelGGL((surfacePrepassKdKernel<0, true, true>), grid, block, lds, s, a);
                      else       hipLaunchKernelGGL((surfacePrepassKdKernel<0, true, false>), grid, block, lds, s, a); }
  else              { if (defer) hipLaunchKernelGGL((surfacePrepassKdKernel<0, false, true>), grid, block, lds, s, a);
                      else       hipLaunchKernelGGL((surfacePrepassKdKernel<0, false, false>), grid, block, lds, s, a); }
  return hipGetLastError();
}

// the ambient-occlusion rays of the hits the pre-pass listed (a.aoRecs / a.aoCount); on the pre-pass' stream, or on another
// one behind an event (the module then runs them beside the march)
hipError_t launchAoRaysKd(const RenderArgs &a, int numBlocks, hipStream_t s)
{
  if (numBlocks <= 0) return hipSuccess;
  const size_t lds = kdLds(a.numXfChannels).total;
  const dim3 block(kKdBlock);
  const bool iso = isoOnly(a);
  const bool defer = a.aoRecs && a.aoCount;
  if (defer && a.fs.ao.enabled) {
    const int maxBlocks = 256 * (iso ? EXA_AO_ISO_WAVES : EXA_PREPASS_WAVES);      // what the device holds at once (workgroups per CU = waves per SIMD)
    const long long upper = ((long long)numBlocks * kTilePixels * 2 + kKdBlock - 1) / kKdBlock;
    const dim3 g2((unsigned)(upper < maxBlocks ? upper : maxBlocks));
    if (a.aoKeys) {
      // sorted: histogram of the rays' bins -> scan -> scatter of the ray indices -> trace in that order -> combine per hit
      const dim3 gs((unsigned)(upper < 2048 ? upper : 2048)), b256(256);
      if (hipError_t e = hipMemsetAsync(a.aoHist, 0, size_t(a.aoBins) * sizeof(uint32_t), s)) return e;   // a stale histogram would send the scatter out of range
      hipLaunchKernelGGL(aoKeyKernel, gs, b256, 0, s, a);
      hipLaunchKernelGGL(aoScanKernel, dim3(1), dim3(1024), 0, s, a.aoHist, a.aoBins);
      hipLaunchKernelGGL(aoScatterKernel, gs, b256, 0, s, a);
      if (iso) hipLaunchKernelGGL((aoRaysKdKernel<true, true>), g2, block, lds, s, a);
      else         hipLaunchKernelGGL((aoRaysKdKernel<false, true>), g2, block, lds, s, a);
      hipLaunchKernelGGL(aoFinalizeKernel, gs, b256, 0, s, a);
    } else {
      if (iso) hipLaunchKernelGGL((aoRaysKdKernel<true, false>), g2, block, lds, s, a);
      else         hipLaunchKernelGGL((aoRaysKdKernel<false, false>), g2, block, lds, s, a);
    }
  }
  return hipGetLastError();
}

#endif // !EXA_TU_ROPE

// the march over a.tileMap[0..numBlocks); `surf`: a surfaces pre-pass has filled a.surf / a.surfRnd
template <bool ROPE>
static hipError_t launchRenderKdT(const RenderArgs &a, int numBlocks, bool grad, bool fast, bool surf, int stats, hipStream_t s)
{
  if (numBlocks <= 0) return hipSuccess;
#ifndef EXA_LDS_PAD
#define EXA_LDS_PAD 0          // occupancy probe: extra bytes of LDS per workgroup (26 KB = 6, 28 KB = 5, 34 KB = 4 workgroups per CU)
#endif
  // 0: one primary channel; 1: several with at most two TF tables (3-entry stack, 6 workgroups per CU); 2: several, more tables.
  // The instrumented variants exist for 0 and 2 only.
  const int mode = a.p.numPrimaryChannels > 1 ? ((a.numXfChannels <= 2 && !stats) ? 1 : 2) : 0;
  const dim3 grid(numBlocks * (256 / kKdBlock)), block(kKdBlock);
  // the instrumented variants keep the general address arithmetic (fewer instantiations)
  // (the 32-bit rope variants also take for granted that the region records pack: see renderFrameKdKernel, PACKED_CT)
  const bool small = a.mul24 && a.addr32 && (!ROPE || (a.ropeAddr32 && a.leafBeginBits));
  // the LDS a launch asks for is the layout of the MULTI it instantiates
#define EXA_LAUNCH(G, F, M, I, S, A) hipLaunchKernelGGL((renderFrameKdKernel<G, F, M, I, S, A, 0, ROPE>), grid, block, \
                                                        marchLds((M) == 1, ROPE, a.numXfChannels, EXA_LDS_PAD).total, s, a)
#define EXA_PICK2(G, F, M, I) do { if (stats == 1) EXA_LAUNCH(G, F, (M ? 2 : 0), I, 1, false); else if (stats == 2) EXA_LAUNCH(G, F, (M ? 2 : 0), I, 2, false); \
                                   else if (small) EXA_LAUNCH(G, F, M, I, 0, true); else EXA_LAUNCH(G, F, M, I, 0, false); } while (0)
#define EXA_PICK(G, F, M) do { if (surf) EXA_PICK2(G, F, M, true); else EXA_PICK2(G, F, M, false); } while (0)
#define EXA_PICKM(G, F) do { if (mode == 0) EXA_PICK(G, F, 0); else if (mode == 1) EXA_PICK(G, F, 1); else EXA_PICK(G, F, 2); } while (0)
#if !EXA_EMPTY_CELLS
  // interleaved march: the module has built float[cell][numPrimaryChannels] (a.cellsIl); shipped kernel only
  const int nch = (a.cellsIl && !stats && a.p.numPrimaryChannels >= 2 && a.p.numPrimaryChannels <= 4) ? a.p.numPrimaryChannels : 0;
  if (nch) {
    // LDS: nch TF tables + a 4-entry stack + the queue = 28 / 30 / 32 KB per workgroup (5 workgroups per CU)
    const bool smallIl = small && a.il32;
#define EXA_IL4(G, F, I, A, N) hipLaunchKernelGGL((renderFrameKdKernel<G, F, 2, I, 0, A, N, ROPE>), grid, block, \
                                                  marchLds(false, ROPE, a.numXfChannels, EXA_LDS_PAD).total, s, a)
#define EXA_IL3(G, F, I, A) do { if (nch == 2) EXA_IL4(G, F, I, A, 2); else if (nch == 3) EXA_IL4(G, F, I, A, 3); else EXA_IL4(G, F, I, A, 4); } while (0)
#define EXA_IL2(G, F, I) do { if (smallIl) EXA_IL3(G, F, I, true); else EXA_IL3(G, F, I, false); } while (0)
#define EXA_IL1(G, F) do { if (surf) EXA_IL2(G, F, true); else EXA_IL2(G, F, false); } while (0)
    if (grad) { if (fast) EXA_IL1(true, true); else EXA_IL1(true, false); }
    else      { if (fast) EXA_IL1(false, true); else EXA_IL1(false, false); }
#undef EXA_IL1
#undef EXA_IL2
#undef EXA_IL3
#undef EXA_IL4
    return hipGetLastError();
  }
#endif
#if EXA_TU_ROPE && EXA_BASIS_FORM == 1 && !EXA_EMPTY_CELLS
  // cube scene (a.leafHdrCube: exa_frame.cpp, option cube_records): the shipped one-channel 32-bit rope march on the cube records
  if (ROPE && mode == 0 && !stats && small && fast && a.leafHdrCube) {
#define EXA_CUBE(G, I) hipLaunchKernelGGL((renderFrameKdKernel<G, true, 0, I, 0, true, 1, ROPE>), grid, block, \
                                          marchLds(false, ROPE, a.numXfChannels, EXA_LDS_PAD).total, s, a)
    if (grad) { if (surf) EXA_CUBE(true, true); else EXA_CUBE(true, false); }
    else      { if (surf) EXA_CUBE(false, true); else EXA_CUBE(false, false); }
#undef EXA_CUBE
    return hipGetLastError();
  }
#endif
  if (grad) { if (fast) EXA_PICKM(true, true); else EXA_PICKM(true, false); }
  else      { if (fast) EXA_PICKM(false, true); else EXA_PICKM(false, false); }
#undef EXA_PICKM
#undef EXA_PICK
#undef EXA_PICK2
#undef EXA_LAUNCH
  return hipGetLastError();
}
#if EXA_TU_ROPE
hipError_t launchRenderKdRope(const RenderArgs &a, int numBlocks, bool grad, bool fast, bool surf, int stats, hipStream_t s)
{ return launchRenderKdT<true>(a, numBlocks, grad, fast, surf, stats, s); }
#else
hipError_t launchRenderKd(const RenderArgs &a, int numBlocks, bool grad, bool fast, bool surf, int stats, hipStream_t s)
{ return launchRenderKdT<false>(a, numBlocks, grad, fast, surf, stats, s); }
#endif

} // namespace EXA_FORM_NS

#if EXA_BASIS_FORM == 0 && !EXA_EMPTY_CELLS && !EXA_TU_ROPE     // kernels that never sample are compiled once
using namespace form0;
// kd activity bits, one height class per launch (children before parents)
__global__ __launch_bounds__(256) void kdRefitKernel(KdNodeDev *nodes, KdNodeDev *marchNodes, const int32_t *nodeIds, int count,
                                                     const uint8_t *active, int which)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int id = nodeIds[i];
  const KdNodeDev n = nodes[id];
  const int sh = 2 + 2 * which;
  auto act = [&](int ref) -> uint32_t {
    if (ref == EXA_KD_EMPTY) return 0u;
    if (ref < 0) return active[~ref] ? 1u : 0u;
    return ((nodes[ref].word >> sh) & 3u) ? 1u : 0u;
  };
  const uint32_t bits = act(n.left) | (act(n.right) << 1);
  const uint32_t word = (n.word & ~(3u << sh)) | (bits << sh);
  nodes[id].word = word;
  if (marchNodes) marchNodes[id].word = word;      // same tree, leaf references replaced by region records
}

hipError_t launchKdRefit(KdNodeDev *nodes, KdNodeDev *marchNodes, const int32_t *nodeIds, int count, const uint8_t *active, int which, hipStream_t s)
{
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(kdRefitKernel, dim3((count + 255) / 256), dim3(256), 0, s, nodes, marchNodes, nodeIds, count, active, which);
  return hipGetLastError();
}

// activity bit of the rope leaves (the rope walk has no subtree bits to refit: every leaf carries its own flag), and the
// number of active regions, from which the module decides which walk a frame takes
__global__ __launch_bounds__(256) void ropeActivityKernel(RopeLeaf *leaves, uint32_t numRegions, const uint8_t *active, int which, uint32_t *activeCount)
{
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  const bool act = r < numRegions && active[r] != 0;
  if (leaves && r < numRegions) {
    const uint32_t f = leaves[r].flags;
    leaves[r].flags = (f & ~(1u << which)) | ((act ? 1u : 0u) << which);
  }
  if (activeCount) {
    const unsigned long long m = __ballot(act);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(activeCount, (uint32_t)__popcll(m));
  }
}
hipError_t launchRopeActivity(RopeLeaf *leaves, uint32_t numRegions, const uint8_t *active, int which, uint32_t *activeCount, hipStream_t s)
{
  if (numRegions == 0) return hipSuccess;
  hipLaunchKernelGGL(ropeActivityKernel, dim3((numRegions + 255) / 256), dim3(256), 0, s, leaves, numRegions, active, which, activeCount);
  return hipGetLastError();
}
#endif

#if !EXA_TU_ROPE
namespace EXA_FORM_NS {

// ------------------------------------------------------------------------
// computeTraces (exabrick.cu:1531-1574) with sampleDirection (:945-963): RK4 advection of trace i
// through the vector field (tracerChannels), one thread per trace.  The reference runs this inside
// renderFrame in the thread of pixel i; the new point is never read by that frame's rays (the
// streamline BVH only holds earlier timesteps), so a separate launch gives the same traces and
// keeps them identical on every GPU of a sharded frame.
// ------------------------------------------------------------------------
__device__ __forceinline__ bool sampleDirection(Ctx<false> &C, V3 pos, V3 &result)
{
  Ray ray; ray.org = pos; ray.dir = mk(1.f, 1.f, 1.f); ray.tmin = 0.f; ray.tmax = 2e-10f;
  const RegionHit prd = traceRegion(C, C.a->volNodes, ray);
  result = mk(0.f, 0.f, 0.f);
  if (prd.leafID < 0) return false;                               // reference: region[-1], undefined
  const RegionInfo ri = C.a->sc.regionInfo[prd.leafID];
  V3 unused;
  float r0 = 0.f, r1 = 0.f, r2 = 0.f;
  bool ok = samplePoint<false, false>(C, r0, unused, ri, pos, C.a->tracerChannels[0]);
  if (ok) ok = samplePoint<false, false>(C, r1, unused, ri, pos, C.a->tracerChannels[1]);
  if (ok) ok = samplePoint<false, false>(C, r2, unused, ri, pos, C.a->tracerChannels[2]);
  result = mk(r0, r1, r2);
  return ok;
}

__global__ __launch_bounds__(256) void computeTracesKernel(const RenderArgs a, float *traces, int count)
{
  __shared__ int stackLds[kStackDepth * 256];                     // traceRegion's per-lane stack, stride 256
  const int i = blockIdx.x * 256 + threadIdx.x;
  Ctx<false> C;
  C.a = &a; C.xfLds = nullptr; C.stack = stackLds + threadIdx.x; C.guardTripped = false;
  if (i >= count) return;
  const int t = a.timestep, NT = a.numTimesteps;
  if (!(t < NT)) return;
  V3 p = mk(traces + 3 * (size_t(i) * NT + (t - 1)));
  const V3 pp = p;
  if (p.x < 2e10f) {
    bool valid = true;
    V3 k1, k2, k3, k4;
    valid &= sampleDirection(C, p, k1);
    k1 = a.steplen * k1;
    const V3 ptry1 = p + .5f * k1;
    valid &= sampleDirection(C, ptry1, k2);
    k2 = a.steplen * k2;
    const V3 ptry2 = p + .5f * k2;
    valid &= sampleDirection(C, ptry2, k3);
    k3 = a.steplen * k3;
    const V3 ptry3 = p + k3;
    valid &= sampleDirection(C, ptry3, k4);
    k4 = a.steplen * k4;
    p = p + (1 / 6.f) * (((k1 + 2.f * k2) + 2.f * k3) + k4);
    const bool inside = p.x >= a.worldLo[0] && p.y >= a.worldLo[1] && p.z >= a.worldLo[2]
                     && p.x <= a.worldHi[0] && p.y <= a.worldHi[1] && p.z <= a.worldHi[2];
    if (!valid || !inside || length(p - pp) < 1e-10f) p = mk(2e10f, 2e10f, 2e10f);
  }
  float *dst = traces + 3 * (size_t(i) * NT + t);
  dst[0] = p.x; dst[1] = p.y; dst[2] = p.z;
}

hipError_t launchComputeTraces(const RenderArgs &a, float *traces, int count, hipStream_t s)
{
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(computeTracesKernel, dim3((count + 255) / 256), dim3(256), 0, s, a, traces, count);
  return hipGetLastError();
}

} // namespace EXA_FORM_NS
#endif // !EXA_TU_ROPE

#if EXA_BASIS_FORM == 0 && !EXA_EMPTY_CELLS && !EXA_TU_ROPE
// ------------------------------------------------------------------------
// Region activity: the OPTIX_BOUNDS_PROGRAMs (exabrick.cu:250-312, 373-402)
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void volumeActivityKernel(DeviceScene sc, ExaHipFrameState fs, ExaHipParams p,
                                                            const float4 *xf, uint8_t *active, float tfFracMagic)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float4 *xfLds = reinterpret_cast<float4 *>(smem);
  for (int i = threadIdx.x; i < p.numChannels * EXA_NUM_XF_VALUES; i += 256) xfLds[i] = xf[i];
  __syncthreads();
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= sc.numRegions) return;
  const float2 vr = sc.valueRange[r];
  bool act = false;
  for (int c = 0; c < p.numChannels && !act; ++c) {           // activeForVolumeSampling :250-281
    const float dlo = fs.xfDomain[c][0], dhi = fs.xfDomain[c][1];
    if (vr.x > dhi) continue;
    if (vr.y < dlo) continue;
    const float scaled_lo = (vr.x - dlo) / ((dhi - dlo) + 1e-20f);
    const float scaled_hi = (vr.y - dlo) / ((dhi - dlo) + 1e-20f);
    const int idx_lo = min(EXA_NUM_XF_VALUES - 1, max(0, int(scaled_lo * (EXA_NUM_XF_VALUES - 1))));
    const int idx_hi = min(EXA_NUM_XF_VALUES - 1, max(0, int(scaled_hi * (EXA_NUM_XF_VALUES - 1)) + 1));
    for (int i = idx_lo; i <= idx_hi; i++) {
      float cellValue = float(i) / (EXA_NUM_XF_VALUES - 1);
      cellValue *= dhi - dlo;
      cellValue += dlo;
      const Color4 rgba = lookupXF(xfLds, fs, cellValue, c, tfFracMagic);
      if (rgba.w > 0.f) { act = true; break; }
    }
  }
  active[r] = (uint8_t)(p.spaceSkippingEnabled ? (act ? 1 : 0) : 1);
}

__global__ __launch_bounds__(256) void isoActivityKernel(DeviceScene sc, ExaHipFrameState fs, uint8_t *active)
{
  const uint32_t r = blockIdx.x * 256u + threadIdx.x;
  if (r >= sc.numRegions) return;
  const float2 vr = sc.valueRange[r];
  bool act = false;
  for (int i = 0; i < EXA_MAX_ISO_SURFACES; i++)
    if (fs.iso[i].enabled && fs.iso[i].value >= vr.x && fs.iso[i].value <= vr.y) act = true;
  active[r] = act ? 1 : 0;
}

hipError_t launchVolumeActivity(const DeviceScene &sc, const ExaHipFrameState &fs, const ExaHipParams &p,
                                const float4 *xf, uint8_t *active, float tfFracMagic, hipStream_t s)
{
  if (sc.numRegions == 0) return hipSuccess;
  const size_t lds = size_t(p.numChannels) * EXA_NUM_XF_VALUES * sizeof(float4);
  hipLaunchKernelGGL(volumeActivityKernel, dim3((sc.numRegions + 255) / 256), dim3(256), lds, s, sc, fs, p, xf, active, tfFracMagic);
  return hipGetLastError();
}
hipError_t launchIsoActivity(const DeviceScene &sc, const ExaHipFrameState &fs, uint8_t *active, hipStream_t s)
{
  if (sc.numRegions == 0) return hipSuccess;
  hipLaunchKernelGGL(isoActivityKernel, dim3((sc.numRegions + 255) / 256), dim3(256), 0, s, sc, fs, active);
  return hipGetLastError();
}

// ------------------------------------------------------------------------
// LBVH refit: one launch per height class, children before parents.
// ------------------------------------------------------------------------
__device__ __forceinline__ void childBox(const BvhNode *nodes, int child, const float *domain, const uint8_t *active,
                                         float lo[3], float hi[3])
{
  lo[0] = lo[1] = lo[2] = FLT_MAX;
  hi[0] = hi[1] = hi[2] = -FLT_MAX;
  if (child == INT32_MIN) return;                    // padding child of a one-region scene
  if (child < 0) {
    const int r = ~child;
    if (!active[r]) return;
    for (int k = 0; k < 3; k++) { lo[k] = domain[6 * size_t(r) + k]; hi[k] = domain[6 * size_t(r) + 3 + k]; }
    return;
  }
  const BvhNode &n = nodes[child];
  const float l0[3] = { n.q0.x, n.q0.y, n.q0.z }, h0[3] = { n.q0.w, n.q1.x, n.q1.y };
  const float l1[3] = { n.q1.z, n.q1.w, n.q2.x }, h1[3] = { n.q2.y, n.q2.z, n.q2.w };
  const bool e0 = l0[0] > h0[0], e1 = l1[0] > h1[0];
  for (int k = 0; k < 3; k++) {
    if (!e0) { lo[k] = fminf(lo[k], l0[k]); hi[k] = fmaxf(hi[k], h0[k]); }
    if (!e1) { lo[k] = fminf(lo[k], l1[k]); hi[k] = fmaxf(hi[k], h1[k]); }
  }
}

__global__ __launch_bounds__(256) void refitKernel(BvhNode *nodes, const int32_t *nodeIds, int count,
                                                   const float *domain, const uint8_t *active)
{
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int id = nodeIds[i];
  BvhNode n = nodes[id];
  float l0[3], h0[3], l1[3], h1[3];
  childBox(nodes, n.child0, domain, active, l0, h0);
  childBox(nodes, n.child1, domain, active, l1, h1);
  n.q0 = make_float4(l0[0], l0[1], l0[2], h0[0]);
  n.q1 = make_float4(h0[1], h0[2], l1[0], l1[1]);
  n.q2 = make_float4(l1[2], h1[0], h1[1], h1[2]);
  nodes[id] = n;
}

hipError_t launchRefit(BvhNode *nodes, const int32_t *nodeIds, int count, const float *domain,
                       const uint8_t *active, hipStream_t s)
{
  if (count <= 0) return hipSuccess;
  hipLaunchKernelGGL(refitKernel, dim3((count + 255) / 256), dim3(256), 0, s, nodes, nodeIds, count, domain, active);
  return hipGetLastError();
}

// ------------------------------------------------------------------------
// Re-laying the cell values brick by brick (option brick_order): brick b's cells move from srcBegin[b] to dstBegin[b] in
// every field; then the `begin` words of the brick records and of the march headers are patched.  The kernels find a
// cell only through its brick's `begin` (exabrick.cu:581-594, Brick.h:57-70), so the order of the bricks in memory is the
// module's to choose.
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void permuteBricksKernel(const float *src, float *dst, const uint32_t *srcBegin, const uint32_t *dstBegin,
                                                           const int4 *bricks, unsigned long long totalCells, int numFields)
{
  const size_t b = blockIdx.x;
  const int4 b0 = bricks[2 * b], b1 = bricks[2 * b + 1];           // (lower.xyz, size.x) (size.yz, level, begin)
  const unsigned long long vol = (unsigned long long)b0.w * (unsigned long long)b1.x * (unsigned long long)b1.y;
  const unsigned long long sb = srcBegin[b], db = dstBegin[b];
  for (int f = 0; f < numFields; f++)
    for (unsigned long long i = threadIdx.x; i < vol; i += 256) dst[f * totalCells + db + i] = src[f * totalCells + sb + i];
}
__global__ __launch_bounds__(256) void patchBeginKernel(int4 *bricks, unsigned long long numBricks, int4 *leafHdr, const int32_t *leafList,
                                                        unsigned long long leafListSize, const uint32_t *dstBegin)
{
  const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
  if (i < numBricks) bricks[2 * i + 1].w = (int)dstBegin[i];
  if (i < leafListSize) leafHdr[2 * i + 1].w = (int)dstBegin[leafList[i]];
}
hipError_t launchPermuteBricks(const float *src, float *dst, const uint32_t *srcBegin, const uint32_t *dstBegin, int4 *bricks,
                               unsigned long long numBricks, int4 *leafHdr, const int32_t *leafList, unsigned long long leafListSize,
                               unsigned long long totalCells, int numFields, hipStream_t s)
{
  if (numBricks == 0) return hipSuccess;
  hipLaunchKernelGGL(permuteBricksKernel, dim3((unsigned)numBricks), dim3(256), 0, s, src, dst, srcBegin, dstBegin, bricks, totalCells, numFields);
  const unsigned long long n = numBricks > leafListSize ? numBricks : leafListSize;
  hipLaunchKernelGGL(patchBeginKernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, bricks, numBricks, leafHdr, leafList, leafListSize, dstBegin);
  return hipGetLastError();
}
// the same for the cube records (exa_cube.h): the brick's index begin / S^3 above the nine level bits
__global__ __launch_bounds__(256) void patchCubeRecordsKernel(int4 *leafHdrCube, const int32_t *leafList, unsigned long long leafListSize,
                                                              const uint32_t *dstBegin, int cubeLog2)
{
  const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
  if (i < leafListSize) leafHdrCube[i].w = (int)(((dstBegin[leafList[i]] >> (3 * cubeLog2)) << 9) | ((uint32_t)leafHdrCube[i].w & 0x1ffu));
}
hipError_t launchPatchCubeRecords(int4 *leafHdrCube, const int32_t *leafList, unsigned long long leafListSize,
                                  const uint32_t *dstBegin, int cubeLog2, hipStream_t s)
{
  if (leafListSize == 0) return hipSuccess;
  hipLaunchKernelGGL(patchCubeRecordsKernel, dim3((unsigned)((leafListSize + 255) / 256)), dim3(256), 0, s, leafHdrCube, leafList,
                     leafListSize, dstBegin, cubeLog2);
  return hipGetLastError();
}

// ------------------------------------------------------------------------
// channel-interleaved copy of the primary channels for the multi-channel march: out[cell][c] = field_c[cell]
// (exabrick.cu:581-594 reads field c at scalarBuffers[offset[c] + index]; the copy only changes where a value lives)
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void interleaveKernel(DeviceScene sc, unsigned long long totalCells, int nch, float *out)
{
  const unsigned long long n = totalCells * (unsigned long long)nch;
  for (unsigned long long i = blockIdx.x * 256ull + threadIdx.x; i < n; i += (unsigned long long)gridDim.x * 256ull) {
    const unsigned long long cell = i / (unsigned)nch;
    const int c = (int)(i - cell * (unsigned)nch);
    out[i] = sc.scalars[sc.channelOffset[c] + cell];
  }
}

hipError_t launchInterleave(const DeviceScene &sc, unsigned long long totalCells, int nch, float *out, hipStream_t s)
{
  if (totalCells == 0) return hipSuccess;
  hipLaunchKernelGGL(interleaveKernel, dim3(256 * 64), dim3(256), 0, s, sc, totalCells, nch, out);
  return hipGetLastError();
}

// ------------------------------------------------------------------------
// root side of the multi-GPU gather: tile-major shards -> row-major image
// ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void untileKernel(const uint32_t *gathered, unsigned long long shardStride,
                                                    int world, int W, int H, int tilesX, uint32_t *out)
{
  const int tile = blockIdx.x;
  const int tx = tile % tilesX, ty = tile / tilesX;
  const int inX = threadIdx.x & 15, inY = threadIdx.x >> 4;
  const int px = tx * kTile + inX, py = ty * kTile + inY;
  if (px >= W || py >= H) return;
  const int rank = tile % world;
  // the render kernel's in-tile order: wave (w&1,w>>1) 8x8 blocks, lane = x + 8*y
  out[size_t(px) + size_t(W) * py]
      = gathered[size_t(rank) * shardStride + size_t(tile / world) * kTilePixels + (inY * kTile + inX)];
}

hipError_t launchUntile(const uint32_t *gathered, unsigned long long shardStride, int world,
                        int W, int H, uint32_t *out, hipStream_t s)
{
  const int tilesX = (W + kTile - 1) / kTile, tilesY = (H + kTile - 1) / kTile;
  hipLaunchKernelGGL(untileKernel, dim3(tilesX * tilesY), dim3(256), 0, s, gathered, shardStride, world, W, H, tilesX, out);
  return hipGetLastError();
}

// an empty one-thread kernel that only exists to be seen in a profiler's dispatch list (option "profile_marker":
// bench.py brackets its timed frames with two of them, so that counters can be summed over exactly those frames)
__global__ void profileMarkerKernel(int tag) { (void)tag; }
hipError_t launchProfileMarker(int tag, hipStream_t s)
{
  hipLaunchKernelGGL(profileMarkerKernel, dim3(1), dim3(1), 0, s, tag);
  return hipGetLastError();
}
#endif // EXA_BASIS_FORM == 0 && !EXA_EMPTY_CELLS
#endif // EXA_TU_SAMPLE, EXA_TU_STREAM
} // namespace exa
