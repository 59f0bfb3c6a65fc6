// exa_isomesh.hip — the kernels of exa_hip_isosurface: classify, count, scan, emit (exa_isomesh.h describes the pipeline,
// include/exa_hip.h the contract).  A translation unit of its own: nothing of the renderer or of the probes is compiled
// here, the lattice values arrive in a device buffer.  Compiled with -ffp-contract=off: a vertex position is
// P(p) + t * (P(q) - P(p)) with every operation rounded separately.  Behind them the kernels of exa_hip_isolines, the same
// pipeline on the squares of a plane lattice (isoline...Kernel), which shares the block scan and the scans; the union-find of
// exa_hip_regions and, behind it, the ascent, the rounds and the table of exa_hip_basins (isoBasin...Kernel); the stretch stencil of exa_hip_flowmap (isoLatticeStretchKernel), another pass over a lattice that does not
// depend on the basis form; and the critical points of a flow on a lattice (exa_hip_critical_points, isoCritical...Kernel),
// which place their output with the same scans.
#include "exa_isomesh.h"

#include <type_traits>

namespace exa {
namespace {

// ---- the six tetrahedra of a cube: permutation (a,b,c) of the axes in lexicographic order; tet vertices v0 = origin,
// v1 = v0 + e_a, v2 = v1 + e_b, v3 = v2 + e_c, as corner codes dx + 2 dy + 4 dz ----
constexpr int kPermAxis[6][3] = { { 0, 1, 2 }, { 0, 2, 1 }, { 1, 0, 2 }, { 1, 2, 0 }, { 2, 0, 1 }, { 2, 1, 0 } };
constexpr int kPermParity[6] = { 0, 1, 1, 0, 0, 1 };        // inversions mod 2

constexpr int tetCorner(int tet, int v)
{
  return v == 0 ? 0 : (v == 1 ? (1 << kPermAxis[tet][0]) : (v == 2 ? ((1 << kPermAxis[tet][0]) | (1 << kPermAxis[tet][1])) : 7));
}
// the six edges of a tet (m < n): 01, 02, 03, 12, 13, 23
constexpr int kEdgeLo[6] = { 0, 0, 0, 1, 1, 2 }, kEdgeHi[6] = { 1, 2, 3, 2, 3, 3 };
constexpr int edgeOf(int m, int n)
{
  const int lo = m < n ? m : n, hi = m < n ? n : m;
  return lo == 0 ? hi - 1 : (lo == 1 ? hi + 1 : 5);
}

// the triangles of a tet whose vertex n is inside iff bit n of `pat` is set, as edge numbers; `par` = parity of the tet's
// permutation.  The rules of the contract, evaluated by the compiler.
struct TetCase { int n; int tri[2][3]; };
constexpr int popc4(int p) { return (p & 1) + ((p >> 1) & 1) + ((p >> 2) & 1) + ((p >> 3) & 1); }
constexpr TetCase tetCase(int pat, int par)
{
  TetCase c = { 0, { { 0, 0, 0 }, { 0, 0, 0 } } };
  const int cnt = popc4(pat);
  if (cnt == 1 || cnt == 3) {
    const int single = cnt == 1 ? pat : (~pat & 15);
    const int s = single == 1 ? 0 : (single == 2 ? 1 : (single == 4 ? 2 : 3));
    int o[3] = { 0, 0, 0 }, k = 0;
    for (int v = 0; v < 4; v++) if (v != s) o[k++] = v;
    const int rev = (s & 1) ^ par ^ (cnt == 3 ? 1 : 0);      // parity(s,o0,o1,o2) = s: s stands in front of s smaller ones
    c.n = 1;
    for (int j = 0; j < 3; j++) c.tri[0][j] = edgeOf(s, o[rev ? 2 - j : j]);
  } else if (cnt == 2) {
    int in[2] = { 0, 0 }, out[2] = { 0, 0 }, ki = 0, ko = 0;
    for (int v = 0; v < 4; v++) { if ((pat >> v) & 1) in[ki++] = v; else out[ko++] = v; }
    const int seq[4] = { in[0], in[1], out[0], out[1] };
    int inv = 0;
    for (int i = 0; i < 4; i++) for (int j = i + 1; j < 4; j++) inv += seq[i] > seq[j] ? 1 : 0;
    const int rev = (inv & 1) ^ par;
    const int q[4] = { edgeOf(in[0], out[0]), edgeOf(in[0], out[1]), edgeOf(in[1], out[1]), edgeOf(in[1], out[0]) };
    const int r[4] = { q[rev ? 3 : 0], q[rev ? 2 : 1], q[rev ? 1 : 2], q[rev ? 0 : 3] };
    c.n = 2;
    c.tri[0][0] = r[0]; c.tri[0][1] = r[1]; c.tri[0][2] = r[2];
    c.tri[1][0] = r[0]; c.tri[1][1] = r[2]; c.tri[1][2] = r[3];
  }
  return c;
}

// the cubes that hold the tet edge p -> p + code: origins p - m for every corner code m disjoint from `code`; bit m
constexpr uint32_t edgeCubes(int code)
{
  uint32_t r = 0;
  for (int m = 0; m < 8; m++) if ((m & code) == 0) r |= 1u << m;
  return r;
}

// exclusive prefix sum over the block's 256 lanes; every lane calls it
__device__ __forceinline__ uint32_t blockScan(uint32_t v, uint32_t &total, uint32_t *lds)
{
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(inc, o, 64);
    if (lane >= unsigned(o)) inc += t;
  }
  if (lane == 63u) lds[wave] = inc;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (unsigned k = 0; k < kIsoBlock / 64; k++) {
    const uint32_t t = lds[k];
    if (k < wave) base += t;
    total += t;
  }
  __syncthreads();
  return base + inc - v;
}

__device__ __forceinline__ size_t cornerOffset(const IsoMeshArgs &a, int m)
{
  return size_t(m & 1) + size_t((m >> 1) & 1) * a.nx + size_t(m >> 2) * (size_t(a.nx) * a.ny);
}

template <int TET>
__device__ __forceinline__ uint32_t tetPattern(uint32_t inside)
{
  return ((inside >> tetCorner(TET, 0)) & 1u) | (((inside >> tetCorner(TET, 1)) & 1u) << 1) |
         (((inside >> tetCorner(TET, 2)) & 1u) << 2) | (((inside >> tetCorner(TET, 3)) & 1u) << 3);
}
__device__ __forceinline__ uint32_t tetTriangles(uint32_t pat)
{
  const uint32_t c = __popc(pat);
  return c == 2u ? 2u : (c & 1u);           // 1 or 3 inside: one triangle, 2: a quad, 0 or 4: none
}

// ---- cube pass ----
__global__ __launch_bounds__(kIsoBlock) void isoCubeKernel(const IsoMeshArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  uint32_t count = 0;
  if (L < a.numPoints) {
    const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
    uint32_t info = 0;
    if (i + 1 < a.nx && j + 1 < a.ny && k + 1 < a.nz) {
      const float *v = a.values + L;
      bool finite = true;
      uint32_t inside = 0;
#pragma unroll
      for (int m = 0; m < 8; m++) {
        const float x = v[cornerOffset(a, m)];
        finite = finite && __builtin_isfinite(x);
        inside |= (x >= a.iso ? 1u : 0u) << m;
      }
      if (finite) {
        count = tetTriangles(tetPattern<0>(inside)) + tetTriangles(tetPattern<1>(inside)) + tetTriangles(tetPattern<2>(inside)) +
                tetTriangles(tetPattern<3>(inside)) + tetTriangles(tetPattern<4>(inside)) + tetTriangles(tetPattern<5>(inside));
        info = 0x80u | count;
      }
    }
    a.cubeInfo[L] = uint8_t(info);
  }
  uint32_t total;
  (void)blockScan(count, total, lds);
  if (threadIdx.x == 0) a.blockCount[a.numBlocks + blockIdx.x] = total;
}

// ---- point pass ----
__global__ __launch_bounds__(kIsoBlock) void isoPointKernel(const IsoMeshArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  uint32_t mask = 0;
  if (L < a.numPoints) {
    const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
    uint32_t cubes = 0;                       // bit m: the cube with origin p - m is valid
#pragma unroll
    for (int m = 0; m < 8; m++)
      if (i >= uint32_t(m & 1) && j >= uint32_t((m >> 1) & 1) && k >= uint32_t(m >> 2))
        cubes |= uint32_t(a.cubeInfo[L - cornerOffset(a, m)] >> 7) << m;
    if (cubes) {
      const float *v = a.values + L;
      const bool inP = v[0] >= a.iso;
#pragma unroll
      for (int code = 1; code < 8; code++)
        if (cubes & edgeCubes(code)) {          // then q = p + code is a lattice point, and both values are finite
          const bool inQ = v[cornerOffset(a, code)] >= a.iso;
          if (inQ != inP) mask |= 1u << (code - 1);
        }
    }
    a.mask[L] = uint8_t(mask);
  }
  uint32_t total;
  const uint32_t before = blockScan(__popc(mask), total, lds);
  if (L < a.numPoints) a.rel[L] = uint16_t(before);
  if (threadIdx.x == 0) a.blockCount[blockIdx.x] = total;
}

// ---- scans: one row of the grid per count (the iso-surface's: blockIdx.y = 0 vertices, 1 triangles) ----
__global__ __launch_bounds__(kIsoBlock) void isoScanChunksKernel(const IsoScanArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  constexpr uint32_t per = kIsoChunk / kIsoBlock;
  const uint32_t *count = a.blockCount + size_t(blockIdx.y) * a.numBlocks;
  uint32_t *base = a.blockBase + size_t(blockIdx.y) * a.numBlocks;
  const uint32_t first = blockIdx.x * kIsoChunk + threadIdx.x * per;
  uint32_t c[per], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < per; k++) {
    c[k] = first + k < a.numBlocks ? count[first + k] : 0u;
    sum += c[k];
  }
  uint32_t total;
  uint32_t run = blockScan(sum, total, lds);
#pragma unroll
  for (uint32_t k = 0; k < per; k++) {
    if (first + k < a.numBlocks) base[first + k] = run;
    run += c[k];
  }
  if (threadIdx.x == 0) a.chunkBase[size_t(blockIdx.y) * a.numChunks + blockIdx.x] = total;     // the sum; scanned in place next
}

__global__ __launch_bounds__(kIsoBlock) void isoScanTopKernel(const IsoScanArgs a)
{
  __shared__ uint64_t sums[kIsoBlock];
  uint64_t *chunk = a.chunkBase + size_t(blockIdx.x) * a.numChunks;
  const uint32_t per = (a.numChunks + kIsoBlock - 1) / kIsoBlock;
  const uint32_t first = threadIdx.x * per;
  uint64_t sum = 0;
  for (uint32_t k = 0; k < per; k++)
    if (first + k < a.numChunks) sum += chunk[first + k];
  sums[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t run = 0;
    for (uint32_t t = 0; t < kIsoBlock; t++) { const uint64_t s = sums[t]; sums[t] = run; run += s; }
    a.totals[blockIdx.x] = run;
  }
  __syncthreads();
  uint64_t run = sums[threadIdx.x];
  for (uint32_t k = 0; k < per; k++)
    if (first + k < a.numChunks) { const uint64_t s = chunk[first + k]; chunk[first + k] = run; run += s; }
}

// ---- emit ----
__device__ __forceinline__ uint64_t blockStart(const IsoMeshArgs &a, uint32_t which, uint32_t block)
{
  return a.chunkBase[size_t(which) * a.numChunks + block / kIsoChunk] + a.blockBase[size_t(which) * a.numBlocks + block];
}

__global__ __launch_bounds__(kIsoBlock) void isoEmitVerticesKernel(const IsoMeshArgs a)
{
  if (a.blockCount[blockIdx.x] == 0) return;          // the same for the whole block
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  const uint32_t mask = a.mask[L];
  if (!mask) return;
  const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
  const float *v = a.values + L;
  const float vp = v[0];
  const float px = a.lo[0] + (float(i) + 0.5f) * a.step[0], py = a.lo[1] + (float(j) + 0.5f) * a.step[1],
              pz = a.lo[2] + (float(k) + 0.5f) * a.step[2];
  float *out = a.vertices + 3 * (blockStart(a, 0, blockIdx.x) + a.rel[L]);
#pragma unroll
  for (int code = 1; code < 8; code++)
    if (mask & (1u << (code - 1))) {
      const float vq = v[cornerOffset(a, code)];
      const float t = (a.iso - vp) / (vq - vp);
      const float qx = a.lo[0] + (float(i + uint32_t(code & 1)) + 0.5f) * a.step[0];
      const float qy = a.lo[1] + (float(j + uint32_t((code >> 1) & 1)) + 0.5f) * a.step[1];
      const float qz = a.lo[2] + (float(k + uint32_t(code >> 2)) + 0.5f) * a.step[2];
      out[0] = px + t * (qx - px);
      out[1] = py + t * (qy - py);
      out[2] = pz + t * (qz - pz);
      out += 3;
    }
}

template <int PAT, int PAR>
__device__ __forceinline__ void emitCase(const int32_t (&e)[6], int32_t *&out)
{
  constexpr TetCase c = tetCase(PAT, PAR);
#pragma unroll
  for (int t = 0; t < c.n; t++) {
    out[0] = e[c.tri[t][0]]; out[1] = e[c.tri[t][1]]; out[2] = e[c.tri[t][2]];
    out += 3;
  }
}

// vb[m], mk[m]: index of the first vertex and edge mask of the lattice point origin + m
template <int TET>
__device__ __forceinline__ void emitTet(uint32_t inside, const uint32_t (&vb)[7], const uint32_t (&mk)[7], int32_t *&out)
{
  const uint32_t pat = tetPattern<TET>(inside);
  if (pat == 0u || pat == 15u) return;
  int32_t e[6];
#pragma unroll
  for (int n = 0; n < 6; n++) {
    const int owner = tetCorner(TET, kEdgeLo[n]);
    const int code = tetCorner(TET, kEdgeHi[n]) ^ owner;
    e[n] = int32_t(vb[owner] + __popc(mk[owner] & ((1u << (code - 1)) - 1u)));
  }
  constexpr int P = kPermParity[TET];
  switch (pat) {
  case 1: emitCase<1, P>(e, out); break;
  case 2: emitCase<2, P>(e, out); break;
  case 3: emitCase<3, P>(e, out); break;
  case 4: emitCase<4, P>(e, out); break;
  case 5: emitCase<5, P>(e, out); break;
  case 6: emitCase<6, P>(e, out); break;
  case 7: emitCase<7, P>(e, out); break;
  case 8: emitCase<8, P>(e, out); break;
  case 9: emitCase<9, P>(e, out); break;
  case 10: emitCase<10, P>(e, out); break;
  case 11: emitCase<11, P>(e, out); break;
  case 12: emitCase<12, P>(e, out); break;
  case 13: emitCase<13, P>(e, out); break;
  default: emitCase<14, P>(e, out); break;
  }
}

__global__ __launch_bounds__(kIsoBlock) void isoEmitTrianglesKernel(const IsoMeshArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  if (a.blockCount[a.numBlocks + blockIdx.x] == 0) return;      // the same for the whole block
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  const uint32_t count = L < a.numPoints ? (a.cubeInfo[L] & 0x7fu) : 0u;
  uint32_t total;
  const uint32_t before = blockScan(count, total, lds);
  if (!count) return;
  const float *v = a.values + L;
  uint32_t inside = 0;
#pragma unroll
  for (int m = 0; m < 8; m++) inside |= (v[cornerOffset(a, m)] >= a.iso ? 1u : 0u) << m;
  uint32_t vb[7], mk[7];
#pragma unroll
  for (int m = 0; m < 7; m++) {
    const uint32_t Lp = L + uint32_t(cornerOffset(a, m));
    vb[m] = uint32_t(blockStart(a, 0, Lp / kIsoBlock)) + a.rel[Lp];     // the vertex count fits 31 bits (checked before the emit)
    mk[m] = a.mask[Lp];
  }
  int32_t *out = a.triangles + 3 * (blockStart(a, 1, blockIdx.x) + before);
  emitTet<0>(inside, vb, mk, out);
  emitTet<1>(inside, vb, mk, out);
  emitTet<2>(inside, vb, mk, out);
  emitTet<3>(inside, vb, mk, out);
  emitTet<4>(inside, vb, mk, out);
  emitTet<5>(inside, vb, mk, out);
}

// ---- contour lines on a plane lattice (exa_hip_isolines): marching triangles, the passes of exa_isomesh.h ----
// the triangles of a square: T0 = permutation (u,v), corners 0, 1, 3 (dx + 2 dy), parity 0; T1 = (v,u), corners 0, 2, 3, parity 1
constexpr int kTriCorner[2][3] = { { 0, 1, 3 }, { 0, 2, 3 } };

__device__ __forceinline__ size_t lineCornerOffset(const IsoLineArgs &a, int m)
{
  return size_t(m & 1) + size_t(m >> 1) * a.nu;
}

// lattice point (i,j), component c: (origin + (float(i) + 0.5f) * du) + (float(j) + 0.5f) * dv
__device__ __forceinline__ float linePosition(const IsoLineArgs &a, uint32_t i, uint32_t j, int c)
{
  return (a.origin[c] + (float(i) + 0.5f) * a.du[c]) + (float(j) + 0.5f) * a.dv[c];
}

template <int TRI>
__device__ __forceinline__ uint32_t triPattern(uint32_t inside)
{
  return ((inside >> kTriCorner[TRI][0]) & 1u) | (((inside >> kTriCorner[TRI][1]) & 1u) << 1) | (((inside >> kTriCorner[TRI][2]) & 1u) << 2);
}
__device__ __forceinline__ uint32_t triSegments(uint32_t pat) { return (pat != 0u && pat != 7u) ? 1u : 0u; }

__global__ __launch_bounds__(kIsoBlock) void isolinePositionsKernel(const IsoLineArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  const uint32_t i = L % a.nu, j = L / a.nu;
  float *out = a.positions + 3 * size_t(L);
  out[0] = linePosition(a, i, j, 0);
  out[1] = linePosition(a, i, j, 1);
  out[2] = linePosition(a, i, j, 2);
}

__global__ __launch_bounds__(kIsoBlock) void isolineSquareKernel(const IsoLineArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  uint32_t count = 0;
  if (L < a.numPoints) {
    const uint32_t i = L % a.nu, j = L / a.nu;
    uint32_t info = 0;
    if (i + 1 < a.nu && j + 1 < a.nv) {
      const float *v = a.values + L;
      bool finite = true;
      uint32_t inside = 0;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const float x = v[lineCornerOffset(a, m)];
        finite = finite && __builtin_isfinite(x);
        inside |= (x >= a.iso ? 1u : 0u) << m;
      }
      if (finite) {
        count = triSegments(triPattern<0>(inside)) + triSegments(triPattern<1>(inside));
        info = 0x80u | count;
      }
    }
    a.squareInfo[L] = uint8_t(info);
  }
  uint32_t total;
  (void)blockScan(count, total, lds);
  if (threadIdx.x == 0) a.blockCount[a.numBlocks + blockIdx.x] = total;
}

__global__ __launch_bounds__(kIsoBlock) void isolinePointKernel(const IsoLineArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  uint32_t mask = 0;
  if (L < a.numPoints) {
    const uint32_t i = L % a.nu, j = L / a.nu;
    uint32_t squares = 0;                     // bit m: the square with origin p - m is valid (m = 3 holds no edge of p)
#pragma unroll
    for (int m = 0; m < 3; m++)
      if (i >= uint32_t(m & 1) && j >= uint32_t(m >> 1))
        squares |= uint32_t(a.squareInfo[L - lineCornerOffset(a, m)] >> 7) << m;
    if (squares) {
      const float *v = a.values + L;
      const bool inP = v[0] >= a.iso;
#pragma unroll
      for (int code = 1; code < 4; code++)
        if (squares & edgeCubes(code)) {        // then q = p + code is a lattice point, and both values are finite
          const bool inQ = v[lineCornerOffset(a, code)] >= a.iso;
          if (inQ != inP) mask |= 1u << (code - 1);
        }
    }
    a.mask[L] = uint8_t(mask);
  }
  uint32_t total;
  const uint32_t before = blockScan(__popc(mask), total, lds);
  if (L < a.numPoints) a.rel[L] = uint16_t(before);
  if (threadIdx.x == 0) a.blockCount[blockIdx.x] = total;
}

__device__ __forceinline__ uint64_t lineBlockStart(const IsoLineArgs &a, uint32_t which, uint32_t block)
{
  return a.chunkBase[size_t(which) * a.numChunks + block / kIsoChunk] + a.blockBase[size_t(which) * a.numBlocks + block];
}

__global__ __launch_bounds__(kIsoBlock) void isolineEmitVerticesKernel(const IsoLineArgs a)
{
  if (a.blockCount[blockIdx.x] == 0) return;          // the same for the whole block
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  const uint32_t mask = a.mask[L];
  if (!mask) return;
  const uint32_t i = L % a.nu, j = L / a.nu;
  const float *v = a.values + L;
  const float vp = v[0];
  const float px = linePosition(a, i, j, 0), py = linePosition(a, i, j, 1), pz = linePosition(a, i, j, 2);
  const float pu = float(i) + 0.5f, pv = float(j) + 0.5f;
  const uint64_t first = lineBlockStart(a, 0, blockIdx.x) + a.rel[L];
  float *out = a.vertices + 3 * first, *outUv = a.uv + 2 * first;
#pragma unroll
  for (int code = 1; code < 4; code++)
    if (mask & (1u << (code - 1))) {
      const uint32_t dx = uint32_t(code & 1), dy = uint32_t(code >> 1);
      const float vq = v[lineCornerOffset(a, code)];
      const float t = (a.iso - vp) / (vq - vp);
      const float qx = linePosition(a, i + dx, j + dy, 0), qy = linePosition(a, i + dx, j + dy, 1), qz = linePosition(a, i + dx, j + dy, 2);
      out[0] = px + t * (qx - px);
      out[1] = py + t * (qy - py);
      out[2] = pz + t * (qz - pz);
      outUv[0] = pu + t * float(dx);
      outUv[1] = pv + t * float(dy);
      out += 3;
      outUv += 2;
    }
}

// vb[m], mk[m]: index of the first vertex and edge mask of the lattice point origin + m (m = 0, 1, 2: the owners of a
// square's five triangle edges)
template <int TRI>
__device__ __forceinline__ void emitTri(uint32_t inside, const uint32_t (&vb)[3], const uint32_t (&mk)[3], int32_t *&out)
{
  const uint32_t pat = triPattern<TRI>(inside);
  if (pat == 0u || pat == 7u) return;
  int32_t e[3];                               // the vertices on the edges 01, 02, 12 of the triangle
#pragma unroll
  for (int n = 0; n < 3; n++) {
    const int owner = kTriCorner[TRI][n == 2 ? 1 : 0];
    const int code = kTriCorner[TRI][n == 0 ? 1 : 2] ^ owner;
    e[n] = int32_t(vb[owner] + __popc(mk[owner] & ((1u << (code - 1)) - 1u)));
  }
  // s: the vertex alone on its side; the segment (s-o0, s-o1), o0 < o1, reversed iff parity(s,o0,o1) = s & 1 XOR the
  // triangle's parity XOR (s is outside)
  const uint32_t outside = __popc(pat) == 2u ? 1u : 0u;
  const uint32_t single = outside ? (~pat & 7u) : pat;
  const uint32_t s = single >> 1;             // 1, 2, 4 -> 0, 1, 2
  const int32_t first = s == 2u ? e[1] : e[0], second = s == 0u ? e[1] : e[2];
  const bool rev = (((s & 1u) ^ uint32_t(TRI) ^ outside) & 1u) != 0u;
  out[0] = rev ? second : first;
  out[1] = rev ? first : second;
  out += 2;
}

__global__ __launch_bounds__(kIsoBlock) void isolineEmitSegmentsKernel(const IsoLineArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  if (a.blockCount[a.numBlocks + blockIdx.x] == 0) return;      // the same for the whole block
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  const uint32_t count = L < a.numPoints ? (a.squareInfo[L] & 0x7fu) : 0u;
  uint32_t total;
  const uint32_t before = blockScan(count, total, lds);
  if (!count) return;
  const float *v = a.values + L;
  uint32_t inside = 0;
#pragma unroll
  for (int m = 0; m < 4; m++) inside |= (v[lineCornerOffset(a, m)] >= a.iso ? 1u : 0u) << m;
  uint32_t vb[3], mk[3];
#pragma unroll
  for (int m = 0; m < 3; m++) {
    const uint32_t Lp = L + uint32_t(lineCornerOffset(a, m));
    vb[m] = a.vertexBase + uint32_t(lineBlockStart(a, 0, Lp / kIsoBlock)) + a.rel[Lp];     // the vertex count fits 31 bits (checked before the emit)
    mk[m] = a.mask[Lp];
  }
  int32_t *out = a.segments + 2 * (lineBlockStart(a, 1, blockIdx.x) + before);
  emitTri<0>(inside, vb, mk, out);
  emitTri<1>(inside, vb, mk, out);
}

// ---- connected regions of the inside set (exa_hip_regions): the union-find and the passes of exa_isomesh.h ----
template <typename A>      // IsoRegionArgs or IsoBasinArgs
__device__ __forceinline__ bool regionInside(const A &a, float v)
{
  return __builtin_isfinite(v) && (a.below ? v < a.iso : v >= a.iso);
}

// the total order of exa_hip_histogram's value range on the float bits
__device__ __forceinline__ uint32_t regionKey(float v)
{
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float regionValueOfKey(uint32_t key)
{
  return __uint_as_float(key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu));
}

// The root of x's tree as the loads show it.  Links descend strictly, so the walk ends within x steps; a link that ascends
// (which no kernel here writes: the outside mark included) or more than numPoints steps trip the guard, and the walk stops
// where it stands.  COHERENT: agent-scope loads for the merge, whose links other workgroups' atomics change meanwhile.
template <bool COHERENT>
__device__ __forceinline__ uint32_t regionFind(const IsoRegionArgs &a, uint32_t x, bool &tripped)
{
  for (uint32_t left = a.numPoints; left; left--) {
    const uint32_t p = COHERENT ? __hip_atomic_load(a.parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : a.parent[x];
    if (p == x) return x;
    if (p > x) break;
    x = p;
  }
  tripped = true;
  return x;
}

// Unites the trees of x and y, both inside; returns the smaller root.  Every round either links a root (and ends) or goes on
// with two indices below the larger one of the round before: at most numPoints rounds.
__device__ __forceinline__ uint32_t regionUnite(const IsoRegionArgs &a, uint32_t x, uint32_t y, bool &tripped)
{
  uint32_t ra = regionFind<true>(a, x, tripped), rb = regionFind<true>(a, y, tripped);
  for (uint32_t left = a.numPoints; ra != rb && !tripped; left--) {
    const uint32_t hi = ra > rb ? ra : rb, lo = ra > rb ? rb : ra;
    const uint32_t old = atomicMin(a.parent + hi, lo);
    if (old == hi) return lo;                         // hi was a root, and now hangs below lo
    if (old > hi || left == 0u) { tripped = true; break; }
    // hi had been linked to `old` in the meantime; the atomicMin kept that link or replaced it by lo, and in both cases
    // what is left to unite is old with lo
    ra = regionFind<true>(a, old, tripped);
    rb = regionFind<true>(a, lo, tripped);
  }
  return ra < rb ? ra : rb;
}

// A block of the init and of the stats pass covers kIsoRegionTiles consecutive blocks of the lattice, tile after tile (a wave
// still reads 64 consecutive L at a time): their atomics all go to a few addresses, one region's record or the two counts,
// and what a lane has gathered over its tiles goes there once.
__global__ __launch_bounds__(kIsoBlock) void isoRegionInitKernel(const IsoRegionArgs a)
{
  __shared__ uint32_t lds[2 * (kIsoBlock / 64)];
  uint32_t count = 0, mag = 0;                        // mag: bits of |V|, ordered as unsigned integers for finite values
  for (uint32_t t = 0; t < kIsoRegionTiles; t++) {
    const uint64_t at = (uint64_t(blockIdx.x) * kIsoRegionTiles + t) * kIsoBlock + threadIdx.x;
    if (at >= a.numPoints) break;
    const uint32_t L = uint32_t(at);
    const float v = a.values[L];
    const bool in = regionInside(a, v);
    if (in) {
      const uint32_t m = __float_as_uint(v) & 0x7fffffffu;
      mag = m > mag ? m : mag;
      count++;
    }
    a.parent[L] = in ? L : kIsoRegionOutside;
  }
  for (int o = 32; o; o >>= 1) {
    const uint32_t m = uint32_t(__shfl_xor(int(mag), o));
    mag = m > mag ? m : mag;
    count += uint32_t(__shfl_xor(int(count), o));
  }
  if ((threadIdx.x & 63u) == 0u) { lds[threadIdx.x >> 6] = count; lds[kIsoBlock / 64 + (threadIdx.x >> 6)] = mag; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0, top = 0;
    for (uint32_t w = 0; w < kIsoBlock / 64; w++) {
      sum += lds[w];
      top = lds[kIsoBlock / 64 + w] > top ? lds[kIsoBlock / 64 + w] : top;
    }
    if (sum) {
      atomicAdd(reinterpret_cast<unsigned long long *>(a.totals + 1), (unsigned long long)sum);
      atomicMax(reinterpret_cast<uint32_t *>(a.totals + 2), top);
    }
  }
}

__global__ __launch_bounds__(kIsoBlock) void isoRegionMergeKernel(const IsoRegionArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  if (a.parent[L] == kIsoRegionOutside) return;       // the mark is the init kernel's and never changes
  const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
  bool tripped = false;
  uint32_t root = L;
#pragma unroll
  for (int code = 1; code < 8; code++) {
    if (a.faces && (code & (code - 1))) continue;
    if (i + uint32_t(code & 1) >= a.nx || j + uint32_t((code >> 1) & 1) >= a.ny || k + uint32_t(code >> 2) >= a.nz) continue;
    const uint32_t Q = L + uint32_t(size_t(code & 1) + size_t((code >> 1) & 1) * a.nx + size_t(code >> 2) * (size_t(a.nx) * a.ny));
    if (a.parent[Q] == kIsoRegionOutside) continue;
    root = regionUnite(a, root, Q, tripped);
  }
  // shorten the walks of those that come later: L straight below the root it has just seen (a monotone update as well)
  if (root < L) atomicMin(a.parent + L, root);
  if (tripped) atomicExch(a.errorFlag, 1);
}

__global__ __launch_bounds__(kIsoBlock) void isoRegionFlattenKernel(const IsoRegionArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  uint32_t isRoot = 0;
  bool tripped = false;
  if (L < a.numPoints) {
    const uint32_t p = a.parent[L];
    if (p != kIsoRegionOutside) {
      // other lanes store roots into their own slots meanwhile: a walk meets a link of the merge or the root itself
      const uint32_t r = p <= L ? regionFind<false>(a, p, tripped) : L;
      tripped = tripped || p > L;
      if (r != p) a.parent[L] = r;
      isRoot = r == L ? 1u : 0u;
    }
  }
  uint32_t total;
  (void)blockScan(isRoot, total, lds);
  if (threadIdx.x == 0) a.blockCount[blockIdx.x] = total;
  if (tripped) atomicExch(a.errorFlag, 1);
}

// A record of the table (ExaHipRegion, or ExaHipBasin with the same leading fields) before the stats pass adds to it, and
// its two keys.  rest(): the record's words behind `max`, stored before the keys: the compiler merges them with the stores
// in front, which it cannot do across the stores to the keys.
template <typename R, typename F>
__device__ __forceinline__ void recordStart(R &r, uint64_t *keys, uint32_t number, uint32_t first, F rest)
{
  r.points = 0;
  r.sumFixed = 0;
  for (int c = 0; c < 3; c++) { r.sumIndex[c] = 0; r.lo[c] = INT32_MAX; r.hi[c] = INT32_MIN; }
  r.first = first;
  r.argMin = r.argMax = 0;
  r.min = r.max = 0.f;
  rest();
  keys[2 * size_t(number)] = ~0ull;
  keys[2 * size_t(number) + 1] = 0ull;
}

// min, max, argMin, argMax of record n out of its two keys
template <typename R>
__device__ __forceinline__ void recordRange(R &r, const uint64_t *keys, uint32_t n)
{
  const uint64_t kmin = keys[2 * size_t(n)], kmax = keys[2 * size_t(n) + 1];
  r.min = regionValueOfKey(uint32_t(kmin >> 32));
  r.argMin = uint32_t(kmin);
  r.max = regionValueOfKey(uint32_t(kmax >> 32));
  r.argMax = ~uint32_t(kmax);
}

__global__ __launch_bounds__(kIsoBlock) void isoRegionRankKernel(const IsoRegionArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  if (a.blockCount[blockIdx.x] == 0) return;          // the same for the whole block
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  const bool isRoot = L < a.numPoints && a.parent[L] == L;
  uint32_t total;
  const uint32_t before = blockScan(isRoot ? 1u : 0u, total, lds);
  if (!isRoot) return;
  const uint32_t number = uint32_t(a.chunkBase[blockIdx.x / kIsoChunk]) + a.blockBase[blockIdx.x] + before;   // < numPoints
  a.parent[L] = kIsoRegionRanked | number;
  ExaHipRegion &r = a.regions[number];
  static_assert(sizeof(ExaHipRegion) == 88, "the table's record: 84 bytes of fields and 4 of padding");
  recordStart(r, a.keys, number, L, [&] { reinterpret_cast<uint32_t *>(&r)[21] = 0u; });     // the padding: every byte of the table is defined
}

// what a lane, or the lanes of a wave that share a label, add to a region
struct RegionPart {
  uint32_t points;
  long long sum;
  unsigned long long si, sj, sk;
  int32_t lo[3], hi[3];
  unsigned long long keyMin, keyMax;
};

__device__ __forceinline__ void regionReduce(RegionPart &p)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    p.points += uint32_t(__shfl_xor(int(p.points), o));
    p.sum += __shfl_xor(p.sum, o);
    p.si += __shfl_xor(p.si, o);
    p.sj += __shfl_xor(p.sj, o);
    p.sk += __shfl_xor(p.sk, o);
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const int32_t l = __shfl_xor(p.lo[c], o), h = __shfl_xor(p.hi[c], o);
      p.lo[c] = l < p.lo[c] ? l : p.lo[c];
      p.hi[c] = h > p.hi[c] ? h : p.hi[c];
    }
    const unsigned long long kmin = __shfl_xor(p.keyMin, o), kmax = __shfl_xor(p.keyMax, o);
    p.keyMin = kmin < p.keyMin ? kmin : p.keyMin;
    p.keyMax = kmax > p.keyMax ? kmax : p.keyMax;
  }
}

template <typename R>
__device__ __forceinline__ void recordAdd(R *table, uint64_t *keys, uint32_t label, const RegionPart &p)
{
  R &r = table[label];
  atomicAdd(reinterpret_cast<unsigned long long *>(&r.points), (unsigned long long)p.points);
  atomicAdd(reinterpret_cast<unsigned long long *>(&r.sumFixed), (unsigned long long)p.sum);
  atomicAdd(reinterpret_cast<unsigned long long *>(&r.sumIndex[0]), p.si);
  atomicAdd(reinterpret_cast<unsigned long long *>(&r.sumIndex[1]), p.sj);
  atomicAdd(reinterpret_cast<unsigned long long *>(&r.sumIndex[2]), p.sk);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    atomicMin(&r.lo[c], p.lo[c]);
    atomicMax(&r.hi[c], p.hi[c]);
  }
  atomicMin(reinterpret_cast<unsigned long long *>(keys + 2 * size_t(label)), p.keyMin);
  atomicMax(reinterpret_cast<unsigned long long *>(keys + 2 * size_t(label) + 1), p.keyMax);
}

__device__ __forceinline__ RegionPart regionNothing()
{
  return { 0u, 0ll, 0ull, 0ull, 0ull, { INT32_MAX, INT32_MAX, INT32_MAX }, { INT32_MIN, INT32_MIN, INT32_MIN }, ~0ull, 0ull };
}

// The stats pass of the regions and of the basins (a: IsoRegionArgs or IsoBasinArgs).  labelOf(L, slot): the number of the
// record of the inside point L, whose slot of `labels` holds `slot`; a number that is none of the table's `count` records is
// not what the passes before leave behind and trips the guard.
template <typename A, typename R, typename F>
__device__ __forceinline__ void recordStats(const A &a, uint32_t *labels, R *table, uint32_t count, F labelOf)
{
  const uint32_t lane = threadIdx.x & 63u;
  // the lane's tiles, 256 points apart: in a region of some size they share its label, and the lane gathers them; where the
  // label changes, what it holds goes to its region first
  bool in = false;
  uint32_t label = 0;
  RegionPart own = regionNothing();
#pragma unroll 1
  for (uint32_t t = 0; t < kIsoRegionTiles; t++) {
    const uint64_t at = (uint64_t(blockIdx.x) * kIsoRegionTiles + t) * kIsoBlock + threadIdx.x;
    if (at >= a.numPoints) break;
    const uint32_t L = uint32_t(at);
    const uint32_t p = labels[L];
    if (p == kIsoRegionOutside) continue;
    const uint32_t mine = labelOf(L, p);
    if (mine >= count) {                              // nothing is added anywhere
      atomicExch(a.errorFlag, 1);
      continue;
    }
    labels[L] = mine;
    if (in && mine != label) {
      recordAdd(table, a.keys, label, own);
      own = regionNothing();
    }
    in = true;
    label = mine;
    const float v = a.values[L];
    const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
    const unsigned long long key = (unsigned long long)regionKey(v) << 32;
    own.points++;
    own.sum += __double2ll_rn(double(v) * a.scale);
    own.si += i; own.sj += j; own.sk += k;
    own.lo[0] = min(own.lo[0], int32_t(i)); own.lo[1] = min(own.lo[1], int32_t(j)); own.lo[2] = min(own.lo[2], int32_t(k));
    own.hi[0] = max(own.hi[0], int32_t(i)); own.hi[1] = max(own.hi[1], int32_t(j)); own.hi[2] = max(own.hi[2], int32_t(k));
    own.keyMin = min(own.keyMin, key | L);
    own.keyMax = max(own.keyMax, key | (~L));
  }
  // the lanes of a wave are consecutive L and mostly share one label or two: the label of the first pending lane is
  // reduced over the wave and added by that lane, twice; what is left then goes lane by lane
  unsigned long long pending = __ballot(in);
#pragma unroll 1
  for (int round = 0; round < 2; round++) {
    if (!pending) return;                             // wave-uniform
    const uint32_t leader = uint32_t(__ffsll(pending)) - 1u;
    const uint32_t lb = uint32_t(__builtin_amdgcn_readlane(int(label), int(leader)));
    const bool same = in && label == lb;
    const unsigned long long m = __ballot(same);
    RegionPart part = own;
    if (!same) part = regionNothing();
    if (__popcll(m) > 1) regionReduce(part);          // wave-uniform
    if (lane == leader) recordAdd(table, a.keys, lb, part);
    in = in && !same;
    pending &= ~m;
  }
  if (in) recordAdd(table, a.keys, label, own);
}

__global__ __launch_bounds__(kIsoBlock) void isoRegionStatsKernel(const IsoRegionArgs a)
{
  // a root's slot holds kIsoRegionRanked | number until the root's lane stores the number itself: the mask reads both
  recordStats(a, a.parent, a.regions, a.numRegions, [&](uint32_t L, uint32_t p) {
    return ((p & kIsoRegionRanked) ? p : a.parent[p < L ? p : L]) & ~kIsoRegionRanked;
  });
}

__global__ __launch_bounds__(kIsoBlock) void isoRegionFinishKernel(const IsoRegionArgs a)
{
  const uint32_t n = blockIdx.x * kIsoBlock + threadIdx.x;
  if (n >= a.numRegions) return;
  recordRange(a.regions[n], a.keys, n);
}

// ---- basins of the inside set (exa_hip_basins): the ascent, the rounds and the table of exa_isomesh.h ----
// the height of the contract: the ordered key, complemented for basins of minima
__device__ __forceinline__ uint32_t basinHeight(const IsoBasinArgs &a, float v)
{
  const uint32_t key = regionKey(v);
  return a.below ? ~key : key;
}

// f(Q) for every lattice neighbour Q of L: p +- d over the seven (three with faces) kinds of edge
template <typename F>
__device__ __forceinline__ void basinNeighbours(const IsoBasinArgs &a, uint32_t L, F f)
{
  const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
#pragma unroll
  for (int code = 1; code < 8; code++) {
    if (a.faces && (code & (code - 1))) continue;
    const uint32_t dx = uint32_t(code & 1), dy = uint32_t((code >> 1) & 1), dz = uint32_t(code >> 2);
    const uint32_t off = uint32_t(size_t(dx) + size_t(dy) * a.nx + size_t(dz) * (size_t(a.nx) * a.ny));
    if (i + dx < a.nx && j + dy < a.ny && k + dz < a.nz) f(L + off);
    if (i >= dx && j >= dy && k >= dz) f(L - off);
  }
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinUpKernel(const IsoBasinArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  const float v = a.values[L];
  if (!regionInside(a, v)) return;                     // the init kernel's outside mark stays
  // the order of the contract as one word: the height, then the smaller L
  unsigned long long best = (unsigned long long)basinHeight(a, v) << 32 | (~L);
  basinNeighbours(a, L, [&](uint32_t Q) {
    const float w = a.values[Q];
    if (!regionInside(a, w)) return;
    const unsigned long long r = (unsigned long long)basinHeight(a, w) << 32 | (~Q);
    best = r > best ? r : best;
  });
  a.comp[L] = ~uint32_t(best);
}

// Pointer doubling in place.  Other lanes move their own slots along their own chains meanwhile, so whatever a load shows
// is an ancestor.  A slot that names nothing of the array (the outside mark inside a chain included) trips the guard.
__global__ __launch_bounds__(kIsoBlock) void isoBasinJumpKernel(const IsoBasinArgs a)
{
  const uint32_t x = blockIdx.x * kIsoBlock + threadIdx.x;
  bool more = false, tripped = false;
  if (x < a.jumpSize) {
    const uint32_t own = a.jumpArray[x];
    if (own != kIsoRegionOutside) {
      uint32_t p = own;
      bool fixed = false;
      for (uint32_t hop = 0; hop <= kIsoBasinHops && !fixed && !tripped; hop++) {
        if (p >= a.jumpSize) { tripped = true; break; }
        const uint32_t q = a.jumpArray[p];
        if (q == p) fixed = true;
        else if (hop < kIsoBasinHops) p = q;            // the last round only looks whether p is a fixed point
      }
      if (!tripped) {
        if (p != own) a.jumpArray[x] = p;
        more = !fixed;
      }
    }
  }
  const unsigned long long m = __ballot(more);
  if (m && (threadIdx.x & 63u) == uint32_t(__ffsll(m)) - 1u) atomicAdd(a.jumpCount, 1u);
  if (tripped) atomicExch(a.errorFlag, 1);
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinCountKernel(const IsoBasinArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  const uint32_t x = blockIdx.x * kIsoBlock + threadIdx.x;
  const uint32_t isRoot = x < a.jumpSize && a.jumpArray[x] == x ? 1u : 0u;
  uint32_t total;
  (void)blockScan(isRoot, total, lds);
  if (threadIdx.x == 0) a.blockCount[blockIdx.x] = total;
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinRankKernel(const IsoBasinArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  if (a.blockCount[blockIdx.x] == 0) return;          // the same for the whole block
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  const bool isPeak = L < a.numPoints && a.comp[L] == L;
  uint32_t total;
  const uint32_t before = blockScan(isPeak ? 1u : 0u, total, lds);
  if (!isPeak) return;
  const uint32_t number = uint32_t(a.chunkBase[blockIdx.x / kIsoChunk]) + a.blockBase[blockIdx.x] + before;   // < numRaw
  a.comp[L] = kIsoRegionRanked | number;
  a.peakOf[number] = L;
  a.link[number] = number;
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinLabelKernel(const IsoBasinArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  const uint32_t p = a.comp[L];
  if (p == kIsoRegionOutside) return;
  // a peak's slot holds kIsoRegionRanked | number until the peak's lane stores the number itself: the mask reads both
  uint32_t mine = kIsoRegionOutside;
  if (p & kIsoRegionRanked) mine = p & ~kIsoRegionRanked;
  else if (p < a.numPoints) mine = a.comp[p] & ~kIsoRegionRanked;
  if (mine >= a.numRaw) {                             // not what the passes before leave behind
    atomicExch(a.errorFlag, 1);
    return;
  }
  a.comp[L] = mine;
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinPassKernel(const IsoBasinArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t mine = kIsoRegionOutside;
  unsigned long long word = 0ull;
  if (L < a.numPoints) mine = a.comp[L];
  if (mine >= a.numRaw) mine = kIsoRegionOutside;     // the outside mark, or what only a tripped guard leaves behind
  if (mine != kIsoRegionOutside) {
    uint32_t height = 0u;
    bool haveHeight = false;
    basinNeighbours(a, L, [&](uint32_t Q) {
      const uint32_t other = a.comp[Q];
      if (other >= a.numRaw || other == mine) return;               // outside, or, most edges, inside: nothing more is read
      if (!haveHeight) { height = basinHeight(a, a.values[L]); haveHeight = true; }
      const uint32_t hq = basinHeight(a, a.values[Q]);
      const unsigned long long w = (unsigned long long)(hq < height ? hq : height) << 32 | (~other);
      word = w > word ? w : word;
    });
  }
  // the lanes of a wave are consecutive L and mostly share one component or two: as in the regions' stats pass
  bool in = word != 0ull;
  unsigned long long pending = __ballot(in);
#pragma unroll 1
  for (int round = 0; round < 2; round++) {
    if (!pending) return;                             // wave-uniform
    const uint32_t leader = uint32_t(__ffsll(pending)) - 1u;
    const uint32_t lb = uint32_t(__builtin_amdgcn_readlane(int(mine), int(leader)));
    const bool same = in && mine == lb;
    const unsigned long long m = __ballot(same);
    unsigned long long top = same ? word : 0ull;
    if (__popcll(m) > 1) {                            // wave-uniform
#pragma unroll
      for (int o = 32; o; o >>= 1) {
        const unsigned long long t = __shfl_xor(top, o);
        top = t > top ? t : top;
      }
    }
    if (lane == leader && top > a.pass[lb]) atomicMax(reinterpret_cast<unsigned long long *>(a.pass + lb), top);
    in = in && !same;
    pending &= ~m;
  }
  if (in && word > a.pass[mine]) atomicMax(reinterpret_cast<unsigned long long *>(a.pass + mine), word);
}

// saddle and depth of the component n out of its word w != 0: one float32 subtraction
__device__ __forceinline__ float basinDepth(const IsoBasinArgs &a, uint32_t n, unsigned long long w, float &saddle)
{
  const uint32_t hs = uint32_t(w >> 32);
  saddle = regionValueOfKey(a.below ? ~hs : hs);
  const float top = a.values[a.peakOf[n]];
  return a.below ? saddle - top : top - saddle;
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinLinkKernel(const IsoBasinArgs a)
{
  const uint32_t n = blockIdx.x * kIsoBlock + threadIdx.x;
  bool linked = false;
  if (n < a.numRaw && a.link[n] == n) {
    const unsigned long long w = a.pass[n];
    const uint32_t B = ~uint32_t(w);
    if (w != 0ull && B < a.numRaw) {
      float saddle;
      const float depth = basinDepth(a, n, w, saddle);
      const uint32_t hn = basinHeight(a, a.values[a.peakOf[n]]), hb = basinHeight(a, a.values[a.peakOf[B]]);
      // raw numbers ascend with the peak's L
      if (depth < a.minDepth && (hb > hn || (hb == hn && B < n))) {
        a.link[n] = B;
        linked = true;
      }
    } else if (w != 0ull) atomicExch(a.errorFlag, 1);
  }
  const unsigned long long m = __ballot(linked);
  if (m && (threadIdx.x & 63u) == uint32_t(__ffsll(m)) - 1u) atomicAdd(a.jumpCount, uint32_t(__popcll(m)));
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinMergeKernel(const IsoBasinArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  const uint32_t c = a.comp[L];
  if (c == kIsoRegionOutside) return;
  if (c >= a.numRaw) { atomicExch(a.errorFlag, 1); return; }
  const uint32_t to = a.link[c];
  if (to != c) a.comp[L] = to;
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinFinalKernel(const IsoBasinArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  if (a.blockCount[blockIdx.x] == 0) return;          // the same for the whole block
  const uint32_t n = blockIdx.x * kIsoBlock + threadIdx.x;
  const bool isRoot = n < a.numRaw && a.link[n] == n;
  uint32_t total;
  const uint32_t before = blockScan(isRoot ? 1u : 0u, total, lds);
  if (!isRoot) return;
  const uint32_t number = uint32_t(a.chunkBase[blockIdx.x / kIsoChunk]) + a.blockBase[blockIdx.x] + before;   // < numBasins
  a.finalOf[n] = number;
  ExaHipBasin &r = a.basins[number];
  static_assert(sizeof(ExaHipBasin) == 96, "the table's record: no padding");
  recordStart(r, a.keys, number, kIsoRegionOutside, [&] {       // `first` comes from the first kernel
    r.neighbour = int32_t(n);                         // parked for the finish kernel, which needs the component's word
    r.saddle = r.depth = 0.f;
  });
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinStatsKernel(const IsoBasinArgs a)
{
  recordStats(a, a.comp, a.basins, a.numBasins, [&](uint32_t, uint32_t c) { return c < a.numRaw ? a.finalOf[c] : kIsoRegionOutside; });
}

// `first` of every basin, behind the stats pass: the labels are final, and a thirteenth value per lane would take the stats
// kernel past its 64 registers.  A wave holds 64 consecutive L; only a lane whose left neighbour holds another label (or the
// wave's first lane) can be its basin's smallest L, and it goes to the record unless an agent-scope load (past the L1, which
// other CUs' atomics never refresh) already shows a smaller one — in a basin of some size nearly every wave finds one.
__global__ __launch_bounds__(kIsoBlock) void isoBasinFirstKernel(const IsoBasinArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  const uint32_t label = L < a.numPoints ? a.comp[L] : kIsoRegionOutside;
  const uint32_t left = uint32_t(__shfl_up(int(label), 1));
  if (label >= a.numBasins) return;                   // outside
  if ((threadIdx.x & 63u) != 0u && left == label) return;
  uint32_t *first = &a.basins[label].first;
  if (L < __hip_atomic_load(first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(first, L);
}

__global__ __launch_bounds__(kIsoBlock) void isoBasinFinishKernel(const IsoBasinArgs a)
{
  const uint32_t b = blockIdx.x * kIsoBlock + threadIdx.x;
  if (b >= a.numBasins) return;
  ExaHipBasin &r = a.basins[b];
  recordRange(r, a.keys, b);
  const uint32_t n = uint32_t(r.neighbour);           // the component's raw number, parked by the final kernel
  const unsigned long long w = n < a.numRaw ? a.pass[n] : 0ull;
  const uint32_t B = ~uint32_t(w);
  if (w != 0ull && B < a.numRaw) {
    float saddle;
    r.depth = basinDepth(a, n, w, saddle);
    r.saddle = saddle;
    r.neighbour = int32_t(a.finalOf[B]);
  } else {
    r.neighbour = -1;
    r.saddle = __uint_as_float(0x7fc00000u);
    r.depth = __uint_as_float(0x7f800000u);
  }
}

// ---- the stretch of a flow map on a lattice (exa_hip_flowmap): the largest eigenvalue of the Cauchy-Green tensor of the
// map's differences, one lane per lattice point.  The matrix lives in named registers and the three rotations of a sweep are
// written out: no indexed local array, so no scratch. ----
__device__ __forceinline__ bool stretchValid(int32_t reason)
{
  return reason == EXA_STREAM_END_MAXSTEPS || reason == EXA_STREAM_END_STAGNANT;
}

// column a of the deformation gradient at point L, index idx of n along the axis, `stride` points apart: central inside,
// one-sided on the faces, zero for an axis of one point; false if a stencil point is not valid
__device__ __forceinline__ bool stretchColumn(const IsoStretchArgs &a, uint32_t L, uint32_t idx, uint32_t n, size_t stride, float lo,
                                              float cell, float &f0, float &f1, float &f2)
{
  f0 = f1 = f2 = 0.f;
  if (n < 2) return true;
  const uint32_t im = idx > 0 ? idx - 1 : 0, ip = idx + 1 < n ? idx + 1 : n - 1;
  const size_t m = size_t(L) - size_t(idx - im) * stride, p = size_t(L) + size_t(ip - idx) * stride;
  const float dx = (lo + (float(ip) + .5f) * cell) - (lo + (float(im) + .5f) * cell);
  f0 = (a.end[3 * p] - a.end[3 * m]) / dx;
  f1 = (a.end[3 * p + 1] - a.end[3 * m + 1]) / dx;
  f2 = (a.end[3 * p + 2] - a.end[3 * m + 2]) / dx;
  return stretchValid(a.reasons[m]) && stretchValid(a.reasons[p]);
}

// one rotation (p, q) of cyclic Jacobi, r the third index
__device__ __forceinline__ void stretchRotate(float &app, float &aqq, float &apq, float &arp, float &arq)
{
  if (apq == 0.0f) return;
  const float theta = (aqq - app) / (2.f * apq);
  const float t = copysignf(1.f, theta) / (fabsf(theta) + sqrtf(theta * theta + 1.f));
  const float c = 1.f / sqrtf(t * t + 1.f);
  const float s = t * c;
  const float tp = t * apq;
  const float rp = c * arp - s * arq, rq = s * arp + c * arq;
  app = app - tp;
  aqq = aqq + tp;
  arp = rp;
  arq = rq;
  apq = 0.f;
}

__global__ __launch_bounds__(kIsoBlock) void isoLatticeStretchKernel(const IsoStretchArgs a)
{
  const uint32_t L = blockIdx.x * kIsoBlock + threadIdx.x;
  if (L >= a.numPoints) return;
  const uint32_t i = L % a.nx, j = (L / a.nx) % a.ny, k = L / (a.nx * a.ny);
  float f00, f10, f20, f01, f11, f21, f02, f12, f22;               // F[c][a]
  bool ok = stretchValid(a.reasons[L]);
  ok = stretchColumn(a, L, i, a.nx, 1, a.lo[0], a.cell[0], f00, f10, f20) && ok;
  ok = stretchColumn(a, L, j, a.ny, a.nx, a.lo[1], a.cell[1], f01, f11, f21) && ok;
  ok = stretchColumn(a, L, k, a.nz, size_t(a.nx) * a.ny, a.lo[2], a.cell[2], f02, f12, f22) && ok;
  if (!ok) { a.stretch[L] = a.fill; return; }
  float a00 = (f00 * f00 + f10 * f10) + f20 * f20, a11 = (f01 * f01 + f11 * f11) + f21 * f21, a22 = (f02 * f02 + f12 * f12) + f22 * f22;
  float a01 = (f00 * f01 + f10 * f11) + f20 * f21, a02 = (f00 * f02 + f10 * f12) + f20 * f22, a12 = (f01 * f02 + f11 * f12) + f21 * f22;
  for (int sweep = 0; sweep < 5; sweep++) {
    stretchRotate(a00, a11, a01, a02, a12);
    stretchRotate(a00, a22, a02, a01, a12);
    stretchRotate(a11, a22, a12, a01, a02);
  }
  float m = a00;
  if (a11 > m) m = a11;
  if (a22 > m) m = a22;
  a.stretch[L] = m;
}

// ---- critical points of a vector field on a lattice (exa_hip_critical_points): the passes of exa_isomesh.h ----
__device__ __forceinline__ size_t criticalOffset(const IsoCriticalArgs &a, int m)
{
  return size_t(m & 1) + size_t((m >> 1) & 1) * a.nx + size_t(m >> 2) * (size_t(a.nx) * a.ny);
}

// The cell pass: a streaming stencil over the three lattices.  Plain loads (EXA_CRITICAL_LDS 0): the eight corners of a wave's
// 64 cells are four rows of 65 consecutive floats per component, so the corner loads of neighbouring lanes and of the next
// y / z row hit the lines the L1 and L2 already hold.  EXA_CRITICAL_LDS 1 stages those rows of a block, 4 x 257 floats per
// component, in LDS first (12 loads per lane instead of 24, and 24 LDS reads); tools/ab_variants.sh builds the two.  Plain
// loads are the default: on a 256^3 lattice the slab takes 2.3 x their time (profiles/critical_cells_ab.txt).  The bytes are
// the same either way.
#ifndef EXA_CRITICAL_LDS
#define EXA_CRITICAL_LDS 0
#endif

__global__ __launch_bounds__(kIsoBlock) void isoCriticalCellKernel(const IsoCriticalArgs a)
{
  __shared__ uint32_t lds[3 * (kIsoBlock / 64)];
#if EXA_CRITICAL_LDS
  __shared__ float slab[3][4][kIsoBlock + 1];           // [component][dy + 2 dz][x]
#endif
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t cells = 0, invalid = 0;
#pragma unroll 1
  for (uint32_t t = 0; t < kIsoCriticalTiles; t++) {
    const uint32_t tile = blockIdx.x * kIsoCriticalTiles + t;
    if (tile >= a.numBlocks) break;                     // the same for the whole block
    const uint64_t at = uint64_t(tile) * kIsoBlock + threadIdx.x;
#if EXA_CRITICAL_LDS
    // a valid cell's corners are lattice points; what lies behind the lattice's end is never read
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const float *v = a.values + size_t(c) * a.numPoints;
        const uint64_t row = uint64_t(tile) * kIsoBlock + criticalOffset(a, 2 * r);
        slab[c][r][threadIdx.x] = row + threadIdx.x < a.numPoints ? v[row + threadIdx.x] : 0.f;
        if (threadIdx.x == 0) slab[c][r][kIsoBlock] = row + kIsoBlock < a.numPoints ? v[row + kIsoBlock] : 0.f;
      }
    __syncthreads();
#endif
    bool cand = false;
    if (at < a.numPoints) {
      const uint32_t L = uint32_t(at);
      const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
      if (i + 1 < a.nx && j + 1 < a.ny && k + 1 < a.nz) {
        cells++;
        bool finite = true;
        cand = true;
#pragma unroll
        for (int c = 0; c < 3; c++) {
#if EXA_CRITICAL_LDS
          float mn = slab[c][0][threadIdx.x], mx = mn;
#else
          const float *v = a.values + size_t(c) * a.numPoints + L;
          float mn = v[0], mx = mn;
#endif
          finite = finite && __builtin_isfinite(mn);
#pragma unroll
          for (int m = 1; m < 8; m++) {
#if EXA_CRITICAL_LDS
            const float x = slab[c][m >> 1][threadIdx.x + (m & 1)];
#else
            const float x = v[criticalOffset(a, m)];
#endif
            finite = finite && __builtin_isfinite(x);
            mn = fminf(mn, x);
            mx = fmaxf(mx, x);
          }
          cand = cand && mn <= 0.f && 0.f <= mx && mn < mx;
        }
        cand = cand && finite;
        invalid += finite ? 0u : 1u;
      }
    }
    const unsigned long long marks = __ballot(cand);
    if (lane == 0u) {
      a.marks[size_t(tile) * (kIsoBlock / 64) + wave] = marks;
      lds[wave] = uint32_t(__popcll(marks));
    }
    __syncthreads();
    if (threadIdx.x == 0) a.blockCount[tile] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
    __syncthreads();
  }
  static_assert(kIsoBlock / 64 == 4, "the block's count is written out for four waves");
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    cells += uint32_t(__shfl_xor(int(cells), o));
    invalid += uint32_t(__shfl_xor(int(invalid), o));
  }
  if (lane == 0u) { lds[4 + wave] = cells; lds[8 + wave] = invalid; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t c = (lds[4] + lds[5]) + (lds[6] + lds[7]), n = (lds[8] + lds[9]) + (lds[10] + lds[11]);
    if (c) atomicAdd(a.counters + 0, (unsigned long long)c);
    if (n) atomicAdd(a.counters + 1, (unsigned long long)n);
  }
}

// candidate number = the candidates in front of the block (the scans) + those of the block's earlier waves + the marks below
// the lane's own bit: the list is in ascending L
__global__ __launch_bounds__(kIsoBlock) void isoCriticalCompactKernel(const IsoCriticalArgs a)
{
  if (a.blockCount[blockIdx.x] == 0) return;          // the same for the whole block
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long *marks = a.marks + size_t(blockIdx.x) * (kIsoBlock / 64);
  const unsigned long long mine = marks[wave];
  if (!((mine >> lane) & 1ull)) return;
  uint32_t before = uint32_t(__popcll(mine & ((1ull << lane) - 1ull)));
  for (unsigned w = 0; w < wave; w++) before += uint32_t(__popcll(marks[w]));
  const uint64_t first = a.chunkBase[blockIdx.x / kIsoChunk] + a.blockBase[blockIdx.x];      // < numPoints
  a.candidates[first + before] = blockIdx.x * kIsoBlock + threadIdx.x;
}

// F = T(s) and J = dT/ds of the cell with origin L, accumulated corner by corner in the contract's association: twelve sums
// in registers instead of 24 corner values
struct CriticalJet { float f[3]; float j[3][3]; };

template <int M>
__device__ __forceinline__ void criticalCorner(const IsoCriticalArgs &a, const float *v, const float (&u)[3][2], CriticalJet &t)
{
  constexpr int dx = M & 1, dy = (M >> 1) & 1, dz = M >> 2;
  const float wxy = u[0][dx] * u[1][dy], wxz = u[0][dx] * u[2][dz], wyz = u[1][dy] * u[2][dz];
  const float w = wxy * u[2][dz];
  const size_t off = criticalOffset(a, M);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float x = v[size_t(c) * a.numPoints + off];
    t.f[c] = t.f[c] + w * x;
    const float px = wyz * x, py = wxz * x, pz = wxy * x;
    t.j[c][0] = t.j[c][0] + (dx ? px : -px);
    t.j[c][1] = t.j[c][1] + (dy ? py : -py);
    t.j[c][2] = t.j[c][2] + (dz ? pz : -pz);
  }
}

__device__ __forceinline__ void criticalJet(const IsoCriticalArgs &a, uint32_t L, float s0, float s1, float s2, CriticalJet &t)
{
  const float u[3][2] = { { 1.f - s0, s0 }, { 1.f - s1, s1 }, { 1.f - s2, s2 } };
#pragma unroll
  for (int c = 0; c < 3; c++) {
    t.f[c] = 0.f;
    t.j[c][0] = t.j[c][1] = t.j[c][2] = 0.f;
  }
  const float *v = a.values + L;
  criticalCorner<0>(a, v, u, t);
  criticalCorner<1>(a, v, u, t);
  criticalCorner<2>(a, v, u, t);
  criticalCorner<3>(a, v, u, t);
  criticalCorner<4>(a, v, u, t);
  criticalCorner<5>(a, v, u, t);
  criticalCorner<6>(a, v, u, t);
  criticalCorner<7>(a, v, u, t);
}

__global__ __launch_bounds__(kIsoBlock) void isoCriticalRefineKernel(const IsoCriticalArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t n = blockIdx.x * kIsoBlock + threadIdx.x;
  int32_t result = -1;                                  // no candidate
  if (n < a.numCandidates) {
    const uint32_t L = a.candidates[n];
    const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
    float s0 = 0.5f, s1 = 0.5f, s2 = 0.5f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
#pragma unroll 1
    for (int32_t it = 0; it < a.iterations; it++) {
      CriticalJet t;
      criticalJet(a, L, s0, s1, s2, t);
      const float a00 = t.j[1][1] * t.j[2][2] - t.j[1][2] * t.j[2][1], a01 = t.j[0][2] * t.j[2][1] - t.j[0][1] * t.j[2][2],
                  a02 = t.j[0][1] * t.j[1][2] - t.j[0][2] * t.j[1][1];
      const float a10 = t.j[1][2] * t.j[2][0] - t.j[1][0] * t.j[2][2], a11 = t.j[0][0] * t.j[2][2] - t.j[0][2] * t.j[2][0],
                  a12 = t.j[0][2] * t.j[1][0] - t.j[0][0] * t.j[1][2];
      const float a20 = t.j[1][0] * t.j[2][1] - t.j[1][1] * t.j[2][0], a21 = t.j[0][1] * t.j[2][0] - t.j[0][0] * t.j[2][1],
                  a22 = t.j[0][0] * t.j[1][1] - t.j[0][1] * t.j[1][0];
      const float det = (a00 * t.j[0][0] + a01 * t.j[1][0]) + a02 * t.j[2][0];
      d0 = -(((a00 * t.f[0] + a01 * t.f[1]) + a02 * t.f[2]) / det);
      d1 = -(((a10 * t.f[0] + a11 * t.f[1]) + a12 * t.f[2]) / det);
      d2 = -(((a20 * t.f[0] + a21 * t.f[1]) + a22 * t.f[2]) / det);
      s0 = s0 + d0;
      s1 = s1 + d1;
      s2 = s2 + d2;
    }
    const bool finite = __builtin_isfinite(s0) && __builtin_isfinite(s1) && __builtin_isfinite(s2) && __builtin_isfinite(d0) &&
                        __builtin_isfinite(d1) && __builtin_isfinite(d2);
    const bool inside = s0 >= 0.f && (s0 < 1.f || (i + 2 == a.nx && s0 <= 1.f)) && s1 >= 0.f && (s1 < 1.f || (j + 2 == a.ny && s1 <= 1.f)) &&
                        s2 >= 0.f && (s2 < 1.f || (k + 2 == a.nz && s2 <= 1.f));
    const float lastStep = fmaxf(fmaxf(fabsf(d0), fabsf(d1)), fabsf(d2));
    result = !finite ? kIsoCriticalNonFinite : (!inside ? kIsoCriticalLeftCell : (!(lastStep <= a.tolerance) ? kIsoCriticalNotConverged : kIsoCriticalFound));
    float *state = a.state + 4 * size_t(n);
    state[0] = s0; state[1] = s1; state[2] = s2; state[3] = lastStep;
    a.result[n] = result;
  }
  const unsigned long long found = __ballot(result == kIsoCriticalFound);
#pragma unroll
  for (int32_t r = kIsoCriticalNonFinite; r <= kIsoCriticalNotConverged; r++) {
    const unsigned long long m = __ballot(result == r);
    if (m && lane == 0u) atomicAdd(a.counters + r, (unsigned long long)__popcll(m));
  }
  if (lane == 0u) lds[wave] = uint32_t(__popcll(found));
  __syncthreads();
  if (threadIdx.x == 0) a.candCount[blockIdx.x] = (lds[0] + lds[1]) + (lds[2] + lds[3]);
}

__global__ __launch_bounds__(kIsoBlock) void isoCriticalEmitKernel(const IsoCriticalArgs a)
{
  __shared__ uint32_t lds[kIsoBlock / 64];
  if (a.candCount[blockIdx.x] == 0) return;           // the same for the whole block
  const uint32_t n = blockIdx.x * kIsoBlock + threadIdx.x;
  const bool found = n < a.numCandidates && a.result[n] == kIsoCriticalFound;
  uint32_t total;
  const uint32_t before = blockScan(found ? 1u : 0u, total, lds);
  if (!found) return;
  const uint64_t index = a.candChunkBase[blockIdx.x / kIsoChunk] + a.candBase[blockIdx.x] + before;     // < numFound
  const uint32_t L = a.candidates[n];
  const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
  const float *state = a.state + 4 * size_t(n);
  const float s0 = state[0], s1 = state[1], s2 = state[2];
  CriticalJet t;
  criticalJet(a, L, s0, s1, s2, t);
  ExaHipCriticalPoint &p = a.points[index];
  static_assert(sizeof(ExaHipCriticalPoint) == 104, "the record: 72 bytes of integers and floats, four doubles, no padding");
  p.cell = L;
  p.local[0] = s0; p.local[1] = s1; p.local[2] = s2;
  const float px = a.lo[0] + ((float(i) + 0.5f) + s0) * a.step[0], py = a.lo[1] + ((float(j) + 0.5f) + s1) * a.step[1],
              pz = a.lo[2] + ((float(k) + 0.5f) + s2) * a.step[2];
  p.position[0] = px; p.position[1] = py; p.position[2] = pz;
  if (a.positions) {
    float *out = a.positions + 3 * index;
    out[0] = px; out[1] = py; out[2] = pz;
  }
  p.lastStep = state[3];
  const float j0 = t.j[0][0] / a.step[0], j1 = t.j[0][1] / a.step[1], j2 = t.j[0][2] / a.step[2];
  const float j3 = t.j[1][0] / a.step[0], j4 = t.j[1][1] / a.step[1], j5 = t.j[1][2] / a.step[2];
  const float j6 = t.j[2][0] / a.step[0], j7 = t.j[2][1] / a.step[1], j8 = t.j[2][2] / a.step[2];
  p.jacobian[0] = j0; p.jacobian[1] = j1; p.jacobian[2] = j2;
  p.jacobian[3] = j3; p.jacobian[4] = j4; p.jacobian[5] = j5;
  p.jacobian[6] = j6; p.jacobian[7] = j7; p.jacobian[8] = j8;
  // the classification, in double from the float32 jacobian
  const double e0 = j0, e1 = j1, e2 = j2, e3 = j3, e4 = j4, e5 = j5, e6 = j6, e7 = j7, e8 = j8;
  const double P = -((e0 + e4) + e8);
  const double Q = ((e0 * e4 - e1 * e3) + (e0 * e8 - e2 * e6)) + (e4 * e8 - e5 * e7);
  const double R = -((e0 * (e4 * e8 - e5 * e7) - e1 * (e3 * e8 - e5 * e6)) + e2 * (e3 * e7 - e4 * e6));
  const double D = (27.0 * (R * R) + (4.0 * ((P * P) * P) - 18.0 * (P * Q)) * R) + (4.0 * ((Q * Q) * Q) - (P * P) * (Q * Q));
  const double num = P * Q - R, third = num / P;
  const bool p1 = P > 0.0, p2 = third > 0.0, p3 = R > 0.0;
  const int32_t nplus = (p1 ? 0 : 1) + (p1 != p2 ? 1 : 0) + (p2 != p3 ? 1 : 0);
  const bool degenerate = P == 0.0 || num == 0.0 || R == 0.0 || !(__builtin_isfinite(P) && __builtin_isfinite(third) && __builtin_isfinite(R));
  p.type = nplus | (D > 0.0 ? EXA_CRITICAL_SPIRAL : 0) | (degenerate ? EXA_CRITICAL_DEGENERATE : 0);
  p.invariants[0] = P; p.invariants[1] = Q; p.invariants[2] = R;
  p.discriminant = D;
}

// the probe's values [n][3] and gradients [n][3][3] into probe [n][3][4]: one lane per point and channel
__global__ __launch_bounds__(kIsoBlock) void isoCriticalPackKernel(const IsoCriticalArgs a)
{
  const uint64_t q = uint64_t(blockIdx.x) * kIsoBlock + threadIdx.x;
  if (q >= 3ull * a.numFound) return;
  const float *g = a.probeGradients + 3 * q;
  float *out = a.probe + 4 * q;
  out[0] = a.probeValues[q];
  out[1] = g[0]; out[2] = g[1]; out[3] = g[2];
}

// ---- profiles and phase plots (exa_hip_profile): the passes of exa_isomesh.h ----
// the lattice position of L in the caller's space, as exa_hip_resample forms it before any world mapping
__device__ __forceinline__ void profilePosition(const IsoProfileArgs &a, uint32_t L, float (&P)[3])
{
  const uint32_t i = L % a.nx, jk = L / a.nx, j = jk % a.ny, k = jk / a.ny;
  P[0] = a.lo[0] + (float(i) + 0.5f) * a.step[0];
  P[1] = a.lo[1] + (float(j) + 0.5f) * a.step[1];
  P[2] = a.lo[2] + (float(k) + 0.5f) * a.step[2];
}

// source `slot` of the call at L; the slot is wave-uniform, and the kinds' and the source's words are read where they are
// needed, not held over the pass
__device__ __forceinline__ float profileSource(const IsoProfileArgs &a, uint32_t slot, uint32_t L, const float (&P)[3])
{
  const IsoProfileSource &s = a.sources[slot];
  const int32_t kind = int32_t((a.kinds >> (4u * slot)) & 15u);
  if (kind == kIsoProfileMemoryKind) return s.values[L];
  if (kind == EXA_SOURCE_COORDINATE) return s.axis == 0 ? P[0] : s.axis == 1 ? P[1] : P[2];
  const float dx = P[0] - s.centre[0], dy = P[1] - s.centre[1], dz = P[2] - s.centre[2];
  return sqrtf((dx * dx + dy * dy) + dz * dz);
}

// the slots of the call's series, the weight's first: [first, end)
__device__ __forceinline__ uint32_t profileFirstSeries(const IsoProfileArgs &a) { return a.hasWeight ? uint32_t(kIsoProfileWeightSlot) : uint32_t(kIsoProfileValueSlot); }
__device__ __forceinline__ uint32_t profileEndSeries(const IsoProfileArgs &a) { return uint32_t(kIsoProfileValueSlot) + a.numValues; }

// The key of axis ax (wave-uniform) at L: false if it is NaN.  range: 0, or 1 + ax (under) / 3 + ax (over) of the first axis
// out of range; bin: the axis' part of the bin index, times `stride`, where the key is in range.
__device__ __forceinline__ bool profileKey(const IsoProfileArgs &a, uint32_t ax, uint32_t L, const float (&P)[3], uint32_t stride,
                                           uint32_t &range, uint32_t &bin)
{
  const IsoProfileKey &key = a.axes[ax];
  const float x = profileSource(a, ax, L, P);
  if (x != x) return false;
  const bool under = x < key.lo, over = x > key.hi;     // edges: lo, hi = the first and the last edge
  if (!range) range = under ? 1u + ax : over ? 3u + ax : 0u;
  uint32_t b = 0;
  if (!under && !over) {
    if (key.mode == kIsoProfileUniform) {
      const float t = (x - key.lo) * key.scale;
      b = uint32_t(min(key.numBins - 1, int32_t(t)));
    } else {
      // the last b with edges[b] <= x, which for x == edges[numBins] is numBins - 1: the last bin is closed
      uint32_t top = uint32_t(key.numBins);
      while (top - b > 1u) {
        const uint32_t mid = (b + top) >> 1;
        if (key.edges[mid] <= x) b = mid; else top = mid;
      }
    }
  }
  bin += b * stride;
  return true;
}

// The series go one after the other in loops that are not unrolled, and what a lane learns of one of them does not wait in
// a register for the others: unrolled over the seven sources, the pass held every source's words in scalar registers and
// spilled 34 of them.
__global__ __launch_bounds__(kIsoBlock) void isoProfileClassifyKernel(const IsoProfileArgs a)
{
  constexpr int kCounts = kIsoProfileBinned + 1;
  __shared__ uint32_t sStat[kCounts + kIsoProfileSeries];
  if (threadIdx.x < kCounts + kIsoProfileSeries) sStat[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t n[kCounts] = {};                             // per lane
#pragma unroll 1
  for (uint32_t t = 0; t < kIsoProfileTiles; t++) {
    const uint64_t first = (uint64_t(blockIdx.x) * kIsoProfileTiles + t) * kIsoBlock;
    if (first >= a.numPoints) break;                    // block-uniform
    const bool there = first + threadIdx.x < a.numPoints;
    const uint32_t L = there ? uint32_t(first) + threadIdx.x : 0u;      // a lane beyond the lattice reads point 0 and counts nothing
    float P[3] = { 0.f, 0.f, 0.f };
    if (a.needPosition) profilePosition(a, L, P);
    bool outside = false, valid = true;
    uint32_t range = 0, bin = 0;
    uint32_t stride = 1;
#pragma unroll 1
    for (uint32_t ax = 0; ax < a.numAxes; ax++) {
      if (a.axes[ax].mode == kIsoProfileLabels) {       // the first axis only
        const int32_t label = a.labels[L];
        outside = label < 0;
        if (there && label >= a.axes[ax].numBins) atomicMin(a.counters + kIsoProfileBadLabel, (unsigned long long)L);
        bin = uint32_t(label);
      } else {
        valid = profileKey(a, ax, L, P, stride, range, bin) && valid;
      }
      stride *= uint32_t(a.axes[ax].numBins);
    }
    const uint32_t sBegin = profileFirstSeries(a), sEnd = profileEndSeries(a);
    float w = 1.f;
#pragma unroll 1
    for (uint32_t q = sBegin; q < sEnd; q++) {
      const float x = profileSource(a, q, L, P);
      if (q == uint32_t(kIsoProfileWeightSlot)) w = x;
      // w * x: the term of a value (1 * x without a weight)
      valid = valid && __builtin_isfinite(x) && (q == uint32_t(kIsoProfileWeightSlot) || __builtin_isfinite(w * x));
    }
    const bool binned = there && !outside && valid && !range;
    n[kIsoProfileOutside] += there && outside;
    n[kIsoProfileInvalid] += there && !outside && !valid;
#pragma unroll
    for (uint32_t c = 0; c < 4; c++) n[kIsoProfileUnder + c] += there && !outside && valid && range == c + 1u;
    n[kIsoProfileBinned] += binned;
    if (there) a.bins[L] = binned ? bin : kIsoProfileUnbinned;
    // the largest |term| of every series over the wave's binned points (its bits order as unsigned integers), once more
    // series by series: whether a point is binned hangs on all of them
    if (__ballot(binned)) {                             // wave-uniform
#pragma unroll 1
      for (uint32_t q = sBegin; q < sEnd; q++) {
        const float x = profileSource(a, q, L, P);
        const float term = q == uint32_t(kIsoProfileWeightSlot) || !a.hasWeight ? x : w * x;
        uint32_t m = binned ? __float_as_uint(term) & 0x7fffffffu : 0u;
#pragma unroll
        for (int o = 32; o; o >>= 1) {
          const uint32_t other = uint32_t(__shfl_xor(int(m), o));
          m = other > m ? other : m;
        }
        if (lane == 0u && m) atomicMax(&sStat[kCounts + q - uint32_t(kIsoProfileWeightSlot)], m);
      }
    }
  }
  for (int o = 32; o; o >>= 1) {
#pragma unroll
    for (int c = 0; c < kCounts; c++) n[c] += uint32_t(__shfl_xor(int(n[c]), o));
  }
  if (lane == 0u) {
#pragma unroll
    for (int c = 0; c < kCounts; c++) if (n[c]) atomicAdd(&sStat[c], n[c]);
  }
  __syncthreads();
  // one set of atomics per block of the launch
  if (threadIdx.x < kCounts + kIsoProfileSeries) {
    const uint32_t x = sStat[threadIdx.x];
    if (x && threadIdx.x < kCounts) atomicAdd(a.counters + threadIdx.x, (unsigned long long)x);
    if (x && threadIdx.x >= kCounts) atomicMax(reinterpret_cast<uint32_t *>(a.counters + kIsoProfileCounters) + (threadIdx.x - kCounts), x);
  }
}

// what a lane, or the lanes of a wave that share a bin, add to the bin's record for one series
struct ProfilePart {
  uint32_t count;
  long long sum;
  uint32_t keyMin, keyMax;
};

__device__ __forceinline__ ProfilePart profileNothing() { return { 0u, 0ll, 0xffffffffu, 0u }; }

__device__ __forceinline__ void profileReduce(ProfilePart &p)
{
#pragma unroll
  for (int o = 32; o; o >>= 1) {
    p.count += uint32_t(__shfl_xor(int(p.count), o));
    p.sum += __shfl_xor(p.sum, o);
    const uint32_t kmin = uint32_t(__shfl_xor(int(p.keyMin), o)), kmax = uint32_t(__shfl_xor(int(p.keyMax), o));
    p.keyMin = kmin < p.keyMin ? kmin : p.keyMin;
    p.keyMax = kmax > p.keyMax ? kmax : p.keyMax;
  }
}

// The table the accumulate pass adds to: the call's in HBM, or the workgroup's copy in LDS, whose counts are 32 bit and which
// always has the weight's column.
template <bool LDS>
struct ProfileTable {
  typedef typename std::conditional<LDS, uint32_t, unsigned long long>::type Count;
  unsigned long long *sums;
  Count *count;
  uint32_t *keyMin, *keyMax;
};

// one series' part into record `bin`: the count with the first series, the sum into column `column` if the call has a
// series at all, the keys of value `value` where it is one and min / max are asked for (all wave-uniform)
template <bool LDS>
__device__ __forceinline__ void profileAdd(const ProfileTable<LDS> &t, uint32_t numBins, uint32_t bin, const ProfilePart &p,
                                           bool withCount, bool withSum, uint32_t column, bool withKeys, uint32_t value)
{
  if (withCount) atomicAdd(t.count + bin, typename ProfileTable<LDS>::Count(p.count));
  if (withSum) atomicAdd(t.sums + size_t(column) * numBins + bin, (unsigned long long)p.sum);
  if (withKeys) {
    atomicMin(t.keyMin + size_t(value) * numBins + bin, p.keyMin);
    atomicMax(t.keyMax + size_t(value) * numBins + bin, p.keyMax);
  }
}

// A workgroup goes over its tiles once per series (once for the count alone where the call has none): the bin indices come
// out of the cache from the second time on, and a pass holds one source, one sum and one pair of keys.
template <bool LDS>
__global__ __launch_bounds__(kIsoBlock) void isoProfileAccumulateKernel(const IsoProfileArgs a)
{
  extern __shared__ unsigned long long profileLds[];
  const uint32_t B = a.numBins, nv = a.numValues, lane = threadIdx.x & 63u;
  ProfileTable<LDS> table;
  if constexpr (LDS) {
    table.sums = profileLds;
    table.count = reinterpret_cast<uint32_t *>(profileLds + size_t(1u + nv) * B);
    table.keyMin = table.count + B;
    table.keyMax = table.keyMin + size_t(nv) * B;
    for (uint32_t b = threadIdx.x; b < (1u + nv) * B; b += kIsoBlock) table.sums[b] = 0ull;
    for (uint32_t b = threadIdx.x; b < B; b += kIsoBlock) table.count[b] = 0;
    for (uint32_t b = threadIdx.x; b < nv * B; b += kIsoBlock) { table.keyMin[b] = 0xffffffffu; table.keyMax[b] = 0u; }
    __syncthreads();
  } else {
    table.sums = a.sums;
    table.count = a.count;
    table.keyMin = a.keyMin; table.keyMax = a.keyMax;
  }
  const uint32_t sBegin = profileFirstSeries(a), sEnd = profileEndSeries(a);
  const bool anySeries = sEnd > sBegin;
#pragma unroll 1
  for (uint32_t q = sBegin; q < (anySeries ? sEnd : sBegin + 1u); q++) {
    const bool withCount = q == sBegin, isValue = anySeries && q >= uint32_t(kIsoProfileValueSlot);
    const bool withKeys = isValue && a.minMax, weighted = isValue && a.hasWeight;
    const uint32_t value = q - uint32_t(kIsoProfileValueSlot);
    // the column of the series: the copy in LDS always has the weight's in front, the table only where there is a weight
    const uint32_t column = LDS ? q - uint32_t(kIsoProfileWeightSlot) : q - sBegin;
    const int32_t exponent = a.exponent[q - uint32_t(kIsoProfileWeightSlot)];
#pragma unroll 1
    for (uint32_t t = 0; t < kIsoProfileTiles; t++) {
      const uint64_t first = (uint64_t(blockIdx.x) * kIsoProfileTiles + t) * kIsoBlock;
      if (first >= a.numPoints) break;                  // block-uniform
      const uint64_t at = first + threadIdx.x;
      const uint32_t L = uint32_t(at);
      const uint32_t bin = at < a.numPoints ? a.bins[L] : kIsoProfileUnbinned;
      bool on = bin < B;                                // the mark is not below B
      ProfilePart own = profileNothing();
      if (on) {
        own.count = 1;
        if (anySeries) {
          float P[3] = { 0.f, 0.f, 0.f };
          if (a.needPosition) profilePosition(a, L, P);
          const float x = profileSource(a, q, L, P);
          const float term = weighted ? profileSource(a, kIsoProfileWeightSlot, L, P) * x : x;
          own.sum = __double2ll_rn(ldexp(double(term), exponent));
          if (withKeys) own.keyMin = own.keyMax = regionKey(x);
        }
      }
      // the bin of the first pending lane is reduced over the wave and added by that lane, twice (recordStats' scheme);
      // what is left then goes lane by lane
      unsigned long long pending = __ballot(on);
#pragma unroll 1
      for (int round = 0; round < 2; round++) {
        if (!pending) break;                            // wave-uniform
        const uint32_t leader = uint32_t(__ffsll(pending)) - 1u;
        const uint32_t lb = uint32_t(__builtin_amdgcn_readlane(int(bin), int(leader)));
        const bool same = on && bin == lb;
        const unsigned long long m = __ballot(same);
        ProfilePart part = own;
        if (!same) part = profileNothing();
        if (__popcll(m) > 1) profileReduce(part);       // wave-uniform
        if (lane == leader) profileAdd(table, B, lb, part, withCount, anySeries, column, withKeys, value);
        on = on && !same;
        pending &= ~m;
      }
      if (on) profileAdd(table, B, bin, own, withCount, anySeries, column, withKeys, value);
    }
  }
  if constexpr (LDS) {
    // the flush: the records of the copy that hold a point, the only accesses of this variant to the table
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < B; b += kIsoBlock) {
      const uint32_t c = table.count[b];
      if (!c) continue;
      atomicAdd(a.count + b, (unsigned long long)c);
      if (a.hasWeight) atomicAdd(a.sums + b, table.sums[b]);
      for (uint32_t f = 0; f < nv; f++) {
        atomicAdd(a.sums + size_t(a.hasWeight + f) * B + b, table.sums[size_t(1u + f) * B + b]);
        if (!a.minMax) continue;
        atomicMin(a.keyMin + size_t(f) * B + b, table.keyMin[size_t(f) * B + b]);
        atomicMax(a.keyMax + size_t(f) * B + b, table.keyMax[size_t(f) * B + b]);
      }
    }
  }
}

// min and max of every bin and value out of the keys, in place; an empty bin holds +INFINITY / -INFINITY
__global__ __launch_bounds__(kIsoBlock) void isoProfileFinishKernel(const IsoProfileArgs a)
{
  const uint64_t at = uint64_t(blockIdx.x) * kIsoBlock + threadIdx.x;
  if (at >= uint64_t(a.numValues) * a.numBins) return;
  const bool any = a.count[at % a.numBins] != 0ull;
  a.keyMin[at] = any ? __float_as_uint(regionValueOfKey(a.keyMin[at])) : 0x7f800000u;
  a.keyMax[at] = any ? __float_as_uint(regionValueOfKey(a.keyMax[at])) : 0xff800000u;
}

// ---- exact Euclidean distance transform (exa_hip_distance): the passes of exa_isomesh.h ----
// term_a(d) of the contract: two roundings, nothing contracted
__device__ __forceinline__ float distanceTerm(float h, uint32_t d)
{
  const float o = h * float(d);
  return o * o;
}

// A count and the bits of a non-negative float of every lane, over the block, to counters[countSlot] and to the low word of
// counters[bitsSlot]: one atomic each per block.  Every lane of the block comes here.
__device__ __forceinline__ void distanceTotals(const IsoDistanceArgs &a, uint32_t *lds, uint32_t count, uint32_t bits, int countSlot, int bitsSlot)
{
  for (int o = 32; o; o >>= 1) {
    const uint32_t m = uint32_t(__shfl_xor(int(bits), o));
    bits = m > bits ? m : bits;
    count += uint32_t(__shfl_xor(int(count), o));
  }
  if ((threadIdx.x & 63u) == 0u) { lds[threadIdx.x >> 6] = count; lds[kIsoBlock / 64 + (threadIdx.x >> 6)] = bits; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0, top = 0;
    for (uint32_t w = 0; w < kIsoBlock / 64; w++) {
      sum += lds[w];
      top = lds[kIsoBlock / 64 + w] > top ? lds[kIsoBlock / 64 + w] : top;
    }
    if (sum) atomicAdd(a.counters + countSlot, (unsigned long long)sum);
    if (top) atomicMax(reinterpret_cast<uint32_t *>(a.counters + bitsSlot), top);
  }
}

__global__ __launch_bounds__(kIsoBlock) void isoDistanceInsideKernel(const IsoDistanceArgs a)
{
  __shared__ uint32_t lds[2 * (kIsoBlock / 64)];
  uint32_t count = 0;
  for (uint32_t t = 0; t < kIsoDistanceTiles; t++) {
    const uint64_t at = (uint64_t(blockIdx.x) * kIsoDistanceTiles + t) * kIsoBlock + threadIdx.x;
    if (at >= a.numPoints) break;
    bool in;
    if (a.byLabel) {
      const int32_t l = a.labels[at];
      in = a.label < 0 ? l >= 0 : l == a.label;
    } else {
      in = regionInside(a, a.values[at]);
    }
    a.inside[at] = in ? 1 : 0;
    count += in ? 1u : 0u;
  }
  distanceTotals(a, lds, count, 0u, kIsoDistanceInside, kIsoDistanceMaxBits);
}

__device__ __forceinline__ bool distanceTarget(const IsoDistanceArgs &a, const uint8_t *row, uint32_t x)
{
  return x < a.nx && (row[x] != 0) != (a.toOutside != 0);
}

// A wave per row.  `last`: the largest target of the chunks behind this one; `next`: the smallest target of the chunks in
// (c, looked), which the look-ahead has read, -1 if they hold none.  Every chunk is looked at once ahead and once in turn.
__global__ __launch_bounds__(kIsoBlock) void isoDistanceRowKernel(const IsoDistanceArgs a)
{
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t row = uint64_t(blockIdx.x) * (kIsoBlock / 64) + (threadIdx.x >> 6);
  if (row >= uint64_t(a.ny) * a.nz) return;
  const uint8_t *bits = a.inside + row * a.nx;
  int32_t *out = a.a + row * a.nx;
  const uint32_t chunks = (a.nx + 63u) / 64u;
  const uint64_t atOrBelow = (2ull << lane) - 1ull, atOrAbove = ~((1ull << lane) - 1ull);
  int32_t last = -1, next = -1;
  uint32_t looked = 0;
  for (uint32_t c = 0; c < chunks; c++) {
    const uint32_t x = c * 64u + lane;
    const uint64_t m = __ballot(distanceTarget(a, bits, x));
    if (next >= 0 && uint32_t(next) < (c + 1u) * 64u) next = -1;        // it lies in this chunk now
    if (looked < c + 1u) looked = c + 1u;
    while (next < 0 && looked < chunks) {
      const uint64_t f = __ballot(distanceTarget(a, bits, looked * 64u + lane));
      if (f) next = int32_t(looked * 64u + uint32_t(__builtin_ctzll(f)));
      looked++;
    }
    const uint64_t lowm = m & atOrBelow, highm = m & atOrAbove;
    const int32_t lo = lowm ? int32_t(c * 64u + 63u - uint32_t(__builtin_clzll(lowm))) : last;
    const int32_t hi = highm ? int32_t(c * 64u + uint32_t(__builtin_ctzll(highm))) : next;
    if (x < a.nx) out[x] = (lo < 0 || (hi >= 0 && uint32_t(hi) - x < x - uint32_t(lo))) ? hi : lo;     // of two, the smaller
    if (m) last = int32_t(c * 64u + 63u - uint32_t(__builtin_clzll(m)));
  }
}

// The scan of one point at position p of an axis of n points: value(q) is gx or gy at position q of the point's column.
// best / arg: the minimum of value(q) + term(|p - q|) and the smallest q that holds it, -1 where the minimum is +INF.
template <typename F>
__device__ __forceinline__ void distanceScan(uint32_t p, uint32_t n, float h, float limit, F value, float &best, int32_t &arg)
{
  best = value(p);                                      // + term(0), which is +0
  arg = best < INFINITY ? int32_t(p) : -1;
  const uint32_t reach = p > n - 1u - p ? p : n - 1u - p, above = n - p;
  // one step: the candidates at distance d on both sides; a side that has left the axis reads position p and counts as +INF
  auto step = [&](uint32_t d, float t, float below, float over) {
    const float vm = d <= p ? below + t : INFINITY, vp = d < above ? over + t : INFINITY;
    if (vm < INFINITY && vm <= best) { best = vm; arg = int32_t(p - d); }
    if (vp < best) { best = vp; arg = int32_t(p + d); }
  };
  // two steps per round, their four loads issued together ahead of the first stop test: the loads of the second step are
  // wasted where the first one ends the scan, and hide each other's latency on a long one
  for (uint32_t d = 1; d <= reach; d += 2) {
    const float t0 = distanceTerm(h, d), t1 = distanceTerm(h, d + 1u);
    const float m0 = value(d <= p ? p - d : p), p0 = value(d < above ? p + d : p);
    const float m1 = value(d + 1u <= p ? p - d - 1u : p), p1 = value(d + 1u < above ? p + d + 1u : p);
    if (t0 > fminf(best, limit)) break;
    step(d, t0, m0, p0);
    if (d + 1u > reach || t1 > fminf(best, limit)) break;
    step(d + 1u, t1, m1, p1);
  }
}

template <int AXIS>
__device__ __forceinline__ float distanceColumnValue(const IsoDistanceArgs &a, uint64_t at, uint32_t i)
{
  if (AXIS == 2) return a.gy[at];
  const int32_t t = a.a[at];
  return t < 0 ? INFINITY : distanceTerm(a.h[0], uint32_t(t) > i ? uint32_t(t) - i : i - uint32_t(t));
}

template <int AXIS>
__device__ __forceinline__ void distanceColumnStore(const IsoDistanceArgs &a, uint64_t at, float best, int32_t arg)
{
  (AXIS == 1 ? a.b : a.c)[at] = arg;
  (AXIS == 1 ? a.gy : a.d2)[at] = best;
}

template <int AXIS>
__global__ __launch_bounds__(kIsoBlock) void isoDistanceColumnKernel(const IsoDistanceArgs a)
{
  const uint64_t at = uint64_t(blockIdx.x) * kIsoBlock + threadIdx.x;
  if (at >= a.numPoints) return;
  const uint32_t L = uint32_t(at), i = L % a.nx, row = L / a.nx;
  const uint32_t n = AXIS == 1 ? a.ny : a.nz, p = AXIS == 1 ? row % a.ny : row / a.ny;
  const uint64_t stride = AXIS == 1 ? uint64_t(a.nx) : uint64_t(a.nx) * a.ny, base = at - p * stride;
  float best;
  int32_t arg;
  distanceScan(p, n, a.h[AXIS], a.limit, [&](uint32_t q) { return distanceColumnValue<AXIS>(a, base + q * stride, i); }, best, arg);
  distanceColumnStore<AXIS>(a, at, best, arg);
}

#if EXA_DISTANCE_LDS
// The column pass out of a slab in LDS: a block takes 64 columns (consecutive x) of one plane of the scan (AXIS 1: the plane
// k = blockIdx.y, AXIS 2: the plane j = blockIdx.y), stages value(q) of all n <= kIsoDistanceLdsAxis positions, 64 floats a
// row (a wave's access is one bank row, no conflicts), and its four waves take the positions in turn.
template <int AXIS>
__global__ __launch_bounds__(kIsoBlock) void isoDistanceColumnLdsKernel(const IsoDistanceArgs a)
{
  extern __shared__ float slab[];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, i = blockIdx.x * 64u + lane;
  const uint32_t n = AXIS == 1 ? a.ny : a.nz;
  const uint64_t stride = AXIS == 1 ? uint64_t(a.nx) : uint64_t(a.nx) * a.ny;
  const uint64_t base = (AXIS == 1 ? uint64_t(blockIdx.y) * a.ny * a.nx : uint64_t(blockIdx.y) * a.nx) + i;
  for (uint32_t q = wave; q < n; q += kIsoBlock / 64)
    slab[q * 64u + lane] = i < a.nx ? distanceColumnValue<AXIS>(a, base + q * stride, i) : INFINITY;
  __syncthreads();
  if (i >= a.nx) return;
  for (uint32_t p = wave; p < n; p += kIsoBlock / 64) {
    float best;
    int32_t arg;
    distanceScan(p, n, a.h[AXIS], a.limit, [&](uint32_t q) { return slab[q * 64u + lane]; }, best, arg);
    distanceColumnStore<AXIS>(a, base + p * stride, best, arg);
  }
}
#endif

__global__ __launch_bounds__(kIsoBlock) void isoDistanceFinishKernel(const IsoDistanceArgs a)
{
  __shared__ uint32_t lds[2 * (kIsoBlock / 64)];
  uint32_t count = 0, top = 0;
  for (uint32_t t = 0; t < kIsoDistanceTiles; t++) {
    const uint64_t at = (uint64_t(blockIdx.x) * kIsoDistanceTiles + t) * kIsoBlock + threadIdx.x;
    if (at >= a.numPoints) break;
    if (a.onlyOthers && (a.inside[at] != 0) != (a.toOutside != 0)) continue;
    const float d2 = a.d2[at];
    const bool reached = d2 <= a.limit && d2 < INFINITY;
    const float d = reached ? sqrtf(d2) : INFINITY;
    a.dist[at] = a.negative ? -d : d;
    if (reached) {
      const uint32_t bits = __float_as_uint(d);
      top = bits > top ? bits : top;
      count++;
    }
    if (a.nearest) {
      int32_t to = -1;
      if (reached) {
        const uint32_t L = uint32_t(at), i = L % a.nx, j = (L / a.nx) % a.ny;
        const uint64_t plane = uint64_t(uint32_t(a.c[at])) * a.ny;
        const uint32_t b = uint32_t(a.b[(plane + j) * a.nx + i]);
        to = int32_t((plane + b) * a.nx + uint32_t(a.a[(plane + b) * a.nx + i]));
      }
      a.nearest[at] = to;
    }
  }
  distanceTotals(a, lds, count, top, kIsoDistanceReached, kIsoDistanceMaxBits);
}

// ---- the launchers: every kernel runs in blocks of kIsoBlock lanes and takes its argument struct by value ----
template <typename A>
hipError_t launch(void (*kernel)(A), dim3 grid, hipStream_t s, const A &a)
{
  hipLaunchKernelGGL(kernel, grid, dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

// blocks of `per` items that hold n of them
constexpr uint32_t blocksOf(uint64_t n, uint32_t per = kIsoBlock) { return uint32_t((n + per - 1) / per); }

} // namespace

hipError_t launchIsoScans(const IsoScanArgs &a, int counts, hipStream_t s)
{
  hipError_t e = launch(isoScanChunksKernel, dim3(a.numChunks, counts), s, a);
  if (e == hipSuccess) e = launch(isoScanTopKernel, dim3(counts), s, a);
  return e;
}

hipError_t launchIsoCubePass(const IsoMeshArgs &a, hipStream_t s) { return launch(isoCubeKernel, a.numBlocks, s, a); }
hipError_t launchIsoPointPass(const IsoMeshArgs &a, hipStream_t s) { return launch(isoPointKernel, a.numBlocks, s, a); }
hipError_t launchIsoEmit(const IsoMeshArgs &a, hipStream_t s)
{
  hipError_t e = launch(isoEmitVerticesKernel, a.numBlocks, s, a);
  if (e == hipSuccess) e = launch(isoEmitTrianglesKernel, a.numBlocks, s, a);
  return e;
}

hipError_t launchIsolinePositions(const IsoLineArgs &a, hipStream_t s) { return launch(isolinePositionsKernel, a.numBlocks, s, a); }
hipError_t launchIsolineSquarePass(const IsoLineArgs &a, hipStream_t s) { return launch(isolineSquareKernel, a.numBlocks, s, a); }
hipError_t launchIsolinePointPass(const IsoLineArgs &a, hipStream_t s) { return launch(isolinePointKernel, a.numBlocks, s, a); }
hipError_t launchIsolineEmit(const IsoLineArgs &a, hipStream_t s)
{
  hipError_t e = launch(isolineEmitVerticesKernel, a.numBlocks, s, a);
  if (e == hipSuccess) e = launch(isolineEmitSegmentsKernel, a.numBlocks, s, a);
  return e;
}

hipError_t launchIsoRegionInit(const IsoRegionArgs &a, hipStream_t s) { return launch(isoRegionInitKernel, blocksOf(a.numBlocks, kIsoRegionTiles), s, a); }
hipError_t launchIsoRegionMerge(const IsoRegionArgs &a, hipStream_t s) { return launch(isoRegionMergeKernel, a.numBlocks, s, a); }
hipError_t launchIsoRegionFlatten(const IsoRegionArgs &a, hipStream_t s) { return launch(isoRegionFlattenKernel, a.numBlocks, s, a); }
hipError_t launchIsoRegionRank(const IsoRegionArgs &a, hipStream_t s) { return launch(isoRegionRankKernel, a.numBlocks, s, a); }
// the labels and the measurements, then min / max / argMin / argMax out of the keys
hipError_t launchIsoRegionStats(const IsoRegionArgs &a, hipStream_t s)
{
  hipError_t e = launch(isoRegionStatsKernel, blocksOf(a.numBlocks, kIsoRegionTiles), s, a);
  if (e == hipSuccess) e = launch(isoRegionFinishKernel, blocksOf(a.numRegions), s, a);
  return e;
}

// the regions' init pass as it is: comp[L] = L or the outside mark, the inside count and max |V| into totals[1], totals[2]
hipError_t launchIsoBasinInit(const IsoBasinArgs &a, hipStream_t s)
{
  IsoRegionArgs r = {};
  r.values = a.values; r.numPoints = a.numPoints; r.nx = a.nx; r.ny = a.ny; r.nz = a.nz;
  r.iso = a.iso; r.below = a.below; r.faces = a.faces;
  r.parent = a.comp; r.numBlocks = a.numBlocks; r.numChunks = a.numChunks; r.totals = a.totals; r.errorFlag = a.errorFlag;
  return launchIsoRegionInit(r, s);
}

hipError_t launchIsoBasinUp(const IsoBasinArgs &a, hipStream_t s) { return launch(isoBasinUpKernel, a.numBlocks, s, a); }
// one pass of pointer doubling over array[0, size); *jumpCount, zeroed by the caller, counts the waves that are not done
hipError_t launchIsoBasinJump(const IsoBasinArgs &a, uint32_t *array, uint32_t size, hipStream_t s)
{
  IsoBasinArgs j = a;
  j.jumpArray = array; j.jumpSize = size;
  return launch(isoBasinJumpKernel, blocksOf(size), s, j);
}
// the fixed points of array[0, size) per block into blockCount
hipError_t launchIsoBasinCount(const IsoBasinArgs &a, uint32_t *array, uint32_t size, hipStream_t s)
{
  IsoBasinArgs j = a;
  j.jumpArray = array; j.jumpSize = size;
  return launch(isoBasinCountKernel, blocksOf(size), s, j);
}
// the peaks' raw numbers, then every point's
hipError_t launchIsoBasinRank(const IsoBasinArgs &a, hipStream_t s)
{
  hipError_t e = launch(isoBasinRankKernel, a.numBlocks, s, a);
  if (e == hipSuccess) e = launch(isoBasinLabelKernel, a.numBlocks, s, a);
  return e;
}
hipError_t launchIsoBasinPass(const IsoBasinArgs &a, hipStream_t s) { return launch(isoBasinPassKernel, a.numBlocks, s, a); }
hipError_t launchIsoBasinLink(const IsoBasinArgs &a, hipStream_t s) { return launch(isoBasinLinkKernel, blocksOf(a.numRaw), s, a); }
hipError_t launchIsoBasinMerge(const IsoBasinArgs &a, hipStream_t s) { return launch(isoBasinMergeKernel, a.numBlocks, s, a); }
hipError_t launchIsoBasinFinal(const IsoBasinArgs &a, hipStream_t s) { return launch(isoBasinFinalKernel, blocksOf(a.numRaw), s, a); }
// the labels and the measurements, then what the keys and the last round's words hold
hipError_t launchIsoBasinStats(const IsoBasinArgs &a, hipStream_t s)
{
  hipError_t e = launch(isoBasinStatsKernel, blocksOf(a.numBlocks, kIsoRegionTiles), s, a);
  if (e == hipSuccess) e = launch(isoBasinFirstKernel, a.numBlocks, s, a);
  if (e == hipSuccess) e = launch(isoBasinFinishKernel, blocksOf(a.numBasins), s, a);
  return e;
}

hipError_t launchIsoLatticeStretch(const IsoStretchArgs &a, hipStream_t s) { return launch(isoLatticeStretchKernel, blocksOf(a.numPoints), s, a); }

hipError_t launchIsoCriticalCells(const IsoCriticalArgs &a, hipStream_t s) { return launch(isoCriticalCellKernel, blocksOf(a.numBlocks, kIsoCriticalTiles), s, a); }
hipError_t launchIsoCriticalCompact(const IsoCriticalArgs &a, hipStream_t s) { return launch(isoCriticalCompactKernel, a.numBlocks, s, a); }
hipError_t launchIsoCriticalRefine(const IsoCriticalArgs &a, hipStream_t s) { return launch(isoCriticalRefineKernel, a.numCandBlocks, s, a); }
hipError_t launchIsoCriticalEmit(const IsoCriticalArgs &a, hipStream_t s) { return launch(isoCriticalEmitKernel, a.numCandBlocks, s, a); }
hipError_t launchIsoCriticalPack(const IsoCriticalArgs &a, hipStream_t s) { return launch(isoCriticalPackKernel, blocksOf(3ull * a.numFound), s, a); }

hipError_t launchIsoProfileClassify(const IsoProfileArgs &a, hipStream_t s) { return launch(isoProfileClassifyKernel, blocksOf(a.numBlocks, kIsoProfileTiles), s, a); }
// the workgroup's copy of a small table in dynamic shared memory, else the atomics straight to the table
hipError_t launchIsoProfileAccumulate(const IsoProfileArgs &a, hipStream_t s)
{
  const dim3 grid(blocksOf(a.numBlocks, kIsoProfileTiles));
  if (isoProfileLdsTable(a.numBins, a.numValues))
    hipLaunchKernelGGL(isoProfileAccumulateKernel<true>, grid, dim3(kIsoBlock), a.numBins * kIsoProfileLdsBinBytes(a.numValues), s, a);
  else
    hipLaunchKernelGGL(isoProfileAccumulateKernel<false>, grid, dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}
hipError_t launchIsoProfileFinish(const IsoProfileArgs &a, hipStream_t s) { return launch(isoProfileFinishKernel, blocksOf(uint64_t(a.numValues) * a.numBins), s, a); }

hipError_t launchIsoDistanceInside(const IsoDistanceArgs &a, hipStream_t s) { return launch(isoDistanceInsideKernel, blocksOf(a.numBlocks, kIsoDistanceTiles), s, a); }
hipError_t launchIsoDistanceRows(const IsoDistanceArgs &a, hipStream_t s) { return launch(isoDistanceRowKernel, blocksOf(uint64_t(a.ny) * a.nz, kIsoBlock / 64), s, a); }
hipError_t launchIsoDistanceFinish(const IsoDistanceArgs &a, hipStream_t s) { return launch(isoDistanceFinishKernel, blocksOf(a.numBlocks, kIsoDistanceTiles), s, a); }

hipError_t launchIsoDistanceColumns(const IsoDistanceArgs &a, int axis, hipStream_t s)
{
#if EXA_DISTANCE_LDS
  // the slab where the axis fits it and the planes fit the grid's second dimension
  const uint32_t n = axis == 1 ? a.ny : a.nz, planes = axis == 1 ? a.nz : a.ny;
  if (n <= kIsoDistanceLdsAxis && planes <= 65535u) {
    const dim3 grid(blocksOf(a.nx, 64), planes);
    if (axis == 1) hipLaunchKernelGGL(isoDistanceColumnLdsKernel<1>, grid, dim3(kIsoBlock), n * 64u * sizeof(float), s, a);
    else hipLaunchKernelGGL(isoDistanceColumnLdsKernel<2>, grid, dim3(kIsoBlock), n * 64u * sizeof(float), s, a);
    return hipGetLastError();
  }
#endif
  return axis == 1 ? launch(isoDistanceColumnKernel<1>, a.numBlocks, s, a) : launch(isoDistanceColumnKernel<2>, a.numBlocks, s, a);
}

} // namespace exa
