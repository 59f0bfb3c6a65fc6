// exa_isomesh.hip — the kernels of exa_hip_isosurface: classify, count, scan, emit (exa_isomesh.h describes the pipeline,
// include/exa_hip.h the contract).  A translation unit of its own: nothing of the renderer or of the probes is compiled
// here, the lattice values arrive in a device buffer.  Compiled with -ffp-contract=off: a vertex position is
// P(p) + t * (P(q) - P(p)) with every operation rounded separately.  Behind them the kernels of exa_hip_isolines, the same
// pipeline on the squares of a plane lattice (isoline...Kernel), which shares the block scan and the scans.
#include "exa_isomesh.h"

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

// ---- scans: blockIdx.y = 0 vertices, 1 triangles ----
__global__ __launch_bounds__(kIsoBlock) void isoScanChunksKernel(const IsoMeshArgs a)
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

__global__ __launch_bounds__(kIsoBlock) void isoScanTopKernel(const IsoMeshArgs a)
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

} // namespace

hipError_t launchIsolinePositions(const IsoLineArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isolinePositionsKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launchIsolineSquarePass(const IsoLineArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isolineSquareKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launchIsolinePointPass(const IsoLineArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isolinePointKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

// the iso-surface's scans over the block counts of the two passes: they read nothing of their arguments but these
hipError_t launchIsolineScans(const IsoLineArgs &a, hipStream_t s)
{
  IsoMeshArgs m = {};
  m.numBlocks = a.numBlocks; m.numChunks = a.numChunks;
  m.blockCount = a.blockCount; m.blockBase = a.blockBase; m.chunkBase = a.chunkBase; m.totals = a.totals;
  return launchIsoScans(m, s);
}

hipError_t launchIsolineEmit(const IsoLineArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isolineEmitVerticesKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(isolineEmitSegmentsKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launchIsoCubePass(const IsoMeshArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isoCubeKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launchIsoPointPass(const IsoMeshArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isoPointKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launchIsoScans(const IsoMeshArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isoScanChunksKernel, dim3(a.numChunks, 2), dim3(kIsoBlock), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(isoScanTopKernel, dim3(2), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

hipError_t launchIsoEmit(const IsoMeshArgs &a, hipStream_t s)
{
  hipLaunchKernelGGL(isoEmitVerticesKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(isoEmitTrianglesKernel, dim3(a.numBlocks), dim3(kIsoBlock), 0, s, a);
  return hipGetLastError();
}

} // namespace exa
