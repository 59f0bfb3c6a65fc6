// exa_histogram.hip — the kernels of exa_hip_histogram (exa_histogram.h describes the pass): histKernel<true> bins,
// histKernel<false> is the range-only pass with the binning compiled out.  Independent of the basis form.
#include "exa_histogram.h"

#include "../../include/exa_hip.h"

namespace exa {

namespace {

__device__ __forceinline__ uint32_t orderedKey(float v)
{
  const uint32_t b = __float_as_uint(v);
  return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// Adds one to counters[bin] for every lane with `on`.  Real fields put most cells into a few bins (background), and 64
// lanes on one LDS counter serialise: the bin of the first pending lane is peeled off twice — its lanes are counted with
// a ballot and added by one lane — and only what is left after that goes lane by lane.  A constant field costs one add
// per wave-load, a two-valued one two; a wave of 64 distinct bins pays the two peels on top of its 64 adds.
__device__ __forceinline__ void addBins(uint32_t *counters, uint32_t bin, bool on, uint32_t lane)
{
  unsigned long long pending = __ballot(on);
#pragma unroll
  for (int round = 0; round < 2; round++) {
    if (!pending) return;                                        // wave-uniform
    const uint32_t leader = uint32_t(__ffsll(pending)) - 1u;
    const uint32_t lb = uint32_t(__builtin_amdgcn_readlane(int(bin), int(leader)));
    const bool same = on && bin == lb;
    const unsigned long long m = __ballot(same);
    if (lane == leader) atomicAdd(&counters[lb], uint32_t(__popcll(m)));
    on = on && !same;
    pending &= ~m;
  }
  if (on) atomicAdd(&counters[bin], 1u);
}

template <bool BINS>
__global__ __launch_bounds__(kHistBlock) void histKernel(const HistArgs a)
{
  __shared__ uint32_t sBins[BINS ? kHistMaxBins : 1];
  __shared__ uint32_t sStat[kHistStatCount];
  __shared__ uint32_t sKey[2];
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t wave = uint32_t(__builtin_amdgcn_readfirstlane(int(tid >> 6)));
  if (BINS)
    for (uint32_t i = tid; i < uint32_t(a.numBins); i += kHistBlock) sBins[i] = 0;
  if (tid < kHistStatCount) sStat[tid] = 0;
  if (tid == 0) { sKey[0] = 0xffffffffu; sKey[1] = 0u; }
  __syncthreads();

  const uint32_t s0 = a.runBegin[blockIdx.x], s1 = a.runBegin[blockIdx.x + 1];
  uint32_t nEmpty = 0, nNan = 0, nUnder = 0, nOver = 0, nBinned = 0;     // per lane
  uint32_t keyMin = 0xffffffffu, keyMax = 0u;                           // per lane
  for (uint32_t s = s0 + wave; s < s1; s += kHistBlock / 64) {
    const HistSeg sg = a.segs[s];
    const int4 b0 = a.bricks[2 * size_t(sg.brick)], b1 = a.bricks[2 * size_t(sg.brick) + 1];
    const int32_t lower[3] = { b0.x, b0.y, b0.z };
    const uint32_t size[3] = { uint32_t(b0.w), uint32_t(b1.x), uint32_t(b1.y) };
    const uint32_t level = uint32_t(b1.z);
    const uint64_t vol = uint64_t(size[0]) * size[1] * size[2];
    const uint64_t first = (uint64_t(sg.z0) * size[1] + sg.y0) * size[0] + sg.x0;
    const uint32_t n = uint32_t(vol - first < kHistSegCells ? vol - first : kHistSegCells);
    // The brick against the box, by its first and last cell centre per axis: 0 = wholly outside (its cells are not
    // touched), 1 = cut (the test per cell), 2 = wholly inside.  The centre rule 2*lo <= 2*p + w < 2*hi (p = lower +
    // idx*w, w = 2^level) is lo <= p + (w >> 1) < hi: w is even or 1, and for w = 1 both read lo <= p < hi.
    int where = 2;
    if (a.hasBox) {
      for (int k = 0; k < 3; k++) {
        const long long c0 = (long long)lower[k] + (long long)((1ull << level) >> 1), c1 = c0 + (long long)((unsigned long long)(size[k] - 1) << level);
        if (c1 < (long long)a.box[k] || c0 >= (long long)a.box[3 + k]) where = 0;
        else if (where && !(c0 >= (long long)a.box[k] && c1 < (long long)a.box[3 + k])) where = 1;
      }
    }
    if (where == 0) continue;
    const float *cells = a.field + (uint64_t(uint32_t(b1.w)) + first);
    for (uint32_t i0 = 0; i0 < n; i0 += 256) {
      float v[4];
      uint32_t ok = 0;                                                 // bit k: load k holds a considered cell
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const uint32_t i = i0 + 64u * k + lane;
        v[k] = 0.f;
        if (i < n) { v[k] = cells[i]; ok |= 1u << k; }
      }
      if (where == 1) {
        // the cell's position from the segment's first one with 32-bit divisions; a centre beyond INT32_MAX is outside
        // every box (it cannot lie below INT32_MIN: lower does not, and idx*w >= 0)
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t xx = sg.x0 + (i0 + 64u * k + lane);           // < size.x + 2048
          const uint32_t qx = xx / size[0], yy = sg.y0 + qx;
          const uint32_t qy = yy / size[1];
          const uint32_t idx[3] = { xx - qx * size[0], yy - qy * size[1], sg.z0 + qy };
          bool inside = true;
          for (int ax = 0; ax < 3; ax++) {
            const long long c = (long long)lower[ax] + (long long)(((unsigned long long)idx[ax] << level) + ((1ull << level) >> 1));
            const int32_t c32 = int32_t(c);
            inside = inside && c == (long long)c32 && c32 >= a.box[ax] && c32 < a.box[3 + ax];
          }
          if (!inside) ok &= ~(1u << k);
        }
      }
      // one value after the other, not unrolled: unrolled, the compiler keeps the lane masks of all four classifications
      // (each a pair of scalar registers) alive at once and spills 33 scalar registers (measured on this file, ROCm 7.2)
#pragma unroll 1
      for (int k = 0; k < 4; k++) {
        const float x = k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
        const bool considered = (ok >> k) & 1u;
        const bool empty = considered && a.emptyCells && x == EXA_EMPTY_CELL_POISON_VALUE;
        const bool nan = considered && !empty && x != x;
        const bool value = considered && !empty && !nan;
        nEmpty += empty;
        nNan += nan;
        if (value) {
          const uint32_t key = orderedKey(x);
          keyMin = key < keyMin ? key : keyMin;
          keyMax = key > keyMax ? key : keyMax;
        }
        if (BINS) {
          const bool under = value && x < a.lo;
          const bool over = value && !under && x > a.hi;
          const bool binned = value && !under && !over;
          nUnder += under;
          nOver += over;
          nBinned += binned;
          const float t = binned ? (x - a.lo) * a.scale : 0.f;
          const int32_t bin = min(a.numBins - 1, int32_t(t));
          addBins(sBins, uint32_t(bin), binned, lane);
        } else {
          nBinned += value;
        }
      }
    }
  }
  for (int o = 32; o; o >>= 1) {
    const uint32_t kmin = uint32_t(__shfl_xor(int(keyMin), o)), kmax = uint32_t(__shfl_xor(int(keyMax), o));
    keyMin = kmin < keyMin ? kmin : keyMin;
    keyMax = kmax > keyMax ? kmax : keyMax;
    nEmpty += uint32_t(__shfl_xor(int(nEmpty), o));
    nNan += uint32_t(__shfl_xor(int(nNan), o));
    nUnder += uint32_t(__shfl_xor(int(nUnder), o));
    nOver += uint32_t(__shfl_xor(int(nOver), o));
    nBinned += uint32_t(__shfl_xor(int(nBinned), o));
  }
  if (lane == 0) {
    if (nEmpty) atomicAdd(&sStat[kHistStatEmpty], nEmpty);
    if (nNan) atomicAdd(&sStat[kHistStatNan], nNan);
    if (nUnder) atomicAdd(&sStat[kHistStatUnder], nUnder);
    if (nOver) atomicAdd(&sStat[kHistStatOver], nOver);
    if (nBinned) atomicAdd(&sStat[kHistStatBinned], nBinned);
    atomicMin(&sKey[0], keyMin);
    atomicMax(&sKey[1], keyMax);
  }
  __syncthreads();

  // the flush: the only accesses to the result.  The run's level from its first segment.
  const uint32_t level = uint32_t(a.bricks[2 * size_t(a.segs[s0].brick) + 1].z);
  unsigned long long *cellsOut = a.result, *volumeOut = a.result + a.numBins, *stat = a.result + 2 * size_t(a.numBins);
  if (BINS) {
    for (uint32_t i = tid; i < uint32_t(a.numBins); i += kHistBlock) {
      const unsigned long long c = sBins[i];
      if (c) {
        atomicAdd(&cellsOut[i], c);
        if (a.withVolume) atomicAdd(&volumeOut[i], c << ((3u * level) & 63u));   // the host refuses a sum beyond 64 bits
      }
    }
  }
  if (tid < kHistStatCount && sStat[tid]) atomicAdd(&stat[tid], (unsigned long long)sStat[tid]);
  if (tid == 64) {
    const unsigned long long nonEmpty = (unsigned long long)sStat[kHistStatNan] + sStat[kHistStatUnder] + sStat[kHistStatOver] + sStat[kHistStatBinned];
    if (nonEmpty) atomicAdd(&stat[kHistStatCount + level], nonEmpty);
  }
  if (tid == 128 && sKey[0] <= sKey[1]) {
    uint32_t *keys = reinterpret_cast<uint32_t *>(stat + kHistStatCount + kHistLevels);
    atomicMin(&keys[0], sKey[0]);
    atomicMax(&keys[1], sKey[1]);
  }
}

} // namespace

hipError_t launchHistogram(const HistArgs &a, hipStream_t s)
{
  if (a.numRuns == 0) return hipSuccess;
  if (a.numBins > 0) hipLaunchKernelGGL(histKernel<true>, dim3(a.numRuns), dim3(kHistBlock), 0, s, a);
  else hipLaunchKernelGGL(histKernel<false>, dim3(a.numRuns), dim3(kHistBlock), 0, s, a);
  return hipGetLastError();
}

} // namespace exa
