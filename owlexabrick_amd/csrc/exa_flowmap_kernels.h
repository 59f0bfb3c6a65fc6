// exa_flowmap_kernels.h — the flow map of exa_hip_flowmap: per point of a lattice where the particle released there is after
// numSteps steps of the streamlines' RK4, how many steps it took and why it stopped.  Included by exa_kernels.hip behind
// exa_stream_kernels.h and exa_lic_kernels.h (the streamline units, -DEXA_TU_STREAM=1): the evaluation is streamEval<false>,
// the step and the stage machine are those of streamlinesKernel — one call site of the evaluation, so that the basis code
// exists once and the lanes of a wave evaluate side by side whatever stage each is in.
//
// Contract (include/exa_hip.h): point L's three outputs are those of the one-direction line of exa_hip_streamlines seeded at
// P(L).  Nothing of size points x numSteps exists: a lane keeps p, the RK4 accumulator, the step count and the reason, and
// stores 20 bytes once at the end.  The stretch is another unit's kernel (exa_isomesh.hip: it does not depend on the form).

// One wave per patch of 64 lattice points, 2^shift[a] of them along axis a (the shifts add up to 6); the lane carries which
// stage of the step its next evaluation is: 0 the candidate vertex q (the seed, or a step's pn), 1..3 the stages k2..k4.
__global__ __launch_bounds__(256) void streamlinesKernelFlowmap(const FlowmapArgs a)
{
  const unsigned long long wave = a.waveBase + (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  if (wave >= a.numWaves) return;
  const uint32_t l = threadIdx.x & 63u;
  const uint32_t pxy = a.patchesX * a.patchesY;
  const uint32_t pz = uint32_t(wave / pxy), rest = uint32_t(wave % pxy);
  const uint32_t py = rest / a.patchesX, px = rest % a.patchesX;
  const uint32_t sx = a.shift[0], sy = a.shift[1];
  const uint32_t i = (px << sx) + (l & ((1u << sx) - 1u));
  const uint32_t j = (py << sy) + ((l >> sx) & ((1u << sy) - 1u));
  const uint32_t k = (pz << a.shift[2]) + (l >> (sx + sy));
  if (i >= a.nx || j >= a.ny || k >= a.nz) return;
  const size_t at = (size_t(k) * a.ny + j) * a.nx + i;

  // P(L), the lattice point of exa_hip_resample
  V3 p = mk(a.lo[0] + (float(i) + .5f) * a.cell[0], a.lo[1] + (float(j) + .5f) * a.cell[1], a.lo[2] + (float(k) + .5f) * a.cell[2]);
  V3 q = p, acc = mk(0.f, 0.f, 0.f), v = mk(0.f, 0.f, 0.f), d = v;
  const float hs = a.hs;
  bool tripped = false, haveSeed = false;
  int stage = 0, reason = EXA_STREAM_END_MAXSTEPS;
  uint32_t taken = 0;              // steps taken = vertices after the seed
  // at most four evaluations per step and one for the seed (numSteps <= EXA_STREAM_MAX_STEPS = 2^20)
  for (int e = 0, ne = 4 * a.numSteps + 1; e < ne; e++) {
    const int r = streamEval<false>(a, q, v, d, tripped);
    if (r) { reason = r; break; }
    if (stage == 0) {
      // q holds a value in all three channels: the seed, or the vertex a step appends
      if (haveSeed) taken++; else haveSeed = true;
      p = q;
      if (taken >= uint32_t(a.numSteps)) break;                    // MAXSTEPS
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
  if (a.end) streamStore(a.end, at, p);
  if (a.steps) a.steps[at] = taken;
  if (a.reasons) a.reasons[at] = reason;
}

hipError_t launchFlowmap(const FlowmapArgs &a, hipStream_t s)
{
  if (a.waveBase >= a.numWaves) return hipSuccess;
  const unsigned long long waves = a.numWaves - a.waveBase < (1ull << 18) ? a.numWaves - a.waveBase : (1ull << 18);
  hipLaunchKernelGGL(streamlinesKernelFlowmap, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}
