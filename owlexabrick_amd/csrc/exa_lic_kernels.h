// exa_lic_kernels.h — line integral convolution on a plane lattice (exa_hip_lic): per pixel the noise samples along the field
// line of the in-plane part of three channels, backward and forward from the pixel's centre, added up in registers.  Included
// by exa_kernels.hip behind exa_stream_kernels.h (the streamline units, -DEXA_TU_STREAM=1): the evaluation is streamEval, the
// step the streamlines' RK4 in the two lattice coordinates, the stage machine that of streamlinesKernel — one call site of the
// evaluation, so that the basis code exists once and the lanes of a wave evaluate side by side whatever stage each is in.
//
// Contract (include/exa_hip.h): a position c = (a, b) in pixel units lies at p(c) = (origin + a*du) + b*dv; E2(c) solves the
// plane's normal equations for the in-plane part (va, vb) of v = E(p(c)) and normalises it; nothing is contracted.  Nothing
// of size pixels x steps exists: a lane keeps c, the RK4 accumulator, the running sum and the count.

// N(ix, iy): the caller's noise, or the built-in hash (uint32 arithmetic)
__device__ __forceinline__ uint32_t licNoise(const LicArgs &a, uint32_t ix, uint32_t iy)
{
  if (a.noise) return a.noise[size_t(iy) * a.nu + ix];
  uint32_t h = ix * 0x9E3779B1u + iy * 0x85EBCA77u + a.seed * 0xC2B2AE3Du;
  h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
  return h >> 24;
}

// One wave per patch of 64 / lanesPerPixel pixels.  lanesPerPixel 1: the lane runs the backward direction, then starts again
// at the centre (whose direction it kept) and runs the forward one.  2: the even lane of a pair runs backward, the odd one
// forward, both evaluate the centre, and the odd lane adds the pair's integer sums and stores.  The lane carries which stage
// of the step its next evaluation is: 0 the candidate position (the centre, or a step's cn), 1..3 the stages k2..k4.
__global__ __launch_bounds__(256, 6) void streamlinesKernelLic(const LicArgs a)
{
  const unsigned long long wave = a.waveBase + (unsigned long long)blockIdx.x * 4u + (threadIdx.x >> 6);
  const uint32_t l = threadIdx.x & 63u;
  const bool two = a.lanesPerPixel == 2;
  const uint32_t pix = two ? l >> 1 : l;                                // the pixel within the patch
  int slot = two ? int(l & 1u) : 0;                                     // 0 backward, 1 forward
  const uint32_t px = uint32_t(wave % a.patchesX);
  const unsigned long long py = wave / a.patchesX;
  const uint32_t pw = 1u << a.patchShift, ph = (two ? 32u : 64u) >> a.patchShift;
  const unsigned long long ii = (unsigned long long)px * pw + (pix & (pw - 1u)), jj = py * ph + (pix >> a.patchShift);
  const bool valid = wave < a.numWaves && ii < a.nu && jj < a.nv;
  const uint32_t i = uint32_t(ii), j = uint32_t(jj);

  const V3 org = mk(a.origin), du = mk(a.du), dv = mk(a.dv);
  const float fnu = float(a.nu), fnv = float(a.nv);
  uint32_t sum = 0, count = 0, centre = 0;                              // the directions' samples; 1 once the centre has a direction
  int reasonB = EXA_STREAM_END_MAXSTEPS, reasonF = EXA_STREAM_END_MAXSTEPS;
  float speed = a.fill;
  bool tripped = false;
  if (valid) {
    const float c0a = float(i) + .5f, c0b = float(j) + .5f;
    float hs = slot ? a.step : -a.step;
    float ca = c0a, cb = c0b, qa = c0a, qb = c0b, acca = 0.f, accb = 0.f, d0a = 0.f, d0b = 0.f;
    int stage = 0;
    uint32_t taken = 0;                                                 // samples of the current direction
    bool haveCentre = false;
    V3 v = mk(0.f, 0.f, 0.f), vd = v;
    // at most four evaluations per step, one for the centre
    for (int e = 0, ne = (two ? 4 : 8) * a.halfLength + 1; e < ne; e++) {
      const V3 q = mk((org.x + qa * du.x) + qb * dv.x, (org.y + qa * du.y) + qb * dv.y, (org.z + qa * du.z) + qb * dv.z);
      int r = streamEval<false>(a, q, v, vd, tripped);
      float da = 0.f, db = 0.f;
      if (!r) {
        if (!haveCentre) speed = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
        const float r1 = (v.x * du.x + v.y * du.y) + v.z * du.z, r2 = (v.x * dv.x + v.y * dv.y) + v.z * dv.z;
        const float va = (a.g22 * r1 - a.g12 * r2) / a.det, vb = (a.g11 * r2 - a.g12 * r1) / a.det;
        const float s = sqrtf(va * va + vb * vb);
        if (!(s > 0.f) || !(s <= FLT_MAX)) r = EXA_STREAM_END_STAGNANT;
        else { da = va / s; db = vb / s; }
      }
      int end = 0;
      bool begin = false;                                               // start a step at c with the direction (da, db)
      if (r) {
        if (!haveCentre) {
          // the centre fails (nothing counted), or stagnates (the centre's own sample): both directions end with r
          centre = r == EXA_STREAM_END_STAGNANT ? 1u : 0u;
          reasonB = reasonF = r;
          break;
        }
        end = r;
      } else if (stage == 0) {
        if (haveCentre) {
          sum += licNoise(a, uint32_t(int(qa)), uint32_t(int(qb)));
          count++;
          taken++;
        } else {
          haveCentre = true;
          centre = 1u;
          d0a = da; d0b = db;
        }
        ca = qa; cb = qb;
        if (taken >= uint32_t(a.halfLength)) end = EXA_STREAM_END_MAXSTEPS;
        else begin = true;
      } else if (stage == 1) {
        const float k2a = hs * da, k2b = hs * db;
        acca = acca + 2.f * k2a; accb = accb + 2.f * k2b;
        qa = ca + .5f * k2a; qb = cb + .5f * k2b;
        stage = 2;
      } else if (stage == 2) {
        const float k3a = hs * da, k3b = hs * db;
        acca = acca + 2.f * k3a; accb = accb + 2.f * k3b;
        qa = ca + k3a; qb = cb + k3b;
        stage = 3;
      } else {
        const float k4a = hs * da, k4b = hs * db;
        acca = acca + k4a; accb = accb + k4b;                           // ((k1 + 2 k2) + 2 k3) + k4
        qa = ca + (1 / 6.f) * acca; qb = cb + (1 / 6.f) * accb;
        if (__float_as_int(qa) == __float_as_int(ca) && __float_as_int(qb) == __float_as_int(cb)) end = EXA_STREAM_END_STAGNANT;
        else if (!(qa >= 0.f && qa < fnu && qb >= 0.f && qb < fnv)) end = EXA_LIC_END_IMAGE;
        stage = 0;
      }
      if (end) {
        if (slot) reasonF = end; else reasonB = end;
        if (two || slot) break;
        // the forward direction, from the centre again
        slot = 1;
        hs = a.step;
        ca = c0a; cb = c0b;
        da = d0a; db = d0b;
        taken = 0;
        begin = true;
      }
      if (begin) {
        const float k1a = hs * da, k1b = hs * db;
        acca = k1a; accb = k1b;
        qa = ca + .5f * k1a; qb = cb + .5f * k1b;
        stage = 1;
      }
    }
  }
  if (tripped) atomicExch(a.s.errorFlag, 1);
  if (two) {
    // the pair's other direction: integer adds, exact in any order (an invalid pair exchanges zeros and stores nothing)
    sum += uint32_t(__shfl_xor(int(sum), 1));
    count += uint32_t(__shfl_xor(int(count), 1));
    const int other = __shfl_xor(reasonB, 1);
    if (slot) reasonB = other;
  }
  if (!valid || (two && !slot)) return;
  const size_t at = size_t(j) * a.nu + i;
  if (centre) {
    sum += licNoise(a, i, j);
    count += 1u;
  }
  if (a.sum) a.sum[at] = sum;
  if (a.count) a.count[at] = count;
  if (a.lic) a.lic[at] = count ? float(sum) / float(count) : a.fill;
  if (a.speed) a.speed[at] = speed;
  if (a.reasons) { a.reasons[2 * at] = reasonB; a.reasons[2 * at + 1] = reasonF; }
}

hipError_t launchLic(const LicArgs &a, hipStream_t s)
{
  if (a.waveBase >= a.numWaves) return hipSuccess;
  const unsigned long long waves = a.numWaves - a.waveBase < (1ull << 18) ? a.numWaves - a.waveBase : (1ull << 18);
  hipLaunchKernelGGL(streamlinesKernelLic, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, a);
  return hipGetLastError();
}
