// exa_sample_locate.h — the activity-free region lookup of the point probes and of the streamline integrator: the pieces of
// the descent of the region kd-tree (contract: include/exa_hip.h, the probes' block).  Included inside namespace
// exa::EXA_FORM_NS by exa_sample_kernels.h and exa_stream_kernels.h, so that both locate a position with the same code.

// p inside the closed root box; false for a NaN coordinate
__device__ __forceinline__ bool sampleInRoot(const SampleArgs &a, V3 p)
{
  return p.x >= a.kdLo[0] && p.x <= a.kdHi[0] && p.y >= a.kdLo[1] && p.y <= a.kdHi[1] && p.z >= a.kdLo[2] && p.z <= a.kdHi[2];
}

// the child of a node on p's side of its plane (only split, axis and children: the activity bits are masked)
__device__ __forceinline__ int sampleKdChild(const KdNodeDev n, V3 p)
{
  const uint32_t axis = n.word & 3u;
  const float c = axis == 0u ? p.x : (axis == 1u ? p.y : p.z);
  return c >= n.split ? n.right : n.left;
}

// from subtree `ref` down to a leaf: the region id, or -1 (an empty child slot, or the bound tripped)
__device__ __forceinline__ int sampleKdLeaf(const SampleArgs &a, int ref, V3 p, bool &tripped)
{
  for (int g = 0; ref >= 0; g++) {
    if (g >= a.maxSteps) { tripped = true; return -1; }
    ref = sampleKdChild(a.kdNodes[ref], p);
  }
  return ref == EXA_KD_EMPTY ? -1 : ~ref;
}

// the same for a wave whose positions lie close together (called by every lane that is inside the root box).  UNIFORM: the
// wave descends from the root together while all these lanes take the same side of every plane, then each lane on its own
// from where they part
template <bool UNIFORM>
__device__ __forceinline__ int sampleKdLeafWave(const SampleArgs &a, V3 p, bool &tripped)
{
  int ref = a.kdRoot;
  if (UNIFORM) {
    for (int g = 0; ref >= 0 && g < a.maxSteps; g++) {
      const int u = __builtin_amdgcn_readfirstlane(ref);           // the same in every lane here
      const int next = sampleKdChild(a.kdNodes[u], p);
      if (anyLane(next != __builtin_amdgcn_readfirstlane(next))) break;   // the lanes part at this node
      ref = next;
    }
  }
  return sampleKdLeaf(a, ref, p, tripped);
}

__device__ __forceinline__ bool sampleInDomain(const RegionRec &R, V3 p)
{
  return p.x >= R.lo[0] && p.x <= R.hi0 && p.y >= R.lo[1] && p.y <= R.hi1 && p.z >= R.lo[2] && p.z <= R.hi2;
}
