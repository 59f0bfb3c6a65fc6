// exa_hostbvh.h — host-side tree building of the exa_hip_* module: Morton keys, the LBVH topology, the boxes of a
// host-built BVH (triangle mesh, streamline segments) and the level order of a bottom-up refit.  No HIP calls.
#pragma once
#include "exa_device.h"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <utility>

namespace exa {

inline uint64_t spread21(uint64_t v)
{
  v &= 0x1fffffull;
  v = (v | v << 32) & 0x1f00000000ffffull;
  v = (v | v << 16) & 0x1f0000ff0000ffull;
  v = (v | v << 8) & 0x100f00f00f00f00full;
  v = (v | v << 4) & 0x10c30c30c30c30c3ull;
  v = (v | v << 2) & 0x1249249249249249ull;
  return v;
}

// Morton key of the point c inside the box [lo, hi]: 21 bits per axis, x in the lowest bit
inline uint64_t mortonKey(const double c[3], const float lo[3], const float hi[3])
{
  uint64_t code = 0;
  for (int k = 0; k < 3; k++) {
    const double ext = double(hi[k]) - double(lo[k]);
    double u = ext > 0 ? (c[k] - double(lo[k])) / ext : 0.0;
    u = std::min(std::max(u, 0.0), 1.0);
    code |= spread21(std::min<uint64_t>(uint64_t(u * 2097152.0), 2097151ull)) << k;
  }
  return code;
}

// ---- LBVH topology: Morton-sorted regions, split at the highest differing bit;
// the depth is capped at kStackDepth so the per-lane LDS stack cannot overflow
// (median splits once the remaining depth budget is tight). ----
struct LbvhTopology {
  std::vector<int32_t> child0, child1;
  std::vector<int32_t> height;          // per internal node
  std::vector<uint64_t> codes;
  std::vector<uint32_t> order;

  static int ceilLog2(uint64_t n) { int l = 0; while ((1ull << l) < n) l++; return l; }

  int32_t buildRange(size_t lo, size_t hi, int depth, int32_t &outHeight)
  {
    if (hi - lo == 1) { outHeight = 0; return ~int32_t(order[lo]); }
    const int32_t me = (int32_t)child0.size();
    child0.push_back(0); child1.push_back(0); height.push_back(0);
    const size_t n = hi - lo;
    size_t split = lo + (n + 1) / 2;                           // median fallback
    const uint64_t first = codes[lo], last = codes[hi - 1];
    if (first != last) {
      const int prefix = __builtin_clzll(first ^ last);
      // Karras-style search: last index whose code shares more than `prefix` leading
      // bits with `first`; the right child starts right after it
      size_t at = lo, step = hi - 1 - lo;
      do {
        step = (step + 1) >> 1;
        const size_t cand = at + step;
        if (cand < hi - 1) {
          const uint64_t x = first ^ codes[cand];
          const int pfx = x ? __builtin_clzll(x) : 64;
          if (pfx > prefix) at = cand;
        }
      } while (step > 1);
      const size_t s = at + 1;
      const size_t big = std::max(s - lo, hi - s);
      if (ceilLog2(big) <= kStackDepth - 1 - depth) split = s;  // keep internal depth <= kStackDepth-1
    }
    int32_t h0, h1;
    const int32_t c0 = buildRange(lo, split, depth + 1, h0);
    const int32_t c1 = buildRange(split, hi, depth + 1, h1);
    child0[me] = c0; child1[me] = c1;
    height[me] = 1 + std::max(h0, h1);
    outHeight = height[me];
    return me;
  }

  // boxes: 6 floats (lo, hi) per primitive
  void build(const float *boxes, size_t n)
  {
    float lo[3] = { INFINITY, INFINITY, INFINITY }, hi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (size_t i = 0; i < n; i++)
      for (int k = 0; k < 3; k++) {
        lo[k] = std::fmin(lo[k], boxes[6 * i + k]);
        hi[k] = std::fmax(hi[k], boxes[6 * i + 3 + k]);
      }
    std::vector<std::pair<uint64_t, uint32_t>> keyed(n);
    for (size_t i = 0; i < n; i++) {
      double c[3];
      for (int k = 0; k < 3; k++) c[k] = 0.5 * (double(boxes[6 * i + k]) + double(boxes[6 * i + 3 + k]));
      keyed[i] = { mortonKey(c, lo, hi), uint32_t(i) };
    }
    std::sort(keyed.begin(), keyed.end());
    codes.resize(n); order.resize(n);
    for (size_t i = 0; i < n; i++) { codes[i] = keyed[i].first; order[i] = keyed[i].second; }
    child0.clear(); child1.clear(); height.clear();
    if (n == 0) return;
    if (n == 1) {                      // one region: a root with one real and one padding child
      child0.push_back(~int32_t(0)); child1.push_back(INT32_MIN); height.push_back(1);
      return;
    }
    child0.reserve(n); child1.reserve(n); height.reserve(n);
    int32_t h;
    buildRange(0, n, 0, h);
  }
};

// The nodes of a host-built BVH with their children's boxes filled in (children have larger indices than their parent:
// one backward sweep).  boxes: 6 floats per primitive, as given to LbvhTopology::build; leafOf(primitive) is the id a
// leaf reference carries on the device.
template <typename LeafOf>
std::vector<BvhNode> fillBoxes(const LbvhTopology &topo, const std::vector<float> &boxes, LeafOf leafOf)
{
  const size_t ni = topo.child0.size();
  std::vector<BvhNode> nodes(ni);
  std::vector<float> nlo(3 * ni), nhi(3 * ni);
  auto childBox = [&](int32_t c, float *lo, float *hi) {
    if (c == INT32_MIN) { for (int k = 0; k < 3; k++) { lo[k] = FLT_MAX; hi[k] = -FLT_MAX; } return; }
    if (c < 0) { for (int k = 0; k < 3; k++) { lo[k] = boxes[6 * size_t(~c) + k]; hi[k] = boxes[6 * size_t(~c) + 3 + k]; } return; }
    for (int k = 0; k < 3; k++) { lo[k] = nlo[3 * size_t(c) + k]; hi[k] = nhi[3 * size_t(c) + k]; }
  };
  auto ref = [&](int32_t c) { return (c < 0 && c != INT32_MIN) ? ~int32_t(leafOf(size_t(~c))) : c; };
  for (size_t i = ni; i-- > 0;) {
    float l0[3], h0[3], l1[3], h1[3];
    childBox(topo.child0[i], l0, h0);
    childBox(topo.child1[i], l1, h1);
    for (int k = 0; k < 3; k++) { nlo[3 * i + k] = std::fmin(l0[k], l1[k]); nhi[3 * i + k] = std::fmax(h0[k], h1[k]); }
    BvhNode &n = nodes[i];
    n.q0 = make_float4(l0[0], l0[1], l0[2], h0[0]);
    n.q1 = make_float4(h0[1], h0[2], l1[0], l1[1]);
    n.q2 = make_float4(l1[2], h1[0], h1[1], h1[2]);
    n.child0 = ref(topo.child0[i]); n.child1 = ref(topo.child1[i]); n.pad0 = n.pad1 = 0;
  }
  return nodes;
}

// Node ids ordered by height (>= 1 for every node) for a refit level by level, children before parents: the nodes of
// height h are ids[levelBegin[h - 1] .. levelBegin[h])
inline void orderByHeight(const std::vector<int32_t> &heights, std::vector<int32_t> &ids, std::vector<int> &levelBegin)
{
  int maxH = 0;
  for (int32_t h : heights) maxH = std::max(maxH, h);
  std::vector<int> count(maxH + 2, 0);
  for (int32_t h : heights) count[h]++;
  levelBegin.assign(1, 0);
  for (int h = 1; h <= maxH; h++) levelBegin.push_back(levelBegin.back() + count[h]);
  ids.resize(heights.size());
  std::vector<int> cursor(levelBegin);
  for (size_t i = 0; i < heights.size(); i++) ids[cursor[heights[i] - 1]++] = (int32_t)i;
}

} // namespace exa
