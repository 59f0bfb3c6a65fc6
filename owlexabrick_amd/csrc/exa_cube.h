// Cube records: the 16-byte brick records of the one-channel rope march for scenes whose bricks are all cubes of one
// power-of-two edge S = 2^k (block-structured AMR with a fixed block size: every BASELINE configuration).  The three
// sizes then are one wave-uniform kernel argument instead of per-lane data, `begin` is a multiple of S^3, and what is
// left of a brick fits one int4 beside the 32-byte march header (exa_create.cpp: buildMarchHeaders), not instead of it:
//   x, y, z = float(lower.xyz) as float bits, the floats of the march header
//   w       = ((begin >> 3k) << 9) | (127 - level): bits 0..7 are the exponent of 2^-level and bit 8 is 0, so
//             w << 23 IS the float 2^-level (the march header's invCw, bit for bit); begin = (w >> 9) << 3k.
// Host only: shared by renderer creation (exa_create.cpp) and the diagnostic entry point exa_prep_cube_records
// (exa_prep.cpp; tests/test_cube_records.py).
#pragma once
#include "../../include/exa_hip.h"

#include <cstdint>
#include <cstring>

namespace exa {

enum { kCubeMinLog2 = 1, kCubeMaxLog2 = 7, kCubeIndexBits = 23, kCubeMaxLevel = 30 };

inline uint32_t cubeRecordWord(uint32_t begin, int k, int level) { return ((begin >> (3 * k)) << 9) | uint32_t(127 - level); }
inline uint32_t cubeRecordBegin(uint32_t w, int k) { return (w >> 9) << (3 * k); }
inline int cubeRecordLevel(uint32_t w) { return 127 - int(w & 0x1ffu); }

// k of the scene's cube edge 2^k, or 0 when the scene is not a cube scene: a brick that is no cube of the first brick's
// edge, an edge that is no power of two in 2..128, a `begin` (in either order of the bricks: beginAlt may be NULL) that
// is no multiple of S^3 or whose index begin / S^3 does not fit 23 bits, a level outside 0..30.
inline int cubeSceneLog2(const ExaBrick *bricks, uint64_t numBricks, const uint32_t *beginAlt)
{
  if (!bricks || numBricks == 0) return 0;
  const int32_t S = bricks[0].size[0];
  int k = 0;
  while (k <= kCubeMaxLog2 && (int32_t(1) << k) != S) k++;
  if (k < kCubeMinLog2 || k > kCubeMaxLog2) return 0;
  const uint32_t volMask = (1u << (3 * k)) - 1u;
  auto beginOk = [&](uint32_t begin) { return (begin & volMask) == 0 && (begin >> (3 * k)) < (1u << kCubeIndexBits); };
  for (uint64_t b = 0; b < numBricks; b++) {
    const ExaBrick &B = bricks[b];
    if (B.size[0] != S || B.size[1] != S || B.size[2] != S || B.level < 0 || B.level > kCubeMaxLevel) return 0;
    if (!beginOk(uint32_t(B.begin)) || (beginAlt && !beginOk(beginAlt[b]))) return 0;
  }
  return k;
}

// one record (four 32-bit words) per leaf-list entry, for a scene whose cubeSceneLog2 is k > 0
inline void buildCubeRecords(const ExaBrick *bricks, const int32_t *leafList, uint64_t leafListSize, int k, int32_t *out)
{
  for (uint64_t i = 0; i < leafListSize; i++) {
    const ExaBrick &B = bricks[leafList[i]];
    const float lowerF[3] = { float(B.lower[0]), float(B.lower[1]), float(B.lower[2]) };
    std::memcpy(out + 4 * i, lowerF, sizeof(lowerF));
    out[4 * i + 3] = int32_t(cubeRecordWord(uint32_t(B.begin), k, B.level));
  }
}

} // namespace exa
