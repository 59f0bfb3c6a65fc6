// exa_isomesh.h — iso-surface extraction on a lattice of sampled values (exa_hip_isosurface): what exa_probe.cpp and
// exa_isomesh.hip share.  Marching tetrahedra on the six-tetrahedra (Kuhn) split of every lattice cube along the diagonal
// (0,0,0)-(1,1,1); include/exa_hip.h states the contract (tetrahedron order, vertex order, orientation).
//
// The pipeline, every kernel one lane per lattice point L = (k*ny + j)*nx + i, blocks of kIsoBlock consecutive L (a wave
// reads 64 consecutive x of a row: the values are x fastest):
//   cube pass     cubeInfo[L] = 0x80 | number of triangles of the cube with origin L (0 = not a cube, or a corner value
//                 is not finite), and the block's triangle count
//   point pass    mask[L] = bit (code-1) for every crossing tet edge L -> L + (dx,dy,dz), code = dx + 2 dy + 4 dz, that lies
//                 in a valid cube; rel[L] = the number of vertices of the block's points in front of L; the block's count
//   scans         the block counts of both passes: exclusive within chunks of kIsoChunk blocks (blockBase, 32 bit), then
//                 over the chunk sums (chunkBase, 64 bit) — placement by prefix sums only, no atomics, so the order of the
//                 output is the order of L
//   emit          vertices at chunkBase + blockBase + rel + popcount(mask below the edge's bit); triangle indices through
//                 the owning point's base and mask
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace exa {

static const uint32_t kIsoBlock = 256;      // lattice points per block
static const uint32_t kIsoChunk = 2048;     // block counts per scan chunk (2^31 points -> 2^23 blocks -> 4096 chunks)

struct IsoMeshArgs {
  const float *values;        // the lattice, numPoints floats
  uint32_t numPoints;         // nx*ny*nz <= 2^31 - 1
  uint32_t nx, ny, nz;
  float iso;
  float lo[3], step[3];       // lattice point i on axis a: lo[a] + (float(i) + 0.5f) * step[a]
  uint8_t *cubeInfo;          // numPoints
  uint8_t *mask;              // numPoints
  uint16_t *rel;              // numPoints
  uint32_t numBlocks, numChunks;
  uint32_t *blockCount;       // [2][numBlocks]: 0 = vertices, 1 = triangles
  uint32_t *blockBase;        // [2][numBlocks]
  uint64_t *chunkBase;        // [2][numChunks]
  uint64_t *totals;           // [2]
  float *vertices;            // 3 floats per vertex
  int32_t *triangles;         // 3 indices per triangle
};

hipError_t launchIsoCubePass(const IsoMeshArgs &a, hipStream_t s);
hipError_t launchIsoPointPass(const IsoMeshArgs &a, hipStream_t s);
hipError_t launchIsoScans(const IsoMeshArgs &a, hipStream_t s);
hipError_t launchIsoEmit(const IsoMeshArgs &a, hipStream_t s);

} // namespace exa
