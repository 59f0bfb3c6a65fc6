// exa_isomesh.h — iso-surface extraction on a lattice of sampled values (exa_hip_isosurface), and contour lines on a plane
// lattice (exa_hip_isolines, further down): what exa_probe.cpp and exa_isomesh.hip share.  Marching tetrahedra on the six-tetrahedra (Kuhn) split of every lattice cube along the diagonal
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

// ---- contour lines on a plane lattice (exa_hip_isolines): the 2D sibling, marching triangles on the split of every lattice
// square along the diagonal (0,0)-(1,1).  One lane per lattice point L = j*nu + i, blocks of kIsoBlock consecutive L, one
// level (iso) per round of passes over the shared values:
//   positions     P(L) = (origin + (float(i) + 0.5f) * du) + (float(j) + 0.5f) * dv into a device buffer; the probes' kernels
//                 fill the values from it
//   square pass   squareInfo[L] = 0x80 | number of segments of the square with origin L (0 = not a square, or a corner value
//                 is not finite), and the block's segment count
//   point pass    mask[L] = bit (code-1) for every crossing triangle edge L -> L + (dx,dy), code = dx + 2 dy, that lies in a
//                 valid square; rel[L] and the block's count as above
//   scans         the iso-surface's (launchIsolineScans hands them the counts)
//   emit          vertices and uv at vertexBase + chunkBase + blockBase + rel + popcount(mask below the edge's bit); segment
//                 indices through the owning point's base and mask.  vertices, uv and segments point at the level's first
//                 entry, vertexBase is the global index of its first vertex
struct IsoLineArgs {
  const float *values;        // the lattice, numPoints floats
  uint32_t numPoints;         // nu*nv <= 2^31 - 1
  uint32_t nu, nv;
  float iso;
  float origin[3], du[3], dv[3];
  float *positions;           // the positions kernel: 3 floats per lattice point
  uint8_t *squareInfo;        // numPoints
  uint8_t *mask;              // numPoints
  uint16_t *rel;              // numPoints
  uint32_t numBlocks, numChunks;
  uint32_t *blockCount;       // [2][numBlocks]: 0 = vertices, 1 = segments
  uint32_t *blockBase;        // [2][numBlocks]
  uint64_t *chunkBase;        // [2][numChunks]
  uint64_t *totals;           // [2]
  uint32_t vertexBase;
  float *vertices;            // 3 floats per vertex
  float *uv;                  // 2 floats per vertex
  int32_t *segments;          // 2 indices per segment
};

hipError_t launchIsolinePositions(const IsoLineArgs &a, hipStream_t s);
hipError_t launchIsolineSquarePass(const IsoLineArgs &a, hipStream_t s);
hipError_t launchIsolinePointPass(const IsoLineArgs &a, hipStream_t s);
hipError_t launchIsolineScans(const IsoLineArgs &a, hipStream_t s);
hipError_t launchIsolineEmit(const IsoLineArgs &a, hipStream_t s);

} // namespace exa
