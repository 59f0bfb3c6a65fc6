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

#include "../../include/exa_hip.h"

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
hipError_t launchIsoEmit(const IsoMeshArgs &a, hipStream_t s);

// the scans of every extraction here: `counts` (1 or 2) arrays of block counts, one behind the other in each of the four
// buffers.  blockBase = the exclusive sums within the chunks, chunkBase = those over the chunk sums, totals = the sums.
struct IsoScanArgs {
  uint32_t numBlocks, numChunks;
  uint32_t *blockCount;       // [counts][numBlocks]
  uint32_t *blockBase;        // [counts][numBlocks]
  uint64_t *chunkBase;        // [counts][numChunks]
  uint64_t *totals;           // [counts]
};

hipError_t launchIsoScans(const IsoScanArgs &a, int counts, hipStream_t s);

// ---- contour lines on a plane lattice (exa_hip_isolines): the 2D sibling, marching triangles on the split of every lattice
// square along the diagonal (0,0)-(1,1).  One lane per lattice point L = j*nu + i, blocks of kIsoBlock consecutive L, one
// level (iso) per round of passes over the shared values:
//   positions     P(L) = (origin + (float(i) + 0.5f) * du) + (float(j) + 0.5f) * dv into a device buffer; the probes' kernels
//                 fill the values from it
//   square pass   squareInfo[L] = 0x80 | number of segments of the square with origin L (0 = not a square, or a corner value
//                 is not finite), and the block's segment count
//   point pass    mask[L] = bit (code-1) for every crossing triangle edge L -> L + (dx,dy), code = dx + 2 dy, that lies in a
//                 valid square; rel[L] and the block's count as above
//   scans         the iso-surface's
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
hipError_t launchIsolineEmit(const IsoLineArgs &a, hipStream_t s);

// ---- connected regions of the set inside(V) on the lattice (exa_hip_regions): a lock-free union-find over the lattice
// points, one lane per point L = (k*ny + j)*nx + i, blocks of kIsoBlock consecutive L.  `parent` is the labels array of the
// result: the forest while the call runs, the region numbers when it returns.
//   init       parent[L] = L if inside, else kIsoRegionOutside; the number of inside points and the largest |V| among them
//              (as float bits) into totals[1] and totals[2], one pair of atomics per block of kIsoRegionTiles tiles
//   merge      for every inside L and every forward edge L -> L + d whose other end is inside: find both roots; while they
//              differ, atomicMin the larger root's parent to the smaller.  A return value that is not the larger root says
//              that it was no root any more: its link was `old`, which the atomicMin kept (old <= smaller) or replaced — in
//              both cases `old` and the smaller root are what is left to unite.  Links only ever go from a larger to a
//              smaller index, so every walk descends strictly and the root of a finished tree is its smallest L, `first`.
//              No lane waits for another: a lost race is a retry with what the atomic returned.  The loads of the walks are
//              agent-scope atomic loads (they bypass the L1, which other CUs' atomics never refresh); a stale value would
//              only be an older ancestor.
//   flatten    parent[L] = find(L); the block's number of roots (parent[L] == L) into blockCount
//   scans      the iso-surface's, over that one count; totals[0] = number of regions
//   rank       a root's number = chunkBase + blockBase + its rank among the block's roots; it goes into the root's own slot
//              as kIsoRegionRanked | number (L < 2^31 leaves the bit free) and starts the region's record
//   stats      label = the number in the own slot (a root) or in the slot parent[L] names (masking the bit reads a root's
//              slot rightly before and after that root's lane has stored its label), stored in place; the region's
//              measurements, gathered by a lane over its kIsoRegionTiles tiles as long as the label stays, then reduced over
//              the lanes of the wave that share the leading lane's label (twice: a wave mostly holds one or two labels)
//              before one lane issues the atomics, what is left lane by lane: all waves of one large region add to one
//              record, and atomics to one address go one after the other
//   finish     min, max, argMin, argMax of every region out of its two 64-bit keys
// Every walk is bounded by numPoints steps (it descends strictly, so it cannot take more) and refuses a link that ascends:
// a bound that trips sets errorFlag, the module's loop guard.
static const uint32_t kIsoRegionOutside = 0xffffffffu, kIsoRegionRanked = 0x80000000u;
static const uint32_t kIsoRegionTiles = 16;     // blocks of the lattice per block of the init and the stats pass

struct IsoRegionArgs {
  const float *values;        // the lattice, numPoints floats
  uint32_t numPoints;         // nx*ny*nz <= 2^31 - 1
  uint32_t nx, ny, nz;
  float iso;
  int32_t below, faces;       // EXA_REGIONS_BELOW, EXA_REGIONS_FACES
  uint32_t *parent;           // numPoints: the forest, then the labels
  uint32_t numBlocks, numChunks;
  uint32_t *blockCount;       // [numBlocks] roots
  uint32_t *blockBase;        // [numBlocks]
  uint64_t *chunkBase;        // [numChunks]
  uint64_t *totals;           // [3]: regions (the scans), inside points, bits of max |V| (init; zeroed by the host)
  int32_t *errorFlag;         // the module's loop guard
  double scale;               // 2^sumExponent
  uint32_t numRegions;
  ExaHipRegion *regions;      // numRegions
  uint64_t *keys;             // [numRegions][2]: (value key << 32) | L, by atomic min; (value key << 32) | ~L, by atomic max
};

hipError_t launchIsoRegionInit(const IsoRegionArgs &a, hipStream_t s);
hipError_t launchIsoRegionMerge(const IsoRegionArgs &a, hipStream_t s);
hipError_t launchIsoRegionFlatten(const IsoRegionArgs &a, hipStream_t s);
hipError_t launchIsoRegionRank(const IsoRegionArgs &a, hipStream_t s);
hipError_t launchIsoRegionStats(const IsoRegionArgs &a, hipStream_t s);

// ---- basins of the inside set on the lattice (exa_hip_basins): one basin per peak, shallow ones merged in rounds.  `comp` is
// the labels array of the result and holds, one after the other: the up link of every point (an index L), its peak (the up
// links resolved), its raw basin (the peak's number among the peaks, ascending L), its component (the raw number of the
// component's peak, round by round) and at last the basin's number.  Outside points hold kIsoRegionOutside throughout.
//   init       isoRegionInitKernel as it is: comp[L] = L or the outside mark, the inside count and max |V|
//   up         one lane per point, the 14 or 6 neighbours by plain loads: comp[L] = the greatest of L and its inside neighbours
//   jump       pointer doubling in place, for the points' links and later for the components': a lane follows kIsoBasinHops
//              links from where its own points and stores where it got; a lane that did not reach a fixed point counts into
//              *jumpCount, which the host reads to end the loop.  Every slot only ever moves along its own chain, so a
//              racing read sees an ancestor, older or newer.  A chain shrinks to a fifth per pass.
//   count      the block's number of fixed points (slot i holds i) into blockCount; the scans are the iso-surface's
//   rank       a peak's raw number goes into its own slot as kIsoRegionRanked | number; peakOf[number] = L, link[number] = number
//   label      comp[L] = the raw number, through the peak's slot (the mask reads it before and after the peak's own lane)
//   pass       one lane per inside point: over its edges into other components the greatest word
//              min(h, h') << 32 | ~component, which orders as the contract's word does since raw numbers ascend with the
//              peak's L; reduced over the lanes of the wave that share the leading lane's component (twice), then one
//              64-bit atomicMax on pass[component] — skipped where a plain load already shows as much
//   link       one lane per raw number that still is a component: saddle and depth from its word; it links to the neighbour
//              if depth < minDepth and the neighbour's peak is greater, and counts the link into *jumpCount
//   merge      comp[L] = link[comp[L]], the links resolved by the jump passes before
//   final      a component's number among the components (count and scans over the raw numbers) into finalOf; its record
//              started, with the raw number parked in `neighbour` for the finish
//   stats      isoRegionStatsKernel's scheme on the 96-byte record
//   first      one lane per point over the final labels: `first` by an atomic min from the lanes that begin a run of a label
//              within their wave, skipped where a load already shows a smaller one
//   finish     min / max / argMin / argMax out of the keys; neighbour, saddle and depth out of the last round's word
static const uint32_t kIsoBasinHops = 4;

struct IsoBasinArgs {
  const float *values;        // the lattice, numPoints floats
  uint32_t numPoints;         // nx*ny*nz <= 2^31 - 1
  uint32_t nx, ny, nz;
  float iso;
  int32_t below, faces;       // EXA_REGIONS_BELOW, EXA_REGIONS_FACES
  uint32_t *comp;             // numPoints, see above
  uint32_t numBlocks, numChunks;   // of the lattice; the count pass and the scans also run over the raw numbers, which are fewer
  uint32_t *blockCount;       // [numBlocks]
  uint32_t *blockBase;        // [numBlocks]
  uint64_t *chunkBase;        // [numChunks]
  uint64_t *totals;           // [3]: the scans' total, inside points, bits of max |V| (init; zeroed by the host)
  int32_t *errorFlag;         // the module's loop guard
  double scale;               // 2^sumExponent
  float minDepth;
  uint32_t *jumpArray;        // jump and count: comp (jumpSize = numPoints) or link (numRaw)
  uint32_t jumpSize;
  uint32_t *jumpCount;        // jump: lanes not yet at a fixed point; link: links made
  uint32_t numRaw;
  uint32_t *peakOf;           // [numRaw] L of the raw basin's peak
  uint32_t *link;             // [numRaw] the component a raw basin belongs to (itself: it is one)
  uint32_t *finalOf;          // [numRaw] a component's number in the table
  uint64_t *pass;             // [numRaw] the round's word, zeroed by the host before the pass kernel
  uint32_t numBasins;
  ExaHipBasin *basins;        // numBasins
  uint64_t *keys;             // [numBasins][2], as for the regions
};

hipError_t launchIsoBasinInit(const IsoBasinArgs &a, hipStream_t s);
hipError_t launchIsoBasinUp(const IsoBasinArgs &a, hipStream_t s);
hipError_t launchIsoBasinJump(const IsoBasinArgs &a, uint32_t *array, uint32_t size, hipStream_t s);
hipError_t launchIsoBasinCount(const IsoBasinArgs &a, uint32_t *array, uint32_t size, hipStream_t s);
hipError_t launchIsoBasinRank(const IsoBasinArgs &a, hipStream_t s);                                     // rank and label
hipError_t launchIsoBasinPass(const IsoBasinArgs &a, hipStream_t s);
hipError_t launchIsoBasinLink(const IsoBasinArgs &a, hipStream_t s);
hipError_t launchIsoBasinMerge(const IsoBasinArgs &a, hipStream_t s);
hipError_t launchIsoBasinFinal(const IsoBasinArgs &a, hipStream_t s);
hipError_t launchIsoBasinStats(const IsoBasinArgs &a, hipStream_t s);                                    // stats, first and finish

// ---- the stretch of a flow map (exa_hip_flowmap): one lane per lattice point L = (k*ny + j)*nx + i reads the map's end
// points and reasons at its stencil (per axis the neighbours at max(i-1, 0) and min(i+1, n-1)), forms the deformation
// gradient, the Cauchy-Green tensor and its largest eigenvalue by five sweeps of cyclic Jacobi, as the contract words them.
struct IsoStretchArgs {
  const float *end;           // the flow map: 3 floats per lattice point
  const int32_t *reasons;     // EXA_STREAM_END_* per lattice point
  uint32_t numPoints;         // nx*ny*nz <= 2^31 - 1
  uint32_t nx, ny, nz;
  float lo[3], cell[3];       // lattice point i on axis a: lo[a] + (float(i) + 0.5f) * cell[a]
  float fill;
  float *stretch;             // numPoints
};

hipError_t launchIsoLatticeStretch(const IsoStretchArgs &a, hipStream_t s);

// ---- critical points of a vector field on a lattice (exa_hip_critical_points): the zeros of the trilinear interpolant of
// three lattices, cell by cell.  `values` holds the three lattices one behind the other (component c at values + c*numPoints).
//   cells      one lane per L, blocks of kIsoBlock consecutive L, a block of the launch taking kIsoCriticalTiles of them one
//              after the other: the 8 x 3 corner loads, validity and the candidate test; the wave's ballot of candidates into
//              marks (one 64-bit word per wave: a bit per lattice point), the block's count into blockCount; what the lanes
//              have counted of cells and invalid cells over their tiles goes to the counters once per block of the launch
//   scans      the iso-surface's over blockCount, then the compaction: candidate number
//              chunkBase + blockBase + the marks below the lane's bit -> candidates[], ascending L
//   refine     one lane per candidate, dense waves, the iteration count wave-uniform: s, lastStep and the class
//              (kIsoCriticalFound or the reject's counter) into state / result, the block's found count into candCount, the
//              rejects to the counters by one integer atomic per wave and class
//   scans      the same over candCount
//   emit       one record per found candidate at candChunkBase + candBase + its rank in the block; J once more at s, the
//              classification in double; the position also into `positions` where the probe follows
//   pack       the probe's values and gradients interleaved into the n x 3 x 4 array of the contract
static const uint32_t kIsoCriticalTiles = 8;    // blocks of the lattice per block of the cell pass
static const int32_t kIsoCriticalFound = 0;     // result[]: found, else the index of the reject's counter in ExaHipCriticalStats
static const int32_t kIsoCriticalNonFinite = 4, kIsoCriticalLeftCell = 5, kIsoCriticalNotConverged = 6;

struct IsoCriticalArgs {
  const float *values;        // 3 * numPoints floats
  uint32_t numPoints;         // nx*ny*nz <= 2^31 - 1
  uint32_t nx, ny, nz;
  float lo[3], step[3];       // lattice point i on axis a: lo[a] + (float(i) + 0.5f) * step[a]
  int32_t iterations;
  float tolerance;
  unsigned long long *marks;  // [numBlocks][kIsoBlock / 64], read and written word by word: behind the counters, 8-byte aligned
  uint32_t numBlocks, numChunks;
  uint32_t *blockCount;       // [numBlocks] candidates
  uint32_t *blockBase;        // [numBlocks]
  uint64_t *chunkBase;        // [numChunks]
  uint64_t *totals;           // [2]: candidates, found (the two rounds of scans)
  unsigned long long *counters;   // an ExaHipCriticalStats, zeroed by the host: the kernels add to cells, invalidCells and the rejects
  uint32_t numCandidates;
  uint32_t *candidates;       // [numCandidates] cell numbers, ascending
  float *state;               // [numCandidates][4]: s, lastStep
  int32_t *result;            // [numCandidates]
  uint32_t numCandBlocks, numCandChunks;
  uint32_t *candCount;        // [numCandBlocks] found
  uint32_t *candBase;         // [numCandBlocks]
  uint64_t *candChunkBase;    // [numCandChunks]
  uint32_t numFound;
  ExaHipCriticalPoint *points;    // [numFound]
  float *positions;           // [numFound][3], or nullptr
  const float *probeValues;   // pack: [numFound][3], [numFound][3][3] -> probe [numFound][3][4]
  const float *probeGradients;
  float *probe;
};

hipError_t launchIsoCriticalCells(const IsoCriticalArgs &a, hipStream_t s);
hipError_t launchIsoCriticalCompact(const IsoCriticalArgs &a, hipStream_t s);
hipError_t launchIsoCriticalRefine(const IsoCriticalArgs &a, hipStream_t s);
hipError_t launchIsoCriticalEmit(const IsoCriticalArgs &a, hipStream_t s);
hipError_t launchIsoCriticalPack(const IsoCriticalArgs &a, hipStream_t s);

// ---- profiles and phase plots on the lattice (exa_hip_profile): the lattice points binned by one or two keys, other
// quantities accumulated per bin.  One lane per lattice point L = (k*ny + j)*nx + i, blocks of kIsoBlock consecutive L, a
// block of the launch taking kIsoProfileTiles of them one after the other.  A source is a lattice in memory (a channel or a
// derived quantity, resampled by the host), or the radius about a centre or a coordinate, formed from (i, j, k).
//   classify    the keys (or the label) and the bin of every point into bins[L], kIsoProfileUnbinned for the classes that are
//               not binned; the class counts and, over the binned points, the largest |term| of every series (as float bits),
//               gathered by a lane over its tiles and added once per block of the launch; the smallest L whose label is not
//               below numBins by an atomic min
//   accumulate  per binned point the terms quantised with the series' scales; count, sums and min / max keys to the bin's
//               record.  The lanes of a wave that share the leading pending lane's bin are reduced before that lane issues the
//               atomics, twice (a radial profile, one giant region or a constant key put whole waves into one bin), what is
//               left goes lane by lane.  The table is columns of B entries: the sums (64 bit; the weight's where there is a
//               weight, then one per value), the counts, the min keys and the max keys (32 bit, one column per value).  Small
//               table: a copy per workgroup in LDS (the counts 32 bit there), its records with a count flushed once by
//               64-bit atomics.  Large table: the atomics go to HBM directly.
//   finish      the keys of the table to floats in place
// The LDS copy holds kIsoProfileLdsBinBytes(numValues) per bin, laid out as if there were a weight and min / max, so that the
// choice hangs on B and numValues alone; it is taken when that fits EXA_PROFILE_LDS_BYTES (dynamic shared memory; at most
// 64 KiB, and 160 KiB per CU are shared by the workgroups in flight).
#ifndef EXA_PROFILE_LDS_BYTES
#define EXA_PROFILE_LDS_BYTES 32768
#endif
static const uint32_t kIsoProfileTiles = 16;              // blocks of the lattice per block of the classify and accumulate passes
static const uint32_t kIsoProfileUnbinned = 0xffffffffu;  // bins[L] of a point that is outside, invalid, under or over
static const int32_t kIsoProfileSeries = 1 + EXA_PROFILE_MAX_VALUES;      // the weight's series, then the values'
static const int32_t kIsoProfileUniform = 0, kIsoProfileEdges = 1, kIsoProfileLabels = 2;     // IsoProfileKey::mode
// the counters of the classify pass, 64-bit words zeroed by the host except the last, which starts at ~0
static const int kIsoProfileOutside = 0, kIsoProfileInvalid = 1, kIsoProfileUnder = 2, kIsoProfileOver = 4, kIsoProfileBinned = 6,
                 kIsoProfileBadLabel = 7, kIsoProfileCounters = 8;

constexpr size_t kIsoProfileLdsBinBytes(int32_t numValues) { return 8 * size_t(1 + numValues) + 4 + 8 * size_t(numValues); }
constexpr bool isoProfileLdsTable(uint64_t numBins, int32_t numValues) { return numBins * kIsoProfileLdsBinBytes(numValues) <= size_t(EXA_PROFILE_LDS_BYTES); }

// What the kernels hold of the call they keep in scalar registers for the whole pass: a source is 16 bytes, its kind a
// nibble of `kinds`, and the flags share a word (the first form of the arguments, one struct per source with its kind and
// every field, spilled 34 scalar registers in the classify and the accumulate pass).
union IsoProfileSource {
  const float *values;        // kIsoProfileMemory: numPoints floats
  int32_t axis;               // EXA_SOURCE_COORDINATE
  float centre[3];            // EXA_SOURCE_RADIUS
};
static const int kIsoProfileWeightSlot = 2, kIsoProfileValueSlot = 3, kIsoProfileSlots = 3 + EXA_PROFILE_MAX_VALUES;    // slots 0, 1: the axes' keys
static const int32_t kIsoProfileMemoryKind = 0;           // a nibble of `kinds`; else EXA_SOURCE_RADIUS / EXA_SOURCE_COORDINATE

struct IsoProfileKey {
  int32_t mode, numBins;
  float lo, hi, scale;        // uniform: scale = float(numBins) / (hi - lo); edges: lo, hi = the first and the last edge
  const float *edges;         // edges: numBins + 1 floats in device memory
};

struct IsoProfileArgs {
  uint32_t numPoints;         // nx*ny*nz <= 2^31 - 1
  uint32_t nx, ny;
  float lo[3], step[3];       // lattice point i on axis a: lo[a] + (float(i) + 0.5f) * step[a]
  uint32_t kinds;             // nibble s: the kind of sources[s]
  uint32_t needPosition : 1;  // a source is a radius or a coordinate
  uint32_t hasWeight : 1, minMax : 1, numAxes : 2, numValues : 3;
  IsoProfileSource sources[kIsoProfileSlots];
  IsoProfileKey axes[2];
  const int32_t *labels;      // axes[0].mode == kIsoProfileLabels: numPoints
  uint32_t numBlocks;         // of kIsoBlock points
  uint32_t *bins;             // numPoints
  unsigned long long *counters;   // [kIsoProfileCounters], and behind them the [kIsoProfileSeries] 32-bit words of the bits of
                              // max |term| over the binned points, zeroed by the host
  int32_t exponent[kIsoProfileSeries];  // accumulate: the series' exponents
  uint32_t numBins;           // B
  unsigned long long *sums;   // [hasWeight + numValues][B]
  unsigned long long *count;  // [B]
  uint32_t *keyMin, *keyMax;  // [numValues][B] each, with minMax; finish turns them into floats in place
};

hipError_t launchIsoProfileClassify(const IsoProfileArgs &a, hipStream_t s);
hipError_t launchIsoProfileAccumulate(const IsoProfileArgs &a, hipStream_t s);     // LDS or HBM by isoProfileLdsTable
hipError_t launchIsoProfileFinish(const IsoProfileArgs &a, hipStream_t s);

// ---- exact Euclidean distance transform on the lattice (exa_hip_distance): per lattice point the distance to the nearest
// point of a target set and that point's index, by one pass per axis (include/exa_hip.h states the passes; they are the
// contract).  A run of the passes serves one target set: the inside points, or (toOutside) the others.
//   inside   the regions' inside test on the values, or the label rule on the labels: a byte per point, and the count
//   row      a wave per row (j, k), 64 points per step: a ballot of the target bytes, per lane the nearest set bit at or below
//            and at or above it by clz / ctz on the masked ballot; the last target of the chunks behind and the next one of
//            the chunks ahead are carried along the row (the look-ahead reads every chunk once).  Writes a; gx is never
//            stored, it is term_x(i - a)
//   column   one lane per point, lanes along x, so a neighbouring row is read in whole lines.  A lane scans d = 0, 1, 2, ...
//            on both sides and stops once term(d) > min(best, limit): the terms are monotone in d and a sum is no smaller
//            than its term, so nothing further out can win or tie, and what lies beyond the limit is dropped by the finish
//            pass anyway.  The minus side accepts <=, the plus side <: of equal candidates the smallest index stays.  Two
//            steps a round, their four loads issued ahead of the stop tests (a side beyond the axis reads its own point).  Runs
//            along y (reads a; writes b, gy), then along z (reads gy; writes c, d2).  EXA_DISTANCE_LDS: a block stages a slab
//            of 64 columns by the whole scan axis in LDS first, where the axis fits (kIsoDistanceLdsAxis); plain loads beyond
//   finish   the reach test, the square root, the sign, the two dependent gathers of `nearest`; reached points and the
//            largest |dist| (an integer max on the float's bits).  With onlyOthers only the points that are not targets are
//            written: EXA_DISTANCE_SIGNED runs the passes once per target set and each finish writes its own half
#ifndef EXA_DISTANCE_LDS
#define EXA_DISTANCE_LDS 0
#endif
static const uint32_t kIsoDistanceTiles = 16;             // blocks of the lattice per block of the inside and the finish pass
static const uint32_t kIsoDistanceLdsAxis = 256;          // 64 columns x 256 floats = 64 KiB of LDS per workgroup
static const int kIsoDistanceInside = 0, kIsoDistanceReached = 1, kIsoDistanceMaxBits = 2, kIsoDistanceCounters = 3;

struct IsoDistanceArgs {
  uint32_t numPoints;         // nx*ny*nz <= 2^31 - 1
  uint32_t nx, ny, nz;
  uint32_t numBlocks;         // of kIsoBlock points
  float h[3];                 // the spacing; term_a(d) = o*o, o = h[a] * float(d)
  float limit;                // maxDistance * maxDistance
  const float *values;        // the inside pass of a field: numPoints
  const int32_t *labels;      // the inside pass of a mask: numPoints
  int32_t label;              // -1: any label >= 0
  float iso;
  uint32_t byLabel : 1, below : 1;
  uint32_t toOutside : 1;     // the run: the targets are the points that are not inside
  uint32_t negative : 1;      // finish: -dist
  uint32_t onlyOthers : 1;    // finish: leave the targets' outputs alone
  uint8_t *inside;            // numPoints
  int32_t *a, *b, *c;         // numPoints each: the nearest target of the row, the argmin along y, along z (-1: none)
  float *gy, *d2;             // numPoints each
  float *dist;                // numPoints
  int32_t *nearest;           // numPoints, or nullptr
  unsigned long long *counters;   // [kIsoDistanceCounters], zeroed by the host
};

hipError_t launchIsoDistanceInside(const IsoDistanceArgs &a, hipStream_t s);
hipError_t launchIsoDistanceRows(const IsoDistanceArgs &a, hipStream_t s);
hipError_t launchIsoDistanceColumns(const IsoDistanceArgs &a, int axis, hipStream_t s);       // axis 1, then axis 2
hipError_t launchIsoDistanceFinish(const IsoDistanceArgs &a, hipStream_t s);

} // namespace exa
