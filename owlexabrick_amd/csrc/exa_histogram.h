// exa_histogram.h — histogram and value range of one channel's cells (exa_hip_histogram): what exa_stats.cpp and
// exa_histogram.hip share.  include/exa_hip.h states the contract (slots, box, classes, bins, min / max).
//
// The pass.  The host cuts every brick into segments of at most kHistSegCells consecutive cells, sorts the segments by
// brick level (stable) and cuts each level's list into runs of about equal cell count: one workgroup per run (built once
// per handle; the box does not change it, a brick_order change does not either: a segment names its brick, and the kernel
// reads the brick's `begin` from the device's brick list).  A wave takes every fourth segment of its run, 64 consecutive
// cells per load instruction, four loads in flight per lane; increments go to the workgroup's counters in LDS; one flush
// per workgroup at its end, with 64-bit integer adds — a run holds one level, so the volume weight 8^level is applied to
// the flushed cell counts, not per cell.  No float is ever summed: the result is exact and the same for any order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace exa {

static const uint32_t kHistBlock = 256;          // threads per workgroup (4 waves)
static const uint32_t kHistSegCells = 2048;      // cells per segment: 8 rounds of 4 loads per lane
static const uint32_t kHistMaxBins = 4096;       // EXA_HIST_MAX_BINS: 16 KiB of LDS counters, 8 workgroups per CU
// Cells per run at the most.  The workgroup's LDS counters and the waves' class counters are 32 bits wide and flushed
// once, at the end of the run: a counter cannot exceed the run's cell count, which stays below 2^32 with room to spare.
static const uint64_t kHistRunMaxCells = 1ull << 30;

// the result on the device, 64-bit words: cells[numBins] | volume[numBins] | counts (kHistStat*) | levelCells[32] |
// {min key, max key} (two 32-bit words; the ordered key of a float: bits ^ (sign ? 0xffffffff : 0x80000000))
enum { kHistStatEmpty = 0, kHistStatNan, kHistStatUnder, kHistStatOver, kHistStatBinned, kHistStatCount, kHistLevels = 32 };
inline size_t histResultWords(uint32_t numBins) { return 2 * size_t(numBins) + kHistStatCount + kHistLevels + 1; }

// kHistSegCells consecutive cells of a brick (fewer at its end), from the cell at (x0, y0, z0)
struct HistSeg { uint32_t brick, x0, y0, z0; };

struct HistArgs {
  const int4 *bricks;            // the device's brick list (two int4 per brick)
  const float *field;            // scalars + channelOffset[channel]
  const HistSeg *segs;           // sorted by level
  const uint32_t *runBegin;      // numRuns + 1 offsets into segs; a run is not empty and holds one level
  uint32_t numRuns;
  int32_t numBins;               // 0: range only
  float lo, hi, scale;           // scale = float(numBins) / (hi - lo)
  int32_t emptyCells;            // the scene is marked allowEmptyCells
  int32_t hasBox;
  int32_t box[6];                // lo.xyz, hi.xyz in voxel coordinates
  int32_t withVolume;
  unsigned long long *result;    // histResultWords(numBins) words, initialised by the host
};

hipError_t launchHistogram(const HistArgs &a, hipStream_t s);

} // namespace exa
