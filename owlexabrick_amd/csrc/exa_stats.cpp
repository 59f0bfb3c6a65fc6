// exa_stats.cpp — statistics of the cells themselves: exa_hip_histogram (kernels in exa_histogram.hip, the pass is
// described in exa_histogram.h).
#include "exa_renderer.h"
#include "exa_histogram.h"

#include <cmath>
#include <cstring>

namespace {

static_assert(sizeof(HistSeg) == sizeof(uint4), "a segment is kept on the handle as a uint4");
static_assert(EXA_HIST_MAX_BINS == kHistMaxBins && EXA_HIST_MAX_LEVELS == kHistLevels, "the header's limits are the kernel's");

// runs the device is given at the least when the scene is large enough (256 CUs x 8 resident workgroups, twice), and the
// cells of a run at the least (one segment per wave)
const uint64_t kHistTargetRuns = 4096, kHistRunMinCells = 4 * uint64_t(kHistSegCells);

// The work list of the pass, once per handle: segments by level, cut into runs (exa_histogram.h), and whether the
// volume-weighted total fits 64 bits.  The brick geometry comes back from the device's own list.
int buildHistPlan(ExaHipRenderer *h, ExaHipRenderer *r, const char *fn)
{
  if (r->hist.planBuilt) return 0;
  std::vector<ExaBrick> bricks(r->numBricks);
  HIP_TRY(h, hipMemcpy(bricks.data(), r->bricks.p, bricks.size() * sizeof(ExaBrick), hipMemcpyDeviceToHost));
  uint64_t segsOfLevel[kHistLevels] = {}, cellsOfLevel[kHistLevels] = {}, slots = 0;
  for (const ExaBrick &B : bricks) {
    // (exa_hip_create already refuses a level above 30: this guards the contract's wording and the arrays below)
    if (B.level < 0 || B.level >= int(kHistLevels)) { h->fail(std::string(fn) + ": a brick level outside 0..31"); return 1; }
    const uint64_t vol = uint64_t(B.size[0]) * uint64_t(B.size[1]) * uint64_t(B.size[2]);
    segsOfLevel[B.level] += (vol + kHistSegCells - 1) / kHistSegCells;
    cellsOfLevel[B.level] += vol;
    slots += vol;
  }
  unsigned __int128 weighted = 0;
  bool fits = true;
  uint64_t numSegs = 0, first[kHistLevels];
  for (uint32_t L = 0; L < kHistLevels; L++) {
    first[L] = numSegs;
    numSegs += segsOfLevel[L];
    // cells * 8^L, summed in 128 bits while it still fits 64: a term is below 2^64 * 2^63, and no term is added to a
    // sum beyond 2^64
    if (fits && cellsOfLevel[L]) {
      if (3 * L >= 64) fits = false;
      else weighted += (unsigned __int128)cellsOfLevel[L] << (3 * L);
      if (weighted >> 64) fits = false;
    }
  }
  if (numSegs >= UINT32_MAX) { h->fail(std::string(fn) + ": the scene has more than 2^32 segments of 2048 cells"); return 1; }
  std::vector<HistSeg> segs(numSegs);
  {
    uint64_t at[kHistLevels];
    std::memcpy(at, first, sizeof(at));
    for (uint64_t b = 0; b < bricks.size(); b++) {
      const ExaBrick &B = bricks[b];
      const uint64_t vol = uint64_t(B.size[0]) * uint64_t(B.size[1]) * uint64_t(B.size[2]);
      const uint64_t sx = uint64_t(B.size[0]), sxy = sx * uint64_t(B.size[1]);
      for (uint64_t c = 0; c < vol; c += kHistSegCells)
        segs[at[B.level]++] = { uint32_t(b), uint32_t(c % sx), uint32_t(c % sxy / sx), uint32_t(c / sxy) };
    }
  }
  const uint64_t runCells = std::min(kHistRunMaxCells, std::max(kHistRunMinCells, slots / kHistTargetRuns));
  std::vector<uint32_t> runs;
  for (uint32_t L = 0; L < kHistLevels; L++) {
    uint64_t inRun = 0;
    for (uint64_t s = first[L]; s < first[L] + segsOfLevel[L]; s++) {
      if (inRun == 0) runs.push_back(uint32_t(s));
      const ExaBrick &B = bricks[segs[s].brick];
      const uint64_t vol = uint64_t(B.size[0]) * uint64_t(B.size[1]) * uint64_t(B.size[2]);
      const uint64_t at = (uint64_t(segs[s].z0) * uint64_t(B.size[1]) + segs[s].y0) * uint64_t(B.size[0]) + segs[s].x0;
      inRun += std::min<uint64_t>(kHistSegCells, vol - at);
      if (inRun >= runCells) inRun = 0;
    }
  }
  const uint32_t numRuns = uint32_t(runs.size());
  runs.push_back(uint32_t(numSegs));
  HIP_TRY(h, r->hist.segs.upload(reinterpret_cast<const uint4 *>(segs.data()), segs.size()));
  HIP_TRY(h, r->hist.runs.upload(runs.data(), runs.size()));
  r->hist.numRuns = numRuns;
  r->hist.volumeFits = fits;
  r->hist.planBuilt = true;
  return 0;
}

float keyToFloat(uint32_t key)
{
  const uint32_t bits = key ^ ((key >> 31) ? 0x80000000u : 0xffffffffu);
  float v;
  std::memcpy(&v, &bits, sizeof(v));
  return v;
}

} // namespace

extern "C" int exa_hip_histogram(ExaHipRenderer *h, int32_t channel, float lo, float hi, int32_t numBins, const int32_t box[6],
                                 uint64_t *cells, uint64_t *volume, ExaHipFieldStats *stats, void *hipStream)
{
  if (!h) return 1;
  const char *fn = "exa_hip_histogram";
  if (!checkChannel(h, fn, channel)) return 1;
  if (numBins < 0 || numBins > EXA_HIST_MAX_BINS) { h->fail(std::string(fn) + ": numBins must be 0 (range only) .. 4096"); return 1; }
  float scale = 0.f;
  if (numBins > 0) {
    if (!(std::isfinite(lo) && std::isfinite(hi) && lo < hi)) { h->fail(std::string(fn) + ": the range needs finite lo < hi"); return 1; }
    const float width = hi - lo;
    scale = float(numBins) / width;
    if (!std::isfinite(width) || !std::isfinite(scale)) { h->fail(std::string(fn) + ": hi - lo and numBins / (hi - lo) must be finite in float32"); return 1; }
    if (!cells) { h->fail(std::string(fn) + ": null cells array"); return 1; }
  } else {
    lo = hi = 0.f;
    cells = volume = nullptr;
  }
  bool emptyBox = false;
  if (box)
    for (int k = 0; k < 3; k++) {
      if (box[k] > box[3 + k]) { h->fail(std::string(fn) + ": the box needs lo <= hi on every axis"); return 1; }
      emptyBox = emptyBox || box[k] == box[3 + k];
    }
  ExaHipRenderer *r = firstChild(h);
  EXA_ON_DEVICE_OF(h, r);
  hipStream_t s = (hipStream_t)hipStream;
  if (buildHistPlan(h, r, fn)) return 1;
  if (volume && !r->hist.volumeFits) { h->fail(std::string(fn) + ": the scene's volume in finest voxels (cells x 8^level over all bricks) does not fit 64 bits: pass volume = NULL"); return 1; }
  if (r->applyBrickOrder(s)) { h->fail(r->err); return 1; }

  const size_t words = histResultWords(uint32_t(numBins)), statAt = 2 * size_t(numBins);
  std::vector<unsigned long long> res(words, 0ull);
  res[words - 1] = 0x00000000ffffffffull;                       // {min key, max key} of no value
  r->hist.kernelMs = 0.f;
  if (!emptyBox) {
    TimingEvents<2> t;                                          // around the call's kernel (exa_hip_histogram_ms)
    HIP_TRY(h, t.create());
    if (r->hist.result.n < words) HIP_TRY(h, r->hist.result.alloc(histResultWords(kHistMaxBins)));
    HistArgs a;
    std::memset(&a, 0, sizeof(a));
    a.bricks = r->bricks.p;
    a.field = r->scalars.p + r->sc.channelOffset[channel];
    a.segs = reinterpret_cast<const HistSeg *>(r->hist.segs.p);
    a.runBegin = r->hist.runs.p;
    a.numRuns = r->hist.numRuns;
    a.numBins = numBins;
    a.lo = lo; a.hi = hi; a.scale = scale;
    a.emptyCells = r->emptyCells ? 1 : 0;
    a.hasBox = box ? 1 : 0;
    if (box) for (int k = 0; k < 6; k++) a.box[k] = box[k];
    a.withVolume = volume ? 1 : 0;
    a.result = r->hist.result.p;
    HIP_TRY(h, hipMemcpyAsync(r->hist.result.p, res.data(), words * sizeof(res[0]), hipMemcpyHostToDevice, s));
    HIP_TRY(h, hipEventRecord(t.ev[0], s));
    HIP_TRY(h, launchHistogram(a, s));
    HIP_TRY(h, hipEventRecord(t.ev[1], s));
    HIP_TRY(h, hipMemcpyAsync(res.data(), r->hist.result.p, words * sizeof(res[0]), hipMemcpyDeviceToHost, s));
    HIP_TRY(h, hipStreamSynchronize(s));
    HIP_TRY(h, t.elapsed(0, 1, &r->hist.kernelMs));
  }
  for (int32_t i = 0; i < numBins; i++) {
    cells[i] = res[i];
    if (volume) volume[i] = res[size_t(numBins) + i];
  }
  if (stats) {
    std::memset(stats, 0, sizeof(*stats));
    stats->empty = res[statAt + kHistStatEmpty];
    stats->nan = res[statAt + kHistStatNan];
    stats->under = res[statAt + kHistStatUnder];
    stats->over = res[statAt + kHistStatOver];
    stats->binned = res[statAt + kHistStatBinned];
    stats->slots = stats->empty + stats->nan + stats->under + stats->over + stats->binned;
    for (uint32_t L = 0; L < kHistLevels; L++) stats->levelCells[L] = res[statAt + kHistStatCount + L];
    const uint32_t keyMin = uint32_t(res[words - 1]), keyMax = uint32_t(res[words - 1] >> 32);
    const bool any = stats->under + stats->over + stats->binned != 0;
    stats->min = any ? keyToFloat(keyMin) : INFINITY;
    stats->max = any ? keyToFloat(keyMax) : -INFINITY;
  }
  return 0;
}

extern "C" int exa_hip_histogram_ms(ExaHipRenderer *h, float *ms)
{
  if (!h || !ms) return 1;
  *ms = firstChild(h)->hist.kernelMs;
  return 0;
}
