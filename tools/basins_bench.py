#!/usr/bin/env python3
"""Cost of exa_hip_basins on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): a --size^3 lattice
over the voxel bounds; the basins of channel 0 >= 0.5 and of Q of the three fields >= 0 (the case exa_hip_regions leaves in
one giant region), each at three depths: 0 (every peak a basin), a middle one (the median of the finite depths of the table
at depth 0) and +inf (the regions).  After a warm-up call, --reps calls are timed: device ms per stage (values, ascent,
passes, links, rank, stats — the module's own events around each stage) and the wall time of the whole call (allocations
and the small read-backs that steer the rounds included); median, and spread = (max - min) / median.  With each: the rounds,
the raw and the final number of basins, the largest basin.

The yardstick, in the same process on the same lattice: exa_hip_regions with the same flags, its stages behind the values
and its wall time.  For Q at the middle depth also where the giant region of exa_hip_regions ends up: how many basins its
points go to, and the share of its points in the largest of them and in the fewest basins that hold half and nine tenths
of them.  No ratio is a pass criterion.  One JSON line per measurement; --out also writes them to a file
(profiles/basins_bench.txt)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from owlexabrick_amd import binding, scenes  # noqa: E402

STAGES = ["values", "ascent", "passes", "links", "rank", "stats"]
REGION_STAGES = ["values", "init", "merge", "flatten", "rank", "stats"]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def summary(xs):
        m = statistics.median(xs)
        return round(m, 3), (round((max(xs) - min(xs)) / m, 4) if m else None)

    def timed(extract, stage_ms, names):
        """reps calls behind a warm-up: per stage, the stages behind the values, and the wall time, each (median, spread)"""
        stages, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            extract()
            wall.append(1e3 * (time.perf_counter() - t))
            stages.append(stage_ms())
        ms, spread = {}, {}
        for k, stage in enumerate(names):
            ms[stage], spread[stage] = summary([s[k] for s in stages])
        return ms, spread, summary([sum(s[1:]) for s in stages]), summary(wall)

    t0 = time.time()
    scene = scenes.config(args.config, scale=args.scale, threads=args.threads, fields=3)
    prep = binding.Prep(scene, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    lo, hi = (np.asarray(b, np.float32) for b in prep.voxel_bounds())
    emit(dict(config=args.config, scale=args.scale, fields=3, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], setup_s=round(time.time() - t0, 1)))
    S = args.size
    dims, n = (S, S, S), S ** 3

    cases = [("channel0", dict(iso=0.5, channel=0)), ("q", dict(iso=0.0, quantity="q", channels=(0, 1, 2)))]
    for name, kw in cases:
        # the yardstick: the regions of the same lattice
        counts = R.extractRegions(lo, hi, dims, **kw)                        # warm-up
        regions = R.readRegions()
        r_ms, r_spread, (r_label, r_label_spread), (r_wall, r_wall_spread) = timed(
            lambda: R.extractRegions(lo, hi, dims, **kw), R.regionsStageMs, REGION_STAGES)
        R.releaseRegions()
        giant = int(np.argmax(regions["regions"]["points"])) if counts[0] else -1
        giant_points = int(regions["regions"]["points"][giant]) if counts[0] else 0
        emit(dict(what="regions", case=name, dims=dims, n=n, iso=kw["iso"], reps=args.reps, num_regions=counts[0], num_inside=counts[1],
                  largest_region=giant_points, stage_ms=r_ms, stage_spread=r_spread, labelling_stages_ms=r_label,
                  labelling_stages_spread=r_label_spread, call_wall_ms=r_wall, call_wall_spread=r_wall_spread))
        in_giant = (regions["labels"] == giant).reshape(-1) if counts[0] else np.zeros(n, bool)
        del regions

        iso = kw["iso"]
        rest = {k: v for k, v in kw.items() if k != "iso"}
        R.extractBasins(lo, hi, dims, iso, 0.0, **rest)
        depth = R.readBasins()["basins"]["depth"]
        finite = depth[np.isfinite(depth)]
        middle = float(np.median(finite)) if finite.size else 1.0
        for level, min_depth in (("zero", 0.0), ("middle", middle), ("inf", float("inf"))):
            counts = R.extractBasins(lo, hi, dims, iso, min_depth, **rest)    # warm-up
            got = R.readBasins()
            ms, spread, (label_ms, label_spread), (wall_ms, wall_spread) = timed(
                lambda: R.extractBasins(lo, hi, dims, iso, min_depth, **rest), R.basinsStageMs, STAGES)
            R.releaseBasins()
            table = got["basins"]
            rec = dict(what="basins", case=name, level=level, min_depth=min_depth if np.isfinite(min_depth) else "inf", dims=dims, n=n,
                       iso=iso, reps=args.reps, num_basins=counts[0], num_raw=counts[1], num_inside=counts[2], rounds=counts[4],
                       largest_basin=int(table["points"].max()) if len(table) else 0,
                       stage_ms=ms, stage_spread=spread, basin_stages_ms=label_ms, basin_stages_spread=label_spread,
                       call_wall_ms=wall_ms, call_wall_spread=wall_spread,
                       basin_stages_over_regions_stages=round(label_ms / r_label, 3) if r_label else None,
                       call_wall_over_regions_wall=round(wall_ms / r_wall, 3) if r_wall else None)
            if giant_points:
                # where the points of the regions' giant go
                share = np.sort(np.bincount(got["labels"].reshape(-1)[in_giant], minlength=len(table)))[::-1]
                share = share[share > 0]
                run = np.cumsum(share)
                rec.update(giant_region_points=giant_points, giant_region_basins=int(len(share)),
                           giant_share_of_largest_basin=round(float(share[0]) / giant_points, 4),
                           basins_holding_half_of_giant=int(np.searchsorted(run, 0.5 * giant_points) + 1),
                           basins_holding_nine_tenths_of_giant=int(np.searchsorted(run, 0.9 * giant_points) + 1))
            emit(rec)
            del got
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
