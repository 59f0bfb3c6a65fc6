#!/usr/bin/env python3
"""Cost of exa_hip_critical_points on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): a --size^3
lattice over the voxel bounds, the zeros of the vector field of the three channels, with and without the probe.  After a
warm-up call, --reps calls are timed: device ms per stage (values, cells, scans, refine, emit, probe — the module's own events
around each stage) and the wall time of the whole call (allocations and the two small read-backs included); median, and
spread = (max - min) / median.  With each: the seven stats and the found points by n+.

The yardsticks, in the same run: three exa_hip_resample calls of the same lattice into device memory, which is the values
stage; a device-to-device copy of the 12 bytes per lattice point that the cell pass reads once, its floor; and
exa_hip_regions of channel 0 >= 0.5 on the same lattice (its stages behind the values).  No ratio is a pass criterion.  One
JSON line per measurement; --out also writes them to a file (profiles/critical_bench.txt)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from owlexabrick_amd import binding, scenes  # noqa: E402

DEV = "cuda:0"
STAGES = ["values", "cells", "scans", "refine", "emit", "probe"]


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

    def device_ms(fn):
        fn()                                                                # warm-up
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return summary(ms)

    t0 = time.time()
    scene = scenes.config(args.config, scale=args.scale, threads=args.threads, fields=3)
    prep = binding.Prep(scene, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    lo, hi = (np.asarray(b, np.float32) for b in prep.voxel_bounds())
    emit(dict(config=args.config, scale=args.scale, fields=3, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], setup_s=round(time.time() - t0, 1)))
    S = args.size
    dims, n = (S, S, S), S ** 3
    stream = torch.cuda.current_stream().cuda_stream

    # the yardsticks
    grid = torch.empty(3 * n, dtype=torch.float32, device=DEV)

    def three_lattices():
        for c in range(3):
            R.resample(lo, hi, dims, channel=c, out_ptr=grid[c * n:], stream=stream, async_=True)

    values_ms, values_spread = device_ms(three_lattices)
    emit(dict(what="resample_reference", channels=3, dims=dims, n=n, reps=args.reps, kernel_ms=values_ms, spread=values_spread))
    dst = torch.empty(3 * n, dtype=torch.float32, device=DEV)
    copy_ms, copy_spread = device_ms(lambda: dst.copy_(grid))
    emit(dict(what="copy_reference", bytes_per_point=12, n=n, reps=args.reps, kernel_ms=copy_ms, spread=copy_spread,
              gb_per_s_read_plus_written=round(2 * 12 * n / copy_ms * 1e-6, 1) if copy_ms else None))
    del grid, dst
    R.extractRegions(lo, hi, dims, iso=0.5, channel=0)                       # warm-up
    stages = []
    for _ in range(args.reps):
        R.extractRegions(lo, hi, dims, iso=0.5, channel=0)
        stages.append(R.regionsStageMs())
    R.releaseRegions()
    regions_values_ms, _ = summary([s[0] for s in stages])
    regions_ms, regions_spread = summary([sum(s[1:]) for s in stages])
    emit(dict(what="regions_reference", case="channel0_kuhn", iso=0.5, dims=dims, n=n, reps=args.reps, values_ms=regions_values_ms,
              labelling_stages_ms=regions_ms, labelling_stages_spread=regions_spread))

    for name, kw in [("plain", dict()), ("probe", dict(probe=True)), ("iterations_32", dict(iterations=32))]:
        _, stats = R.extractCriticalPoints(lo, hi, dims, channels=(0, 1, 2), **kw)      # warm-up
        points = R.readCriticalPoints()[0]
        stages, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            R.extractCriticalPoints(lo, hi, dims, channels=(0, 1, 2), **kw)
            wall.append(1e3 * (time.perf_counter() - t))
            stages.append(R.criticalPointsStageMs())
        R.releaseCriticalPoints()
        ms, spread = {}, {}
        for k, stage in enumerate(STAGES):
            ms[stage], spread[stage] = summary([s[k] for s in stages])
        rest_ms, rest_spread = summary([sum(s[1:]) for s in stages])
        wall_ms, wall_spread = summary(wall)
        emit(dict(what="critical_points", case=name, dims=dims, n=n, iterations=kw.get("iterations", 8), tolerance=2.0 ** -10,
                  reps=args.reps, stats=stats, by_n_plus=np.bincount(points["type"] & 3, minlength=4).tolist(),
                  spiral=int(((points["type"] & 4) != 0).sum()), degenerate=int(((points["type"] & 8) != 0).sum()),
                  stage_ms=ms, stage_spread=spread, stages_behind_values_ms=rest_ms, stages_behind_values_spread=rest_spread,
                  call_wall_ms=wall_ms, call_wall_spread=wall_spread,
                  values_over_resample=round(ms["values"] / values_ms, 3) if values_ms else None,
                  cells_over_values=round(ms["cells"] / ms["values"], 4) if ms["values"] else None,
                  cells_over_copy=round(ms["cells"] / copy_ms, 3) if copy_ms else None,
                  behind_values_over_regions_labelling=round(rest_ms / regions_ms, 3) if regions_ms else None))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
