#!/usr/bin/env python3
"""Cost of exa_hip_distance on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): a --size^3 lattice
over the voxel bounds, four target sets
  sparse  channel 0 >= 0.5
  dense   Q >= 0
  wall    the points without data (iso = -FLT_MAX, to_outside), on the box grown by a tenth of its extent on every side:
          the voxel bounds themselves hold no such point
  none    channel 0 >= FLT_MAX: no target at all, so that without a reach every lane walks its whole column, the worst case
each with max_distance = +INF and = 8 lattice cells, with and without `nearest`; outputs in device memory.  After a warm-up
call, --reps calls are timed: device ms per stage (values, rows, columns, finish — the module's own events) and the wall
time of the whole call; median, and spread = (max - min) / median.  --cases picks target sets by name.

The yardsticks, in the same process: exa_hip_resample / exa_hip_resample_derived of the lattice into device memory (the
values stage is one of them plus the inside pass) and a device-to-device copy of 4 bytes per point.  No ratio is a pass
criterion: few and far targets without a reach cost O(points x axis length) by design.  One JSON line per measurement;
--out also writes them to a file (profiles/distance_bench.txt)."""
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
from owlexabrick_amd import distance as dt  # noqa: E402

DEV = "cuda:0"
STAGES = ["values", "rows", "columns", "finish"]
FLT_MAX = float(np.finfo(np.float32).max)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--cases", default="sparse,dense,wall,none")
    ap.add_argument("--label", default=None, help="a word for every line (which build of the module this is)")
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        if args.label:
            rec = dict(label=args.label, **rec)
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
    emit(dict(config=args.config, scale=args.scale, fields=3, bricks=int(prep.scene.numBricks), cells=int(prep.scene.totalCells),
              voxel_bounds=[lo.tolist(), hi.tolist()], lib=os.path.basename(binding.LIB_PATH), setup_s=round(time.time() - t0, 1)))
    S = args.size
    dims, n = (S, S, S), S ** 3
    stream = torch.cuda.current_stream().cuda_stream

    # the yardsticks
    grid = torch.empty(n, dtype=torch.float32, device=DEV)
    resample_ms, _ = device_ms(lambda: R.resample(lo, hi, dims, out_ptr=grid, stream=stream, async_=True))
    emit(dict(what="resample_reference", dims=dims, n=n, reps=args.reps, kernel_ms=resample_ms))
    q_ms, _ = device_ms(lambda: R.resampleDerived(lo, hi, dims, "q", out_ptr=grid, stream=stream, async_=True))
    emit(dict(what="resample_derived_reference", quantity="q", dims=dims, n=n, reps=args.reps, kernel_ms=q_ms))
    src = torch.empty(n, dtype=torch.float32, device=DEV)
    copy_ms, copy_spread = device_ms(lambda: grid.copy_(src))                # 4 bytes per point read and 4 written
    emit(dict(what="copy_reference", bytes_per_point=4, n=n, reps=args.reps, kernel_ms=copy_ms, spread=copy_spread,
              gb_per_s_read_plus_written=round(2 * 4 * n / copy_ms * 1e-6, 1) if copy_ms else None))
    del src

    ext = hi - lo
    wlo, whi = (lo - np.float32(0.1) * ext).astype(np.float32), (hi + np.float32(0.1) * ext).astype(np.float32)
    grown_ms, _ = device_ms(lambda: R.resample(wlo, whi, dims, out_ptr=grid, stream=stream, async_=True))
    emit(dict(what="resample_reference_grown_box", dims=dims, n=n, reps=args.reps, kernel_ms=grown_ms))
    dist = grid
    near = torch.empty(n, dtype=torch.int32, device=DEV)
    sets = {"sparse": (dict(iso=0.5, channel=0), resample_ms, (lo, hi)),
            "dense": (dict(iso=0.0, quantity="q", channels=(0, 1, 2)), q_ms, (lo, hi)),
            "wall": (dict(iso=-FLT_MAX, channel=0, to_outside=True), grown_ms, (wlo, whi)),
            "none": (dict(iso=FLT_MAX, channel=0), resample_ms, (lo, hi))}
    for name in args.cases.split(","):
        kw, values_ms, (blo, bhi) = sets[name]
        for reach_cells in (None, 8):
            reach = float("inf") if reach_cells is None else reach_cells * float(((bhi - blo) / np.float32(S)).max())
            for nearest in (False, True):
                call = lambda: dt.distance(R, blo, bhi, dims, max_distance=reach, out=(dist, near if nearest else None), **kw)   # noqa: E731
                got = call()                                                # warm-up
                stages, wall = [], []
                for _ in range(args.reps):
                    t = time.perf_counter()
                    call()
                    wall.append(1e3 * (time.perf_counter() - t))
                    stages.append(dt.distance_stage_ms(R))
                ms, spread = {}, {}
                for k, stage in enumerate(STAGES):
                    ms[stage], spread[stage] = summary([s[k] for s in stages])
                passes_ms, passes_spread = summary([s[1] + s[2] + s[3] for s in stages])
                wall_ms, wall_spread = summary(wall)
                st = got["stats"]
                emit(dict(what="distance", case=name, max_distance_cells=reach_cells, nearest=nearest, dims=dims, n=n, reps=args.reps,
                          inside=st["inside"], reached=st["reached"], max_distance_found=st["maxDistance"],
                          targets=st["points"] - st["inside"] if kw.get("to_outside") else st["inside"],
                          stage_ms=ms, stage_spread=spread, rows_columns_finish_ms=passes_ms, spread=passes_spread,
                          call_wall_ms=wall_ms, call_wall_spread=wall_spread,
                          values_over_resample=round(ms["values"] / values_ms, 3) if values_ms else None,
                          passes_over_resample=round(passes_ms / values_ms, 3) if values_ms else None,
                          passes_over_copy=round(passes_ms / copy_ms, 3) if copy_ms else None))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
