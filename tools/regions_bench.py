#!/usr/bin/env python3
"""Cost of exa_hip_regions on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): a --size^3 lattice
over the voxel bounds; the regions of channel 0 >= 0.5 joined along the Kuhn edges and along the faces only, and the regions
of Q of the three fields >= 0 (many small regions).  After a warm-up call, --reps calls are timed: device ms per stage
(values, init, merge, flatten, rank, stats — the module's own events around each stage) and the wall time of the whole call
(allocations and the two small read-backs included); median, and spread = (max - min) / median.  With each: the number of
regions and of inside points, and the largest region.

The yardsticks, in the same run: exa_hip_resample (exa_hip_resample_derived for Q) of the same lattice into device memory,
which is the values stage, and a device-to-device copy of 8 bytes per lattice point (the values and the labels, read or
written once).  No ratio is a pass criterion.  One JSON line per measurement; --out also writes them to a file
(profiles/regions_bench.txt)."""
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
STAGES = ["values", "init", "merge", "flatten", "rank", "stats"]


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
    grid = torch.empty(n, dtype=torch.float32, device=DEV)
    ref = {}
    ref["channel"] = device_ms(lambda: R.resample(lo, hi, dims, out_ptr=grid, stream=stream, async_=True))
    emit(dict(what="resample_reference", dims=dims, n=n, reps=args.reps, kernel_ms=ref["channel"][0], spread=ref["channel"][1]))
    ref["q"] = device_ms(lambda: R.resampleDerived(lo, hi, dims, "q", out_ptr=grid, stream=stream, async_=True))
    emit(dict(what="resample_derived_reference", quantity="q", dims=dims, n=n, reps=args.reps, kernel_ms=ref["q"][0], spread=ref["q"][1]))
    src, dst = torch.empty(2 * n, dtype=torch.float32, device=DEV), torch.empty(2 * n, dtype=torch.float32, device=DEV)
    copy_ms, copy_spread = device_ms(lambda: dst.copy_(src))
    emit(dict(what="copy_reference", bytes_per_point=8, n=n, reps=args.reps, kernel_ms=copy_ms, spread=copy_spread,
              gb_per_s_read_plus_written=round(2 * 8 * n / copy_ms * 1e-6, 1) if copy_ms else None))
    del grid, src, dst

    cases = [("channel0_kuhn", dict(iso=0.5, channel=0), "channel"), ("channel0_faces", dict(iso=0.5, channel=0, faces=True), "channel"),
             ("q_kuhn", dict(iso=0.0, quantity="q", channels=(0, 1, 2)), "q")]
    for name, kw, yard in cases:
        counts = R.extractRegions(lo, hi, dims, **kw)                        # warm-up
        table = R.readRegions()["regions"]
        stages, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            R.extractRegions(lo, hi, dims, **kw)
            wall.append(1e3 * (time.perf_counter() - t))
            stages.append(R.regionsStageMs())
        R.releaseRegions()
        ms, spread = {}, {}
        for k, stage in enumerate(STAGES):
            ms[stage], spread[stage] = summary([s[k] for s in stages])
        label_ms, label_spread = summary([sum(s[1:]) for s in stages])
        wall_ms, wall_spread = summary(wall)
        ref_ms = ref[yard][0]
        emit(dict(what="regions", case=name, dims=dims, n=n, iso=kw["iso"], faces=bool(kw.get("faces")), reps=args.reps,
                  num_regions=counts[0], num_inside=counts[1], sum_exponent=counts[2],
                  largest_region=int(table["points"].max()) if len(table) else 0,
                  single_point_regions=int((table["points"] == 1).sum()),
                  stage_ms=ms, stage_spread=spread, labelling_stages_ms=label_ms, labelling_stages_spread=label_spread,
                  call_wall_ms=wall_ms, call_wall_spread=wall_spread,
                  values_over_resample=round(ms["values"] / ref_ms, 3) if ref_ms else None,
                  labelling_over_resample=round(label_ms / ref_ms, 3) if ref_ms else None,
                  labelling_over_copy=round(label_ms / copy_ms, 3) if copy_ms else None))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
