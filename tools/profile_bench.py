#!/usr/bin/env python3
"""Cost of exa_hip_profile on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): a --size^3 lattice
over the voxel bounds, five cases:
  a  a 256-bin profile of channel 1 by channel 0
  b  a 256 x 256 phase plot of (channel 0, Q) with two values
  c  the labels of regionsDerived Q >= 0 as the axis (in device memory) with three values: one region holds most of the
     lattice, the worst case for traffic to equal bins
  d  a constant key (a coordinate over a range that puts every point into one of 256 bins)
  e  a radial profile of channel 0: no values stage for the key
After a warm-up call, --reps calls are timed: device ms per stage (values, classify, accumulate, finish — the module's own
events) and the wall time of the whole call; median, and spread = (max - min) / median.

The yardsticks, in the same run: exa_hip_resample / exa_hip_resample_derived of the lattice into device memory (the values
stage is one of them per distinct source), a device-to-device copy of the bytes that classify and accumulate read and write
per point (4 per key and per value read by each of the two passes, 4 for the bin index written and 4 per series read back),
and for (c) the stats stage of exa_hip_regions on the same labels.  No ratio is a pass criterion.  One JSON line per
measurement; --out also writes them to a file (profiles/profile_bench.txt)."""
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
from owlexabrick_amd.binding import channel, coordinate, derived, radius  # noqa: E402

DEV = "cuda:0"
STAGES = ["values", "classify", "accumulate", "finish"]


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
    emit(dict(config=args.config, scale=args.scale, fields=3, bricks=int(prep.scene.numBricks), cells=int(prep.scene.totalCells),
              voxel_bounds=[lo.tolist(), hi.tolist()], lds_bytes_threshold="EXA_PROFILE_LDS_BYTES (exa_isomesh.h)",
              setup_s=round(time.time() - t0, 1)))
    S = args.size
    dims, n = (S, S, S), S ** 3
    stream = torch.cuda.current_stream().cuda_stream

    # the yardsticks
    grid = torch.empty(n, dtype=torch.float32, device=DEV)
    resample_ms, _ = device_ms(lambda: R.resample(lo, hi, dims, out_ptr=grid, stream=stream, async_=True))
    emit(dict(what="resample_reference", dims=dims, n=n, reps=args.reps, kernel_ms=resample_ms))
    q_ms, _ = device_ms(lambda: R.resampleDerived(lo, hi, dims, "q", out_ptr=grid, stream=stream, async_=True))
    emit(dict(what="resample_derived_reference", quantity="q", dims=dims, n=n, reps=args.reps, kernel_ms=q_ms))
    src, dst = torch.empty(n, dtype=torch.float32, device=DEV), torch.empty(n, dtype=torch.float32, device=DEV)
    copy_ms, copy_spread = device_ms(lambda: dst.copy_(src))                # 4 bytes per point read and 4 written
    emit(dict(what="copy_reference", bytes_per_point=4, n=n, reps=args.reps, kernel_ms=copy_ms, spread=copy_spread,
              gb_per_s_read_plus_written=round(2 * 4 * n / copy_ms * 1e-6, 1) if copy_ms else None))
    del src, dst

    # the ranges of the keys, from the lattices themselves
    c0 = R.resample(lo, hi, dims, channel=0)
    r0 = (float(np.nanmin(c0)), float(np.nanmax(c0)))
    q = R.resampleDerived(lo, hi, dims, "q")
    rq = tuple(float(v) for v in np.nanpercentile(q, [1, 99]))
    del c0, q
    centre = tuple(0.5 * (lo + hi))
    rmax = float(np.linalg.norm(hi - lo)) * 0.5

    # (c): the labels of Q >= 0, left on the device; the regions' own stats stage on them
    counts = R.extractRegions(lo, hi, dims, 0.0, quantity="q", channels=(0, 1, 2))
    stats_ms, _ = summary([(R.extractRegions(lo, hi, dims, 0.0, quantity="q", channels=(0, 1, 2)), R.regionsStageMs()[5])[1]
                           for _ in range(args.reps)])
    labels = torch.empty(n, dtype=torch.int32, device=DEV)
    table = R.readRegions()["regions"]
    R._check(binding.lib().exa_hip_regions_read(R.h, binding._dev_ptr(labels), None, None, 1, None))
    R.releaseRegions()
    emit(dict(what="regions_stats_reference", num_regions=counts[0], num_inside=counts[1], largest_region=int(table["points"].max()),
              stats_stage_ms=stats_ms))

    Q = derived("q", (0, 1, 2))
    # name, axes, values, weight; reads: the 4-byte loads per point of classify + accumulate (keys once, series twice, the bin
    # index written once and read once per series); sources: the resample yardsticks that bound the values stage
    cases = [
        ("a_profile_256", [binding.uniform(channel(0), *r0, 256)], [channel(1)], None, resample_ms * 2),
        ("b_phase_256x256", [binding.uniform(channel(0), *r0, 256), binding.uniform(Q, *rq, 256)], [channel(1), channel(2)], None,
         resample_ms * 3 + q_ms),
        ("c_region_labels", [binding.labels(labels, max(1, counts[0]))], [channel(0), channel(1), channel(2)], None, resample_ms * 3),
        ("d_constant_key", [binding.uniform(coordinate(0), float(lo[0]) - 1e6, float(hi[0]) + 1e6, 256)], [channel(1)], None, resample_ms),
        ("e_radial", [binding.uniform(radius(centre), 0.0, rmax, 256)], [channel(0)], None, resample_ms),
    ]
    for name, axes, values, weight, bound_ms in cases:
        got = R.profile(lo, hi, dims, axes, values, weight)                  # warm-up
        stages, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            R.profile(lo, hi, dims, axes, values, weight)
            wall.append(1e3 * (time.perf_counter() - t))
            stages.append(R.profileStageMs())
        ms, spread = {}, {}
        for k, stage in enumerate(STAGES):
            ms[stage], spread[stage] = summary([s[k] for s in stages])
        binning_ms, binning_spread = summary([s[1] + s[2] + s[3] for s in stages])
        wall_ms, wall_spread = summary(wall)
        keys = sum(1 for a in axes)
        series = len(values) + (1 if weight is not None else 0)
        words = keys + 2 * series + 1 + max(1, series)                       # 4-byte words per point over both passes
        st = got["stats"]
        emit(dict(what="profile", case=name, dims=dims, n=n, bins=int(got["count"].size), values=len(values), reps=args.reps,
                  lds_table=st["ldsTable"], binned=st["binned"], invalid=st["invalid"], outside=st["outside"],
                  under=st["under"], over=st["over"], largest_bin=int(got["count"].max()), occupied_bins=int(np.count_nonzero(got["count"])),
                  stage_ms=ms, stage_spread=spread, classify_accumulate_finish_ms=binning_ms, spread=binning_spread,
                  call_wall_ms=wall_ms, call_wall_spread=wall_spread,
                  values_over_resample_of_sources=round(ms["values"] / bound_ms, 3) if bound_ms else None,
                  binning_over_values=round(binning_ms / ms["values"], 3) if ms["values"] else None,
                  words_per_point=words, binning_over_copy_of_those_bytes=round(binning_ms / (copy_ms * words / 2), 3) if copy_ms else None,
                  accumulate_over_regions_stats=round(ms["accumulate"] / stats_ms, 3) if name.startswith("c_") and stats_ms else None))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
