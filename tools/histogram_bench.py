#!/usr/bin/env python3
"""Cost of exa_hip_histogram on the bench scene (scenes.config("c4_exajet")): the range-only pass, a 256-bin histogram over
min..max with and without the volume weights, and the same histogram on a constant extra field — every lane of every wave
in one bin, the worst case for contention on a counter.  Per pass: the device time of its kernel (the module's events
around the launch, exa_hip_histogram_ms), the wall time of the whole synchronous call, and channel bytes / kernel time.  The
yardstick, timed in the same loop: a device-to-device copy of one channel's bytes (it reads AND writes them; a pass that
only reads moves half the traffic).  After a warm-up of every pass, --reps rounds run the passes one after the other, so
that a drift of the machine hits all of them alike; medians and minima are reported.  One JSON line per pass."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from owlexabrick_amd import binding, scenes  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--bins", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    t0 = time.time()
    scene = scenes.config(args.config, scale=args.scale, threads=args.threads)
    const = len(scene.fields)
    scene.fields.append(np.full(len(scene.fields[0]), 0.5, dtype=np.float32))
    prep = binding.Prep(scene, num_region_fields=const, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    cells = int(prep.scene.totalCells)
    nbytes = 4 * cells
    emit(dict(config=args.config, scale=args.scale, bricks=int(prep.scene.numBricks), cells=cells, channel_bytes=nbytes,
              setup_s=round(time.time() - t0, 1)))
    st = R.fieldStats(0)
    lo, hi = float(st["min"]), float(st["max"])
    levels = {int(L): int(n) for L, n in enumerate(st["levelCells"]) if n}

    src = torch.empty(cells, dtype=torch.float32, device="cuda:0").normal_()
    dst = torch.empty_like(src)

    def copy():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t = time.perf_counter()
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), 1e3 * (time.perf_counter() - t), None

    def call(channel, a, b, bins, volume):
        def run():
            t = time.perf_counter()
            got = R.histogram(channel, a, b, bins, volume=volume)
            wall = 1e3 * (time.perf_counter() - t)
            return R.histogramMs(), wall, got
        return run

    passes = [("range_only", call(0, 0.0, 0.0, 0, False)),
              ("hist_cells_and_volume", call(0, lo, hi, args.bins, True)),
              ("hist_cells_only", call(0, lo, hi, args.bins, False)),
              ("hist_constant_field_cells_and_volume", call(const, 0.0, 1.0, args.bins, True)),
              ("hist_constant_field_cells_only", call(const, 0.0, 1.0, args.bins, False)),
              ("device_to_device_copy", copy)]
    first = {name: fn() for name, fn in passes}                   # warm-up of every pass, and the results to check
    ms = {name: [] for name, _ in passes}
    wall = {name: [] for name, _ in passes}
    for _ in range(args.reps):
        for name, fn in passes:
            k, w, got = fn()
            ms[name].append(k)
            wall[name].append(w)
            if got is not None:                                   # two calls give the same bytes
                assert got[0].tobytes() == first[name][2][0].tobytes() and got[2]["slots"] == first[name][2][2]["slots"]
    spread = first["hist_cells_and_volume"][2]
    assert int(spread[0].sum()) == spread[2]["binned"] == cells - spread[2]["nan"] - spread[2]["empty"]
    flat = first["hist_constant_field_cells_and_volume"][2]
    assert int((flat[0] > 0).sum()) == 1 and int(flat[0].sum()) == cells
    copy_ms = statistics.median(ms["device_to_device_copy"])
    for name, _ in passes:
        med = statistics.median(ms[name])
        emit(dict(what=name, bins=0 if name == "range_only" else args.bins, reps=args.reps, kernel_ms=round(med, 4),
                  kernel_min_ms=round(min(ms[name]), 4), kernel_max_ms=round(max(ms[name]), 4),
                  call_wall_ms=round(statistics.median(wall[name]), 4),
                  channel_GBps=round(nbytes / (med * 1e6), 1), time_over_copy=round(med / copy_ms, 3)))
    emit(dict(what="summary", range=[lo, hi], level_cells=levels,
              occupied_bins=int((spread[0] > 0).sum()), largest_bin_share=round(float(spread[0].max()) / cells, 4),
              constant_over_spread=round(statistics.median(ms["hist_constant_field_cells_and_volume"])
                                         / statistics.median(ms["hist_cells_and_volume"]), 3),
              volume_over_cells_only=round(statistics.median(ms["hist_cells_and_volume"])
                                           / statistics.median(ms["hist_cells_only"]), 3)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    R.close()


if __name__ == "__main__":
    main()
