#!/usr/bin/env python3
"""Cost of exa_hip_resample_derived on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): the kernel
time (exa_hip_derived_ms; median, minimum and maximum over --reps calls) of the Q-criterion and of the vorticity on a
--size^3 lattice over the voxel bounds, into a device array.

The reference is the existing points kernel on the same positions: exa_hip_sample_points with the three channels and the
normalized gradient, device pointers, timed as tools/sample_bench.py times it (device events around the asynchronous call:
its launches only).  It does the same sums per point and stores 12 floats and 3 status words where the derived grid kernel
stores 1 or 3 floats, and descends the tree lane by lane.  The reference is measured five times over (each the median of --reps
calls) to show its run-to-run spread, against which the ratio derived / reference is to be read.  One JSON line per
measurement; --out also writes them to a file (profiles/derived_bench.txt)."""
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

C = binding.C
DEV = "cuda:0"


def lattice_positions(lo, hi, n):
    """the positions of exa_hip_resample's lattice in its float32 operations, x fastest, [n^3, 3] on the device"""
    axes = []
    for k in range(3):
        l, h = torch.tensor(float(lo[k]), dtype=torch.float32, device=DEV), torch.tensor(float(hi[k]), dtype=torch.float32, device=DEV)
        axes.append(l + (torch.arange(n, dtype=torch.float32, device=DEV) + 0.5) * ((h - l) / float(n)))
    z, y, x = torch.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], dim=1).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    t0 = time.time()
    scene = scenes.config(args.config, scale=args.scale, threads=args.threads, fields=3)
    prep = binding.Prep(scene, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    lo, hi = prep.voxel_bounds()
    emit(dict(config=args.config, scale=args.scale, fields=3, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], setup_s=round(time.time() - t0, 1)))
    L = binding.lib()
    S = args.size
    n = S ** 3
    stream = torch.cuda.current_stream().cuda_stream

    # the reference: the points kernel, three channels, normalized gradient
    pts = lattice_positions(lo, hi, S)
    vals = torch.empty((n, 3), dtype=torch.float32, device=DEV)
    grads = torch.empty((n, 3, 3), dtype=torch.float32, device=DEV)
    status = torch.empty((n, 3), dtype=torch.int32, device=DEV)
    ch = (C.c_int32 * 3)(0, 1, 2)
    flags = binding.SAMPLE_GRADIENT | binding.SAMPLE_GRADIENT_NORMALIZED

    def points():
        R._check(L.exa_hip_sample_points(R.h, binding._dev_ptr(pts), n, ch, 3, flags, float("nan"), binding._dev_ptr(vals),
                                         binding._dev_ptr(grads), binding._dev_ptr(status), 1, C.c_void_p(stream), 1))

    points()                                                                # warm-up
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        ms = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            points()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        runs.append(statistics.median(ms))
    ref_ms = statistics.median(runs)
    spread = (max(runs) - min(runs)) / ref_ms
    valid = int((status >= 0).all(dim=1).sum().item())
    emit(dict(what="points_kernel_reference", n=n, channels=3, gradient="normalized", reps=args.reps,
              runs_ms=[round(r, 3) for r in runs], kernel_ms=round(ref_ms, 3), spread=round(spread, 4), valid_points=valid,
              points_per_s=n / (ref_ms * 1e-3)))
    # the two quantities composed from the reference's gradients, one rounded float32 operation per torch operation
    g = grads
    d = (g[:, 0, 0] * g[:, 0, 0] + g[:, 1, 1] * g[:, 1, 1]) + g[:, 2, 2] * g[:, 2, 2]
    o = (g[:, 0, 1] * g[:, 1, 0] + g[:, 0, 2] * g[:, 2, 0]) + g[:, 1, 2] * g[:, 2, 1]
    want = {"q": -0.5 * d - o,
            "vorticity": torch.stack([g[:, 2, 1] - g[:, 1, 2], g[:, 0, 2] - g[:, 2, 0], g[:, 1, 0] - g[:, 0, 1]], dim=1)}
    del pts, vals, grads, g, status

    for name in ("q", "vorticity"):
        comps = 3 if name == "vorticity" else 1
        out = torch.empty((n, comps), dtype=torch.float32, device=DEV)

        def run():
            R.resampleDerived(lo, hi, (S, S, S), name, fill=float("nan"), out_ptr=out, stream=stream)
            return R.derivedMs()

        run()                                                               # warm-up
        ms, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            ms.append(run())
            wall.append(1e3 * (time.perf_counter() - t))
        kernel_ms = statistics.median(ms)
        ref = want[name].reshape(n, comps)                              # composed from the reference's output (NaN: no value)
        same = bool(((out == ref) | (out.isnan() & ref.isnan())).all().item())
        emit(dict(what="resample_derived_" + name, size=S, n=n, components=comps, reps=args.reps, kernel_ms=round(kernel_ms, 3),
                  kernel_min_ms=round(min(ms), 3), kernel_max_ms=round(max(ms), 3), call_wall_ms=round(statistics.median(wall), 3),
                  points_per_s=n / (kernel_ms * 1e-3), over_reference=round(kernel_ms / ref_ms, 3), reference_spread=round(spread, 4),
                  within_the_spread=bool(kernel_ms <= ref_ms * (1.0 + spread)), equals_the_reference_composed=same))
        del out
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
