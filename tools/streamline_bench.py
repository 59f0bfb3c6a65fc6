#!/usr/bin/env python3
"""Cost of exa_hip_streamlines on the bench scene with three fields (scenes.config("c4_exajet", fields=3), at reduced --scale
by default): N seeds uniform in the voxel bounds, both directions, normalised.  Reports the device time of the extraction's
two kernels (exa_hip_streamlines_ms: the count pass and the emit pass integrate the same lines), the evaluations of the
result per second of that time (4 per step plus 1 per line; the kernels execute twice as many), and the mean and the
largest number of vertices per line.  The comparison is the kernel time of exa_hip_sample_points for three channels on
uniformly drawn positions with device pointers, scaled to the same number of evaluations: what the same evaluations cost
through the existing API, leaving out the host round trips a hand-written RK4 loop would add.  It is timed as
tools/sample_bench.py times it: device events around the asynchronous call (its launches only: no copy, no wait and no
read-back between them), where the streamline figure comes from the module's own events around its two kernels.  One JSON line per
measurement; --out also writes them to a file (profiles/streamline_bench.txt)."""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=0.5)
    ap.add_argument("--seeds", type=float, default=1e5)
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-points", type=float, default=5e7, help="cap of the comparison's point count (its rate is per point)")
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
              cells=int(prep.scene.totalCells), setup_s=round(time.time() - t0, 1)))

    n = int(args.seeds)
    seeds = np.random.default_rng(1).uniform(lo, hi, (n, 3)).astype(np.float32)
    kw = dict(channels=(0, 1, 2), step=args.step, max_steps=args.max_steps, forward=True, backward=True, normalize=True)
    R.extractStreamlines(seeds, **kw)                                     # warm-up, and the result to describe
    verts, offsets, seed_vertex, reasons, _ = R.readStreamlines()
    ms, wall = [], []
    for _ in range(args.reps):
        t = time.perf_counter()
        nv = R.extractStreamlines(seeds, **kw)
        wall.append(1e3 * (time.perf_counter() - t))
        ms.append(R.streamlinesMs())
        assert nv == len(verts)                                           # two calls give the same lines
    R.releaseStreamlines()
    per_line = np.diff(offsets.astype(np.int64))
    steps = int(per_line.sum()) - n                                       # vertices appended after the seeds
    evaluations = 4 * steps + n
    kernel_ms = statistics.median(ms)
    names = {1: "maxsteps", 2: "left", 3: "novalue", 4: "stagnant"}
    emit(dict(what="streamlines", seeds=n, step=args.step, max_steps=args.max_steps, reps=args.reps, vertices=int(len(verts)),
              mean_vertices_per_line=round(float(per_line.mean()), 2), max_vertices_per_line=int(per_line.max()),
              reasons={nm: int((reasons == r).sum()) for r, nm in names.items()},
              kernel_ms=round(kernel_ms, 3), kernel_min_ms=round(min(ms), 3), kernel_max_ms=round(max(ms), 3),
              call_wall_ms=round(statistics.median(wall), 3), evaluations=evaluations,
              evaluations_per_s=evaluations / (kernel_ms * 1e-3), executed_evaluations_per_s=2 * evaluations / (kernel_ms * 1e-3)))

    npts = int(min(evaluations, args.max_points))
    g = torch.Generator(device="cuda:0").manual_seed(1)
    lo_t, hi_t = torch.tensor(lo, device="cuda:0"), torch.tensor(hi, device="cuda:0")
    pts = (lo_t + torch.rand((npts, 3), generator=g, device="cuda:0") * (hi_t - lo_t)).contiguous()
    vals = torch.empty((npts, 3), dtype=torch.float32, device="cuda:0")
    status = torch.empty((npts, 3), dtype=torch.int32, device="cuda:0")
    L = binding.lib()
    ch = (binding.C.c_int32 * 3)(0, 1, 2)
    stream = torch.cuda.current_stream().cuda_stream

    def run_points():
        R._check(L.exa_hip_sample_points(R.h, binding._dev_ptr(pts), npts, ch, 3, 0, float("nan"), binding._dev_ptr(vals), None,
                                         binding._dev_ptr(status), 1, binding.C.c_void_p(stream), 1))

    run_points()                                                          # warm-up
    torch.cuda.synchronize()
    pms = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run_points()
        e1.record()
        e1.synchronize()
        pms.append(e0.elapsed_time(e1))
    points_ms = statistics.median(pms)
    points_per_s = npts / (points_ms * 1e-3)
    emit(dict(what="sample_points_3_channels", n=npts, reps=args.reps, kernel_ms=round(points_ms, 3), points_per_s=points_per_s,
              valid_fraction=round((status[:, 0] >= 0).float().mean().item(), 4),
              ms_for_the_streamlines_evaluations=round(evaluations / points_per_s * 1e3, 3)))
    emit(dict(what="summary", streamline_evaluations_per_s=evaluations / (kernel_ms * 1e-3), points_per_s=points_per_s,
              ratio=round(evaluations / (kernel_ms * 1e-3) / points_per_s, 3),
              executed_ratio=round(2 * evaluations / (kernel_ms * 1e-3) / points_per_s, 3)))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
