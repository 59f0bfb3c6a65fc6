#!/usr/bin/env python3
"""Throughput of the point probes on the bench scene (scenes.config("c4_exajet")): exa_hip_resample over the voxel bounds at
512^3 and 1024^3 and exa_hip_sample_points at 1e8 uniform random points, everything in device memory.  Each measurement is
warmed up once, then timed with device events over --reps calls; one JSON line per measurement (ms per call, points/s).
With --ab the grid kernel runs in every patch shape (option sample_patch) with and without its wave-uniform path
(sample_uniform) in the same process.  Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from owlexabrick_amd import binding, scenes  # noqa: E402

SHAPES = ["64x1x1", "16x4x1", "8x8x1", "4x4x4"]


def timed(fn, reps):
    fn()                                                          # warm-up
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--points", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ab", action="store_true", help="every patch shape, with and without the wave-uniform path")
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()

    t0 = time.time()
    scene = scenes.config(args.config, threads=args.threads)
    prep = binding.Prep(scene, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    lo, hi = prep.voxel_bounds()
    print(json.dumps(dict(config=args.config, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
                          setup_s=round(time.time() - t0, 1))), flush=True)
    stream = torch.cuda.current_stream().cuda_stream

    out = torch.empty(max(args.sizes) ** 3, dtype=torch.float32, device="cuda:0")
    variants = [(s, u) for s in range(len(SHAPES)) for u in (1, 0)] if args.ab else [(None, None)]
    for n in args.sizes:
        for shape, uniform in variants:
            if shape is not None:
                R.setOption("sample_patch", shape)
                R.setOption("sample_uniform", uniform)
            ms = timed(lambda: R.resample(lo, hi, (n, n, n), out_ptr=out, stream=stream, async_=True), args.reps)
            rec = dict(what="resample", n=n, ms=round(ms, 3), points_per_s=n ** 3 / (ms * 1e-3))
            if shape is not None:
                rec.update(patch=SHAPES[shape], uniform=uniform)
            print(json.dumps(rec), flush=True)
        valid = torch.isfinite(out[:n ** 3]).float().mean().item()
        print(json.dumps(dict(what="resample_valid_fraction", n=n, fraction=round(valid, 4))), flush=True)
    del out
    torch.cuda.empty_cache()

    npts = int(args.points)
    g = torch.Generator(device="cuda:0").manual_seed(1)
    lo_t, hi_t = torch.tensor(lo, device="cuda:0"), torch.tensor(hi, device="cuda:0")
    pts = (lo_t + torch.rand((npts, 3), generator=g, device="cuda:0") * (hi_t - lo_t)).contiguous()
    vals = torch.empty((npts, 1), dtype=torch.float32, device="cuda:0")
    status = torch.empty((npts, 1), dtype=torch.int32, device="cuda:0")
    L = binding.lib()
    ch = (binding.C.c_int32 * 1)(0)

    def run_points(flags, grads=None):
        R._check(L.exa_hip_sample_points(R.h, binding._dev_ptr(pts), npts, ch, 1, flags, float("nan"), binding._dev_ptr(vals),
                                         binding._dev_ptr(grads), binding._dev_ptr(status), 1, binding.C.c_void_p(stream), 1))

    ms = timed(lambda: run_points(0), args.reps)
    print(json.dumps(dict(what="sample_points", n=npts, ms=round(ms, 3), points_per_s=npts / (ms * 1e-3),
                          valid_fraction=round((status >= 0).float().mean().item(), 4))), flush=True)
    grads = torch.empty((npts, 1, 3), dtype=torch.float32, device="cuda:0")
    ms = timed(lambda: run_points(binding.SAMPLE_GRADIENT, grads), args.reps)
    print(json.dumps(dict(what="sample_points_gradient", n=npts, ms=round(ms, 3), points_per_s=npts / (ms * 1e-3))), flush=True)
    R.close()


if __name__ == "__main__":
    main()
