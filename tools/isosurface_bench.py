#!/usr/bin/env python3
"""Cost of exa_hip_isosurface on the bench scene (scenes.config("c4_exajet")): the iso-surface 0.5 over the voxel bounds on
lattices of 512^3 and 1024^3 points.  After a warm-up call, --reps calls are timed: device ms per stage (lattice values, cube
pass, point pass, scans, emit, gradients — the module's own events around each stage), the wall time of the whole call
(allocation of the work space included), and in the same run exa_hip_resample of the same lattice into device memory, the
yardstick: the stages behind the sampling read each 4-byte lattice value a small number of times and should cost a minor
fraction of it.  One JSON line per lattice.  Kernel times: run this under `rocprofv3 --kernel-trace --stats -- python ...`."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from owlexabrick_amd import binding, scenes  # noqa: E402

STAGES = ["lattice_values", "cube_pass", "point_pass", "scans", "emit", "gradients"]


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sizes", type=int, nargs="*", default=[512, 1024])
    ap.add_argument("--iso", type=float, default=0.5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-gradients", action="store_true")
    ap.add_argument("--threads", type=int, default=16)
    args = ap.parse_args()

    t0 = time.time()
    scene = scenes.config(args.config, scale=args.scale, threads=args.threads)
    prep = binding.Prep(scene, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    lo, hi = prep.voxel_bounds()
    print(json.dumps(dict(config=args.config, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
                          setup_s=round(time.time() - t0, 1))), flush=True)
    stream = torch.cuda.current_stream().cuda_stream
    med = lambda xs: round(statistics.median(xs), 3)             # noqa: E731

    for n in args.sizes:
        dims = (n, n, n)
        out = torch.empty(n ** 3, dtype=torch.float32, device="cuda:0")
        R.resample(lo, hi, dims, out_ptr=out, stream=stream)     # warm-up
        resample = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            R.resample(lo, hi, dims, out_ptr=out, stream=stream, async_=True)
            e1.record()
            e1.synchronize()
            resample.append(e0.elapsed_time(e1))
        del out
        torch.cuda.empty_cache()

        grads = not args.no_gradients
        nv, nt = R.extractIsoSurface(lo, hi, dims, args.iso, gradients=grads)     # warm-up
        stages, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            R.extractIsoSurface(lo, hi, dims, args.iso, gradients=grads)
            wall.append(1e3 * (time.perf_counter() - t))
            stages.append(R.isoSurfaceStageMs())
        R.releaseIsoSurface()
        ms = {name: med([s[k] for s in stages]) for k, name in enumerate(STAGES)}
        mesh_ms = ms["cube_pass"] + ms["point_pass"] + ms["scans"] + ms["emit"]
        points = n ** 3
        rec = dict(what="isosurface", n=n, iso=args.iso, vertices=nv, triangles=nt, reps=args.reps, stage_ms=ms,
                   mesh_stages_ms=round(mesh_ms, 3), call_wall_ms=med(wall), resample_ms=med(resample),
                   resample_min_ms=round(min(resample), 3), mesh_over_resample=round(mesh_ms / statistics.median(resample), 3),
                   # bytes the passes must move at the least: the cube pass reads the values (4 B) and writes a byte per
                   # point; the point pass reads values and cube bytes (5 B) and writes mask and offset (3 B)
                   cube_pass_GBps=round(5 * points / (ms["cube_pass"] * 1e6), 1) if ms["cube_pass"] else None,
                   point_pass_GBps=round(8 * points / (ms["point_pass"] * 1e6), 1) if ms["point_pass"] else None)
        print(json.dumps(rec), flush=True)
    R.close()


if __name__ == "__main__":
    main()
