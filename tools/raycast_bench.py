#!/usr/bin/env python3
"""Cost of exa_hip_raycast_iso on the bench scene (scenes.config("c4_exajet")): the rays of tools/project_bench.py — a 1024^2
orthographic image along z over the voxel bounds and a 1024^2 perspective image with the default bench camera, at a dt of one
finest cell, unit directions, device outputs — cast for the first crossing of --iso (default: the middle of channel 0's value
range).  Per image: the device time of the call's kernel (exa_hip_raycast_iso_ms; median, minimum and maximum over --reps
calls behind one warm-up call) with all seven outputs and without the `crossings` array (a ray may then stop at its first
crossing), at refine 0, 8 and 24; and exa_hip_project on the same ExaHipRays in the same process, timed before and after the
casts, with the ratio of each cast to the mean of the two.  samples/s: the valid samples of the whole rays (the projection's
count, summed) over the kernel time — for the casts without `crossings` an effective rate, they evaluate fewer.  With --world
the perspective image also runs through the world-space path (identity transform), which marches every index.

A report, not a gate.  One JSON line per measurement; --out also writes them to a file (profiles/raycast_bench.txt)."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from owlexabrick_amd import binding, harness, scenes  # noqa: E402
from project_bench import DEV, rays_struct  # noqa: E402

C = binding.C
REFINES = (0, 8, 24)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dt", type=float, default=1.0, help="in finest cells")
    ap.add_argument("--iso", type=float, default=None, help="default: the middle of channel 0's value range")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--world", action="store_true", help="also the perspective image through the world-space path")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=None, help="also write the JSON lines to this file")
    args = ap.parse_args()
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    t0 = time.time()
    scene = scenes.config(args.config, scale=args.scale, threads=args.threads)
    prep = binding.Prep(scene, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    R._push_state()                                                     # the identity transform, for --world
    lo, hi = prep.voxel_bounds()
    stats = R.fieldStats(0)
    iso = float(np.float32(0.5 * (stats["min"] + stats["max"]) if args.iso is None else args.iso))
    emit(dict(config=args.config, scale=args.scale, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], value_range=[float(stats["min"]), float(stats["max"])],
              iso=iso, setup_s=round(time.time() - t0, 1)))
    L = binding.lib()
    S = args.size
    ext = (hi - lo).astype(np.float64)
    stream = torch.cuda.current_stream().cuda_stream

    cam = harness.default_camera(lo, hi, S, S)
    far = max(float(np.linalg.norm(cam["pos"] - np.array(c))) for c in
              [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    cases = [("orthographic", rays_struct(lo, (0, 0, 1), (S, S), 0.0, args.dt, math.ceil(ext[2] / args.dt),
                                          orgDu=(ext[0] / S, 0, 0), orgDv=(0, ext[1] / S, 0)), 0),
             ("perspective", rays_struct(cam["pos"], cam["dir00"], (S, S), 0.0, args.dt, math.ceil(far / args.dt),
                                         dirDu=cam["dirDu"], dirDv=cam["dirDv"]), 0)]
    if args.world:
        cases.append(("perspective_world_space", cases[1][1], binding.SAMPLE_WORLD_SPACE))

    f32, i32 = torch.float32, torch.int32
    prj = dict(sum=torch.empty((S, S), dtype=torch.float64, device=DEV), count=torch.empty((S, S), dtype=i32, device=DEV),
               max=torch.empty((S, S), dtype=f32, device=DEV), min=torch.empty((S, S), dtype=f32, device=DEV),
               max_index=torch.empty((S, S), dtype=i32, device=DEV))
    hit = dict(t=torch.empty((S, S), dtype=f32, device=DEV), position=torch.empty((S, S, 3), dtype=f32, device=DEV),
               value=torch.empty((S, S), dtype=f32, device=DEV), gradient=torch.empty((S, S, 3), dtype=f32, device=DEV),
               index=torch.empty((S, S), dtype=i32, device=DEV), side=torch.empty((S, S), dtype=i32, device=DEV),
               crossings=torch.empty((S, S), dtype=i32, device=DEV))

    def timed(run):
        """(median, min, max) of the call's kernel ms over --reps calls behind one warm-up call"""
        run()
        ms = [run() for _ in range(args.reps)]
        return statistics.median(ms), min(ms), max(ms)

    for name, s, space in cases:
        flags = binding.PROJECT_NORMALIZE | space
        n = s.numSamples

        def project():
            R._check(L.exa_hip_project(R.h, C.byref(s), 0, flags, *[C.c_void_p(prj[k].data_ptr()) for k in prj], 1, C.c_void_p(stream)))
            return R.projectMs()

        def cast(refine, counts):
            ptrs = [C.c_void_p(hit[k].data_ptr()) if counts or k != "crossings" else None for k in binding.RAYCAST_KEYS]
            R._check(L.exa_hip_raycast_iso(R.h, C.byref(s), 0, iso, refine, flags, float("nan"), *ptrs, 1, C.c_void_p(stream)))
            return R.raycastIsoMs()

        before = timed(project)
        valid = int(prj["count"].to(torch.int64).sum().item())
        recs = []
        for counts in (True, False):
            for refine in REFINES:
                med, lo_ms, hi_ms = timed(lambda: cast(refine, counts))
                recs.append(dict(what=name, size=S, dt=args.dt, num_samples=n, iso=iso, refine=refine, crossings_array=counts, reps=args.reps,
                                 kernel_ms=round(med, 3), kernel_min_ms=round(lo_ms, 3), kernel_max_ms=round(hi_ms, 3),
                                 ray_valid_samples=valid, ray_valid_samples_per_s=valid / (med * 1e-3),
                                 pixels_hit=int((hit["index"] >= 0).sum().item())))
                if counts:
                    recs[-1]["crossings_total"] = int(hit["crossings"].to(torch.int64).sum().item())
        after = timed(project)
        mean = 0.5 * (before[0] + after[0])
        emit(dict(what=name + "_project", size=S, dt=args.dt, num_samples=n, reps=args.reps, kernel_ms_before=round(before[0], 3),
                  kernel_min_ms_before=round(before[1], 3), kernel_max_ms_before=round(before[2], 3), kernel_ms_after=round(after[0], 3),
                  kernel_min_ms_after=round(after[1], 3), kernel_max_ms_after=round(after[2], 3), valid_samples=valid,
                  valid_samples_per_s=valid / (mean * 1e-3), pixels_hit=int((prj["count"] > 0).sum().item())))
        for rec in recs:
            rec["raycast_over_project"] = round(rec["kernel_ms"] / mean, 3)
            emit(rec)
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
