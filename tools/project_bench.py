#!/usr/bin/env python3
"""Cost of exa_hip_project on the bench scene (scenes.config("c4_exajet")): a 1024^2 orthographic projection along z over the
voxel bounds and a 1024^2 perspective projection with the default bench camera, at a dt of one finest cell (voxel space is
in finest-cell units: dt = 1), unit directions, device outputs.  Reports per projection the device time of the call's
kernel (exa_hip_project_ms; median, minimum and maximum over --reps calls), the valid samples per second of that time, and
the share of the pixels x samples indices that are not marched: per ray (indices whose position lies outside the root box)
and per wave (a wave of 8 x 8 rays marches the union of its rays' ranges).  With --world the perspective projection also runs
through the world-space path (identity transform), which marches every index.

The yardstick is the existing points kernel on the same positions, handed over as a device array, pixel-major: what the
projection costs when it is emulated through exa_hip_sample_points, leaving out the host's reduction and the upload.  The
positions are formed on the device band of rows by band of rows (the array of a whole image would not fit), each band's
launches timed with device events around the asynchronous call as tools/sample_bench.py times them, the bands' times
summed; its valid samples are counted beside the projection's.  One JSON line per measurement; --out also writes
them to a file (profiles/project_bench.txt)."""
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

import torch  # noqa: E402

from owlexabrick_amd import binding, harness, scenes  # noqa: E402

C = binding.C
DEV = "cuda:0"


def rays_struct(org, dir, size, tmin, dt, n, orgDu=(0, 0, 0), orgDv=(0, 0, 0), dirDu=(0, 0, 0), dirDv=(0, 0, 0)):
    s = binding.ExaHipRays()
    for k, v in (("org", org), ("orgDu", orgDu), ("orgDv", orgDv), ("dir", dir), ("dirDu", dirDu), ("dirDv", dirDv)):
        setattr(s, k, (C.c_float * 3)(*[float(c) for c in v]))
    s.width, s.height = size
    s.tmin, s.dt, s.numSamples = float(tmin), float(dt), int(n)
    return s


def band_positions(s, y0, y1):
    """the positions of rows [y0, y1) in the contract's float32 operations, [rows, W, N, 3] on the device (unit directions)"""
    f = lambda v: torch.tensor(list(v), dtype=torch.float32, device=DEV)                      # noqa: E731
    sx = (torch.arange(s.width, dtype=torch.float32, device=DEV) + 0.5)[None, :, None]
    sy = (torch.arange(y0, y1, dtype=torch.float32, device=DEV) + 0.5)[:, None, None]
    o = (f(s.org) + sx * f(s.orgDu)) + sy * f(s.orgDv)
    d = (f(s.dir) + sx * f(s.dirDu)) + sy * f(s.dirDv)
    o, d = o.expand(y1 - y0, s.width, 3), d.expand(y1 - y0, s.width, 3)
    length = torch.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    d = d / length[..., None]
    t = s.tmin + (torch.arange(s.numSamples, dtype=torch.float32, device=DEV) + 0.5) * s.dt
    return (o[:, :, None, :] + t[None, None, :, None] * d[:, :, None, :]).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--dt", type=float, default=1.0, help="in finest cells")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--band-points", type=float, default=2 ** 26, help="positions per band of the yardstick")
    ap.add_argument("--world", action="store_true", help="also the perspective projection through the world-space path")
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
    reg = prep.regions()
    box_lo = torch.tensor(np.stack(list(reg["dom_lo"])).min(axis=0), device=DEV)
    box_hi = torch.tensor(np.stack(list(reg["dom_hi"])).max(axis=0), device=DEV)
    emit(dict(config=args.config, scale=args.scale, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], setup_s=round(time.time() - t0, 1)))
    L = binding.lib()
    S = args.size
    ext = (hi - lo).astype(np.float64)
    stream = torch.cuda.current_stream().cuda_stream
    ch = (C.c_int32 * 1)(0)

    cam = harness.default_camera(lo, hi, S, S)
    far = max(float(np.linalg.norm(cam["pos"] - np.array(c))) for c in
              [(x, y, z) for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in (lo[2], hi[2])])
    cases = [("orthographic", rays_struct(lo, (0, 0, 1), (S, S), 0.0, args.dt, math.ceil(ext[2] / args.dt),
                                          orgDu=(ext[0] / S, 0, 0), orgDv=(0, ext[1] / S, 0)), 0),
             ("perspective", rays_struct(cam["pos"], cam["dir00"], (S, S), 0.0, args.dt, math.ceil(far / args.dt),
                                         dirDu=cam["dirDu"], dirDv=cam["dirDv"]), 0)]
    if args.world:
        cases.append(("perspective_world_space", cases[1][1], binding.SAMPLE_WORLD_SPACE))

    out = dict(sum=torch.empty((S, S), dtype=torch.float64, device=DEV), count=torch.empty((S, S), dtype=torch.int32, device=DEV),
               max=torch.empty((S, S), dtype=torch.float32, device=DEV), min=torch.empty((S, S), dtype=torch.float32, device=DEV),
               max_index=torch.empty((S, S), dtype=torch.int32, device=DEV))
    ptr = lambda k: C.c_void_p(out[k].data_ptr())                       # noqa: E731
    for name, s, space in cases:
        flags = binding.PROJECT_NORMALIZE | space
        n = s.numSamples

        def run():
            R._check(L.exa_hip_project(R.h, C.byref(s), 0, flags, ptr("sum"), ptr("count"), ptr("max"), ptr("min"),
                                       ptr("max_index"), 1, C.c_void_p(stream)))
            return R.projectMs()

        run()                                                           # warm-up
        ms, wall = [], []
        for _ in range(args.reps):
            t = time.perf_counter()
            ms.append(run())
            wall.append(1e3 * (time.perf_counter() - t))
        kernel_ms = statistics.median(ms)
        valid = int(out["count"].to(torch.int64).sum().item())
        rec = dict(what=name, size=S, dt=args.dt, num_samples=n, indices=S * S * n, reps=args.reps, kernel_ms=round(kernel_ms, 3),
                   kernel_min_ms=round(min(ms), 3), kernel_max_ms=round(max(ms), 3), call_wall_ms=round(statistics.median(wall), 3),
                   valid_samples=valid, valid_samples_per_s=valid / (kernel_ms * 1e-3),
                   pixels_hit=int((out["count"] > 0).sum().item()))
        if space:
            emit(rec)
            continue
        # the yardstick, and on the same positions the indices a ray / a wave does not march
        rows = max(8, int(args.band_points // (S * n)) // 8 * 8)
        points_ms, points_valid, ray_in, wave_marched = 0.0, 0, 0, 0
        for y0 in range(0, S, rows):
            y1 = min(S, y0 + rows)
            pts = band_positions(s, y0, y1)
            m = pts.numel() // 3
            vals = torch.empty((m, 1), dtype=torch.float32, device=DEV)
            status = torch.empty((m, 1), dtype=torch.int32, device=DEV)

            def points():
                R._check(L.exa_hip_sample_points(R.h, binding._dev_ptr(pts), m, ch, 1, 0, float("nan"), binding._dev_ptr(vals), None,
                                                 binding._dev_ptr(status), 1, C.c_void_p(stream), 1))

            points()                                                    # warm-up
            torch.cuda.synchronize()
            band = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                points()
                e1.record()
                e1.synchronize()
                band.append(e0.elapsed_time(e1))
            points_ms += statistics.median(band)
            points_valid += int((status >= 0).sum().item())
            inside = ((pts >= box_lo) & (pts <= box_hi)).all(dim=3)                            # [rows, W, N]
            ray_in += int(inside.sum().item())
            r8, w8 = (y1 - y0 + 7) // 8 * 8, (S + 7) // 8 * 8
            pad = torch.zeros((r8, w8, n), dtype=torch.bool, device=DEV)
            pad[:y1 - y0, :S] = inside
            patch = pad.view(r8 // 8, 8, w8 // 8, 8, n).any(dim=3).any(dim=1)                  # [patches y, patches x, N]
            idx = torch.arange(n, device=DEV)
            first = torch.where(patch, idx, n).amin(dim=2)
            last = torch.where(patch, idx, -1).amax(dim=2)
            wave_marched += int(((last - first + 1).clamp(min=0) * 64).sum().item())
            del pts, vals, status, inside, pad, patch
        total = S * S * n
        rec.update(indices_skipped_per_ray=round(1 - ray_in / total, 4), indices_skipped_per_wave=round(1 - wave_marched / total, 4))
        emit(rec)
        emit(dict(what=name + "_points_kernel_yardstick", n=total, bands=math.ceil(S / rows), reps=args.reps, kernel_ms=round(points_ms, 3),
                  valid_samples=points_valid, valid_samples_equal_the_projections=points_valid == valid, points_per_s=total / (points_ms * 1e-3),
                  project_over_points=round(kernel_ms / points_ms, 3)))
    emit(dict(what="leaf_reuse_across_steps", built=False,
              note="the optional reuse of the previous step's kd leaf was not built: no A/B was run, the kernel descends at every index"))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
