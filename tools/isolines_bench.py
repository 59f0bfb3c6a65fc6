#!/usr/bin/env python3
"""Cost of exa_hip_isolines on the bench scene (scenes.config("c4_exajet")): a plane lattice of --size^2 points through the
centre of the voxel bounds, once axis-aligned (z = centre, u along x, v along y) and once oblique, at 1 level (0.5) and at 16
levels (0.05 .. 0.95).  After a warm-up call, --reps calls are timed: device ms per stage summed over the levels (positions
and values, square pass, point pass, scans, emit, gradients — the module's own events around each stage) and the wall time of
the whole call (allocations included); median, and spread = (max - min) / median.

The yardstick, in the same run: exa_hip_sample_points on the same positions (one channel, device pointers, device events
around the asynchronous call, as tools/sample_bench.py times it).  The first stage is that kernel plus the positions kernel;
the contouring stages behind it read each 4-byte value a small number of times per level.  One JSON line per measurement;
--out also writes them to a file (profiles/isolines_bench.txt)."""
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
STAGES = ["positions_and_values", "square_pass", "point_pass", "scans", "emit", "gradients"]


def lattice_positions(origin, du, dv, n):
    """the positions of exa_hip_isolines' lattice in its float32 operations, i fastest, [n^2, 3] on the device"""
    o, u, v = (torch.tensor(np.asarray(x, np.float32), device=DEV) for x in (origin, du, dv))
    f = torch.arange(n, dtype=torch.float32, device=DEV) + 0.5
    return ((o[None, None, :] + f[None, :, None] * u[None, None, :]) + f[:, None, None] * v[None, None, :]).reshape(-1, 3).contiguous()


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--size", type=int, default=2048)
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

    t0 = time.time()
    scene = scenes.config(args.config, scale=args.scale, threads=args.threads)
    prep = binding.Prep(scene, num_threads=args.threads)
    R = binding.Renderer(prep, device=0)
    lo, hi = (np.asarray(b, np.float64) for b in prep.voxel_bounds())
    emit(dict(config=args.config, scale=args.scale, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], setup_s=round(time.time() - t0, 1)))
    L = binding.lib()
    S = args.size
    n = S * S
    ext, centre = hi - lo, 0.5 * (lo + hi)
    stream = torch.cuda.current_stream().cuda_stream
    planes = {}
    du, dv = np.array([ext[0] / S, 0, 0]), np.array([0, ext[1] / S, 0])
    planes["axis_aligned"] = (np.array([lo[0], lo[1], np.floor(centre[2]) + 0.5]), du, dv)
    du, dv = np.array([0.75, 0.2, 0.15]) * ext[0] / S, np.array([-0.1, 0.8, 0.35]) * ext[1] / S
    planes["oblique"] = (centre - 0.5 * S * du - 0.5 * S * dv, du, dv)
    level_sets = {1: [0.5], 16: [float(x) for x in np.linspace(0.05, 0.95, 16, dtype=np.float32)]}

    for pname, plane in planes.items():
        plane = tuple(np.asarray(x, np.float32) for x in plane)
        pts = lattice_positions(*plane, S)
        vals = torch.empty(n, dtype=torch.float32, device=DEV)
        ch = (C.c_int32 * 1)(0)

        def points():
            R._check(L.exa_hip_sample_points(R.h, binding._dev_ptr(pts), n, ch, 1, 0, float("nan"), binding._dev_ptr(vals), None, None,
                                             1, C.c_void_p(stream), 1))

        points()                                                            # warm-up
        torch.cuda.synchronize()
        ref = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            points()
            e1.record()
            e1.synchronize()
            ref.append(e0.elapsed_time(e1))
        ref_ms, ref_spread = summary(ref)
        valid = int(torch.isfinite(vals).sum().item())
        emit(dict(what="points_kernel_reference", plane=pname, origin=plane[0].tolist(), du=plane[1].tolist(), dv=plane[2].tolist(),
                  n=n, reps=args.reps, kernel_ms=ref_ms, spread=ref_spread, valid_points=valid))
        del pts, vals

        for nlev, isos in level_sets.items():
            for grads in (False, True):
                nv, ns = R.extractIsolines(*plane, (S, S), isos, gradients=grads)       # warm-up
                stages, wall = [], []
                for _ in range(args.reps):
                    t = time.perf_counter()
                    R.extractIsolines(*plane, (S, S), isos, gradients=grads)
                    wall.append(1e3 * (time.perf_counter() - t))
                    stages.append(R.isolinesStageMs())
                R.releaseIsolines()
                ms, spread = {}, {}
                for k, name in enumerate(STAGES):
                    ms[name], spread[name] = summary([s[k] for s in stages])
                contour = [sum(s[1:5]) for s in stages]
                contour_ms, contour_spread = summary(contour)
                wall_ms, wall_spread = summary(wall)
                emit(dict(what="isolines", plane=pname, size=S, levels=nlev, gradients=grads, vertices=nv, segments=ns, reps=args.reps,
                          stage_ms=ms, stage_spread=spread, contour_stages_ms=contour_ms, contour_stages_spread=contour_spread,
                          contour_ms_per_level=round(contour_ms / nlev, 3), call_wall_ms=wall_ms, call_wall_spread=wall_spread,
                          values_over_reference=round(ms["positions_and_values"] / ref_ms, 3) if ref_ms else None,
                          contour_over_reference=round(contour_ms / ref_ms, 3) if ref_ms else None))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
