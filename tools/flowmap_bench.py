#!/usr/bin/env python3
"""Cost of exa_hip_flowmap on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): a 128^3 lattice over the
voxel bounds and a 256 x 256 x 1 lattice on the plane through the centre of the volume, forward and backward, with both values
of the option flowmap_patch (0 = a wave takes 64 points along x, 1 = a 4 x 4 x 4 patch; 8 x 8 x 1 on the plane).  The step is
half a voxel divided by the largest speed on a 32^3 lattice, so a step moves at most half a voxel per axis; 32 steps.  Per case
the device time of the two stages (exa_hip_flowmap_ms: integrate, stretch), median of 7 calls with the smallest and the largest
(the run-to-run spread), the end reasons and the device bytes.  For comparison, on the same tree, exa_hip_streamlines seeded at
the same points with the same step and maxSteps, one direction: its kernel time (two passes, count and emit) and the device
bytes of its result.  Within a repetition the two patch shapes and the streamlines alternate.  One JSON line per measurement; --out also writes them to a file (profiles/flowmap_bench.txt)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from owlexabrick_amd import binding, scenes  # noqa: E402

NAMES = {1: "maxsteps", 2: "left", 3: "novalue", 4: "stagnant"}


def grid_positions(lo, hi, dims):
    """the positions of exa_hip_resample's lattice, x fastest, in the float32 operations of the kernel"""
    f = np.float32
    lo, hi = np.asarray(lo, f), np.asarray(hi, f)
    axes = [lo[k] + (np.arange(dims[k], dtype=f) + f(0.5)) * ((hi[k] - lo[k]) / f(dims[k])) for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(f)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--num-steps", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
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
    lo, hi = (np.asarray(b, np.float64) for b in prep.voxel_bounds())
    mid = 0.5 * (lo + hi)
    speed = np.sqrt(sum(np.nan_to_num(R.resample(lo, hi, (32, 32, 32), channel=c)).astype(np.float64) ** 2 for c in range(3)))
    step = float(np.float32(0.5 / speed.max()))
    emit(dict(config=args.config, scale=args.scale, fields=3, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], largest_speed=float(speed.max()),
              step=step, num_steps=args.num_steps, setup_s=round(time.time() - t0, 1)))

    thin = 0.5 * (hi[2] - lo[2]) / 128                          # the plane: one layer of the 128^3 lattice's thickness
    lattices = [("128x128x128", lo, hi, (128, 128, 128)),
                ("256x256x1", np.array([lo[0], lo[1], mid[2] - thin]), np.array([hi[0], hi[1], mid[2] + thin]), (256, 256, 1))]
    for name, l, h, dims in lattices:
        n = dims[0] * dims[1] * dims[2]
        seeds = grid_positions(l, h, dims)
        for backward in (False, True):
            kw = dict(channels=(0, 1, 2), step=step, max_steps=args.num_steps, forward=not backward, backward=backward)
            # warm-up, and the results to describe
            res = {}
            for patch in (1, 0):
                R.setOption("flowmap_patch", patch)
                res[patch] = R.flowmap(l, h, dims, (0, 1, 2), step, args.num_steps, backward)
            assert all(np.array_equal(res[0][k].view(np.uint32), res[1][k].view(np.uint32)) for k in ("end", "steps", "reasons", "stretch"))
            nv = R.extractStreamlines(seeds, **kw)
            # the three alternate within a repetition, so that what else runs on the machine meets all of them alike
            integrate, stretch, stream = {1: [], 0: []}, {1: [], 0: []}, []
            for _ in range(args.reps):
                for patch in (1, 0):                            # the default first
                    R.setOption("flowmap_patch", patch)
                    again = R.flowmap(l, h, dims, (0, 1, 2), step, args.num_steps, backward)
                    ms = R.flowmapMs()
                    integrate[patch].append(ms[0])
                    stretch[patch].append(ms[1])
                    assert np.array_equal(again["end"].view(np.uint32), res[patch]["end"].view(np.uint32))      # two calls: the same bytes
                assert R.extractStreamlines(seeds, **kw) == nv
                stream.append(R.streamlinesMs())
            R.releaseStreamlines()
            R.setOption("flowmap_patch", 1)
            r = res[1]
            for patch in (1, 0):
                emit(dict(what="flowmap", lattice=name, backward=backward, flowmap_patch=patch, reps=args.reps,
                          integrate_ms=round(statistics.median(integrate[patch]), 3), integrate_min_ms=round(min(integrate[patch]), 3),
                          integrate_max_ms=round(max(integrate[patch]), 3), stretch_ms=round(statistics.median(stretch[patch]), 3),
                          stretch_min_ms=round(min(stretch[patch]), 3), stretch_max_ms=round(max(stretch[patch]), 3),
                          steps_taken=int(r["steps"].astype(np.int64).sum()), points_with_stretch=int(np.isfinite(r["stretch"]).sum()),
                          reasons={nm: int((r["reasons"] == k).sum()) for k, nm in NAMES.items()},
                          device_bytes_with_device_pointers=24 * n))
            # the same lines through exa_hip_streamlines: one seed per lattice point, one direction
            stream_ms = statistics.median(stream)
            stream_bytes = 12 * nv + 40 * n                                     # vertices; offsets, seedVertex, reasons, counts; the seeds
            emit(dict(what="streamlines_at_the_lattice_points", lattice=name, backward=backward, seeds=n, vertices=int(nv),
                      reps=args.reps, kernel_ms=round(stream_ms, 3), kernel_min_ms=round(min(stream), 3), kernel_max_ms=round(max(stream), 3),
                      device_bytes=int(stream_bytes)))
            for patch in (1, 0):
                med = statistics.median(integrate[patch])
                emit(dict(what="summary", lattice=name, backward=backward, flowmap_patch=patch, integrate_ms=round(med, 3),
                          streamlines_kernel_ms=round(stream_ms, 3), streamlines_over_integrate_time=round(stream_ms / med, 2),
                          # beyond the spread: the slowest integrate call against the fastest streamlines call
                          integrate_no_slower_beyond_spread=bool(max(integrate[patch]) <= min(stream)),
                          flowmap_device_bytes=24 * n, streamlines_device_bytes=int(stream_bytes),
                          streamlines_over_flowmap_bytes=round(stream_bytes / (24 * n), 2)))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
