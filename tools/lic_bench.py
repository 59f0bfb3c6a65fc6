#!/usr/bin/env python3
"""Cost of exa_hip_lic on the bench scene with three fields (scenes.config("c4_exajet", fields=3)): a 1024^2 and a 2048^2
image on a plane through the centre of the volume, axis-aligned (z = centre, the image covers the x-y extent) and oblique,
step 0.5 pixels, half length 20, median of 7 calls.  Per image the device time of the call's kernels (exa_hip_lic_ms) and the
counted samples per second of that time, sum(count) / time — in every lane layout: options lic_lanes (a lane per pixel, or a
lane per pixel and direction) and lic_patch (a wave's pixels in a row, or in a patch 8 pixels wide); the first line of an image
is the default layout.  For comparison, on the same tree, exa_hip_streamlines with both directions, normalised, seeded at the
pixel centres of the 1024^2 axis-aligned image with the same number of steps of the same length in voxels: its kernel time
(two passes, count and emit) and the device bytes of its result, against the LIC call's.  One JSON line per measurement; --out
also writes them to a file (profiles/lic_bench.txt)."""
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

LAYOUTS = [(1, 1), (1, 0), (2, 1), (2, 0)]                      # (lic_lanes, lic_patch); the first is the default
NAMES = {1: "maxsteps", 2: "left", 3: "novalue", 4: "stagnant", 5: "image"}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--sizes", default="1024,2048")
    ap.add_argument("--step", type=float, default=0.5)
    ap.add_argument("--half-length", type=int, default=20)
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
    ext, mid = hi - lo, 0.5 * (lo + hi)
    emit(dict(config=args.config, scale=args.scale, fields=3, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], setup_s=round(time.time() - t0, 1)))

    def planes(n):
        """(name, plane): the image's centre is the volume's"""
        du, dv = np.array([ext[0] / n, 0, 0]), np.array([0, ext[1] / n, 0])
        yield "axis_aligned", (mid - 0.5 * n * (du + dv), du, dv, (n, n))
        du, dv = np.array([0.8 * ext[0], 0.1 * ext[1], 0.25 * ext[2]]) / n, np.array([-0.1 * ext[0], 0.7 * ext[1], 0.5 * ext[2]]) / n
        yield "oblique", (mid - 0.5 * n * (du + dv), du, dv, (n, n))

    lic_ms_1024 = None
    for n in (int(s) for s in args.sizes.split(",")):
        for name, pl in planes(n):
            for lanes, patch in LAYOUTS:
                R.setOption("lic_lanes", lanes)
                R.setOption("lic_patch", patch)
                res = R.lic(pl, (0, 1, 2), args.step, args.half_length)     # warm-up, and the result to describe
                ms = []
                for _ in range(args.reps):
                    again = R.lic(pl, (0, 1, 2), args.step, args.half_length)
                    ms.append(R.licMs())
                    assert np.array_equal(again["sum"], res["sum"])          # two calls give the same bytes
                kernel_ms = statistics.median(ms)
                samples = int(res["count"].astype(np.int64).sum())
                emit(dict(what="lic", plane=name, size=n, step=args.step, half_length=args.half_length, lic_lanes=lanes,
                          lic_patch=patch, reps=args.reps, kernel_ms=round(kernel_ms, 3), kernel_min_ms=round(min(ms), 3),
                          kernel_max_ms=round(max(ms), 3), samples=samples, samples_per_s=samples / (kernel_ms * 1e-3),
                          pixels_covered=int((res["count"] > 0).sum()),
                          reasons={nm: int((res["reasons"] == r).sum()) for r, nm in NAMES.items()},
                          device_bytes_with_device_pointers=24 * n * n))
                if n == 1024 and name == "axis_aligned" and (lanes, patch) == LAYOUTS[0]:
                    lic_ms_1024 = kernel_ms
    R.setOption("lic_lanes", LAYOUTS[0][0])
    R.setOption("lic_patch", LAYOUTS[0][1])

    # the same lines through exa_hip_streamlines: one seed per pixel centre of the 1024^2 axis-aligned image
    if lic_ms_1024 is not None:
        n = 1024
        _, (origin, du, dv, _) = next(planes(n))
        jj, ii = np.meshgrid(np.arange(n) + 0.5, np.arange(n) + 0.5, indexing="ij")
        seeds = (origin[None, :] + ii.reshape(-1, 1) * du[None, :] + jj.reshape(-1, 1) * dv[None, :]).astype(np.float32)
        kw = dict(channels=(0, 1, 2), step=args.step * float(np.linalg.norm(du)), max_steps=args.half_length, forward=True,
                  backward=True, normalize=True)
        nv = R.extractStreamlines(seeds, **kw)
        ms = []
        for _ in range(args.reps):
            assert R.extractStreamlines(seeds, **kw) == nv
            ms.append(R.streamlinesMs())
        R.releaseStreamlines()
        stream_ms = statistics.median(ms)
        stream_bytes = 12 * nv + 40 * len(seeds)                               # vertices; offsets, seedVertex, reasons, counts; the seeds
        emit(dict(what="streamlines_at_the_pixel_centres", size=n, seeds=len(seeds), step_voxels=kw["step"], max_steps=args.half_length,
                  reps=args.reps, vertices=int(nv), kernel_ms=round(stream_ms, 3), kernel_min_ms=round(min(ms), 3),
                  kernel_max_ms=round(max(ms), 3), device_bytes=int(stream_bytes)))
        emit(dict(what="summary", size=n, lic_kernel_ms=round(lic_ms_1024, 3), streamlines_kernel_ms=round(stream_ms, 3),
                  streamlines_over_lic_time=round(stream_ms / lic_ms_1024, 2), lic_device_bytes=24 * n * n,
                  streamlines_device_bytes=int(stream_bytes), streamlines_over_lic_bytes=round(stream_bytes / (24 * n * n), 2)))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
