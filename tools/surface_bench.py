#!/usr/bin/env python3
"""Cost of exa_hip_sample_triangles on the bench scene (scenes.config("c4_exajet")), on the mesh an extraction left on the
device (EXA_SURFACE_FROM_ISOSURFACE, device outputs, channel 0):
  (a) the iso-0.5 surface of a 256^3 lattice over the voxel bounds, at a spacing of one finest cell (voxel space is in
      finest-cell units: spacing = 1): n mostly 1 - 2;
  (b) the same surface from a 32^3 lattice at the same spacing: large n;
  (c) the mesh of (b) with spacing = 0, maxN = 64: 4096 samples per triangle;
  (d) the mesh of (a) at a spacing of one cell of its lattice (the longest voxel extent / 256): n mostly 1 - 2, the iso mesh
      on a lattice as fine as the data, which is what surface_pack is for.
Per case and for surface_pack 1 and 0: the device time of the call's kernels (exa_hip_sample_triangles_ms; median, minimum and
maximum over --reps calls), the samples per second of that time, and the histogram of n.

The yardstick is the existing points kernel on the very positions of the samples, handed over as a device array, triangle by
triangle within each n: what the call costs when it is emulated through exa_hip_sample_points, leaving out the reduction.  The
positions are formed on the device in bands (timed with device events around the asynchronous call as tools/project_bench.py
times them, the bands' times summed); its valid samples are counted beside the call's.  One JSON line per measurement; --out
also writes them to a file (profiles/surface_bench.txt)."""
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


def barycentrics(n):
    """(b1, b2) float32 [n*n] of the contract (include/exa_hip.h)"""
    f32 = np.float32
    k = np.arange(n * n)
    a, b = k // n, k % n
    up = a + b < n
    t = np.where(up, f32(1) / f32(3), f32(2) / f32(3)).astype(f32)
    fa, fb = np.where(up, a, n - 1 - a).astype(f32) + t, np.where(up, b, n - 1 - b).astype(f32) + t
    return fa / f32(n), fb / f32(n)


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--config", default="c4_exajet")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--iso", type=float, default=0.5)
    ap.add_argument("--fine", type=int, default=256, help="lattice of case (a)")
    ap.add_argument("--coarse", type=int, default=32, help="lattice of cases (b) and (c)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--band-points", type=float, default=2 ** 25, help="positions per band of the yardstick")
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
    lo, hi = prep.voxel_bounds()
    emit(dict(config=args.config, scale=args.scale, regions=int(prep.scene.numRegions), bricks=int(prep.scene.numBricks),
              cells=int(prep.scene.totalCells), voxel_bounds=[lo.tolist(), hi.tolist()], setup_s=round(time.time() - t0, 1)))
    L = binding.lib()
    stream = torch.cuda.current_stream().cuda_stream
    ch = (C.c_int32 * 1)(0)

    for name, lattice, spacing, max_n in (("a_fine_lattice", args.fine, 1.0, 64), ("b_coarse_lattice", args.coarse, 1.0, 64),
                                          ("c_coarse_lattice_max_n", args.coarse, 0.0, 64),
                                          ("d_fine_lattice_cell_spacing", args.fine, float((hi - lo).max()) / args.fine, 64)):
        nv, nt = R.extractIsoSurface(lo, hi, (lattice,) * 3, args.iso)
        if nt == 0:
            emit(dict(what=name, lattice=lattice, triangles=0, note="no surface at this iso value"))
            continue
        out = dict(sum=torch.empty((nt, 1), dtype=torch.float64, device=DEV), count=torch.empty((nt, 1), dtype=torch.int32, device=DEV),
                   areaNormal=torch.empty((nt, 3), dtype=torch.float32, device=DEV), subdiv=torch.empty(nt, dtype=torch.int32, device=DEV))

        def run():
            R._check(L.exa_hip_sample_triangles(R.h, None, 0, None, 0, ch, 1, spacing, max_n, binding.SURFACE_FROM_ISOSURFACE,
                                                *[C.c_void_p(out[k].data_ptr()) for k in binding.SURFACE_KEYS], 1, C.c_void_p(stream)))
            return R.sampleTrianglesMs()

        recs = {}
        for pack in (1, 0):
            R.setOption("surface_pack", pack)
            run()                                                           # warm-up
            ms = [run() for _ in range(args.reps)]
            sub = out["subdiv"].to(torch.int64)
            samples = int((sub * sub).sum().item())
            hist = torch.bincount(sub, minlength=65).tolist()
            kernel_ms = statistics.median(ms)
            recs[pack] = dict(what=name, surface_pack=pack, lattice=lattice, spacing=spacing, max_n=max_n, vertices=nv, triangles=nt,
                              samples=samples, valid_samples=int(out["count"].to(torch.int64).sum().item()), reps=args.reps,
                              kernel_ms=round(kernel_ms, 4), kernel_min_ms=round(min(ms), 4), kernel_max_ms=round(max(ms), 4),
                              samples_per_s=samples / (kernel_ms * 1e-3), n_histogram={str(n): c for n, c in enumerate(hist) if c})
        R.setOption("surface_pack", 1)
        # the yardstick: the points kernel on the samples' positions, band by band
        verts, tris, _ = R.readIsoSurface()
        sub = out["subdiv"].cpu().numpy()
        dv = torch.from_numpy(verts).to(DEV)
        points_ms, points_n, points_valid = 0.0, 0, 0
        for n in np.unique(sub[sub > 0]):
            ids = np.flatnonzero(sub == n)
            b1, b2 = (torch.from_numpy(b).to(DEV) for b in barycentrics(int(n)))
            per = max(1, int(args.band_points // (int(n) * int(n))))
            for at in range(0, len(ids), per):
                t = torch.from_numpy(tris[ids[at:at + per]].astype(np.int64)).to(DEV)
                v0, v1, v2 = dv[t[:, 0]], dv[t[:, 1]], dv[t[:, 2]]
                pts = ((v0[:, None, :] + b1[None, :, None] * (v1 - v0)[:, None, :]) + b2[None, :, None] * (v2 - v0)[:, None, :]).contiguous()
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
                points_n += m
                points_valid += int((status >= 0).sum().item())
                del pts, vals, status
        R.releaseIsoSurface()
        for pack in (1, 0):
            recs[pack]["over_points_kernel"] = round(recs[pack]["kernel_ms"] / points_ms, 3)
            emit(recs[pack])
        emit(dict(what=name + "_points_kernel_yardstick", n=points_n, reps=args.reps, kernel_ms=round(points_ms, 4),
                  valid_samples=points_valid, valid_samples_equal_the_calls=points_valid == recs[1]["valid_samples"],
                  points_per_s=points_n / (points_ms * 1e-3), pack0_over_pack1=round(recs[0]["kernel_ms"] / recs[1]["kernel_ms"], 3)))
    R.close()
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
