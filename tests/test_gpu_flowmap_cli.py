"""exaRender --ftle: the file holds the arrays that the binding's Renderer.flowmap returns for the same lattice, channels, step,
number of steps and direction — end, steps, reasons and stretch byte for byte, ftle (formed on the host in both, with two
implementations of the double logarithm) within one float32 ulp; a bad channel list, a bad direction and what the module
refuses are errors."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
DIMS = (11, 9, 7)


def _read(path):
    nx, ny, nz = DIMS
    n = nx * ny * nz
    with open(path, "rb") as f:
        head = f.readline().decode()
        body = f.read()
    assert len(body) == 28 * n, (len(body), n)
    cut = lambda dtype, count, offset: np.frombuffer(body, dtype=dtype, count=count, offset=offset)      # noqa: E731
    return head, dict(end=cut(np.float32, 3 * n, 0).reshape(nz, ny, nx, 3), steps=cut(np.uint32, n, 12 * n).reshape(nz, ny, nx),
                      reasons=cut(np.int32, n, 16 * n).reshape(nz, ny, nx), stretch=cut(np.float32, n, 20 * n).reshape(nz, ny, nx),
                      ftle=cut(np.float32, n, 24 * n).reshape(nz, ny, nx))


def _same(got, want):
    for k in ("end", "steps", "reasons", "stretch"):
        assert got[k].tobytes() == want[k].tobytes(), k
    a, b = got["ftle"], want["ftle"]
    assert np.array_equal(np.isnan(a), np.isnan(b))
    ok = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(a[~ok & ~np.isnan(a)], b[~ok & ~np.isnan(b)])
    assert np.all(np.abs(a[ok].view(np.int32).astype(np.int64) - b[ok].view(np.int32).astype(np.int64)) <= 1)


def test_exarender_ftle_writes_the_bindings_arrays():
    scene = scenes.example("ex3")
    R = Case(scene).hip_renderer()
    lo, hi = (np.asarray(b, np.float64) for b in R.prep.voxel_bounds())
    ext = hi - lo
    box = [np.float32(v) for v in (lo - 0.1 * ext, hi + 0.05 * ext)]
    field = R.resample(*box, DIMS)
    step = float(np.float32(0.02 * ext.max() / np.nanmax(np.abs(field))))          # a step moves at most 2 % of the volume
    want = R.flowmap(*box, DIMS, (0, 0, 0), step, 9)
    back = R.flowmap(*box, DIMS, (0, 0, 0), step, 9, backward=True)
    assert np.isfinite(want["ftle"]).sum() > 50 and np.isnan(want["ftle"]).any() and not np.array_equal(want["end"], back["end"])
    args = [*(repr(float(c)) for v in box for c in v), *map(str, DIMS), repr(step), "9"]      # l u NX NY NZ STEP NUMSTEPS
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        out = os.path.join(d, "flow.ftle")
        run = lambda *a: subprocess.run([EXE, cfg, "--frames", "0", *a], capture_output=True, text=True, timeout=300)      # noqa: E731
        r = run("--ftle", "0,0,0", *args, "fwd", out)
        assert r.returncode == 0, r.stderr
        head, got = _read(out)
        assert head == f"ftle 11 9 7 channels 0 0 0 step {step:.9g} numSteps 9 direction fwd\n", head
        _same(got, want)
        assert f"numSteps 9 direction fwd points_with_ftle {int((~np.isnan(want['ftle'])).sum())}" in r.stdout, r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        r = run("--ftle", "0,0,0", *args, "bwd", out)
        assert r.returncode == 0, r.stderr
        head, got = _read(out)
        assert head.endswith("direction bwd\n")
        _same(got, back)
        for channels, tail, direction, word in (("0,0", args, "fwd", "--ftle wants"), ("0;0;0", args, "fwd", "--ftle wants"),
                                                ("0,0,0", args, "up", "--ftle wants"), ("0,0,7", args, "fwd", "exa_hip_flowmap"),
                                                ("0,0,0", args[:-1] + ["0"], "fwd", "exa_hip_flowmap")):
            r = run("--ftle", channels, *tail, direction, out)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (channels, direction, r.stderr)
    R.close()
