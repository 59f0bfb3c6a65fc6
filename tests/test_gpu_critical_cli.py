"""exaRender --critical: the file holds the records that the binding's Renderer.criticalPoints returns for the same lattice,
byte for byte, behind one header line that names the lattice, the channels, iterations, tolerance and the seven stats; the
summary on stdout counts the found points by n+ and spiral; a bad channel list and what the module refuses are errors."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import binding, scenes
from test_gpu_critical import CENTRE, DEFAULT, SINE, _linear, _sine, _with_fields

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
DIMS = (23, 19, 17)


def _read(path):
    """the .crit format: one text line, then the records"""
    with open(path, "rb") as f:
        head = f.readline().decode()
        body = f.read()
    num = r"(-?[0-9.e+-]+)"
    m = re.fullmatch(rf"critical (\d+) (\d+) (\d+) box {num} {num} {num} {num} {num} {num} channels (\d+) (\d+) (\d+) iterations (\d+) "
                     rf"tolerance {num} cells (\d+) invalidCells (\d+) candidates (\d+) found (\d+) nonFinite (\d+) leftCell (\d+) "
                     r"notConverged (\d+)\n", head)
    assert m, head
    g = m.groups()
    stats = dict(zip(binding.CRITICAL_STATS, (int(v) for v in g[14:21])))
    points = np.frombuffer(body, dtype=binding.CRITICAL_POINT_DTYPE, count=stats["found"])
    assert points.nbytes == len(body)
    return dict(dims=tuple(int(v) for v in g[0:3]), box=[float(v) for v in g[3:9]], channels=tuple(int(v) for v in g[9:12]),
                iterations=int(g[12]), tolerance=float(g[13]), stats=stats, points=points, head=head)


def test_exarender_critical_writes_the_bindings_bytes():
    scene = _with_fields(scenes.amr(levels=3, fields=1), _linear(DEFAULT, CENTRE) + _sine())
    R = Case(scene).hip_renderer()
    lo, hi = (np.asarray(b, np.float64) for b in R.prep.voxel_bounds())
    ext = hi - lo
    box = [np.float32(v) for v in (lo - 0.1 * ext, hi + 0.05 * ext)]
    want, want_stats = R.criticalPoints(*box, DIMS, channels=SINE, iterations=6, tolerance=2.0 ** -12)
    assert len(want) > 100 and want_stats["invalidCells"] > 0
    boxargs = [repr(float(c)) for v in box for c in v]
    lattice = [*map(str, DIMS)]
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "flow")
        out = os.path.join(d, "flow.crit")
        run = lambda *a: subprocess.run([EXE, cfg, "--frames", "0", *a], capture_output=True, text=True, timeout=300)      # noqa: E731
        r = run("--critical", "4,5,6", *boxargs, *lattice, "6", repr(2.0 ** -12), out)
        assert r.returncode == 0, r.stderr
        got = _read(out)
        assert got["points"].tobytes() == want.tobytes() and got["stats"] == want_stats
        assert got["dims"] == DIMS and got["channels"] == SINE and got["iterations"] == 6 and got["tolerance"] == 2.0 ** -12
        assert np.array_equal(np.float32(got["box"]), np.concatenate(box))
        kinds = [int(((want["type"] & 3) == k).sum()) for k in range(4)]
        spiral = [int((((want["type"] & 3) == k) & ((want["type"] & 4) != 0)).sum()) for k in range(4)]
        summary = (f"sinks {kinds[0]} spiral {spiral[0]} saddles1 {kinds[1]} spiral {spiral[1]} saddles2 {kinds[2]} spiral {spiral[2]} "
                   f"sources {kinds[3]} spiral {spiral[3]} degenerate {int(((want['type'] & 8) != 0).sum())}")
        assert got["head"].strip() + " " + summary in r.stdout, r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        # the linear field: one spiralling saddle
        r = run("--critical", "1,2,3", *boxargs, *lattice, "8", repr(2.0 ** -10), out)
        assert r.returncode == 0, r.stderr
        got = _read(out)
        assert got["points"].tobytes() == R.criticalPoints(*box, DIMS, channels=(1, 2, 3))[0].tobytes() and len(got["points"]) == 1
        assert "saddles2 1 spiral 1" in r.stdout, r.stdout
        for chans, its, tol, word in (("4,5", "8", "0.001", "C0,C1,C2"), ("4,5,6,7", "8", "0.001", "C0,C1,C2"), ("4,5,99", "8", "0.001", "exa_hip_critical_points"),
                                      ("4,5,6", "0", "0.001", "exa_hip_critical_points"), ("4,5,6", "8", "2", "exa_hip_critical_points")):
            r = run("--critical", chans, *boxargs, *lattice, its, tol, out)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (chans, its, tol, r.stderr)
    R.close()
