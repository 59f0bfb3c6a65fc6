"""exaRender --distance: the file holds dist and nearest that the binding's distance returns for the same lattice, byte for
byte, and the stats in its text line; with --distance-signed, --distance-outside and --derived those calls'; a vector
quantity and a bad reach are refused."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import distance as dt
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
DIMS = (23, 19, 17)


def _read(path):
    """the .dist format: one text line, then dist and nearest"""
    with open(path, "rb") as f:
        head = f.readline().decode()
        body = f.read()
    m = re.fullmatch(r"distance (\d+) (\d+) (\d+) points (\d+) inside (\d+) reached (\d+) maxDistance (\S+)\n", head)
    assert m, head
    nx, ny, nz, points, inside, reached = (int(g) for g in m.groups()[:6])
    assert (nx, ny, nz) == DIMS and points == nx * ny * nz
    dist = np.frombuffer(body, dtype=np.float32, count=points).reshape(nz, ny, nx)
    nearest = np.frombuffer(body, dtype=np.int32, count=points, offset=dist.nbytes).reshape(nz, ny, nx)
    assert dist.nbytes + nearest.nbytes == len(body)
    return dict(dist=dist, nearest=nearest, stats=dict(points=points, inside=inside, reached=reached, maxDistance=float(m.group(7))))


def _same(got, want):
    assert got["dist"].tobytes() == want["dist"].tobytes() and got["nearest"].tobytes() == want["nearest"].tobytes()
    assert {k: v for k, v in got["stats"].items() if k != "maxDistance"} == {k: v for k, v in want["stats"].items() if k != "maxDistance"}
    assert np.float32(got["stats"]["maxDistance"]) == np.float32(want["stats"]["maxDistance"])          # printed with %.9g


def test_exarender_distance_writes_the_bindings_bytes():
    scene = scenes.example("ex3")
    R = Case(scene).hip_renderer()
    lo, hi = (np.asarray(b, np.float64) for b in R.prep.voxel_bounds())
    ext = hi - lo
    box = [np.float32(v) for v in (lo - 0.1 * ext, hi + 0.05 * ext)]
    V = R.resample(*box, DIMS, fill=float("nan"))
    iso = float(np.float32(np.median(V[np.isfinite(V)])))
    reach = float(np.float32(0.1 * ext.max()))
    want = dt.distance(R, *box, DIMS, iso, nearest=True)
    want_signed = dt.distance(R, *box, DIMS, iso, max_distance=reach, signed=True, nearest=True)
    want_wall = dt.distance(R, *box, DIMS, -3.4028235e38, to_outside=True, nearest=True)
    want_q = dt.distance(R, *box, DIMS, 0.0, quantity="q", channels=(0, 0, 0), nearest=True)
    assert 0 < want["stats"]["inside"] < V.size and np.isnan(V).any() and want["stats"]["reached"] == V.size
    assert 0 < want_signed["stats"]["reached"] <= V.size and (want_signed["dist"] < 0).any() and (want_signed["dist"] > 0).any()
    assert want_wall["stats"]["inside"] == int(np.isfinite(V).sum())
    lattice = [*map(str, DIMS)]
    boxargs = ["--distance-box", *(repr(float(c)) for v in box for c in v)]
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        out = os.path.join(d, "wall.dist")
        run = lambda *a: subprocess.run([EXE, cfg, "--frames", "0", *a], capture_output=True, text=True, timeout=300)      # noqa: E731
        r = run("--distance", "0", repr(iso), "inf", *lattice, out, *boxargs)
        assert r.returncode == 0, r.stderr
        _same(_read(out), want)
        st = want["stats"]
        assert (f"distance 23 19 17 channel 0 iso {iso:.9g} maxDistance inf signed 0 outside 0 points {st['points']} "
                f"inside {st['inside']} reached {st['reached']} maxDistance {st['maxDistance']:.9g}") in r.stdout, r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        r = run("--distance", "0", repr(iso), repr(reach), *lattice, out, *boxargs, "--distance-signed")
        assert r.returncode == 0, r.stderr
        _same(_read(out), want_signed)
        assert "signed 1 outside 0" in r.stdout, r.stdout
        r = run("--distance", "0", "-3.4028235e38", "inf", *lattice, out, *boxargs, "--distance-outside")
        assert r.returncode == 0, r.stderr
        _same(_read(out), want_wall)
        r = run("--derived", "q", "0", "0", "0", "--distance", "0", "0", "inf", *lattice, out, *boxargs)
        assert r.returncode == 0, r.stderr
        _same(_read(out), want_q)
        assert "distance 23 19 17 derived 4 channels 0 0 0" in r.stdout, r.stdout
        for extra, reach_word, word in ((["--derived", "vorticity", "0", "0", "0"], "inf", "one-component"), ([], "0", "exa_hip_distance"),
                                        (["--distance-signed", "--distance-outside"], "inf", "EXA_DISTANCE_SIGNED")):
            r = run(*extra, "--distance", "0", "0.5", reach_word, *lattice, out, *boxargs)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (extra, reach_word, r.stderr)
    R.close()
