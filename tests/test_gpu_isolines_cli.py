"""exaRender --isolines: the file holds the arrays that the binding's Renderer.isolines returns for the same plane and
levels, byte for byte; with --derived those of Renderer.isolinesDerived; a vector quantity and a bad list are refused."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
SIZE = (67, 41)


def _read(path, levels):
    """the .isolines format: one text line, then levels, both offset arrays, vertices, uv, segments"""
    with open(path, "rb") as f:
        head = f.readline().decode()
        body = f.read()
    m = re.fullmatch(r"isolines (\d+) (\d+) levels (\d+) vertices (\d+) segments (\d+)\n", head)
    assert m, head
    nu, nv, n, V, S = (int(g) for g in m.groups())
    assert (nu, nv, n) == (*SIZE, levels)
    out, at = {}, 0
    for key, dtype, count in (("levels", np.float32, n), ("vertex_offsets", np.uint64, n + 1), ("segment_offsets", np.uint64, n + 1),
                              ("vertices", np.float32, 3 * V), ("uv", np.float32, 2 * V), ("segments", np.int32, 2 * S)):
        out[key] = np.frombuffer(body, dtype=dtype, count=count, offset=at)
        at += out[key].nbytes
    assert at == len(body)
    return out


def test_exarender_isolines_writes_the_bindings_bytes():
    scene = scenes.example("ex3")
    R = Case(scene).hip_renderer()
    lo, hi = (np.asarray(b, np.float64) for b in R.prep.voxel_bounds())
    ext = hi - lo
    plane = [np.float32(v) for v in (lo + ext * (0.05, -0.1, 0.2), ext * (0.9, 0.7, 0.1) / SIZE[0], ext * (-0.03, 0.4, 0.6) / SIZE[1])]
    V = R.isolines(*plane, SIZE, [3e38], values=True)["values"]
    fin = np.unique(V[np.isfinite(V)])
    isos = [np.float32(fin[(3 * fin.size) // 4]), np.float32(0.5 * (float(fin[fin.size // 2]) + float(fin[fin.size // 2 + 1])))]
    want = R.isolines(*plane, SIZE, isos)
    assert len(want["segments"]) > 20 and not np.isfinite(V).all()
    Q = R.isolinesDerived(*plane, SIZE, [3e38], "q", channels=(0, 0, 0), values=True)["values"]
    qfin = np.unique(Q[np.isfinite(Q)])
    qiso = [np.float32(0.5 * (float(qfin[qfin.size // 2]) + float(qfin[qfin.size // 2 + 1])))]
    want_q = R.isolinesDerived(*plane, SIZE, qiso, "q", channels=(0, 0, 0))
    assert len(want_q["segments"]) > 0
    args = ["0", *(repr(float(c)) for v in plane for c in v), *map(str, SIZE)]          # CHANNEL o u v NU NV
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        out = os.path.join(d, "cut.isolines")
        r = subprocess.run([EXE, cfg, "--frames", "0", "--isolines", *args, ",".join(repr(float(v)) for v in isos), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = _read(out, 2)
        assert got["levels"].tobytes() == np.asarray(isos, np.float32).tobytes()
        for k, v in want.items():
            assert got[k].tobytes() == v.tobytes(), k
        assert f"isolines 67 41 channel 0 world 0 levels 2 vertices {len(want['vertices'])} segments {len(want['segments'])}" in r.stdout, r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        r = subprocess.run([EXE, cfg, "--frames", "0", "--derived", "q", "0", "0", "0", "--isolines", *args, repr(float(qiso[0])), out],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = _read(out, 1)
        for k, v in want_q.items():
            assert got[k].tobytes() == v.tobytes(), k
        assert "isolines 67 41 derived 4 channels 0 0 0 world 0 levels 1" in r.stdout, r.stdout
        for extra, levels, word in ((["--derived", "vorticity", "0", "0", "0"], "0.5", "one-component"), ([], "0.5,,1", "--isolines wants"),
                                    ([], "0.5;1", "--isolines wants"), ([], "nan", "exa_hip_isolines")):
            r = subprocess.run([EXE, cfg, "--frames", "0", *extra, "--isolines", *args, levels, out], capture_output=True, text=True, timeout=300)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (extra, levels, r.stderr)
    R.close()
