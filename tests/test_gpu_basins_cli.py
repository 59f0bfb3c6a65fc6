"""exaRender --basins: the file holds the table, the labels and the counts that the binding's Renderer.basins returns for the
same lattice, byte for byte; with --derived those of Renderer.basinsDerived; a vector quantity and a bad depth are refused."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import binding, scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")
DIMS = (23, 19, 17)


def _read(path):
    """the .basins format: one text line, then the table and the labels"""
    with open(path, "rb") as f:
        head = f.readline().decode()
        body = f.read()
    m = re.fullmatch(r"basins (\d+) (\d+) (\d+) count (\d+) raw (\d+) rounds (\d+) inside (\d+) exponent (-?\d+)\n", head)
    assert m, head
    nx, ny, nz, count, raw, rounds, inside, exponent = (int(g) for g in m.groups())
    assert (nx, ny, nz) == DIMS
    table = np.frombuffer(body, dtype=binding.BASIN_DTYPE, count=count)
    labels = np.frombuffer(body, dtype=np.int32, count=nx * ny * nz, offset=table.nbytes).reshape(nz, ny, nx)
    assert table.nbytes + labels.nbytes == len(body)
    return dict(basins=table, labels=labels, num_inside=inside, sum_exponent=exponent, num_raw=raw, rounds=rounds)


def _same(got, want):
    assert got["basins"].tobytes() == want["basins"].tobytes() and got["labels"].tobytes() == want["labels"].tobytes()
    for key in ("num_inside", "sum_exponent", "num_raw", "rounds"):
        assert got[key] == want[key], key


def test_exarender_basins_writes_the_bindings_bytes():
    scene = scenes.example("ex3")
    R = Case(scene).hip_renderer()
    lo, hi = (np.asarray(b, np.float64) for b in R.prep.voxel_bounds())
    ext = hi - lo
    box = [np.float32(v) for v in (lo - 0.1 * ext, hi + 0.05 * ext)]
    V = R.resample(*box, DIMS, fill=float("nan"))
    iso = float(np.float32(np.median(V[np.isfinite(V)])))
    depth = 0.0625
    want = R.basins(*box, DIMS, iso, depth)
    want_inf = R.basins(*box, DIMS, iso, float("inf"), below=True, faces=True)
    want_q = R.basinsDerived(*box, DIMS, 0.0, depth, "q", channels=(0, 0, 0))
    assert len(want["basins"]) > 0 and len(want_inf["basins"]) > 0 and 0 < want["num_inside"] < V.size and np.isnan(V).any()
    lattice = [*map(str, DIMS)]
    boxargs = ["--regions-box", *(repr(float(c)) for v in box for c in v)]
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        out = os.path.join(d, "peaks.basins")
        run = lambda *a: subprocess.run([EXE, cfg, "--frames", "0", *a], capture_output=True, text=True, timeout=300)      # noqa: E731
        r = run("--basins", "0", repr(iso), repr(depth), *lattice, out, *boxargs)
        assert r.returncode == 0, r.stderr
        _same(_read(out), want)
        assert (f"basins 23 19 17 channel 0 iso {iso:.9g} minDepth {depth:.9g} world 0 below 0 faces 0 count {len(want['basins'])} "
                f"raw {want['num_raw']} rounds {want['rounds']} inside {want['num_inside']} exponent {want['sum_exponent']}") in r.stdout, r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        r = run("--basins", "0", repr(iso), "inf", *lattice, out, *boxargs, "--regions-below", "--regions-faces")
        assert r.returncode == 0, r.stderr
        _same(_read(out), want_inf)
        assert "minDepth inf" in r.stdout and "below 1 faces 1" in r.stdout, r.stdout
        r = run("--derived", "q", "0", "0", "0", "--basins", "0", "0", repr(depth), *lattice, out, *boxargs)
        assert r.returncode == 0, r.stderr
        _same(_read(out), want_q)
        assert "basins 23 19 17 derived 4 channels 0 0 0" in r.stdout, r.stdout
        for extra, level, word in ((["--derived", "vorticity", "0", "0", "0"], "0.5", "one-component"), ([], "-1", "exa_hip_basins")):
            r = run(*extra, "--basins", "0", repr(iso), level, *lattice, out, *boxargs)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (extra, level, r.stderr)
    R.close()
