"""exaRender --regions: the file holds the table and the labels that the binding's Renderer.regions returns for the same
lattice, byte for byte; with --derived those of Renderer.regionsDerived; a vector quantity and a bad level are refused."""
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
    """the .regions format: one text line, then the table and the labels"""
    with open(path, "rb") as f:
        head = f.readline().decode()
        body = f.read()
    m = re.fullmatch(r"regions (\d+) (\d+) (\d+) count (\d+) inside (\d+) exponent (-?\d+)\n", head)
    assert m, head
    nx, ny, nz, count, inside, exponent = (int(g) for g in m.groups())
    assert (nx, ny, nz) == DIMS
    table = np.frombuffer(body, dtype=binding.LABELLED_REGION_DTYPE, count=count)
    labels = np.frombuffer(body, dtype=np.int32, count=nx * ny * nz, offset=table.nbytes).reshape(nz, ny, nx)
    assert table.nbytes + labels.nbytes == len(body)
    return dict(regions=table, labels=labels, num_inside=inside, sum_exponent=exponent)


def _same(got, want):
    assert got["regions"].tobytes() == want["regions"].tobytes() and got["labels"].tobytes() == want["labels"].tobytes()
    assert (got["num_inside"], got["sum_exponent"]) == (want["num_inside"], want["sum_exponent"])


def test_exarender_regions_writes_the_bindings_bytes():
    scene = scenes.example("ex3")
    R = Case(scene).hip_renderer()
    lo, hi = (np.asarray(b, np.float64) for b in R.prep.voxel_bounds())
    ext = hi - lo
    box = [np.float32(v) for v in (lo - 0.1 * ext, hi + 0.05 * ext)]
    V = R.resample(*box, DIMS, fill=float("nan"))
    iso = float(np.float32(np.median(V[np.isfinite(V)])))
    want = R.regions(*box, DIMS, iso)
    want_bf = R.regions(*box, DIMS, iso, below=True, faces=True)
    want_q = R.regionsDerived(*box, DIMS, 0.0, "q", channels=(0, 0, 0))
    assert len(want["regions"]) > 0 and len(want_bf["regions"]) > 0 and 0 < want["num_inside"] < V.size and np.isnan(V).any()
    lattice = [*map(str, DIMS)]
    boxargs = ["--regions-box", *(repr(float(c)) for v in box for c in v)]
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "ex3")
        out = os.path.join(d, "blobs.regions")
        run = lambda *a: subprocess.run([EXE, cfg, "--frames", "0", *a], capture_output=True, text=True, timeout=300)      # noqa: E731
        r = run("--regions", "0", repr(iso), *lattice, out, *boxargs)
        assert r.returncode == 0, r.stderr
        _same(_read(out), want)
        assert (f"regions 23 19 17 channel 0 iso {iso:.9g} world 0 below 0 faces 0 count {len(want['regions'])} "
                f"inside {want['num_inside']} exponent {want['sum_exponent']}") in r.stdout, r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        r = run("--regions", "0", repr(iso), *lattice, out, *boxargs, "--regions-below", "--regions-faces")
        assert r.returncode == 0, r.stderr
        _same(_read(out), want_bf)
        assert "below 1 faces 1" in r.stdout, r.stdout
        r = run("--derived", "q", "0", "0", "0", "--regions", "0", "0", *lattice, out, *boxargs)
        assert r.returncode == 0, r.stderr
        _same(_read(out), want_q)
        assert "regions 23 19 17 derived 4 channels 0 0 0" in r.stdout, r.stdout
        for extra, level, word in ((["--derived", "vorticity", "0", "0", "0"], "0.5", "one-component"), ([], "nan", "exa_hip_regions")):
            r = run(*extra, "--regions", "0", level, *lattice, out, *boxargs)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (extra, level, r.stderr)
    R.close()
