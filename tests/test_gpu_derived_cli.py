"""exaRender --derived: --resample and --isomesh work on a derived flow quantity instead of a channel and write what the
binding's Renderer.resampleDerived / isosurfaceDerived return, byte for byte; a channel flag beside it is an error."""
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
DIMS = (33, 27, 19)


def test_exarender_derived_writes_the_bindings_bytes():
    scene = scenes.amr(levels=3, fields=3)
    R = Case(scene).hip_renderer()
    lo, hi = R.prep.voxel_bounds()
    ext = hi - lo
    lo, hi = (lo - 0.1 * ext).astype(np.float32), (hi + 0.1 * ext).astype(np.float32)
    box = [repr(float(v)) for v in lo] + [repr(float(v)) for v in hi]
    want_q = R.resampleDerived(lo, hi, DIMS, "q", fill=-7.0)
    want_w = R.resampleDerived(lo, hi, DIMS, "vorticity", channels=(2, 0, 1), fill=-7.0)
    invalid = int((want_q == np.float32(-7.0)).sum())
    assert 0 < invalid < want_q.size
    fin = R.resampleDerived(lo, hi, DIMS, "q")
    iso = float(np.float32(np.median(fin[np.isfinite(fin)])))
    verts, tris = R.isosurfaceDerived(lo, hi, DIMS, iso, "q")
    assert len(tris) >= 500
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr")
        raw, mesh = os.path.join(d, "grid.raw"), os.path.join(d, "surface.tris")
        r = subprocess.run([EXE, cfg, "--frames", "0", "--derived", "q", "0", "1", "2", "--resample", *map(str, DIMS), raw,
                            "--resample-box", *box, "--resample-fill", "-7", "--isomesh", repr(iso), *map(str, DIMS), mesh,
                            "--isomesh-box", *box], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert np.fromfile(raw, dtype=np.float32).tobytes() == want_q.tobytes()
        with open(mesh, "rb") as f:
            got = f.read()
        # the triangle file format: int32 nVerts, vec3f[nVerts], int32 nTris, vec3i[nTris]
        assert got == (np.int32(len(verts)).tobytes() + verts.tobytes() + np.int32(len(tris)).tobytes() + tris.tobytes())
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("resample ")]
        m = len(line) == 1 and re.fullmatch(r"resample 33 27 19 box (\S+ ){6}derived 4 channels 0 1 2 components 1 invalid (\d+)", line[0])
        assert m and int(m.group(2)) == invalid, r.stdout
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("isomesh ")]
        m = len(line) == 1 and re.fullmatch(r"isomesh 33 27 19 box (\S+ ){6}derived 4 channels 0 1 2 iso \S+ vertices (\d+) triangles (\d+)", line[0])
        assert m and (int(m.group(2)), int(m.group(3))) == (len(verts), len(tris)), r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        # the vector quantity, by number, interleaved
        r = subprocess.run([EXE, cfg, "--frames", "0", "--derived", "2", "2", "0", "1", "--resample", *map(str, DIMS), raw,
                            "--resample-box", *box, "--resample-fill", "-7"], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        assert np.fromfile(raw, dtype=np.float32).tobytes() == want_w.tobytes()
        assert "derived 2 channels 2 0 1 components 3" in r.stdout
        # refused: a channel flag beside --derived, a surface of the vector quantity, an unknown name
        for extra, word in ((["--derived", "q", "0", "1", "2", "--resample-channel", "1"], "--resample-channel"),
                            (["--derived", "q", "0", "1", "2", "--isomesh-channel", "1"], "--isomesh-channel"),
                            (["--derived", "vorticity", "0", "1", "2", "--isomesh", "0.5", *map(str, DIMS), mesh], "one-component"),
                            (["--derived", "lambda2", "0", "1", "2"], "--derived wants")):
            r = subprocess.run([EXE, cfg, "--frames", "0", "--resample", *map(str, DIMS), raw, *extra],
                               capture_output=True, text=True, timeout=300)
            assert r.returncode != 0 and word in r.stderr + r.stdout, (extra, r.stderr)
    R.close()
