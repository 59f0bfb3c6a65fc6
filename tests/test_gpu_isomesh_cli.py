"""exaRender --isomesh: the CLI writes the mesh the binding's Renderer.isosurface returns, in the triangle file format a
config's `triangles` line reads, reports its counts, and a second run that lists the file as a surface loads and renders it."""
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


def _decode(raw):
    """the documented format: repeated int32 nVerts, vec3f[nVerts], int32 nTris, vec3i[nTris]"""
    meshes, at = [], 0
    while at < len(raw):
        nv = int(np.frombuffer(raw, np.int32, 1, at)[0])
        verts = np.frombuffer(raw, np.float32, 3 * nv, at + 4).reshape(nv, 3)
        at += 4 + 12 * nv
        nt = int(np.frombuffer(raw, np.int32, 1, at)[0])
        tris = np.frombuffer(raw, np.int32, 3 * nt, at + 4).reshape(nt, 3)
        at += 4 + 12 * nt
        meshes.append((verts, tris))
    assert at == len(raw)
    return meshes


@pytest.mark.parametrize("box", [None, "grown"], ids=["voxel-bounds", "grown-box"])
def test_exarender_isomesh_writes_the_bindings_mesh_and_loads_it_back(box):
    scene = scenes.amr(levels=3, fields=2)
    R = Case(scene).hip_renderer()
    lo, hi = R.prep.voxel_bounds()
    dims = (33, 27, 19)
    args = []
    if box == "grown":
        ext = hi - lo
        lo, hi = (lo - 0.1 * ext).astype(np.float32), (hi + 0.1 * ext).astype(np.float32)
        args = ["--isomesh-box"] + [repr(float(v)) for v in lo] + [repr(float(v)) for v in hi]
    iso = 0.5
    verts, tris, _ = R.isosurface(lo, hi, dims, iso, channel=1)
    assert len(tris) >= 500
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr")
        out = os.path.join(d, "surface.tris")
        r = subprocess.run([EXE, cfg, "--isomesh", repr(iso), *map(str, dims), out, "--isomesh-channel", "1", "--frames", "0",
                            *args], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        with open(out, "rb") as f:
            raw = f.read()
        meshes = _decode(raw)
        assert len(meshes) == 1
        assert meshes[0][0].tobytes() == verts.tobytes() and meshes[0][1].tobytes() == tris.tobytes()
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("isomesh ")]
        assert len(line) == 1, r.stdout
        m = re.fullmatch(r"isomesh 33 27 19 box (\S+ ){6}channel 1 iso 0\.5 vertices (\d+) triangles (\d+)", line[0])
        assert m and (int(m.group(2)), int(m.group(3))) == (len(verts), len(tris)), line[0]
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        # the file goes back in as a surface of the scene
        cfg2 = scenes.write_exa(scene, os.path.join(d, "again"), "amr", meshes=[(verts, tris)])
        with open(os.path.join(d, "again", "amr.tris"), "rb") as f:
            assert f.read() == raw                             # the writer of the tests and TriangleMesh::save agree
        os.replace(out, os.path.join(d, "again", "amr.tris"))  # ... and the renderer reads exaRender's own file
        r2 = subprocess.run([EXE, cfg2, "--size", "64", "64", "--frames", "1", "-o", os.path.join(d, "frame.ppm")],
                            capture_output=True, text=True, timeout=300)
        assert r2.returncode == 0, r2.stderr
        assert "Avg. after 1 frames" in r2.stdout
        assert os.path.getsize(os.path.join(d, "frame.ppm")) > 64 * 64 * 3
    R.close()
