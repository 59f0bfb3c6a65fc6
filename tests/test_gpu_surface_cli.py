"""exaRender --surface: the CLI integrates channels over a triangle file, or (the word `iso`) over the mesh its own --isomesh
left on the device, and writes per triangle and in total what the binding's Renderer.surfaceIntegrals returns — the text
holds floats as %.9g and doubles as %.17g, which read back to the same bits."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from common import ROOT, Case
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")


def _same(a, b):
    """equal values, NaN equal to NaN (text does not carry a NaN's bits)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def _compare(path, I, channels, spacing, max_n, world=0):
    with open(path) as f:
        lines = f.read().splitlines()
    S = I["samples"]
    m, nc = S["sum"].shape
    head = lines[0].split()
    assert head[:4] == ["surface", "triangles", str(m), "channels"] and head[4:5 + nc] == [str(nc)] + [str(c) for c in channels], lines[0]
    assert head[5 + nc:] == ["spacing", "%.9g" % np.float32(spacing), "maxN", str(max_n), "world", str(world)], lines[0]
    rows = np.array([[float(x) for x in ln.split()] for ln in lines[1:1 + m]])
    assert rows.shape == (m, 5 + 4 * nc)
    assert np.array_equal(rows[:, 0], S["subdiv"]) and _same(rows[:, 1:4].astype(np.float32), S["areaNormal"]) and _same(rows[:, 4], I["area"])
    for c in range(nc):
        col = rows[:, 5 + 4 * c: 9 + 4 * c]
        assert np.array_equal(col[:, 0], S["count"][:, c]) and _same(col[:, 1], S["sum"][:, c])
        assert _same(col[:, 2], I["mean"][:, c]) and _same(col[:, 3], I["integral"][:, c])
    tail = lines[1 + m:]
    assert tail[0] == f"invalid {I['invalid_triangles']}"
    for c in range(nc):
        t = tail[1 + c].split()
        assert t[0::2][:5] == ["total", "covered_area", "uncovered_area", "uncovered_triangles", "integral"] and t[10] == "force", tail[1 + c]
        assert int(t[1]) == channels[c] and int(t[7]) == I["uncovered_triangles"][c]
        assert _same(float(t[3]), I["covered_area"][c]) and _same(float(t[5]), I["uncovered_area"][c])
        assert _same(float(t[9]), I["total_integral"][c]) and _same([float(x) for x in t[11:14]], I["force"][c])
    if nc == 3:
        assert tail[1 + nc].split()[0] == "flux" and _same(float(tail[1 + nc].split()[1]), I["flux"])
    assert len(tail) == 1 + nc + (1 if nc == 3 else 0)


def test_exarender_surface_on_its_iso_mesh_and_on_a_file():
    scene = scenes.amr(levels=3, fields=3)
    R = Case(scene).hip_renderer()
    lo, hi = R.prep.voxel_bounds()
    dims, iso, spacing, max_n = (14, 12, 10), 0.5, 1.5, 8
    verts, tris, _ = R.isosurface(lo, hi, dims, iso, channel=1)
    assert len(tris) >= 200
    three = R.surfaceIntegrals(verts, tris, channels=(0, 1, 2), spacing=spacing, max_n=max_n)
    one = R.surfaceIntegrals(verts, tris, channels=(2,), spacing=0.0, max_n=3)
    assert (three["samples"]["count"] > 0).any() and len(set(three["samples"]["subdiv"].tolist())) >= 2 and np.isfinite(three["flux"])
    assert three["uncovered_triangles"].sum() > 0 or three["covered_area"].min() > 0
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(scene, d, "amr")
        mesh, a, b = os.path.join(d, "surface.tris"), os.path.join(d, "a.surf"), os.path.join(d, "b.surf")
        r = subprocess.run([EXE, cfg, "--isomesh", repr(iso), *map(str, dims), mesh, "--isomesh-channel", "1", "--frames", "0",
                            "--surface", "iso", "0,1,2", repr(spacing), str(max_n), a], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        _compare(a, three, (0, 1, 2), spacing, max_n)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("surface ")]
        assert line == [f"surface triangles {len(tris)} channels 3 spacing 1.5 maxN 8 invalid 0"], r.stdout
        assert "Avg. after" not in r.stdout                    # --frames 0: nothing rendered
        # the file that run wrote, as a mesh of its own
        r = subprocess.run([EXE, cfg, "--frames", "0", "--surface", mesh, "2", "0", "3", b], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        _compare(b, one, (2,), 0.0, 3)
        # `iso` without --isomesh, and a bad channel list, are errors
        r = subprocess.run([EXE, cfg, "--frames", "0", "--surface", "iso", "0", "1", "4", b], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "--isomesh" in r.stderr
        r = subprocess.run([EXE, cfg, "--frames", "0", "--surface", mesh, "0;1", "1", "4", b], capture_output=True, text=True, timeout=300)
        assert r.returncode != 0 and "channels" in r.stderr
    R.close()
