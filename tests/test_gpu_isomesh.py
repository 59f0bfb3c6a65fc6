"""Iso-surface extraction on the GPU (exa_hip_isosurface, include/exa_hip.h): the mesh equals the numpy restatement of the
contract (tests/isomesh_ref.py) bit for bit when that is fed the lattice exa_hip_resample returns; gradients equal the
points probe at the vertices; a sphere comes out closed and oriented; nothing a frame or a tuning knob sets changes a byte;
bad arguments are refused with a message and leave the handle usable."""
import ctypes as C
import math

import numpy as np
import pytest

import isomesh_ref as ref
from analysis_steps import bits as _bits, frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes

pytestmark = pytest.mark.gpu

NAN = float("nan")
DIMS = (37, 29, 23)
XFM = dict(vx=[1.6, 0.5, -0.2], vy=[-0.4, 1.3, 0.3], vz=[0.25, -0.15, 0.9], p=[3.5, -1.25, 2.0])


def _root_box(prep, grow=0.1):
    """the root box of the region kd-tree (the union of the region domains), grown"""
    r = prep.regions()
    lo = np.stack(list(r["dom_lo"])).min(axis=0).astype(np.float64)
    hi = np.stack(list(r["dom_hi"])).max(axis=0).astype(np.float64)
    ext = hi - lo
    return (lo - grow * ext).astype(np.float32), (hi + grow * ext).astype(np.float32)


def _isos(V):
    """the median of the finite lattice values, and one lattice value exactly (a vertex with t == 0).  Where more than half
    of the lattice holds the field's minimum (ex1, the generated scene: a background of zeros) the median is that minimum, at
    and below which no surface exists: there the median of the values above the minimum is taken."""
    fin = np.sort(V[np.isfinite(V)])
    assert fin.size > 100
    median = np.float32(np.median(fin))
    if median <= fin[0] < fin[-1]:
        median = np.float32(np.median(fin[fin > fin[0]]))
    exact = fin[(2 * fin.size) // 5]
    if exact == fin[0] and fin[0] < fin[-1]:          # a constant lower part: the first value above it
        exact = fin[np.searchsorted(fin, fin[0], side="right")]
    return [("median", float(median)), ("exact", float(exact))]


def _cases():
    out = []
    # ex0 is a single cell: its reconstruction is constant and has no iso-surface (the empty mesh is compared)
    for nm in ["ex0", "ex1", "ex2", "ex3", "ex4"]:
        out += [(nm, lambda nm=nm: scenes.example(nm), form, False, 0 if nm == "ex0" else 1) for form in (0, 1)]
    out += [("amr3", lambda: scenes.amr(levels=3, fields=3), form, False, 500) for form in (0, 1)]
    out += [("gen", lambda: scenes.generated(root=(2, 2, 2), B=4, levels=2), form, False, 500) for form in (0, 1)]
    out += [("amr3_holes", lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=2), fraction=0.15), 0, True, 500)]
    return out


CASES = _cases()


def _compare(R, lo, hi, dims, iso, channel, world, min_tris, what):
    V = R.resample(lo, hi, dims, channel=channel, world=world, fill=NAN)
    want_v, want_t = ref.extract(V, lo, hi, iso)
    # the case is not vacuous: a surface, and cubes that must stay silent
    assert len(want_t) >= min_tris, (what, len(want_t))
    valid = ref.valid_cubes(V)
    ncubes = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    assert 0 < valid.sum() < ncubes, (what, int(valid.sum()), ncubes)
    verts, tris, grads = R.isosurface(lo, hi, dims, iso, channel=channel, world=world, gradients=True)
    print(f"{what}: vertices {len(verts)} triangles {len(tris)} valid cubes {int(valid.sum())}/{ncubes}")
    assert verts.shape == want_v.shape and tris.shape == want_t.shape, (what, verts.shape, want_v.shape, tris.shape, want_t.shape)
    assert np.array_equal(_bits(verts), _bits(want_v)), (what, np.nonzero(_bits(verts) != _bits(want_v))[0][:10])
    assert tris.dtype == np.int32 and np.array_equal(tris, want_t), (what, np.nonzero(tris != want_t)[0][:10])
    # gradients: the points probe at the returned vertices, fills included
    _, g, _ = R.samplePoints(verts, channels=(channel,), gradient=True, normalized=True, world=world, fill=NAN)
    assert grads.shape == verts.shape and np.array_equal(_bits(grads), _bits(g[:, 0])), what
    assert len(verts) == 0 or np.isfinite(grads).any()
    return verts, tris


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{c[0]}-f{c[2]}" for c in CASES])
def test_mesh_equals_the_restatement_bit_for_bit(idx):
    name, make, form, empty, min_tris = CASES[idx]
    case = Case(make(), basis_form=form, allow_empty_cells=empty)
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    channel = len(case.scene.fields) - 1
    V = R.resample(lo, hi, DIMS, channel=channel, fill=NAN)
    for label, iso in _isos(V):
        if label == "exact":
            assert (V == np.float32(iso)).any()
        _compare(R, lo, hi, DIMS, iso, channel, False, min_tris, f"{name} form {form} {label} iso {iso!r}")
    R.close()


def test_mesh_in_world_space_equals_the_restatement():
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lo, hi = np.array([-4, -6, -5], np.float32), np.array([30, 24, 26], np.float32)
    dims = (41, 33, 27)
    V = R.resample(lo, hi, dims, channel=1, world=True, fill=NAN)
    iso = _isos(V)[0][1]
    verts, tris = _compare(R, lo, hi, dims, iso, 1, True, 500, "amr3 world")
    # positions stay in the caller's space: inside the world box, and different from the voxel-space extraction
    assert np.all(verts >= lo) and np.all(verts <= hi)
    v2, t2, _ = R.isosurface(lo, hi, dims, iso, channel=1, world=False)
    assert v2.shape != verts.shape or not np.array_equal(_bits(v2), _bits(verts))
    R.close()


def test_sphere_is_closed_oriented_and_of_genus_zero():
    centre, radius = np.array([31.3, 32.1, 30.7]), 20.0
    scene = scenes.with_extra_field(scenes.example("c1_64"),       # one level, 64^3 cells
                                    lambda c: 1.0 - np.linalg.norm(c.astype(np.float64) - centre, axis=1) / radius)
    R = Case(scene).hip_renderer()
    lo, hi = (0.0, 0.0, 0.0), (64.0, 64.0, 64.0)                   # the lattice is the cell centres
    assert np.array_equal(R.prep.voxel_bounds()[0], [0, 0, 0]) and np.array_equal(R.prep.voxel_bounds()[1], [64, 64, 64])
    assert radius >= 4 and np.all(centre - radius > 0.5) and np.all(centre + radius < 63.5)
    verts, tris, grads = R.isosurface(lo, hi, (64, 64, 64), 0.0, channel=1, gradients=True)
    assert len(tris) > 10000
    bad = ref.degenerate(verts, tris)
    print(f"sphere: vertices {len(verts)} triangles {len(tris)} degenerate {int(bad.sum())}")
    assert bad.mean() <= 0.01
    tris = tris[~bad]
    rep = ref.closed_manifold_report(len(verts), tris)
    assert rep == dict(boundary=0, repeated=0, euler=2), rep        # every edge: two triangles, opposite directions
    assert ref.unreferenced_vertices(len(verts), tris) == 0
    nrm = ref.normals64(verts, tris)
    centroid = verts.astype(np.float64)[tris].mean(axis=1)
    assert np.all(np.einsum("ij,ij->i", nrm, centroid - centre) > 0)   # toward the lower values: outward
    rad = np.linalg.norm(verts.astype(np.float64) - centre, axis=1)
    assert np.all(np.abs(rad - radius) < 0.1), (rad.min(), rad.max())
    # the shading normal -grad/|grad| points outward as well
    assert np.all(np.einsum("ij,ij->i", -grads.astype(np.float64), verts.astype(np.float64) - centre) > 0)
    R.close()


def test_mesh_does_not_depend_on_frame_state_or_options():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    want = R.isosurface(lo, hi, DIMS, iso, channel=1, gradients=True)
    assert len(want[1]) >= 500

    def same(what):
        got = R.isosurface(lo, hi, DIMS, iso, channel=1, gradients=True)
        for x, y in zip(got, want):
            assert x.tobytes() == y.tobytes(), what

    same("two consecutive calls")
    for what in frame_perturbations(case, R):
        same(what)
    for patch in range(4):
        R.setOption("sample_patch", patch)
        same(f"sample_patch {patch}")
    R.setOption("sample_uniform", 0)
    same("sample_uniform 0")
    R.close()


def _raw(R, lo=(0, 0, 0), hi=(8, 8, 8), dims=(9, 9, 9), channel=0, iso=0.5, flags=0):
    lo3, hi3, d3 = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*dims)
    nv, nt = C.c_uint64(77), C.c_uint64(77)
    rc = binding.lib().exa_hip_isosurface(R.h, lo3, hi3, d3, channel, iso, flags, C.byref(nv), C.byref(nt), None)
    return rc, int(nv.value), int(nt.value), binding.lib().exa_hip_last_error(R.h).decode()


def test_empty_surface_and_refused_arguments():
    case = Case(scenes.example("ex3"), W=32, H=32)
    R = case.hip_renderer()                                    # no render yet: the module holds no frame state
    L = binding.lib()
    buf = np.zeros(64, np.float32)
    # a read before any extraction
    assert L.exa_hip_isosurface_read(R.h, buf.ctypes.data, None, None, 0, None) != 0
    assert "exa_hip_isosurface" in L.exa_hip_last_error(R.h).decode()
    rc, nv, nt, msg = _raw(R, flags=binding.SAMPLE_WORLD_SPACE)
    assert rc != 0 and "frame state" in msg, msg
    frame = R.render()
    lo, hi = R.prep.voxel_bounds()
    top = max(float(f.max()) for f in case.scene.fields)
    rc, nv, nt, _ = _raw(R, lo, hi, iso=top + 1.0)             # above the maximum: nothing, and no error
    assert (rc, nv, nt) == (0, 0, 0)
    v, t, g = R.readIsoSurface()
    assert v.shape == (0, 3) and t.shape == (0, 3)
    rc, nv, nt, _ = _raw(R, lo, hi, iso=0.5 * top)
    assert rc == 0 and nv > 0 and nt > 0
    bad = [dict(iso=math.nan), dict(iso=math.inf), dict(iso=-math.inf), dict(dims=(1, 9, 9)), dict(dims=(9, 9, 0)),
           dict(dims=(9, -3, 9)), dict(channel=len(case.scene.fields)), dict(channel=-1), dict(flags=4), dict(flags=8),
           dict(flags=1 << 30), dict(hi=(8, 0, 8)), dict(lo=(math.nan, 0, 0))]
    for kw in bad:
        rc, nv, nt, msg = _raw(R, **kw)
        assert rc != 0 and (nv, nt) == (0, 0) and msg.startswith("exa_hip_isosurface: "), (kw, rc, msg)
        assert R.render().shape == frame.shape, kw             # the handle still renders
    rc, nv, nt, msg = _raw(R, dims=(2 ** 22, 2 ** 21, 2 ** 21))        # 2^64 lattice points: the product is 0 in 64 bits
    assert rc != 0 and (nv, nt) == (0, 0) and "more than 2^31 - 1 points" in msg, msg
    # a failed extraction dropped the mesh
    assert L.exa_hip_isosurface_read(R.h, buf.ctypes.data, None, None, 0, None) != 0
    with pytest.raises(RuntimeError, match="exa_hip_isosurface"):
        R.isosurface(lo, hi, (2 ** 11, 2 ** 11, 2 ** 10), 0.5)      # 2^32 lattice points
    # gradients asked of a mesh extracted without them
    R.extractIsoSurface(lo, hi, (9, 9, 9), 0.5 * top)
    n = R._iso_counts[0]
    g = np.zeros((n, 3), np.float32)
    assert L.exa_hip_isosurface_read(R.h, None, g.ctypes.data, None, 0, None) != 0
    assert "EXA_SAMPLE_GRADIENT" in L.exa_hip_last_error(R.h).decode()
    R.releaseIsoSurface()
    assert L.exa_hip_isosurface_read(R.h, buf.ctypes.data, None, None, 0, None) != 0
    assert R.render().shape == frame.shape
    R.close()


def test_scene_without_kd_tree_is_refused():
    R = without_kd_tree(Case(scenes.amr(levels=3), W=32, H=32)).hip_renderer()
    rc, nv, nt, msg = _raw(R)
    assert rc != 0 and (nv, nt) == (0, 0) and "kd-tree" in msg, msg
    assert R.render().shape == (32, 32)                        # the handle still renders (through its LBVH)
    R.close()


def test_device_read_and_multi_device_handle_equal_the_host_read():
    import torch
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    want = R.isosurface(lo, hi, DIMS, iso, channel=1, gradients=True)
    nv, nt = R.extractIsoSurface(lo, hi, DIMS, iso, channel=1, gradients=True)
    assert (nv, nt) == (len(want[0]), len(want[1]))
    dv = torch.empty((nv, 3), dtype=torch.float32, device="cuda:0")
    dg = torch.empty((nv, 3), dtype=torch.float32, device="cuda:0")
    dt = torch.empty((nt, 3), dtype=torch.int32, device="cuda:0")
    R._check(binding.lib().exa_hip_isosurface_read(R.h, binding._dev_ptr(dv), binding._dev_ptr(dg), binding._dev_ptr(dt), 1, None))
    for x, y in zip((dv, dt, dg), want):
        assert x.cpu().numpy().tobytes() == y.tobytes()
    ms = R.isoSurfaceStageMs()
    assert len(ms) == 6 and all(m >= 0 for m in ms) and ms[0] > 0
    M = multi_handle(R)
    got = M.isosurface(lo, hi, DIMS, iso, channel=1, gradients=True)
    for x, y in zip(got, want):
        assert x.tobytes() == y.tobytes()
    M.close()
    R.close()


def test_c2_lanl_256_cubed():
    sc = scenes.config("c2_lanl")
    R = Case(sc, xf_domains=[(0.0, 1.0)] * len(sc.fields)).hip_renderer()
    lo, hi = R.prep.voxel_bounds()
    dims = (256, 256, 256)
    V = R.resample(lo, hi, dims, fill=NAN)
    iso = _isos(V)[0][1]
    nv, nt = R.extractIsoSurface(lo, hi, dims, iso)
    verts, tris, _ = R.readIsoSurface()
    R.releaseIsoSurface()
    print(f"c2_lanl 256^3 iso {iso!r}: vertices {nv} triangles {nt}")
    assert nt > 100000
    assert ref.repeated_directed_edges(tris) == 0
    assert ref.unreferenced_vertices(nv, tris) == 0
    want_v, want_t = ref.extract(V, lo, hi, iso)
    assert (nv, nt) == (len(want_v), len(want_t))
    assert np.array_equal(_bits(verts), _bits(want_v)) and np.array_equal(tris, want_t)
    R.close()
