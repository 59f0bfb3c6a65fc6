"""The derived flow quantities on the GPU (exa_hip_sample_derived, exa_hip_resample_derived, exa_hip_isosurface_derived;
include/exa_hip.h states the contract): the composition of the points probe with the table of tests/derived_ref.py bit for
bit, the lattice against the points, the surface against tests/isomesh_ref.py, a float64 reference with a derived allowance,
exact scaling by powers of two, independence of what a frame sets, and the errors."""
import ctypes as C
import math

import numpy as np
import pytest

import derived_ref as dr
import isomesh_ref
import probe_ref64 as r64
import probe_sets as ps
from analysis_steps import bits, frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes

pytestmark = pytest.mark.gpu

NAN = float("nan")
FILL = np.float32(-12345.5)
DIMS = (37, 29, 23)
XFM = dict(vx=[1.6, 0.5, -0.2], vy=[-0.4, 1.3, 0.3], vz=[0.25, -0.15, 0.9], p=[3.5, -1.25, 2.0])     # not axis-aligned
WORLD_BOX = (np.array([-4, -6, -5], np.float32), np.array([30, 24, 26], np.float32))
NAMES = sorted(dr.QUANTITIES, key=dr.QUANTITIES.get)


def _amr3():
    return scenes.amr(levels=3, fields=3)


# ---- 1. composition, bit for bit ----
def _ex4_two_fields():
    """ex4 (one field) with a second one, so that channels (0, 1, 0) exist"""
    return scenes.with_extra_field(scenes.example("ex4"), lambda c: 0.5 + 0.5 * np.sin(0.7 * c[:, 0] + 0.4 * c[:, 1] - 0.9 * c[:, 2]))


# (name of the scene in probe_sets.REF_CASES, its index there (the points' seed), basis forms, channels, another make or None)
COMPOSE = [("amr3", 2, (0, 1), (0, 1, 2), None), ("amr3_offset", 3, (0, 1), (0, 1, 2), None),
           ("ex4", 1, (0, 1), (0, 1, 0), _ex4_two_fields), ("amr3_holes", 5, (0,), (0, 1, 1), None)]
COMPOSE_CASES = [(c, f) for c in COMPOSE for f in c[2]]


def _compose_points(prep, idx):
    lo, hi = ps.root_box(prep)
    ext = hi - lo
    outside = np.array([lo - 0.5 * ext, hi + 0.5 * ext, [lo[0] - 1, hi[1], hi[2]], [hi[0], hi[1], hi[2] + 0.25]], np.float32)
    odd = np.array([[np.nan, lo[1], lo[2]], [lo[0], np.inf, lo[2]]], np.float32)
    # ref_points holds points on region faces (probe_points); a few more on the lower and upper faces of the regions
    dom = ps.domains(prep)
    mid = 0.5 * (dom[:, :3] + dom[:, 3:])
    faces = np.concatenate([np.concatenate([dom[:, :1], mid[:, 1:]], axis=1), np.concatenate([mid[:, :2], dom[:, 5:6]], axis=1)])
    return np.ascontiguousarray(np.concatenate([ps.ref_points(prep, idx), outside, odd, faces[:400]]).astype(np.float32))


def _check_composition(R, pts, channels, world=False):
    """every quantity at pts against derived_ref on samplePoints of the same handle; returns the status"""
    v, g, st = R.samplePoints(pts, channels=channels, gradient=True, normalized=True, world=world, fill=FILL)
    status = None
    for name in NAMES:
        q = dr.QUANTITIES[name]
        want, want_st = dr.from_probe(q, v, g, st, FILL)
        got, got_st = R.sampleDerived(pts, name, channels=channels, world=world, fill=FILL)
        assert got.shape == want.shape and got.dtype == np.float32, (name, got.shape, want.shape)
        assert np.array_equal(got_st, want_st), (name, np.nonzero(got_st != want_st)[0][:10])
        assert np.array_equal(bits(got), bits(want)), (name, np.nonzero(bits(got) != bits(want))[0][:10])
        assert np.all(bits(got[got_st < 0]) == bits(FILL)), name
        got_n, st_n = R.sampleDerived(pts, q, channels=channels, world=world, fill=FILL)         # by number
        assert np.array_equal(bits(got_n), bits(got)) and np.array_equal(st_n, got_st), name
        status = got_st
    return status


@pytest.mark.parametrize("case,form", COMPOSE_CASES, ids=[f"{c[0]}-f{f}" for c, f in COMPOSE_CASES])
def test_every_quantity_is_the_table_applied_to_the_points_probe(case, form):
    name, idx, _, channels, other = case
    _, make, _, empty = ps.REF_CASES[idx]
    assert ps.REF_CASES[idx][0] == name
    R = Case((other or make)(), basis_form=form, allow_empty_cells=empty).hip_renderer()
    pts = _compose_points(R.prep, idx)
    assert len(pts) <= 25000
    st = _check_composition(R, pts, channels)
    assert (st == -1).sum() > 0 and (st >= 0).sum() > 0
    if name == "amr3_holes":
        assert (st == -2).sum() > 0
    print(f"{name} form {form}: points {len(pts)} with a value {(st >= 0).sum()} no region {(st == -1).sum()} no weight {(st == -2).sum()}")
    R.close()


def test_device_pointers_and_timing():
    import torch
    R = Case(_amr3()).hip_renderer()
    assert R.derivedMs() == 0.0
    pts = _compose_points(R.prep, 2)
    want, want_st = R.sampleDerived(pts, "vorticity", fill=FILL)
    assert R.derivedMs() > 0.0
    d = torch.from_numpy(pts).to("cuda:0")
    got, st = R.sampleDerived(d, "vorticity", fill=FILL)
    assert R.derivedMs() > 0.0
    assert got.cpu().numpy().tobytes() == want.tobytes() and st.cpu().numpy().tobytes() == want_st.tobytes()
    lo, hi = ps.root_box(R.prep, grow=0.1)
    V = R.resampleDerived(lo, hi, DIMS, "vorticity", fill=FILL)
    assert V.shape == DIMS[::-1] + (3,) and R.derivedMs() > 0.0
    out = torch.empty(DIMS[::-1] + (3,), dtype=torch.float32, device="cuda:0")
    R.resampleDerived(lo, hi, DIMS, "vorticity", fill=FILL, out_ptr=out)
    assert out.cpu().numpy().tobytes() == V.tobytes()
    got0, st0 = R.sampleDerived(np.zeros((0, 3), np.float32), "q")          # n == 0 does nothing
    assert got0.shape == (0,) and st0.shape == (0,)
    with pytest.raises(RuntimeError, match="exa_hip_sample_derived"):
        R.sampleDerived(pts, 17)
    assert R.derivedMs() == 0.0                                             # after a refused call
    R.close()


# ---- 2. grid == points ----
@pytest.mark.parametrize("world", [False, True], ids=["voxel", "world"])
def test_lattice_equals_the_points_in_every_patch_shape(world):
    R = Case(_amr3()).hip_renderer()
    if world:
        R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lo, hi = WORLD_BOX if world else ps.root_box(R.prep, grow=0.1)
    for dims in (DIMS, (1, 1, 1), (65, 3, 2)):
        pos = ps.grid_positions(lo, hi, dims)
        for name in ("q", "vorticity"):
            want, st = R.sampleDerived(pos, name, world=world, fill=FILL)
            if dims == DIMS:
                assert (st >= 0).sum() > 1000 and (st == -1).sum() > 100, (world, (st >= 0).sum(), (st == -1).sum())
            for patch in range(4):
                for uniform in (0, 1):
                    R.setOption("sample_patch", patch)
                    R.setOption("sample_uniform", uniform)
                    got = R.resampleDerived(lo, hi, dims, name, world=world, fill=FILL)
                    assert got.shape == dims[::-1] + ((3,) if name == "vorticity" else ())
                    assert got.tobytes() == want.tobytes(), (world, dims, name, patch, uniform)
    R.close()


# ---- 3. the surface ----
def _median(V):
    fin = V[np.isfinite(V)]
    assert fin.size > 100
    return float(np.float32(np.median(fin)))


def test_surfaces_of_q_and_vorticity_magnitude_equal_the_restatement():
    R = Case(_amr3()).hip_renderer()
    L = binding.lib()
    lo, hi = ps.root_box(R.prep, grow=0.1)
    for name in ("q", "vorticity_magnitude"):
        V = R.resampleDerived(lo, hi, DIMS, name, fill=NAN)
        assert np.isnan(V).any()
        iso = _median(V)
        want_v, want_t = isomesh_ref.extract(V, lo, hi, iso)
        verts, tris = R.isosurfaceDerived(lo, hi, DIMS, iso, name)
        print(f"{name}: iso {iso!r} vertices {len(verts)} triangles {len(tris)}")
        assert len(tris) >= 500
        assert verts.tobytes() == want_v.astype(np.float32).tobytes() and tris.tobytes() == want_t.astype(np.int32).tobytes(), name
    # the mesh stays for the shared read; it has no gradients; a channel's surface replaces it
    nv, nt = R.extractIsoSurfaceDerived(lo, hi, DIMS, iso, "vorticity_magnitude")
    assert (nv, nt) == (len(verts), len(tris))
    g = np.zeros((nv, 3), np.float32)
    assert L.exa_hip_isosurface_read(R.h, None, g.ctypes.data, None, 0, None) != 0
    assert "EXA_SAMPLE_GRADIENT" in L.exa_hip_last_error(R.h).decode()
    ms = R.isoSurfaceStageMs()
    assert len(ms) == 6 and ms[0] > 0
    Vc = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    isoc = _median(Vc)
    cv, ct, _ = R.isosurface(lo, hi, DIMS, isoc, channel=1)
    assert len(ct) > 0 and cv.tobytes() != verts.tobytes()
    nv2, nt2 = R.extractIsoSurface(lo, hi, DIMS, isoc, channel=1)
    v2, t2, _ = R.readIsoSurface()
    assert (nv2, nt2) == (len(cv), len(ct)) and v2.tobytes() == cv.tobytes() and t2.tobytes() == ct.tobytes()
    R.releaseIsoSurface()
    R.close()


# ---- 4. the float64 reference ----
# A quantity in float64 with a bound of the float32 result's error beside it: pairs (value, error) go through the formula.
# Inputs carry the bounds the project already holds (the value's from K_VALUE, a Jacobian entry's from normalized_bound with
# K_NUM); every operation propagates its operands' errors (exactly for + and -, with the second-order term for *, by the
# concavity of the root for sqrt) and adds one float32 rounding of its own result.
EPS = r64.EPS32


def _rounded(val, err):
    return val, err + EPS * (np.abs(val) + err)


def _add(a, b):
    return _rounded(a[0] + b[0], a[1] + b[1])


def _sub(a, b):
    return _rounded(a[0] - b[0], a[1] + b[1])


def _mul(a, b):
    return _rounded(a[0] * b[0], np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])


def _sqrt(a):
    root = np.sqrt(a[0])
    return _rounded(root, np.maximum(root - np.sqrt(np.maximum(a[0] - a[1], 0.0)), np.sqrt(a[0] + a[1]) - root))


def _bounded(q, v, J):
    """v[c], J[c][k]: pairs of [n] arrays -> the quantity's pairs, one per component"""
    w = [_sub(J[2][1], J[1][2]), _sub(J[0][2], J[2][0]), _sub(J[1][0], J[0][1])]
    if q == dr.SPEED:
        return [_sqrt(_add(_add(_mul(v[0], v[0]), _mul(v[1], v[1])), _mul(v[2], v[2])))]
    if q == dr.DIVERGENCE:
        return [_add(_add(J[0][0], J[1][1]), J[2][2])]
    if q == dr.VORTICITY:
        return w
    if q == dr.VORTICITY_MAGNITUDE:
        return [_sqrt(_add(_add(_mul(w[0], w[0]), _mul(w[1], w[1])), _mul(w[2], w[2])))]
    if q == dr.Q:
        d = _add(_add(_mul(J[0][0], J[0][0]), _mul(J[1][1], J[1][1])), _mul(J[2][2], J[2][2]))
        o = _add(_add(_mul(J[0][1], J[1][0]), _mul(J[0][2], J[2][0])), _mul(J[1][2], J[2][1]))
        half = (-0.5 * d[0], 0.5 * d[1])                           # times a power of two: exact
        return [_sub(half, o)]
    return [_add(_add(_mul(v[0], w[0]), _mul(v[1], w[1])), _mul(v[2], w[2]))]


@pytest.mark.parametrize("form", [0, 1])
def test_quantities_against_the_float64_reference(form):
    case = Case(_amr3(), basis_form=form)
    R = case.hip_renderer()
    pts = ps.ref_points(R.prep, 2)
    owner = ps.brute_owner(R.prep, pts)
    recon = r64.Reconstruction(case.scene, R.prep.regions(), R.prep.bricks(), R.prep.leaflist(), False)
    ref = recon.evaluate(pts, owner, (0, 1, 2))
    sw = ref["sumW"]
    assert ((sw > 0) & (sw < r64.STATUS_BAND)).sum() == 0
    has = (owner >= 0) & np.all(sw > r64.STATUS_SUMW, axis=1)
    combos = ps.region_levels(R.prep)
    cls = np.array([ps.level_class(combos[o]) if o >= 0 else "none" for o in owner])
    for what in ("single", "coarse", "mixed"):
        assert (has & (cls == what)).sum() >= 100, what
    worst = {}
    for stratum in ("covered", "all"):
        m = has & np.all(r64.stratum(ref, stratum), axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            ev = r64.K_VALUE[stratum][form] * EPS * ref["aWV"] / sw
            eg = r64.normalized_bound(ref, r64.K_NUM[stratum][form])
        v = [(ref["value"][m, c], ev[m, c]) for c in range(3)]
        J = [[(ref["grad"][m, c, k], eg[m, c, k]) for k in range(3)] for c in range(3)]
        for name in NAMES:
            q = dr.QUANTITIES[name]
            got, st = R.sampleDerived(pts, name, fill=FILL)
            assert np.array_equal(st >= 0, has)
            got = got.reshape(len(pts), -1)[m].astype(np.float64)
            want64 = dr.derived(q, ref["value"][m], ref["grad"][m], dtype=np.float64).reshape(len(got), -1)
            ratio = 0.0
            for c, (val, tol) in enumerate(_bounded(q, v, J)):
                assert np.array_equal(val, want64[:, c])                  # the pairs' values are derived_ref in float64
                err = np.abs(got[:, c] - val)
                with np.errstate(divide="ignore", invalid="ignore"):
                    ratio = max(ratio, float(np.where(err == 0, 0.0, err / tol).max()))
            worst[(name, stratum)] = ratio
            print(f"amr3 form {form} {name} {stratum}: n {int(m.sum())} largest error / allowance {ratio:.3g}")
    assert all(r <= 1.0 for r in worst.values()), worst
    R.close()


# ---- 5. scaling by a power of two ----
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("form", [0, 1])
def test_scaling_by_a_power_of_two_is_exact(form, k):
    A = _amr3()
    RA = Case(A, basis_form=form).hip_renderer()
    RB = Case(ps.scaled(A, k), basis_form=form).hip_renderer()
    s = np.float32(2 ** k)
    rng = np.random.default_rng(50 + k)
    lo, hi = ps.root_box(RA.prep, grow=0.02)
    pts = np.concatenate([rng.uniform(lo, hi, (400, 3)).astype(np.float32), ps.level_points(RA.prep, 400, seed=k)])
    tiny = np.finfo(np.float32).tiny
    for name in NAMES:
        a, sa = RA.sampleDerived(pts, name, fill=NAN)
        b, sb = RB.sampleDerived(pts * s, name, fill=NAN)
        assert np.array_equal(sa, sb) and (sa >= 0).sum() > 700
        div = np.float32(1) if name == "speed" else (s * s if name == "q" else s)
        want = a / div                                                     # a division by a power of two: exact where normal
        normal = (sa >= 0).reshape((-1,) + (1,) * (a.ndim - 1)) & np.isfinite(a) & (np.abs(want) >= tiny)
        assert normal.sum() > 700 * (3 if a.ndim == 2 else 1) // 2, (name, int(normal.sum()))
        assert np.array_equal(bits(b)[normal], bits(want)[normal]), (name, int((bits(b)[normal] != bits(want)[normal]).sum()))
    RA.close()
    RB.close()


# ---- 6. nothing else moves it ----
def test_results_do_not_depend_on_what_a_frame_sets():
    case = Case(_amr3(), W=32, H=32, basis_form=1)
    R = case.hip_renderer()
    lo, hi = ps.root_box(R.prep, grow=0.1)
    want_grid = R.resampleDerived(lo, hi, DIMS, "vorticity", fill=FILL)
    iso = _median(R.resampleDerived(lo, hi, DIMS, "q", fill=NAN))
    want_mesh = R.isosurfaceDerived(lo, hi, DIMS, iso, "q")
    assert len(want_mesh[1]) >= 500

    def same(what, H=R):
        assert H.resampleDerived(lo, hi, DIMS, "vorticity", fill=FILL).tobytes() == want_grid.tobytes(), what
        for x, y in zip(H.isosurfaceDerived(lo, hi, DIMS, iso, "q"), want_mesh):
            assert x.tobytes() == y.tobytes(), what

    same("two consecutive calls")
    for what in frame_perturbations(case, R):
        same(what)
    rng = np.random.default_rng(7)
    for c in range(3):                                                      # another transfer function
        R.updateXF(c, rng.random(128).astype(np.float32), case.xfs[c][:, :3], (0.25, 0.5), 3.0)
    R.render()
    same("another transfer function")
    M = multi_handle(R, form=1)
    same("a multi-device handle", M)
    M.close()
    R.close()


def _raw_sample(R, pts=None, n=None, channels=(0, 1, 2), quantity=dr.Q, flags=0, out=True):
    pts = np.zeros((4, 3), np.float32) if pts is None else pts
    res = np.zeros((len(pts), 3), np.float32)
    rc = binding.lib().exa_hip_sample_derived(R.h, pts.ctypes.data if len(pts) else None, len(pts) if n is None else n,
                                              (C.c_int32 * 3)(*channels) if channels is not None else None, quantity, flags,
                                              0.0, res.ctypes.data if out else None, None, 0, None, 0)
    return rc, binding.lib().exa_hip_last_error(R.h).decode()


def _raw_resample(R, lo=(0, 0, 0), hi=(8, 8, 8), dims=(9, 9, 9), channels=(0, 1, 2), quantity=dr.Q, flags=0, out=True):
    res = np.zeros(max(int(np.prod(np.maximum(dims, 1))), 1) * 3, np.float32)
    rc = binding.lib().exa_hip_resample_derived(R.h, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*dims),
                                                (C.c_int32 * 3)(*channels) if channels is not None else None, quantity, flags,
                                                0.0, res.ctypes.data if out else None, 0, None, 0)
    return rc, binding.lib().exa_hip_last_error(R.h).decode()


def _raw_iso(R, lo=(0, 0, 0), hi=(8, 8, 8), dims=(9, 9, 9), channels=(0, 1, 2), quantity=dr.Q, iso=0.0, flags=0):
    nv, nt = C.c_uint64(77), C.c_uint64(77)
    rc = binding.lib().exa_hip_isosurface_derived(R.h, (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*dims),
                                                  (C.c_int32 * 3)(*channels) if channels is not None else None, quantity, iso,
                                                  flags, C.byref(nv), C.byref(nt), None)
    return rc, binding.lib().exa_hip_last_error(R.h).decode(), int(nv.value), int(nt.value)


def test_scene_without_kd_tree_is_refused():
    R = without_kd_tree(Case(_amr3(), W=32, H=32)).hip_renderer()
    for fn, (rc, msg, *_) in (("exa_hip_sample_derived", _raw_sample(R)), ("exa_hip_resample_derived", _raw_resample(R)),
                              ("exa_hip_isosurface_derived", _raw_iso(R))):
        assert rc != 0 and msg.startswith(fn + ": ") and "the scene has no region kd-tree" in msg, (fn, msg)
    assert R.render().shape == (32, 32)
    R.close()


# ---- 7. errors ----
def test_refused_arguments_leave_the_handle_usable():
    R = Case(_amr3(), W=32, H=32).hip_renderer()                    # no render yet: the module holds no frame state
    W = binding.SAMPLE_WORLD_SPACE
    calls = {"exa_hip_sample_derived": _raw_sample, "exa_hip_resample_derived": _raw_resample, "exa_hip_isosurface_derived": _raw_iso}
    for fn, raw in calls.items():
        rc, msg, *_ = raw(R, flags=W)
        assert rc != 0 and msg.startswith(fn + ": ") and "frame state" in msg, (fn, msg)
    frame = R.render()
    common = [dict(quantity=6), dict(quantity=-1), dict(quantity=1 << 20), dict(channels=(0, 1, 3)), dict(channels=(-1, 1, 2)),
              dict(channels=None), dict(flags=4), dict(flags=8), dict(flags=1 << 30)]
    box = [dict(hi=(8, 0, 8)), dict(lo=(math.nan, 0, 0)), dict(hi=(math.inf, 8, 8)), dict(dims=(9, 0, 9)), dict(dims=(9, -3, 9))]
    bad = {"exa_hip_sample_derived": common + [dict(flags=2), dict(flags=2 | 4), dict(out=False), dict(pts=np.zeros((0, 3), np.float32), n=4)],
           "exa_hip_resample_derived": common + box + [dict(flags=2), dict(out=False)],
           "exa_hip_isosurface_derived": common + box + [dict(flags=2), dict(dims=(1, 9, 9)), dict(iso=math.nan), dict(iso=math.inf),
                                                         dict(quantity=dr.VORTICITY), dict(dims=(2 ** 11, 2 ** 11, 2 ** 10))]}
    for fn, raw in calls.items():
        for kw in bad[fn]:
            rc, msg, *counts = raw(R, **kw)
            assert rc != 0 and msg.startswith(fn + ": "), (fn, kw, rc, msg)
            assert counts in ([], [0, 0]), (fn, kw, counts)
        assert R.render().shape == frame.shape, fn                 # the handle still renders
    assert R.derivedMs() == 0.0
    # ... and still answers: the composition of check 1
    st = _check_composition(R, _compose_points(R.prep, 2), (0, 1, 2))
    assert (st >= 0).sum() > 0
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    rng = np.random.default_rng(3)
    st = _check_composition(R, rng.uniform(*WORLD_BOX, (3000, 3)).astype(np.float32), (2, 0, 1), world=True)
    assert (st >= 0).sum() > 300 and (st == -1).sum() > 300
    with pytest.raises(ValueError):
        R.sampleDerived(np.zeros((1, 3), np.float32), "lambda2")
    R.close()
