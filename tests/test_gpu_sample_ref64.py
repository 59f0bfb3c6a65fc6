"""The point probes and the iso-surface gradients on the GPU against the float64 reference of the reconstruction
(tests/probe_ref64.py): status, value, raw numerator and the normalized (voxel-space) gradient, in single-level, coarse and
mixed-level regions, within the bounds measured for the float32 operation order on the CPU (K_VALUE, K_NUM); and the exact
behaviour under a scaling of the scene by a power of two: values and raw numerators keep every bit, the normalized
gradient is divided by the factor.

Before the normalized gradient took each brick's derivative weights in voxel units (2^-level), the normalized parts of
these tests failed: 2^L too large in regions of level L, a mixture in mixed regions, and equal instead of halved under
scaling.  Values and raw numerators passed then as now."""
import numpy as np
import pytest

import probe_ref64 as r64
import probe_sets as ps
from common import Case
from owlexabrick_amd import scenes

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.5)
NAN = float("nan")
GRID = (24, 20, 16)
ISO_DIMS = (37, 29, 23)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _reference(case, prep):
    return r64.Reconstruction(case.scene, prep.regions(), prep.bricks(), prep.leaflist(), case.allow_empty_cells)


def _classes(prep, owner):
    combos = ps.region_levels(prep)
    return np.array([ps.level_class(combos[o]) if o >= 0 else "none" for o in owner]), set(ps.level_class(c) for c in combos)


def _check_status(st, owner, ref):
    """-1 exactly where no region owns the point, else the region, or -2 exactly where the float64 weights vanish"""
    sw = ref["sumW"]
    assert ((sw > 0) & (sw < r64.STATUS_BAND)).sum() == 0, "pick another seed: float32 may round such a sum to either side"
    has = (owner >= 0)[:, None] & (sw > r64.STATUS_SUMW)
    want = np.where(has, owner[:, None], np.where((owner >= 0)[:, None], -2, -1))
    assert np.array_equal(st, want), np.nonzero(st != want)[0][:10]
    return has


def _check_normalized(gn, ref, has, form, what):
    err = np.abs(gn.astype(np.float64) - ref["grad"])
    for stratum in ("covered", "all"):
        m = has & r64.stratum(ref, stratum)
        tol = r64.normalized_bound(ref, r64.K_NUM[stratum][form])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err == 0, 0.0, err / tol)[m]
        print(f"{what} {stratum}: n {int(m.sum())} largest |normalized - gradient| / allowance {ratio.max():.3g}")
        assert np.all(err[m] <= tol[m]), (what, stratum, float(ratio.max()))


CASES = [(i, f) for i, c in enumerate(ps.REF_CASES) for f in c[2]]


@pytest.mark.parametrize("idx,form", CASES, ids=[f"{ps.REF_CASES[i][0]}-f{f}" for i, f in CASES])
def test_probe_against_the_float64_reference(idx, form):
    name, make, forms, empty = ps.REF_CASES[idx]
    check_probe_against_the_float64_reference(Case(make(), basis_form=form, allow_empty_cells=empty), name, form, idx)


def check_probe_against_the_float64_reference(case, name, form, idx):
    """the probes of `case`'s scene at ps.ref_points (seeded by idx) and on a lattice against tests/probe_ref64.py: status
    rule, K_VALUE, K_NUM, the normalized bound (shared with tests/test_gpu_translation.py, which moves the scene)"""
    R = case.hip_renderer()
    pts = ps.ref_points(R.prep, idx)
    assert len(pts) <= 5000
    owner = ps.brute_owner(R.prep, pts)
    chans = tuple(range(len(case.scene.fields)))
    recon = _reference(case, R.prep)
    ref = recon.evaluate(pts, owner, chans)
    v, g, st = R.samplePoints(pts, channels=chans, gradient=True, fill=FILL)
    vn, gn, stn = R.samplePoints(pts, channels=chans, gradient=True, normalized=True, fill=FILL)
    has = _check_status(st, owner, ref)
    assert np.array_equal(stn, st) and np.array_equal(_bits(vn), _bits(v))
    assert np.all(_bits(v[~has]) == _bits(FILL)) and np.all(_bits(g[~has]) == _bits(FILL)) and np.all(_bits(gn[~has]) == _bits(FILL))
    cls, present = _classes(R.prep, owner)
    if name != "gen":                                               # the generated scene refines nowhere at this size
        assert present == {"single", "coarse", "mixed"}
    for what in present:
        assert (has & (cls == what)[:, None]).sum() >= 100, what
    kv, kg = r64.scaled_errors(ref, v, g)
    for stratum in ("covered", "all"):
        m = has & r64.stratum(ref, stratum)
        print(f"K {name} form {form} {stratum}: n {int(m.sum())} K_value {kv[m].max():.4g} K_num {kg[m].max():.4g}")
        assert kv[m].max() <= r64.K_VALUE[stratum][form], (stratum, float(kv[m].max()))
        assert kg[m].max() <= r64.K_NUM[stratum][form], (stratum, float(kg[m].max()))
    _check_normalized(gn, ref, has, form, f"{name} form {form}")
    # the lattice of exa_hip_resample over the grown root box
    lo, hi = ps.root_box(R.prep, grow=0.1)
    c = len(chans) - 1
    V = R.resample(lo, hi, GRID, channel=c, fill=FILL).reshape(-1)
    pos = ps.grid_positions(lo, hi, GRID)
    gown = ps.brute_owner(R.prep, pos)
    gref = recon.evaluate(pos, gown, (c,))
    sw = gref["sumW"][:, 0]
    assert ((sw > 0) & (sw < r64.STATUS_BAND)).sum() == 0
    ghas = (gown >= 0) & (sw > r64.STATUS_SUMW)
    assert np.all(_bits(V[~ghas]) == _bits(FILL)) and ghas.sum() > 1000 and (~ghas).sum() > 0
    gkv, _ = r64.scaled_errors(gref, V[:, None], np.zeros((len(V), 1, 3)))
    for stratum in ("covered", "all"):
        m = ghas & r64.stratum(gref, stratum)[:, 0]
        print(f"K {name} form {form} lattice {stratum}: n {int(m.sum())} K_value {gkv[m, 0].max():.4g}")
        assert gkv[m, 0].max() <= r64.K_VALUE[stratum][form], (stratum, float(gkv[m, 0].max()))
    R.close()


def _median_iso(V):
    fin = V[np.isfinite(V)]
    assert fin.size > 100
    return float(np.float32(np.median(fin)))


@pytest.mark.parametrize("form", [0, 1])
def test_isosurface_gradients_against_the_float64_reference(form):
    case = Case(scenes.amr(levels=3, fields=2), basis_form=form)
    R = case.hip_renderer()
    lo, hi = ps.root_box(R.prep, grow=0.1)
    iso = _median_iso(R.resample(lo, hi, ISO_DIMS, channel=1, fill=NAN))
    verts, tris, grads = R.isosurface(lo, hi, ISO_DIMS, iso, channel=1, gradients=True)
    assert len(tris) >= 500 and grads.shape == verts.shape
    owner = ps.brute_owner(R.prep, verts)
    ref = _reference(case, R.prep).evaluate(verts, owner, (1,))
    has = (owner >= 0)[:, None] & (ref["sumW"] > r64.STATUS_SUMW)
    assert np.array_equal(np.isnan(grads).any(axis=1), ~has[:, 0]) and has.mean() > 0.9      # the fill, by the status rule
    cls, _ = _classes(R.prep, owner)
    print("vertices per class:", {k: int((cls == k).sum()) for k in ("single", "coarse", "mixed")})
    assert (cls == "coarse").sum() >= 100 and (cls == "mixed").sum() >= 100
    _check_normalized(grads[:, None, :], ref, has, form, f"iso-surface form {form}")
    R.close()


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("form", [0, 1])
def test_scaling_by_a_power_of_two_is_exact(form, k):
    A = scenes.amr(levels=3, fields=2)
    RA = Case(A, basis_form=form).hip_renderer()
    RB = Case(ps.scaled(A, k), basis_form=form).hip_renderer()
    s = np.float32(2 ** k)
    rng = np.random.default_rng(30 + k)
    lo, hi = ps.root_box(RA.prep, grow=0.02)
    pts = np.concatenate([rng.uniform(lo, hi, (400, 3)).astype(np.float32), ps.level_points(RA.prep, 400, seed=k)])
    a = RA.samplePoints(pts, channels=(0, 1), gradient=True, fill=FILL)
    b = RB.samplePoints(pts * s, channels=(0, 1), gradient=True, fill=FILL)
    assert np.array_equal(a[2], b[2]) and (a[2] >= 0).sum() > 1000 and (a[2] < 0).sum() > 0
    assert np.array_equal(_bits(a[0]), _bits(b[0]))
    assert np.array_equal(_bits(a[1]), _bits(b[1]))               # the numerator is in each brick's cell units: unchanged
    an = RA.samplePoints(pts, channels=(0, 1), gradient=True, normalized=True, fill=NAN)
    bn = RB.samplePoints(pts * s, channels=(0, 1), gradient=True, normalized=True, fill=NAN)
    assert np.array_equal(an[2], a[2]) and np.array_equal(bn[2], a[2])
    ok = an[2] >= 0
    assert np.abs(an[1][ok]).max() > 1e-3 and np.isnan(an[1][~ok]).all() and np.isnan(bn[1][~ok]).all()
    assert np.array_equal(_bits(bn[1][ok]), _bits(an[1][ok] / s))  # the gradient in voxel space: divided by 2^k, exactly
    # the mesh on the scaled lattice: the same surface, its positions scaled, its gradients divided
    loi, hii = ps.root_box(RA.prep, grow=0.1)
    iso = _median_iso(RA.resample(loi, hii, ISO_DIMS, channel=1, fill=NAN))
    va, ta, ga = RA.isosurface(loi, hii, ISO_DIMS, iso, channel=1, gradients=True)
    vb, tb, gb = RB.isosurface(loi * s, hii * s, ISO_DIMS, iso, channel=1, gradients=True)
    assert len(ta) >= 500 and np.array_equal(ta, tb)
    assert np.array_equal(_bits(vb), _bits(va * s))
    fin = np.isfinite(ga)
    assert fin.mean() > 0.9 and np.array_equal(np.isfinite(gb), fin) and np.array_equal(_bits(gb[fin]), _bits(ga[fin] / s))
    RA.close()
    RB.close()
