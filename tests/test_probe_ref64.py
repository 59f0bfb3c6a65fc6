"""The float64 reference of the reconstruction (tests/probe_ref64.py) on the CPU: its gradient is the derivative of its own
value; the float32 oracle agrees with it within a few roundings of the sums that cancel, in both basis forms, and says "no
sample" exactly where the reference's weights vanish; and scaling a scene by a power of two changes no bit of the oracle's
value and raw numerator (the raw numerator is in per-brick cell units: it does not scale with the cell width)."""
import numpy as np
import pytest

import probe_ref64 as r64
import probe_sets as ps
from common import Case
from owlexabrick_amd import binding, scenes

H = 2.0 ** -10


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _reference(scene, prep, empty=False):
    return r64.Reconstruction(scene, prep.regions(), prep.bricks(), prep.leaflist(), empty)


def oracle_samples(S, pts, owner, chans):
    """the oracle's samplePoint with derivatives at every point that has a region: ok [n, c], value [n, c], numerator [n, c, 3]"""
    n, nc = len(pts), len(chans)
    ok = np.zeros((n, nc), dtype=bool)
    v = np.full((n, nc), np.nan, dtype=np.float32)
    g = np.full((n, nc, 3), np.nan, dtype=np.float32)
    for i in np.nonzero(owner >= 0)[0]:
        for k, c in enumerate(chans):
            ok[i, k], v[i, k], g[i, k] = S.sample_point(int(owner[i]), pts[i], c, True)
    return ok, v, g


@pytest.mark.parametrize("name", ["amr3", "ex4"])
def test_reference_gradient_is_the_derivative_of_its_value(name):
    scene = scenes.amr(levels=3, fields=3) if name == "amr3" else scenes.example("ex4")
    prep = binding.Prep(scene)
    ref = _reference(scene, prep)
    lo, hi = ps.root_box(prep)
    rng = np.random.default_rng(21)
    pts = rng.uniform(lo, hi, (4000, 3)).astype(np.float32)
    owner = ps.brute_owner(prep, pts)
    pts, owner = pts[owner >= 0], owner[owner >= 0]
    chans = tuple(range(len(scene.fields)))
    has = ref.evaluate(pts, owner, chans)["sumW"][:, 0] > r64.STATUS_SUMW      # elsewhere the region has no value
    pts, owner = pts[has], owner[has]
    r = ref.evaluate(pts, owner, chans)
    # the value has kinks on the cell-centre planes and the region changes at a domain face: not differentiable there;
    # nor where sumW reaches zero within 2h along an axis (the edge of the bricks' support: u >= 1/2 below)
    u3 = H * np.abs(r["sumDC"]) / r["sumW"][..., None]
    out = ref.near_a_kink(pts, owner, 2 * H) | np.any(u3 >= 0.5, axis=(1, 2))
    print(f"{name}: {len(pts)} points, {int(out.sum())} ({out.mean():.2%}) within 2h of a kink")
    assert out.mean() <= 0.02
    keep = ~out
    p64 = pts.astype(np.float64)
    worst = 0.0
    for ax in range(3):
        e = np.zeros(3)
        e[ax] = H
        cd = (ref.evaluate(p64 + e, owner, chans)["value"] - ref.evaluate(p64 - e, owner, chans)["value"]) / (2 * H)
        g = r["grad"][..., ax]
        # along an axis, between kinks, sumWV and sumW are linear: value = (a + b x) / (c + d x) with d = sumDC, whose
        # central difference is g / (1 - u^2), u = h d / sumW, exactly.  The rest is the rounding of the two float64 values
        # (a few eps64 of aWV / sumW each: 64 is generous) over 2h.
        u = H * np.abs(r["sumDC"][..., ax]) / r["sumW"]
        assert u[keep].max() < 0.5
        tol = np.abs(g) * (u * u / (1 - u * u)) * (1 + 1e-6) + 64 * 2.0 ** -52 * (r["aWV"] / r["sumW"]) / (2 * H)
        err = np.abs(cd - g)
        assert np.all(err[keep] <= tol[keep]), (ax, float((err[keep] - tol[keep]).max()))
        pos = keep[:, None] & (tol > 0)                               # (a constant field: no error and no allowance)
        worst = max(worst, float((err[pos] / tol[pos]).max()))
    print(f"{name}: largest |central difference - gradient| / allowance {worst:.3g}")
    # the check is not vacuous: gradients of every size, and points where sumW is not 1 (the quotient rule matters)
    assert np.abs(r["grad"][keep]).max() > 1e-3 and (np.abs(r["sumW"][keep] - 1) > 0.01).mean() > 0.05


_oracle_cache = {}


def _oracle_case(idx, form):
    if (idx, form) not in _oracle_cache:
        name, make, forms, empty = ps.REF_CASES[idx]
        case = Case(make(), basis_form=form, allow_empty_cells=empty)
        prep = binding.Prep(case.scene, allow_empty_cells=empty)
        pts = ps.ref_points(prep, idx)
        owner = ps.brute_owner(prep, pts)
        chans = tuple(range(len(case.scene.fields)))
        ref = _reference(case.scene, prep, empty).evaluate(pts, owner, chans)
        ok, v, g = oracle_samples(case.oracle_scene(), pts, owner, chans)
        _oracle_cache[(idx, form)] = (name, prep, pts, owner, ref, ok, v, g)
    return _oracle_cache[(idx, form)]


ORACLE_CASES = [(i, f) for i, c in enumerate(ps.REF_CASES) for f in c[2]]
ORACLE_IDS = [f"{ps.REF_CASES[i][0]}-f{f}" for i, f in ORACLE_CASES]


@pytest.mark.parametrize("idx,form", ORACLE_CASES, ids=ORACLE_IDS)
def test_oracle_says_no_exactly_where_the_weights_vanish(idx, form):
    name, prep, pts, owner, ref, ok, v, g = _oracle_case(idx, form)
    sw = ref["sumW"]
    band = (sw > 0) & (sw < r64.STATUS_BAND)
    assert band.sum() == 0, "pick another seed: float32 may round such a sum to either side"
    has = owner >= 0
    assert np.array_equal(ok[has], sw[has] > r64.STATUS_SUMW)
    assert ok.sum() > 1000 and (~ok[has]).sum() > 0


@pytest.mark.parametrize("idx,form", ORACLE_CASES, ids=ORACLE_IDS)
def test_oracle_against_the_reference(idx, form):
    name, prep, pts, owner, ref, ok, v, g = _oracle_case(idx, form)
    combos = ps.region_levels(prep)
    cls = np.array([ps.level_class(combos[o]) if o >= 0 else "none" for o in owner])
    present = set(ps.level_class(c) for c in combos)
    kv, kg = r64.scaled_errors(ref, v, g)
    assert len(pts) <= 5000 and ok.all(axis=1).sum() > 1000
    for stratum in ("covered", "all"):
        s = ok & r64.stratum(ref, stratum)
        line = f"K {name} form {form} {stratum}: n {int(s.sum())} K_value {kv[s].max():.4g} K_num {kg[s].max():.4g} "
        for what in sorted(present):
            m = s & (cls == what)[:, None]
            assert m.sum() >= 100, (stratum, what)                  # every class of regions the scene has is measured
            line += f" [{what} n {int(m.sum())} K_value {kv[m].max():.3g} K_num {kg[m].max():.3g}]"
        print(line)
        worst = lambda k: (float(np.where(s, k, 0).max()), pts[np.unravel_index(np.argmax(np.where(s, k, 0)), k.shape)[0]])  # noqa: E731
        assert kv[s].max() <= r64.K_VALUE[stratum][form], worst(kv)
        assert kg[s].max() <= r64.K_NUM[stratum][form], worst(kg)
    if name != "gen":                                               # the generated scene refines nowhere at this size
        assert present == {"single", "coarse", "mixed"}


@pytest.mark.parametrize("k", [1, 3])
def test_scaling_by_a_power_of_two_changes_no_bit_of_the_oracle(k):
    A = scenes.amr(levels=3, fields=2)
    B = ps.scaled(A, k)
    pa, pb = binding.Prep(A), binding.Prep(B)
    s = np.float32(2 ** k)
    # the region tables scale exactly
    ra, rb = pa.regions(), pb.regions()
    assert np.array_equal(np.stack(list(ra["dom_lo"])) * s, np.stack(list(rb["dom_lo"])))
    assert np.array_equal(np.stack(list(ra["dom_hi"])) * s, np.stack(list(rb["dom_hi"])))
    assert np.array_equal(ra["leafListBegin"], rb["leafListBegin"]) and np.array_equal(ra["leafListSize"], rb["leafListSize"])
    assert np.array_equal(pa.leaflist(), pb.leaflist())
    rng = np.random.default_rng(30 + k)
    lo, hi = ps.root_box(pa, grow=0.02)
    pts = np.concatenate([rng.uniform(lo, hi, (400, 3)).astype(np.float32), ps.level_points(pa, 400, seed=k)])
    owner = ps.brute_owner(pa, pts)
    assert np.array_equal(owner, ps.brute_owner(pb, pts * s))
    for form in (0, 1):
        a = oracle_samples(Case(A, basis_form=form).oracle_scene(), pts, owner, (0, 1))
        b = oracle_samples(Case(B, basis_form=form).oracle_scene(), pts * s, owner, (0, 1))
        assert np.array_equal(a[0], b[0]) and a[0].sum() > 1000
        assert np.array_equal(_bits(a[1]), _bits(b[1]))
        assert np.array_equal(_bits(a[2]), _bits(b[2]))       # NOT halved: the numerator is in cell units of each brick
        assert np.abs(a[2][a[0]]).max() > 1e-3
