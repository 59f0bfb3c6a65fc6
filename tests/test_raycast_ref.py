"""tests/raycast_ref.py, the numpy restatement of exa_hip_raycast_iso's contract, on the CPU with analytic samplers rounded to
float32: the crossings, the side, the refinement's brackets and the edge cases of the contract (tests/test_gpu_raycast.py
holds the kernel to this restatement bit for bit)."""
import numpy as np

import project_ref as pr
import raycast_ref as rr

f32 = np.float32
N = 48


def analytic(fn, grad=None, bad=None):
    """a sampler of fn(points as float64) rounded to float32; status 0, -1 where bad(points) says so or a coordinate is not
    finite; the gradient call returns grad(points), or zeros"""
    def sample(points, gradient=False):
        p = np.asarray(points, dtype=f32).astype(np.float64)
        with np.errstate(all="ignore"):
            v = np.asarray(fn(p), dtype=np.float64).astype(f32)
        st = np.zeros(len(p), dtype=np.int32)
        st[~np.isfinite(p).all(axis=1)] = -1
        if bad is not None:
            st[bad(p)] = -1
        if not gradient:
            return v, st
        g = np.asarray(grad(p), dtype=f32) if grad is not None else np.zeros((len(p), 3), f32)
        return v, g, st
    return sample


def z_rays(size=(5, 3), tmin=0.0, dt=0.5, n=N):
    """rays along +z from the plane z = 0, one unit apart: p.z = t exactly"""
    return pr.rays((0, 0, 0), (0, 0, 1), size, tmin, dt, n, orgDu=(1, 0, 0), orgDv=(0, 1, 0))


def plain(ta, va, tb, vb, iso):
    s = (f32(iso) - f32(va)) / (f32(vb) - f32(va))
    return f32(ta) + s * (f32(tb) - f32(ta))


def test_a_linear_field_has_one_crossing_at_the_expected_index():
    r = z_rays()
    t = pr.times(r)
    for slope, want_side in ((2.0, 1), (-2.0, -1)):
        # zero at z = 5: between t_9 = 4.75 and t_10 = 5.25
        res, info = rr.raycast(analytic(lambda p: slope * (p[:, 2] - 5.0), grad=lambda p: np.tile([0, 0, slope], (len(p), 1))),
                               r, 0.0, 0)
        assert (res["crossings"] == 1).all() and (res["index"] == 10).all() and (res["side"] == want_side).all()
        want = plain(t[9], slope * -0.25, t[10], slope * 0.25, 0.0)
        assert want == f32(5.0)
        assert rr.same_bits(res["t"], np.full((3, 5), want, f32))
        assert np.array_equal(res["position"][..., 2], res["t"])
        assert np.array_equal(res["value"], np.zeros((3, 5), f32)) and (res["gradient"][..., 2] == f32(slope)).all()
        # the refinement of a linear field stays on the same t
        fine, _ = rr.raycast(analytic(lambda p: slope * (p[:, 2] - 5.0)), r, 0.0, 12)
        assert np.array_equal(fine["t"], res["t"]) and np.array_equal(fine["index"], res["index"])


def _sphere():
    c, radius = np.array([7.3, 5.1, 11.2]), 4.0
    r = pr.rays((0, 0, 0), (0.02, -0.01, 1), (16, 12), 0.0, 0.5, N, orgDu=(1, 0, 0), orgDv=(0, 1, 0))
    fn = lambda p: np.sqrt(((p - c) ** 2).sum(axis=1))                    # noqa: E731
    grad = lambda p: (p - c) / np.sqrt(((p - c) ** 2).sum(axis=1))[:, None]   # noqa: E731
    return r, analytic(fn, grad), c, radius


def test_a_sphere_is_entered_and_left():
    r, sample, c, radius = _sphere()
    res, info = rr.raycast(sample, r, radius, 20, fill=-7.0)
    o, d, _ = pr.origins_and_directions(r)
    # distance of the sphere's centre from each ray, in float64: well inside, or well outside
    oc = c - o.astype(np.float64)
    d64 = d.astype(np.float64)
    along = (oc * d64).sum(axis=2) / (d64 * d64).sum(axis=2)
    dist = np.sqrt(((oc - along[..., None] * d64) ** 2).sum(axis=2))
    through, miss = dist < radius - 1.0, dist > radius + 0.1
    assert through.sum() >= 20 and miss.sum() >= 50
    assert (res["crossings"][through] == 2).all() and (res["side"][through] == -1).all() and (res["index"][through] > 0).all()
    assert (res["crossings"][miss] == 0).all() and (res["index"][miss] == -1).all() and (res["side"][miss] == 0).all()
    for k in ("t", "value"):
        assert (res[k][miss] == f32(-7.0)).all(), k
    for k in ("position", "gradient"):
        assert (res[k][miss] == f32(-7.0)).all(), k
    # the refined hit lies on the sphere, and the gradient there points away from the centre
    hit = res["position"][through].astype(np.float64)
    assert np.abs(np.sqrt(((hit - c) ** 2).sum(axis=1)) - radius).max() < 1e-4
    assert np.abs(res["value"][through] - f32(radius)).max() < 1e-4
    assert ((res["gradient"][through] * (hit - c)).sum(axis=1) > 0).all()


def test_every_round_keeps_a_bracket_that_straddles_iso():
    r, sample, c, radius = _sphere()
    res, info = rr.raycast(sample, r, radius, 32)
    t = pr.times(r)
    rows, iso = info["rows"], f32(radius)
    i = res["index"].reshape(-1)[rows]
    assert len(rows) >= 20 and len(info["brackets"]) == 33
    widths = []
    for ta, va, tb, vb in info["brackets"]:
        assert (ta >= t[i - 1]).all() and (tb <= t[i]).all() and (ta <= tb).all()
        assert ((va >= iso) != (vb >= iso)).all()
        widths.append(tb - ta)
    assert all((w1 <= w0).all() for w0, w1 in zip(widths, widths[1:])) and (widths[-1] < widths[0]).all()
    ta, va, tb, vb = info["brackets"][-1]
    th = res["t"].reshape(-1)[rows]
    assert ((th >= ta) & (th <= tb)).all()
    # 32 rounds of a bracket 2^23 ulps wide at the most: every refinement ends on a collapsed bracket
    assert info["ended_collapsed"].all() and not info["ended_unusable"].any()


def test_a_pair_across_an_unusable_sample_is_no_crossing():
    r = z_rays()
    fn = lambda p: p[:, 2] - 5.0                                           # noqa: E731
    # sample 10 (z = 5.25), the one behind the zero, is outside every region; or NaN
    gap = analytic(fn, bad=lambda p: p[:, 2] == 5.25)
    nan = analytic(lambda p: np.where(p[:, 2] == 5.25, np.nan, fn(p)))
    for sample in (gap, nan):
        res, info = rr.raycast(sample, r, 0.0, 8, fill=-7.0)
        assert (res["crossings"] == 0).all() and (res["index"] == -1).all() and (res["side"] == 0).all()
        assert (res["t"] == f32(-7.0)).all() and (res["position"] == f32(-7.0)).all()
    assert np.isnan(info["values"][..., 10]).all() and (info["status"][..., 10] == 0).all()      # NaN samples are unusable
    # a gap elsewhere changes nothing; a ray that begins on the >= iso side behind a gap has no cap
    res, _ = rr.raycast(analytic(fn, bad=lambda p: p[:, 2] == 2.25), r, 0.0, 0)
    assert (res["crossings"] == 1).all() and (res["index"] == 10).all()
    res, _ = rr.raycast(analytic(fn, bad=lambda p: p[:, 2] < 7.0), r, 0.0, 0)
    assert (res["crossings"] == 0).all()
    # an unusable midpoint ends the refinement: t is the interpolation of the bracket so far
    first, _ = rr.raycast(analytic(fn), r, 0.0, 0)
    res, info = rr.raycast(analytic(fn, bad=lambda p: p[:, 2] == 5.0), r, 0.0, 8)
    assert info["ended_unusable"].all() and rr.same_bits(res["t"], first["t"])


def test_a_sample_equal_to_iso_is_inside():
    r = z_rays()
    # v_10 = 0 exactly: rising, the crossing is at index 10 (v_9 < iso <= v_10) and t is t_10 ...
    res, _ = rr.raycast(analytic(lambda p: p[:, 2] - 5.25), r, 0.0, 0)
    assert (res["index"] == 10).all() and (res["side"] == 1).all() and (res["crossings"] == 1).all()
    assert (res["t"] == f32(5.25)).all()
    # ... falling, v_10 = 0 is still inside: the crossing is at index 11 and t is t_10
    res, _ = rr.raycast(analytic(lambda p: 5.25 - p[:, 2]), r, 0.0, 0)
    assert (res["index"] == 11).all() and (res["side"] == -1).all() and (res["crossings"] == 1).all()
    assert (res["t"] == f32(5.25)).all()


def test_a_bracket_one_ulp_wide_is_not_refined():
    # the ulp of a float32 in [512, 1024) is 2^-14: steps of 1.5 ulps round to steps of 1 and of 2 ulps
    r = z_rays(tmin=1000.0, dt=1.5 * 2.0 ** -14, n=16)
    t = pr.times(r)
    k = 1 + int(np.flatnonzero(t[2:] == np.nextafter(t[1:-1], f32(np.inf)))[0])       # t_k and t_k+1 are neighbours
    c = float(t[k]) + 2.0 ** -16
    sample = analytic(lambda p: p[:, 2] - c)
    plain_res, _ = rr.raycast(sample, r, 0.0, 0)
    res, info = rr.raycast(sample, r, 0.0, 8)
    assert (res["index"] == k + 1).all() and info["ended_collapsed"].all()
    assert rr.same_bits(res["t"], plain_res["t"])
    assert rr.same_bits(res["t"], np.full((3, 5), plain(t[k], f32(t[k] - c), t[k + 1], f32(t[k + 1] - c), 0.0), f32))
    ta, va, tb, vb = info["brackets"][-1]
    assert (ta == t[k]).all() and (tb == t[k + 1]).all()


def test_infinite_samples_propagate_by_the_formulas():
    r = z_rays()
    # +Inf up to z = 5, then -1: the crossing's s is (iso - inf) / (-1 - inf) = NaN
    sample = analytic(lambda p: np.where(p[:, 2] < 5.0, np.inf, -1.0))
    res, info = rr.raycast(sample, r, 0.0, 0, fill=-7.0)
    assert (res["index"] == 10).all() and (res["side"] == -1).all() and (res["crossings"] == 1).all()
    assert np.isnan(res["t"]).all() and np.isnan(res["position"][..., 2]).all()
    assert (res["value"] == f32(-7.0)).all() and (res["gradient"] == f32(-7.0)).all()      # no sample at a NaN position
    # the other way round s is (0 - -1) / (inf - -1) = 0: t is ta
    res, _ = rr.raycast(analytic(lambda p: np.where(p[:, 2] < 5.0, -1.0, np.inf)), r, 0.0, 0)
    assert (res["index"] == 10).all() and (res["side"] == 1).all() and (res["t"] == f32(4.75)).all()
    # refined, the bracket closes in on the jump from the finite side
    res, info = rr.raycast(analytic(lambda p: np.where(p[:, 2] < 5.0, -1.0, np.inf)), r, 0.0, 32)
    assert info["ended_collapsed"].all() and (res["t"] == np.nextafter(f32(5.0), f32(0))).all()
