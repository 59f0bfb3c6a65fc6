"""tests/project_ref.py, the numpy restatement of exa_hip_project's contract, on the CPU: the property the kernel's skipping
of indices rests on — per axis the float32 position of a ray's samples is monotone in the sample index, so the indices
inside a box form one contiguous range that a bisection on the entered / not-yet-left halves of the box test finds — and
the reduction on hand-made sequences."""
import numpy as np
import pytest

import project_ref as pr

f32 = np.float32
BOX_LO, BOX_HI = np.array([-2, -2, -2], f32), np.array([50, 50, 34], f32)


def random_rays(rng, kind):
    ext = (BOX_HI - BOX_LO).astype(np.float64)
    n = int(rng.choice([1, 2, 17, 96, 1000, 4096]))
    org = BOX_LO + rng.uniform(-1.5, 2.5, 3) * ext
    d = rng.normal(size=3)
    if kind == "axis":
        d[rng.integers(3)] = 0.0
        if rng.random() < 0.5:
            d[rng.integers(3)] = -0.0
    if kind == "far":
        org = org - d / np.linalg.norm(d) * 10.0 ** rng.uniform(3, 7)
    if kind == "tiny":
        d = d * 10.0 ** rng.uniform(-30, -20)
    dt = 10.0 ** rng.uniform(-3, 1) if kind != "tiny" else 10.0 ** rng.uniform(20, 30)
    tmin = rng.uniform(-100, 100) if kind != "far" else 10.0 ** rng.uniform(3, 7)
    spread = rng.normal(size=(4, 3)) * (0.0 if kind == "axis" else 0.05)
    return pr.rays(org, d, (5, 3), tmin, dt, n, orgDu=spread[0] * 10, orgDv=spread[1] * 10, dirDu=spread[2], dirDv=spread[3])


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("kind", ["plain", "axis", "far", "tiny"])
def test_positions_are_monotone_per_axis_and_the_inside_indices_contiguous(kind, normalize):
    rng = np.random.default_rng(["plain", "axis", "far", "tiny"].index(kind) * 2 + int(normalize))
    repeats = 0
    for _ in range(60):
        r = random_rays(rng, kind)
        p, has = pr.positions(r, normalize)
        o, d, _ = pr.origins_and_directions(r, normalize)
        assert p.dtype == f32 and np.isfinite(p[has]).all()
        t = pr.times(r)
        assert np.all(np.diff(t) >= 0)
        repeats += int((np.diff(t) == 0).sum())
        step = np.diff(p.astype(np.float64), axis=2)
        up = (d >= 0)[:, :, None, :]
        assert np.all(np.where(up, step >= 0, step <= 0)[has])
        # the two halves of the closed-box test, dealt by the sign of the direction: a suffix and a prefix of the indices
        dd = d[:, :, None, :]
        entered = np.all(np.where(dd >= 0, p >= BOX_LO, p <= BOX_HI), axis=3)
        not_left = np.all(np.where(dd >= 0, p <= BOX_HI, p >= BOX_LO), axis=3)
        inside = np.all((p >= BOX_LO) & (p <= BOX_HI), axis=3)
        assert np.array_equal(inside, entered & not_left)
        assert np.all(np.diff(entered.astype(int), axis=2) >= 0) and np.all(np.diff(not_left.astype(int), axis=2) <= 0)
        # ... which a bisection finds: the kernel's two searches, restated
        n = r["num_samples"]
        for y, x in np.ndindex(has.shape):
            if not has[y, x]:
                continue
            lo, hi = 0, n
            while lo < hi:
                mid = lo + ((hi - lo) >> 1)
                lo, hi = (lo, mid) if entered[y, x, mid] else (mid + 1, hi)
            beg, hi = lo, n
            while lo < hi:
                mid = lo + ((hi - lo) >> 1)
                lo, hi = (mid + 1, hi) if not_left[y, x, mid] else (lo, mid)
            want = np.zeros(n, dtype=bool)
            want[beg:lo] = True
            assert np.array_equal(inside[y, x], want), (kind, y, x, beg, lo)
    if kind == "far":
        assert repeats > 0                   # t_i spaced wider than dt: positions repeat


def test_normalisation_and_the_association_of_the_header():
    r = pr.rays((1, 2, 3), (3, 4, 12), (2, 2), 0.5, 0.25, 4, orgDu=(0.1, 0, 0), orgDv=(0, 0.3, 0), dirDu=(0, 0, 0), dirDv=(0, 0, 0))
    o, d, has = pr.origins_and_directions(r, True)
    assert has.all() and np.array_equal(d[0, 0], np.array([3, 4, 12], f32) / f32(13))
    sx, sy = f32(1.5), f32(0.5)
    assert o[0, 1, 0] == f32(1) + sx * f32(0.1) and o[0, 1, 1] == f32(2) + sy * f32(0.3)
    p, _ = pr.positions(r, True)
    t2 = f32(0.5) + (f32(2) + f32(0.5)) * f32(0.25)
    assert np.array_equal(p[0, 1, 2], o[0, 1] + t2 * d[0, 1])
    # no direction: no samples with normalize, every sample at the origin without
    z = pr.rays((1, 2, 3), (0, 0, 0), (1, 1), 0, 1, 3)
    assert not pr.origins_and_directions(z, True)[2].any() and pr.origins_and_directions(z, False)[2].all()
    assert np.array_equal(pr.positions(z, False)[0][0, 0], np.tile(np.array([1, 2, 3], f32), (3, 1)))
    # an overflowing direction: not finite, no samples
    big = pr.rays((0, 0, 0), (3e38, 3e38, 0), (1, 1), 0, 1, 2)
    assert not pr.origins_and_directions(big, True)[2].any()


SEQUENCES = {
    "all invalid": ([1.0, 2.0, 3.0], [-1, -2, -1]),
    "plain": ([1.0, -2.0, 3.5, 0.25], [4, 4, 5, 6]),
    "invalid skipped": ([9.0, 1.0, 9.0, 2.0, 9.0], [-1, 0, -2, 3, -1]),
    "a nan": ([1.0, np.nan, 3.0, 2.0], [0, 0, 0, 0]),
    "only nan": ([np.nan, np.nan], [1, 1]),
    "nan first": ([np.nan, -1.0], [0, 0]),
    "zeros, minus first": ([-0.0, 0.0, -0.0], [0, 0, 0]),
    "zeros, plus first": ([0.0, -0.0, 0.0], [0, 0, 0]),
    "minus zero alone": ([-0.0], [7]),
    "first of equal maxima": ([1.0, 5.0, 2.0, 5.0, 5.0], [0, 0, 0, 0, 0]),
    "first of equal maxima behind an invalid one": ([5.0, 5.0, 1.0, 5.0], [-1, 2, 2, 2]),
    "infinities": ([-np.inf, np.inf, 1.0], [0, 0, 0]),
    "only minus infinity": ([-np.inf, -np.inf], [0, 0]),
    "only plus infinity": ([np.inf], [0]),
    "cancellation in float32, not in float64": ([1e8, 1.0, -1e8], [0, 0, 0]),
    "one sample": ([2.5], [0]),
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
def test_reduction_on_hand_made_sequences(name):
    values, status = SEQUENCES[name]
    got = pr.reduce(np.array([values], f32), np.array([status]))
    want = pr.reduce_literal(values, status)
    for k, v in want.items():
        a, b = np.asarray(got[k][0]), np.asarray(v)
        assert a.dtype == b.dtype, (k, a.dtype, b.dtype)
        if k == "sum" and np.isnan(b):
            assert np.isnan(a)
        else:
            assert a.tobytes() == b.tobytes(), (name, k, a, b)


def test_reduction_expectations_spelled_out():
    def red(name):
        values, status = SEQUENCES[name]
        return {k: v[0] for k, v in pr.reduce(np.array([values], f32), np.array([status])).items()}

    r = red("all invalid")
    assert r["count"] == 0 and r["sum"] == 0.0 and r["max"] == -np.inf and r["min"] == np.inf and r["max_index"] == -1
    r = red("a nan")
    assert r["count"] == 4 and np.isnan(r["sum"]) and r["max"] == 3.0 and r["min"] == 1.0 and r["max_index"] == 2
    r = red("only nan")
    assert r["count"] == 2 and np.isnan(r["sum"]) and r["max"] == -np.inf and r["min"] == np.inf and r["max_index"] == -1
    r = red("zeros, minus first")
    assert np.signbit(r["max"]) and np.signbit(r["min"]) and r["max_index"] == 0 and not np.signbit(r["sum"])
    r = red("zeros, plus first")
    assert not np.signbit(r["max"]) and not np.signbit(r["min"]) and r["max_index"] == 0
    r = red("minus zero alone")
    assert r["count"] == 1 and not np.signbit(r["sum"]) and np.signbit(r["max"])
    assert red("first of equal maxima")["max_index"] == 1
    assert red("first of equal maxima behind an invalid one")["max_index"] == 1
    r = red("only minus infinity")
    assert r["max"] == -np.inf and r["max_index"] == -1 and r["min"] == -np.inf
    r = red("only plus infinity")
    assert r["max"] == np.inf and r["max_index"] == 0 and r["min"] == np.inf
    assert red("cancellation in float32, not in float64")["sum"] == 1.0
    r = red("invalid skipped")
    assert r["count"] == 2 and r["sum"] == 3.0 and r["max_index"] == 3


def test_reduce_keeps_the_shape_of_an_image():
    rng = np.random.default_rng(3)
    values = rng.normal(size=(4, 5, 7)).astype(f32)
    status = rng.integers(-2, 3, size=(4, 5, 7))
    got = pr.reduce(values, status)
    for y, x in np.ndindex(4, 5):
        want = pr.reduce_literal(values[y, x], status[y, x])
        for k, v in want.items():
            assert got[k].shape == (4, 5) and np.asarray(got[k][y, x]).tobytes() == np.asarray(v).tobytes(), (k, y, x)
