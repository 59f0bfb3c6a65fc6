"""tests/distance_ref.py, the numpy restatement of exa_hip_distance's passes, against the all-pairs global minimum that the
header's theorem states (no GPU needed): d2 = min over all targets of (term_x + term_y) + term_z in float32, bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import distance_ref as ref  # noqa: E402

F = np.float32
ISO = ((0, 0, 0), (1, 1, 1))                            # lo, hi of a unit box: spacing 1 / n per axis
BOXES = {"isotropic": lambda d: ((0, 0, 0), tuple(float(n) for n in d)),
         "x10": lambda d: ((0, 0, 0), (10.0 * d[0], float(d[1]), float(d[2]))),
         "z10": lambda d: ((-1, 2, 0.5), (-1 + 0.3 * d[0], 2 + 0.3 * d[1], 0.5 + 3.0 * d[2])),
         "odd": lambda d: ((0.1, -0.7, 3.0), (1.3, 0.9, 3.7))}


def brute_d2(target, h):
    """the theorem: per point the float32 minimum over all targets of (term_x + term_y) + term_z, +INF without a target"""
    nz, ny, nx = target.shape
    tk, tj, ti = np.nonzero(target)
    out = np.full(target.shape, np.inf, F)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                if ti.size:
                    s = (ref.term(h[0], i - ti) + ref.term(h[1], j - tj)).astype(F)
                    out[k, j, i] = ((s + ref.term(h[2], k - tk)).astype(F)).min()
    return out


def d2_to(target, h, L, nearest):
    """(term_x + term_y) + term_z from the point L to the point nearest"""
    nz, ny, nx = target.shape
    i, j, k = L % nx, (L // nx) % ny, L // (nx * ny)
    p, q, r = nearest % nx, (nearest // nx) % ny, nearest // (nx * ny)
    return F(F(ref.term(h[0], np.int64(i - p)) + ref.term(h[1], np.int64(j - q))) + ref.term(h[2], np.int64(k - r)))


def random_cases():
    rng = np.random.default_rng(20261021)
    for n in range(24):
        shape = tuple(int(s) for s in rng.integers(1, 8, 3))
        yield n, rng.random(shape) < rng.choice([0.05, 0.3, 0.9]), list(BOXES)[n % len(BOXES)]


@pytest.mark.parametrize("n,target,box", list(random_cases()))
def test_the_passes_equal_the_all_pairs_minimum(n, target, box):
    dims = target.shape[::-1]
    lo, hi = BOXES[box](dims)
    h = ref.spacing(lo, hi, dims)
    a, b, c, d2 = ref.passes(target, h)
    want = brute_d2(target, h)
    assert d2.dtype == F and d2.tobytes() == want.tobytes()
    dist, nearest, stats = ref.distance(target, lo, hi)
    assert dist.tobytes() == np.sqrt(want, dtype=F).tobytes()
    flat = target.reshape(-1)
    for L in range(flat.size):
        t = int(nearest.reshape(-1)[L])
        if not target.any():
            assert t == -1
            continue
        assert flat[t] and d2_to(target, h, L, t) == want.reshape(-1)[L]       # a target, and one that holds the minimum
        if flat[L]:
            assert t == L
    assert stats["inside"] == int(target.sum()) and stats["reached"] == (target.size if target.any() else 0)


def test_one_target_is_the_distance_to_it():
    target = np.zeros((4, 5, 6), bool)
    target[3, 0, 5] = True
    lo, hi = (0, 0, 0), (3, 10, 2)                      # spacing 0.5, 2, 0.5
    dist, nearest, stats = ref.distance(target, lo, hi, )
    k, j, i = np.meshgrid(np.arange(4), np.arange(5), np.arange(6), indexing="ij")
    exact = np.sqrt((0.5 * (i - 5.0)) ** 2 + (2.0 * j) ** 2 + (0.5 * (k - 3.0)) ** 2)
    assert np.allclose(dist, exact, rtol=4 * 2.0 ** -24, atol=0)
    assert (nearest == (3 * 5 + 0) * 6 + 5).all()
    assert dist[3, 0, 5] == 0 and not np.signbit(dist[3, 0, 5])
    assert stats == dict(points=120, inside=1, reached=120, maxDistance=float(dist.max()))


def test_no_target_and_all_targets():
    none = np.zeros((3, 4, 5), bool)
    dist, nearest, stats = ref.distance(none, *ISO)
    assert np.isposinf(dist).all() and (nearest == -1).all()
    assert stats == dict(points=60, inside=0, reached=0, maxDistance=0.0)
    dist, nearest, stats = ref.distance(~none, *ISO)
    assert dist.tobytes() == np.zeros(none.shape, F).tobytes()
    assert (nearest.reshape(-1) == np.arange(60)).all()
    assert stats == dict(points=60, inside=60, reached=60, maxDistance=0.0)
    dist, nearest, stats = ref.distance(none, *ISO, to_outside=True)       # every point is a target of the outside set
    assert dist.tobytes() == np.zeros(none.shape, F).tobytes() and stats["inside"] == 0 and stats["reached"] == 60
    dist, nearest, _ = ref.distance(~none, *ISO, signed=True)              # inside everywhere, no outside point
    assert np.isneginf(dist).all() and (nearest == -1).all()


def test_ties_take_the_smaller_index_axis_by_axis():
    target = np.zeros((5, 5, 5), bool)
    target[0], target[4] = True, True                   # two planes k = 0 and k = 4
    target[:, 0, :] = True
    target[:, 4, :] = True                              # and j = 0, j = 4
    _, nearest, _ = ref.distance(target, (0, 0, 0), (5, 5, 5))
    # the centre is 2 away from four planes: Z picks the smallest k' among equal sums, and in that plane the point itself
    assert nearest[2, 2, 2] == (0 * 5 + 2) * 5 + 2
    row = np.zeros((1, 1, 5), bool)
    row[0, 0, 0] = row[0, 0, 4] = True
    _, nearest, _ = ref.distance(row, (0, 0, 0), (5, 1, 1))
    assert nearest.reshape(-1).tolist() == [0, 0, 0, 4, 4]
    col = np.zeros((1, 5, 1), bool)
    col[0, 0, 0] = col[0, 4, 0] = True
    _, nearest, _ = ref.distance(col, (0, 0, 0), (1, 5, 1))
    assert nearest.reshape(-1).tolist() == [0, 0, 0, 4, 4]


def test_max_distance_on_both_sides_of_an_exact_distance():
    target = np.zeros((1, 1, 9), bool)
    target[0, 0, 0] = True
    lo, hi = (0, 0, 0), (9, 1, 1)                       # spacing 1: the point i is i away, exactly
    for reach, last in ((3.0, 3), (np.nextafter(F(3), F(0)), 2), (np.nextafter(F(3), F(4)), 3)):
        dist, nearest, stats = ref.distance(target, lo, hi, max_distance=reach)
        assert dist.reshape(-1)[:last + 1].tolist() == [float(i) for i in range(last + 1)]
        assert np.isposinf(dist.reshape(-1)[last + 1:]).all() and (nearest.reshape(-1)[last + 1:] == -1).all()
        assert stats["reached"] == last + 1 and stats["maxDistance"] == float(last)


@pytest.mark.parametrize("seed", range(4))
def test_signed_is_the_two_one_sided_calls_merged(seed):
    rng = np.random.default_rng(seed)
    inside = rng.random((4, 6, 5)) < 0.4
    lo, hi = BOXES["z10"](inside.shape[::-1])
    for reach in (np.inf, 1.0):
        to_in, near_in, _ = ref.distance(inside, lo, hi, max_distance=reach)
        to_out, near_out, _ = ref.distance(inside, lo, hi, max_distance=reach, to_outside=True)
        dist, nearest, stats = ref.distance(inside, lo, hi, max_distance=reach, signed=True)
        assert dist.tobytes() == np.where(inside, -to_out, to_in).astype(F).tobytes()
        assert nearest.tobytes() == np.where(inside, near_out, near_in).astype(np.int32).tobytes()
        assert (dist[inside] < 0).all() and (dist[~inside] > 0).all()
        assert stats["reached"] == int(np.isfinite(dist).sum()) and stats["inside"] == int(inside.sum())


def test_bands_are_floor_of_the_distance_over_the_width():
    dist = np.array([0.0, 0.49, 0.5, -0.5, 1.49, 1.5, np.inf, -np.inf, np.nan], F)
    assert ref.bands(dist, 0.5, 3).tolist() == [0, 0, 1, 1, 2, -1, -1, -1, -1]


@pytest.mark.parametrize("box", list(BOXES))
def test_against_scipy_in_float64(box):
    """Against scipy's exact transform of the same float32 spacing in float64.  The allowance, with u = 2^-24: a term
    o*o with o = fl(h*d) carries (1+u)^2 from o and (1+u) from the product, 3u; the two sums add one rounding each to
    non-negative operands, 5u on d2; every candidate of the minimum is within that, so the minimum is; the square root halves
    it to 2.5u and rounds once more, 3.5u and second-order terms: relative 4 * 2^-24."""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(7)
    target = rng.random((7, 6, 5)) < 0.1
    target[3, 2, 1] = True
    dims = target.shape[::-1]
    lo, hi = BOXES[box](dims)
    h = ref.spacing(lo, hi, dims)
    dist, _, _ = ref.distance(target, lo, hi)
    want = ndimage.distance_transform_edt(~target, sampling=[float(h[2]), float(h[1]), float(h[0])])
    assert np.all(np.abs(dist.astype(np.float64) - want) <= 4 * 2.0 ** -24 * want)
