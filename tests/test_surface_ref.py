"""tests/surface_ref.py, the numpy restatement of the contract of exa_hip_sample_triangles (include/exa_hip.h), held against
the contract's own words: the sample map with exact fractions, the two constants' bits, the 64-slot reduction and its tree
against the literal loops and against plain sums, the -0.0 rule and the clamp of n.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import surface_ref as sr

f32 = np.float32
NS = [1, 2, 3, 4, 5, 8, 9, 64]


def test_the_two_constants():
    assert sr.T1.dtype == f32 and sr.T2.dtype == f32
    assert sr.T1.view(np.uint32) == 0x3EAAAAAB and sr.T2.view(np.uint32) == 0x3F2AAAAB


def _sub_triangles(n):
    """the n * n congruent sub-triangles of the unit triangle in barycentric (b1, b2), as frozensets of three exact corners:
    the upright ones with corner (i, j)/n, i + j < n, and the inverted ones between them"""
    out = set()
    for i in range(n):
        for j in range(n - i):
            out.add(frozenset([(Fraction(i, n), Fraction(j, n)), (Fraction(i + 1, n), Fraction(j, n)), (Fraction(i, n), Fraction(j + 1, n))]))
            if i + j < n - 1:
                out.add(frozenset([(Fraction(i + 1, n), Fraction(j, n)), (Fraction(i, n), Fraction(j + 1, n)),
                                   (Fraction(i + 1, n), Fraction(j + 1, n))]))
    assert len(out) == n * n
    return out


@pytest.mark.parametrize("n", NS)
def test_the_map_hits_every_sub_triangle_exactly_once(n):
    a, b, upright = sr.ab_map(n)
    assert len(a) == n * n
    third = lambda t: Fraction(1, 3) if t else Fraction(2, 3)                # noqa: E731
    centroid = {}
    for tri in _sub_triangles(n):
        c = (sum(p[0] for p in tri) / 3, sum(p[1] for p in tri) / 3)
        assert c not in centroid
        centroid[c] = tri
    hit = set()
    for k in range(n * n):
        c = ((int(a[k]) + third(upright[k])) / n, (int(b[k]) + third(upright[k])) / n)
        assert c in centroid, (n, k)
        assert c not in hit, (n, k)
        hit.add(c)
        assert c[0] + c[1] < 1
    assert len(hit) == n * n
    assert sum(c[0] for c in hit) / (n * n) == Fraction(1, 3) and sum(c[1] for c in hit) / (n * n) == Fraction(1, 3)
    # the literal map of the contract
    for k in range(n * n):
        ka, kb = k // n, k % n
        want = (ka, kb, True) if ka + kb < n else (n - 1 - ka, n - 1 - kb, False)
        assert (int(a[k]), int(b[k]), bool(upright[k])) == want


@pytest.mark.parametrize("n", NS)
def test_float32_positions_are_distinct_and_inside(n):
    b1, b2 = sr.barycentrics(n)
    assert len(set(zip(b1.tolist(), b2.tolist()))) == n * n
    assert np.all(b1.astype(np.float64) + b2.astype(np.float64) < 1) and np.all(b1 > 0) and np.all(b2 > 0)
    assert abs(b1.astype(np.float64).mean() - 1 / 3) < 1e-6 and abs(b2.astype(np.float64).mean() - 1 / 3) < 1e-6
    v0, v1, v2 = f32([1, 2, 3]), f32([5, 2, 3]), f32([1, 10, 7])
    p = sr.positions(v0, v1, v2, n)
    assert p.shape == (n * n, 3) and p.dtype == f32
    with np.errstate(all="ignore"):
        k = n * n - 1
        want = (v0 + b1[k] * (v1 - v0)) + b2[k] * (v2 - v0)
    assert sr.same_bits(p[k], want)


def test_tree_equals_a_plain_sum_on_integers():
    rng = np.random.default_rng(3)
    for K in (1, 4, 16, 25, 64, 81, 4096):
        v = rng.integers(-1000, 1000, size=(5, K)).astype(f32)
        st = np.where(rng.random((5, K)) < 0.8, 3, -1)
        st[0] = -2
        total, count = sr.reduce(v, st)
        assert np.array_equal(total, np.where(st >= 0, v, 0).astype(np.float64).sum(axis=1))
        assert np.array_equal(count, (st >= 0).sum(axis=1)) and count.dtype == np.uint32
        assert sr.same_bits(total[0], np.float64(0.0))                      # no valid sample: +0.0
    P = rng.integers(-5, 5, size=(3, 64)).astype(np.float64)
    assert np.array_equal(sr.tree(P), P.sum(axis=1))


def test_reduce_equals_the_literal_loops():
    rng = np.random.default_rng(4)
    for K in (1, 4, 9, 16, 25, 64, 65, 81, 130, 4096):
        v = (rng.standard_normal(K) * 10.0 ** rng.integers(-3, 4, K)).astype(f32)
        st = np.where(rng.random(K) < 0.7, 1, rng.choice([-1, -2], K))
        total, count = sr.reduce(v, st)
        want, n = sr.reduce_literal(v, st)
        assert sr.same_bits(np.float64(total), np.float64(want)) and count == n, K
    # the tree is not the sequential sum: a case where the two differ, which reduce must follow
    v = np.zeros(64, f32)
    v[0], v[1], v[32] = f32(2.0 ** 60), f32(1.0), f32(-2.0 ** 60)
    total, _ = sr.reduce(v, np.zeros(64, int))
    assert total == 1.0 and np.cumsum(v.astype(np.float64))[-1] == 0.0
    # NaN poisons
    v[5] = np.nan
    assert np.isnan(sr.reduce(v, np.zeros(64, int))[0])


def test_a_lone_negative_zero_becomes_positive_zero():
    for K in (1, 4, 16, 64, 81):
        v = np.zeros(K, f32)
        v[K - 1] = f32(-0.0)
        st = np.full(K, -1)
        st[K - 1] = 0
        total, count = sr.reduce(v, st)
        assert count == 1 and sr.same_bits(np.float64(total), np.float64(0.0)), K
        assert sr.same_bits(np.float64(sr.reduce_literal(v, st)[0]), np.float64(0.0))
    assert sr.same_bits(sr.reduce(np.full(64, f32(-0.0)), np.zeros(64, int))[0], np.float64(0.0))


def test_the_clamp_of_n():
    one, up, down = f32(1), np.nextafter(f32(1), f32(2)), np.nextafter(f32(1), f32(0))
    for max_n in (1, 7, 64):
        m = f32(max_n)
        L = np.array([m, np.nextafter(m, f32(0)), np.nextafter(m, f32(1000)), f32(0), f32(1e-30), one, up, down, f32(3.4e38), f32(2.5)], f32)
        n = sr.subdiv_of_length(L, one, max_n)
        want = [max_n, max_n, max_n, 1, 1, 1, min(2, max_n), 1, max_n, min(3, max_n)]
        assert n.tolist() == want and n.dtype == np.int32, (max_n, n.tolist())
        assert sr.subdiv_of_length(L, f32(0), max_n).tolist() == [max_n] * len(L)
    # q = L / spacing is a float32 quotient: exactly an integer stays, one ulp more goes up
    assert sr.subdiv_of_length(f32([1.5, 1.5000001]), f32(0.5), 64).tolist() == [3, 4]
    # an overflowing quotient is >= maxN
    assert sr.subdiv_of_length(f32([1e30]), f32(1e-30), 64).tolist() == [64]


def test_triangles_that_are_not_valid():
    verts = f32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0], [np.inf, 0, 0], [3e38, 0, 0], [-3e38, 0, 0]])
    tris = np.array([[0, 1, 2], [0, 1, 7], [-1, 1, 2], [0, 1, 3], [0, 1, 4], [0, 5, 6], [0, 0, 0], [2, 1, 0]], np.int32)
    sub = sr.subdivision(verts, tris, 0.25, 64)
    assert sub.tolist() == [6, 0, 0, 0, 0, 0, 1, 6]              # sqrt(2) / 0.25 = 5.66; an overflowing edge length; a point
    an = sr.area_normal(verts, tris)
    assert an[0].tolist() == [0, 0, 0.5] and an[7].tolist() == [0, 0, -0.5] and an[6].tolist() == [0, 0, 0]
    assert np.isnan(an[1]).all() and np.isnan(an[2]).all() and np.isnan(an[3]).any()
    out, values, status = sr.sample_triangles(lambda p: (np.ones((len(p), 2), f32), np.zeros((len(p), 2), int)), verts, tris, 2, 0.25, 64)
    assert out["count"][:, 0].tolist() == [36, 0, 0, 0, 0, 0, 1, 36] and np.array_equal(out["sum"], out["count"].astype(np.float64))
    assert len(values) == 73
    assert sr.subdivision(np.zeros((0, 3), f32), tris, 0.25, 64).tolist() == [0] * 8
