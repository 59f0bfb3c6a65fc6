"""The numpy restatement of exa_hip_isolines' contract (tests/isolines_ref.py) on analytic lattices: the lines close, the
>= iso side lies to their left, no vertex comes twice, the order is the stated one, a lattice value equal to iso gives
zero-length segments, and the levels are independent.  No GPU, no kernel."""
import numpy as np
import pytest

import isolines_ref as ref

NU, NV = 23, 17
ORIGIN, DU, DV = (1.0, -2.0, 0.5), (0.5, 0.25, 0.0), (-0.125, 0.25, 0.75)        # an oblique plane


def _uv():
    return np.meshgrid(np.arange(NU) + 0.5, np.arange(NV) + 0.5)              # [NV, NU] each


def _dist(cu=11.3, cv=8.4):
    u, v = _uv()
    return np.hypot(u - cu, v - cv)


def _circle():
    return (6.2 - _dist()).astype(np.float32), [0.0]


def _nested():
    return (1.0 - np.abs(_dist() - 4.6)).astype(np.float32), [-0.7, 0.1]     # >= iso: an annulus, two circles per level


def _saddle():
    u, v = _uv()
    return ((u - 11.3) * (v - 8.4)).astype(np.float32), [0.0, 2.5, -1.0]


def _hole():
    V, isos = _circle()
    V[6:10, 3:8] = np.nan                                                    # across the circle
    V[0, 0] = np.inf
    return V, isos


FIELDS = dict(circle=_circle, nested=_nested, saddle=_saddle, hole=_hole)


def _levels(r):
    for n in range(len(r["vertex_offsets"]) - 1):
        yield n, slice(int(r["vertex_offsets"][n]), int(r["vertex_offsets"][n + 1])), \
            slice(int(r["segment_offsets"][n]), int(r["segment_offsets"][n + 1]))


def _interior(V, owner, code):
    """the vertex's edge is shared by two triangles of valid squares: a diagonal always, a side if both its squares are"""
    valid = np.zeros((NV + 1, NU + 1), bool)                                  # padded: [j+1, i+1]
    valid[1:NV, 1:NU] = ref.valid_squares(V)
    j, i = owner // NU, owner % NU
    return np.where(code == 3, True, np.where(code == 1, valid[j + 1, i + 1] & valid[j, i + 1], valid[j + 1, i + 1] & valid[j + 1, i]))


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_lines_close_and_keep_the_inside_on_their_left(name):
    V, isos = FIELDS[name]()
    r = ref.extract(V, ORIGIN, DU, DV, isos)
    assert len(r["segments"]) > 8 * len(isos)
    for n, vs, ss in _levels(r):
        seg = r["segments"][ss]
        assert seg.min() >= vs.start and seg.max() < vs.stop                  # global indices into the level's own range
        starts = np.bincount(seg[:, 0] - vs.start, minlength=vs.stop - vs.start)
        ends = np.bincount(seg[:, 1] - vs.start, minlength=vs.stop - vs.start)
        inner = _interior(V, r["owner"][vs], r["code"][vs])
        assert np.all(starts[inner] == 1) and np.all(ends[inner] == 1), name
        assert np.all(starts + ends >= 1) and np.all(starts[~inner] + ends[~inner] == 1), name     # the rim: one triangle
        if name == "hole":
            assert (~inner).sum() >= 2
        # the >= iso side: the emitting triangle's linear interpolant a small step left of the midpoint, in uv
        uv = r["uv"].astype(np.float64)
        a, b = uv[seg[:, 0]], uv[seg[:, 1]]
        d = b - a
        length = np.hypot(d[:, 0], d[:, 1])
        keep = length > 1e-4
        left = np.stack([-d[:, 1], d[:, 0]], axis=1)[keep] / length[keep, None]
        probe = 0.5 * (a + b)[keep] + 1e-3 * left
        sq, tri = r["square"][ss][keep], r["tri"][ss][keep]
        j, i = sq // NU, sq % NU
        u, v = probe[:, 0] - (i + 0.5), probe[:, 1] - (j + 0.5)                # in the square: [0,1]^2
        V64 = V.astype(np.float64)
        f00, f11 = V64[j, i], V64[j + 1, i + 1]
        f10, f01 = V64[j, i + 1], V64[j + 1, i]
        # T0 (u >= v): f00 + u (f10 - f00) + v (f11 - f10); T1: f00 + v (f01 - f00) + u (f11 - f01)
        val = np.where(tri == 0, f00 + u * (f10 - f00) + v * (f11 - f10), f00 + v * (f01 - f00) + u * (f11 - f01))
        assert keep.sum() > 8 and np.all(val > float(np.float32(isos[n]))), name


@pytest.mark.parametrize("name", sorted(FIELDS))
def test_vertices_are_unique_and_the_order_is_the_stated_one(name):
    V, isos = FIELDS[name]()
    r = ref.extract(V, ORIGIN, DU, DV, isos)
    P = ref.positions(ORIGIN, DU, DV, NU, NV).reshape(-1, 3)
    for n, vs, ss in _levels(r):
        key = r["owner"][vs] * 4 + r["code"][vs]
        assert np.all(np.diff(key) > 0), name                                  # ascending L(p), then edge code: no edge twice
        assert len(np.unique(r["uv"][vs], axis=0)) == vs.stop - vs.start       # and no position twice on these fields
        skey = r["square"][ss] * 2 + r["tri"][ss]
        assert np.all(np.diff(skey) > 0), name                                 # ascending L of the square, T0 before T1
        # every vertex lies on its edge, between P(p) and P(q), and uv says where
        code = r["code"][vs]
        q = r["owner"][vs] + (code & 1) + (code >> 1) * NU
        t = np.where(code == 2, r["uv"][vs][:, 1] - (r["owner"][vs] // NU + 0.5), r["uv"][vs][:, 0] - (r["owner"][vs] % NU + 0.5))
        assert np.all((t >= 0) & (t <= 1))
        want = P[r["owner"][vs]] + t[:, None] * (P[q] - P[r["owner"][vs]]).astype(np.float64)
        assert np.allclose(r["vertices"][vs], want, atol=1e-4)
    assert r["segments"].dtype == np.int32 and r["vertices"].dtype == np.float32 and r["uv"].dtype == np.float32
    assert r["vertex_offsets"].dtype == np.uint64 and r["segment_offsets"].dtype == np.uint64


def test_a_lattice_value_equal_to_iso_gives_zero_length_segments():
    V, _ = _circle()
    iso = float(V[5, 7])                                                     # an inner lattice point: the line runs through it
    assert (V == np.float32(iso)).any() and V.min() < iso < V.max()
    r = ref.extract(V, ORIGIN, DU, DV, [iso])
    a, b = r["vertices"][r["segments"][:, 0]], r["vertices"][r["segments"][:, 1]]
    zero = np.all(a == b, axis=1)
    assert zero.any() and not zero.all()
    assert np.isfinite(r["vertices"]).all() and np.isfinite(r["uv"]).all()
    # several vertices coincide with the lattice point (t == 0 on its own edges, t == 1 on the edges that end there)
    j, i = np.argwhere(V == np.float32(iso))[0]
    at = np.all(r["uv"] == np.array([i + 0.5, j + 0.5], np.float32), axis=1)
    assert at.sum() >= 2


def test_levels_are_independent_and_come_in_the_order_given():
    V, _ = _saddle()
    a, b = 2.5, -1.0
    both, ra, rb = (ref.extract(V, ORIGIN, DU, DV, isos) for isos in ([a, b, a], [a], [b]))
    na, nb = len(ra["vertices"]), len(rb["vertices"])
    assert na and nb
    assert np.array_equal(both["vertex_offsets"], np.array([0, na, na + nb, 2 * na + nb], np.uint64))
    assert np.array_equal(both["segment_offsets"], np.cumsum([0, len(ra["segments"]), len(rb["segments"]), len(ra["segments"])]).astype(np.uint64))
    for k in ("vertices", "uv"):
        assert np.concatenate([ra[k], rb[k], ra[k]]).tobytes() == both[k].tobytes()
    assert np.array_equal(both["segments"], np.concatenate([ra["segments"], rb["segments"] + na, ra["segments"] + na + nb]))


def test_nothing_crosses_and_nothing_is_valid():
    V, _ = _circle()
    r = ref.extract(V, ORIGIN, DU, DV, [100.0, -100.0])
    assert r["vertices"].shape == (0, 3) and r["uv"].shape == (0, 2) and r["segments"].shape == (0, 2)
    assert np.array_equal(r["vertex_offsets"], np.zeros(3, np.uint64))
    r = ref.extract(np.full((2, 2), np.nan, np.float32), ORIGIN, DU, DV, [0.0])
    assert len(r["vertices"]) == 0 and len(r["segments"]) == 0
    r = ref.extract(np.array([[0, 1], [1, 2]], np.float32), ORIGIN, DU, DV, [0.5])       # a single square
    assert len(r["vertices"]) == 3 and len(r["segments"]) == 2
