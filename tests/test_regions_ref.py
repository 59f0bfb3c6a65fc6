"""The numpy restatement of exa_hip_regions' contract (tests/regions_ref.py) checked on its own, without a GPU: against
scipy.ndimage.label where that is installed, on hand cases of the two neighbourhoods, and through the identities of the
table."""
import math
import time

import numpy as np
import pytest

import regions_ref as ref


def _field(seed, shape=(13, 17, 19), nan=0.1):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal(shape).astype(np.float32)
    V[rng.random(shape) < nan] = np.nan
    V[rng.random(shape) < 0.01] = np.inf
    V[rng.random(shape) < 0.01] = -np.inf
    return V


def _structure(faces):
    """scipy's structuring element [z, y, x]: the centre, and +-d for every edge kind d"""
    S = np.zeros((3, 3, 3), bool)
    S[1, 1, 1] = True
    for dx, dy, dz in (ref.FACES if faces else ref.KUHN):
        S[1 + dz, 1 + dy, 1 + dx] = S[1 - dz, 1 - dy, 1 - dx] = True
    assert S.sum() == (7 if faces else 15)
    return S


@pytest.mark.parametrize("below", [False, True])
@pytest.mark.parametrize("faces", [False, True])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_labels_equal_scipy_minus_one(seed, faces, below):
    ndimage = pytest.importorskip("scipy.ndimage")
    V = _field(seed)
    iso = (0.8 if seed != 3 else 1.0) * (-1 if below else 1)       # a fifth of the points inside: many components
    mask = ref.inside(V, iso, below)
    assert 0 < mask.sum() < V.size and not mask[~np.isfinite(V)].any()
    want, count = ndimage.label(mask, structure=_structure(faces))
    labels, T, _ = ref.regions(V, iso, below=below, faces=faces)
    # scipy numbers the components in raster order of their first point
    assert len(T) == count and count > 3
    assert np.array_equal(labels, want.astype(np.int32) - 1)


def _points(shape, pts):
    V = np.full(shape, -1.0, np.float32)
    for i, j, k in pts:
        V[k, j, i] = 1.0
    return V


def test_hand_cases_of_the_two_neighbourhoods():
    joined = lambda pts, faces: len(ref.regions(_points((3, 3, 3), pts), 0.0, faces=faces)[1]) == 1      # noqa: E731
    assert joined([(0, 0, 0), (1, 1, 1)], False)                   # the cube diagonal
    assert joined([(0, 0, 0), (1, 1, 0)], False)                   # the face diagonal of the split
    assert not joined([(1, 0, 0), (0, 1, 0)], False)               # the other face diagonal is no tetrahedron edge
    for pts in ([(0, 0, 0), (1, 1, 1)], [(0, 0, 0), (1, 1, 0)], [(1, 0, 0), (0, 1, 0)]):
        assert not joined(pts, True)
    assert joined([(0, 0, 0), (1, 0, 0)], True) and joined([(0, 0, 0), (0, 0, 1)], True)


def checkerboard(n):
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    return np.where((i + j + k) % 2 == 0, 1.0, -1.0).astype(np.float32)


def boustrophedon(nx, ny, nz):
    """+1 on a path through the rows of even y and even z, joined at alternating ends, -1 elsewhere: [nz, ny, nx] and the
    path's length"""
    V = np.full((nz, ny, nx), -1.0, np.float32)
    row = 0
    for k in range(0, nz, 2):
        js = list(range(0, ny, 2))
        if (k // 2) % 2:
            js.reverse()
        for n, j in enumerate(js):
            V[k, j, :] = 1.0
            if n + 1 < len(js):                                     # the joint to the next row of this slice
                V[k, (j + js[n + 1]) // 2, nx - 1 if row % 2 == 0 else 0] = 1.0
            elif k + 2 < nz:                                        # and to the next slice
                V[k + 1, j, nx - 1 if row % 2 == 0 else 0] = 1.0
            row += 1
    return V, int((V > 0).sum())


def test_checkerboard_is_one_point_per_region_under_faces():
    V = checkerboard((6, 5, 4))
    labels, T, _ = ref.regions(V, 0.0, faces=True)
    assert len(T) == (V > 0).sum() == 60 and np.all(T["points"] == 1)
    assert np.array_equal(labels[V > 0], np.arange(60))            # numbered by ascending L
    assert len(ref.regions(V, 0.0)[1]) < 60


def test_a_long_path_is_one_region_in_few_rounds():
    V, length = boustrophedon(100, 100, 60)                          # 600 000 points, a path of more than 60 000
    assert V.size == 600000 and length > 60000
    t0 = time.time()
    for faces in (False, True):
        parent, rounds = ref.roots(V > 0, faces)
        assert rounds <= 40, rounds
        assert np.all(parent[(V > 0).reshape(-1)] == 0)
    labels, T, _ = ref.regions(V, 0.0, faces=True)
    assert len(T) == 1 and T["points"][0] == length and T["first"][0] == 0
    assert time.time() - t0 < 60


@pytest.mark.parametrize("faces,below", [(False, False), (True, True)])
def test_identities_of_the_table(faces, below):
    V = _field(7, shape=(11, 12, 13)) * np.float32(37.5)
    V[0, 0, 0], V[0, 0, 1] = 0.0, -0.0
    iso = 0.0
    labels, T, s = ref.regions(V, iso, below=below, faces=faces)
    mask = ref.inside(V, iso, below)
    n = int(mask.sum())
    assert T["points"].sum() == n == (labels >= 0).sum() and np.array_equal(labels >= 0, mask)
    assert np.all(np.diff(T["first"].astype(np.int64)) > 0)
    M = float(np.abs(V[mask]).max())
    assert 2.0 ** 29 <= M * 2.0 ** s < 2.0 ** 30
    flat, lab = V.reshape(-1), labels.reshape(-1)
    nz, ny, nx = V.shape
    for r, t in enumerate(T):
        pts = np.nonzero(lab == r)[0]
        assert len(pts) == t["points"] and pts[0] == t["first"]
        ijk = np.stack([pts % nx, (pts // nx) % ny, pts // (nx * ny)], axis=1)
        assert np.array_equal(t["lo"], ijk.min(axis=0)) and np.array_equal(t["hi"], ijk.max(axis=0))
        assert np.array_equal(t["sumIndex"], ijk.sum(axis=0))
        for L in (t["first"], t["argMin"], t["argMax"]):
            p = np.array([L % nx, (L // nx) % ny, L // (nx * ny)])
            assert lab[L] == r and np.all(p >= t["lo"]) and np.all(p <= t["hi"])
        vals = flat[pts]
        assert t["min"] == vals.min() and t["max"] == vals.max()
        assert t["argMin"] == pts[ref.ordered_key(vals) == ref.ordered_key(vals).min()][0]
        assert t["argMax"] == pts[ref.ordered_key(vals) == ref.ordered_key(vals).max()][0]
        assert abs(int(t["sumFixed"])) <= int(t["points"]) << 30
        exact = math.fsum(float(x) for x in vals)
        assert abs(int(t["sumFixed"]) * 2.0 ** -s - exact) <= int(t["points"]) * 2.0 ** -(s + 1)


def test_signed_zeros_order_and_the_empty_lattice():
    V = np.array([[[0.0, -0.0, 0.0, -0.0]]], np.float32)
    labels, T, s = ref.regions(V, 0.0)                              # -0.0 >= 0.0: all four inside, M == 0
    assert s == 0 and len(T) == 1 and T["sumFixed"][0] == 0
    assert (T["argMin"][0], T["argMax"][0]) == (1, 0)
    assert np.signbit(T["min"][0]) and not np.signbit(T["max"][0])
    labels, T, s = ref.regions(np.full((2, 3, 4), np.nan, np.float32), 0.0)
    assert s == 0 and len(T) == 0 and np.all(labels == -1)
    assert ref.REGION.itemsize == 88
