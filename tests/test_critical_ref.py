"""The numpy restatement of exa_hip_critical_points (tests/critical_ref.py) on analytic lattices, without a scene and without
a GPU, held against checks that do not share its arithmetic: n+ and the spiral bit against numpy's eigenvalues of the float64
Jacobian, positions against the analytic zeros, counts against what the fields' zeros give by hand.

The sine field v = (sin(k1 x + 0.3), sin(k2 y + 0.7), sin(k3 z + 1.1)), k = 5 pi (1, 2, 3), on [0,1]^3 has 5 x 10 x 15 = 750
zeros inside the lattice of 48^3 cell centres; the restatement gives 750 candidates, 750 found, n+ = 0..3 for 120 / 305 / 255 /
70 of them (the signs of the three cosines), no spiral and no degenerate point, with 4, 6 and 8 iterations alike; at 24^3 two
zeros of the third component share a cell in places, and the one point per cell leaves 600."""
import numpy as np
import pytest

import critical_ref as ref

F32 = np.float32


def centres(dims, lo, hi):
    """the lattice's coordinates as exa_hip_resample forms them (float32), as float64 arrays x, y, z of shape [nz, ny, nx]"""
    ax = [F32(lo[a]) + (np.arange(dims[a], dtype=F32) + F32(0.5)) * ((F32(hi[a]) - F32(lo[a])) / F32(dims[a])) for a in range(3)]
    z, y, x = np.meshgrid(ax[2].astype(np.float64), ax[1].astype(np.float64), ax[0].astype(np.float64), indexing="ij")
    return x, y, z


K = 5.0 * np.pi * np.array([1.0, 2.0, 3.0])
PHASE = np.array([0.3, 0.7, 1.1])


def sine_lattices(n):
    p = centres((n, n, n), (0, 0, 0), (1, 1, 1))
    return [np.sin(K[c] * p[c] + PHASE[c]).astype(F32) for c in range(3)]


def linear_lattices(A, c, dims=(10, 10, 10), lo=(0, 0, 0), hi=(1, 1, 1)):
    x, y, z = centres(dims, lo, hi)
    p = np.stack([x - c[0], y - c[1], z - c[2]])
    return [np.tensordot(np.asarray(A, np.float64)[r], p, axes=1).astype(F32) for r in range(3)]


# distinct eigenvalues, a trace well away from 0, D well away from 0: (matrix, n+, spiral)
LINEAR = dict(
    sink=([[-1, .5, .2], [0, -2, .3], [.1, 0, -3.5]], 0, False),
    saddle_1=([[1, .5, .2], [0, -2, .3], [.1, 0, -3.5]], 1, False),
    saddle_2=([[1, .5, .2], [0, 2, .3], [.1, 0, -3.5]], 2, False),
    source=([[1, -.5, -.2], [0, 2, -.3], [-.1, 0, 3.5]], 3, False),
    spiral_saddle_2=([[.5, -2, 0], [2, .5, 0], [0, 0, -2]], 2, True),
    spiral_sink=([[-.5, -2, 0], [2, -.5, 0], [0, 0, -1.5]], 0, True),
    spiral_source=([[.5, -2, 0], [2, .5, 0], [.3, 0, 1.5]], 3, True),
    spiral_saddle_1=([[-.5, -2, 0], [2, -.5, 0], [0, .3, 1.5]], 1, True),
)
CENTRE = (0.43, 0.52, 0.61)            # in cell (3, 4, 5) of the 10^3 lattice on [0,1]^3, at s = (0.8, 0.7, 0.6)


def eig_kind(jac):
    """(n+, spiral) from numpy's eigenvalues of a float64 3 x 3 matrix"""
    lam = np.linalg.eigvals(np.asarray(jac, np.float64).reshape(3, 3))
    return int((lam.real > 0).sum()), bool((np.abs(lam.imag) > 0).any())


def check_types_against_eigenvalues(rec):
    for r in rec:
        assert not r["type"] & ref.DEGENERATE, r
        assert (r["type"] & 3, bool(r["type"] & ref.SPIRAL)) == eig_kind(r["jacobian"]), r


def test_linear_matrices_are_what_they_are_called():
    for name, (A, nplus, spiral) in LINEAR.items():
        assert eig_kind(A) == (nplus, spiral), name
        lam = np.linalg.eigvals(np.asarray(A, np.float64))
        assert abs(np.trace(A)) >= 0.5 and min(abs(lam[i] - lam[j]) for i in range(3) for j in range(i)) > 0.4, name


@pytest.mark.parametrize("iterations", [4, 6, 8])
def test_sine_field_counts_types_and_positions(iterations):
    n = 48
    rec, stats, order = ref.critical_points(sine_lattices(n), (0, 0, 0), (1, 1, 1), iterations=iterations)
    print(stats, np.bincount(rec["type"] & 3, minlength=4))
    assert stats == dict(cells=47 ** 3, invalidCells=0, candidates=750, found=750, nonFinite=0, leftCell=0, notConverged=0)
    assert np.bincount(rec["type"] & 3, minlength=4).tolist() == [120, 305, 255, 70] and not (rec["type"] & 12).any()
    assert np.all(np.diff(rec["cell"].astype(np.int64)) > 0) and np.array_equal(order["cells"], rec["cell"])
    check_types_against_eigenvalues(rec)
    # the analytic zeros: k x + phase = m pi.  A linear interpolant of sin(k x) between samples h apart is off by at most
    # h^2 k^2 / 8, which moves its zero by that over the slope, about k: h^2 k / 8 — twice that is allowed (the slope of
    # the chord next to a zero is at least cos(k h) k > k / 2 here)
    h = 1.0 / n
    zeros = [np.array([(m * np.pi - PHASE[c]) / K[c] for m in range(1, 5 * (c + 1) + 1)]) for c in range(3)]
    hit = set()
    for r in rec:
        which = []
        for c in range(3):
            d = np.abs(zeros[c] - float(r["position"][c]))
            assert d.min() <= h * h * K[c] / 4, (r, c, d.min())
            which.append(int(d.argmin()))
        hit.add(tuple(which))
        # the Jacobian is diagonal, k cos(k x + phase), up to the interpolation: its signs are the point's kind
        assert (r["type"] & 3) == sum(np.cos(K[c] * zeros[c][which[c]] + PHASE[c]) > 0 for c in range(3)), r
    assert len(hit) == 750                                      # every zero once


def test_sine_field_at_half_the_resolution_is_limited_by_one_point_per_cell():
    rec, stats, _ = ref.critical_points(sine_lattices(24), (0, 0, 0), (1, 1, 1))
    assert (stats["candidates"], stats["found"]) == (600, 600) and len(np.unique(rec["cell"])) == 600
    check_types_against_eigenvalues(rec)


@pytest.mark.parametrize("name", list(LINEAR))
def test_linear_field_gives_one_point_of_its_kind_in_its_cell(name):
    A, nplus, spiral = LINEAR[name]
    rec, stats, order = ref.critical_points(linear_lattices(A, CENTRE), (0, 0, 0), (1, 1, 1))
    print(name, stats, rec)
    assert stats["found"] == 1 and stats["found"] + stats["nonFinite"] + stats["leftCell"] + stats["notConverged"] == stats["candidates"]
    r = rec[0]
    assert r["cell"] == (5 * 10 + 4) * 10 + 3
    assert r["type"] == nplus | (ref.SPIRAL if spiral else 0)
    check_types_against_eigenvalues(rec)
    # a trilinear interpolant reproduces a linear field: the root is the centre, up to the rounding of the lattice values
    assert np.abs(r["local"].astype(np.float64) - [0.8, 0.7, 0.6]).max() <= 2.0 ** -16
    assert np.abs(r["position"].astype(np.float64) - CENTRE).max() <= 2.0 ** -16 / 10 + 2.0 ** -24
    assert np.abs(r["jacobian"].reshape(3, 3).astype(np.float64) - A).max() <= 1e-4
    lam = np.linalg.eigvals(np.asarray(A, np.float64))
    coeff = np.poly(lam).real                                   # lambda^3 + P lambda^2 + Q lambda + R
    assert np.allclose(r["invariants"], coeff[1:], rtol=0, atol=1e-4)
    assert r["lastStep"] <= 2.0 ** -16


def test_nan_slab_leaves_the_point_and_counts_invalid_cells():
    V = linear_lattices(LINEAR["spiral_saddle_2"][0], CENTRE)
    for v in V[:1]:
        v[:2] = np.nan                                          # two z layers of one component
    rec, stats, _ = ref.critical_points(V, (0, 0, 0), (1, 1, 1))
    assert stats["invalidCells"] == 2 * 81 and stats["found"] == 1 and rec[0]["cell"] == 543
    V[2][9, 9, 9] = np.inf                                      # one more corner: one more cell
    assert ref.critical_points(V, (0, 0, 0), (1, 1, 1))[1]["invalidCells"] == 2 * 81 + 1


@pytest.mark.parametrize("iterations", [2, 8, 32])
def test_zero_plateau(iterations):
    """v = 0 for x below x0, away from the centre: the cells inside the plateau hold constant components and are no
    candidates; in the layer of cells around it the interpolant is s_x G(s_y, s_z), zero on the whole face s_x = 0: the first
    step lands on that face exactly, the second divides 0 by 0 (the header says why), and nothing is found there"""
    V = linear_lattices(LINEAR["spiral_saddle_2"][0], CENTRE)
    for v in V:
        v[:, :, :2] = 0
    rec, stats, order = ref.critical_points(V, (0, 0, 0), (1, 1, 1), iterations=iterations)
    i = order["cells"] % 10
    assert not (i == 0).any()
    assert (i == 1).sum() == 81 and np.all(order["result"][i == 1] == ref.NON_FINITE)
    assert stats["found"] == 1 and rec[0]["cell"] == 543 and stats["nonFinite"] == 81


def _dyadic(c, A=((1, .5, 0), (0, -2, .25), (.5, 0, 4))):
    """A (x - c) on the 8^3 lattice over [0,8]^3, whose points i + 0.5 and values are exact in float32"""
    return linear_lattices(A, c, dims=(8, 8, 8), lo=(0, 0, 0), hi=(8, 8, 8))


def test_a_root_on_a_face_belongs_to_one_cell_by_rule():
    lo, hi = (0, 0, 0), (8, 8, 8)
    # x on the lattice plane i = 3, the face between the cells 2 and 3: s_x = 1 in cell 2 is outside, s_x = 0 in cell 3 inside
    rec, stats, order = ref.critical_points(_dyadic((3.5, 2.25, 5.75)), lo, hi)
    assert stats["found"] == 1 and rec[0]["cell"] == (5 * 8 + 1) * 8 + 3 and rec[0]["local"].tolist() == [0.0, 0.75, 0.25]
    left = order["cells"] == (5 * 8 + 1) * 8 + 2
    assert left.sum() == 1 and order["result"][left][0] == ref.LEFT_CELL
    # x on the lattice's last plane, i = 7: the last cell of the axis, 6, takes s_x = 1
    rec, stats, order = ref.critical_points(_dyadic((7.5, 2.25, 5.75)), lo, hi)
    assert stats["found"] == 1 and rec[0]["cell"] == (5 * 8 + 1) * 8 + 6 and rec[0]["local"].tolist() == [1.0, 0.75, 0.25]
    assert rec[0]["position"].tolist() == [7.5, 2.25, 5.75]
    # on the last planes of all three axes: the last cell of the lattice
    rec, stats, _ = ref.critical_points(_dyadic((7.5, 7.5, 7.5)), lo, hi)
    assert stats["found"] == 1 and rec[0]["cell"] == (6 * 8 + 6) * 8 + 6 and rec[0]["local"].tolist() == [1.0, 1.0, 1.0]


def test_degenerate_bit():
    lo, hi = (0, 0, 0), (8, 8, 8)
    # a trace of exactly zero: P == 0, the Routh column's third entry is not finite
    rec, stats, _ = ref.critical_points(_dyadic((3.25, 2.25, 5.75), A=((1, 0, 0), (0, 1, 0), (0, 0, -2))), lo, hi)
    assert stats["found"] == 1 and rec[0]["type"] & ref.DEGENERATE and rec[0]["invariants"][0] == 0.0
    # a singular matrix with no constant component: every candidate divides by a determinant of exactly 0
    rec, stats, order = ref.critical_points(_dyadic((3.25, 2.25, 5.75), A=((1, 0, 0), (0, 1, 0), (1, 1, 0))), lo, hi)
    assert stats["candidates"] > 0 and stats["found"] == 0 and stats["nonFinite"] == stats["candidates"]
    # the classification alone: a singular Jacobian has R == 0, a rotation in a plane P Q - R == 0
    kind, inv, _ = ref.classify(np.array([[1, 0, 0, 0, 1, 0, 1, 1, 0], [0, -1, 0, 1, 0, 0, 0, 0, -1], [-1, .5, .25, 0, -2, .5, 0, 0, -3]], F32))
    assert inv[0][2] == 0.0 and kind[0] & ref.DEGENERATE
    assert inv[1][0] * inv[1][1] - inv[1][2] == 0.0 and kind[1] & ref.DEGENERATE
    assert kind[2] == 0
    # a constant component is never a candidate
    assert ref.critical_points(_dyadic((3.25, 2.25, 5.75), A=((1, 0, 0), (0, 1, 0), (0, 0, 0))), lo, hi)[1]["candidates"] == 0


def test_iterations_and_tolerance():
    V = sine_lattices(24)
    one = ref.critical_points(V, (0, 0, 0), (1, 1, 1), iterations=1, tolerance=1.0)[1]
    tight = ref.critical_points(V, (0, 0, 0), (1, 1, 1), iterations=1, tolerance=2.0 ** -20)[1]
    assert one["candidates"] == tight["candidates"] == 600 and tight["notConverged"] > 0 and one["found"] > tight["found"]
    for st in (one, tight):
        assert st["found"] + st["nonFinite"] + st["leftCell"] + st["notConverged"] == st["candidates"]


def test_record_layout():
    assert ref.POINT_DTYPE.itemsize == 104 and ref.POINT_DTYPE.fields["invariants"][1] == 72
