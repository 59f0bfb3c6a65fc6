"""tests/derived_ref.py, the numpy statement of the derived flow quantities, on velocity gradient tensors whose quantities are
known in closed form (no GPU needed)."""
import numpy as np

import derived_ref as dr


def _all(v, J):
    return {name: dr.derived(q, np.array([v], np.float32), np.array([J], np.float32)) for name, q in dr.QUANTITIES.items()}


def test_rigid_rotation():
    """v = omega x r with omega = (1, 2, 3): vorticity 2 omega, no divergence, Q = |omega|^2, all exact in float32"""
    r = _all((1, 2, 3), [[0, -3, 2], [3, 0, -1], [-2, 1, 0]])
    assert all(x.dtype == np.float32 for x in r.values())
    assert r["vorticity"].shape == (1, 3) and np.array_equal(r["vorticity"][0], [2, 4, 6])
    assert r["divergence"][0] == 0 and r["q"][0] == 14 and r["helicity"][0] == 28
    assert r["vorticity_magnitude"][0] == np.sqrt(np.float32(56)) and r["speed"][0] == np.sqrt(np.float32(14))


def test_uniform_expansion():
    """v = a r: divergence 3a, no vorticity, Q = -3/2 a^2"""
    a = 0.75
    r = _all((a, 2 * a, -a), [[a, 0, 0], [0, a, 0], [0, 0, a]])
    assert r["divergence"][0] == np.float32(3 * a) and r["q"][0] == np.float32(-1.5 * a * a)
    assert np.array_equal(r["vorticity"][0], [0, 0, 0]) and r["vorticity_magnitude"][0] == 0 and r["helicity"][0] == 0
    assert r["speed"][0] == np.sqrt(np.float32(6 * a * a))


def test_nan_reaches_exactly_the_quantities_that_read_its_entry():
    J = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    # J01 is read by the vorticity's z component and by Q's off-diagonal sum
    Jn = [[1, np.nan, 3], [4, 5, 6], [7, 8, 9]]
    r, want = _all((1, 2, 3), Jn), _all((1, 2, 3), J)
    assert np.array_equal(np.isnan(r["vorticity"][0]), [False, False, True])
    assert np.array_equal(r["vorticity"][0, :2], want["vorticity"][0, :2])
    for name in ("vorticity_magnitude", "q", "helicity"):
        assert np.isnan(r[name][0]), name
    for name in ("speed", "divergence"):
        assert r[name][0] == want[name][0], name
    # J11 is read by the divergence and by Q's diagonal sum alone
    r = _all((1, 2, 3), [[1, 2, 3], [4, np.nan, 6], [7, 8, 9]])
    assert np.isnan(r["divergence"][0]) and np.isnan(r["q"][0])
    for name in ("speed", "vorticity", "vorticity_magnitude", "helicity"):
        assert np.array_equal(r[name], want[name]), name
    # v1 is read by speed and helicity alone
    r = _all((1, np.nan, 3), J)
    assert np.isnan(r["speed"][0]) and np.isnan(r["helicity"][0])
    for name in ("divergence", "vorticity", "vorticity_magnitude", "q"):
        assert np.array_equal(r[name], want[name]), name


def test_from_probe_takes_the_worst_status_and_fills():
    v = np.ones((4, 3), np.float32)
    J = np.ones((4, 3, 3), np.float32)
    st = np.array([[5, 5, 5], [5, -2, 5], [-1, -1, -1], [7, 7, -2]], np.int32)
    out, s = dr.from_probe(dr.VORTICITY, v, J, st, -7.5)
    assert np.array_equal(s, [5, -2, -1, -2]) and out.shape == (4, 3)
    assert np.array_equal(out[0], [0, 0, 0]) and np.all(out[1:] == np.float32(-7.5))
