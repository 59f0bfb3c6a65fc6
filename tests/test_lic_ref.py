"""The numpy restatement of exa_hip_lic's contract (tests/lic_ref.py), held on the CPU: the noise hash's known answers; on a
uniform field along du, where the RK4 step lands exactly on a + step, its sums, counts and reasons equal a clipped running box
sum of the noise rows computed with numpy alone; and the inputs the GPU test uses reach every end reason, the failed and the
stagnant centre, so that test cannot pass on empty ground."""
import numpy as np
import pytest

import lic_ref as lr
from common import Case

F = np.float32


def test_hash_known_answers():
    for (ix, iy, seed), want in (((1, 0, 0), 109), ((0, 1, 0), 196), ((3, 5, 7), 178), ((66, 44, 1), 71)):
        assert int(lr.hash_noise(ix, iy, seed)) == want, (ix, iy, seed)
    img = lr.hash_image(67, 45, 1)
    assert img.shape == (45, 67) and img.dtype == np.uint8 and img[44, 66] == 71
    assert int(lr.hash_noise(np.array([3]), np.array([5]), 7)[0]) == 178


@pytest.mark.parametrize("step", [1.0, 0.5, 0.75, 2.0 ** -6])
def test_rk4_step_lands_on_a_plus_step(step):
    # what the closed form rests on: with d = (1, 0) the step's float32 operations give c + step exactly
    hs = F(step)
    for sign in (F(1), F(-1)):
        k = sign * hs
        inc = (F(1) / F(6)) * (((k + F(2) * k) + F(2) * k) + k)
        assert inc.dtype == F and inc == k
    a = np.arange(0, 72 * 64, dtype=np.float64) / 64.0 + 0.5
    assert np.array_equal((a.astype(F) + hs).astype(np.float64), a + step)


_uniform = {}


def _uniform_oracle():
    if not _uniform:
        _uniform["S"] = Case(lr.uniform_scene(3), basis_form=1).oracle_scene()
    return _uniform["S"]


@pytest.mark.parametrize("half_length", [1, 6, 4096])
@pytest.mark.parametrize("step", [1.0, 0.5, 0.75, 2.0 ** -6])
def test_uniform_field_equals_the_running_box_sum(step, half_length):
    S = _uniform_oracle()
    nu, nv = 7, 2
    noise = lr.hash_image(nu, nv, 5)
    got = lr.lic(lr.oracle_evaluator(S, (1, 2, 3)), lr.uniform_plane(nu, nv), step, half_length, noise=noise)
    total, count, reasons = lr.uniform_closed_form(noise, step, half_length)
    assert np.array_equal(got["sum"], total) and np.array_equal(got["count"], count) and np.array_equal(got["reasons"], reasons)
    assert np.array_equal(got["lic"].view(np.uint32), (total.astype(F) / count.astype(F)).view(np.uint32))
    assert np.all(got["speed"] == 1.0)
    if half_length == 4096:
        assert np.all(reasons == lr.END_IMAGE) and count.max() > 1
    # the hash instead of the array: the same bytes
    lr.same(lr.lic(lr.oracle_evaluator(S, (1, 2, 3)), lr.uniform_plane(nu, nv), step, min(half_length, 6), seed=5),
            lr.lic(lr.oracle_evaluator(S, (1, 2, 3)), lr.uniform_plane(nu, nv), step, min(half_length, 6), noise=noise), "hash")


def test_closed_form_reaches_maxsteps_on_the_wide_image():
    # the 67 x 3 image of the GPU test at L = 4096, step 2^-6: numpy alone
    total, count, reasons = lr.uniform_closed_form(lr.hash_image(67, 3, 0), 2.0 ** -6, 4096)
    assert (reasons[:, :, 1] == lr.END_MAXSTEPS).sum() == 3 * 3 and (reasons[:, :, 0] == lr.END_MAXSTEPS).sum() == 3 * 3
    # pixel 0: 32 samples backward (down to a = 0), 4096 forward; pixel 66: 31 forward (a < 67), 4096 backward; a pixel clipped
    # on both sides: every 1/64 of the row once
    assert count[0, 0] == 1 + 32 + 4096 and count.min() == 1 + 31 + 4096 and count.max() == 67 * 64
    assert int(total.max()) <= 8193 * 255


# what each input of the GPU test must reach: {reason or centre kind: at least this many}
WANT = {
    "rotation": {lr.END_MAXSTEPS: 40, lr.END_LEFT: 20, lr.END_IMAGE: 4, "failed_centre": 20},
    "amr3_oblique": {lr.END_MAXSTEPS: 10, lr.END_LEFT: 4, "failed_centre": 2},
    "amr3_holes": {lr.END_NOVALUE: 1},
    "zero": {lr.END_STAGNANT: 20, "stagnant_centre": 10, "failed_centre": 1},
    "normal": {"stagnant_centre": 20},
}


@pytest.mark.parametrize("idx", range(len(lr.CASES)), ids=[c[0] for c in lr.CASES])
def test_inputs_of_the_gpu_test_reach_every_reason(idx):
    name, make, channels, forms, empty, pl, step, L = lr.CASES[idx]
    S = Case(make(), basis_form=forms[-1], allow_empty_cells=empty).oracle_scene()
    res = lr.lic(lr.oracle_evaluator(S, channels), pl, step, L, seed=idx)
    n = lr.reason_counts(res)
    print(name, n)
    for k, least in WANT[name].items():
        assert n[k] >= least, (name, k, n)
    # a stagnant centre counts its own sample, a failed one nothing; the sums stay within the box filter's bound
    assert np.all(res["count"] <= 1 + 2 * L) and np.all(res["sum"] <= res["count"] * 255)
    assert np.all(np.isnan(res["lic"][res["count"] == 0])) and np.all(np.isnan(res["speed"][res["count"] == 0]))


def test_every_reason_occurs_somewhere():
    seen = set()
    for idx, (name, make, channels, forms, empty, pl, step, L) in enumerate(lr.CASES):
        seen |= set(WANT[name])
    assert {lr.END_MAXSTEPS, lr.END_LEFT, lr.END_NOVALUE, lr.END_STAGNANT, lr.END_IMAGE, "failed_centre", "stagnant_centre"} <= seen


def test_refused_planes():
    assert lr.metric(lr.plane((0, 0, 0), (1, 0, 0), (2, 0, 0), (4, 4))) is None              # parallel
    assert lr.metric(lr.plane((0, 0, 0), (0, 0, 0), (0, 1, 0), (4, 4))) is None              # a zero vector
    assert lr.metric(lr.plane((0, 0, 0), (1e30, 0, 0), (0, 1e30, 0), (4, 4))) is None        # det overflows
    assert lr.metric(lr.oblique_plane()) is not None


def test_a_nan_velocity_ends_a_direction_stagnant():
    """tests/nan_scenes.py: the case tests/test_gpu_nan_cells.py holds the module to.  A NaN velocity is a value; the speed of
    the in-plane direction is then NaN and !(s > 0) ends the direction STAGNANT (a NaN centre: both, count 1)"""
    import nan_scenes as ns
    S = ns.case(ns.flow_scene(), basis_form=1).oracle_scene()
    evaluate = ns.counting_evaluator(lr.oracle_evaluator(S, ns.FLOW_CHANNELS))
    res = lr.lic(evaluate, lr.plane(*ns.FLOW_PLANE), ns.FLOW_LIC_STEP, ns.FLOW_LIC_HALF_LENGTH, seed=4)
    n = lr.reason_counts(res)
    print(evaluate.nan, n)
    # every evaluation with a NaN velocity ends its direction (a NaN centre: both directions, counted once)
    assert evaluate.nan >= 5 and n[lr.END_STAGNANT] >= evaluate.nan and n[lr.END_MAXSTEPS] >= 50
    nan_centre = np.isnan(res["speed"]) & (res["count"] == 1)
    assert np.all(res["reasons"][nan_centre] == lr.END_STAGNANT)
    assert not np.isnan(res["lic"][res["count"] > 0]).any()
