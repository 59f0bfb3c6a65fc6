"""The numpy restatement of exa_hip_streamlines' contract (tests/streamline_ref.py), held on the CPU: its forward,
unnormalised line equals the oracle's tracer point for point wherever the tracer keeps a trace alive; on a rotation field
it follows float64 RK4 of the analytic field within a stated multiple of the float32 rounding; and the seeds the GPU test
uses reach every end reason, so that test cannot pass on empty ground."""
import numpy as np
import pytest

import streamline_ref as sr
from common import Case
from owlexabrick_amd import scenes
from probe_ref64 import bound_from
from test_tracer import tracer_case


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("form", [0, 1])
def test_forward_line_equals_the_oracle_tracer(form):
    case, seeds = tracer_case(None)
    case.basis_form = form
    opaque = case.xfs[0].copy()
    opaque[:, 3] = 1.0                                  # all regions visible: the tracer looks regions up through the active set
    case.xfs = [opaque] * len(case.xfs)
    S = case.oracle_scene()
    S.reset_tracer(True, (0, 1, 2), len(seeds), 6, 6.0, seeds)
    for _ in range(5):
        S.advance_tracer()
        fs, P = case.oracle_state(S)
        S.render(fs, P, case.W, case.H, nthreads=4)
    T = S.traces()
    ref = sr.StreamRef(S, (0, 1, 2), normalize=False)
    compared = 0
    for i, seed in enumerate(seeds):
        verts, _, _, _ = ref.line(seed, 6.0, 5)
        alive = int((T[i, :, 0] < 2e10).sum())          # once out, stays out (tests/test_tracer.py)
        assert len(verts) >= alive, (i, len(verts), alive)
        assert np.array_equal(_bits(verts[:alive]), _bits(T[i, :alive])), i
        compared += max(alive - 1, 0)                   # vertex 0 is the seed, copied by both sides: not counted
    print(f"form {form}: {compared} integrated trace points compared")
    assert compared >= 150


@pytest.mark.parametrize("form", [0, 1])
def test_rotation_field_follows_float64_rk4(form):
    case = Case(sr.rotation_scene(), basis_form=form)
    S = case.oracle_scene()
    assert S.num_regions == 75
    seeds = sr.rotation_seeds()
    step, steps = 0.125, 60
    got = sr.streamlines(S, seeds, channels=(1, 2, 3), step=step, max_steps=steps)
    verts, offsets, seed_vertex, reasons, _ = got
    assert np.all(reasons[:, 1] == sr.END_MAXSTEPS) and np.all(reasons[:, 0] == sr.END_NONE)
    assert np.array_equal(offsets, np.arange(len(seeds) + 1, dtype=np.uint64) * (steps + 1)) and not seed_vertex.any()
    want = sr.rotation_rk4_64(seeds, step, steps)
    err = np.abs(verts.reshape(len(seeds), steps + 1, 3).astype(np.float64) - want).max(axis=2)
    unit = 2.0 ** -24 * 12.0 * np.arange(1, steps + 1)
    k = float((err[:, 1:] / unit).max())
    print(f"form {form}: error against float64 RK4 {k:.4f} x 2^-24 * 12 * steps (recorded {sr.ROTATION_K_MEASURED[form]})")
    assert k <= bound_from(sr.ROTATION_K_MEASURED[form]), k


SETTINGS = [(True, False), (True, True), (False, False), (False, True)]      # (forward, normalize)


def _run(S, channels, forward, normalize):
    seeds = sr.uniform_seeds(S)
    return sr.streamlines(S, seeds, channels=channels, step=0.5, max_steps=40, forward=forward, backward=not forward,
                          normalize=normalize)


def test_amr3_reaches_left_and_maxsteps():
    S = Case(scenes.amr(levels=3, fields=3), basis_form=1).oracle_scene()
    for forward, normalize in SETTINGS:
        res = _run(S, (0, 1, 2), forward, normalize)
        n = sr.reason_counts(res[3], 1 if forward else 0)
        print(f"amr3 forward {forward} normalize {normalize}: {n}")
        assert n[sr.END_LEFT] >= 15 and n[sr.END_MAXSTEPS] >= 15, (forward, normalize, n)


def test_empty_cells_reach_novalue():
    sc = scenes.with_empty_cells(scenes.amr(levels=3, fields=3), fraction=0.15)
    S = Case(sc, basis_form=0, allow_empty_cells=True).oracle_scene()
    total = 0
    for forward, normalize in SETTINGS:
        res = _run(S, (0, 1, 2), forward, normalize)
        n = sr.reason_counts(res[3], 1 if forward else 0)
        print(f"amr3_holes forward {forward} normalize {normalize}: {n}")
        total += n[sr.END_NOVALUE]
    assert total >= 1


@pytest.mark.parametrize("normalize", [False, True])
def test_zero_field_stagnates_after_one_vertex(normalize):
    S = Case(sr.zero_fields_scene(), basis_form=1).oracle_scene()
    seeds = sr.uniform_seeds(S)
    ref = sr.StreamRef(S, (1, 2, 3))
    inside = np.array([ref.owner(s) >= 0 for s in seeds])
    assert inside.sum() >= 10 and (~inside).sum() >= 1
    verts, offsets, seed_vertex, reasons, _ = sr.streamlines(S, seeds, channels=(1, 2, 3), step=0.5, max_steps=40, forward=True,
                                                              backward=True, normalize=normalize)
    assert np.array_equal(offsets, np.arange(len(seeds) + 1, dtype=np.uint64))      # one vertex each
    assert np.all(reasons[inside] == sr.END_STAGNANT) and np.all(reasons[~inside] == sr.END_LEFT)


@pytest.mark.parametrize("normalize", [False, True])
def test_a_nan_velocity_ends_a_line_left_or_stagnant(normalize):
    """tests/nan_scenes.py: 1 % of the cells NaN in one of three channels (the case tests/test_gpu_nan_cells.py holds the
    module to).  A NaN velocity is a value: the line ends at the next evaluation — LEFT at the NaN position without
    EXA_STREAM_NORMALIZE, STAGNANT by !(s > 0) with it — and no NaN position is appended"""
    import nan_scenes as ns
    S = ns.case(ns.flow_scene(), basis_form=1).oracle_scene()
    seeds = sr.uniform_seeds(S, ns.FLOW_SEEDS)
    v, off, _, reasons, w = sr.streamlines(S, seeds, ns.FLOW_CHANNELS, ns.FLOW_STEP, ns.FLOW_MAX_STEPS, True, False, normalize)
    ended = ns.directions_ended_by_nan(S, seeds, ns.FLOW_STEP, ns.FLOW_MAX_STEPS, normalize)
    print(f"normalize {normalize}: {int(ended.sum())} lines end for a NaN velocity; {sr.reason_counts(reasons, 1)}")
    assert ended.sum() >= 5 and (~ended).sum() >= 5
    assert np.all(reasons[ended, 1] == (sr.END_STAGNANT if normalize else sr.END_LEFT))
    assert not np.isnan(v).any()
    first, last = off[:-1].astype(np.int64), off[1:].astype(np.int64) - 1
    failed_seed = np.zeros(len(w), dtype=bool)
    failed_seed[first[np.isnan(w[first]).all(axis=1)]] = True           # a failed seed's velocity is three NaN by contract
    assert failed_seed.sum() >= 1 and np.all((last - first)[failed_seed[first]] == 0)
    nan_vertex = np.isnan(w).any(axis=1) & ~failed_seed
    if normalize:
        assert not nan_vertex.any()                                   # the evaluation that meets the NaN fails: nothing is appended
    else:
        # the vertex whose own velocity is NaN is appended (its position is finite) and is the last of its line
        assert set(np.nonzero(nan_vertex)[0]) <= set(last[ended]) and nan_vertex.sum() >= 1
