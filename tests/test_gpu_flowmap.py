"""exa_hip_flowmap on the GPU (include/exa_hip.h): end, steps, reasons and stretch equal the numpy restatement of the contract
(tests/flowmap_ref.py) byte for byte — fed by the CPU oracle on small lattices, in both basis forms and with empty cells,
forward and backward, at 1 and 12 steps, and by the point probes on lattice shapes that break a patch map and on a long
integration —, with both values of flowmap_patch, with a NaN, a finite and an infinite fill, with host or device arrays; the
flow map equals what exa_hip_streamlines returns for the same seeds; and nothing a frame sets changes a byte."""
import ctypes as C
import time

import numpy as np
import pytest

import flowmap_ref as fr
import lic_ref as lr
import streamline_ref as sr
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from probe_sets import grid_positions

pytestmark = pytest.mark.gpu

F = np.float32
PARAMS = [(i, f) for i, c in enumerate(fr.CASES) for f in c[3]]
IDS = [f"{fr.CASES[i][0]}-f{f}" for i, f in PARAMS]

_cache = {}


def _setup(idx, form):
    if (idx, form) not in _cache:
        name, make, channels, _, empty, box, step = fr.CASES[idx]
        case = Case(make(), basis_form=form, allow_empty_cells=empty, W=32, H=32)
        _cache[(idx, form)] = (case, case.hip_renderer())
    return _cache[(idx, form)]


def _amr3():
    """the renderer of the amr3 case in form 1 (scenes.amr(levels=3, fields=4)) and its channels"""
    return _setup(1, 1)[1], fr.CASES[1][2]


def _patches(R):
    for patch in (0, 1):                                        # ends on the default
        R.setOption("flowmap_patch", patch)
        yield f"patch {patch}"


def _ftle_follows(got, step, num_steps, fill=np.nan):
    want = fr.ftle(got["stretch"], step, num_steps, fill)
    assert got["ftle"].dtype == F and np.array_equal(got["ftle"].view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("idx,form", PARAMS, ids=IDS)
def test_equals_the_oracle_fed_restatement_byte_for_byte(idx, form):
    from test_flowmap_ref import reaches
    name, make, channels, _, empty, box, step = fr.CASES[idx]
    case, R = _setup(idx, form)
    for dims in fr.LATTICES:
        lo, hi = box(dims)
        for num_steps in fr.NUM_STEPS:
            for backward in (False, True):
                want = fr.case_result(idx, form, dims, num_steps, backward)
                if num_steps == 12:                             # the reference test's coverage, on what is compared here
                    print(name, form, dims, backward, reaches(name, dims, want))
                for what in _patches(R):
                    got = R.flowmap(lo, hi, dims, channels, step, num_steps, backward)
                    fr.same(got, want, (name, form, dims, num_steps, backward, what))
                _ftle_follows(got, step, num_steps)
    # a finite fill, and an infinite one, land where the point or a stencil point is not valid; the flow map is the same
    dims = fr.LATTICES[1]
    lo, hi = box(dims)
    want = fr.case_result(idx, form, dims, 12, False)
    assert np.isnan(want["stretch"]).any()
    for fill in (-7.5, np.inf):
        got = R.flowmap(lo, hi, dims, channels, step, 12, fill=fill)
        fr.same(got, fr.with_fill(want, fill), (name, form, fill))
        _ftle_follows(got, step, 12, fill)
        assert np.all(got["ftle"][np.isnan(want["stretch"])] == F(fill))


@pytest.mark.parametrize("dims", fr.SHAPES, ids=lambda d: "x".join(map(str, d)))
def test_shapes_that_break_a_patch_map(dims):
    R, channels = _amr3()
    # inside the volume (48 x 48 x 32), oblique to nothing: what matters is which lane takes which point
    lo = (6.0, 8.0, 7.0)
    hi = tuple(a + min(0.6 * n, b) for a, n, b in zip(lo, dims, (42.0, 40.0, 26.0)))
    for num_steps, backward in ((1, False), (7, True)):
        want = fr.flowmap(fr.stepper_feed(lr.probe_evaluator(R, channels)), lo, hi, dims, 0.5, num_steps, backward)
        assert fr.valid(want["reasons"]).all() and (want["steps"] == num_steps).all()
        assert np.isfinite(want["stretch"]).all()              # also for an axis of one point: its column is zero
        for what in _patches(R):
            fr.same(R.flowmap(lo, hi, dims, channels, 0.5, num_steps, backward), want, (dims, num_steps, what))


def test_larger_lattice_equals_the_probe_fed_restatement():
    R, channels = _amr3()
    lo, hi, dims = (-4.0, -3.0, 2.0), (50.0, 47.0, 30.5), (37, 21, 6)
    for backward in (False, True):
        want = fr.flowmap(fr.stepper_feed(lr.probe_evaluator(R, channels)), lo, hi, dims, 0.5, 12, backward)
        n = fr.coverage(want)
        print(n)
        assert n[fr.END_MAXSTEPS] >= 2000 and n[fr.END_LEFT] >= 300 and n["failed_seed"] >= 200 and n["through_neighbour"] >= 100
        for what in _patches(R):
            fr.same(R.flowmap(lo, hi, dims, channels, 0.5, 12, backward), want, (backward, what))


@pytest.mark.parametrize("backward", [False, True])
def test_flow_map_equals_the_streamlines_of_the_same_seeds(backward):
    # the existing call, on the GPU, with no numpy in between
    R, channels = _amr3()
    lo, hi, dims = (-4.0, -3.0, 2.0), (50.0, 47.0, 30.5), (13, 9, 5)
    got = R.flowmap(lo, hi, dims, channels, 0.5, 12, backward)
    verts, offsets, _, reasons, _ = R.streamlines(grid_positions(lo, hi, dims), channels, step=0.5, max_steps=12,
                                                  forward=not backward, backward=backward)
    offsets = offsets.astype(np.int64)
    # a backward line is stored farthest vertex first
    last = verts[offsets[:-1]] if backward else verts[offsets[1:] - 1]
    assert np.array_equal(got["end"].reshape(-1, 3).view(np.uint32), last.view(np.uint32))
    assert np.array_equal(got["steps"].ravel(), (offsets[1:] - offsets[:-1] - 1).astype(np.uint32))
    assert np.array_equal(got["reasons"].ravel(), reasons[:, 0 if backward else 1])
    assert len(set(got["reasons"].ravel().tolist())) >= 2 and got["steps"].max() == 12


def test_a_long_integration():
    # 4096 steps of 2^-9 on the rotation scene: a little more than one revolution, 2 voxels up; the lines stay inside
    case, R = _setup(0, 1)
    lo, hi, dims, step, n = (4.0, 5.0, 2.0), (8.5, 7.0, 3.0), (3, 2, 1), 2.0 ** -9, 4096
    t0 = time.perf_counter()
    want = fr.flowmap(fr.stepper_feed(lr.probe_evaluator(R, (1, 2, 3))), lo, hi, dims, step, n)
    t1 = time.perf_counter()
    assert (want["reasons"] == fr.END_MAXSTEPS).all() and (want["steps"] == n).all()
    for what in _patches(R):
        fr.same(R.flowmap(lo, hi, dims, (1, 2, 3), step, n), want, what)
    print(f"long integration: restatement {t1 - t0:.2f} s, module {time.perf_counter() - t1:.2f} s, integrate {R.flowmapMs()[0]:.3f} ms")
    # against float64 RK4 of the analytic field (a rigid rotation does not amplify an error): a step's p + increment rounds by
    # at most half an ulp of a coordinate below 8, 2^-22, and what the small increment itself carries is far below that; twice
    # that per step
    P = fr.positions(lo, hi, dims).astype(np.float64)
    ref = sr.rotation_rk4_64(P, step, n)[:, -1]
    err = np.abs(want["end"].reshape(-1, 3) - ref).max()
    print(f"long integration: |end - float64 RK4| <= {err:.3e}")
    assert err <= n * 2.0 ** -21


def _dyadic_lattice():
    """a lattice of amr3 whose positions have few bits: lo +- 0.5 around a point is exact"""
    return (2.0, 3.0, 1.0), (42.0, 31.0, 25.0), (5, 4, 3)


def test_point_of_a_batch_equals_the_one_point_call():
    R, channels = _amr3()
    lo, hi, dims = _dyadic_lattice()
    batch = R.flowmap(lo, hi, dims, channels, 0.5, 12)
    P = fr.positions(lo, hi, dims)
    for L in (0, 7, 23, 38, 59):
        p = P[L].astype(np.float64)
        one = R.flowmap(p - 0.5, p + 0.5, (1, 1, 1), channels, 0.5, 12)
        for k in ("end", "steps", "reasons"):
            a, b = one[k].reshape(-1), batch[k].reshape(len(P), -1)[L]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (L, k)


def test_host_and_device_pointers_two_calls_and_null_outputs():
    import torch
    R, channels = _amr3()
    L = binding.lib()
    lo, hi, dims = (-4.0, -3.0, 2.0), (50.0, 47.0, 30.5), (37, 21, 6)
    nx, ny, nz = dims
    want = R.flowmap(lo, hi, dims, channels, 0.5, 8)
    fr.same(R.flowmap(lo, hi, dims, channels, 0.5, 8), want, "two calls")
    assert R.flowmapMs()[0] > 0.0 and R.flowmapMs()[1] > 0.0
    dev = torch.device("cuda:0")
    dtypes = dict(end=torch.float32, steps=torch.int32, reasons=torch.int32, stretch=torch.float32)
    fresh = lambda: {k: torch.full((nz, ny, nx, 3) if k == "end" else (nz, ny, nx), 77, dtype=t, device=dev) for k, t in dtypes.items()}   # noqa: E731
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])      # noqa: E731
    ch, d3 = (C.c_int32 * 3)(*channels), (C.c_int32 * 3)(*dims)

    def call(out, keys, device=1):
        ptr = lambda k: (C.c_void_p(out[k].data_ptr()) if device else out[k].ctypes.data) if k in keys else None     # noqa: E731
        rc = L.exa_hip_flowmap(R.h, f3(lo), f3(hi), d3, ch, 0.5, 8, binding.FLOWMAP_FORWARD, float("nan"), ptr("end"), ptr("steps"),
                               ptr("reasons"), ptr("stretch"), device, None)
        assert rc == 0, L.exa_hip_last_error(R.h).decode()

    out = fresh()
    call(out, fr.KEYS)
    torch.cuda.synchronize()
    fr.same({k: out[k].cpu().numpy().view(want[k].dtype) for k in fr.KEYS}, want, "device pointers")
    # NULL outputs are skipped, and the stretch alone works on a flow map the call keeps to itself: on the device ...
    for keys in (("stretch",), ("end", "stretch"), ("reasons", "stretch"), ("steps",), ("end", "reasons")):
        out = fresh()
        call(out, keys)
        torch.cuda.synchronize()
        for k in fr.KEYS:
            got = out[k].cpu().numpy().view(want[k].dtype)
            assert np.array_equal(got.view(np.uint32), want[k].view(np.uint32)) == (k in keys), (keys, k)
            assert k in keys or bool((out[k] == 77).all()), (keys, k)
    # ... and on the host; and none at all
    for keys in (("stretch",), ("end", "steps"), ()):
        host = {k: np.full(want[k].shape, 77, want[k].dtype) for k in fr.KEYS}
        call(host, keys, device=0)
        for k in fr.KEYS:
            assert np.array_equal(host[k].view(np.uint32), want[k].view(np.uint32)) == (k in keys), (keys, k)


def test_bytes_do_not_depend_on_the_frame_state_or_options():
    case = Case(scenes.amr(levels=3, fields=4), W=32, H=32)
    R = case.hip_renderer()
    (lo, hi, dims), channels = _dyadic_lattice(), (1, 3, 0)
    want = R.flowmap(lo, hi, dims, channels, 0.5, 12, backward=True)
    fr.same(want, _amr3()[0].flowmap(lo, hi, dims, channels, 0.5, 12, backward=True), "another handle")
    for what in frame_perturbations(case, R):
        fr.same(R.flowmap(lo, hi, dims, channels, 0.5, 12, backward=True), want, what)
    R.close()


def test_multi_device_handle_equals_single():
    R, channels = _amr3()
    lo, hi, dims = _dyadic_lattice()
    M = multi_handle(R, 1)
    for what in _patches(M):
        fr.same(M.flowmap(lo, hi, dims, channels, 0.5, 12), R.flowmap(lo, hi, dims, channels, 0.5, 12), "multi " + what)
    assert M.flowmapMs()[0] > 0.0
    M.close()


def test_scene_without_kd_tree_is_refused():
    R = binding.Renderer(without_kd_tree(binding.Prep(scenes.amr(levels=3, fields=3))))
    with pytest.raises(RuntimeError, match="exa_hip_flowmap: .*kd-tree"):
        R.flowmap(*_dyadic_lattice())
    assert R.flowmapMs() == (0.0, 0.0)
    R.close()


def test_bad_arguments_are_refused_and_the_handle_stays_usable():
    R, channels = _amr3()
    L = binding.lib()
    lo, hi, dims = _dyadic_lattice()
    want = R.flowmap(lo, hi, dims, channels, 0.5, 6)
    buf = {k: np.zeros(want[k].shape, want[k].dtype) for k in fr.KEYS}
    f3 = lambda v: None if v is None else (C.c_float * 3)(*[float(x) for x in v])      # noqa: E731
    i3 = lambda v: None if v is None else (C.c_int32 * 3)(*[int(x) for x in v])        # noqa: E731

    def call(lo=lo, hi=hi, dims=dims, ch=channels, step=0.5, num_steps=6, flags=binding.FLOWMAP_FORWARD, fill=float("nan")):
        rc = L.exa_hip_flowmap(R.h, f3(lo), f3(hi), i3(dims), i3(ch), step, num_steps, flags, fill,
                               *[buf[k].ctypes.data for k in fr.KEYS], 0, None)
        return rc, L.exa_hip_last_error(R.h).decode()

    nan, inf = float("nan"), float("inf")
    bad = [(dict(lo=None), "null"), (dict(hi=None), "null"), (dict(dims=None), "null"), (dict(ch=None), "null"),
           (dict(lo=(nan, 3, 1)), "finite lo < hi"), (dict(hi=(42, inf, 25)), "finite lo < hi"), (dict(hi=(2, 31, 25)), "finite lo < hi"),
           (dict(lo=(2, 3, 26)), "finite lo < hi"),
           (dict(dims=(0, 4, 3)), "dims"), (dict(dims=(5, -1, 3)), "dims"), (dict(dims=(65536, 32768, 1)), "2^31"),
           (dict(dims=(2048, 2048, 1024)), "2^31"), (dict(dims=(2 ** 31 - 1, 2 ** 31 - 1, 2)), "2^31"),
           (dict(ch=(0, 1, 4)), "channel"), (dict(ch=(-1, 1, 2)), "channel"),
           (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=nan), "step"), (dict(step=inf), "step"),
           (dict(num_steps=0), "numSteps"), (dict(num_steps=binding.STREAM_MAX_STEPS + 1), "numSteps"),
           (dict(flags=0), "direction"), (dict(flags=binding.FLOWMAP_FORWARD | binding.FLOWMAP_BACKWARD), "direction"),
           (dict(flags=binding.FLOWMAP_FORWARD | 4), "flag"), (dict(flags=1 << 30), "flag")]
    for kw, match in bad:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("exa_hip_flowmap: ") and match in msg, (kw, rc, msg)
        assert R.flowmapMs() == (0.0, 0.0)
        rc, msg = call()                                            # ... and the handle still computes
        assert rc == 0, msg
        fr.same(buf, want, kw)
        assert R.flowmapMs()[0] > 0.0
    # a non-finite fill is allowed
    for fill in (nan, inf, -inf):
        rc, msg = call(fill=fill)
        assert rc == 0, msg
    # the descent's loop guard (return code 3) is a backstop no scene reaches: a kd-tree that could trip it is refused where
    # it enters the module (test_gpu_streamlines.test_a_cyclic_kd_tree_never_reaches_the_descent)


def test_ms_is_zero_before_any_call():
    R = Case(scenes.example("ex3")).hip_renderer()
    assert R.flowmapMs() == (0.0, 0.0)
    R.close()
