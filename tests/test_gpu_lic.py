"""exa_hip_lic on the GPU (include/exa_hip.h): lic, sum, count, speed and reasons equal the numpy restatement of the contract
(tests/lic_ref.py) byte for byte — fed by the CPU oracle on small images, in both basis forms and with empty cells, and by
the point probes on larger ones —, in every lane layout (options lic_lanes, lic_patch), on image shapes that break a patch
map, at the shortest and the longest half length (the latter against the closed form of a uniform field), with the hash or
the same noise as an array, with host or device arrays; and nothing a frame sets changes a byte."""
import ctypes as C

import numpy as np
import pytest

import lic_ref as lr
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes

pytestmark = pytest.mark.gpu

PARAMS = [(i, f) for i, c in enumerate(lr.CASES) for f in c[3]]
IDS = [f"{lr.CASES[i][0]}-f{f}" for i, f in PARAMS]
LAYOUTS = [(1, 1), (1, 0), (2, 1), (2, 0)]                      # (lic_lanes, lic_patch); the first is the default

_cache = {}


def _setup(idx, form):
    if (idx, form) not in _cache:
        name, make, channels, _, empty, pl, step, L = lr.CASES[idx]
        case = Case(make(), basis_form=form, allow_empty_cells=empty, W=32, H=32)
        _cache[(idx, form)] = (case, case.hip_renderer())
    return _cache[(idx, form)]


def _amr3():
    """the renderer of the oblique case in form 1 (scenes.amr(levels=3, fields=4)) and its channels"""
    return _setup(1, 1)[1], lr.CASES[1][2]


def _layouts(R):
    for lanes, patch in LAYOUTS[1:] + LAYOUTS[:1]:              # ends on the default
        R.setOption("lic_lanes", lanes)
        R.setOption("lic_patch", patch)
        yield f"lanes {lanes} patch {patch}"


@pytest.mark.parametrize("idx,form", PARAMS, ids=IDS)
def test_equals_the_oracle_fed_restatement_byte_for_byte(idx, form):
    name, make, channels, _, empty, pl, step, L = lr.CASES[idx]
    case, R = _setup(idx, form)
    want = lr.lic(lr.oracle_evaluator(case.oracle_scene(), channels), pl, step, L, seed=idx)
    n = lr.reason_counts(want)
    print(name, form, n)
    from test_lic_ref import WANT
    for k, least in WANT[name].items():                         # the reference test's coverage, on what is compared here
        assert n[k] >= least, (name, k, n)
    for what in _layouts(R):
        lr.same(R.lic(pl, channels, step, L, seed=idx), want, (name, form, what))
    # a finite fill, and an infinite one, land in the pixels whose centre has no value
    for fill in (-7.5, np.inf):
        got = R.lic(pl, channels, step, L, seed=idx, fill=fill)
        empty_px = want["count"] == 0
        lr.same(got, dict(want, lic=np.where(empty_px, np.float32(fill), want["lic"]),
                          speed=np.where(empty_px, np.float32(fill), want["speed"])), (name, form, fill))


def test_larger_image_equals_the_probe_fed_restatement():
    R, channels = _amr3()
    pl = lr.plane((3.0, 1.0, 6.0), (0.6, 0.1, 0.05), (-0.1, 1.0, 0.35), (67, 45))
    want = lr.lic(lr.probe_evaluator(R, channels), pl, 0.5, 12, seed=9)
    n = lr.reason_counts(want)
    print(n)
    assert n[lr.END_MAXSTEPS] >= 1000 and n[lr.END_IMAGE] >= 100 and n[lr.END_LEFT] >= 10 and n["failed_centre"] >= 5
    for what in _layouts(R):
        lr.same(R.lic(pl, channels, 0.5, 12, seed=9), want, what)


@pytest.mark.parametrize("size", [(1, 1), (67, 1), (1, 5), (8, 8), (9, 7)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_that_break_a_patch_map(size):
    R, channels = _amr3()
    pl = lr.plane((20.0, 17.0, 13.0), (0.4, 0.05, 0.0), (0.0, 0.5, 0.3), size)
    for L in (1, 7):
        want = lr.lic(lr.probe_evaluator(R, channels), pl, 0.75, L, seed=3)
        assert want["count"].max() >= 2 or size[0] == 1         # a line mostly along u leaves a one-pixel-wide image at once
        for what in _layouts(R):
            lr.same(R.lic(pl, channels, 0.75, L, seed=3), want, (size, L, what))


def test_longest_half_length_equals_the_closed_form():
    case = Case(lr.uniform_scene(18), W=32, H=32)
    R = case.hip_renderer()
    nu, nv, L, step = 67, 3, binding.LIC_MAX_STEPS, 2.0 ** -6
    total, count, reasons = lr.uniform_closed_form(lr.hash_image(nu, nv, 0), step, L)
    assert (reasons == lr.END_MAXSTEPS).sum() == 18 and count.max() == 67 * 64
    for what in _layouts(R):
        got = R.lic(lr.uniform_plane(nu, nv), (1, 2, 3), step, L)
        assert np.array_equal(got["sum"], total) and np.array_equal(got["count"], count), what
        assert np.array_equal(got["reasons"], reasons), what
        assert np.array_equal(got["lic"].view(np.uint32), (total.astype(np.float32) / count.astype(np.float32)).view(np.uint32)), what
        assert np.all(got["speed"] == 1.0), what
    R.close()


def test_noise_array_equal_to_the_hash_gives_the_same_bytes():
    R, channels = _amr3()
    pl = lr.oblique_plane()
    want = R.lic(pl, channels, 0.5, 6, seed=11)
    lr.same(R.lic(pl, channels, 0.5, 6, noise=lr.hash_image(9, 7, 11)), want, "the hash as an array")
    other = R.lic(pl, channels, 0.5, 6, noise=lr.hash_image(9, 7, 12))
    assert not np.array_equal(other["sum"], want["sum"])
    assert np.array_equal(other["count"], want["count"]) and np.array_equal(other["reasons"], want["reasons"])
    lr.same(R.lic(pl, channels, 0.5, 6, noise=lr.hash_image(9, 7, 12)),
            lr.lic(lr.probe_evaluator(R, channels), pl, 0.5, 6, noise=lr.hash_image(9, 7, 12)), "an array against the restatement")


def _struct(pl):
    origin, du, dv, (nu, nv) = pl
    f3 = lambda v: (C.c_float * 3)(*[float(x) for x in v])      # noqa: E731
    return binding.ExaHipPlane(f3(origin), f3(du), f3(dv), nu, nv)


def test_host_and_device_pointers_two_calls_and_null_outputs():
    import torch
    R, channels = _amr3()
    L = binding.lib()
    pl = lr.plane((3.0, 1.0, 6.0), (0.6, 0.1, 0.05), (-0.1, 1.0, 0.35), (67, 45))
    nu, nv = pl[3]
    noise = lr.hash_image(nu, nv, 4) ^ np.uint8(0x5A)
    want = R.lic(pl, channels, 0.5, 8, noise=noise)
    lr.same(R.lic(pl, channels, 0.5, 8, noise=noise), want, "two calls")
    assert R.licMs() > 0.0
    dev = torch.device("cuda:0")
    dtypes = dict(lic=torch.float32, sum=torch.int32, count=torch.int32, speed=torch.float32, reasons=torch.int32)
    fresh = lambda: {k: torch.full((nv, nu, 2) if k == "reasons" else (nv, nu), 77, dtype=t, device=dev) for k, t in dtypes.items()}   # noqa: E731
    dnoise = torch.from_numpy(noise).to(dev)
    s, ch = _struct(pl), (C.c_int32 * 3)(*channels)

    def call(out, keys, device=1, noise_ptr=None):
        ptr = lambda k: (C.c_void_p(out[k].data_ptr()) if device else out[k].ctypes.data) if k in keys else None     # noqa: E731
        rc = L.exa_hip_lic(R.h, C.byref(s), ch, 0.5, 8, noise_ptr, 0, 0, float("nan"), ptr("lic"), ptr("sum"), ptr("count"),
                           ptr("speed"), ptr("reasons"), device, None)
        assert rc == 0, L.exa_hip_last_error(R.h).decode()

    out = fresh()
    call(out, lr.KEYS, noise_ptr=C.c_void_p(dnoise.data_ptr()))
    torch.cuda.synchronize()
    lr.same({k: out[k].cpu().numpy().view(want[k].dtype) for k in lr.KEYS}, want, "device pointers")
    # NULL outputs are skipped: on the device ...
    out = fresh()
    call(out, ("count", "speed"), noise_ptr=C.c_void_p(dnoise.data_ptr()))
    torch.cuda.synchronize()
    for k in lr.KEYS:
        got = out[k].cpu().numpy().view(want[k].dtype)
        assert np.array_equal(got.view(np.uint32), want[k].view(np.uint32)) == (k in ("count", "speed")), k
        assert k in ("count", "speed") or bool((out[k] == 77).all()), k
    # ... and on the host; and all five
    host = {k: np.full(want[k].shape, 77, want[k].dtype) for k in lr.KEYS}
    call(host, ("lic", "reasons"), device=0, noise_ptr=noise.ctypes.data)
    for k in lr.KEYS:
        assert np.array_equal(host[k].view(np.uint32), want[k].view(np.uint32)) == (k in ("lic", "reasons")), k
    call(host, (), device=0)


def test_bytes_do_not_depend_on_the_frame_state_or_options():
    case = Case(scenes.amr(levels=3, fields=4), W=32, H=32)
    R = case.hip_renderer()
    pl, channels = lr.oblique_plane(), (1, 3, 0)
    want = R.lic(pl, channels, 0.5, 6, seed=1)
    lr.same(want, _amr3()[0].lic(pl, channels, 0.5, 6, seed=1), "another handle")
    for what in frame_perturbations(case, R):
        lr.same(R.lic(pl, channels, 0.5, 6, seed=1), want, what)
    R.close()


def test_multi_device_handle_equals_single():
    R, channels = _amr3()
    pl = lr.oblique_plane()
    M = multi_handle(R, 1)
    lr.same(M.lic(pl, channels, 0.5, 6, seed=1), R.lic(pl, channels, 0.5, 6, seed=1), "multi")
    assert M.licMs() > 0.0
    M.close()


def test_scene_without_kd_tree_is_refused():
    R = binding.Renderer(without_kd_tree(binding.Prep(scenes.amr(levels=3, fields=3))))
    with pytest.raises(RuntimeError, match="exa_hip_lic: .*kd-tree"):
        R.lic(lr.oblique_plane())
    assert R.licMs() == 0.0
    R.close()


def test_bad_arguments_are_refused_and_the_handle_stays_usable():
    R, channels = _amr3()
    L = binding.lib()
    pl = lr.oblique_plane()
    want = R.lic(pl, channels, 0.5, 6, seed=2)
    buf = {k: np.zeros(want[k].shape, want[k].dtype) for k in lr.KEYS}
    good = (C.c_int32 * 3)(*channels)

    def call(plane=pl, ch=good, step=0.5, half_length=6, flags=0, null_plane=False):
        s = _struct(plane)
        rc = L.exa_hip_lic(R.h, None if null_plane else C.byref(s), ch, step, half_length, None, 2, flags, float("nan"),
                           *[buf[k].ctypes.data for k in lr.KEYS], 0, None)
        return rc, L.exa_hip_last_error(R.h).decode()

    def edited(**kw):
        origin, du, dv, size = pl
        return dict(plane=(kw.get("origin", origin), kw.get("du", du), kw.get("dv", dv), kw.get("size", size)))

    nan, inf = float("nan"), float("inf")
    bad = [(dict(null_plane=True), "null"), (dict(ch=None), "null"),
           (edited(origin=(nan, 0, 0)), "finite"), (edited(du=(1, inf, 0)), "finite"), (edited(dv=(0, 0, -inf)), "finite"),
           (edited(du=(1, 2, 3), dv=(2, 4, 6)), "span"), (edited(du=(0, 0, 0)), "span"), (edited(du=(1e30, 0, 0), dv=(0, 1e30, 0)), "span"),
           (edited(size=(0, 7)), "nu and nv"), (edited(size=(9, -1)), "nu and nv"), (edited(size=(65536, 32768)), "2^31"),
           (dict(ch=(C.c_int32 * 3)(0, 1, 4)), "channel"), (dict(ch=(C.c_int32 * 3)(-1, 1, 2)), "channel"),
           (dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=nan), "step"), (dict(step=inf), "step"),
           (dict(half_length=0), "halfLength"), (dict(half_length=binding.LIC_MAX_STEPS + 1), "halfLength"),
           (dict(flags=1), "flag"), (dict(flags=1 << 30), "flag")]
    for kw, match in bad:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("exa_hip_lic: ") and match in msg, (kw, rc, msg)
        assert R.licMs() == 0.0
        rc, msg = call()                                            # ... and the handle still computes
        assert rc == 0, msg
        lr.same(buf, want, kw)
        assert R.licMs() > 0.0
    # the descent's loop guard (return code 3) is a backstop no scene reaches: a kd-tree that could trip it is refused where
    # it enters the module (test_gpu_streamlines.test_a_cyclic_kd_tree_never_reaches_the_descent)


def test_ms_is_zero_before_any_call():
    R = Case(scenes.example("ex3")).hip_renderer()
    assert R.licMs() == 0.0
    R.close()
