"""NaN cell scalars on the frame path and in the probes, against the CPU oracle ("Input domain": cell scalars
are finite or NaN, and a NaN cell poisons the samples that read it exactly as in the reference).

The scenes, the marker transfer function (entry 0, where a NaN sample lands, is opaque magenta) and the variants are those of
tests/nan_scenes.py; tests/test_nan_cells.py holds, on the CPU, that every one of them exercises what it is here for.  No
oracle frame of these scenes has a NaN pixel, so compare() of tests/common.py applies as it stands: a NaN pixel of the module
is an infinite ulp distance and fails every bound.

Bounds: MAX_ULP_TIGHT, MAX_ULP_SHIPPED, ULP_P999_SHIPPED, ACCUM_ATOL / ACCUM_RTOL, FLIP_BOUND and AO_FLIP_BOUND are those of
tests/common.py, unchanged; the AO rule is _check_ao's of tests/test_gpu_parity.py with nothing observed (at most 2 pixels);
K_VALUE / K_NUM are those of tests/probe_ref64.py.  The share of bit-identical pixels is held to half of the clean twin's,
measured in the same test against the oracle, not to a recorded figure."""
import numpy as np
import pytest

import nan_scenes as ns
import probe_ref64 as r64
import probe_sets as ps
from common import (ACCUM_ATOL, ACCUM_RTOL, AO_FLIP_BOUND, FLIP_BOUND, MAX_ULP_SHIPPED, MAX_ULP_TIGHT, ULP_P999_SHIPPED, compare,
                    error_profile_line)
from test_gpu_multi import MultiCase
from test_gpu_parity import STAT_KEYS
from test_gpu_sample_ref64 import _check_normalized, _check_status

pytestmark = pytest.mark.gpu

ACCELS = [1, 0, 2]
ACCEL_IDS = ["kd", "lbvh", "rope"]
FORMS = [0, 1]
FORM_IDS = ["source_order", "per_axis"]
FILL = np.float32(-12345.5)
GRID = (16, 12, 10)

FRAMES = [(n, v) for n in ns.SCENES for v in ns.variants_of(n)]
NO_AO = [(n, v) for n, v in FRAMES if not ns.VARIANTS[v].get("ao")]

_oracle, _hip = {}, {}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_frame(name, variant, form, clean=False):
    """the oracle's frame, its activity arrays and its empty-range regions (computed once, shared, never changed)"""
    key = (name, variant, form, clean)
    if key not in _oracle:
        case = ns.named_case(name, variant, clean=clean, basis_form=form)
        S = case.oracle_scene()
        fs, P = case.oracle_state(S)
        rgba, acc, st = S.render(fs, P, case.W, case.H, nthreads=8)
        _oracle[key] = dict(out=(rgba, acc, st), vol=S.volume_active(fs, P), iso=S.iso_active(fs),
                            empty=ns.empty_range_regions(S.regions()))
        S.close()
    return _oracle[key]


def render(case, stats=True):
    """one frame of the case through the C ABI: (rgba, accum, counters or None), and the two activity arrays"""
    R = case.hip_renderer()
    try:
        R.updateFrameID(case.frameID)
        rgba, st = R.renderStats() if stats else (R.render(), None)
        return dict(out=(np.array(rgba, copy=True), R.readAccum().copy(), st), vol=R.readActivity(0), iso=R.readActivity(1))
    finally:
        R.close()


def hip_frame(name, variant, accel, form, clean=False, fast_math=0):
    """the counting variant's frame (computed once per key, shared, never changed)"""
    key = (name, variant, accel, form, clean, fast_math)
    if key not in _hip:
        _hip[key] = render(ns.named_case(name, variant, clean=clean, basis_form=form, accel=accel, fast_math=fast_math))
    return _hip[key]


def same_frame(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(_bits(a[1]), _bits(b[1]))


def check_ao(o, h, what):
    """_check_ao of tests/test_gpu_parity.py, kind "tight", for a case with no recorded observation: at most 2 pixels beyond
    ACCUM_ATOL, none by more than one AO flip and one termination flip, the work within 1 % + 64"""
    da = np.abs(o[1].astype(np.float64) - h[1].astype(np.float64)).max(axis=-1)
    n = int((da > ACCUM_ATOL).sum())
    print(f"PROFILE {what} AO tight: {n} of {da.size} pixels beyond {ACCUM_ATOL:g}, max |d accum| {da.max():.3g}")
    assert not np.isnan(da).any(), what
    assert n <= max(2, 0.003 * da.size) and n <= 2, (what, n)
    assert da.max() <= AO_FLIP_BOUND + FLIP_BOUND, (what, float(da.max()))
    loose = [(k, o[2][k], h[2][k]) for k in STAT_KEYS if abs(o[2][k] - h[2][k]) > 0.01 * o[2][k] + 64]
    assert not loose, (what, loose)


# ---- a. frames equal the oracle ----
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name,variant", FRAMES, ids=[f"{n}-{v}" for n, v in FRAMES])
def test_frames_of_nan_scenes_equal_the_oracle(name, variant, accel, form):
    """test_hip_matches_oracle on the NaN scenes (fast_math 0: the work counters match sample for sample), and with it: no NaN
    in the accumulation buffer, both activity arrays equal the bounds programs', and with skipping on exactly the regions
    of empty range are switched off beyond those the TF leaves transparent"""
    ref, got = oracle_frame(name, variant, form), hip_frame(name, variant, accel, form)
    o, h = ref["out"], got["out"]
    what = f"nan {name} {variant} {accel} {form} fast_math 0"
    assert not np.isnan(o[1]).any(), "the oracle's frame (tests/test_nan_cells.py holds this on the CPU)"
    assert not np.isnan(h[1]).any(), (what, int(np.isnan(h[1]).any(axis=-1).sum()), "NaN pixels")
    assert np.array_equal(got["vol"], ref["vol"]) and np.array_equal(got["iso"], ref["iso"]), what
    case = ns.named_case(name, variant)
    if case.space_skipping:
        # the marker TF is opaque at entry 0 and the ramp above it: no region with a value is transparent
        assert np.array_equal(got["vol"] == 0, ref["empty"]), what
        assert int((got["vol"] == 0).sum()) == int(ref["empty"].sum())
    else:
        assert got["vol"].all()
    assert not got["iso"][ref["empty"]].any()
    r = compare(o, h, what)
    if case.ao:
        check_ao(o, h, what)
        return
    print(error_profile_line(r))
    assert r["accum_bad"] == 0 and r["rgba_bad"] == 0, r
    assert r["max_ulp"] <= MAX_ULP_TIGHT, r
    assert {k: o[2][k] for k in STAT_KEYS} == {k: h[2][k] for k in STAT_KEYS}, what     # identical work, sample for sample
    assert h[2]["diag"][8] == 0


# ---- b. shipped defaults ----
SHIPPED = [(n, v) for n in ns.SPARSE + ns.BLOCK + ns.BORDER for v in ns.variants_of(n) if v not in ("dvr", "iso_ao")]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name,variant", SHIPPED, ids=[f"{n}-{v}" for n, v in SHIPPED])
def test_shipped_defaults_on_nan_scenes_within_stated_tolerance(name, variant, accel, form):
    """test_shipped_defaults_within_stated_tolerance (fast_math unset: the hardware exp2 / log2 / rcp / rsqrt paths see the
    NaN samples) on the sparse, block and brick-border scenes"""
    o = oracle_frame(name, variant, form)["out"]
    h = render(ns.named_case(name, variant, basis_form=form, accel=accel))["out"]
    r = compare(o, h, f"nan {name} {variant} {accel} {form} defaults")
    print(error_profile_line(r))
    assert not np.isnan(h[1]).any()
    assert r["flips_ok"] and r["rgba_bad"] <= 3 * r["flip_pixels"], r
    assert r["max_ulp"] <= MAX_ULP_SHIPPED and r["ulp_p999"] <= ULP_P999_SHIPPED, r
    for k in ("samples", "brick_visits", "segments"):
        assert abs(o[2][k] - h[2][k]) <= 1e-3 * o[2][k] + 2, (k, o[2][k], h[2][k])


# ---- c. bit-identical pixels ----
EXACT = [(n, v) for n, v in NO_AO if v in ("grad", "iso", "faint_skip", "faint_noskip")]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name,variant", EXACT, ids=[f"{n}-{v}" for n, v in EXACT])
def test_nan_cells_cost_no_bit_identical_pixels(name, variant, accel, form):
    """the kernels and the oracle execute one operation sequence, so most pixels are bit-identical; the poisoned scene must
    keep at least half the share its clean twin reaches — same camera, TF and options, both against the oracle"""
    r = {}
    for clean in (False, True):
        o, h = oracle_frame(name, variant, form, clean)["out"], hip_frame(name, variant, accel, form, clean)["out"]
        r[clean] = compare(o, h, f"nan {name} {variant} {accel} {form} {'clean twin' if clean else 'poisoned'}")
        print(error_profile_line(r[clean]))
    assert r[True]["accum_bad"] == 0 and r[True]["max_ulp"] <= MAX_ULP_TIGHT, r[True]
    assert r[False]["exact_px"] >= 0.5 * r[True]["exact_px"], (r[False]["exact_px"], r[True]["exact_px"])


# ---- d. shipped kernel == counting variant ----
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("fast_math", [0, 1])
@pytest.mark.parametrize("accel", [None, 1], ids=["default_walk", "kd"])
@pytest.mark.parametrize("name", sorted(ns.SCENES))
def test_shipped_kernel_equals_counting_variant_on_nan_scenes(name, accel, fast_math, form):
    """the frames above come from the counting variant; the kernel a caller gets — on the cube records where the scene and
    the walk allow them (amr3 with one channel on the rope walk, the default walk of these dense scenes) — produces the
    same accumulation buffer bit for bit"""
    for variant in ["iso"] + (["faint_skip"] if name in ns.BLOCK else []):
        case = ns.named_case(name, variant, basis_form=form, accel=accel, fast_math=fast_math)
        plain, counted = render(case, stats=False)["out"], render(case, stats=True)["out"]
        assert same_frame(plain, counted), (name, variant)
        assert not np.isnan(plain[1]).any()


# ---- e. nothing about the records or the launch changes a pixel ----
OPTIONS = [("pack_records", 0, 1), ("pack_records", 0, 2), ("interleave", 0, 1), ("brick_order", 1, 1), ("brick_order", 1, 2),
           ("prepass_split", 0, 1), ("prepass_split", 1, 1), ("ao_overlap", 1, 1), ("ao_overlap", 1, 2), ("lbvh_build", 1, 0),
           ("cube_records", 0, 2)]


@pytest.mark.parametrize("key,value,accel", OPTIONS, ids=[f"{k}{v}-{ACCEL_IDS[ACCELS.index(a)]}" for k, v, a in OPTIONS])
@pytest.mark.parametrize("name", ns.SPARSE + ns.BORDER + ["amr3_2f_ch0_multi"])
def test_records_and_launch_options_change_no_pixel_of_a_nan_scene(name, key, value, accel):
    """DVR with gradient shading, the iso pre-pass and AO rays in one frame (the shipped kernels, defaults otherwise), two
    accumulated frames: the option set to the other value gives the same RGBA8 frame and accumulation buffer bit for bit"""
    out = []
    for options in ({}, {key: value}):
        case = ns.named_case(name, "iso_ao", grad=1, accel=accel)
        case.options = options
        out.append(case.run_hip(frames=2))
    assert same_frame(out[0], out[1]), (name, key, value)
    assert not np.isnan(out[0][1]).any() and (out[0][1][..., :3] > 0).any()


@pytest.mark.parametrize("name", ns.SPARSE + ns.BORDER)
def test_two_shards_of_a_nan_scene_join_to_the_frame(name):
    """one handle over two device entries (tests/test_gpu_multi.py): interleaved tiles, joined in the first device's frame"""
    one = ns.named_case(name, "iso_ao", grad=1).run_hip(frames=2, stats=True)
    mc = ns.named_case(name, "iso_ao", grad=1, cls=MultiCase)
    mc.devices = [0, 0]
    two = mc.run_hip(frames=2, stats=True)
    assert same_frame(one, two)
    assert {k: one[2][k] for k in STAT_KEYS} == {k: two[2][k] for k in STAT_KEYS}


# ---- f. the skipping asymmetry is the oracle's ----
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("accel", ACCELS, ids=ACCEL_IDS)
@pytest.mark.parametrize("name", ns.BLOCK)
def test_skipping_changes_the_same_pixels_as_in_the_oracle(name, accel, form):
    """a region all of whose cells are NaN has the empty range and is never sampled with skipping on; with skipping off its
    samples take TF entry 0.  Skipping is therefore not neutral on such a scene, in the reference as here: the pixels that
    differ between the two settings (beyond ACCUM_ATOL + ACCUM_RTOL |accum|) are the same set on both sides"""
    def differs(on, off):
        d = np.abs(on.astype(np.float64) - off.astype(np.float64))
        return (d > ACCUM_ATOL + ACCUM_RTOL * np.abs(on)).any(axis=-1)
    want = differs(oracle_frame(name, "faint_skip", form)["out"][1], oracle_frame(name, "faint_noskip", form)["out"][1])
    got = differs(hip_frame(name, "faint_skip", accel, form)["out"][1], hip_frame(name, "faint_noskip", accel, form)["out"][1])
    print(f"{name} {accel} {form}: skipping on / off differ in {int(want.sum())} pixels (oracle), {int(got.sum())} (module)")
    assert want.sum() >= 800, "tests/test_nan_cells.py holds this on the CPU"
    assert np.array_equal(got, want), int((got != want).sum())


# ---- g. border versus interior: the clamped read with weight 0 ----
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("accel", [1, 2], ids=["kd", "rope"])
@pytest.mark.parametrize("name", ns.BORDER + ns.INTERIOR)
def test_masked_weight_sampler_equals_the_literal_sampler_on_nan_scenes(name, accel, form):
    """the iso pre-pass of the kd kernels samples through the masked-weight basis (option fast_sampler, default 1): indices
    clamped into the brick, the cells outside read with weight 0 — and 0 * NaN is NaN.  fast_sampler 0 is the literal
    addBasisFunctions, which does not read them.  With fast_math 0 the two frames are the same bit for bit (the shipped
    kernels: the counting variant always takes the literal form)"""
    for variant in ("iso", "iso_ao"):
        out = []
        for fast_sampler in (1, 0):
            case = ns.named_case(name, variant, basis_form=form, accel=accel, fast_math=0)
            case.options = {"fast_sampler": fast_sampler}
            out.append(render(case, stats=False)["out"])
        assert same_frame(out[0], out[1]), (name, variant, int((_bits(out[0][1]) != _bits(out[1][1])).any(axis=-1).sum()))
        assert not np.isnan(out[0][1]).any()


# ---- h. point probes ----
@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", ns.SPARSE + ns.BORDER)
def test_probes_carry_nan_as_a_value(name, form):
    """samplePoints (value, numerator, normalized gradient) and resample against the oracle's samplePoint: the status rule of
    tests/test_gpu_sample_ref64.py — a NaN value is a value: the status stays the region and the entry is not the fill —,
    the same NaN entries, the same bits everywhere else; and against the float64 reconstruction, K_VALUE / K_NUM and the
    normalized bound on the entries that are not NaN"""
    idx = 2 if name.startswith("amr3") else 0                     # the seeds of ps.REF_CASES' amr3 and ex3
    case = ns.named_case(name, "grad", basis_form=form)
    R, S = case.hip_renderer(), case.oracle_scene()
    try:
        pts = ps.ref_points(R.prep, idx)
        owner = ps.brute_owner(R.prep, pts)
        recon = r64.Reconstruction(case.scene, R.prep.regions(), R.prep.bricks(), R.prep.leaflist())
        ref = recon.evaluate(pts, owner, (0,))
        v, g, st = R.samplePoints(pts, channels=(0,), gradient=True, fill=FILL)
        vn, gn, stn = R.samplePoints(pts, channels=(0,), gradient=True, normalized=True, fill=FILL)
        has = _check_status(st, owner, ref)
        assert np.array_equal(stn, st) and np.array_equal(np.isnan(vn), np.isnan(v))
        assert np.array_equal(_bits(vn)[~np.isnan(v)], _bits(v)[~np.isnan(v)])
        assert np.all(_bits(v[~has]) == _bits(FILL)) and np.all(_bits(g[~has]) == _bits(FILL)) and np.all(_bits(gn[~has]) == _bits(FILL))
        assert not (_bits(v[has]) == _bits(FILL)).any()
        ov, og = np.full(v.shape, FILL), np.full(g.shape, FILL)
        for i in np.nonzero(has[:, 0])[0]:
            ok, ov[i, 0], og[i, 0] = S.sample_point(int(st[i, 0]), pts[i], 0, True)
            assert ok, (i, pts[i])
        nan = np.isnan(ov)
        print(f"{name} form {form}: {int(has.sum())} probes with a value, {int(nan.sum())} of them NaN")
        assert nan.sum() >= 20 and (has & ~nan).sum() >= 200
        assert np.array_equal(np.isnan(v), nan) and np.array_equal(np.isnan(g), np.isnan(og))
        assert np.array_equal(np.isnan(og).all(axis=-1), nan) and np.array_equal(np.isnan(og).any(axis=-1), nan)
        assert np.array_equal(np.isnan(gn).any(axis=-1), nan)
        assert np.array_equal(_bits(v)[~nan], _bits(ov)[~nan]) and np.array_equal(_bits(g)[~np.isnan(og)], _bits(og)[~np.isnan(og)])
        # the float64 reference reads the same cells except where float32 rounds the position across a cell-centre plane
        nan64 = np.isnan(ref["value"])
        assert (nan64 != nan)[has].mean() <= 0.01
        fin = has & ~nan & ~nan64
        kv, kg = r64.scaled_errors(ref, v, g)
        for stratum in ("covered", "all"):
            m = fin & r64.stratum(ref, stratum)
            print(f"K nan {name} form {form} {stratum}: n {int(m.sum())} K_value {kv[m].max():.4g} K_num {kg[m].max():.4g}")
            assert kv[m].max() <= r64.K_VALUE[stratum][form] and kg[m].max() <= r64.K_NUM[stratum][form], stratum
        _check_normalized(gn, ref, fin, form, f"nan {name} form {form}")
        # the lattice of exa_hip_resample
        lo, hi = ps.root_box(R.prep, grow=0.1)
        V = R.resample(lo, hi, GRID, channel=0, fill=FILL).reshape(-1)
        pos = ps.grid_positions(lo, hi, GRID)
        gown = ps.brute_owner(R.prep, pos)
        want = np.full(len(pos), FILL)
        for i in np.nonzero(gown >= 0)[0]:
            ok, val, _ = S.sample_point(int(gown[i]), pos[i], 0, False)
            if ok:
                want[i] = val
        assert np.array_equal(np.isnan(V), np.isnan(want)) and np.array_equal(_bits(V)[~np.isnan(want)], _bits(want)[~np.isnan(want)])
        if name.startswith("amr3"):
            assert np.isnan(want).sum() >= 5
    finally:
        R.close()
        S.close()


# ---- i. the integrators take a NaN velocity as the contract says ----
_flow = {}


def flow(form):
    """the renderer and the oracle scene of ns.flow_scene() in one basis form (made once)"""
    if form not in _flow:
        case = ns.case(ns.flow_scene(), basis_form=form, W=32, H=32)
        _flow[form] = (case.hip_renderer(), case.oracle_scene())
    return _flow[form]


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_streamlines_through_nan_velocities_equal_the_restatement(form):
    """a NaN velocity is a value: without EXA_STREAM_NORMALIZE the next position is NaN and its lookup ends the direction LEFT,
    with the flag !(s > 0) ends it STAGNANT (include/exa_hip.h); tests/streamline_ref.py, bit for bit"""
    import streamline_ref as sr
    from test_gpu_streamlines import _same
    R, S = flow(form)
    seeds = sr.uniform_seeds(S, ns.FLOW_SEEDS)
    for fw, bw, nm in ((True, False, False), (True, True, False), (True, False, True)):
        want = sr.streamlines(S, seeds, ns.FLOW_CHANNELS, ns.FLOW_STEP, ns.FLOW_MAX_STEPS, fw, bw, nm)
        got = R.streamlines(seeds, ns.FLOW_CHANNELS, ns.FLOW_STEP, ns.FLOW_MAX_STEPS, forward=fw, backward=bw, normalize=nm,
                            velocities=True)
        _same(got, want, ("nan flow", form, fw, bw, nm))
        assert not np.isnan(got[0]).any()                             # no NaN position is ever appended
    for nm in (False, True):
        ended = ns.directions_ended_by_nan(S, seeds, ns.FLOW_STEP, ns.FLOW_MAX_STEPS, nm)
        print(f"form {form} normalize {nm}: {int(ended.sum())} of {len(seeds)} forward lines end for a NaN velocity")
        assert ended.sum() >= 5


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_lic_through_nan_velocities_equals_the_restatement(form):
    import lic_ref as lr
    R, S = flow(form)
    pl = lr.plane(*ns.FLOW_PLANE)
    evaluate = ns.counting_evaluator(lr.oracle_evaluator(S, ns.FLOW_CHANNELS))
    want = lr.lic(evaluate, pl, ns.FLOW_LIC_STEP, ns.FLOW_LIC_HALF_LENGTH, seed=4)
    print(f"form {form}: {evaluate.nan} evaluations with a NaN velocity, each the end of its direction; {lr.reason_counts(want)}")
    assert evaluate.nan >= 5 and not np.isnan(want["lic"][want["count"] > 0]).any()
    lr.same(R.lic(pl, ns.FLOW_CHANNELS, ns.FLOW_LIC_STEP, ns.FLOW_LIC_HALF_LENGTH, seed=4), want, ("nan flow", form))


@pytest.mark.parametrize("form", FORMS, ids=FORM_IDS)
def test_flowmap_through_nan_velocities_equals_the_restatement(form):
    import flowmap_ref as fr
    R, S = flow(form)
    lo, hi = ns.FLOW_BOX
    for backward in (False, True):
        want = fr.flowmap(fr.oracle_feed(S, ns.FLOW_CHANNELS), lo, hi, ns.FLOW_DIMS, ns.FLOW_STEP, ns.FLOW_NUM_STEPS, backward)
        hs = -ns.FLOW_STEP if backward else ns.FLOW_STEP
        ended = ns.directions_ended_by_nan(S, fr.positions(lo, hi, ns.FLOW_DIMS), hs, ns.FLOW_NUM_STEPS)
        print(f"form {form} backward {backward}: {int(ended.sum())} of {ended.size} points end for a NaN velocity; {fr.coverage(want)}")
        assert ended.sum() >= 5 and not np.isnan(want["end"]).any()
        fr.same(R.flowmap(lo, hi, ns.FLOW_DIMS, ns.FLOW_CHANNELS, ns.FLOW_STEP, ns.FLOW_NUM_STEPS, backward), want,
                ("nan flow", form, backward))
