"""Translated scenes on the GPU: negative coordinates, scenes that straddle the origin, and coordinates that are large against
the cell width (probe_sets.TRANSLATIONS of the amr3 scene).  Where the positions are float32 in both frames of reference
every call that reads the field outside a frame returns the same bits as on the untranslated scene (point probes, derived
quantities, lattices, axis-aligned projections, histograms, the triangles of an iso-surface); in its own frame of reference
each call equals its restatement or stays within the existing bounds against the float64 reference (probes, pinhole
projections, meshes, streamlines), and a frame meets the oracle with the tolerances of tests/test_gpu_parity.py on all three
walks, among them cameras at the origin (the rope walk's |o| == 0 arm), at a tiny non-zero origin (its fallback to the
plain division) and in a region face at coordinate 0.  tests/test_translation_ref.py holds the CPU side of all this."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import histogram_ref as hr
import isomesh_ref
import probe_sets as ps
import project_ref as pr
import streamline_ref as sr
import test_gpu_isomesh as tgi
import test_gpu_project as tgp
import test_gpu_sample_ref64 as g64
import test_gpu_streamlines as tgs
from analysis_steps import bits as _bits, multi_handle
from common import MAX_ULP_TIGHT, ROOT, Case, band_xf, compare, error_profile_line
from owlexabrick_amd import binding, scenes
from test_gpu_parity import STAT_KEYS

pytestmark = pytest.mark.gpu

f32 = np.float32
FILL = f32(-12345.5)
NAN = float("nan")
NAMES = [n for n, _ in ps.TRANSLATIONS]
# a lattice whose positions are float32 in every frame: integer corners, power-of-two dims, cells of 1.75 and 1.25 voxels
LAT_LO, LAT_HI, LAT_DIMS = np.array([-4, -4, -4], f32), np.array([52, 52, 36], f32), (32, 32, 32)
EXE = os.path.join(ROOT, "owlexabrick_amd", "host", "exaRender")


def amr3(holes=False):
    sc = scenes.amr(levels=3, fields=3)
    return scenes.with_empty_cells(sc, fraction=0.15) if holes else sc


_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_renderers():
    yield
    for _, R in _cache.values():
        R.close()
    _cache.clear()


def setup(name, form, holes=False):
    """(case, renderer) of amr3 translated by TRANSLATIONS[name] (None: where it is), made once per frame of reference and
    form and shared; no test changes a shared renderer's options"""
    key = (name, form, holes)
    if key not in _cache:
        scene = amr3(holes)
        if name is not None:
            scene = ps.translated(scene, ps.TRANSLATION[name])
        case = Case(scene, basis_form=form, allow_empty_cells=holes, W=32, H=32)
        _cache[key] = (case, case.hip_renderer())
    return _cache[key]


FORMS = [(0, False), (1, False), (0, True)]
FORM_IDS = ["f0", "f1", "holes-f0"]


def lattice(t):
    """the lattice of LAT_* moved by t, after asserting in float64 that each of its float32 positions is exact"""
    t64 = np.asarray(t, dtype=np.float64)
    lo, hi = (LAT_LO.astype(np.float64) + t64).astype(f32), (LAT_HI.astype(np.float64) + t64).astype(f32)
    assert np.array_equal(lo.astype(np.float64), LAT_LO + t64) and np.array_equal(hi.astype(np.float64), LAT_HI + t64)
    axes = [LAT_LO[k] + t64[k] + (np.arange(LAT_DIMS[k]) + 0.5) * (float(LAT_HI[k] - LAT_LO[k]) / LAT_DIMS[k]) for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    want = np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1)
    assert np.array_equal(ps.grid_positions(lo, hi, LAT_DIMS).astype(np.float64), want), "a lattice position rounds"
    return lo, hi


# ---- a. point probes, exact ----
@pytest.mark.parametrize("form,holes", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("name", NAMES)
def test_probes_keep_every_bit(name, form, holes):
    t = ps.TRANSLATION[name]
    _, RA = setup(None, form, holes)
    _, RB = setup(name, form, holes)
    pts = ps.dyadic_points(RA.prep, t)
    assert len(pts) <= 5000
    q = ps.moved(pts, t)
    chans = (0, 1, 2)
    a = RA.samplePoints(pts, channels=chans, gradient=True, fill=FILL)
    b = RB.samplePoints(q, channels=chans, gradient=True, fill=FILL)
    assert np.array_equal(a[2], b[2]) and (a[2] >= 0).sum() > 1000 and (a[2] < 0).sum() > 0
    if holes:
        assert (a[2] == -2).sum() > 0
    assert np.array_equal(_bits(a[0]), _bits(b[0]))
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    an = RA.samplePoints(pts, channels=chans, gradient=True, normalized=True, fill=FILL)
    bn = RB.samplePoints(q, channels=chans, gradient=True, normalized=True, fill=FILL)
    assert np.array_equal(an[2], a[2]) and np.array_equal(bn[2], a[2])
    assert np.array_equal(_bits(an[1]), _bits(bn[1]))                 # translation does not rescale
    assert np.abs(an[1][an[2] >= 0]).max() > 1e-3
    for quantity in binding.DERIVED:
        da, sa = RA.sampleDerived(pts, quantity, channels=chans, fill=FILL)
        db, sb = RB.sampleDerived(q, quantity, channels=chans, fill=FILL)
        assert np.array_equal(sa, sb) and (sa >= 0).sum() > 1000, quantity
        assert np.array_equal(_bits(da), _bits(db)), quantity
    lo, hi = lattice(t)
    VA = RA.resample(LAT_LO, LAT_HI, LAT_DIMS, channel=1, fill=FILL)
    VB = RB.resample(lo, hi, LAT_DIMS, channel=1, fill=FILL)
    assert np.array_equal(_bits(VA), _bits(VB))
    assert (_bits(VA) != _bits(FILL)).sum() > 10000 and (_bits(VA) == _bits(FILL)).sum() > 100


# ---- b. point probes against float64 ----
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["straddle", "negative", "far"])
def test_probe_against_the_float64_reference_in_the_translated_frame(name, form):
    case = Case(ps.translated(amr3(), ps.TRANSLATION[name]), basis_form=form)
    g64.check_probe_against_the_float64_reference(case, f"amr3 {name}", form, 2)


# ---- c. projections ----
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["straddle", "odd", "negative", "moderate"])
def test_axis_aligned_projections_keep_every_bit(name, form):
    t = ps.TRANSLATION[name]
    _, RA = setup(None, form)
    _, RB = setup(name, form)
    for axis in range(3):
        ra, rb = ps.axis_rays(RA.prep, t, axis)
        a, b = RA.project(**ra, channel=1), RB.project(**rb, channel=1)
        for k in tgp.KEYS:
            assert pr.same_bits(a[k], b[k]), (axis, k)
        # every ray crosses the scene, 32 voxels deep at the least, at two samples a voxel: 48 valid samples a ray leave room
        # for the half cells at both ends where the weights vanish
        assert int(a["count"].sum()) >= 24 * 16 * 48 and (a["max_index"] >= 0).all()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["straddle", "far"])
def test_pinhole_projection_equals_the_point_probe_reduced(name, form):
    _, R = setup(name, form)
    for normalize in (False, True):
        rays = tgp.pinhole_rays(R.prep, normalize)
        ref, values, status = tgp.check(R, rays, normalize, channel=1, what=(name, form, normalize))
        assert (status >= 0).sum() >= 2000 and (ref["count"] == 0).sum() >= 20


# ---- d. histogram ----
@pytest.mark.parametrize("holes", [False, True], ids=["amr3", "holes"])
@pytest.mark.parametrize("name", NAMES)
def test_histogram_keeps_every_count(name, holes):
    t = np.array(ps.TRANSLATION[name])
    _, RA = setup(None, 0, holes)
    case, RB = setup(name, 0, holes)
    S = hr.Slots(case.scene, holes)
    for channel in (0, 2):
        whole = RA.fieldStats(channel)
        assert hr.same_stats(whole, RB.fieldStats(channel)) and hr.same_stats(whole, S.histogram(channel, 0, 0, 0)[2])
        assert whole["slots"] == 23552 and (whole["empty"] > 0) == holes and (whole["levelCells"] > 0).sum() == 3
        for box in ps.translated_boxes(t):
            box_a = None if box is None else [int(x) for x in np.asarray(box) - np.concatenate([t, t])]
            a = RA.histogram(channel, whole["min"], whole["max"], 128, box=box_a)
            b = RB.histogram(channel, whole["min"], whole["max"], 128, box=box)
            want = S.histogram(channel, whole["min"], whole["max"], 128, box=box)
            for got in (a, b):
                assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (channel, box)
                assert hr.same_stats(got[2], want[2]), (channel, box, got[2], want[2])
            assert hr.same_stats(RB.fieldStats(channel, box=box), S.histogram(channel, 0, 0, 0, box=box)[2])
    if name == "straddle":
        slots = [S.histogram(0, 0, 0, 0, box=box)[2]["slots"] for box in ps.translated_boxes(t)]
        assert 0 < slots[1] < 23552 and 0 < slots[2] < 23552 and slots[3] == 0 and 0 < slots[4] < 23552


# ---- e. iso-surface meshes ----
@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", ["straddle", "negative"])
def test_mesh_keeps_its_triangles_and_equals_the_restatement(name, form):
    t = ps.TRANSLATION[name]
    _, RA = setup(None, form)
    _, RB = setup(name, form)
    lo, hi = lattice(t)
    iso = g64._median_iso(RA.resample(LAT_LO, LAT_HI, LAT_DIMS, channel=1, fill=NAN))
    va, ta, _ = RA.isosurface(LAT_LO, LAT_HI, LAT_DIMS, iso, channel=1, gradients=True)
    # vertices and gradients against the restatement and the point probe, in the translated frame (no tolerance on
    # vb - (va + t): the interpolation along an edge rounds differently in the two frames)
    vb, tb = tgi._compare(RB, lo, hi, LAT_DIMS, iso, 1, False, 500, f"amr3 {name} form {form}")
    assert np.array_equal(ta, tb) and len(va) == len(vb)


def test_mesh_of_a_derived_quantity_keeps_its_triangles_and_equals_the_restatement():
    t = ps.TRANSLATION["straddle"]
    _, RA = setup(None, 1)
    _, RB = setup("straddle", 1)
    lo, hi = lattice(t)
    QA = RA.resampleDerived(LAT_LO, LAT_HI, LAT_DIMS, "q", fill=NAN)
    QB = RB.resampleDerived(lo, hi, LAT_DIMS, "q", fill=NAN)
    assert np.array_equal(_bits(QA), _bits(QB)) and np.isnan(QA).any()
    iso = g64._median_iso(QA)
    va, ta = RA.isosurfaceDerived(LAT_LO, LAT_HI, LAT_DIMS, iso, "q")
    vb, tb = RB.isosurfaceDerived(lo, hi, LAT_DIMS, iso, "q")
    want_v, want_t = isomesh_ref.extract(QB, lo, hi, iso)
    assert len(tb) >= 500 and np.array_equal(ta, tb) and len(va) == len(vb)
    assert vb.tobytes() == want_v.astype(f32).tobytes() and tb.tobytes() == want_t.astype(np.int32).tobytes()


# ---- f. streamlines ----
def zero_plane_seeds(prep):
    """eight seeds in the planes x = 0, y = 0, z = 0 of a scene that reaches them, the last one the origin itself"""
    lo, hi = (x.astype(np.float64) for x in ps.root_box(prep))
    assert np.all(lo <= 0) and np.all(hi >= 0)
    rng = np.random.default_rng(11)
    s = rng.uniform(lo + 0.25 * (hi - lo), hi - 0.25 * (hi - lo), (8, 3))
    for i in range(7):
        s[i, i % 3] = 0.0
    s[6, 1] = 0.0                               # on the line x = y = 0
    s[7] = 0.0
    return s.astype(f32)


@pytest.mark.parametrize("name", ["straddle", "negative"])
def test_streamlines_equal_the_restatement_in_the_translated_frame(name):
    case, R = setup(name, 1)
    S = case.oracle_scene()
    seeds = np.ascontiguousarray(np.concatenate([tgs.seeds_of(R.prep), zero_plane_seeds(R.prep)]))
    chans = (0, 1, 2)
    crossing = 0
    for nm in (False, True):
        fwd = sr.streamlines(S, seeds, chans, tgs.STEP, tgs.MAX_STEPS, True, False, nm)
        back = sr.streamlines(S, seeds, chans, tgs.STEP, tgs.MAX_STEPS, False, True, nm)
        for (fw, bw), want in (((True, False), fwd), ((False, True), back), ((True, True), sr.joined(back, fwd))):
            got = R.streamlines(seeds, chans, tgs.STEP, tgs.MAX_STEPS, forward=fw, backward=bw, normalize=nm, velocities=True)
            tgs._same(got, want, (name, fw, bw, nm))
            for slot in ([1] if fw else []) + ([0] if bw else []):
                n = sr.reason_counts(got[3][:tgs.N_UNIFORM], slot)
                print(f"amr3 {name} fw {fw} bw {bw} norm {nm} slot {slot}: {n}")
                assert n[sr.END_LEFT] >= 10 and n[sr.END_MAXSTEPS] >= 10, n
            v, off = got[0], got[1].astype(np.int64)
            for i in range(len(off) - 1):
                line = v[off[i]:off[i + 1]]
                if len(line) and ((line.min(axis=0) < 0) & (line.max(axis=0) > 0)).any():
                    crossing += 1
    print(f"amr3 {name}: lines with vertices on both sides of a zero plane: {crossing}")
    if name == "straddle":                      # (`negative` reaches 0 only in the closed upper faces of its root box)
        assert crossing >= 10


# ---- g. frames ----
def _amr1(name):
    return ps.translated(scenes.amr(levels=3, fields=1), ps.TRANSLATION[name])


def _an_integer_interior_x_plane():
    """the integer x-plane that most regions of the single-channel amr3 scene share as a lower face"""
    P = binding.Prep(scenes.amr(levels=3, fields=1))
    x = np.stack(list(P.regions()["dom_lo"]))[:, 0]
    vals, counts = np.unique(x[(x == np.round(x)) & (x > x.min())], return_counts=True)
    P.close()
    return int(vals[np.argmax(counts)])


def _in_a_zero_plane():
    """the translated twin of amr_rays_in_an_x_plane (tests/test_gpu_parity.py): every ray lies in a face of many regions,
    and that face is the plane x = 0"""
    plane = _an_integer_interior_x_plane()
    scene = ps.translated(scenes.amr(levels=3, fields=1), (-plane, -20, -12))
    return Case(scene, W=64, H=48, grad=1, camera=dict(
        pos=np.array([0.0, -40.0, -2.9], f32), dir00=np.array([0.0, 1.0, -0.12], f32),
        dirDu=np.array([0.0, 0.0, 0.004], f32), dirDv=np.array([0.0, 0.006, 0.0], f32)))


def _from_the_origin(pos):
    """a camera at `pos` (the origin, or next to it) inside the scene translated by `straddle`, which puts the interior point
    (24, 20, 12) there; every component of the central direction is non-zero"""
    from owlexabrick_amd import harness
    cam = harness.camera([0, 0, 0], [13.0, 9.5, -7.25], [0, 1, 0], 50.0, 64, 48)
    mid = cam["dir00"] + f32(32) * cam["dirDu"] + f32(24) * cam["dirDv"]
    assert np.all(cam["pos"] == 0) and np.all(np.abs(mid) > 0.1 * np.abs(mid).max())
    cam["pos"] = np.array(pos, f32)
    return Case(_amr1("straddle"), W=64, H=48, grad=1, camera=cam)


def _far():
    """integer position 374 voxels from the scene's centre, dyadic directions and pixel steps (orthogonal to each other), dt = 1:
    positions out there have an ulp of 0.125"""
    t = np.array(ps.TRANSLATION["far"], dtype=np.float64)
    c = np.array([0.5, 0.25, 0.75])
    pos = t + np.array([24, 24, 16]) - 400 * c
    du, dv = np.array([3, 0, -2]) * 2.0 ** -11, np.array([-2, 13, -3]) * 2.0 ** -13
    assert np.dot(c, du) == 0 and np.dot(c, dv) == 0 and np.dot(du, dv) == 0
    cam = dict(pos=pos.astype(f32), dir00=(c - 32 * du - 24 * dv).astype(f32), dirDu=du.astype(f32), dirDv=dv.astype(f32))
    assert np.array_equal(cam["pos"].astype(np.float64), pos) and np.array_equal(cam["dir00"].astype(np.float64), c - 32 * du - 24 * dv)
    return Case(_amr1("far"), W=64, H=48, grad=1, dt=1.0, camera=cam)


FRAMES = {
    "straddle_grad": lambda: Case(_amr1("straddle"), W=64, H=48, grad=1),
    "straddle_iso": lambda: Case(_amr1("straddle"), W=64, H=48, grad=1, iso=[(0.45, 0)]),
    "straddle_band": lambda: Case(_amr1("straddle"), W=64, H=48, grad=1, xf=band_xf()),      # inactive regions are skipped
    "negative_grad": lambda: Case(_amr1("negative"), W=64, H=48, grad=1),
    "moderate_grad": lambda: Case(_amr1("moderate"), W=64, H=48, grad=1),
    "straddle_camera_at_the_origin": lambda: _from_the_origin([0.0, 0.0, 0.0]),
    # non-zero origin components below 2^-20: outside the short division's range, every wave takes the plain division
    "straddle_camera_next_to_the_origin": lambda: _from_the_origin([2.0 ** -22, -2.0 ** -25, 0.0]),
    "rays_in_a_region_face_at_zero": _in_a_zero_plane,
    "far_dyadic_camera": _far,
}


@pytest.mark.parametrize("form", [0, 1], ids=["source_order", "per_axis"])
@pytest.mark.parametrize("name", sorted(FRAMES))
def test_frames_match_the_oracle_on_every_walk(name, form):
    """the assertions of test_gpu_parity.py::test_hip_matches_oracle without its floor on exact_px (a measurement of the code
    under test), on the stack walk, the LBVH and the rope walk; and the rope walk's accum buffer is the stack walk's"""
    case = FRAMES[name]()
    case.basis_form, case.fast_math = form, 0
    o = case.run_oracle()
    assert o[2]["samples"] > 10000, o[2]                            # the camera sees the volume
    accum = {}
    for accel in (1, 0, 2):
        case.accel = accel
        h = case.run_hip(stats=True)
        r = compare(o, h, f"translated {name} {accel} {form} fast_math 0")
        print(error_profile_line(r))
        assert r["accum_bad"] == 0 and r["rgba_bad"] == 0, r
        assert r["max_ulp"] <= MAX_ULP_TIGHT, r
        assert {k: o[2][k] for k in STAT_KEYS} == {k: h[2][k] for k in STAT_KEYS}
        assert h[2]["diag"][8] == 0
        accum[accel] = h[1]
    assert np.array_equal(_bits(accum[2]), _bits(accum[1]))


# ---- h. the address form, the interleaving and the brick order ----
@pytest.mark.parametrize("option", [("addr64", 1), ("interleave", 0), ("brick_order", 1)], ids=lambda o: f"{o[0]}={o[1]}")
def test_options_change_no_bit_on_a_scene_that_straddles_the_origin(option):
    def run(options):
        case = FRAMES["straddle_grad"]()
        case.basis_form, case.fast_math, case.accel, case.options = 1, 0, 2, options
        R = case.hip_renderer()
        R.updateFrameID(0)
        R.render()
        accum = R.readAccum()
        pts = ps.dyadic_points(binding.Prep(scenes.amr(levels=3, fields=1)), ps.TRANSLATION["straddle"])
        probe = R.samplePoints(ps.moved(pts, ps.TRANSLATION["straddle"]), channels=(0,), gradient=True, fill=FILL)
        R.close()
        return accum, probe

    a0, p0 = run({})
    a1, p1 = run(dict([option]))
    assert np.abs(a0).max() > 0 and (p0[2] >= 0).sum() > 1000
    assert np.array_equal(_bits(a0), _bits(a1))
    assert np.array_equal(p0[2], p1[2]) and np.array_equal(_bits(p0[0]), _bits(p1[0])) and np.array_equal(_bits(p0[1]), _bits(p1[1]))


# ---- the multi-device handle and the command-line tool ----
def test_multi_device_handle_equals_single_on_a_translated_scene():
    t = ps.TRANSLATION["straddle"]
    case, R = setup("straddle", 1)
    _, RA = setup(None, 1)
    q = ps.moved(ps.dyadic_points(RA.prep, t), t)
    want = R.samplePoints(q, channels=(0, 1, 2), gradient=True, fill=FILL)
    r = R.fieldStats(1)
    box = ps.translated_boxes(t)[1]
    want_h = R.histogram(1, r["min"], r["max"], 128, box=box)
    M = multi_handle(R, 1)
    got = M.samplePoints(q, channels=(0, 1, 2), gradient=True, fill=FILL)
    assert np.array_equal(got[2], want[2]) and np.array_equal(_bits(got[0]), _bits(want[0])) and np.array_equal(_bits(got[1]), _bits(want[1]))
    got_h = M.histogram(1, r["min"], r["max"], 128, box=box)
    assert got_h[0].tobytes() == want_h[0].tobytes() and got_h[1].tobytes() == want_h[1].tobytes() and hr.same_stats(got_h[2], want_h[2])
    assert hr.same_stats(M.fieldStats(1), r) and int(want_h[0].sum()) > 0
    M.close()


def test_exarender_resamples_a_translated_scene_like_the_binding():
    case, R = setup("straddle", binding.DEFAULT_BASIS_FORM)
    lo, hi = R.prep.voxel_bounds()
    assert np.all(lo < 0) and np.all(hi > 0)
    ext = hi - lo
    lo, hi = (lo - 0.1 * ext).astype(f32), (hi + 0.1 * ext).astype(f32)
    dims = (23, 17, 9)
    want = R.resample(lo, hi, dims, channel=1, fill=-7.0)
    _, _, st = R.samplePoints(ps.grid_positions(lo, hi, dims), channels=(1,))
    invalid = int((st < 0).sum())
    assert 0 < invalid < st.size
    with tempfile.TemporaryDirectory() as d:
        cfg = scenes.write_exa(case.scene, d, "amr")
        raw = os.path.join(d, "grid.raw")
        r = subprocess.run([EXE, cfg, "--resample", *map(str, dims), raw, "--resample-channel", "1", "--resample-fill", "-7", "--frames", "0",
                            "--resample-box"] + [repr(float(v)) for v in lo] + [repr(float(v)) for v in hi],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        got = np.fromfile(raw, dtype=f32)
    assert got.tobytes() == want.tobytes()
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("resample ")]
    assert len(line) == 1, r.stdout
    m = re.fullmatch(r"resample 23 17 9 box (\S+ ){6}channel 1 invalid (\d+)", line[0])
    assert m and int(m.group(2)) == invalid, line[0]


# ---- coordinates the float32 tables cannot hold, in a scene filled by hand ----
def test_renderer_creation_refuses_a_brick_whose_planes_are_no_float32():
    prep = binding.Prep(scenes.amr(levels=3, fields=1))
    lower = prep.bricks()["lower"]
    saved = lower[5].copy()
    lower[5] = (0, 2 ** 24 + 1, 0)                              # an odd integer beyond 2^24 is no float32
    with pytest.raises(RuntimeError, match=r"exa_hip_create: brick 5 \(lower 0 16777217 0, .*: its plane y = 16777217 is not a float32"):
        binding.Renderer(prep)
    lower[5] = saved
    binding.Renderer(prep).close()                              # the scene as it was prepared is taken
