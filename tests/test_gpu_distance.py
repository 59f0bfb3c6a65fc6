"""The distance transform on the GPU (exa_hip_distance, include/exa_hip.h): dist and nearest equal the numpy restatement of
the passes (tests/distance_ref.py) byte for byte and the stats are equal — on constructed masks through exa_hip_distance_mask
(rows over one and two 64-lane chunks, every axis in turn the long one; a far corner, no target, every point, a checkerboard,
symmetric planes, sparse and dense random sets; isotropic and anisotropic spacing; labels from the host and from the device),
on the scenes of the iso-surface tests fed the lattice exa_hip_resample returns, for a derived quantity and in world space;
a reach at, just below and just above a distance that occurs; nothing a frame or a tuning knob sets changes a byte; bad
arguments are refused with a message and leave the handle usable; the bands of a distance are a label axis of the profile.
The failed allocation has no test."""
import ctypes as C
import math

import numpy as np
import pytest

import distance_ref as ref
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from owlexabrick_amd import distance as dt
from test_gpu_isomesh import CASES, DIMS, XFM, _isos, _root_box

pytestmark = pytest.mark.gpu

NAN = float("nan")
F = np.float32
FLT_MAX = float(np.finfo(np.float32).max)
SHAPES = [(1, 1, 1), (65, 1, 1), (1, 65, 1), (1, 1, 65), (130, 3, 2), (3, 130, 2), (2, 3, 130), (67, 9, 7)]      # (nx, ny, nz)


def _same(got, want, what, nearest=True):
    dist, near, stats = want
    print(what, got["stats"])
    g = got["dist"]
    assert g.dtype == F and g.shape == dist.shape, (what, g.shape, dist.shape)
    assert g.tobytes() == dist.tobytes(), (what, np.argwhere(g.view(np.uint32) != dist.view(np.uint32))[:5])
    if nearest:
        assert got["nearest"].dtype == np.int32 and got["nearest"].tobytes() == near.tobytes(), \
            (what, np.argwhere(got["nearest"] != near)[:5])
    else:
        assert "nearest" not in got
    assert got["stats"] == stats, (what, got["stats"], stats)


def _bytes(got):
    return got["dist"].tobytes(), got["nearest"].tobytes(), got["stats"]


def _targets(shape, rng):
    """name -> boolean lattice [nz, ny, nx]"""
    nx, ny, nz = shape
    zyx = (nz, ny, nx)
    corner = np.zeros(zyx, bool)
    corner[-1, -1, -1] = True
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    planes = np.zeros(zyx, bool)
    for axis, n in enumerate(zyx):                      # the two end planes of the long axis: every point between them ties
        if n == max(zyx):
            sel = [slice(None)] * 3
            sel[axis] = [0, n - 1]
            planes[tuple(sel)] = True
            break
    return {"far corner": corner, "empty": np.zeros(zyx, bool), "full": np.ones(zyx, bool), "checkerboard": (i + j + k) % 2 == 0,
            "planes": planes, "random 2%": rng.random(zyx) < 0.02, "random 90%": rng.random(zyx) < 0.9}


@pytest.fixture(scope="module")
def amr3():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    yield case, R
    R.close()


@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_constructed_masks_equal_the_restatement(amr3, shape):
    import torch
    _, R = amr3
    rng = np.random.default_rng(sum(shape))
    lo = (0.5, -1.0, 2.0)
    boxes = {"isotropic": tuple(l + 0.25 * n for l, n in zip(lo, shape))}
    for long_axis in range(3):
        boxes[f"axis {long_axis} x10"] = tuple(l + (2.5 if a == long_axis else 0.25) * n for a, (l, n) in enumerate(zip(lo, shape)))
    for name, inside in _targets(shape, rng).items():
        labels = np.where(inside, 3, rng.integers(-1, 3, inside.shape)).astype(np.int32)         # label 3 is the set
        any_label = np.where(inside, rng.integers(0, 5, inside.shape), -1).astype(np.int32)      # label -1: labels >= 0
        device = torch.from_numpy(labels.reshape(-1)).to("cuda:0")
        for box, hi in boxes.items():
            what = f"{shape} {name} {box}"
            want = ref.distance(inside, lo, hi)
            _same(dt.distance_mask(R, lo, hi, shape, labels, label=3, nearest=True), want, what + " host labels")
            _same(dt.distance_mask(R, lo, hi, shape, device, label=3, nearest=True), want, what + " device labels")
            _same(dt.distance_mask(R, lo, hi, shape, any_label, nearest=True), want, what + " any label")
            _same(dt.distance_mask(R, lo, hi, shape, labels, label=3), want, what + " no nearest", nearest=False)
            _same(dt.distance_mask(R, lo, hi, shape, device, label=3, to_outside=True, nearest=True),
                  ref.distance(inside, lo, hi, to_outside=True), what + " to outside")
            _same(dt.distance_mask(R, lo, hi, shape, labels, label=3, signed=True, nearest=True),
                  ref.distance(inside, lo, hi, signed=True), what + " signed")
            # three cells of 0.25: in the isotropic box a distance that occurs, exactly; at it, just below and just above
            for reach in (F(0.75), np.nextafter(F(0.75), F(0)), np.nextafter(F(0.75), F(1))) if box == "isotropic" else (F(0.75),):
                _same(dt.distance_mask(R, lo, hi, shape, labels, label=3, max_distance=float(reach), nearest=True),
                      ref.distance(inside, lo, hi, max_distance=float(reach)), what + f" reach {reach!r}")


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{c[0]}-f{c[2]}" for c in CASES])
def test_fields_equal_the_restatement_fed_the_resampled_lattice(idx):
    name, make, form, empty, _ = CASES[idx]
    case = Case(make(), basis_form=form, allow_empty_cells=empty)
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    channel = len(case.scene.fields) - 1
    V = R.resample(lo, hi, DIMS, channel=channel, fill=NAN)
    assert np.isnan(V).any(), name                             # the box overhangs the scene
    for label, iso in _isos(V):
        inside = ref.inside_of(V, iso)
        assert inside.any() and (~inside).any(), (name, label)
        what = f"{name} form {form} {label} iso {iso!r}"
        _same(dt.distance(R, lo, hi, DIMS, iso, channel=channel, nearest=True), ref.distance(inside, lo, hi), what)
        _same(dt.distance(R, lo, hi, DIMS, iso, channel=channel, below=True, nearest=True),
              ref.distance(ref.inside_of(V, iso, below=True), lo, hi), what + " below")
        _same(dt.distance(R, lo, hi, DIMS, iso, channel=channel, to_outside=True, nearest=True),
              ref.distance(inside, lo, hi, to_outside=True), what + " to outside")
        _same(dt.distance(R, lo, hi, DIMS, iso, channel=channel, signed=True, nearest=True),
              ref.distance(inside, lo, hi, signed=True), what + " signed")
    # the wall distance: to the nearest point without data
    wall = dt.distance(R, lo, hi, DIMS, -FLT_MAX, channel=channel, to_outside=True, nearest=True)
    _same(wall, ref.distance(np.isfinite(V), lo, hi, to_outside=True), f"{name} wall")
    assert (wall["dist"] == 0).tobytes() == (~np.isfinite(V)).tobytes()
    R.close()


def test_a_derived_quantity_and_world_space():
    case = Case(scenes.amr(levels=3, fields=3))
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    Q = R.resampleDerived(lo, hi, DIMS, "q", channels=(0, 1, 2), fill=NAN)
    inside = ref.inside_of(Q, 0.0)
    assert inside.any() and (~inside).any() and np.isnan(Q).any()
    _same(dt.distance(R, lo, hi, DIMS, 0.0, quantity="q", channels=(0, 1, 2), nearest=True), ref.distance(inside, lo, hi), "Q >= 0")
    _same(dt.distance(R, lo, hi, DIMS, 0.0, quantity="q", channels=(0, 1, 2), signed=True, nearest=True),
          ref.distance(inside, lo, hi, signed=True), "Q >= 0 signed")
    # world space: the values of the mapped box's lattice, distances in the caller's space
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    wlo, whi, dims = np.array([-4, -6, -5], F), np.array([30, 24, 26], F), (41, 33, 27)
    V = R.resample(wlo, whi, dims, channel=1, world=True, fill=NAN)
    iso = _isos(V)[0][1]
    inside = ref.inside_of(V, iso)
    assert inside.any() and (~inside).any() and np.isnan(V).any()
    got = dt.distance(R, wlo, whi, dims, iso, channel=1, world=True, nearest=True)
    _same(got, ref.distance(inside, wlo, whi), "world")
    _same(dt.distance_mask(R, wlo, whi, dims, inside.astype(np.int32) - 1, nearest=True), ref.distance(inside, wlo, whi), "world, as a mask")
    voxel = dt.distance(R, wlo, whi, dims, iso, channel=1, nearest=True)
    assert voxel["dist"].tobytes() != got["dist"].tobytes()
    R.close()


def test_max_distance_at_and_beside_a_distance_that_occurs(amr3):
    _, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    inside = ref.inside_of(V, iso)
    full, _, _ = ref.distance(inside, lo, hi)
    occurring = np.unique(full[np.isfinite(full) & (full > 0)])
    d = F(occurring[occurring.size // 2])
    reached = {}
    for what, reach in (("at", d), ("below", np.nextafter(d, F(0))), ("above", np.nextafter(d, F(np.inf))), ("8 cells", 8 * float(ref.spacing(lo, hi, DIMS)[0]))):
        got = dt.distance(R, lo, hi, DIMS, iso, channel=1, max_distance=float(reach), nearest=True)
        _same(got, ref.distance(inside, lo, hi, max_distance=float(reach)), f"reach {what} {reach!r}")
        reached[what] = got["stats"]["reached"]
        keep = np.isfinite(got["dist"])
        assert got["dist"][keep].tobytes() == full[keep].tobytes() and (full[keep] <= F(reach)).all(), what
    # the reach test is d2 <= fl(reach*reach), not dist <= reach: whether the points at d itself are reached hangs on two
    # roundings (the exact case is in the constructed masks), but the counts are ordered and a reach cuts something off
    assert 0 < reached["below"] <= reached["at"] <= reached["above"] < int(np.isfinite(full).sum()), reached


def test_distances_do_not_depend_on_frame_state_options_or_where_the_arrays_live(amr3):
    import torch
    case, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    call = lambda H=None, **kw: dt.distance(H or R, lo, hi, DIMS, iso, channel=1, signed=True, nearest=True, **kw)      # noqa: E731
    first = call()
    _same(first, ref.distance(ref.inside_of(V, iso), lo, hi, signed=True), "before")
    want = _bytes(first)
    assert _bytes(call()) == want, "two consecutive calls"
    ms = dt.distance_stage_ms(R)
    assert len(ms) == 4 and all(m > 0 for m in ms), ms
    n = int(np.prod(DIMS))
    dist, near = torch.empty(n, dtype=torch.float32, device="cuda:0"), torch.empty(n, dtype=torch.int32, device="cuda:0")
    got = call(out=(dist, near))
    assert (dist.cpu().numpy().tobytes(), near.cpu().numpy().tobytes(), got["stats"]) == want, "device outputs"
    got = dt.distance(R, lo, hi, DIMS, iso, channel=1, signed=True, out=(dist.zero_(), None))
    assert dist.cpu().numpy().tobytes() == want[0] and "nearest" not in got, "device dist alone"
    M = multi_handle(R)
    assert _bytes(call(M)) == want, "a multi-device handle"
    M.close()
    for what in frame_perturbations(case, R):
        assert _bytes(call()) == want, what
    for patch in range(4):
        R.setOption("sample_patch", patch)
        assert _bytes(call()) == want, f"sample_patch {patch}"
    R.setOption("sample_patch", 0)
    # regions, an iso-surface and a distance call coexist
    regions = R.extractRegions(lo, hi, DIMS, iso, channel=1)
    R.extractIsoSurface(lo, hi, DIMS, iso, channel=1)
    assert _bytes(call()) == want, "between two extractions and their reads"
    verts, tris, _ = R.readIsoSurface()
    labels = R.readRegions()["labels"]
    assert len(tris) > 0 and regions[0] > 0
    R.releaseIsoSurface()
    R.releaseRegions()
    inside = ref.inside_of(V, iso)
    assert ((labels >= 0) == inside).all()
    _same(dt.distance_mask(R, lo, hi, DIMS, labels, signed=True, nearest=True), (first["dist"], first["nearest"], first["stats"]),
          "the regions' labels as the mask")


# ---- errors ----
def _raw(R, which="field", lo=(0, 0, 0), hi=(8, 8, 8), dims=(9, 9, 9), channel=0, channels=(0, 1, 2), quantity=4, iso=0.5,
         labels="host", label=-1, max_distance=math.inf, flags=0, null=()):
    """a C entry point with one thing wrong; `null`: names of pointers passed as NULL"""
    n = 729
    dist, near = np.full(n, 77, F), np.full(n, 77, np.int32)
    lab = np.zeros(n, np.int32)
    st = dt.ExaHipDistanceStats()
    p = lambda name, obj: None if name in null else obj            # noqa: E731
    head = (R.h, p("lo", (C.c_float * 3)(*lo)), p("hi", (C.c_float * 3)(*hi)), p("dims", (C.c_int32 * 3)(*dims)))
    tail = (float(max_distance), flags, p("dist", dist.ctypes.data), near.ctypes.data, C.byref(st), 0, None)
    L = binding.lib()
    if which == "field":
        rc = L.exa_hip_distance(*head, channel, float(iso), *tail)
    elif which == "derived":
        rc = L.exa_hip_distance_derived(*head, p("channels", (C.c_int32 * 3)(*channels)), quantity, float(iso), *tail)
    else:
        rc = L.exa_hip_distance_mask(*head, p("labels", lab.ctypes.data), label, *tail)
    untouched = bool(np.all(dist == 77) and np.all(near == 77))
    return rc, untouched, L.exa_hip_last_error(R.h).decode()


NAMES = {"field": "exa_hip_distance: ", "derived": "exa_hip_distance_derived: ", "mask": "exa_hip_distance_mask: "}


def test_refused_arguments():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()                                    # no render yet: the module holds no frame state
    lo, hi, dims = (0, 0, 0), (8, 8, 8), (9, 9, 9)
    V = R.resample(lo, hi, dims, channel=0, fill=NAN)
    iso = float(np.median(V[np.isfinite(V)]))
    want = ref.distance(ref.inside_of(V, iso), lo, hi)
    nf = len(case.scene.fields)
    common = [dict(null=("lo",)), dict(null=("hi",)), dict(null=("dims",)), dict(null=("dist",)), dict(lo=(math.nan, 0, 0)),
              dict(hi=(8, math.inf, 8)), dict(lo=(-3e38, 0, 0), hi=(3e38, 8, 8)), dict(dims=(0, 9, 9)), dict(dims=(9, 9, -1)),
              dict(dims=(2 ** 11, 2 ** 11, 2 ** 9)), dict(max_distance=math.nan), dict(max_distance=0.0), dict(max_distance=-1.0),
              dict(max_distance=-math.inf), dict(flags=dt.DISTANCE_SIGNED | dt.DISTANCE_TO_OUTSIDE), dict(flags=2), dict(flags=16),
              dict(flags=512), dict(flags=1 << 30)]
    bad = {"field": common + [dict(flags=binding.SAMPLE_WORLD_SPACE), dict(channel=nf), dict(channel=-1), dict(iso=math.nan), dict(iso=math.inf),
                              dict(flags=dt.DISTANCE_LABELS_DEVICE)],
           "derived": common + [dict(flags=binding.SAMPLE_WORLD_SPACE), dict(null=("channels",)), dict(quantity=2), dict(quantity=99),
                                dict(channels=(0, 1, nf)), dict(iso=math.nan), dict(flags=dt.DISTANCE_LABELS_DEVICE)],
           "mask": common + [dict(null=("labels",)), dict(label=-2), dict(label=-2 ** 31), dict(flags=dt.DISTANCE_BELOW)]}
    for which, cases in bad.items():
        for kw in cases:
            rc, untouched, msg = _raw(R, which, **kw)
            assert rc != 0 and untouched and msg.startswith(NAMES[which]), (which, kw, rc, msg)
            _same(dt.distance(R, lo, hi, dims, iso, nearest=True), want, f"after {which} {sorted(kw)}")      # the handle still works, and rightly
    assert "frame state" in _raw(R, flags=binding.SAMPLE_WORLD_SPACE)[2]
    assert "EXA_DISTANCE_SIGNED" in _raw(R, "mask", flags=dt.DISTANCE_SIGNED | dt.DISTANCE_TO_OUTSIDE)[2]
    assert "maxDistance" in _raw(R, "mask", max_distance=0.0)[2] and "label" in _raw(R, "mask", label=-2)[2]
    # the valid raw calls pass; the mask call takes the world-space flag and ignores it, before a frame state too
    assert _raw(R)[0] == 0 and _raw(R, "derived")[0] == 0 and _raw(R, "mask")[0] == 0
    assert _raw(R, "mask", flags=binding.SAMPLE_WORLD_SPACE)[0] == 0
    frame = R.render()
    assert _raw(R, flags=binding.SAMPLE_WORLD_SPACE)[0] == 0
    assert R.render().shape == frame.shape
    R.close()


def test_scene_without_kd_tree_is_refused_for_the_fields_only():
    R = without_kd_tree(Case(scenes.amr(levels=3, fields=3), W=32, H=32)).hip_renderer()
    for which in ("field", "derived"):
        rc, untouched, msg = _raw(R, which)
        assert rc != 0 and untouched and msg.startswith(NAMES[which]) and "kd-tree" in msg, msg
    rng = np.random.default_rng(5)
    inside = rng.random((7, 8, 9)) < 0.1
    lo, hi, dims = (0, 0, 0), (9, 4, 7), (9, 8, 7)
    _same(dt.distance_mask(R, lo, hi, dims, inside.astype(np.int32) - 1, nearest=True), ref.distance(inside, lo, hi), "no kd tree, a mask")
    assert R.render().shape == (32, 32)                        # the handle still renders (through its LBVH)
    R.close()


def test_bands_of_a_distance_are_a_label_axis_of_the_profile(amr3):
    _, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    W = R.resample(lo, hi, DIMS, channel=0, fill=NAN)
    iso = _isos(V)[0][1]
    got = dt.distance(R, lo, hi, DIMS, iso, channel=1, signed=True)
    width, n = float(ref.spacing(lo, hi, DIMS).max()), 4
    bands = dt.distance_bands(got["dist"], width, n)
    assert bands.tobytes() == ref.bands(got["dist"], width, n).tobytes() and bands.shape == V.shape
    assert len(np.unique(bands)) >= 3                          # several bands hold points
    prof = R.profile(lo, hi, DIMS, binding.labels(bands, n), [binding.channel(0)])
    e = prof["stats"]["valueExponent"][0]
    assert prof["count"].sum() > 0
    for b in range(n):
        sel = (bands == b) & np.isfinite(W)
        assert prof["count"][b] == int(sel.sum()), b
        fixed = np.rint(W[sel].astype(np.float64) * 2.0 ** e).astype(np.int64).sum()
        assert prof["sums"][0][b] == fixed, b
