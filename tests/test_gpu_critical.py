"""Critical points on the GPU (exa_hip_critical_points, include/exa_hip.h): the records, the stats and the probe's arrays equal,
byte for byte, the numpy restatement of the contract (tests/critical_ref.py) fed the three lattices exa_hip_resample returns,
and exa_hip_sample_points at the found positions — on an AMR scene and on the odd grids of the histogram test, whose extra
fields are set per cell from the cell centres: the linear fields A (x - c) of tests/test_critical_ref.py and a sine field;
on one cell, on partial blocks, on a lattice that reaches outside the scene, across more than one scan chunk with more than
one block of found points and with rejects, for 1, 8 and 32 iterations, both ends of the tolerance, a slab of zeros and world
space; nothing a frame or a tuning knob sets changes a byte, in both basis forms; the mesh, the lines, the regions and the
points coexist; bad arguments are refused with a message and leave the handle usable.  The failed allocation has no test.

The choices below were checked without a GPU first, with the restatement on the lattice of tests/probe_ref64.py: every linear
field reconstructs to exactly one point of its kind near c = (17.3, 21.6, 13.2) on both lattices used here, and the sine field
of wavelengths (10, 12, 11) gives 365 found points and 13 rejects (all leftCell) on the 96^3 lattice."""
import ctypes as C
import math

import numpy as np
import pytest

import critical_ref as ref
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from histogram_ref import Slots
from owlexabrick_amd import binding, scenes
from test_critical_ref import LINEAR
from test_gpu_histogram import ODD_GRIDS
from test_gpu_isomesh import XFM, _root_box

pytestmark = pytest.mark.gpu

NAN = float("nan")
CENTRE = np.array([17.3, 21.6, 13.2])
WAVE = (10.0, 12.0, 11.0)
PHASE = (0.3, 0.7, 1.1)
DEFAULT = LINEAR["spiral_saddle_2"][0]


def _with_fields(scene, fns):
    """the scene with one more field per fn, fn(cell centres [n, 3]) per cell slot"""
    S = Slots(scene)
    centre = S.centre2.astype(np.float64) / 2.0
    fields = list(scene.fields)
    for fn in fns:
        f = np.zeros(len(scene.fields[0]), np.float32)
        f[S.ids[S.ids >= 0]] = np.asarray(fn(centre))[S.ids >= 0].astype(np.float32)
        fields.append(f)
    return scenes.Scene(scene.bricks7, scene.cellIDs, fields, name=scene.name + "_flow", value_range=scene.value_range,
                        meta=dict(scene.meta))


def _linear(A, c, keep=None):
    A = np.asarray(A, np.float64)
    return [lambda p, r=r: ((p - c) @ A[r]) * (1.0 if keep is None else keep(p)) for r in range(3)]


def _sine():
    return [lambda p, a=a: np.sin(2 * np.pi / WAVE[a] * p[:, a] + PHASE[a]) for a in range(3)]


def _bounds(R):
    lo, hi = R.prep.voxel_bounds()
    return np.asarray(lo, np.float32), np.asarray(hi, np.float32)


def _holds(rec, p, lo, hi, dims):
    """the record's cell and local coordinates name the point p of the lattice's space (a root may sit on a lattice plane,
    where the rule and the rounding choose between two cells: so the cell is not computed from p)"""
    cell = int(rec["cell"])
    idx = np.array([cell % dims[0], (cell // dims[0]) % dims[1], cell // (dims[0] * dims[1])], np.float64)
    step = (hi.astype(np.float64) - lo) / np.array(dims)
    return bool(np.abs(lo + (idx + 0.5 + rec["local"]) * step - p).max() < 0.01 and np.abs(rec["position"] - p).max() < 0.01)


def test_the_binding_s_record_is_the_restatement_s():
    assert binding.CRITICAL_POINT_DTYPE == ref.POINT_DTYPE and binding.CRITICAL_POINT_DTYPE.itemsize == 104
    assert binding.CRITICAL_STATS == ref.STATS
    assert (binding.CRITICAL["spiral"], binding.CRITICAL["degenerate"]) == (ref.SPIRAL, ref.DEGENERATE)


def _compare(R, lo, hi, dims, channels, what, iterations=8, tolerance=2.0 ** -10, world=False):
    """the call against the restatement on the lattices R.resample returns, and its probe against R.samplePoints; returns the
    restatement's (records, stats)"""
    V = [R.resample(lo, hi, dims, channel=c, world=world, fill=NAN) for c in channels]
    want, want_stats, _ = ref.critical_points(V, lo, hi, iterations=iterations, tolerance=tolerance)
    got, stats, probe, status = R.criticalPoints(lo, hi, dims, channels=channels, iterations=iterations, tolerance=tolerance,
                                                 world=world, probe=True)
    print(f"{what}: {stats} types {np.bincount(want['type'] & 15, minlength=16).tolist()}")
    assert stats == want_stats, (what, stats, want_stats)
    assert len(got) == len(want), what
    for name in ref.POINT_DTYPE.names:
        assert got[name].tobytes() == want[name].tobytes(), (what, name, got[name][:4], want[name][:4])
    assert got.tobytes() == want.tobytes(), what
    assert probe.shape == (len(want), 3, 4) and status.shape == (len(want), 3)
    if len(want):
        values, grads, st = R.samplePoints(want["position"], channels, gradient=True, normalized=True, world=world)
        assert probe[:, :, 0].tobytes() == values.tobytes() and probe[:, :, 1:].tobytes() == grads.tobytes(), what
        assert status.tobytes() == st.tobytes(), what
    plain, stats2 = R.criticalPoints(lo, hi, dims, channels=channels, iterations=iterations, tolerance=tolerance, world=world)
    assert plain.tobytes() == want.tobytes() and stats2 == want_stats, (what, "without the probe")
    return want, want_stats


# ---- the AMR scene: channel 0 its own field, 1..3 the default linear field, 4..6 the sine field ----
FLOW, SINE = (1, 2, 3), (4, 5, 6)


@pytest.fixture(scope="module")
def amr3():
    case = Case(_with_fields(scenes.amr(levels=3, fields=1), _linear(DEFAULT, CENTRE) + _sine()), W=32, H=32)
    R = case.hip_renderer()
    yield case, R
    R.close()


@pytest.mark.parametrize("dims", [(2, 2, 2), (9, 10, 11), (37, 29, 23)], ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("channels", [FLOW, SINE], ids=["linear", "sine"])
def test_points_equal_the_restatement_byte_for_byte(amr3, dims, channels):
    case, R = amr3
    lo, hi = _bounds(R)
    want, stats = _compare(R, lo, hi, dims, channels, f"amr3 {dims} {channels}")
    assert stats["cells"] == (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1) and stats["invalidCells"] == 0
    if channels == FLOW and dims != (2, 2, 2):
        assert stats["found"] == 1 and want["type"][0] == 2 | ref.SPIRAL and _holds(want[0], CENTRE, lo, hi, dims)
        assert np.abs(want["position"][0] - CENTRE).max() < 0.01
        # the probe of the real field at the lattice's root: a small residual, and the matrix as the voxel-space Jacobian
        _, _, probe, status = R.criticalPoints(lo, hi, dims, channels=channels, probe=True)
        assert np.all(status >= 0) and np.abs(probe[0, :, 0]).max() < 1e-3 and np.abs(probe[0, :, 1:] - np.array(DEFAULT)).max() < 1e-3
    if channels == SINE and dims == (37, 29, 23):
        assert stats["found"] > 256 and stats["leftCell"] > 0


def test_lattice_reaching_outside_the_scene(amr3):
    case, R = amr3
    lo, hi = _root_box(R.prep, 0.1)
    for channels in (FLOW, SINE):
        want, stats = _compare(R, lo, hi, (37, 29, 23), channels, f"amr3 grown {channels}")
        assert 0 < stats["invalidCells"] < stats["cells"] and stats["found"] >= 1
    # channels may repeat: two components that are the same have a singular matrix everywhere
    want, stats = _compare(R, lo, hi, (19, 17, 13), (1, 1, 2), "amr3 repeated channels")
    assert stats["found"] == 0


@pytest.mark.parametrize("name", list(LINEAR))
def test_every_linear_field_gives_one_point_of_its_kind(name):
    A, nplus, spiral = LINEAR[name]
    R = Case(_with_fields(scenes.amr(levels=3, fields=1), _linear(A, CENTRE)), W=32, H=32).hip_renderer()
    lo, hi = _bounds(R)
    for dims in [(9, 10, 11), (37, 29, 23)]:
        want, stats = _compare(R, lo, hi, dims, FLOW, f"{name} {dims}")
        assert stats["found"] == 1 and want["type"][0] == nplus | (ref.SPIRAL if spiral else 0), (name, dims, want)
        assert _holds(want[0], CENTRE, lo, hi, dims)
    R.close()


def test_more_than_one_scan_chunk_more_than_one_block_of_points_and_rejects(amr3):
    case, R = amr3
    lo, hi = _bounds(R)
    dims = (96, 96, 96)
    assert dims[0] * dims[1] * dims[2] > 2048 * 256
    want, stats = _compare(R, lo, hi, dims, SINE, "amr3 96^3 sine")
    assert stats["found"] > 256 and stats["nonFinite"] + stats["leftCell"] + stats["notConverged"] > 0
    assert (want["cell"] < 2048 * 256).any() and (want["cell"] >= 2048 * 256).any()


@pytest.mark.parametrize("iterations,tolerance", [(1, 1.0), (1, 2.0 ** -20), (8, 2.0 ** -10), (32, 1.0), (32, 2.0 ** -20)])
def test_iterations_and_tolerance(amr3, iterations, tolerance):
    case, R = amr3
    lo, hi = _bounds(R)
    want, stats = _compare(R, lo, hi, (37, 29, 23), SINE, f"amr3 sine {iterations} {tolerance}", iterations=iterations, tolerance=tolerance)
    assert stats["candidates"] > 256
    if (iterations, tolerance) == (1, 2.0 ** -20):
        assert stats["notConverged"] > 0


def test_slab_of_zeros():
    """the linear field set to zero in the cells below x = 8: the lattice cells inside the slab hold constant components and
    are no candidates, the layer around it is mostly rejected as nonFinite (0/0 on the face of zeros), the one point stays.
    Where fine and coarse cells meet, a cell of that layer has zeros at some corners of a face only, and the interpolant's
    zeros on that face are found by the rule (three of them on the reconstruction in float64)"""
    R = Case(_with_fields(scenes.amr(levels=3, fields=1), _linear(DEFAULT, CENTRE, keep=lambda p: p[:, 0] >= 8.0)), W=32, H=32).hip_renderer()
    lo, hi = _bounds(R)
    dims = (37, 29, 23)
    V = R.resample(lo, hi, dims, channel=1, fill=NAN)
    assert (V[:, :, :4] == 0).all() and (V[:, :, 8:] != 0).any()
    want, stats = _compare(R, lo, hi, dims, FLOW, "amr3 zero slab")
    assert stats["nonFinite"] > 100 and (np.abs(want["position"] - CENTRE).max(axis=1) < 0.01).sum() == 1
    assert (want["cell"] % dims[0] >= 4).all()
    R.close()


def test_points_in_world_space():
    case = Case(_with_fields(scenes.amr(levels=3, fields=1), _sine()))
    R = case.hip_renderer()
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lo, hi = np.array([-4, -6, -5], np.float32), np.array([30, 24, 26], np.float32)
    want, stats = _compare(R, lo, hi, (41, 33, 27), FLOW, "amr3 world", world=True)
    assert stats["invalidCells"] > 0 and stats["found"] > 0
    voxel = R.criticalPoints(lo, hi, (41, 33, 27), channels=FLOW)[0]
    assert voxel.tobytes() != want.tobytes()
    R.close()


@pytest.fixture(scope="module")
def odd():
    scene = scenes.artificial(scenes.parse_grids(ODD_GRIDS), name="odd")
    case = Case(_with_fields(scene, _linear(DEFAULT, np.array([4.4, 5.3, 5.6])) + _sine()), W=32, H=32)
    R = case.hip_renderer()
    yield case, R
    R.close()


@pytest.mark.parametrize("dims", [(2, 2, 2), (9, 10, 11), (37, 29, 23)], ids=lambda d: "x".join(map(str, d)))
def test_odd_grids(odd, dims):
    case, R = odd
    for lo, hi in (_bounds(R), _root_box(R.prep, 0.1)):
        for channels in (FLOW, SINE):
            want, stats = _compare(R, lo, hi, dims, channels, f"odd {dims} {channels}")
            assert stats["invalidCells"] > 0                        # the grids leave most of their bounding box empty
    # the lattice of the first grid's own cell centres
    want, stats = _compare(R, (0, 0, 0), (9, 10, 11), (9, 10, 11), FLOW, "odd first grid")
    assert stats["invalidCells"] == 0 and stats["found"] == 1 and want["cell"][0] == (5 * 10 + 4) * 9 + 3


def _bytes(got):
    points, stats, probe, status = got
    return [points.tobytes(), tuple(stats.items()), probe.tobytes(), status.tobytes()]


@pytest.mark.parametrize("form", [0, 1])
def test_points_do_not_depend_on_frame_state_or_options(form):
    case = Case(_with_fields(scenes.amr(levels=3, fields=1), _linear(DEFAULT, CENTRE) + _sine()), W=32, H=32, basis_form=form)
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep, 0.1)
    dims = (37, 29, 23)
    want_rec, _ = _compare(R, lo, hi, dims, SINE, f"form {form}")
    call = lambda H: _bytes(H.criticalPoints(lo, hi, dims, channels=SINE, probe=True))        # noqa: E731
    want = call(R)
    assert want[0] == want_rec.tobytes() and len(want_rec) > 256
    assert call(R) == want, "two consecutive calls"
    M = multi_handle(R, form)
    assert call(M) == want, "a multi-device handle"
    M.close()
    for what in frame_perturbations(case, R):
        assert call(R) == want, what
    for patch in range(4):
        R.setOption("sample_patch", patch)
        assert call(R) == want, f"sample_patch {patch}"
    R.setOption("sample_uniform", 0)
    assert call(R) == want, "sample_uniform 0"
    R.close()


def test_results_do_not_drop_each_other_and_a_second_extraction_replaces_the_first(amr3):
    import torch
    case, R = amr3
    lo, hi = _bounds(R)
    dims = (37, 29, 23)
    plane, size = ((float(lo[0]), float(lo[1]), 0.5 * float(lo[2] + hi[2])), (float(hi[0] - lo[0]) / 64, 0.0, 0.0),
                   (0.0, float(hi[1] - lo[1]) / 9, 0.0)), (64, 9)
    want_sine = R.criticalPoints(lo, hi, dims, channels=SINE)[0]
    want_flow = R.criticalPoints(lo, hi, dims, channels=FLOW)[0]
    want_mesh = R.isosurface(lo, hi, (19, 17, 13), 0.0, channel=4)
    want_lines = R.isolines(*plane, size, [0.0], channel=4)
    want_regions = R.regions(lo, hi, dims, 0.0, channel=4)
    assert len(want_mesh[1]) > 0 and len(want_lines["segments"]) > 0 and len(want_regions["regions"]) > 0 and len(want_sine) > 256
    R.extractIsoSurface(lo, hi, (19, 17, 13), 0.0, channel=4)
    R.extractIsolines(*plane, size, [0.0], channel=4)
    R.extractRegions(lo, hi, dims, 0.0, channel=4)
    n, stats = R.extractCriticalPoints(lo, hi, dims, channels=SINE)
    mesh, lines, regions = R.readIsoSurface(), R.readIsolines(), R.readRegions()      # extracted before the points: still there
    assert mesh[0].tobytes() == want_mesh[0].tobytes() and mesh[1].tobytes() == want_mesh[1].tobytes()
    assert all(lines[k].tobytes() == want_lines[k].tobytes() for k in want_lines)
    assert regions["labels"].tobytes() == want_regions["labels"].tobytes() and regions["regions"].tobytes() == want_regions["regions"].tobytes()
    R.extractIsoSurface(lo, hi, (9, 9, 9), 0.0, channel=4)
    R.extractIsolines(*plane, (8, 8), [0.0], channel=4)
    R.extractRegions(lo, hi, (9, 9, 9), 0.0, channel=4)
    R.releaseIsoSurface()
    R.releaseIsolines()
    R.releaseRegions()
    got = R.readCriticalPoints()                                       # behind later results of the others and their release
    assert n == len(want_sine) and got[0].tobytes() == want_sine.tobytes() and got[1] is None and got[2] is None
    # the device read, and the stage times
    dp = torch.empty(n * 26, dtype=torch.int32, device="cuda:0")                    # records of 104 bytes
    R._check(binding.lib().exa_hip_critical_points_read(R.h, binding._dev_ptr(dp), None, None, 1, None))
    assert dp.cpu().numpy().tobytes() == want_sine.tobytes()
    ms = R.criticalPointsStageMs()
    assert len(ms) == 6 and all(m >= 0 for m in ms) and ms[0] > 0 and ms[1] > 0 and ms[3] > 0 and ms[4] > 0 and ms[5] == 0
    # probe arrays of an extraction without the probe are refused
    buf = np.zeros(12 * n, np.float32)
    assert binding.lib().exa_hip_critical_points_read(R.h, None, buf.ctypes.data, None, 0, None) != 0
    assert "EXA_CRITICAL_PROBE" in binding.lib().exa_hip_last_error(R.h).decode()
    # a second extraction replaces the first
    n2, _ = R.extractCriticalPoints(lo, hi, dims, channels=FLOW, probe=True)
    got = R.readCriticalPoints()
    assert n2 == 1 and got[0].tobytes() == want_flow.tobytes() and got[1].shape == (1, 3, 4)
    assert R.criticalPointsStageMs()[5] > 0
    R.releaseCriticalPoints()
    with pytest.raises(RuntimeError, match="exa_hip_critical_points_read"):
        R.readCriticalPoints()


def _raw(R, lo=(0, 0, 0), hi=(48, 48, 32), dims=(9, 10, 11), channels=SINE, iterations=8, tolerance=2.0 ** -10, flags=0, null=None):
    lo3, hi3, d3, ch = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*dims), (C.c_int32 * 3)(*channels)
    lo3, hi3, d3, ch = (None if null == "lo" else lo3), (None if null == "hi" else hi3), (None if null == "dims" else d3), \
        (None if null == "channels" else ch)
    n, st = C.c_uint64(77), (C.c_uint64 * 7)(*([77] * 7))
    L = binding.lib()
    rc = L.exa_hip_critical_points(R.h, lo3, hi3, d3, ch, iterations, tolerance, flags, C.byref(n), st, None)
    return rc, int(n.value), [int(v) for v in st], L.exa_hip_last_error(R.h).decode()


def test_no_point_and_refused_arguments():
    case = Case(_with_fields(scenes.amr(levels=3, fields=1), _linear(DEFAULT, CENTRE) + _sine()), W=32, H=32)
    R = case.hip_renderer()                                    # no render yet: the module holds no frame state
    L = binding.lib()
    buf = np.zeros(1024 * 26, np.int32)
    assert L.exa_hip_critical_points_read(R.h, buf.ctypes.data, None, None, 0, None) != 0       # before any extraction
    assert L.exa_hip_last_error(R.h).decode().startswith("exa_hip_critical_points_read: ")
    rc, n, st, msg = _raw(R, flags=binding.SAMPLE_WORLD_SPACE)
    assert rc != 0 and msg.startswith("exa_hip_critical_points: ") and "frame state" in msg, msg
    frame = R.render()
    rc, n, st, _ = _raw(R, channels=(0, 0, 0))                 # the scene's own field, three times: no point, and no error
    assert rc == 0 and n == 0 and st[0] == 8 * 9 * 10 and st[3] == 0
    assert L.exa_hip_critical_points_read(R.h, buf.ctypes.data, None, None, 0, None) == 0
    want = R.criticalPoints((0, 0, 0), (48, 48, 32), (9, 10, 11), channels=SINE)[0]
    assert len(want) > 100
    nf = len(case.scene.fields)
    bad = [dict(null="lo"), dict(null="hi"), dict(null="dims"), dict(null="channels"),
           dict(lo=(math.nan, 0, 0)), dict(hi=(48, math.inf, 32)), dict(lo=(48, 0, 0)), dict(dims=(0, 9, 9)), dict(dims=(9, 9, -1)),
           dict(dims=(1, 9, 9)), dict(dims=(9, 1, 9)), dict(dims=(9, 9, 1)),
           dict(dims=(2 ** 11, 2 ** 11, 2 ** 9)), dict(dims=(2 ** 16, 2 ** 16, 2 ** 16)), dict(channels=(1, 2, nf)), dict(channels=(-1, 2, 3)),
           dict(iterations=0), dict(iterations=-3), dict(iterations=33), dict(tolerance=0.0), dict(tolerance=-0.5), dict(tolerance=1.5),
           dict(tolerance=math.nan), dict(tolerance=math.inf), dict(flags=2), dict(flags=4), dict(flags=8), dict(flags=32),
           dict(flags=1 << 30)]
    for kw in bad:
        rc, n, st, msg = _raw(R, **kw)
        assert rc != 0 and n == 0 and st == [0] * 7 and msg.startswith("exa_hip_critical_points: "), (kw, rc, msg)
        assert L.exa_hip_critical_points_read(R.h, buf.ctypes.data, None, None, 0, None) != 0, kw      # a failed call drops the result
        rc, n, st, _ = _raw(R)                                                                          # and the handle still works
        assert rc == 0 and n == len(want) and st[3] == n, kw
        assert L.exa_hip_critical_points_read(R.h, buf.ctypes.data, None, None, 0, None) == 0
        assert buf[:26 * n].tobytes() == want.tobytes(), kw
    rc, n, st, _ = _raw(R, flags=binding.SAMPLE_WORLD_SPACE | binding.CRITICAL_PROBE)                   # every flag
    assert rc == 0
    assert R.render().shape == frame.shape
    R.close()


def test_scene_without_kd_tree_is_refused():
    R = without_kd_tree(Case(scenes.amr(levels=3, fields=3), W=32, H=32)).hip_renderer()
    rc, n, st, msg = _raw(R, channels=(0, 1, 2))
    assert rc != 0 and n == 0 and msg.startswith("exa_hip_critical_points: ") and "kd-tree" in msg, msg
    assert R.render().shape == (32, 32)                        # the handle still renders (through its LBVH)
    R.close()
