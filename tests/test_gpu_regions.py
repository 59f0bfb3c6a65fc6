"""Connected regions on the GPU (exa_hip_regions, include/exa_hip.h): the labels, the whole table and the sum's exponent
equal the numpy restatement of the contract (tests/regions_ref.py) byte for byte when that is fed the lattice exa_hip_resample
returns — on the scenes of the iso-surface test with both neighbourhoods and both senses of inside, on lattice shapes that
trip indexing mistakes, on constructed fields (a path whose diameter is its length, a comb, a checkerboard, a ball in a
shell), across more than one scan chunk, for a derived quantity and in world space; nothing a frame or a tuning knob sets
changes a byte; the mesh, the lines and the regions coexist; bad arguments are refused with a message and leave the handle
usable.  The failed allocation has no test."""
import ctypes as C
import math

import numpy as np
import pytest

import regions_ref as ref
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from test_gpu_isomesh import CASES, DIMS, XFM, _isos, _root_box
from test_regions_ref import boustrophedon, checkerboard

pytestmark = pytest.mark.gpu

NAN = float("nan")
FLAGS = [(False, False), (False, True), (True, False), (True, True)]        # (below, faces)


def test_the_binding_s_record_is_the_restatement_s():
    assert binding.LABELLED_REGION_DTYPE == ref.REGION and binding.LABELLED_REGION_DTYPE.itemsize == 88


def _same(got, want, what):
    labels, table, s = want
    assert got["sum_exponent"] == s, (what, got["sum_exponent"], s)
    assert got["labels"].dtype == np.int32 and got["labels"].shape == labels.shape, what
    assert len(got["regions"]) == len(table), (what, len(got["regions"]), len(table))
    assert got["labels"].tobytes() == labels.tobytes(), (what, np.argwhere(got["labels"] != labels)[:5])
    for name in ref.REGION.names:
        assert got["regions"][name].tobytes() == table[name].tobytes(), (what, name)
    assert got["regions"].tobytes() == table.tobytes(), what                   # the padding too
    assert got["num_inside"] == int((labels >= 0).sum()), what


def _compare(R, V, lo, hi, dims, iso, what, flags=FLAGS, wants=None, **kw):
    """every flag combination against the restatement on the lattice V (wants: its results where the caller has them); the
    restatement's results by (below, faces)"""
    out = {}
    for below, faces in flags:
        want = wants[below, faces] if wants else ref.regions(V, iso, below=below, faces=faces)
        got = R.regions(lo, hi, dims, iso, below=below, faces=faces, **kw) if "quantity" not in kw else \
            R.regionsDerived(lo, hi, dims, iso, below=below, faces=faces, **kw)
        print(f"{what} below {below} faces {faces}: regions {len(want[1])} inside {got['num_inside']} exponent {want[2]}")
        _same(got, want, (what, below, faces))
        out[below, faces] = want
    return out


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{c[0]}-f{c[2]}" for c in CASES])
def test_regions_equal_the_restatement_byte_for_byte(idx):
    name, make, form, empty, _ = CASES[idx]
    case = Case(make(), basis_form=form, allow_empty_cells=empty)
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    channel = len(case.scene.fields) - 1
    V = R.resample(lo, hi, DIMS, channel=channel, fill=NAN)
    assert np.isnan(V).any()                                        # the box is grown: points outside the volume
    for label, iso in _isos(V):
        for below in (False, True):
            n = int(ref.inside(V, iso, below).sum())
            # ex0 is a single cell, its reconstruction one value up to rounding: nothing need lie below a level taken from it
            assert 0 < n < V.size or (name == "ex0" and below and n == 0), (name, label, below, n)
        _compare(R, V, lo, hi, DIMS, iso, f"{name} form {form} {label} iso {iso!r}", channel=channel)
    R.close()


@pytest.fixture(scope="module")
def amr3():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    yield case, R
    R.close()


@pytest.mark.parametrize("dims", [(1, 1, 1), (65, 1, 1), (1, 1, 65), (64, 3, 1), (257, 2, 2), (3, 3, 300), (63, 65, 5)],
                         ids=lambda d: "x".join(map(str, d)))
def test_lattice_shapes(amr3, dims):
    case, R = amr3
    lo, hi = R.prep.voxel_bounds()
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    V = R.resample(lo, hi, dims, channel=1, fill=NAN)
    assert V.shape == dims[::-1] and np.isfinite(V).any()
    iso = float(np.median(V[np.isfinite(V)]))
    n = int(ref.inside(V, iso).sum())
    assert 0 < n and (n < V.size or V.size == 1)
    _compare(R, V, lo, hi, dims, iso, f"amr3 {dims}", channel=1)


# ---- constructed fields on the 64^3 cells of one level: the lattice is the cell centres, the values are +-1 ----
N = 64


def _comb():
    """a spine along x at y = 0, z = 0 and a tooth along y from every second point of it, on every fourth slice; the slices'
    combs are joined along z at the origin"""
    A = np.full((N, N, N), -1.0, np.float32)
    for k in range(0, N, 4):
        A[k, 0, :] = 1.0
        A[k, :, 0::2] = 1.0
    A[:, 0, 0] = 1.0
    return A


def _ball_in_shell():
    k, j, i = np.meshgrid(*(np.arange(N) + 0.5,) * 3, indexing="ij")
    rad = np.sqrt((i - 32.0) ** 2 + (j - 32.0) ** 2 + (k - 32.0) ** 2)
    return np.where((rad < 8.0) | ((rad > 16.0) & (rad < 24.0)), 1.0, -1.0).astype(np.float32)


FIELDS = dict(path=lambda: boustrophedon(N, N, N)[0], comb=_comb, checkerboard=lambda: checkerboard((N, N, N)),
              ball_in_shell=_ball_in_shell)


def _constructed(A):
    scene = scenes.with_extra_field(scenes.example("c1_64"),
                                    lambda c: A[c[:, 2].astype(np.int64), c[:, 1].astype(np.int64), c[:, 0].astype(np.int64)])
    R = Case(scene).hip_renderer()
    assert np.array_equal(R.prep.voxel_bounds()[0], [0, 0, 0]) and np.array_equal(R.prep.voxel_bounds()[1], [N, N, N])
    return R


@pytest.mark.parametrize("name", list(FIELDS))
def test_constructed_fields(name):
    A = FIELDS[name]()
    R = _constructed(A)
    lo, hi, dims = (0.0, 0.0, 0.0), (float(N),) * 3, (N, N, N)
    V = R.resample(lo, hi, dims, channel=1, fill=NAN)
    assert np.array_equal(V > 0, A > 0) and np.isfinite(V).all()      # the structure survives the reconstruction
    flags = FLAGS if name == "ball_in_shell" else [(False, False), (False, True)]
    want = {f: ref.regions(V, 0.0, below=f[0], faces=f[1]) for f in flags}     # the structure, on the restatement alone
    kuhn, faces = want[False, False][1], want[False, True][1]
    if name == "path":
        for t in (kuhn, faces):
            assert len(t) == 1 and t["points"][0] == (A > 0).sum() > 60000 and t["first"][0] == 0
    elif name == "comb":
        for t in (kuhn, faces):
            assert len(t) == 1 and t["points"][0] == (A > 0).sum() and np.array_equal(t["hi"][0], [N - 1, N - 1, N - 1])
    elif name == "checkerboard":
        assert len(faces) == 131072 and np.all(faces["points"] == 1) and np.array_equal(faces["first"], np.nonzero(A.reshape(-1) > 0)[0])
        assert len(kuhn) < len(faces)
    else:
        for key in FLAGS:                                             # the ball and the shell; the gap and the outside
            t = want[key][1]
            assert len(t) == 2 and np.all(np.diff(t["first"].astype(np.int64)) > 0), (key, len(t))
        assert kuhn["points"][0] > kuhn["points"][1]                  # the shell comes first in L, and is the larger one
        outside = want[True, False][1]
        assert outside["first"][0] == 0 and outside["points"][0] > outside["points"][1]
    _compare(R, V, lo, hi, dims, 0.0, name, flags=flags, wants=want, channel=1)
    R.close()


def test_more_than_one_scan_chunk():
    R = _constructed(checkerboard((N, N, N)))
    lo, hi, dims = (0.0, 0.0, 0.0), (float(N),) * 3, (96, 96, 64)      # 589 824 points; a chunk is 2048 * 256
    V = R.resample(lo, hi, dims, channel=1, fill=NAN)
    assert V.size > 2048 * 256
    # between the cell centres the reconstruction passes through 0: a level above it leaves islands around the centres of the
    # +1 cells, which the faces keep apart
    iso = 0.2
    want = {f: ref.regions(V, iso, faces=f[1]) for f in [(False, False), (False, True)]}
    first = want[False, True][1]["first"]
    assert len(first) > 10000 and (first < 2048 * 256).sum() > 1000 and (first >= 2048 * 256).sum() > 1000
    assert len(want[False, False][1]) >= 1
    _compare(R, V, lo, hi, dims, iso, "checkerboard 96x96x64", flags=list(want), wants=want, channel=1)
    R.close()


def test_derived_regions_of_q(amr3):
    case, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resampleDerived(lo, hi, DIMS, "q", channels=(0, 1, 2), fill=NAN)
    assert np.isnan(V).any() and 0 < ref.inside(V, 0.0).sum() < V.size
    want = _compare(R, V, lo, hi, DIMS, 0.0, "amr3 Q", quantity="q", channels=(0, 1, 2))
    assert len(want[False, False][1]) > 1


def test_regions_in_world_space():
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lo, hi = np.array([-4, -6, -5], np.float32), np.array([30, 24, 26], np.float32)
    dims = (41, 33, 27)
    V = R.resample(lo, hi, dims, channel=1, world=True, fill=NAN)
    iso = _isos(V)[0][1]
    assert np.isnan(V).any() and 0 < ref.inside(V, iso).sum() < V.size
    _compare(R, V, lo, hi, dims, iso, "amr3 world", channel=1, world=True)
    assert not np.array_equal(np.isnan(R.resample(lo, hi, dims, channel=1, fill=NAN)), np.isnan(V))
    R.close()


def _bytes(got):
    return [got["labels"].tobytes(), got["regions"].tobytes(), got["values"].tobytes(), got["sum_exponent"], got["num_inside"]]


def test_regions_do_not_depend_on_frame_state_or_options(amr3):
    case, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    call = lambda H: _bytes(H.regions(lo, hi, DIMS, iso, channel=1, keep_values=True))        # noqa: E731
    want = call(R)
    assert len(want[1]) > 88 and want[2] == V.tobytes()
    assert call(R) == want, "two consecutive calls"
    M = multi_handle(R)
    assert call(M) == want, "a multi-device handle"
    M.close()
    for what in frame_perturbations(case, R):
        assert call(R) == want, what
    for patch in range(4):
        R.setOption("sample_patch", patch)
        assert call(R) == want, f"sample_patch {patch}"
    R.setOption("sample_uniform", 0)
    assert call(R) == want, "sample_uniform 0"
    R.setOption("sample_uniform", 1)
    R.setOption("sample_patch", 0)


def test_mesh_lines_and_regions_do_not_drop_each_other():
    import torch
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    plane, size = ((float(lo[0]), float(lo[1]), 0.5 * float(lo[2] + hi[2])), (float(hi[0] - lo[0]) / 64, 0.0, 0.0),
                   (0.0, float(hi[1] - lo[1]) / 9, 0.0)), (64, 9)
    want_regions = R.regions(lo, hi, DIMS, iso, channel=1)
    want_mesh = R.isosurface(lo, hi, (19, 17, 13), iso, channel=1)
    want_lines = R.isolines(*plane, size, [iso], channel=1)
    assert len(want_mesh[1]) > 0 and len(want_lines["segments"]) > 0 and len(want_regions["regions"]) > 0
    R.extractIsoSurface(lo, hi, (19, 17, 13), iso, channel=1)
    R.extractIsolines(*plane, size, [iso], channel=1)
    nr, ni, s = R.extractRegions(lo, hi, DIMS, iso, channel=1)
    mesh, lines = R.readIsoSurface(), R.readIsolines()                 # extracted before the regions: still there
    assert mesh[0].tobytes() == want_mesh[0].tobytes() and mesh[1].tobytes() == want_mesh[1].tobytes()
    assert all(lines[k].tobytes() == want_lines[k].tobytes() for k in want_lines)
    R.extractIsoSurface(lo, hi, (9, 9, 9), iso, channel=1)
    R.extractIsolines(*plane, (8, 8), [iso], channel=1)
    R.releaseIsoSurface()
    R.releaseIsolines()
    got = R.readRegions()                                              # behind a later mesh, later lines and their release
    assert got["labels"].tobytes() == want_regions["labels"].tobytes() and got["regions"].tobytes() == want_regions["regions"].tobytes()
    # the device read, and the stage times
    dl = torch.empty(DIMS[::-1], dtype=torch.int32, device="cuda:0")
    dr = torch.empty(nr * 22, dtype=torch.int32, device="cuda:0")                   # records of 88 bytes
    R._check(binding.lib().exa_hip_regions_read(R.h, binding._dev_ptr(dl), binding._dev_ptr(dr), None, 1, None))
    assert dl.cpu().numpy().tobytes() == got["labels"].tobytes() and dr.cpu().numpy().tobytes() == got["regions"].tobytes()
    ms = R.regionsStageMs()
    assert len(ms) == 6 and all(m >= 0 for m in ms) and ms[0] > 0 and ms[2] > 0 and ms[5] > 0
    m = binding.region_measures(got["regions"], got["sum_exponent"], lo, hi, DIMS)
    flat, lab = V.reshape(-1).astype(np.float64), got["labels"].reshape(-1)
    big = int(np.argmax(got["regions"]["points"]))
    assert abs(m["sum"][big] - flat[lab == big].sum()) <= 1e-6 * np.abs(flat[lab == big]).sum()
    assert np.all(m["centroid"][big] > lo) and np.all(m["centroid"][big] < hi) and m["volume"][big] > 0
    R.releaseRegions()
    with pytest.raises(RuntimeError, match="exa_hip_regions_read"):
        R.readRegions()
    R.close()


def _raw(R, lo=(0, 0, 0), hi=(8, 8, 8), dims=(9, 9, 9), channel=0, iso=0.5, flags=0, quantity=None, null=None):
    lo3, hi3, d3 = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*dims)
    lo3, hi3, d3 = (None if null == "lo" else lo3), (None if null == "hi" else hi3), (None if null == "dims" else d3)
    nr, ni, se = C.c_uint64(77), C.c_uint64(77), C.c_int32(77)
    L = binding.lib()
    if quantity is None:
        rc = L.exa_hip_regions(R.h, lo3, hi3, d3, channel, iso, flags, C.byref(nr), C.byref(ni), C.byref(se), None)
    else:
        ch = (C.c_int32 * 3)(*channel) if null != "channels" else None
        rc = L.exa_hip_regions_derived(R.h, lo3, hi3, d3, ch, quantity, iso, flags, C.byref(nr), C.byref(ni), C.byref(se), None)
    return rc, (int(nr.value), int(ni.value), int(se.value)), L.exa_hip_last_error(R.h).decode()


def test_no_region_and_refused_arguments():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()                                    # no render yet: the module holds no frame state
    L = binding.lib()
    buf = np.zeros(1024, np.int32)
    assert L.exa_hip_regions_read(R.h, buf.ctypes.data, None, None, 0, None) != 0       # before any extraction
    assert L.exa_hip_last_error(R.h).decode().startswith("exa_hip_regions_read: ")
    rc, counts, msg = _raw(R, flags=binding.SAMPLE_WORLD_SPACE)
    assert rc != 0 and msg.startswith("exa_hip_regions: ") and "frame state" in msg, msg
    frame = R.render()
    V0 = R.resample((0, 0, 0), (8, 8, 8), (9, 9, 9), fill=NAN)  # _raw's lattice
    top, mid = float(np.nanmax(V0)), float(np.median(V0[np.isfinite(V0)]))
    rc, counts, _ = _raw(R, iso=top + 1.0)                     # above the maximum: no region, and no error
    assert (rc, counts) == (0, (0, 0, 0))
    assert L.exa_hip_regions_read(R.h, buf.ctypes.data, None, None, 0, None) == 0 and np.all(buf[:729] == -1)
    rc, counts, _ = _raw(R, iso=mid)
    assert rc == 0 and counts[0] > 0 and counts[1] >= counts[0]
    nf = len(case.scene.fields)
    bad = [dict(null="lo"), dict(null="hi"), dict(null="dims"), dict(iso=math.nan), dict(iso=math.inf), dict(iso=-math.inf),
           dict(lo=(math.nan, 0, 0)), dict(hi=(8, math.inf, 8)), dict(dims=(0, 9, 9)), dict(dims=(9, 9, -1)),
           dict(dims=(2 ** 11, 2 ** 11, 2 ** 9)), dict(dims=(2 ** 16, 2 ** 16, 2 ** 16)), dict(channel=nf), dict(channel=-1),
           dict(flags=2), dict(flags=4), dict(flags=8), dict(flags=128), dict(flags=1 << 30)]
    for kw in bad:
        rc, counts, msg = _raw(R, **kw)
        assert rc != 0 and counts == (0, 0, 0) and msg.startswith("exa_hip_regions: "), (kw, rc, msg)
        assert L.exa_hip_regions_read(R.h, buf.ctypes.data, None, None, 0, None) != 0, kw      # a failed call drops the result
        rc, counts, _ = _raw(R, iso=mid)                                                 # and the handle still works
        assert rc == 0 and counts[0] > 0, kw
    bad = [dict(quantity=-1), dict(quantity=binding.DERIVED["vorticity"]), dict(quantity=99), dict(channel=(0, 1, nf)),
           dict(null="channels"), dict(null="dims"), dict(iso=math.nan), dict(dims=(9, 0, 9)), dict(flags=2), dict(flags=256)]
    for kw in bad:
        kw = dict(dict(quantity=binding.DERIVED["q"], channel=(0, 1, 2)), **kw)
        rc, counts, msg = _raw(R, **kw)
        assert rc != 0 and counts == (0, 0, 0) and msg.startswith("exa_hip_regions_derived: "), (kw, rc, msg)
    # the next valid calls succeed, with every flag
    every = binding.SAMPLE_WORLD_SPACE | binding.REGIONS_BELOW | binding.REGIONS_FACES
    rc, counts, _ = _raw(R, iso=mid, flags=every)
    assert rc == 0
    vals = np.zeros(729, np.float32)
    assert L.exa_hip_regions_read(R.h, None, None, vals.ctypes.data, 0, None) != 0             # values it did not keep
    assert "EXA_REGIONS_KEEP_VALUES" in L.exa_hip_last_error(R.h).decode()
    rc, counts, _ = _raw(R, quantity=binding.DERIVED["q"], channel=(0, 1, 2), iso=0.0, flags=binding.REGIONS_KEEP_VALUES)
    assert rc == 0
    assert L.exa_hip_regions_read(R.h, None, None, vals.ctypes.data, 0, None) == 0
    assert vals.tobytes() == R.resampleDerived((0, 0, 0), (8, 8, 8), (9, 9, 9), "q", fill=NAN).tobytes()
    assert R.render().shape == frame.shape
    R.close()


def test_scene_without_kd_tree_is_refused():
    R = without_kd_tree(Case(scenes.amr(levels=3), W=32, H=32)).hip_renderer()
    rc, counts, msg = _raw(R)
    assert rc != 0 and counts == (0, 0, 0) and msg.startswith("exa_hip_regions: ") and "kd-tree" in msg, msg
    assert R.render().shape == (32, 32)                        # the handle still renders (through its LBVH)
    R.close()
