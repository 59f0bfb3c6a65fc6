"""Basins on the GPU (exa_hip_basins, include/exa_hip.h): the labels, the whole table and the five scalars equal the numpy
restatement of the contract (tests/basins_ref.py) byte for byte when that is fed the lattice exa_hip_resample returns — on the
scenes of the iso-surface test with both neighbourhoods, both senses of inside and three depths, on lattice shapes that trip
indexing mistakes, on constructed fields (an egg carton, pure plateaus, a ridge whose chain of up links is its length),
across more than one scan chunk, for a derived quantity and in world space; with an infinite depth the basins are the regions
of exa_hip_regions; nothing a frame or a tuning knob sets changes a byte; the mesh, the lines, the regions and the basins
coexist; bad arguments are refused with a message and leave the handle usable.  The failed allocation has no test."""
import ctypes as C
import math

import numpy as np
import pytest

import basins_ref as ref
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from test_gpu_isomesh import CASES, DIMS, XFM, _isos, _root_box
from test_gpu_regions import N, _ball_in_shell, _constructed
from test_regions_ref import boustrophedon, checkerboard

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
FLAGS = [(False, False), (False, True), (True, False), (True, True)]        # (below, faces)


def test_the_binding_s_record_is_the_restatement_s():
    assert binding.BASIN_DTYPE == ref.BASIN and binding.BASIN_DTYPE.itemsize == 96


def _same(got, want, what):
    labels, table, s, raw, rounds = want
    assert (got["sum_exponent"], got["num_raw"], got["rounds"]) == (s, raw, rounds), (what, got["sum_exponent"], got["num_raw"], got["rounds"], want[2:])
    assert got["labels"].dtype == np.int32 and got["labels"].shape == labels.shape, what
    assert len(got["basins"]) == len(table), (what, len(got["basins"]), len(table))
    assert got["labels"].tobytes() == labels.tobytes(), (what, np.argwhere(got["labels"] != labels)[:5])
    for name in ref.BASIN.names:
        assert got["basins"][name].tobytes() == table[name].tobytes(), (what, name)
    assert got["basins"].tobytes() == table.tobytes(), what
    assert got["regions"] is got["basins"] and got["num_inside"] == int((labels >= 0).sum()), what


def _middle(V, iso, below, faces):
    """the restatement without merging, and the median of the finite depths of its table (None: there is none)"""
    zero = ref.basins(V, iso, 0.0, below=below, faces=faces)
    depth = zero[1]["depth"]
    fin = depth[np.isfinite(depth)]
    return zero, (float(np.median(fin)) if fin.size else None)


def _compare(R, V, lo, hi, dims, iso, what, flags=FLAGS, depths=(0.0, "middle", INF), merging=False, **kw):
    """every flag combination and depth against the restatement on the lattice V; merging: the inputs are meant to merge
    something at the middle depth and at the infinite one.  The restatement's results by (below, faces, depth)."""
    out = {}
    for below, faces in flags:
        zero, mid = _middle(V, iso, below, faces)
        for depth in depths:
            d = mid if depth == "middle" else depth
            if d is None:
                continue
            want = zero if d == 0.0 else ref.basins(V, iso, d, below=below, faces=faces)
            nb, raw, rounds = len(want[1]), want[3], want[4]
            print(f"{what} below {below} faces {faces} minDepth {d!r}: raw {raw} basins {nb} rounds {rounds}")
            assert rounds <= 64, (what, below, faces, d, rounds)
            assert (rounds == 0) == (nb == raw) and (d > 0 or rounds == 0)
            if merging and d > 0:
                assert 0 < nb < raw, (what, below, faces, d, nb, raw)
            got = R.basins(lo, hi, dims, iso, d, below=below, faces=faces, **kw) if "quantity" not in kw else \
                R.basinsDerived(lo, hi, dims, iso, d, below=below, faces=faces, **kw)
            _same(got, want, (what, below, faces, d))
            out[below, faces, depth] = want
    return out


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{c[0]}-f{c[2]}" for c in CASES])
def test_basins_equal_the_restatement_byte_for_byte(idx):
    name, make, form, empty, _ = CASES[idx]
    case = Case(make(), basis_form=form, allow_empty_cells=empty)
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    channel = len(case.scene.fields) - 1
    V = R.resample(lo, hi, DIMS, channel=channel, fill=NAN)
    assert np.isnan(V).any()                                        # the box is grown: points outside the volume
    for label, iso in _isos(V):
        # the fields of the generated scenes have many peaks on either side of their median; the examples are a few cells
        _compare(R, V, lo, hi, DIMS, iso, f"{name} form {form} {label} iso {iso!r}",
                 merging=label == "median" and name in ("amr3", "gen", "amr3_holes"), channel=channel)
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


# ---- constructed fields on the 64^3 cells of one level: the lattice is the cell centres ----
BUMPS = 256


def _egg_carton():
    """sin * sin * sin with eight half periods per axis, the phase such that every lobe has one greatest lattice point:
    256 positive bumps (and 256 negative ones)"""
    f = np.sin(np.pi * (np.arange(N) + 0.75) / 8.0)
    return (f[:, None, None] * f[None, :, None] * f[None, None, :]).astype(np.float32)


def _ridge():
    """the boustrophedon path, rising from 1 to 2 along its length, in a plain of -1; and the path's length"""
    A, length = boustrophedon(N, N, N)
    # the position along the path, row by row in the order boustrophedon lays them: a row runs towards the end its joint is at
    pos = np.full(A.shape, -1, np.int64)
    at = row = 0
    for k in range(0, N, 2):
        js = list(range(0, N, 2))
        if (k // 2) % 2:
            js.reverse()
        for n, j in enumerate(js):
            end = N - 1 if row % 2 == 0 else 0
            pos[k, j, :] = at + (np.arange(N) if end else np.arange(N)[::-1])
            at += N
            if n + 1 < len(js):
                pos[k, (j + js[n + 1]) // 2, end] = at
                at += 1
            elif k + 2 < N:
                pos[k + 1, j, end] = at
                at += 1
            row += 1
    assert at == length and np.array_equal(pos >= 0, A > 0)
    return np.where(pos >= 0, 1.0 + pos / float(length), -1.0).astype(np.float32), length


FIELDS = dict(egg_carton=_egg_carton, checkerboard=lambda: checkerboard((N, N, N)), ball_in_shell=_ball_in_shell,
              ridge=lambda: _ridge()[0])


@pytest.mark.parametrize("name", list(FIELDS))
def test_constructed_fields(name):
    A = FIELDS[name]()
    R = _constructed(A)
    lo, hi, dims = (0.0, 0.0, 0.0), (float(N),) * 3, (N, N, N)
    V = R.resample(lo, hi, dims, channel=1, fill=NAN)
    assert np.array_equal(V > 0, A > 0) and np.isfinite(V).all()      # the structure survives the reconstruction
    if name == "egg_carton":
        for faces in (False, True):
            zero = ref.basins(V, 0.0, 0.0, faces=faces)
            assert zero[3] == len(zero[1]) == BUMPS, (faces, zero[3])             # one peak per bump
        assert len(ref.basins(V, 0.0, INF, faces=True)[1]) == BUMPS               # the axis edges keep the bumps apart
        assert len(ref.basins(V, 0.0, INF)[1]) < BUMPS                            # the Kuhn diagonals join them
        assert len(ref.basins(V, 0.0, 0.0, below=True)[1]) == BUMPS
        _compare(R, V, lo, hi, dims, 0.0, name, flags=[(False, False), (False, True), (True, False)], channel=1)
    elif name == "ridge":
        for faces in (False, True):
            chain = ref.longest_chain(V, 0.0, faces=faces)
            print(f"ridge faces {faces}: longest chain of up links {chain}")
            assert chain > 1024, chain
            assert ref.basins(V, 0.0, 0.0, faces=faces)[3] == 1                  # one peak, at the end of the path
        _compare(R, V, lo, hi, dims, 0.0, name, flags=[(False, False), (False, True)], depths=(0.0, INF), channel=1)
    else:
        # pure plateaus: many raw basins of depth 0, and any positive depth gives the regions' partition
        flags = FLAGS if name == "ball_in_shell" else [(False, False), (False, True)]
        tiny = float(np.finfo(np.float32).tiny)
        got = _compare(R, V, lo, hi, dims, 0.0, name, flags=flags, depths=(0.0, tiny, INF), channel=1)
        for below, faces in flags:
            regions = R.regions(lo, hi, dims, 0.0, channel=1, below=below, faces=faces)
            zero, small, all_ = (got[below, faces, d] for d in (0.0, tiny, INF))
            if not (name == "checkerboard" and faces):                            # there every point is a region of its own
                assert zero[3] > len(regions["regions"]), (name, below, faces, zero[3])
            finite = zero[1]["depth"][zero[1]["neighbour"] >= 0]
            assert np.all(finite == 0.0)
            for want in (small, all_):
                assert len(want[1]) == len(regions["regions"]) and ref.same_partition(want[0], regions["labels"]), (name, below, faces)
    R.close()


def test_more_than_one_scan_chunk():
    R = _constructed(checkerboard((N, N, N)))
    lo, hi, dims = (0.0, 0.0, 0.0), (float(N),) * 3, (96, 96, 64)      # 589 824 points; a chunk is 2048 * 256
    V = R.resample(lo, hi, dims, channel=1, fill=NAN)
    assert V.size > 2048 * 256
    iso = 0.2                                                          # islands around the centres of the +1 cells
    want = _compare(R, V, lo, hi, dims, iso, "checkerboard 96x96x64", flags=[(False, False), (False, True)], channel=1)
    peaks = want[False, True, 0.0][1]["argMax"]
    assert len(peaks) > 10000 and (peaks < 2048 * 256).sum() > 1000 and (peaks >= 2048 * 256).sum() > 1000
    R.close()


def test_derived_basins_of_q(amr3):
    case, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resampleDerived(lo, hi, DIMS, "q", channels=(0, 1, 2), fill=NAN)
    assert np.isnan(V).any() and 0 < ref.inside(V, 0.0).sum() < V.size
    _compare(R, V, lo, hi, DIMS, 0.0, "amr3 Q", merging=True, quantity="q", channels=(0, 1, 2))


def test_basins_in_world_space():
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lo, hi = np.array([-4, -6, -5], np.float32), np.array([30, 24, 26], np.float32)
    dims = (41, 33, 27)
    V = R.resample(lo, hi, dims, channel=1, world=True, fill=NAN)
    iso = _isos(V)[0][1]
    assert np.isnan(V).any() and 0 < ref.inside(V, iso).sum() < V.size
    _compare(R, V, lo, hi, dims, iso, "amr3 world", flags=[(False, False), (True, True)], merging=True, channel=1, world=True)
    R.close()


def test_with_an_infinite_depth_the_basins_are_the_regions(amr3):
    case, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    for below, faces in FLAGS:
        regions = R.regions(lo, hi, DIMS, iso, channel=1, below=below, faces=faces)
        basins = R.basins(lo, hi, DIMS, iso, INF, channel=1, below=below, faces=faces)
        assert len(basins["basins"]) == len(regions["regions"]) > 0 and basins["num_raw"] > len(regions["regions"])
        assert ref.same_partition(basins["labels"], regions["labels"])
        assert np.all(basins["basins"]["neighbour"] == -1) and basins["num_inside"] == regions["num_inside"]
        order = np.argsort(basins["basins"]["first"])
        for field in ("points", "sumFixed", "sumIndex", "lo", "hi", "first", "argMin", "argMax", "min", "max"):
            assert basins["basins"][field][order].tobytes() == regions["regions"][field].tobytes(), field


def _bytes(got):
    return [got["labels"].tobytes(), got["basins"].tobytes(), got["values"].tobytes(), got["sum_exponent"], got["num_inside"],
            got["num_raw"], got["rounds"]]


def test_basins_do_not_depend_on_frame_state_or_options(amr3):
    case, R = amr3
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    mid = _middle(V, iso, False, False)[1]
    call = lambda H: _bytes(H.basins(lo, hi, DIMS, iso, mid, channel=1, keep_values=True))        # noqa: E731
    want = call(R)
    assert len(want[1]) > 96 and want[2] == V.tobytes() and want[6] > 0
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


def test_mesh_lines_regions_and_basins_do_not_drop_each_other():
    import torch
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    lo, hi = _root_box(R.prep)
    V = R.resample(lo, hi, DIMS, channel=1, fill=NAN)
    iso = _isos(V)[0][1]
    mid = _middle(V, iso, False, False)[1]
    plane, size = ((float(lo[0]), float(lo[1]), 0.5 * float(lo[2] + hi[2])), (float(hi[0] - lo[0]) / 64, 0.0, 0.0),
                   (0.0, float(hi[1] - lo[1]) / 9, 0.0)), (64, 9)
    want_basins = R.basins(lo, hi, DIMS, iso, mid, channel=1)
    want_regions = R.regions(lo, hi, DIMS, iso, channel=1)
    want_mesh = R.isosurface(lo, hi, (19, 17, 13), iso, channel=1)
    want_lines = R.isolines(*plane, size, [iso], channel=1)
    assert len(want_mesh[1]) > 0 and len(want_lines["segments"]) > 0 and len(want_regions["regions"]) > 0 and len(want_basins["basins"]) > 0
    R.extractIsoSurface(lo, hi, (19, 17, 13), iso, channel=1)
    R.extractIsolines(*plane, size, [iso], channel=1)
    R.extractRegions(lo, hi, DIMS, iso, channel=1)
    nb = R.extractBasins(lo, hi, DIMS, iso, mid, channel=1)[0]
    mesh, lines, regions = R.readIsoSurface(), R.readIsolines(), R.readRegions()       # extracted before the basins: still there
    assert mesh[0].tobytes() == want_mesh[0].tobytes() and mesh[1].tobytes() == want_mesh[1].tobytes()
    assert all(lines[k].tobytes() == want_lines[k].tobytes() for k in want_lines)
    assert regions["labels"].tobytes() == want_regions["labels"].tobytes() and regions["regions"].tobytes() == want_regions["regions"].tobytes()
    R.extractIsoSurface(lo, hi, (9, 9, 9), iso, channel=1)
    R.extractIsolines(*plane, (8, 8), [iso], channel=1)
    R.extractRegions(lo, hi, (9, 9, 9), iso, channel=1)
    R.releaseIsoSurface()
    R.releaseIsolines()
    R.releaseRegions()
    got = R.readBasins()                                   # behind a later mesh, later lines, later regions and their release
    assert got["labels"].tobytes() == want_basins["labels"].tobytes() and got["basins"].tobytes() == want_basins["basins"].tobytes()
    # the device read, and the stage times
    dl = torch.empty(DIMS[::-1], dtype=torch.int32, device="cuda:0")
    db = torch.empty(nb * 24, dtype=torch.int32, device="cuda:0")                      # records of 96 bytes
    R._check(binding.lib().exa_hip_basins_read(R.h, binding._dev_ptr(dl), binding._dev_ptr(db), None, 1, None))
    assert dl.cpu().numpy().tobytes() == got["labels"].tobytes() and db.cpu().numpy().tobytes() == got["basins"].tobytes()
    ms = R.basinsStageMs()
    assert len(ms) == 6 and all(m >= 0 for m in ms) and all(m > 0 for m in ms[:3]) and ms[5] > 0
    m = binding.region_measures(got["basins"], got["sum_exponent"], lo, hi, DIMS)
    flat, lab = V.reshape(-1).astype(np.float64), got["labels"].reshape(-1)
    big = int(np.argmax(got["basins"]["points"]))
    assert abs(m["sum"][big] - flat[lab == big].sum()) <= 1e-6 * np.abs(flat[lab == big]).sum()
    R.releaseBasins()
    with pytest.raises(RuntimeError, match="exa_hip_basins_read"):
        R.readBasins()
    R.close()


def _raw(R, lo=(0, 0, 0), hi=(8, 8, 8), dims=(9, 9, 9), channel=0, iso=0.5, depth=0.25, flags=0, quantity=None, null=None):
    lo3, hi3, d3 = (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), (C.c_int32 * 3)(*dims)
    lo3, hi3, d3 = (None if null == "lo" else lo3), (None if null == "hi" else hi3), (None if null == "dims" else d3)
    nb, nr, ni, se, rounds = C.c_uint64(77), C.c_uint64(77), C.c_uint64(77), C.c_int32(77), C.c_int32(77)
    outs = (C.byref(nb), C.byref(nr), C.byref(ni), C.byref(se), C.byref(rounds))
    L = binding.lib()
    if quantity is None:
        rc = L.exa_hip_basins(R.h, lo3, hi3, d3, channel, iso, depth, flags, *outs, None)
    else:
        ch = (C.c_int32 * 3)(*channel) if null != "channels" else None
        rc = L.exa_hip_basins_derived(R.h, lo3, hi3, d3, ch, quantity, iso, depth, flags, *outs, None)
    return rc, (int(nb.value), int(nr.value), int(ni.value), int(se.value), int(rounds.value)), L.exa_hip_last_error(R.h).decode()


def test_no_basin_and_refused_arguments():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()                                    # no render yet: the module holds no frame state
    L = binding.lib()
    none = (0, 0, 0, 0, 0)
    buf = np.zeros(1024, np.int32)
    assert L.exa_hip_basins_read(R.h, buf.ctypes.data, None, None, 0, None) != 0        # before any extraction
    assert L.exa_hip_last_error(R.h).decode().startswith("exa_hip_basins_read: ")
    rc, counts, msg = _raw(R, flags=binding.SAMPLE_WORLD_SPACE)
    assert rc != 0 and msg.startswith("exa_hip_basins: ") and "frame state" in msg, msg
    frame = R.render()
    V0 = R.resample((0, 0, 0), (8, 8, 8), (9, 9, 9), fill=NAN)  # _raw's lattice
    top, mid = float(np.nanmax(V0)), float(np.median(V0[np.isfinite(V0)]))
    rc, counts, _ = _raw(R, iso=top + 1.0)                     # above the maximum: no basin, and no error
    assert (rc, counts) == (0, none)
    assert L.exa_hip_basins_read(R.h, buf.ctypes.data, None, None, 0, None) == 0 and np.all(buf[:729] == -1)
    rc, counts, _ = _raw(R, iso=mid)
    assert rc == 0 and 0 < counts[0] <= counts[1] <= counts[2]
    rc, counts, _ = _raw(R, iso=mid, depth=INF)
    assert rc == 0 and 0 < counts[0] <= counts[1]
    nf = len(case.scene.fields)
    bad = [dict(null="lo"), dict(null="hi"), dict(null="dims"), dict(iso=math.nan), dict(iso=math.inf), dict(iso=-math.inf),
           dict(depth=math.nan), dict(depth=-1.0), dict(depth=-math.inf), dict(depth=-1e-30),
           dict(lo=(math.nan, 0, 0)), dict(hi=(8, math.inf, 8)), dict(dims=(0, 9, 9)), dict(dims=(9, 9, -1)),
           dict(dims=(2 ** 11, 2 ** 11, 2 ** 9)), dict(dims=(2 ** 16, 2 ** 16, 2 ** 16)), dict(channel=nf), dict(channel=-1),
           dict(flags=2), dict(flags=4), dict(flags=8), dict(flags=128), dict(flags=1 << 30)]
    for kw in bad:
        rc, counts, msg = _raw(R, **kw)
        assert rc != 0 and counts == none and msg.startswith("exa_hip_basins: "), (kw, rc, msg)
        assert L.exa_hip_basins_read(R.h, buf.ctypes.data, None, None, 0, None) != 0, kw       # a failed call drops the result
        rc, counts, _ = _raw(R, iso=mid)                                                 # and the handle still works
        assert rc == 0 and counts[0] > 0, kw
    bad = [dict(quantity=-1), dict(quantity=binding.DERIVED["vorticity"]), dict(quantity=99), dict(channel=(0, 1, nf)),
           dict(null="channels"), dict(null="dims"), dict(iso=math.nan), dict(depth=math.nan), dict(depth=-2.0), dict(dims=(9, 0, 9)),
           dict(flags=2), dict(flags=256)]
    for kw in bad:
        kw = dict(dict(quantity=binding.DERIVED["q"], channel=(0, 1, 2)), **kw)
        rc, counts, msg = _raw(R, **kw)
        assert rc != 0 and counts == none and msg.startswith("exa_hip_basins_derived: "), (kw, rc, msg)
    # the next valid calls succeed, with every flag
    every = binding.SAMPLE_WORLD_SPACE | binding.REGIONS_BELOW | binding.REGIONS_FACES
    rc, counts, _ = _raw(R, iso=mid, flags=every)
    assert rc == 0
    vals = np.zeros(729, np.float32)
    assert L.exa_hip_basins_read(R.h, None, None, vals.ctypes.data, 0, None) != 0              # values it did not keep
    assert "EXA_REGIONS_KEEP_VALUES" in L.exa_hip_last_error(R.h).decode()
    rc, counts, _ = _raw(R, quantity=binding.DERIVED["q"], channel=(0, 1, 2), iso=0.0, flags=binding.REGIONS_KEEP_VALUES)
    assert rc == 0
    assert L.exa_hip_basins_read(R.h, None, None, vals.ctypes.data, 0, None) == 0
    assert vals.tobytes() == R.resampleDerived((0, 0, 0), (8, 8, 8), (9, 9, 9), "q", fill=NAN).tobytes()
    assert R.render().shape == frame.shape
    R.close()


def test_scene_without_kd_tree_is_refused():
    R = without_kd_tree(Case(scenes.amr(levels=3), W=32, H=32)).hip_renderer()
    rc, counts, msg = _raw(R)
    assert rc != 0 and counts == (0, 0, 0, 0, 0) and msg.startswith("exa_hip_basins: ") and "kd-tree" in msg, msg
    assert R.render().shape == (32, 32)                        # the handle still renders (through its LBVH)
    R.close()
