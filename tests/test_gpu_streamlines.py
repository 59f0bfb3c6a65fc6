"""exa_hip_streamlines on the GPU (include/exa_hip.h): the packed polylines, velocities, offsets, seed indices and end reasons
equal the numpy restatement of the contract (tests/streamline_ref.py) bit for bit, in both basis forms and with empty cells; a
line through the seed is its backward line reversed plus its forward line; every vertex is a point the probes give a value
for; and nothing a frame sets, nor the batch a seed arrives in, changes a line."""
import ctypes as C

import numpy as np
import pytest

import streamline_ref as sr
from analysis_steps import bits as _bits, frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from probe_sets import domains, root_box

pytestmark = pytest.mark.gpu

STEP, MAX_STEPS, N_UNIFORM = 0.5, 40, 48


def _ex3():
    sc = scenes.example("ex3")
    return scenes.Scene(sc.bricks7, sc.cellIDs, [sc.fields[0]] * 3, name="ex3x3", value_range=sc.value_range, meta=dict(sc.meta))


# (name, make, channels, basis forms, allow_empty_cells)
CASES = [
    ("amr3", lambda: scenes.amr(levels=3, fields=3), (0, 1, 2), (0, 1), False),
    ("amr3_holes", lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=3), fraction=0.15), (0, 1, 2), (0,), True),
    ("zero", sr.zero_fields_scene, (1, 2, 3), (0, 1), False),
    ("rotation", sr.rotation_scene, (1, 2, 3), (0, 1), False),
    ("ex3", _ex3, (0, 1, 2), (0, 1), False),
]
PARAMS = [(i, f) for i, c in enumerate(CASES) for f in c[3]]
IDS = [f"{CASES[i][0]}-f{f}" for i, f in PARAMS]
# (forward, backward) x normalize
FLAG_SETS = [(fw, bw, nm) for nm in (False, True) for fw, bw in ((True, False), (False, True), (True, True))]


def seeds_of(prep):
    """the 48 uniform seeds of the reference's coverage test, then: NaN, infinite, far outside, on a region's upper face, on a
    brick corner, the root box's upper corner"""
    dom = domains(prep)
    mid = len(dom) // 2
    face = 0.5 * (dom[mid, :3] + dom[mid, 3:])
    face[0] = dom[mid, 3]
    b = np.asarray(prep.bricks())
    corner = np.asarray(b["lower"][len(b) // 2], dtype=np.float32)
    extra = np.array([[np.nan, 4, 4], [4, np.inf, 4], [1e6, -1e6, 3], face, corner, root_box(prep)[1]], dtype=np.float32)
    return np.ascontiguousarray(np.concatenate([sr.uniform_seeds(prep, N_UNIFORM), extra]))


_cache = {}


def _setup(idx, form):
    key = (idx, form)
    if key not in _cache:
        name, make, channels, _, empty = CASES[idx]
        case = Case(make(), basis_form=form, allow_empty_cells=empty, W=32, H=32)
        R = case.hip_renderer()
        S = case.oracle_scene()
        seeds = seeds_of(R.prep)
        ref = {}
        for nm in (False, True):      # every direction integrated once per mode; {F,B} is what the two imply (sr.joined)
            fwd = sr.streamlines(S, seeds, channels, STEP, MAX_STEPS, True, False, nm)
            back = sr.streamlines(S, seeds, channels, STEP, MAX_STEPS, False, True, nm)
            ref[(True, False, nm)], ref[(False, True, nm)], ref[(True, True, nm)] = fwd, back, sr.joined(back, fwd)
        _cache[key] = (case, R, S, seeds, channels, ref)
    return _cache[key]


def _same(got, want, what):
    names = ("vertices", "offsets", "seed_vertex", "reasons", "velocities")
    for k, nm in enumerate(names[:len(want)]):
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape, (what, nm, a.shape, b.shape)
        if a.dtype == np.float32:
            a, b = _bits(a), _bits(b)
        assert np.array_equal(a, b), (what, nm, np.argwhere(a != b)[:5])


@pytest.mark.parametrize("idx,form", PARAMS, ids=IDS)
def test_lines_equal_the_restatement_bit_for_bit(idx, form):
    case, R, S, seeds, channels, ref = _setup(idx, form)
    name = CASES[idx][0]
    novalue = 0
    for fw, bw, nm in FLAG_SETS:
        got = R.streamlines(seeds, channels, STEP, MAX_STEPS, forward=fw, backward=bw, normalize=nm, velocities=True)
        _same(got, ref[(fw, bw, nm)], (name, form, fw, bw, nm))
        # the reason counts of tests/test_streamline_ref.py, on what the GPU returned (the 48 uniform seeds)
        reasons, offsets = got[3][:N_UNIFORM], got[1]
        for slot in ([1] if fw else []) + ([0] if bw else []):
            n = sr.reason_counts(reasons, slot)
            print(f"{name} f{form} fw {fw} bw {bw} norm {nm} slot {slot}: {n}")
            if name == "amr3" and form == 1:
                assert n[sr.END_LEFT] >= 15 and n[sr.END_MAXSTEPS] >= 15, n
            if fw != bw:
                novalue += n[sr.END_NOVALUE]
        if name == "zero":
            inside = np.array([sr.StreamRef(S, channels).owner(s) >= 0 for s in seeds[:N_UNIFORM]])
            assert inside.sum() >= 10
            assert np.array_equal(np.diff(offsets.astype(np.int64)), np.ones(len(seeds), np.int64))
            want = np.array([sr.END_STAGNANT if bw else sr.END_NONE, sr.END_STAGNANT if fw else sr.END_NONE])
            assert np.all(reasons[inside] == want)
    if name == "amr3_holes":
        assert novalue >= 1


def test_structure_of_the_lines():
    case, R, S, seeds, channels, ref = _setup(0, 1)
    for nm in (False, True):
        fwd = R.streamlines(seeds, channels, STEP, MAX_STEPS, True, False, nm, True)
        back = R.streamlines(seeds, channels, STEP, MAX_STEPS, False, True, nm, True)
        both = R.streamlines(seeds, channels, STEP, MAX_STEPS, True, True, nm, True)
        _same(both, sr.joined(back, fwd), ("joined", nm))
        verts, offsets, seed_vertex, reasons, vels = both
        assert offsets[0] == 0 and np.all(np.diff(offsets.astype(np.int64)) >= 1) and int(offsets[-1]) == len(verts)
        assert np.array_equal(seed_vertex.astype(np.int64), np.diff(back[1].astype(np.int64)) - 1)
        assert np.array_equal(_bits(verts[(offsets[:-1] + seed_vertex).astype(np.int64)]), _bits(seeds))
        # every vertex but a failed seed: a value in all three channels, and that value is its velocity
        v, _, st = R.samplePoints(verts, channels=channels)
        failed = np.zeros(len(verts), dtype=bool)
        one = np.diff(offsets.astype(np.int64)) == 1
        failed[offsets[:-1][one].astype(np.int64)] = np.all(np.isnan(vels[offsets[:-1][one].astype(np.int64)]), axis=1)
        assert failed.sum() >= 3 and np.all(st[failed].min(axis=1) < 0)            # the NaN, infinite and far seeds at the least
        assert np.all(st[~failed] >= 0)
        assert np.array_equal(_bits(vels[~failed]), _bits(v[~failed]))
        assert np.all(np.isnan(vels[failed]))


def test_velocities_only_when_asked_for():
    case, R, S, seeds, channels, ref = _setup(0, 1)
    got = R.streamlines(seeds, channels, STEP, MAX_STEPS)
    assert got[4] is None
    _same(got[:4], ref[(True, False, False)][:4], "no velocities")


def test_lines_do_not_depend_on_the_batch_the_frame_state_or_options():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    seeds = sr.uniform_seeds(R.prep, 257)
    kw = dict(channels=(0, 1, 2), step=STEP, max_steps=MAX_STEPS, forward=True, backward=True, normalize=True, velocities=True)
    picks = (0, 63, 64, 256)
    single = {i: R.streamlines(seeds[i:i + 1], **kw) for i in picks}
    assert sum(len(s[0]) for s in single.values()) > 40

    def line(res, i):
        verts, offsets, seed_vertex, reasons, vels = res
        a, b = int(offsets[i]), int(offsets[i + 1])
        return _bits(verts[a:b]).tobytes(), _bits(vels[a:b]).tobytes(), int(seed_vertex[i]), reasons[i].tobytes()

    def same(what, batch=seeds, index=lambda i: i):
        res = R.streamlines(batch, **kw)
        for i in picks:
            if index(i) < len(batch):
                assert line(res, index(i)) == line(single[i], 0), (what, i)
        return res

    for n in (1, 63, 64, 65, 257):
        same(f"batch of {n}", seeds[:n])
    same("reversed", seeds[::-1].copy(), lambda i: 256 - i)
    first = same("again")
    _same(same("two calls"), first, "two calls")
    for what in frame_perturbations(case, R):
        same(what)
    R.close()


def test_multi_device_handle_equals_single():
    case, R, S, seeds, channels, ref = _setup(0, 1)
    M = multi_handle(R, 1)
    got = M.streamlines(seeds, channels, STEP, MAX_STEPS, True, True, True, True)
    _same(got, ref[(True, True, True)], "multi")
    M.close()


def test_scene_without_kd_tree_is_refused():
    R = binding.Renderer(without_kd_tree(binding.Prep(scenes.amr(levels=3, fields=3))))
    with pytest.raises(RuntimeError, match="kd-tree"):
        R.streamlines(np.zeros((4, 3), np.float32))
    R.close()


def test_a_cyclic_kd_tree_never_reaches_the_descent():
    # the descent's loop guard (return code 3) is a backstop: a tree that could trip it — a child that does not come after
    # its parent, here the root as its own child — is refused where it enters the module, by the prep and by creation
    prep = binding.Prep(scenes.amr(levels=3, fields=3))
    nodes = prep.kd_nodes().copy()
    root = int(prep.scene.kdRoot)
    assert root >= 0 and len(nodes) > 1
    nodes[root]["left"] = root
    with pytest.raises(RuntimeError, match="malformed kd-tree"):
        prep.set_kd_tree(nodes, root)
    prep.scene.kdNodes = nodes.ctypes.data                      # as a host that fills ExaHipScene by hand would
    with pytest.raises(RuntimeError, match="malformed kd-tree"):
        binding.Renderer(prep)


def test_bad_arguments_are_refused_and_the_handle_stays_usable():
    case, R, S, seeds, channels, ref = _setup(0, 1)
    L = binding.lib()
    ch = (C.c_int32 * 3)(*channels)
    nv = C.c_uint64(7)
    F, B = binding.STREAM_FORWARD, binding.STREAM_BACKWARD

    def call(n=len(seeds), ch=ch, step=STEP, max_steps=MAX_STEPS, flags=F):
        rc = L.exa_hip_streamlines(R.h, seeds.ctypes.data, n, ch, step, max_steps, flags, C.byref(nv), None)
        return rc, L.exa_hip_last_error(R.h).decode()

    def read_fails(match, velocities=None):
        buf = np.zeros(len(seeds) + 1, np.uint64)
        rc = L.exa_hip_streamlines_read(R.h, None, velocities, buf.ctypes.data if velocities is None else None, None, None, 0, None)
        assert rc != 0 and match in L.exa_hip_last_error(R.h).decode(), L.exa_hip_last_error(R.h).decode()

    bad = [(dict(step=0.0), "step"), (dict(step=-1.0), "step"), (dict(step=float("nan")), "step"), (dict(step=float("inf")), "step"),
           (dict(max_steps=0), "maxSteps"), (dict(max_steps=binding.STREAM_MAX_STEPS + 1), "maxSteps"),
           (dict(flags=0), "direction"), (dict(flags=binding.STREAM_NORMALIZE), "direction"), (dict(flags=F | 16), "flag"),
           (dict(flags=F | (1 << 30)), "flag"), (dict(ch=(C.c_int32 * 3)(0, 1, 3)), "channel"),
           (dict(ch=(C.c_int32 * 3)(-1, 1, 2)), "channel"), (dict(n=2 ** 31), "INT32_MAX")]
    for kw, match in bad:
        rc, msg = call(**kw)
        assert rc != 0 and "exa_hip_streamlines" in msg and match in msg, (kw, rc, msg)
        assert nv.value == 0
        read_fails("no lines")                                  # a failed extraction drops the lines
        got = R.streamlines(seeds, channels, STEP, MAX_STEPS, velocities=True)      # ... and the handle still extracts
        _same(got, ref[(True, False, False)], kw)
    # n == 0: zero vertices, and a read that copies offsets = {0}
    rc, _ = call(n=0)
    assert rc == 0 and nv.value == 0
    off = np.full(1, 99, np.uint64)
    assert L.exa_hip_streamlines_read(R.h, None, None, off.ctypes.data, None, None, 0, None) == 0 and off[0] == 0
    empty = R.streamlines(np.zeros((0, 3), np.float32), channels, STEP, MAX_STEPS, velocities=True)
    assert empty[0].shape == (0, 3) and empty[1].tolist() == [0] and empty[2].shape == (0,) and empty[3].shape == (0, 2)
    # velocities without the flag; release, then read
    rc, _ = call(flags=F | B)
    assert rc == 0 and nv.value == len(ref[(True, True, False)][0])
    vel = np.zeros((int(nv.value), 3), np.float32)
    read_fails("EXA_STREAM_VELOCITIES", velocities=vel.ctypes.data)
    assert L.exa_hip_streamlines_release(R.h) == 0
    read_fails("no lines")
    with pytest.raises(RuntimeError, match="no lines"):
        R.readStreamlines()


def test_read_before_any_extraction_is_an_error():
    R = Case(scenes.example("ex3")).hip_renderer()
    with pytest.raises(RuntimeError, match="no lines"):
        R.readStreamlines()
    ms = R.streamlinesMs()
    assert ms == 0.0
    R.close()
