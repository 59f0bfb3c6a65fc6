"""exa_hip_histogram on the GPU against the numpy restatement of its contract (tests/histogram_ref.py): cells, volume and every
stats field bit for bit, over scenes, bin counts, ranges, boxes, special values and the shapes where the wave-level
aggregation of equal bins can go wrong; nothing but the scene, the channel, the range, the bins and the box moves the
result; every error of the contract is refused and leaves the handle usable."""
import ctypes as C
import math

import numpy as np
import pytest

from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case, band_xf
from owlexabrick_amd import binding, scenes
from histogram_ref import Slots, same_stats

pytestmark = pytest.mark.gpu

BINS = (1, 7, 128, 4096)
ODD_GRIDS = ("0 0 0 9 10 11 0  0.0 1.0 0.25 0.75 0.5 0.1 0.9 0.3\n"      # larger than a workgroup, partial last wave
             "16 0 0 3 5 7 2  0.2 0.4 0.6 0.8 1.0 0.0 0.3 0.7\n"           # level 2
             "0 16 0 1 1 1 3  0.45\n"                                        # one cell, level 3
             "0 12 0 67 1 1 0  0.0 1.0 0.0 1.0 0.0 1.0 0.0 1.0")             # one row of 67: a wave and three cells


def _with_field(scene, by_slot):
    """the scene with one more field whose value in cell slot s (brick order) is by_slot[s]"""
    ids = np.asarray(scene.cellIDs)
    f = np.zeros(len(scene.fields[0]), dtype=np.float32)
    f[ids[ids >= 0]] = np.asarray(by_slot, dtype=np.float32)[ids >= 0]
    return scenes.Scene(scene.bricks7, scene.cellIDs, list(scene.fields) + [f], name=scene.name + "_x", meta=dict(scene.meta))


def _build(name):
    if name in ("ex0", "ex3", "ex4"):
        return scenes.example(name), False
    if name == "amr3":
        return scenes.amr(levels=3, fields=3), False
    if name == "generated":
        return scenes.generated(root=(2, 2, 2), B=4, levels=2), False
    if name == "amr3_holes":
        return scenes.with_empty_cells(scenes.amr(levels=3, fields=2), 0.15), True
    if name == "odd":
        return scenes.artificial(scenes.parse_grids(ODD_GRIDS), name="odd"), False
    raise KeyError(name)


_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_renderers():
    yield
    for _, _, R in _CACHE.values():
        R.close()
    _CACHE.clear()


def _case(name):
    """(scene, Slots, Renderer) of a named scene, made once and shared (the reference side is never changed)"""
    if name not in _CACHE:
        scene, allow = _build(name)
        R = Case(scene, W=32, H=32, allow_empty_cells=allow).hip_renderer()
        _CACHE[name] = (scene, Slots(scene, allow), R)
    return _CACHE[name]


def _check(R, S, channel, lo, hi, bins, box=None, what=""):
    got = R.histogram(channel, lo, hi, bins, box=box)
    want = S.histogram(channel, lo, hi, bins, box=box)
    assert got[0].dtype == np.uint64 and got[0].tobytes() == want[0].tobytes(), (what, channel, lo, hi, bins, box)
    assert got[1].tobytes() == want[1].tobytes(), (what, channel, lo, hi, bins, box)
    assert same_stats(got[2], want[2]), (what, channel, lo, hi, bins, box, got[2], want[2])
    no_volume = R.histogram(channel, lo, hi, bins, box=box, volume=False)
    assert no_volume[1] is None and no_volume[0].tobytes() == want[0].tobytes() and same_stats(no_volume[2], want[2])
    return got


def _ranges(S, channel):
    """min..max; a narrow one that sends most cells to under / over; lo and hi each exactly a data value"""
    v = S.values(channel)
    v = np.unique(v[np.isfinite(v) & (v != np.float32(-1e20))])
    if len(v) < 2:
        return []
    lo, hi = v[0], v[-1]
    span = np.float32(hi - lo)
    out = [(lo, hi), (np.float32(lo + np.float32(0.48) * span), np.float32(lo + np.float32(0.52) * span))]
    if len(v) >= 4:
        out.append((v[len(v) // 4], v[3 * len(v) // 4]))
    return out


def _boxes(scene):
    lo, hi = ([int(x) for x in b] for b in scene.bounds())
    b7 = np.asarray(scene.bricks7, dtype=np.int64).reshape(-1, 7)
    big = b7[np.argmax(b7[:, 0] * b7[:, 1] * b7[:, 2])]
    w = 1 << int(big[6])
    inside_lo = [int(big[3 + k]) + (w if big[k] >= 3 else 0) for k in range(3)]
    inside_hi = [int(big[3 + k]) + w * (int(big[k]) - (1 if big[k] >= 3 else 0)) for k in range(3)]
    return [None,
            [(lo[0] + 1) | 1, (lo[1] + 2) | 1, lo[2] | 1, (hi[0] - 2) | 1, (hi[1] - 4) | 1, (hi[2] - 2) | 1],   # odd: cuts bricks and coarse cells
            inside_lo + inside_hi,                                                                               # inside one brick
            [hi[0] + 5, hi[1] + 5, hi[2] + 5, hi[0] + 9, hi[1] + 9, hi[2] + 9],                                   # outside the scene
            [lo[0], lo[1], lo[2], hi[0], lo[1], hi[2]]]                                                          # lo == hi on y


def test_single_cell_scene():
    scene, S, R = _case("ex0")
    st = R.fieldStats(0)
    assert same_stats(st, S.histogram(0, 0, 0, 0)[2]) and st["slots"] == st["binned"] == 1 and st["min"] == st["max"] == np.float32(1.0)
    for bins in BINS:
        _check(R, S, 0, 0.5, 1.5, bins)
        _check(R, S, 0, 1.0, 2.0, bins)
        _check(R, S, 0, 0.0, 1.0, bins)          # hi == the value: the last bin


@pytest.mark.parametrize("name", ["ex3", "ex4", "amr3", "generated", "amr3_holes", "odd"])
def test_histogram_equals_the_restatement(name):
    scene, S, R = _case(name)
    if name == "amr3":
        assert len(S.ids) == 23552 and len(np.asarray(scene.bricks7).reshape(-1, 7)) == 368
    if name == "amr3_holes":
        assert int((S.ids < 0).sum()) == 3787 and len(S.ids) == 23552
    if name == "odd":
        assert len(S.ids) == 1163 and R.prep.scene.numRegions == 19
    boxes = _boxes(scene)
    for channel in range(len(scene.fields)):
        for box in boxes:
            st = R.fieldStats(channel, box=box)
            assert same_stats(st, S.histogram(channel, 0, 0, 0, box=box)[2]), (channel, box)
        whole = R.fieldStats(channel)
        ranges = _ranges(S, channel)
        assert ranges and (whole["min"], whole["max"]) == ranges[0]                 # min..max comes from the range-only call
        for lo, hi in ranges:
            for bins in BINS:
                for box in boxes:
                    got = _check(R, S, channel, lo, hi, bins, box=box)
                    if name == "amr3" and bins == 128 and box is None and (lo, hi) == ranges[0]:
                        assert int((got[0] > 0).sum()) == (121, 128, 126)[channel]      # occupied bins over min..max
    cut = R.fieldStats(0, box=boxes[1])
    assert 0 < cut["slots"] < len(S.ids)                                             # the odd box really cuts
    assert 0 < R.fieldStats(0, box=boxes[2])["slots"] < len(S.ids)
    assert R.fieldStats(0, box=boxes[3])["slots"] == 0 and R.fieldStats(0, box=boxes[4])["slots"] == 0


def test_special_values():
    base = scenes.artificial(scenes.parse_grids(ODD_GRIDS), name="odd")
    n = base.num_cells
    special = np.linspace(-2.0, 2.0, n).astype(np.float32)
    special[[0, 63, 64, 700, 989]] = np.nan
    special[[1, 65, 990]] = np.inf
    special[[2, 127, 1095]] = -np.inf          # 1095: the level-3 cell
    special[[3, 500]] = -0.0
    special[[4, 501]] = 0.0
    zeros = np.zeros(n, dtype=np.float32)       # only zeros of both signs: min is -0.0, max is +0.0, by their bits
    zeros[5::7] = -0.0
    scene = _with_field(_with_field(base, special), zeros)
    S = Slots(scene)
    R = Case(scene, W=32, H=32, xf_domains=[(0.0, 1.0)] * len(scene.fields)).hip_renderer()   # no frame is rendered here
    st = R.fieldStats(1)
    assert st["nan"] == 5 and st["min"] == -np.inf and st["max"] == np.inf
    assert same_stats(st, S.histogram(1, 0, 0, 0)[2])
    for lo, hi in ((-2.0, 2.0), (-1.0, 1.0), (0.0, 1.0), (-1.0, 0.0), (-0.0, 3.0e38), (-1.5e38, 1.5e38)):
        for bins in BINS:
            for box in _boxes(scene)[:3]:
                _check(R, S, 1, lo, hi, bins, box=box)
    st = R.fieldStats(2)
    assert np.float32(st["min"]).tobytes() == np.float32(-0.0).tobytes() and np.float32(st["max"]).tobytes() == np.float32(0.0).tobytes()
    assert same_stats(st, S.histogram(2, 0, 0, 0)[2])
    _check(R, S, 2, -1.0, 1.0, 7)
    _check(R, S, 2, 0.0, 1.0, 7)                 # -0.0 is not below lo = +0.0
    R.close()


def test_contention_and_aggregation_shapes():
    base = scenes.amr(levels=3, fields=1)
    n = base.num_cells
    s = np.arange(n)
    scene = _with_field(base, np.full(n, 0.25))                          # every lane of every wave in one bin
    scene = _with_field(scene, np.where((s // 3) % 2 == 0, 0.25, 0.75))  # two values, in runs of three lanes
    scene = _with_field(scene, (s % 64) + 0.5)                           # 64 distinct bins in every wave
    scene = _with_field(scene, np.where(s % 64 < 40, 7.5, (s % 64) + 0.5))   # one heavy bin, one lighter, the rest spread
    S = Slots(scene)
    R = Case(scene, W=32, H=32, xf_domains=[(0.0, 1.0)] * len(scene.fields)).hip_renderer()   # no frame is rendered here
    for channel, (lo, hi) in ((1, (0.0, 1.0)), (2, (0.0, 1.0)), (3, (0.0, 64.0)), (4, (0.0, 64.0))):
        for bins in BINS + (64,):
            for box in _boxes(scene)[:3]:
                got = _check(R, S, channel, lo, hi, bins, box=box)
        assert int(got[0].sum()) > 0
    whole = R.histogram(3, 0.0, 64.0, 64)
    assert int((whole[0] > 0).sum()) == 64
    R.close()


def test_nothing_else_moves_the_result():
    scene = scenes.amr(levels=3, fields=3)
    S = Slots(scene)
    case = Case(scene, W=32, H=32)
    R = case.hip_renderer()
    box = _boxes(scene)[1]
    r = R.fieldStats(1)
    want = S.histogram(1, r["min"], r["max"], 128, box=box)

    def same(Rx, what):
        got = Rx.histogram(1, r["min"], r["max"], 128, box=box)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and same_stats(got[2], want[2]), what
        assert same_stats(Rx.fieldStats(1), r), what

    same(R, "fresh handle")
    same(R, "second call")
    R.render()
    same(R, "after a frame")
    xf = band_xf()
    R.updateXF(1, xf[:, 3], xf[:, :3], (0.2, 0.6), 0.5)
    R.render()
    same(R, "after a TF change")
    for what in frame_perturbations(case, R):
        same(R, what)
    R.setOption("interleave", 1)
    R.render()
    same(R, "interleave 1")
    for form in (0, 1):
        R.setOption("basis_form", form)
        R.render()
        same(R, f"basis_form {form}")
    M = multi_handle(R)
    same(M, "multi-device handle with a repeated device")
    M.close()
    R.close()
    N = without_kd_tree(case).hip_renderer()
    same(N, "scene without kd nodes")
    N.close()


@pytest.mark.parametrize("extra, fits", [("0 16777216 0 1 1 1 21  0.35", True),      # 2^63 + the rest: the largest shift, 63 bits
                                         ("0 16777216 0 2 2 2 21  0.35", False),     # 8 cells at level 21: 2^66
                                         ("0 16777216 0 1 1 1 22  0.35", False)],    # one cell at level 22: 2^66
                         ids=["one-cell-level-21", "eight-cells-level-21", "one-cell-level-22"])
def test_volume_beyond_64_bits_is_refused(extra, fits):
    # exa_hip_create takes levels up to 30, the volume-weighted total fits 64 bits only up to level 21: with a volume array the
    # call is refused when the sum over all bricks of cells * 8^level does not fit, and everything else still works
    scene = scenes.artificial(scenes.parse_grids(ODD_GRIDS + "\n" + extra), name="odd_coarse")
    S = Slots(scene)
    R = Case(scene, W=32, H=32).hip_renderer()                            # no frame is rendered here
    r = R.fieldStats(0)
    assert same_stats(r, S.histogram(0, 0, 0, 0)[2]) and r["levelCells"][int(extra.split()[6])] > 0
    boxes = [None, [1, 3, 1, 65, 21, 27], [0, 16777216, 0, 1 << 23, 16777216 + (1 << 23), 1 << 23]]
    for box in boxes:
        for bins in (7, 128):
            if fits:
                got = _check(R, S, 0, r["min"], r["max"], bins, box=box)
                if box != boxes[1]:
                    assert int(got[1].sum()) >= 1 << 63                   # the coarse cell's 8^21 voxels are in it
            else:
                with pytest.raises(RuntimeError, match=r"exa_hip_histogram: .*does not fit 64 bits"):
                    R.histogram(0, r["min"], r["max"], bins, box=box, volume=True)
                got = R.histogram(0, r["min"], r["max"], bins, box=box, volume=False)      # the next valid call
                want = S.histogram(0, r["min"], r["max"], bins, box=box)                   # (its volume wraps: not compared)
                assert got[1] is None and got[0].tobytes() == want[0].tobytes() and same_stats(got[2], want[2])
                assert same_stats(R.fieldStats(0, box=box), S.histogram(0, 0, 0, 0, box=box)[2])
    R.close()


def test_bad_arguments_are_refused_and_leave_the_handle_usable():
    # (the contract's "brick level outside 0..31" cannot be reached through the public interface: exa_hip_create refuses a
    # level above 30; the refusal of a volume beyond 64 bits has its own test above)
    scene, S, R = _case("amr3")
    L = binding.lib()
    cells = np.zeros(4096, dtype=np.uint64)
    vol = np.zeros(4096, dtype=np.uint64)

    def raw(channel=0, lo=0.0, hi=1.0, bins=16, box=None, cells_ptr=cells.ctypes.data, vol_ptr=vol.ctypes.data):
        b6 = (C.c_int32 * 6)(*box) if box is not None else None
        st = binding.ExaHipFieldStats()
        rc = L.exa_hip_histogram(R.h, channel, lo, hi, bins, b6, cells_ptr, vol_ptr, C.byref(st), None)
        return rc, L.exa_hip_last_error(R.h).decode()

    assert raw()[0] == 0
    big = float(np.finfo(np.float32).max)
    tiny = float(np.float32(1e-45))
    bad = [dict(lo=math.nan), dict(hi=math.nan), dict(lo=-math.inf), dict(hi=math.inf), dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0),
           dict(lo=-big, hi=big),                      # hi - lo is not finite
           dict(lo=0.0, hi=tiny, bins=4096),           # numBins / (hi - lo) is not finite
           dict(bins=4097), dict(bins=-1), dict(cells_ptr=None), dict(channel=len(scene.fields)), dict(channel=-1),
           dict(box=[4, 0, 0, 3, 9, 9]), dict(box=[0, 0, 9, 9, 9, 8])]
    for kw in bad:
        rc, msg = raw(**kw)
        assert rc != 0 and msg.startswith("exa_hip_histogram: ") and len(msg) > 25, (kw, rc, msg)
        r = R.fieldStats(1)
        _check(R, S, 1, r["min"], r["max"], 128, box=_boxes(scene)[1], what=str(kw))       # the next valid call
    # range only ignores lo / hi / cells / volume
    assert raw(lo=math.nan, hi=math.nan, bins=0, cells_ptr=None, vol_ptr=None)[0] == 0
    # an empty box is no error
    rc, _ = raw(box=[3, 3, 3, 3, 9, 9])
    assert rc == 0 and not cells[:16].any() and not vol[:16].any()
