"""The numpy restatement of exa_hip_histogram's contract (tests/histogram_ref.py) checked against itself and against
np.histogram, on the CPU: the GPU tests compare the module with it bit for bit, so it has to be right on its own."""
import numpy as np
import pytest

from owlexabrick_amd import scenes
from histogram_ref import Slots, key_to_float, ordered_key, same_stats


def _cases():
    return {
        "ex3": (scenes.example("ex3"), False),
        "ex4": (scenes.example("ex4"), False),
        "amr3": (scenes.amr(levels=3, fields=3), False),
        "amr3_holes": (scenes.with_empty_cells(scenes.amr(levels=3, fields=2), 0.15), True),
    }


CASES = _cases()
SLOTS = {name: Slots(scene, allow) for name, (scene, allow) in CASES.items()}


def test_exact_bins_equal_numpy_histogram():
    # one level, values k/256 + 1/512 (exact in float32), lo = 0, hi = 1, 256 bins: v - 0, * 256 and the cast are all exact
    n = 8 * 8 * 8
    k = (np.arange(n) * 37) % 256
    values = (k / 256.0 + 1.0 / 512.0).astype(np.float32)
    assert np.array_equal(values.astype(np.float64), k / 256.0 + 1.0 / 512.0)
    scene = scenes.Scene(np.array([[8, 8, 8, 0, 0, 0, 0]], dtype=np.int32), np.arange(n, dtype=np.int32), [values])
    cells, volume, st = Slots(scene).histogram(0, 0.0, 1.0, 256)
    want, _ = np.histogram(values.astype(np.float64), bins=256, range=(0.0, 1.0))
    assert np.array_equal(cells, want.astype(np.uint64))
    assert np.array_equal(volume, cells)                  # level 0: one voxel per cell
    assert st["slots"] == st["binned"] == n and st["levelCells"][0] == n
    assert st["min"] == values.min() and st["max"] == values.max()


@pytest.mark.parametrize("name", sorted(CASES))
def test_classes_add_up_and_levels_count_the_non_empty(name):
    S = SLOTS[name]
    for ch in range(len(S.fields)):
        r = S.histogram(ch, 0.0, 0.0, 0)[2]
        lo, hi = r["min"], r["max"]
        mid = np.float32(0.5) * (lo + hi)
        for (a, b, bins) in ((lo, hi, 128), (lo, mid, 7), (mid, hi, 1)):
            if not a < b:
                continue
            cells, volume, st = S.histogram(ch, a, b, bins)
            assert st["slots"] == st["empty"] + st["nan"] + st["under"] + st["over"] + st["binned"] == len(S.ids)
            assert int(st["levelCells"].sum()) == st["slots"] - st["empty"]
            assert int(cells.sum()) == st["binned"]
            assert st["empty"] == (int((S.ids < 0).sum()) if S.allow_empty else 0)
            assert same_stats({**st, "under": 0, "over": 0, "binned": r["binned"]}, r)   # the range pass: same but unsplit


@pytest.mark.parametrize("name", ["amr3", "amr3_holes"])
def test_two_boxes_split_at_an_odd_coordinate_add_up(name):
    S = SLOTS[name]
    scene = CASES[name][0]
    lo, hi = (int(v) for v in scene.bounds()[0]), (int(v) for v in scene.bounds()[1])
    lo, hi = list(lo), list(hi)
    r = S.histogram(0, 0.0, 0.0, 0)[2]
    whole = S.histogram(0, r["min"], r["max"], 128)
    for axis in range(3):
        # an odd coordinate inside a level-2 cell (4 voxels wide, centre at lower + 2): one past the centre of the median one
        c2 = np.sort(S.centre2[S.level == 2, axis])
        cut = int(c2[len(c2) // 2]) // 2 + 1
        assert cut % 2 == 1 and lo[axis] < cut < hi[axis]
        through = (S.centre2[:, axis] - (1 << S.level) < 2 * cut) & (S.centre2[:, axis] + (1 << S.level) > 2 * cut)
        assert (S.level[through] == 2).any()                          # the centre rule decides for them
        a_hi, b_lo = list(hi), list(lo)
        a_hi[axis], b_lo[axis] = cut, cut
        a = S.histogram(0, r["min"], r["max"], 128, box=lo + a_hi)
        b = S.histogram(0, r["min"], r["max"], 128, box=b_lo + hi)
        assert a[2]["slots"] and b[2]["slots"]
        assert np.array_equal(a[0] + b[0], whole[0]) and np.array_equal(a[1] + b[1], whole[1])
        for k in ("slots", "empty", "nan", "under", "over", "binned"):
            assert a[2][k] + b[2][k] == whole[2][k]
        assert np.array_equal(a[2]["levelCells"] + b[2]["levelCells"], whole[2]["levelCells"])
        assert min(a[2]["min"], b[2]["min"]) == whole[2]["min"] and max(a[2]["max"], b[2]["max"]) == whole[2]["max"]


@pytest.mark.parametrize("name", sorted(CASES))
def test_volume_is_the_level_weighted_sum(name):
    S = SLOTS[name]
    r = S.histogram(0, 0.0, 0.0, 0)[2]
    per_level, volume, st = S.histogram(0, r["min"], r["max"], 128, per_level=True)
    cells = S.histogram(0, r["min"], r["max"], 128)[0]
    assert np.array_equal(per_level.sum(axis=0, dtype=np.uint64), cells)
    want = sum(int(8 ** L) * per_level[L].astype(object) for L in range(per_level.shape[0]))   # python integers
    assert [int(v) for v in volume] == [int(v) for v in want]
    assert len(set(S.level.tolist())) >= 2 and not np.array_equal(volume, cells)


def test_ordered_key_is_the_total_order():
    v = np.array([-np.inf, -1.5, -np.float32(1e-45), -0.0, 0.0, np.float32(1e-45), 2.0, np.inf], dtype=np.float32)
    k = ordered_key(v)
    assert (np.diff(k.astype(np.int64)) > 0).all()
    assert all(key_to_float(x).tobytes() == y.tobytes() for x, y in zip(k, v))
