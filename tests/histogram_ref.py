"""The contract of exa_hip_histogram (include/exa_hip.h) restated in numpy from a scene's own arrays — bricks7, cellIDs
(negative = empty when the case allows empty cells), fields — without the module's prep: the slots of every brick in list
order with the running `begin`, the centre rule of the box in 64-bit integers, the classes in their order, the bin in
float32 with every operation rounded separately, uint64 counts, min / max through the ordered key.  Not a test module."""
import numpy as np

POISON = np.float32(-1e20)          # EXA_EMPTY_CELL_POISON_VALUE
MAX_LEVELS = 32


def ordered_key(v):
    """the sign-flip map of float32 bit patterns to uint32 keys whose order is the total order with -0.0 < +0.0"""
    bits = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    return np.where(bits >> np.uint32(31) != 0, ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(key):
    key = np.uint32(key)
    bits = key ^ np.uint32(0x80000000) if key >> np.uint32(31) else ~key
    return np.array([bits], dtype=np.uint32).view(np.float32)[0]


class Slots:
    """every cell slot (b, i) of a scene, in brick order, x fastest: its cell id, its brick's level and the doubled
    coordinates of its centre, 2*(lower + idx*2^level) + 2^level.  Built once per scene and shared by the tests."""

    def __init__(self, scene, allow_empty_cells=False):
        b7 = np.asarray(scene.bricks7, dtype=np.int64).reshape(-1, 7)
        ids, level, centre2 = [], [], []
        begin = 0
        for sx, sy, sz, lx, ly, lz, lv in b7:
            n = int(sx * sy * sz)
            i = np.arange(n, dtype=np.int64)
            idx = np.stack([i % sx, (i // sx) % sy, i // (sx * sy)], axis=1)
            w = np.int64(1) << lv
            centre2.append(2 * (np.array([lx, ly, lz], dtype=np.int64) + idx * w) + w)
            level.append(np.full(n, lv, dtype=np.int64))
            ids.append(np.asarray(scene.cellIDs[begin:begin + n], dtype=np.int64))
            begin += n
        assert begin == len(scene.cellIDs)
        self.ids = np.concatenate(ids)
        self.level = np.concatenate(level)
        self.centre2 = np.concatenate(centre2)
        self.allow_empty = bool(allow_empty_cells)
        self.fields = [np.ascontiguousarray(f, dtype=np.float32) for f in scene.fields]
        if not self.allow_empty:
            assert (self.ids >= 0).all()

    def values(self, channel):
        f = self.fields[channel]
        v = f[np.maximum(self.ids, 0)].copy()
        v[self.ids < 0] = POISON                          # the slot of a missing cell holds the poison value
        return v

    def histogram(self, channel, lo, hi, bins, box=None, per_level=False):
        """(cells uint64 [bins], volume uint64 [bins], stats) as Renderer.histogram returns them; bins = 0: range only.
        per_level: cells as [MAX_LEVELS, bins] instead, one row per brick level."""
        v = self.values(channel)
        level = self.level
        if box is not None:
            blo, bhi = np.asarray(box[:3], dtype=np.int64), np.asarray(box[3:], dtype=np.int64)
            assert (blo <= bhi).all()
            keep = ((2 * blo <= self.centre2) & (self.centre2 < 2 * bhi)).all(axis=1)
            v, level = v[keep], level[keep]
        empty = (v == POISON) if self.allow_empty else np.zeros(v.shape, dtype=bool)
        nan = ~empty & np.isnan(v)
        rest = ~empty & ~nan
        cells = np.zeros((MAX_LEVELS, bins), dtype=np.uint64)
        if bins > 0:
            lo, hi = np.float32(lo), np.float32(hi)
            under = rest & (v < lo)
            over = rest & ~under & (v > hi)
            binned = rest & ~under & ~over
            scale = np.float32(np.float32(bins) / np.float32(hi - lo))
            with np.errstate(invalid="ignore", over="ignore"):
                t = (v[binned] - lo).astype(np.float32) * scale
            assert t.dtype == np.float32
            b = np.minimum(bins - 1, t.astype(np.int32))
            np.add.at(cells, (level[binned], b), np.uint64(1))
        else:
            under = over = np.zeros(v.shape, dtype=bool)
            binned = rest
        level_cells = np.zeros(MAX_LEVELS, dtype=np.uint64)
        np.add.at(level_cells, level[~empty], np.uint64(1))
        stats = dict(empty=int(empty.sum()), nan=int(nan.sum()), under=int(under.sum()), over=int(over.sum()),
                     binned=int(binned.sum()), levelCells=level_cells)
        stats["slots"] = stats["empty"] + stats["nan"] + stats["under"] + stats["over"] + stats["binned"]
        if rest.any():
            keys = ordered_key(v[rest])
            stats["min"], stats["max"] = key_to_float(keys.min()), key_to_float(keys.max())
        else:
            stats["min"], stats["max"] = np.float32(np.inf), np.float32(-np.inf)
        weight = np.uint64(8) ** np.arange(MAX_LEVELS, dtype=np.uint64)[:, None] if bins else np.zeros((MAX_LEVELS, 0), np.uint64)
        with np.errstate(over="ignore"):
            volume = (cells * weight).sum(axis=0, dtype=np.uint64) if bins else np.zeros(0, dtype=np.uint64)
        if per_level:
            return cells, volume, stats
        return cells.sum(axis=0, dtype=np.uint64), volume, stats


def same_stats(a, b):
    """every field of two stats dicts, min / max by their bits"""
    keys = ("slots", "empty", "nan", "under", "over", "binned")
    return (all(int(a[k]) == int(b[k]) for k in keys) and np.array_equal(a["levelCells"], b["levelCells"])
            and np.float32(a["min"]).tobytes() == np.float32(b["min"]).tobytes()
            and np.float32(a["max"]).tobytes() == np.float32(b["max"]).tobytes())
