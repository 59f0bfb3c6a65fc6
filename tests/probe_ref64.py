"""The reconstructed field and its gradient in float64, from the definition (plain numpy; no oracle, no kernel, nothing of
tests/isomesh_ref.py).

The reconstruction at a position p inside a region is the hat-basis interpolant over the bricks of that region,

    value(p) = sumWV / sumW,     sumW = SUM w,   sumWV = SUM w * s

summed over the cells of every brick of the region.  In a brick with lower corner `lower`, cell width cw = 2^level and
`size` cells per axis, with lp = (p - lower) / cw - 0.5 (the position in units of cells, measured from the first cell
centre), l = max(floor(lp), -1) and f = lp - l, the cells that take part are l and l + 1 per axis, those with
0 <= index < size; the weight of a cell is the product over the axes of (1 - f) for l and f for l + 1.  Scenes marked
allow_empty_cells skip a cell whose float32 scalar equals EMPTY_CELL_POISON_VALUE.

d w / d p_x of a cell is -+1/cw times the other two axes' factors, which gives sumD = SUM dw * s and sumDC = SUM dw and

    gradient(p) = (sumW * sumD - sumWV * sumDC) / sumW^2          (the gradient of value with respect to p)

The reference renderer takes -+1 instead of -+1/cw (its INV_CELL_WIDTH is 1) and does not divide: its numerator
sumW * sumD1 - sumWV * sumDC1 (`num`) is what EXA_SAMPLE_GRADIENT returns and what the shading uses.  Both are computed
here.  The cell scalars are the only float32 data: positions are taken exactly, everything else is float64.

Measured error of the CPU oracle (oracle/exa_oracle.c: float32, the operation order of the reference) against this
reference, in the scaled units of scaled_errors() below, over ref_points (tests/probe_sets.py: probe_points and
level_points) of every scene of REF_CASES; tests/test_probe_ref64.py::test_oracle_against_the_reference prints the figures.

Two strata of points.  The unit of scaled_errors() is the rounding of the SUMS; it knows nothing of the rounding of lp itself
(an absolute eps * |lp|), which a per-axis factor f or 1 - f inherits as a RELATIVE error eps * |lp| / f.  Where the position
sits in the last thousandth of a brick's support (f ~ 1e-3, sumW ~ 1e-3 and less: the rim of the scene, a few hundred of
the points, all in the grown bounding box or on region faces) that is hundreds of units.  So the constants are measured and
asserted twice: over "covered" points (sumW >= 0.5 in float64: the interior and every coarse-fine boundary), where they
are a handful of roundings, and over "all" points that have a value.
"""
import numpy as np

# measured 2026-10-17: the largest K_value / K_num over all cases, per stratum and basis form (0 = source order, 1 = per
# axis with fused multiply-adds)
K_VALUE_MEASURED = {"covered": {0: 6.141, 1: 4.422}, "all": {0: 329.5, 1: 324.9}}
K_NUM_MEASURED = {"covered": {0: 3.016, 1: 2.292}, "all": {0: 1742.0, 1: 601.2}}


def bound_from(measured):
    """4 x measured, rounded up to a power of two"""
    return float(2.0 ** np.ceil(np.log2(4.0 * measured)))


# the tests' bounds (the margin covers other point sets and seeds)
K_VALUE = {s: {f: bound_from(k) for f, k in d.items()} for s, d in K_VALUE_MEASURED.items()}
K_NUM = {s: {f: bound_from(k) for f, k in d.items()} for s, d in K_NUM_MEASURED.items()}
COVERED_SUMW = 0.5

EPS32 = 2.0 ** -24
POISON = np.float32(-1e20)        # EXA_EMPTY_CELL_POISON_VALUE (include/exa_hip.h)
STATUS_SUMW = 1e-20               # samplePoint says no where sumW <= this
STATUS_BAND = 1e-18               # 0 < sumW64 < this: float32 may land on either side of STATUS_SUMW


def stratum(ref, which):
    """[n, c] mask of evaluate()'s points: "covered" (sumW >= COVERED_SUMW) or "all" (every point; the caller adds its status)"""
    return ref["sumW"] >= COVERED_SUMW if which == "covered" else np.ones(ref["sumW"].shape, dtype=bool)


class Reconstruction:
    """scene: bricks7 / cellIDs / fields; regions, bricks, leaflist: the region table as the host preparation built it
    (regions(), bricks(), leaflist() of a binding.Prep or of an oracle scene)"""

    def __init__(self, scene, regions, bricks, leaflist, allow_empty_cells=False):
        self.cellIDs = np.asarray(scene.cellIDs, dtype=np.int64)
        self.fields = [np.asarray(f, dtype=np.float32) for f in scene.fields]
        self.allow_empty = bool(allow_empty_cells)
        self.list_begin = np.asarray(regions["leafListBegin"], dtype=np.int64)
        self.list_size = np.asarray(regions["leafListSize"], dtype=np.int64)
        self.dom_lo = np.stack(list(regions["dom_lo"])).astype(np.float64)
        self.dom_hi = np.stack(list(regions["dom_hi"])).astype(np.float64)
        self.leaflist = np.asarray(leaflist, dtype=np.int64)
        self.lower = np.stack(list(bricks["lower"])).astype(np.float64)
        self.size = np.stack(list(bricks["size"])).astype(np.int64)
        self.level = np.asarray(bricks["level"], dtype=np.int64)
        self.begin = np.asarray(bricks["begin"], dtype=np.int64)
        b7 = np.asarray(scene.bricks7, dtype=np.int64).reshape(-1, 7)
        assert np.array_equal(b7[:, 0:3], self.size) and np.array_equal(b7[:, 3:6], self.lower) and \
            np.array_equal(b7[:, 6], self.level), "the prepared bricks are the scene's bricks in the scene's order"
        assert np.array_equal(self.begin, np.cumsum(self.size.prod(axis=1)) - self.size.prod(axis=1))

    def pairs(self, region):
        """(point index, brick index) of every brick of every point's region; points with region < 0 have none"""
        sel = np.nonzero(region >= 0)[0]
        n = self.list_size[region[sel]]
        pid = np.repeat(sel, n)
        k = np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
        return pid, self.leaflist[np.repeat(self.list_begin[region[sel]], n) + k]

    def evaluate(self, pts, region, channels=(0,)):
        """pts [n, 3] (any float type, taken exactly as float64), region [n] (< 0: no region, every output 0 / NaN).
        Returns a dict of float64 arrays, [n, channels] and [n, channels, 3]:
          sumW, sumWV, value
          num    sumW * sumD1 - sumWV * sumDC1, derivative weights -+1 (the reference's numerator)
          grad   (sumW * sumD - sumWV * sumDC) / sumW^2, derivative weights -+1/cw (the gradient of value)
          aWV = SUM |w s|;  aD1, aDC1 = SUM |dw s|, SUM |dw| with -+1;  aD, aDC the same with -+1/cw;  sumDC"""
        pts = np.asarray(pts, dtype=np.float64)
        region = np.asarray(region, dtype=np.int64)
        n, nc = len(pts), len(channels)
        pid, bid = self.pairs(region)
        m = len(pid)
        size, cw, begin = self.size[bid], 2.0 ** self.level[bid].astype(np.float64), self.begin[bid]
        lp = (pts[pid] - self.lower[bid]) / cw[:, None] - 0.5
        lo = np.maximum(np.floor(lp), -1.0)
        f = lp - lo
        lo = lo.astype(np.int64)
        W, WV, aWV = np.zeros((m, nc)), np.zeros((m, nc)), np.zeros((m, nc))
        D, DC, aD, aDC = (np.zeros((m, nc, 3)) for _ in range(4))
        for cz in (0, 1):
            for cy in (0, 1):
                for cx in (0, 1):
                    side = np.array([cx, cy, cz])
                    idx = lo + side                                            # [m, 3]
                    inside = np.all((idx >= 0) & (idx < size), axis=1)
                    fac = np.where(side == 1, f, 1.0 - f)                      # per-axis factors
                    sgn = np.where(side == 1, 1.0, -1.0)
                    w = fac[:, 0] * fac[:, 1] * fac[:, 2]
                    dw = np.stack([sgn[0] * fac[:, 1] * fac[:, 2], fac[:, 0] * sgn[1] * fac[:, 2],
                                   fac[:, 0] * fac[:, 1] * sgn[2]], axis=1)
                    ic = np.clip(idx, 0, size - 1)
                    cell = begin + ic[:, 0] + size[:, 0] * (ic[:, 1] + size[:, 1] * ic[:, 2])
                    ids = self.cellIDs[cell]
                    for k, c in enumerate(channels):
                        s32 = np.where(ids >= 0, self.fields[c][np.maximum(ids, 0)], POISON).astype(np.float32)
                        ok = inside & ~(s32 == POISON) if self.allow_empty else inside
                        s = s32.astype(np.float64)
                        wk = np.where(ok, w, 0.0)
                        dk = np.where(ok[:, None], dw, 0.0)
                        W[:, k] += wk
                        WV[:, k] += wk * s
                        aWV[:, k] += np.abs(wk * s)
                        D[:, k] += dk * s[:, None]
                        DC[:, k] += dk
                        aD[:, k] += np.abs(dk * s[:, None])
                        aDC[:, k] += np.abs(dk)

        def per_point(x, scale=None):
            out = np.zeros((n,) + x.shape[1:])
            np.add.at(out, pid, x if scale is None else x * scale.reshape((-1,) + (1,) * (x.ndim - 1)))
            return out

        inv = 1.0 / cw
        r = dict(sumW=per_point(W), sumWV=per_point(WV), aWV=per_point(aWV),
                 sumD1=per_point(D), sumDC1=per_point(DC), aD1=per_point(aD), aDC1=per_point(aDC),
                 sumD=per_point(D, inv), sumDC=per_point(DC, inv), aD=per_point(aD, inv), aDC=per_point(aDC, inv))
        sw, swv = r["sumW"][..., None], r["sumWV"][..., None]
        with np.errstate(divide="ignore", invalid="ignore"):
            r["value"] = r["sumWV"] / r["sumW"]
            r["num"] = sw * r["sumD1"] - swv * r["sumDC1"]
            r["grad"] = (sw * r["sumD"] - swv * r["sumDC"]) / (sw * sw)
        return r

    def near_a_kink(self, pts, region, dist):
        """per point: closer than `dist` (voxel units) on some axis to a cell-centre plane of a brick of its region (the planes
        lp = 0 .. size, where a brick's interpolant changes its piece), or to a face of the region's domain"""
        pts = np.asarray(pts, dtype=np.float64)
        region = np.asarray(region, dtype=np.int64)
        pid, bid = self.pairs(region)
        cw = 2.0 ** self.level[bid].astype(np.float64)
        lp = (pts[pid] - self.lower[bid]) / cw[:, None] - 0.5
        k = np.round(lp)
        hit = np.any((np.abs(lp - k) * cw[:, None] < dist) & (k >= 0) & (k <= self.size[bid]), axis=1)
        out = np.zeros(len(pts), dtype=bool)
        np.logical_or.at(out, pid, hit)
        ok = region >= 0
        r = np.maximum(region, 0)
        face = np.any((np.abs(pts - self.dom_lo[r]) < dist) | (np.abs(pts - self.dom_hi[r]) < dist), axis=1)
        return out | (face & ok)


def scaled_errors(ref, value, num, eps=EPS32):
    """the errors of a float32 value [n, c] and raw numerator [n, c, 3] against evaluate()'s result, in units of the float32
    rounding of the sums that cancel:  |v - v64| / (eps aWV / sumW)  and  max over the axes of
    |g - num64| / (eps (sumW aD1 + aWV aDC1)).  A term that is exactly zero (a constant zero field) with a zero error counts 0."""
    sw, awv = ref["sumW"], ref["aWV"]
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = eps * awv / sw
        ev = np.abs(np.asarray(value, dtype=np.float64) - ref["value"])
        kv = np.where(ev == 0, 0.0, ev / uv)
        ug = eps * (sw[..., None] * ref["aD1"] + awv[..., None] * ref["aDC1"])
        eg = np.abs(np.asarray(num, dtype=np.float64) - ref["num"])
        kg = np.where(eg == 0, 0.0, eg / ug).max(axis=-1)
    return kv, kg


def normalized_bound(ref, k_num, eps=EPS32):
    """the allowance for a float32 normalized gradient [n, c, 3]: the numerator's error (k_num: the bound K_NUM of the form) in
    voxel units over sumW^2, plus 4 eps of the result for the product sumW * sumW and the division"""
    sw, awv = ref["sumW"][..., None], ref["aWV"][..., None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return k_num * eps * (sw * ref["aD"] + awv * ref["aDC"]) / (sw * sw) + 4.0 * eps * np.abs(ref["grad"])
