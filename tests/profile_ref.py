"""The contract of exa_hip_profile (include/exa_hip.h) restated in numpy: lattice points binned by one or two keys, with the
count, the fixed-point sums and the min / max of other quantities per bin.  The inputs are flat float32 arrays of one entry
per lattice point (on the GPU tests: what Renderer.resample / resampleDerived return, and positions / radius / coordinate
below for the sources the kernels form themselves); no kernel is looked at."""
import math

import numpy as np

from regions_ref import ordered_key, quantised

F = np.float32


def positions(lo, hi, dims):
    """P[3][n] float32: per axis lo + (float(i) + 0.5f) * ((hi - lo) / float(n)), every operation in float32, L = (k*ny + j)*nx + i"""
    nx, ny, nz = (int(d) for d in dims)
    L = np.arange(nx * ny * nz, dtype=np.int64)
    idx = (L % nx, (L // nx) % ny, L // (nx * ny))
    out = []
    for a in range(3):
        step = (F(hi[a]) - F(lo[a])) / F(dims[a])
        out.append(F(lo[a]) + (idx[a].astype(F) + F(0.5)) * step)
    return out


def coordinate(lo, hi, dims, axis):
    return positions(lo, hi, dims)[axis]


def radius(lo, hi, dims, centre):
    """sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z), d = P - centre, in float32"""
    P = positions(lo, hi, dims)
    d = [P[a] - F(centre[a]) for a in range(3)]
    with np.errstate(all="ignore"):
        return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]).astype(F)


def uniform(v, lo, hi, n):
    return dict(mode="uniform", v=np.ascontiguousarray(v, F).reshape(-1), lo=F(lo), hi=F(hi), n=int(n))


def edges(v, e):
    e = np.ascontiguousarray(e, F).reshape(-1)
    assert e.size >= 2 and np.isfinite(e).all() and (np.diff(e) > 0).all()
    return dict(mode="edges", v=np.ascontiguousarray(v, F).reshape(-1), e=e, n=e.size - 1)


def labels(lab, n):
    return dict(mode="labels", lab=np.ascontiguousarray(lab, np.int32).reshape(-1), n=int(n))


def exponent(terms):
    """s = 0 without a term or with M = max |term| = 0, else 30 - e, M = f * 2^e, f in [0.5, 1)"""
    if terms.size == 0:
        return 0
    M = float(np.abs(terms).max())
    return 0 if M == 0.0 else 30 - math.frexp(M)[1]


def _axis_bins(ax):
    """(nan, under, over, bin) of a uniform or edges axis, per point; bin is meaningful where none of the three holds"""
    v = ax["v"]
    with np.errstate(all="ignore"):
        nan = np.isnan(v)
        if ax["mode"] == "uniform":
            lo, hi, n = ax["lo"], ax["hi"], ax["n"]
            under, over = v < lo, v > hi
            ok = ~(nan | under | over)
            t = np.zeros(v.shape, F)
            t[ok] = (v[ok] - lo) * (F(n) / (hi - lo))
            b = np.minimum(n - 1, t.astype(np.int32)).astype(np.int64)
        else:
            e, n = ax["e"], ax["n"]
            under, over = v < e[0], v > e[n]
            ok = ~(nan | under | over)
            b = np.zeros(v.shape, np.int64)
            b[ok] = np.minimum(n - 1, np.searchsorted(e, v[ok], side="right") - 1)
    return nan, under, over, b


def profile(axes, values=(), weight=None, minmax=True):
    """the dict of Renderer.profile (the arrays flat over the bins, b1 * numBins0 + b0) for axes built by uniform / edges /
    labels, flat float32 `values` and `weight`.  A label >= numBins is a ValueError that names the first such L."""
    axes = list(axes)
    assert len(axes) in (1, 2) and all(a["mode"] != "labels" for a in axes[1:])
    values = [np.ascontiguousarray(v, F).reshape(-1) for v in values]
    n = (axes[0]["lab"] if axes[0]["mode"] == "labels" else axes[0]["v"]).size
    outside = np.zeros(n, bool)
    invalid = np.zeros(n, bool)
    under = [np.zeros(n, bool), np.zeros(n, bool)]
    over = [np.zeros(n, bool), np.zeros(n, bool)]
    bin_ = np.zeros(n, np.int64)
    stride = 1
    for k, ax in enumerate(axes):
        if ax["mode"] == "labels":
            lab = ax["lab"]
            bad = np.nonzero(lab >= ax["n"])[0]
            if bad.size:
                raise ValueError(f"a label >= numBins, first at L = {int(bad[0])}")
            outside = lab < 0
            b = lab.astype(np.int64)
        else:
            nan, under[k], over[k], b = _axis_bins(ax)
            invalid |= nan
        bin_ += b * stride
        stride *= ax["n"]
    B = stride
    with np.errstate(all="ignore"):
        w = None if weight is None else np.ascontiguousarray(weight, F).reshape(-1)
        terms = [v if w is None else (w * v).astype(F) for v in values]
        for x in values + terms + ([w] if w is not None else []):
            invalid |= ~np.isfinite(x)
    invalid &= ~outside
    free = ~outside & ~invalid
    u0 = free & under[0]
    o0 = free & ~under[0] & over[0]
    free1 = free & ~under[0] & ~over[0]
    u1 = free1 & under[1]
    o1 = free1 & ~under[1] & over[1]
    binned = free1 & ~under[1] & ~over[1]
    at = bin_[binned]
    count = np.bincount(at, minlength=B).astype(np.uint64)
    stats = dict(points=n, outside=int(outside.sum()), invalid=int(invalid.sum()), under=[int(u0.sum()), int(u1.sum())],
                 over=[int(o0.sum()), int(o1.sum())], binned=int(binned.sum()), weightExponent=0, valueExponent=[0, 0, 0, 0])
    sum_weight = None
    if w is not None:
        s = stats["weightExponent"] = exponent(w[binned])
        sum_weight = np.zeros(B, np.int64)
        np.add.at(sum_weight, at, quantised(w[binned], s))
    sums = np.zeros((len(values), B), np.int64)
    mins = np.full((len(values), B), np.inf, F)
    maxs = np.full((len(values), B), -np.inf, F)
    for f, (v, term) in enumerate(zip(values, terms)):
        s = stats["valueExponent"][f] = exponent(term[binned])
        np.add.at(sums[f], at, quantised(term[binned], s))
        key = ordered_key(v[binned])
        kmin, kmax = np.full(B, 0xffffffff, np.uint32), np.zeros(B, np.uint32)
        np.minimum.at(kmin, at, key)
        np.maximum.at(kmax, at, key)
        have = count > 0
        back = lambda k: np.where(k >> 31 != 0, k & np.uint32(0x7fffffff), ~k).astype(np.uint32).view(F)     # noqa: E731
        mins[f][have], maxs[f][have] = back(kmin)[have], back(kmax)[have]
    return dict(count=count, sum_weight=sum_weight, sums=sums, mins=mins if minmax else None, maxs=maxs if minmax else None,
                stats=stats)
