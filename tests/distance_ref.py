"""The numpy restatement of exa_hip_distance (include/exa_hip.h states the contract): the three passes X, Y, Z as the header
words them, in float32 with every operation rounded on its own, vectorised over the lattice and O(points x axis length).
tests/test_distance_ref.py holds it against the all-pairs minimum of the header's theorem; the GPU tests hold the module
against it byte for byte."""
import numpy as np

F = np.float32
INF = F(np.inf)


def spacing(lo, hi, dims):
    """h_a = (hi_a - lo_a) / float(n_a) in float32, as exa_hip_resample forms it"""
    lo, hi = np.asarray(lo, F).reshape(3), np.asarray(hi, F).reshape(3)
    return ((hi - lo) / np.asarray(dims, np.int64).reshape(3).astype(F)).astype(F)


def term(h, d):
    """term(d) = o*o, o = h * float(|d|): two float32 roundings"""
    o = (F(h) * np.abs(d).astype(F)).astype(F)
    return (o * o).astype(F)


def inside_of(values, iso, below=False):
    """the regions' rule on a lattice of values: finite and >= iso (below: finite and < iso)"""
    v = np.asarray(values, F)
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & ((v < F(iso)) if below else (v >= F(iso)))


def inside_of_labels(labels, label=-1):
    labels = np.asarray(labels, np.int32)
    return labels >= 0 if label == -1 else labels == label


def _column_pass(g, h, axis):
    """best[p] = min over q of g[q] + term(p - q) along `axis`, and the smallest q that holds it (-1 where best is +INF)"""
    n = g.shape[axis]
    g = np.moveaxis(g, axis, 0)
    best = np.full(g.shape, INF, F)
    arg = np.full(g.shape, -1, np.int64)
    at = np.arange(n).reshape((n,) + (1,) * (g.ndim - 1))
    for q in range(n):                                  # ascending: a strict < keeps the smallest q of equal candidates
        cand = (g[q][None] + term(h, at - q)).astype(F)
        win = cand < best
        best = np.where(win, cand, best)
        arg = np.where(win, q, arg)
    return np.moveaxis(best, 0, axis), np.moveaxis(arg, 0, axis)


def passes(target, h):
    """(a, b, c, d2) of the contract for the boolean target lattice [nz, ny, nx]; an index is -1 where its minimum is +INF"""
    target = np.asarray(target, bool)
    nz, ny, nx = target.shape
    i = np.arange(nx, dtype=np.int64)[None, None, :]
    none = np.int64(1) << 40
    lo = np.maximum.accumulate(np.where(target, i, -1), axis=2)
    hi = np.minimum.accumulate(np.where(target, i, none)[..., ::-1], axis=2)[..., ::-1]
    dl = np.where(lo >= 0, i - lo, none)
    dh = np.where(hi < none, hi - i, none)
    a = np.where(dl <= dh, lo, hi)                      # of two, the smaller i'
    a = np.where((lo < 0) & (hi >= none), -1, a)
    gx = np.where(a >= 0, term(h[0], i - a), INF).astype(F)
    gy, b = _column_pass(gx, h[1], 1)
    d2, c = _column_pass(gy, h[2], 0)
    return a, b, c, d2


def _one_sided(target, h, limit):
    """(dist >= 0 or +INF, nearest) of one target set"""
    nz, ny, nx = target.shape
    a, b, c, d2 = passes(target, h)
    reached = (d2 <= limit) & (d2 < INF)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    cc = np.where(reached, c, 0)
    bb = np.where(reached, b[cc, j, i], 0)
    aa = np.where(reached, a[cc, bb, i], 0)
    nearest = np.where(reached, (cc * ny + bb) * nx + aa, -1).astype(np.int32)
    dist = np.where(reached, np.sqrt(d2, dtype=F), INF).astype(F)
    return dist, nearest


def distance(inside, lo, hi, max_distance=np.inf, to_outside=False, signed=False):
    """dist float32 [nz, ny, nx], nearest int32, and the stats of exa_hip_distance for the boolean lattice `inside`"""
    inside = np.asarray(inside, bool)
    dims = inside.shape[::-1]
    h = spacing(lo, hi, dims)
    limit = F(F(max_distance) * F(max_distance))
    if signed:
        plus, near_plus = _one_sided(inside, h, limit)
        minus, near_minus = _one_sided(~inside, h, limit)
        dist = np.where(inside, -minus, plus).astype(F)
        nearest = np.where(inside, near_minus, near_plus).astype(np.int32)
    else:
        dist, nearest = _one_sided(~inside if to_outside else inside, h, limit)
    finite = np.isfinite(dist)
    stats = dict(points=int(inside.size), inside=int(inside.sum()), reached=int(finite.sum()),
                 maxDistance=float(np.abs(dist[finite]).max()) if finite.any() else 0.0)
    return dist, nearest, stats


def bands(dist, width, n):
    """what owlexabrick_amd.distance.distance_bands states: floor(|dist| / width) in float64, -1 where that is >= n or dist is
    not finite"""
    d = np.abs(np.asarray(dist, F).astype(np.float64))
    with np.errstate(invalid="ignore"):
        q = np.floor(d / float(width))
    ok = np.isfinite(d) & (q < n)
    return np.where(ok, q, -1).astype(np.int32)
