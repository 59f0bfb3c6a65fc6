"""The contract of exa_hip_basins (include/exa_hip.h) restated in numpy: height and order, the up links, the raw basins, the
rounds of merging across the highest pass and the table.  The input is the lattice; no kernel is looked at.  Everything works
on whole arrays: the up links come from seven (three) shifted maxima of one 64-bit word per point, chains are resolved by
squaring the link array, and a round finds every component's highest pass by one sort of the edges that cross components —
which is not the device's algorithm (one lane per point, atomic maxima per component).  A component is named by the linear
index of its peak throughout."""
import math

import numpy as np

from regions_ref import FACES, KUHN, edges, inside, ordered_key, quantised, sum_exponent

BASIN = np.dtype([("points", "<u8"), ("sumFixed", "<i8"), ("sumIndex", "<u8", 3), ("lo", "<i4", 3), ("hi", "<i4", 3),
                  ("first", "<u4"), ("argMin", "<u4"), ("argMax", "<u4"), ("min", "<f4"), ("max", "<f4"),
                  ("neighbour", "<i4"), ("saddle", "<f4"), ("depth", "<f4")])
LOW32 = np.uint64(0xffffffff)
S32 = np.uint64(32)


def height(V, below=False):
    """h(L): the ordered key of V(L), complemented with below; uint32, V's shape"""
    k = ordered_key(V)
    return ~k if below else k


def value_of_height(h, below=False):
    """the float32 whose height is h"""
    k = np.asarray(h, np.uint32)
    k = ~k if below else k
    return np.where(k >> 31 != 0, k ^ np.uint32(0x80000000), ~k).astype(np.uint32).view(np.float32)


def order_word(V, below=False):
    """p is greater than q iff word(p) > word(q): h << 32 | (0xffffffff - L); uint64 [n]"""
    h = height(V, below).reshape(-1).astype(np.uint64)
    return (h << S32) | (LOW32 - np.arange(h.size, dtype=np.uint64))


def up_links(V, iso, below=False, faces=False):
    """up(p) per lattice point (its own index outside), int64 [n]"""
    V = np.ascontiguousarray(V, dtype=np.float32)
    nz, ny, nx = V.shape
    mask = inside(V, iso, below)
    word = np.where(mask, order_word(V, below).reshape(V.shape), np.uint64(0))     # 0: below every inside point's word
    best = word.copy()
    for dx, dy, dz in (FACES if faces else KUHN):
        p = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        q = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        best[p] = np.maximum(best[p], word[q])                       # one after the other: the two views overlap
        best[q] = np.maximum(best[q], word[p])
    up = (LOW32 - (best & LOW32)).astype(np.int64).reshape(-1)
    own = np.arange(V.size, dtype=np.int64)
    return np.where(mask.reshape(-1), up, own)


def resolve(link):
    """the fixed point of every chain of link, by squaring"""
    while True:
        nxt = link[link]
        if np.array_equal(nxt, link):
            return link
        link = nxt


def chain_lengths(link):
    """the number of links from every index to its fixed point"""
    dist = (link != np.arange(link.size)).astype(np.int64)
    while True:
        nxt = link[link]
        if np.array_equal(nxt, link):
            return dist
        dist = dist + dist[link]
        link = nxt


def longest_chain(V, iso, below=False, faces=False):
    return int(chain_lengths(up_links(V, iso, below, faces)).max(initial=0))


def basins(V, iso, min_depth, below=False, faces=False):
    """(labels int32 [nz, ny, nx], table BASIN [numBasins], sum_exponent, num_raw, rounds) of the lattice V [nz, ny, nx]"""
    V = np.ascontiguousarray(V, dtype=np.float32)
    md = np.float32(min_depth)
    assert V.ndim == 3 and math.isfinite(iso) and md >= 0
    nz, ny, nx = V.shape
    n = V.size
    flat = V.reshape(-1)
    mask = inside(V, iso, below)
    at = np.nonzero(mask.reshape(-1))[0]                             # the inside points, ascending L
    h = height(V, below).reshape(-1).astype(np.uint64)
    word = order_word(V, below)
    comp = resolve(up_links(V, iso, below, faces))                   # the peak of every point
    num_raw = int((comp[at] == at).sum())
    a, b = edges(mask, faces)
    hs = np.minimum(h[a], h[b])
    rounds = 0
    while True:
        ca, cb = comp[a], comp[b]
        live = ca != cb                                              # an edge inside a component stays inside one
        a, b, hs, ca, cb = a[live], b[live], hs[live], ca[live], cb[live]
        A, B = np.concatenate([ca, cb]), np.concatenate([cb, ca])    # every edge seen from both ends
        packed = (np.concatenate([hs, hs]) << S32) | (LOW32 - B.astype(np.uint64))
        order = np.argsort(packed, kind="stable")
        best = np.zeros(n, np.uint64)
        best[A[order]] = packed[order]                               # ascending: the last assignment, the greatest, stays
        roots = np.unique(A)
        other = (LOW32 - (best[roots] & LOW32)).astype(np.int64)
        saddle = value_of_height((best[roots] >> S32).astype(np.uint32), below)
        with np.errstate(over="ignore"):
            depth = (saddle - flat[roots]) if below else (flat[roots] - saddle)
        assert depth.dtype == np.float32 and np.all(depth >= 0)
        go = (depth < md) & (word[other] > word[roots])
        if not go.any():
            break
        assert rounds < num_raw
        link = np.arange(n, dtype=np.int64)
        link[roots[go]] = other[go]
        comp = resolve(link)[comp]
        rounds += 1
    peaks = np.unique(comp[at])                                      # a component's name is its peak: ascending L
    lab = np.searchsorted(peaks, comp[at])
    labels = np.full(n, -1, np.int32)
    labels[at] = lab
    s = sum_exponent(V, mask)
    nb = len(peaks)
    T = np.zeros(nb, BASIN)
    v = flat[at]
    T["points"] = np.bincount(lab, minlength=nb)
    np.add.at(T["sumFixed"], lab, quantised(v, s))
    ijk = (at % nx, (at // nx) % ny, at // (nx * ny))
    for c in range(3):
        col = np.zeros(nb, np.uint64)
        np.add.at(col, lab, ijk[c].astype(np.uint64))
        T["sumIndex"][:, c] = col
        lo, hi = np.full(nb, np.iinfo(np.int32).max, np.int32), np.full(nb, np.iinfo(np.int32).min, np.int32)
        np.minimum.at(lo, lab, ijk[c].astype(np.int32))
        np.maximum.at(hi, lab, ijk[c].astype(np.int32))
        T["lo"][:, c], T["hi"][:, c] = lo, hi
    first = np.full(nb, n, np.int64)
    np.minimum.at(first, lab, at)
    T["first"] = first
    key = ordered_key(v).astype(np.uint64) << S32
    kmin, kmax = np.full(nb, ~np.uint64(0)), np.zeros(nb, np.uint64)
    np.minimum.at(kmin, lab, key | at.astype(np.uint64))
    np.maximum.at(kmax, lab, key | (~at.astype(np.uint32)).astype(np.uint64))
    T["argMin"] = (kmin & LOW32).astype(np.uint32)
    T["argMax"] = ~(kmax & LOW32).astype(np.uint32)
    T["min"], T["max"] = flat[T["argMin"]], flat[T["argMax"]]
    # the last round's passes
    T["neighbour"], T["saddle"], T["depth"] = -1, np.float32(np.nan), np.float32(np.inf)
    mine = np.searchsorted(peaks, roots)
    T["neighbour"][mine] = np.searchsorted(peaks, other)
    T["saddle"][mine] = saddle
    T["depth"][mine] = depth
    return labels.reshape(V.shape), T, s, num_raw, rounds


def same_partition(x, y):
    """two label arrays (-1 outside) split the lattice into the same sets"""
    x, y = np.asarray(x).reshape(-1), np.asarray(y).reshape(-1)
    if not np.array_equal(x < 0, y < 0):
        return False
    x, y = x[x >= 0], y[y >= 0]
    if x.size == 0:
        return True
    pairs = np.unique(np.stack([x, y]), axis=1)
    return pairs.shape[1] == len(np.unique(x)) == len(np.unique(y))
