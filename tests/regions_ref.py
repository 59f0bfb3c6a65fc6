"""The contract of exa_hip_regions (include/exa_hip.h) restated in numpy: the connected components of the inside set of a
lattice of values under the Kuhn edges (or the axis edges), numbered by their smallest linear index, with the exact
measurements of the table.  The input is the lattice; no kernel is looked at.  The components come from hooking and pointer
jumping over the edge lists — every round hangs each root below the smallest root an edge joins it to and then compresses
every path, so the number of rounds grows with the logarithm of a component's size, not with its diameter — which is not
the device's algorithm (one lane per point, unions in arrival order)."""
import math

import numpy as np

REGION = np.dtype(dict(names=["points", "sumFixed", "sumIndex", "lo", "hi", "first", "argMin", "argMax", "min", "max"],
                       formats=["<u8", "<i8", ("<u8", 3), ("<i4", 3), ("<i4", 3), "<u4", "<u4", "<u4", "<f4", "<f4"],
                       offsets=[0, 8, 16, 40, 52, 64, 68, 72, 76, 80], itemsize=88))
KUHN = [(dx, dy, dz) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)][1:]       # d in {0,1}^3 \ {0}, as (dx, dy, dz)
FACES = [(1, 0, 0), (0, 1, 0), (0, 0, 1)]


def inside(V, iso, below=False):
    """V finite and V >= iso (below: V < iso); V is [nz, ny, nx] float32"""
    V = np.asarray(V, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(V) & ((V < np.float32(iso)) if below else (V >= np.float32(iso)))


def edges(mask, faces=False):
    """the pairs (L(p), L(p + d)) of linear indices with both ends inside, for every edge kind"""
    nz, ny, nx = mask.shape
    L = np.arange(mask.size, dtype=np.int64).reshape(mask.shape)
    a, b = [], []
    for dx, dy, dz in (FACES if faces else KUHN):
        p = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
        q = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
        both = mask[p] & mask[q]
        a.append(L[p][both])
        b.append(L[q][both])
    return np.concatenate(a), np.concatenate(b)


def roots(mask, faces=False):
    """per lattice point the smallest linear index of its component (its own index outside), int64 [n]; and the rounds"""
    a, b = edges(mask, faces)
    parent = np.arange(mask.size, dtype=np.int64)
    rounds = 0
    while True:
        ra, rb = parent[a], parent[b]                 # roots: every path is compressed
        live = ra != rb
        if not live.any():
            break
        a, b, ra, rb = a[live], b[live], ra[live], rb[live]
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:
            up = parent[parent]
            if np.array_equal(up, parent):
                break
            parent = up
        rounds += 1
    return parent, rounds


def ordered_key(V):
    """the total order of exa_hip_histogram's value range: uint32 keys of the float bits (-0.0 < +0.0)"""
    b = np.ascontiguousarray(V, dtype=np.float32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def sum_exponent(V, mask):
    """s = 0 without inside points or with M = max |V| = 0, else 30 - e, M = f * 2^e, f in [0.5, 1)"""
    if not mask.any():
        return 0
    M = float(np.abs(V[mask]).max())
    return 0 if M == 0.0 else 30 - math.frexp(M)[1]


def quantised(v, s):
    """q(v) = (double)v * 2^s to the nearest integer, ties to even"""
    return np.rint(np.ldexp(np.asarray(v, dtype=np.float32).astype(np.float64), s)).astype(np.int64)


def regions(V, iso, below=False, faces=False):
    """(labels int32 [nz, ny, nx], table REGION [numRegions], sum_exponent) of the lattice V [nz, ny, nx]"""
    V = np.ascontiguousarray(V, dtype=np.float32)
    assert V.ndim == 3 and math.isfinite(iso)
    nz, ny, nx = V.shape
    mask = inside(V, iso, below)
    parent, _ = roots(mask, faces)
    at = np.nonzero(mask.reshape(-1))[0]                            # the inside points, ascending L
    first = np.unique(parent[at])                                   # a component's root is its smallest index
    lab = np.searchsorted(first, parent[at])
    labels = np.full(V.size, -1, np.int32)
    labels[at] = lab
    s = sum_exponent(V, mask)
    n = len(first)
    T = np.zeros(n, REGION)
    T["first"] = first
    v = V.reshape(-1)[at]
    T["points"] = np.bincount(lab, minlength=n)
    np.add.at(T["sumFixed"], lab, quantised(v, s))
    ijk = (at % nx, (at // nx) % ny, at // (nx * ny))
    T["lo"], T["hi"] = np.iinfo(np.int32).max, np.iinfo(np.int32).min
    for c in range(3):
        col = np.zeros(n, np.uint64)
        np.add.at(col, lab, ijk[c].astype(np.uint64))
        T["sumIndex"][:, c] = col
        lo, hi = np.full(n, np.iinfo(np.int32).max, np.int32), np.full(n, np.iinfo(np.int32).min, np.int32)
        np.minimum.at(lo, lab, ijk[c].astype(np.int32))
        np.maximum.at(hi, lab, ijk[c].astype(np.int32))
        T["lo"][:, c], T["hi"][:, c] = lo, hi
    # min / max with the smallest L among equals: a 64-bit key, the value key above L (min) or above ~L (max)
    key = ordered_key(v).astype(np.uint64) << np.uint64(32)
    kmin, kmax = np.full(n, ~np.uint64(0)), np.zeros(n, np.uint64)
    np.minimum.at(kmin, lab, key | at.astype(np.uint64))
    np.maximum.at(kmax, lab, key | (~at.astype(np.uint32)).astype(np.uint64))
    flat = V.reshape(-1)
    T["argMin"] = (kmin & np.uint64(0xffffffff)).astype(np.uint32)
    T["argMax"] = ~(kmax & np.uint64(0xffffffff)).astype(np.uint32)
    T["min"], T["max"] = flat[T["argMin"]], flat[T["argMax"]]
    return labels.reshape(V.shape), T, s
