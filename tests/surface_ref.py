"""The contract of exa_hip_sample_triangles (include/exa_hip.h) restated in numpy: a triangle's areaNormal and subdivision n,
the float32 positions of its n * n samples operation for operation in the header's association, and the reduction of a
triangle's samples in 64 slots and a tree.  What a sample IS comes from outside, as in project_ref.py: the (values, status)
that the existing point probe (Renderer.samplePoints) returns at those positions, and never the new call itself.

numpy's float32 multiply, add, subtract, divide and sqrt are correctly rounded, each call one operation."""
import numpy as np

f32 = np.float32
T1 = f32(1.0) / f32(3.0)
T2 = f32(2.0) / f32(3.0)
SLOTS = 64


def _corners(vertices, triangles):
    """(in_range [m], v0, v1, v2 [m,3] float32; the corners of a triangle with a bad index are NaN)"""
    v = np.ascontiguousarray(vertices, dtype=f32).reshape(-1, 3)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = ((t >= 0) & (t < len(v))).all(axis=1)
    safe = np.where(ok[:, None], t, 0)
    if len(v) == 0:
        nan = np.full((len(t), 3), np.nan, f32)
        return ok, nan, nan, nan
    c = [np.where(ok[:, None], v[safe[:, k]], f32(np.nan)).astype(f32) for k in range(3)]
    return ok, c[0], c[1], c[2]


def area_normal(vertices, triangles):
    """0.5f * (e1 x e2), float32 [m,3]; three NaN where an index is out of range"""
    ok, v0, v1, v2 = _corners(vertices, triangles)
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        n = f32(0.5) * n
    assert n.dtype == f32
    return n


def longest_edge(vertices, triangles):
    """L float32 [m]: the maximum of the lengths of v1-v0, v2-v1, v0-v2, NaN if one of them is (np.maximum propagates it)"""
    ok, v0, v1, v2 = _corners(vertices, triangles)
    with np.errstate(all="ignore"):
        lengths = []
        for d in (v1 - v0, v2 - v1, v0 - v2):
            lengths.append(np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2], dtype=f32))
        L = np.maximum(np.maximum(lengths[0], lengths[1]), lengths[2])
    assert L.dtype == f32
    return L


def subdiv_of_length(L, spacing, max_n):
    """n of valid triangles whose longest edge is L (finite) float32 [m]"""
    L = np.asarray(L, dtype=f32)
    if f32(spacing) == 0:
        return np.full(L.shape, max_n, np.int32)
    with np.errstate(all="ignore"):
        q = L / f32(spacing)
        assert q.dtype == f32
        small = np.maximum(1, np.ceil(np.where(q >= f32(max_n), f32(0), q)).astype(np.int64))
    return np.where(q >= f32(max_n), max_n, small).astype(np.int32)


def subdivision(vertices, triangles, spacing, max_n):
    """subdiv int32 [m]: n, 0 for a triangle that is not valid"""
    ok, _, _, _ = _corners(vertices, triangles)
    L = longest_edge(vertices, triangles)
    valid = ok & np.isfinite(L)
    return np.where(valid, subdiv_of_length(np.where(valid, L, f32(0)), spacing, max_n), 0).astype(np.int32)


def ab_map(n):
    """(a, b, upright) of the samples k = 0 .. n*n-1: the integers whose float32 plus T1 (upright) or T2 is fa, fb times n"""
    k = np.arange(n * n)
    a, b = k // n, k % n
    upright = a + b < n
    return np.where(upright, a, n - 1 - a), np.where(upright, b, n - 1 - b), upright


def barycentrics(n):
    """(b1, b2) float32 [n*n]"""
    a, b, upright = ab_map(n)
    t = np.where(upright, T1, T2).astype(f32)
    fa, fb = a.astype(f32) + t, b.astype(f32) + t
    b1, b2 = fa / f32(n), fb / f32(n)
    assert b1.dtype == f32 and b2.dtype == f32
    return b1, b2


def positions(v0, v1, v2, n):
    """p_k float32 [.., n*n, 3] of triangles with corners v0, v1, v2 [.., 3] and the same n"""
    v0, v1, v2 = (np.asarray(x, dtype=f32) for x in (v0, v1, v2))
    b1, b2 = barycentrics(n)
    with np.errstate(all="ignore"):
        e1, e2 = v1 - v0, v2 - v0
        p = (v0[..., None, :] + b1[:, None] * e1[..., None, :]) + b2[:, None] * e2[..., None, :]
    assert p.dtype == f32
    return p


def tree(P):
    """the contract's tree over the last axis (64 float64 slots): o = 32 .. 1, P_l = P_l + P_{l+o} for l < o; returns P_0"""
    P = np.array(P, dtype=np.float64, copy=True)
    assert P.shape[-1] == SLOTS
    o = SLOTS // 2
    with np.errstate(all="ignore"):
        while o >= 1:
            P[..., :o] = P[..., :o] + P[..., o:2 * o]
            o //= 2
    return P[..., 0]


def reduce(values, status):
    """(sum float64 [..], count uint32 [..]) of samples along the last axis: values float32 [.., K], status int [.., K].

    Slot l takes the valid samples k = l, l + 64, .. in ascending k from +0.0: np.cumsum adds along an axis in order, and an
    invalid sample is skipped by adding +0.0 in its place, which is the same thing bit for bit — x + 0.0 == x for every x but
    -0.0, and a slot, started at +0.0, is never -0.0 (a sum is -0.0 only if both terms are)."""
    values = np.asarray(values, dtype=f32)
    valid = np.asarray(status) >= 0
    K = values.shape[-1]
    blocks = -(-K // SLOTS)
    pad = [(0, 0)] * (values.ndim - 1) + [(0, blocks * SLOTS - K)]
    v = np.pad(np.where(valid, values, f32(0)).astype(np.float64), pad).reshape(values.shape[:-1] + (blocks, SLOTS))
    zero = np.zeros(values.shape[:-1] + (1, SLOTS))
    with np.errstate(all="ignore"):
        P = np.cumsum(np.concatenate([zero, v], axis=-2), axis=-2)[..., -1, :]
    return tree(P), valid.sum(axis=-1).astype(np.uint32)


def reduce_literal(values, status):
    """one triangle and channel, the contract's loops as written (tests/test_surface_ref.py holds reduce against it)"""
    P = [np.float64(0.0)] * SLOTS
    count = 0
    with np.errstate(all="ignore"):
        for k, (v, st) in enumerate(zip(np.asarray(values, dtype=f32), status)):
            if st < 0:
                continue
            count += 1
            P[k % SLOTS] = P[k % SLOTS] + np.float64(v)
        o = SLOTS // 2
        while o >= 1:
            for l in range(o):
                P[l] = P[l] + P[l + o]
            o //= 2
    return P[0], np.uint32(count)


def sample_triangles(sample, vertices, triangles, num_channels, spacing, max_n):
    """the reference: sample(points [n,3]) -> (values [n,C], status [n,C]) is the existing point probe.  Returns the dict of
    Renderer.sampleTriangles (sum, count, areaNormal, subdiv) and (values, status) of all samples (by n, then by triangle)"""
    ok, v0, v1, v2 = _corners(vertices, triangles)
    m = len(ok)
    sub = subdivision(vertices, triangles, spacing, max_n)
    total = np.zeros((m, num_channels), np.float64)
    count = np.zeros((m, num_channels), np.uint32)
    groups = [(n, np.flatnonzero(sub == n)) for n in np.unique(sub) if n > 0]
    pts = [positions(v0[ids], v1[ids], v2[ids], int(n)).reshape(-1, 3) for n, ids in groups]
    values = np.zeros((0, num_channels), f32)
    status = np.zeros((0, num_channels), np.int64)
    if pts:
        values, status = sample(np.ascontiguousarray(np.concatenate(pts)))
        values = np.asarray(values, dtype=f32).reshape(-1, num_channels)
        status = np.asarray(status, dtype=np.int64).reshape(-1, num_channels)
    at = 0
    for n, ids in groups:
        k = int(n) * int(n)
        v = values[at:at + len(ids) * k].reshape(len(ids), k, num_channels)
        s = status[at:at + len(ids) * k].reshape(len(ids), k, num_channels)
        at += len(ids) * k
        total[ids], count[ids] = reduce(np.moveaxis(v, 1, 2), np.moveaxis(s, 1, 2))
    return dict(sum=total, count=count, areaNormal=area_normal(vertices, triangles), subdiv=sub), values, status


def same_bits(a, b):
    """equal shape, dtype and bytes (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_sums(a, b):
    """sums equal bit for bit, a NaN comparing as a NaN (its payload and sign are not part of the contract)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return same_bits(np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b))
