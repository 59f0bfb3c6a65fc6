"""The contract of exa_hip_isolines (include/exa_hip.h) restated in numpy, operation for operation in float32: marching
triangles on the split of every lattice square along the diagonal (0,0)-(1,1).  The input is the lattice of values; no
kernel is looked at.  Written from the rules as the header words them (the lone vertex, the parity of (s, o0, o1) by counting
inversions), not from the kernels' tables."""
import numpy as np

F = np.float32
TRI_CORNERS = (((0, 0), (1, 0), (1, 1)), ((0, 0), (0, 1), (1, 1)))      # T0 = (u,v), T1 = (v,u): (dx, dy) of v0, v1, v2
TRI_PARITY = (0, 1)


def positions(origin, du, dv, nu, nv):
    """P[j, i] = (origin + (float(i) + 0.5f) * du) + (float(j) + 0.5f) * dv per component, float32 [nv, nu, 3]"""
    o, u, v = (np.asarray(x, dtype=F).reshape(3) for x in (origin, du, dv))
    fi = (np.arange(nu, dtype=np.int64).astype(F) + F(0.5))[None, :, None]
    fj = (np.arange(nv, dtype=np.int64).astype(F) + F(0.5))[:, None, None]
    return ((o[None, None, :] + fi * u[None, None, :]) + fj * v[None, None, :]).astype(F)


def valid_squares(V):
    """[nv-1, nu-1]: the four corner values are finite"""
    f = np.isfinite(V)
    return f[:-1, :-1] & f[:-1, 1:] & f[1:, :-1] & f[1:, 1:]


def _inversions(seq):
    return sum(1 for a in range(len(seq)) for b in range(a + 1, len(seq)) if seq[a] > seq[b])


def _segment_rule(pattern, tri):
    """for the triangle-vertex pattern (bit n: vertex n is inside): ((s, o0), (s, o1)) as pairs of triangle vertices, in
    the order the segment runs"""
    ins = [n for n in range(3) if (pattern >> n) & 1]
    outs = [n for n in range(3) if not (pattern >> n) & 1]
    s, outside = (ins[0], 0) if len(ins) == 1 else (outs[0], 1)
    o0, o1 = sorted(n for n in range(3) if n != s)
    reverse = (_inversions((s, o0, o1)) & 1) ^ TRI_PARITY[tri] ^ outside
    seg = ((s, o0), (s, o1))
    return seg[::-1] if reverse else seg


def _level(V, P, iso):
    nv, nu = V.shape
    iso = F(iso)
    valid = valid_squares(V)
    inside = V >= iso
    # has[j, i, code-1]: the edge (i,j) -> (i+dx, j+dy), code = dx + 2 dy, belongs to a valid square
    has = np.zeros((nv, nu, 3), bool)
    has[:-1, :-1, 0] |= valid
    has[1:, :-1, 0] |= valid                    # the square below: origin p - e_v
    has[:-1, :-1, 1] |= valid
    has[:-1, 1:, 1] |= valid                    # the square to the left: origin p - e_u
    has[:-1, :-1, 2] |= valid
    cross = np.zeros((nv, nu, 3), bool)
    for code, (dx, dy) in ((1, (1, 0)), (2, (0, 1)), (3, (1, 1))):
        q = inside[dy:, dx:]
        cross[:nv - dy, :nu - dx, code - 1] = has[:nv - dy, :nu - dx, code - 1] & (inside[:nv - dy, :nu - dx] != q)
    jj, ii, cc = np.nonzero(cross)              # ascending L = j*nu + i, then ascending code
    code = cc + 1
    dx, dy = code & 1, code >> 1
    vid = np.full((nv, nu, 3), -1, np.int64)
    vid[jj, ii, cc] = np.arange(len(jj))
    with np.errstate(all="ignore"):
        vp, vq = V[jj, ii], V[jj + dy, ii + dx]
        t = ((iso - vp) / (vq - vp)).astype(F)
        Pp, Pq = P[jj, ii], P[jj + dy, ii + dx]
        verts = (Pp + t[:, None] * (Pq - Pp)).astype(F)
        uv = np.stack([(ii.astype(F) + F(0.5)) + t * dx.astype(F), (jj.astype(F) + F(0.5)) + t * dy.astype(F)], axis=1).astype(F)
    # segments: [nv-1, nu-1, tri, end]
    seg = np.full((nv - 1, nu - 1, 2, 2), -1, np.int64)
    emits = np.zeros((nv - 1, nu - 1, 2), bool)
    sj, si = np.meshgrid(np.arange(nv - 1), np.arange(nu - 1), indexing="ij")
    for tri in (0, 1):
        corners = TRI_CORNERS[tri]
        pat = sum(inside[cy:nv - 1 + cy, cx:nu - 1 + cx].astype(np.int64) << n for n, (cx, cy) in enumerate(corners))
        for pattern in range(1, 7):
            where = valid & (pat == pattern)
            if not where.any():
                continue
            emits[..., tri] |= where
            for end, (m, n) in enumerate(_segment_rule(pattern, tri)):
                lo, hi = corners[min(m, n)], corners[max(m, n)]
                ecode = (hi[0] - lo[0]) + 2 * (hi[1] - lo[1])
                seg[..., tri, end][where] = vid[sj[where] + lo[1], si[where] + lo[0], ecode - 1]
    segments = seg[emits]
    assert (segments >= 0).all()
    square = np.broadcast_to((sj * nu + si)[..., None], emits.shape)[emits]
    tri_of = np.broadcast_to(np.arange(2)[None, None, :], emits.shape)[emits]
    return dict(vertices=verts, uv=uv, segments=segments, owner=jj * nu + ii, code=code, square=square, tri=tri_of)


def extract(V, origin, du, dv, isos):
    """the result of exa_hip_isolines on the lattice values V [nv, nu] (float32): vertices [n,3], uv [n,2], segments int32
    [m,2] with global indices, vertex_offsets and segment_offsets uint64 [levels+1] — and, for the tests of the restatement
    itself, per vertex the owning lattice point `owner` and edge `code`, per segment the emitting `square` and `tri`"""
    V = np.ascontiguousarray(V, dtype=F)
    nv, nu = V.shape
    P = positions(origin, du, dv, nu, nv)
    levels = [_level(V, P, iso) for iso in np.asarray(isos, dtype=F).reshape(-1)]
    voff = np.cumsum([0] + [len(lv["vertices"]) for lv in levels]).astype(np.uint64)
    soff = np.cumsum([0] + [len(lv["segments"]) for lv in levels]).astype(np.uint64)
    cat = lambda k, dt, shape: (np.concatenate([lv[k] for lv in levels]).astype(dt).reshape(shape))      # noqa: E731
    segments = np.concatenate([lv["segments"] + int(voff[n]) for n, lv in enumerate(levels)]).astype(np.int32).reshape(-1, 2)
    return dict(vertices=cat("vertices", F, (-1, 3)), uv=cat("uv", F, (-1, 2)), segments=segments, vertex_offsets=voff,
                segment_offsets=soff, owner=cat("owner", np.int64, -1), code=cat("code", np.int64, -1),
                square=cat("square", np.int64, -1), tri=cat("tri", np.int64, -1))


ABI_KEYS = ("vertices", "uv", "segments", "vertex_offsets", "segment_offsets")
