"""Marching tetrahedra on a lattice of values, restated in numpy from the contract of exa_hip_isosurface (include/exa_hip.h),
operation for operation in float32 — the checker of tests/test_gpu_isomesh.py, with property tests of its own in
tests/test_isomesh_ref.py.  Nothing here looks at the kernels.

Lattice point (i,j,k) of a dims = (nx,ny,nz) lattice over [lo, hi] lies at lo + (float(i) + 0.5f) * ((hi - lo) / float(n))
per axis; V has the shape [nz, ny, nx] (what Renderer.resample returns), L = (k*ny + j)*nx + i."""
import numpy as np

F = np.float32
# the six tetrahedra of a cube: permutation (a,b,c) of the axes, lexicographic; v0 = origin, v1 = v0+e_a, v2 = v1+e_b, v3 = v2+e_c
PERMS = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], dtype=np.int64)


def parity(seq):
    """number of inversions mod 2"""
    return sum(1 for i in range(len(seq)) for j in range(i + 1, len(seq)) if seq[i] > seq[j]) & 1


def tet_corners(perm):
    """the tet's four vertices as corner codes dx + 2*dy + 4*dz of the cube"""
    a, b, c = perm
    return [0, 1 << a, (1 << a) | (1 << b), (1 << a) | (1 << b) | (1 << c)]


def tet_triangles(pattern, perm):
    """the triangles of a tet whose vertex n is inside iff bit n of `pattern` is set: a list of triangles, each three tet
    edges (x, y) — "the vertex on the edge between tet vertices x and y" """
    ins = [v for v in range(4) if (pattern >> v) & 1]
    outs = [v for v in range(4) if not (pattern >> v) & 1]
    if len(ins) in (1, 3):
        s = ins[0] if len(ins) == 1 else outs[0]
        o = [v for v in range(4) if v != s]
        tri = [(s, o[0]), (s, o[1]), (s, o[2])]
        if parity([s] + o) ^ parity(perm) ^ (1 if len(ins) == 3 else 0):
            tri.reverse()
        return [tri]
    if len(ins) == 2:
        (a, b), (c, d) = ins, outs
        q = [(a, c), (a, d), (b, d), (b, c)]
        if parity([a, b, c, d]) ^ parity(perm):
            q.reverse()
        return [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    return []


def lattice_axes(lo, hi, dims):
    """the float32 coordinates of the lattice points per axis"""
    axes = []
    for a in range(3):
        step = (F(hi[a]) - F(lo[a])) / F(dims[a])
        axes.append(F(lo[a]) + (np.arange(dims[a]).astype(F) + F(0.5)) * step)
    return axes


def _shifted(arr, d, fill=False):
    """out[p] = arr[p - d] (d a corner code), `fill` where p - d leaves the lattice"""
    dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
    out = np.full_like(arr, fill)
    nz, ny, nx = arr.shape
    out[dz:, dy:, dx:] = arr[:nz - dz, :ny - dy, :nx - dx]
    return out


def _ahead(arr, d, fill):
    """out[p] = arr[p + d], `fill` where p + d leaves the lattice"""
    dx, dy, dz = d & 1, (d >> 1) & 1, d >> 2
    out = np.full_like(arr, fill)
    nz, ny, nx = arr.shape
    out[:nz - dz, :ny - dy, :nx - dx] = arr[dz:, dy:, dx:]
    return out


def valid_cubes(V):
    """[nz, ny, nx] bool, indexed by the cube's origin: all 8 corner values finite (False where no cube starts)"""
    fin = np.isfinite(V)
    ok = fin.copy()
    for m in range(1, 8):
        ok &= _ahead(fin, m, False)
    ok[-1, :, :] = False
    ok[:, -1, :] = False
    ok[:, :, -1] = False
    return ok


def extract(V, lo, hi, iso):
    """-> (verts float32 [n,3], tris int32 [m,3]) of the surface V == iso"""
    V = np.ascontiguousarray(V, dtype=F)
    nz, ny, nx = V.shape
    assert min(nx, ny, nz) >= 2 and np.isfinite(iso)
    iso = F(iso)
    with np.errstate(invalid="ignore"):
        inside = V >= iso
    valid = valid_cubes(V)
    # mask[p] bit (code-1): the edge p -> p + code crosses and belongs to a valid cube.  The cubes that hold it: origin
    # p - m for every corner code m that shares no axis with `code` (then p = origin + m and q = origin + m + code are
    # corners of it, and m, m + code lie on a common chain origin -> ... -> origin + (1,1,1): a tet edge)
    mask = np.zeros(V.shape, dtype=np.uint8)
    for code in range(1, 8):
        crosses = inside != _ahead(inside, code, False)
        belongs = np.zeros(V.shape, dtype=bool)
        for m in range(8):
            if m & code == 0:
                belongs |= _shifted(valid, m)          # a valid cube keeps q inside the lattice
        mask |= (crosses & belongs).astype(np.uint8) << np.uint8(code - 1)
    flat = mask.reshape(-1)
    count = _POPCOUNT[flat]
    first = np.cumsum(count) - count               # vertices in front of lattice point L: ascending L, then edge code
    nverts = int(count.sum())

    axes = lattice_axes(lo, hi, (nx, ny, nz))
    verts = np.empty((nverts, 3), dtype=F)
    Vf = V.reshape(-1)
    for code in range(1, 8):
        dx, dy, dz = code & 1, (code >> 1) & 1, code >> 2
        L = np.nonzero(flat & (1 << (code - 1)))[0]
        i, j, k = L % nx, (L // nx) % ny, L // (nx * ny)
        vp, vq = Vf[L], Vf[L + dx + dy * nx + dz * nx * ny]
        with np.errstate(all="ignore"):
            t = (iso - vp) / (vq - vp)
            at = first[L] + _POPCOUNT[flat[L] & ((1 << (code - 1)) - 1)]
            for a, (c, dc) in enumerate(((i, dx), (j, dy), (k, dz))):
                pp, pq = axes[a][c], axes[a][c + dc]
                verts[at, a] = pp + t * (pq - pp)

    # triangles: ascending L of the cube origin, then the tet order, then the order of tet_triangles
    cubes = np.nonzero(valid.reshape(-1))[0]
    corner = [(m & 1) + ((m >> 1) & 1) * nx + (m >> 2) * nx * ny for m in range(8)]
    ins = [inside.reshape(-1)[cubes + corner[m]] for m in range(8)]
    tri = np.full((cubes.size, 6, 2, 3), -1, dtype=np.int64)
    for ti, perm in enumerate(PERMS):
        cc = tet_corners(perm)
        pattern = sum(ins[cc[v]].astype(np.int64) << v for v in range(4))
        for pat in range(1, 15):
            sel = np.nonzero(pattern == pat)[0]
            if sel.size == 0:
                continue
            for n, t3 in enumerate(tet_triangles(pat, perm)):
                for e, (x, y) in enumerate(t3):
                    lo_v, hi_v = min(x, y), max(x, y)
                    code = cc[hi_v] ^ cc[lo_v]
                    P = cubes[sel] + corner[cc[lo_v]]
                    assert np.all(flat[P] & (1 << (code - 1)))       # every edge a triangle names carries a vertex
                    tri[sel, ti, n, e] = first[P] + _POPCOUNT[flat[P] & ((1 << (code - 1)) - 1)]
    tri = tri.reshape(-1, 3)
    tri = tri[tri[:, 0] >= 0]
    assert tri.max(initial=-1) < 2 ** 31
    return verts, tri.astype(np.int32)


# ---- mesh properties ----
def directed_edges(tris):
    """[3m, 2] the directed edges (A,B), (B,C), (C,A) of every triangle"""
    t = np.asarray(tris, dtype=np.int64)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def degenerate(verts, tris):
    """bool per triangle: its three positions are not pairwise distinct"""
    p = verts[tris]
    same = lambda a, b: np.all(p[:, a] == p[:, b], axis=1)      # noqa: E731
    return same(0, 1) | same(1, 2) | same(0, 2)


def repeated_directed_edges(tris):
    """the number of directed edges that occur more than once"""
    e = directed_edges(tris)
    key = e[:, 0] * (int(e.max(initial=0)) + 1) + e[:, 1]
    _, n = np.unique(key, return_counts=True)
    return int((n > 1).sum())


def unreferenced_vertices(nverts, tris):
    used = np.zeros(nverts, dtype=bool)
    used[np.asarray(tris).reshape(-1)] = True
    return int((~used).sum())


def closed_manifold_report(nverts, tris):
    """dict: boundary (directed edges without their opposite), repeated (directed edges occurring twice), euler V-E+F"""
    e = directed_edges(tris)
    big = int(e.max(initial=0)) + 1
    key, back = e[:, 0] * big + e[:, 1], e[:, 1] * big + e[:, 0]
    uniq, n = np.unique(key, return_counts=True)
    boundary = int((~np.isin(back, uniq)).sum())
    und = np.unique(np.minimum(key, back))
    return dict(boundary=boundary, repeated=int((n > 1).sum()), euler=int(nverts) - int(und.size) + int(len(tris)))


def normals64(verts, tris):
    p = verts.astype(np.float64)[tris]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
