"""exa_hip_critical_points restated in numpy from the contract in include/exa_hip.h (not a test module, and written from the
header, not from the kernels): three float32 lattices in, the records, the stats and the order of the candidates out.  Every
float32 step is a float32 numpy operation of its own, in the header's association; the classification is float64."""
import numpy as np

F32 = np.float32
SPIRAL, DEGENERATE = 4, 8
FOUND, NON_FINITE, LEFT_CELL, NOT_CONVERGED = 0, 1, 2, 3
POINT_DTYPE = np.dtype(dict(names=["cell", "type", "local", "position", "lastStep", "jacobian", "invariants", "discriminant"],
                            formats=["<u4", "<i4", ("<f4", 3), ("<f4", 3), "<f4", ("<f4", 9), ("<f8", 3), "<f8"],
                            offsets=[0, 4, 8, 20, 32, 36, 72, 96], itemsize=104))
STATS = ("cells", "invalidCells", "candidates", "found", "nonFinite", "leftCell", "notConverged")


def _corner(V, m):
    """the values at corner m = dx + 2 dy + 4 dz of every cell, [nz-1, ny-1, nx-1]"""
    nz, ny, nx = V.shape
    dx, dy, dz = m & 1, (m >> 1) & 1, m >> 2
    return V[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]


def interpolant(corners, s):
    """F [n,3] and J [n,3,3] (J[:, c, a] = dT_c/ds_a) of the cells with corner values corners [n,3,8] at s [n,3], float32,
    accumulated corner by corner as the header words it"""
    n = s.shape[0]
    u = [(F32(1) - s[:, a], s[:, a]) for a in range(3)]
    Fv, J = np.zeros((n, 3), F32), np.zeros((n, 3, 3), F32)
    for m in range(8):
        dx, dy, dz = m & 1, (m >> 1) & 1, m >> 2
        wxy, wxz, wyz = u[0][dx] * u[1][dy], u[0][dx] * u[2][dz], u[1][dy] * u[2][dz]
        w = wxy * u[2][dz]
        for c in range(3):
            v = corners[:, c, m]
            Fv[:, c] = Fv[:, c] + w * v
            for a, (d, wa) in enumerate(((dx, wyz), (dy, wxz), (dz, wxy))):
                t = wa * v
                J[:, c, a] = J[:, c, a] + (t if d else -t)
    return Fv, J


def newton_step(corners, s):
    """one step of the header's iteration: the new s and delta, [n,3] float32"""
    Fv, J = interpolant(corners, s)
    j = lambda r, c: J[:, r, c]                                                  # noqa: E731
    A = [[j(1, 1) * j(2, 2) - j(1, 2) * j(2, 1), j(0, 2) * j(2, 1) - j(0, 1) * j(2, 2), j(0, 1) * j(1, 2) - j(0, 2) * j(1, 1)],
         [j(1, 2) * j(2, 0) - j(1, 0) * j(2, 2), j(0, 0) * j(2, 2) - j(0, 2) * j(2, 0), j(0, 2) * j(1, 0) - j(0, 0) * j(1, 2)],
         [j(1, 0) * j(2, 1) - j(1, 1) * j(2, 0), j(0, 1) * j(2, 0) - j(0, 0) * j(2, 1), j(0, 0) * j(1, 1) - j(0, 1) * j(1, 0)]]
    det = (A[0][0] * j(0, 0) + A[0][1] * j(1, 0)) + A[0][2] * j(2, 0)
    delta = np.stack([-(((A[a][0] * Fv[:, 0] + A[a][1] * Fv[:, 1]) + A[a][2] * Fv[:, 2]) / det) for a in range(3)], axis=1)
    return s + delta, delta


def classify(jac):
    """(type, invariants [n,3], discriminant [n]) of float32 jacobians [n,9], in float64 as the header words it"""
    j = jac.astype(np.float64).T
    P = -((j[0] + j[4]) + j[8])
    Q = ((j[0] * j[4] - j[1] * j[3]) + (j[0] * j[8] - j[2] * j[6])) + (j[4] * j[8] - j[5] * j[7])
    R = -((j[0] * (j[4] * j[8] - j[5] * j[7]) - j[1] * (j[3] * j[8] - j[5] * j[6])) + j[2] * (j[3] * j[7] - j[4] * j[6]))
    D = (27.0 * (R * R) + (4.0 * ((P * P) * P) - 18.0 * (P * Q)) * R) + (4.0 * ((Q * Q) * Q) - (P * P) * (Q * Q))
    num = P * Q - R
    e2 = num / P
    pos = [np.ones(P.shape, bool), P > 0, e2 > 0, R > 0]
    nplus = sum((pos[k] != pos[k + 1]).astype(np.int32) for k in range(3))
    degenerate = (P == 0) | (num == 0) | (R == 0) | ~(np.isfinite(P) & np.isfinite(e2) & np.isfinite(R))
    kind = nplus | np.where(D > 0, SPIRAL, 0) | np.where(degenerate, DEGENERATE, 0)
    return kind.astype(np.int32), np.stack([P, Q, R], axis=1), D


def critical_points(V, lo, hi, iterations=8, tolerance=2.0 ** -10):
    """V: the three lattices, float32 [nz, ny, nx] each (what resample(lo, hi, dims, channels[c]) returns).  Returns
    (records POINT_DTYPE, stats dict, order): order = dict(cells = the candidates' cell numbers, ascending; result = FOUND /
    NON_FINITE / LEFT_CELL / NOT_CONVERGED of each)."""
    V = [np.ascontiguousarray(v, dtype=F32) for v in V]
    nz, ny, nx = V[0].shape
    assert min(nx, ny, nz) >= 2 and all(v.shape == (nz, ny, nx) for v in V)
    lo, hi = np.asarray(lo, F32), np.asarray(hi, F32)
    step = (hi - lo) / np.array([nx, ny, nz], F32)
    with np.errstate(all="ignore"):
        valid = np.ones((nz - 1, ny - 1, nx - 1), bool)
        cand = np.ones_like(valid)
        for c in range(3):
            cs = np.stack([_corner(V[c], m) for m in range(8)])
            valid &= np.isfinite(cs).all(axis=0)
            mn, mx = cs.min(axis=0), cs.max(axis=0)
            cand &= (mn <= 0) & (0 <= mx) & (mn < mx)
        cand &= valid
        k, j, i = np.nonzero(cand)                                                # C order: ascending cell number
        cells = ((k * ny + j) * nx + i).astype(np.uint32)
        n = cells.size
        corners = np.empty((n, 3, 8), F32)
        for c in range(3):
            for m in range(8):
                corners[:, c, m] = _corner(V[c], m)[k, j, i]
        s = np.full((n, 3), 0.5, F32)
        delta = np.zeros((n, 3), F32)
        for _ in range(int(iterations)):
            s, delta = newton_step(corners, s)
        finite = np.isfinite(s).all(axis=1) & np.isfinite(delta).all(axis=1)
        idx = np.stack([i, j, k], axis=1)
        last = idx == np.array([nx - 2, ny - 2, nz - 2])
        inside = ((s >= 0) & ((s < 1) | (last & (s <= 1)))).all(axis=1)
        last_step = np.maximum(np.maximum(np.abs(delta[:, 0]), np.abs(delta[:, 1])), np.abs(delta[:, 2]))
        result = np.where(~finite, NON_FINITE, np.where(~inside, LEFT_CELL, np.where(~(last_step <= F32(tolerance)), NOT_CONVERGED, FOUND)))
        f = result == FOUND
        rec = np.zeros(int(f.sum()), POINT_DTYPE)
        rec["cell"] = cells[f]
        rec["local"] = s[f]
        rec["position"] = lo + ((idx[f].astype(F32) + F32(0.5)) + s[f]) * step
        rec["lastStep"] = last_step[f]
        _, J = interpolant(corners[f], s[f])
        rec["jacobian"] = (J / step).reshape(-1, 9)
        rec["type"], rec["invariants"], rec["discriminant"] = classify(rec["jacobian"])
    stats = dict(cells=(nx - 1) * (ny - 1) * (nz - 1), invalidCells=int((~valid).sum()), candidates=int(n), found=int(f.sum()),
                 nonFinite=int((result == NON_FINITE).sum()), leftCell=int((result == LEFT_CELL).sum()),
                 notConverged=int((result == NOT_CONVERGED).sum()))
    return rec, stats, dict(cells=cells, result=result.astype(np.int32))
