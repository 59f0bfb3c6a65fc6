"""The contract of exa_hip_raycast_iso (include/exa_hip.h) restated in numpy, float32 operation for operation: the crossings of
a value along the rays of exa_hip_project (tests/project_ref.py forms the positions), the bisection of the first crossing's
bracket and the interpolation, the value and gradient at the hit.  What a sample IS comes from outside, as in project_ref:

    sample(points [n,3])                 -> (values [n], status [n])
    sample(points [n,3], gradient=True)  -> (values [n], gradients [n,3], status [n])

— on the GPU the existing point probe (Renderer.samplePoints; with gradient=True its normalized gradient), on the CPU any
function of the position.  The rounds of the refinement are batched over the rays: one round is one call of the sampler."""
import numpy as np

import project_ref as pr

f32 = np.float32
KEYS = ("t", "position", "value", "gradient", "index", "side", "crossings")
same_bits = pr.same_bits


def usable(values, status):
    """a sample counts if its status is >= 0 and its value is not NaN"""
    return (np.asarray(status) >= 0) & ~np.isnan(np.asarray(values, dtype=f32))


def crossing_mask(values, ok, iso):
    """[..., N] bool: index i >= 1 is a crossing if samples i-1 and i are both usable and on different sides of iso
    (inside(v) = v >= iso); index 0 never is"""
    with np.errstate(invalid="ignore"):
        inside = np.asarray(values, dtype=f32) >= f32(iso)
    cross = np.zeros(ok.shape, dtype=bool)
    cross[..., 1:] = ok[..., 1:] & ok[..., :-1] & (inside[..., 1:] != inside[..., :-1])
    return cross


def raycast(sample, r, iso, refine, normalize=False, fill=np.nan):
    """the reference: (dict of the arrays of KEYS, shaped [H,W] or [H,W,3], and a dict of what the tests look at beside them:
    values, status [H,W,N] of the march; rows = the flat pixel indices with a crossing; brackets = per round the (ta, va, tb,
    vb) of those rows AFTER the round (entry 0: before the first); ended_collapsed / ended_unusable = those rows whose
    refinement stopped early on tm == ta or tb / on an unusable midpoint)"""
    iso, fill = f32(iso), f32(fill)
    assert np.isfinite(iso) and 0 <= refine <= 32
    p, has = pr.positions(r, normalize)
    o, d, _ = pr.origins_and_directions(r, normalize)
    t = pr.times(r)
    H, W, N, _ = p.shape
    out = sample(np.ascontiguousarray(p.reshape(-1, 3)))
    values = np.asarray(out[0], dtype=f32).reshape(H * W, N)
    status = np.array(out[1], dtype=np.int64).reshape(H * W, N)
    status[~has.reshape(-1)] = -1                                           # a pixel without a direction has no samples
    ok = usable(values, status)
    cross = crossing_mask(values, ok, iso)
    crossings = cross.sum(axis=1).astype(np.uint32)
    index = np.where(crossings > 0, np.argmax(cross, axis=1), -1).astype(np.int32)
    rows = np.flatnonzero(index >= 0)
    i = index[rows]
    ta, va, tb, vb = t[i - 1].copy(), values[rows, i - 1].copy(), t[i].copy(), values[rows, i].copy()
    side = np.zeros(H * W, dtype=np.int32)
    side[rows] = np.where(va < iso, 1, -1)
    ro, rd = o.reshape(-1, 3)[rows], d.reshape(-1, 3)[rows]

    active = np.ones(len(rows), dtype=bool)
    collapsed, unusable = np.zeros(len(rows), dtype=bool), np.zeros(len(rows), dtype=bool)
    brackets = [(ta.copy(), va.copy(), tb.copy(), vb.copy())]
    with np.errstate(all="ignore"):
        for _ in range(refine):
            tm = f32(0.5) * (ta + tb)
            stop = active & ((tm == ta) | (tm == tb))
            collapsed |= stop
            active &= ~stop
            k = np.flatnonzero(active)
            if len(k):
                pm = ro[k] + tm[k, None] * rd[k]
                assert pm.dtype == f32
                vm, st = sample(np.ascontiguousarray(pm))[:2]
                vm = np.asarray(vm, dtype=f32)
                good = usable(vm, st)
                unusable[k[~good]] = True
                active[k[~good]] = False
                k, vm = k[good], vm[good]
                low = (vm >= iso) == (va[k] >= iso)
                ta[k[low]], va[k[low]] = tm[k[low]], vm[low]
                tb[k[~low]], vb[k[~low]] = tm[k[~low]], vm[~low]
            brackets.append((ta.copy(), va.copy(), tb.copy(), vb.copy()))
        s = (iso - va) / (vb - va)
        th = ta + s * (tb - ta)
        pos = ro + th[:, None] * rd
    assert th.dtype == f32 and pos.dtype == f32

    res = dict(t=np.full(H * W, fill, f32), position=np.full((H * W, 3), fill, f32), value=np.full(H * W, fill, f32),
               gradient=np.full((H * W, 3), fill, f32), index=index, side=side, crossings=crossings)
    if len(rows):
        v, g, st = sample(np.ascontiguousarray(pos), gradient=True)
        valid = np.asarray(st) >= 0                                         # the probe's own rule: `fill` where status < 0
        res["t"][rows], res["position"][rows] = th, pos
        res["value"][rows] = np.where(valid, np.asarray(v, dtype=f32), fill)
        res["gradient"][rows] = np.where(valid[:, None], np.asarray(g, dtype=f32).reshape(-1, 3), fill)
    res = {k: a.reshape((H, W) + a.shape[1:]) for k, a in res.items()}
    info = dict(values=values.reshape(H, W, N), status=status.reshape(H, W, N), rows=rows, brackets=brackets,
                ended_collapsed=collapsed, ended_unusable=unusable)
    return res, info
