"""The contract of exa_hip_project (include/exa_hip.h) restated in numpy: the float32 positions of the samples, operation for
operation in the header's association, and the reduction of a pixel's samples.  What a sample IS comes from outside: the
(values, status) that the existing point probe (Renderer.samplePoints) returns at those positions — so the reference of the
ray kernel is the points kernel, which tests/probe_ref64.py holds to float64, and never the new call itself.

Rays are a dict with the keywords of binding.Renderer.project: org, orgDu, orgDv, dir, dirDu, dirDv (3 floats each),
size = (width, height), tmin, dt, num_samples."""
import numpy as np

f32 = np.float32


def rays(org, dir, size, tmin, dt, num_samples, orgDu=(0, 0, 0), orgDv=(0, 0, 0), dirDu=(0, 0, 0), dirDv=(0, 0, 0)):
    v = lambda a: np.asarray(a, dtype=f32).reshape(3)                       # noqa: E731
    return dict(org=v(org), orgDu=v(orgDu), orgDv=v(orgDv), dir=v(dir), dirDu=v(dirDu), dirDv=v(dirDv),
                size=(int(size[0]), int(size[1])), tmin=f32(tmin), dt=f32(dt), num_samples=int(num_samples))


def origins_and_directions(r, normalize=False):
    """(o [H,W,3], d [H,W,3], has [H,W]): numpy's float32 multiply, add, sqrt and divide are correctly rounded, each call
    one operation; has = False where normalisation leaves the pixel without samples"""
    W, H = r["size"]
    sx = (np.arange(W, dtype=f32) + f32(0.5))[None, :, None]
    sy = (np.arange(H, dtype=f32) + f32(0.5))[:, None, None]
    with np.errstate(all="ignore"):
        o = (r["org"].astype(f32) + sx * r["orgDu"].astype(f32)) + sy * r["orgDv"].astype(f32)
        d = (r["dir"].astype(f32) + sx * r["dirDu"].astype(f32)) + sy * r["dirDv"].astype(f32)
        o, d = np.broadcast_to(o, (H, W, 3)).astype(f32), np.broadcast_to(d, (H, W, 3)).astype(f32)
        has = np.ones((H, W), dtype=bool)
        if normalize:
            s = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], dtype=f32)
            has = (s > 0) & np.isfinite(s)
            d = (d / s[..., None]).astype(f32)
    assert o.dtype == f32 and d.dtype == f32
    return o, d, has


def times(r):
    """t_i = tmin + (float(i) + 0.5f) * dt"""
    with np.errstate(all="ignore"):
        t = f32(r["tmin"]) + (np.arange(r["num_samples"], dtype=f32) + f32(0.5)) * f32(r["dt"])
    assert t.dtype == f32
    return t


def positions(r, normalize=False):
    """(p [H,W,N,3] float32, has [H,W]): p_i = o + t_i * d per component"""
    o, d, has = origins_and_directions(r, normalize)
    t = times(r)
    with np.errstate(all="ignore"):
        p = o[:, :, None, :] + t[None, None, :, None] * d[:, :, None, :]
    assert p.dtype == f32
    return p, has


def reduce(values, status):
    """the reduction over the last axis: values float32 [..., N], status int [..., N] (valid where >= 0).  Returns the
    dict of Renderer.project: sum float64, count uint32, max, min float32, max_index int32, shaped like values[..., 0].

    sum: a sequential float64 accumulation (np.cumsum adds along the axis in order) started at +0.0 over the valid values.
    The invalid ones are skipped by adding +0.0 in their place, which is the same thing bit for bit: x + 0.0 == x for every
    x but -0.0, and the accumulator, started at +0.0, can never be -0.0 (a sum is -0.0 only if both terms are)."""
    values = np.asarray(values, dtype=f32)
    valid = np.asarray(status) >= 0
    shape, n = values.shape[:-1], values.shape[-1]
    v, ok = values.reshape(-1, n), valid.reshape(-1, n)
    terms = np.concatenate([np.zeros((len(v), 1)), np.where(ok, v, f32(0)).astype(np.float64)], axis=1)
    with np.errstate(all="ignore"):
        total = np.cumsum(terms, axis=1)[:, -1]
    count = ok.sum(axis=1).astype(np.uint32)
    rows = np.arange(len(v))

    def extreme(cand, key):
        """the value and index of the first candidate that no other candidate beats; key: larger is better"""
        k = np.where(cand, key, -np.inf)
        best = k.max(axis=1, initial=-np.inf)
        first = np.argmax(cand & (k == best[:, None]), axis=1)               # equal values (also -0.0 and +0.0): the first
        some = cand.any(axis=1)
        return some, first

    num = ok & ~np.isnan(v)
    with np.errstate(all="ignore"):
        some, first = extreme(num & (v > -np.inf), v.astype(np.float64))   # `v > vmax` from -inf: -inf itself never wins
        vmax = np.where(some, v[rows, first], f32(-np.inf)).astype(f32)
        max_index = np.where(some, first, -1).astype(np.int32)
        some, first = extreme(num & (v < np.inf), -v.astype(np.float64))
        vmin = np.where(some, v[rows, first], f32(np.inf)).astype(f32)
    return dict(sum=total.reshape(shape), count=count.reshape(shape), max=vmax.reshape(shape), min=vmin.reshape(shape),
                max_index=max_index.reshape(shape))


def reduce_literal(values, status):
    """one pixel, the contract's loop as written (tests/test_project_ref.py holds reduce against it)"""
    total, count, vmax, vmin, max_index = np.float64(0.0), 0, f32(-np.inf), f32(np.inf), -1
    with np.errstate(all="ignore"):
        for i, (v, st) in enumerate(zip(np.asarray(values, dtype=f32), status)):
            if st < 0:
                continue
            count += 1
            total = total + np.float64(v)
            if v > vmax:
                vmax, max_index = v, i
            if v < vmin:
                vmin = v
    return dict(sum=total, count=np.uint32(count), max=vmax, min=vmin, max_index=np.int32(max_index))


def project(sample, r, normalize=False):
    """the reference projection: sample(points [n,3]) -> (values [n], status [n]) is the existing point probe.  Returns
    (dict of [H,W] arrays, values [H,W,N], status [H,W,N])"""
    p, has = positions(r, normalize)
    H, W, N, _ = p.shape
    values, status = sample(np.ascontiguousarray(p.reshape(-1, 3)))
    values = np.asarray(values, dtype=f32).reshape(H, W, N)
    status = np.array(status, dtype=np.int64).reshape(H, W, N)
    status[~has] = -1                                                       # a pixel without a direction has no samples
    return reduce(values, status), values, status


def same_bits(a, b):
    """equal shape, dtype and bytes (NaN payloads and the sign of zero included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
