"""The contract of exa_hip_lic (include/exa_hip.h) restated in numpy float32, one operation at a time and all lanes (pixel,
direction) of a stage side by side: the lattice coordinates, the plane's metric, E2, the RK4 step in two components, the end
reasons, the noise hash and the outputs exactly as the header words them.  The evaluation E(q) comes from outside, in one of
two ways:

    oracle_evaluator(S, channels)   the CPU oracle's sample_point under the half-open owner rule (streamline_ref.StreamRef):
                                    independent of the module, one point at a time;
    probe_evaluator(R, channels)    Renderer.samplePoints, for larger images: the header defines E(q) as what it returns.

tests/test_lic_ref.py holds the restatement itself (the hash's known answers, a uniform field against a running box sum in
numpy alone, the coverage of the end reasons); tests/test_gpu_lic.py holds the module to it byte for byte."""
import numpy as np

import streamline_ref as sr
from probe_sets import with_field_of_centres

from owlexabrick_amd import scenes

F = np.float32
U = np.uint32
END_MAXSTEPS, END_LEFT, END_NOVALUE, END_STAGNANT, END_IMAGE = 1, 2, 3, 4, 5
KEYS = ("lic", "sum", "count", "speed", "reasons")


def hash_noise(ix, iy, seed):
    """N(ix, iy) of the built-in hash, uint32 arithmetic (arrays or scalars)"""
    with np.errstate(over="ignore"):
        h = np.asarray(ix).astype(U) * U(0x9E3779B1) + np.asarray(iy).astype(U) * U(0x85EBCA77) + U(seed & 0xFFFFFFFF) * U(0xC2B2AE3D)
        h = h ^ (h >> U(16))
        h = h * U(0x7FEB352D)
        h = h ^ (h >> U(15))
        h = h * U(0x846CA68B)
        h = h ^ (h >> U(16))
    return (h >> U(24)).astype(U)


def hash_image(nu, nv, seed):
    """the hash as the noise array a caller would pass: uint8 [nv, nu]"""
    iy, ix = np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij")
    return hash_noise(ix, iy, seed).astype(np.uint8)


def oracle_evaluator(S, channels):
    """E(q) of every row of q from the CPU oracle: (reason [n] (0: a value), v [n, 3])"""
    ref = sr.StreamRef(S, channels, normalize=False)

    def evaluate(q):
        reason, v = np.zeros(len(q), np.int32), np.zeros((len(q), 3), F)
        for k, p in enumerate(q):
            r, val, _ = ref.evaluate(p)
            reason[k] = r
            if not r:
                v[k] = val
        return reason, v
    return evaluate


def probe_evaluator(R, channels):
    """E(q) from Renderer.samplePoints: LEFT where the lookup fails (status -1), NOVALUE where any channel has status -2"""
    def evaluate(q):
        if not len(q):
            return np.zeros(0, np.int32), np.zeros((0, 3), F)
        values, _, status = R.samplePoints(np.ascontiguousarray(q, dtype=F), channels=channels)
        reason = np.where((status == -1).any(axis=1), END_LEFT, np.where((status < 0).any(axis=1), END_NOVALUE, 0)).astype(np.int32)
        return reason, np.where(reason[:, None] == 0, values, F(0)).astype(F)
    return evaluate


def plane(origin, du, dv, size):
    return (np.asarray(origin, F), np.asarray(du, F), np.asarray(dv, F), (int(size[0]), int(size[1])))


def metric(pl):
    """(G11, G12, G22, det) as the header forms them, or None where the plane is refused"""
    _, du, dv, _ = pl
    with np.errstate(all="ignore"):
        dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]          # noqa: E731
        g11, g12, g22 = dot(du, du), dot(du, dv), dot(dv, dv)
        det = g11 * g22 - g12 * g12
    assert det.dtype == F
    return (g11, g12, g22, det) if np.isfinite(det) and det > 0 else None


def lic(evaluate, pl, step, half_length, noise=None, seed=0, fill=np.nan):
    """what Renderer.lic returns: the dict of KEYS, arrays [nv, nu] (reasons [nv, nu, 2])"""
    origin, du, dv, (nu, nv) = pl
    g11, g12, g22, det = metric(pl)
    step, fill = F(step), F(fill)
    n = nu * nv
    N = (lambda ix, iy: np.asarray(noise).reshape(nv, nu)[iy, ix].astype(U)) if noise is not None else (lambda ix, iy: hash_noise(ix, iy, seed))

    def E2(ca, cb):
        """(reason, E gave a value, v, da, db) of the positions (ca, cb)"""
        with np.errstate(all="ignore"):
            q = np.stack([(origin[k] + ca * du[k]) + cb * dv[k] for k in range(3)], axis=1)
            assert q.dtype == F
            r, v = evaluate(q)
            r = r.copy()
            ok = r == 0
            r1 = (v[:, 0] * du[0] + v[:, 1] * du[1]) + v[:, 2] * du[2]
            r2 = (v[:, 0] * dv[0] + v[:, 1] * dv[1]) + v[:, 2] * dv[2]
            va = (g22 * r1 - g12 * r2) / det
            vb = (g11 * r2 - g12 * r1) / det
            s = np.sqrt(va * va + vb * vb)
            assert s.dtype == F
            moving = (s > 0) & np.isfinite(s)
            r[ok & ~moving] = END_STAGNANT
            return r, ok, v, va / s, vb / s

    jj, ii = (x.ravel() for x in np.meshgrid(np.arange(nv), np.arange(nu), indexing="ij"))
    c0a, c0b = ii.astype(F) + F(.5), jj.astype(F) + F(.5)
    r0, ok0, v0, d0a, d0b = E2(c0a, c0b)
    with np.errstate(all="ignore"):
        speed = np.where(ok0, np.sqrt((v0[:, 0] * v0[:, 0] + v0[:, 1] * v0[:, 1]) + v0[:, 2] * v0[:, 2]), fill).astype(F)
    total = np.where(ok0, N(ii, jj), U(0)).astype(U)
    count = ok0.astype(U)
    reasons = np.zeros((n, 2), np.int32)
    for slot, hs in ((0, -step), (1, step)):
        reasons[:, slot] = np.where(r0 != 0, r0, END_MAXSTEPS)
        act = np.nonzero(r0 == 0)[0]                                # the lanes still integrating, and their state
        ca, cb, da, db = c0a[act], c0b[act], d0a[act], d0b[act]

        def keep(mask, *state):
            return [x[mask] for x in state]

        for _ in range(half_length):
            if not len(act):
                break
            with np.errstate(all="ignore"):
                k1a, k1b = hs * da, hs * db
                r, _, _, ea, eb = E2(ca + F(.5) * k1a, cb + F(.5) * k1b)
                reasons[act[r != 0], slot] = r[r != 0]
                act, ca, cb, k1a, k1b, ea, eb = keep(r == 0, act, ca, cb, k1a, k1b, ea, eb)
                k2a, k2b = hs * ea, hs * eb
                r, _, _, ea, eb = E2(ca + F(.5) * k2a, cb + F(.5) * k2b)
                reasons[act[r != 0], slot] = r[r != 0]
                act, ca, cb, k1a, k1b, k2a, k2b, ea, eb = keep(r == 0, act, ca, cb, k1a, k1b, k2a, k2b, ea, eb)
                k3a, k3b = hs * ea, hs * eb
                r, _, _, ea, eb = E2(ca + k3a, cb + k3b)
                reasons[act[r != 0], slot] = r[r != 0]
                act, ca, cb, k1a, k1b, k2a, k2b, k3a, k3b, ea, eb = keep(r == 0, act, ca, cb, k1a, k1b, k2a, k2b, k3a, k3b, ea, eb)
                k4a, k4b = hs * ea, hs * eb
                na = ca + (F(1) / F(6)) * (((k1a + F(2) * k2a) + F(2) * k3a) + k4a)
                nb = cb + (F(1) / F(6)) * (((k1b + F(2) * k2b) + F(2) * k3b) + k4b)
                assert na.dtype == F and nb.dtype == F
                still = (na.view(U) == ca.view(U)) & (nb.view(U) == cb.view(U))
                reasons[act[still], slot] = END_STAGNANT
                act, na, nb = keep(~still, act, na, nb)
                inside = (na >= F(0)) & (na < F(nu)) & (nb >= F(0)) & (nb < F(nv))
                reasons[act[~inside], slot] = END_IMAGE
                act, na, nb = keep(inside, act, na, nb)
                r, _, _, ea, eb = E2(na, nb)
                reasons[act[r != 0], slot] = r[r != 0]
                act, ca, cb, da, db = keep(r == 0, act, na, nb, ea, eb)
                np.add.at(total, act, N(ca.astype(np.int32), cb.astype(np.int32)))
                np.add.at(count, act, U(1))
    with np.errstate(all="ignore"):
        image = np.where(count > 0, total.astype(F) / count.astype(F), fill).astype(F)
    return dict(lic=image.reshape(nv, nu), sum=total.reshape(nv, nu), count=count.reshape(nv, nu), speed=speed.reshape(nv, nu),
                reasons=reasons.reshape(nv, nu, 2))


def same(got, want, what=""):
    """every array of KEYS byte for byte"""
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == F:
            a, b = a.view(U), b.view(U)
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5])


def reason_counts(res):
    """{reason: number of directions that ended with it}, and the pixels whose centre failed / stagnated"""
    r = np.asarray(res["reasons"])
    n = {k: int((r == k).sum()) for k in (END_MAXSTEPS, END_LEFT, END_NOVALUE, END_STAGNANT, END_IMAGE)}
    n["failed_centre"] = int((res["count"] == 0).sum())
    n["stagnant_centre"] = int(((res["count"] == 1) & (r == END_STAGNANT).all(axis=2)).sum())
    return n


# ---- a uniform field along du on an axis-aligned plane: the closed form, numpy alone ----
def uniform_closed_form(noise, step, half_length):
    """sum, count, reasons of a field along +u everywhere in the image, du and dv unit axes, for a step with which the RK4
    step lands exactly on a + step: position k of a direction is a0 +- k*step, kept while it lies in [0, nu); a clipped
    running box sum of the noise rows"""
    noise = np.asarray(noise)
    nv, nu = noise.shape
    a0 = np.arange(nu, dtype=np.float64) + 0.5
    k = np.arange(1, half_length + 1, dtype=np.float64)
    total = noise.astype(np.int64)                                           # the centre's own sample
    count = np.ones((nv, nu), np.int64)
    reasons = np.zeros((nv, nu, 2), np.int32)
    for slot, sign in ((0, -1.0), (1, 1.0)):
        a = a0[:, None] + sign * float(step) * k[None, :]                    # [nu, L]: exact in float64 and in float32
        assert np.array_equal(a.astype(F).astype(np.float64), a)
        inside = (a >= 0) & (a < nu)
        taken = np.cumprod(inside, axis=1).astype(bool)                     # up to the first position outside
        idx = np.where(taken, np.floor(a), 0).astype(np.int64)
        total += (noise.astype(np.int64)[:, idx] * taken[None]).sum(axis=2)
        count += taken.sum(axis=1)[None, :]
        reasons[:, :, slot] = np.where(taken.all(axis=1), END_MAXSTEPS, END_IMAGE)[None, :]
    return total.astype(U), count.astype(U), reasons


def uniform_scene(cells_x=18):
    """one level, 4*cells_x x 8 x 8 voxels; fields 1..3 = (1, 0, 0)"""
    sc = scenes.amr(levels=1, root=(cells_x, 2, 2), B=4)
    sc = with_field_of_centres(sc, lambda c: np.ones(len(c)))
    sc = with_field_of_centres(sc, lambda c: np.zeros(len(c)))
    return with_field_of_centres(sc, lambda c: np.zeros(len(c)))


def uniform_plane(nu, nv):
    """pixel centres at (2.5 + i, 2.5 + j, 3.25): inside uniform_scene for nu <= 4*cells_x - 4, nv <= 4"""
    return plane((2, 2, 3.25), (1, 0, 0), (0, 1, 0), (nu, nv))


# ---- the inputs the reference tests and the GPU tests share: (name, scene, channels, forms, empty cells, plane, step, L) ----
def normal_field_scene():
    """rotation_scene's volume with fields 1..3 = (0, 0, 1): normal to a z plane, every centre stagnates"""
    sc = scenes.amr(levels=1, root=(3, 3, 2), B=4)
    sc = with_field_of_centres(sc, lambda c: np.zeros(len(c)))
    sc = with_field_of_centres(sc, lambda c: np.zeros(len(c)))
    return with_field_of_centres(sc, lambda c: np.ones(len(c)))


def oblique_plane():
    """9 x 7 pixels through the middle of amr(levels=3) (48 x 48 x 32), tilted against every axis and wider than the volume on
    one side"""
    return plane((2.0, 5.0, 9.0), (5.5, 1.25, 0.75), (-1.0, 6.0, 2.0), (9, 7))


CASES = [
    ("rotation", sr.rotation_scene, (1, 2, 3), (0, 1), False, plane((-2, -1.5, 2.25), (1, 0, 0), (0, 1, 0), (16, 12)), 0.5, 6),
    ("amr3_oblique", lambda: scenes.amr(levels=3, fields=4), (1, 3, 0), (0, 1), False, oblique_plane(), 0.5, 6),
    ("amr3_holes", lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=3), fraction=0.15), (0, 1, 2), (0,), True,
     plane((8, 10, 15.5), (1, 0, 0), (0, 1, 0), (24, 20)), 0.5, 5),      # the centre plane of a layer of fine cells: empty rows
    ("zero", sr.zero_fields_scene, (1, 2, 3), (1,), False, plane((3, 3, 7.6), (4, 0, 0), (0, 4, 0), (6, 5)), 0.5, 4),
    ("normal", normal_field_scene, (1, 2, 3), (0, 1), False, plane((1, 1, 2.25), (1, 0, 0), (0, 1, 0), (7, 6)), 0.5, 4),
]
