"""The contract of exa_hip_flowmap (include/exa_hip.h) restated in numpy float32, one operation at a time: the lattice positions,
the flow map (end point, step count and reason of the one-direction line of exa_hip_streamlines from every lattice point),
validity, the stencil, the Cauchy-Green tensor, five sweeps of cyclic Jacobi and the maximum, exactly as the header words them;
and ftle(), the formula the upper layers apply.  The flow map is fed in one of two ways:

    oracle_flow_map(S, channels, ...)   streamline_ref.StreamRef(S, channels).direction(...), the CPU oracle, point by point:
                                        independent of the module;
    stepper_flow_map(evaluate, ...)     the same step for all points side by side on an evaluation E(q) from outside —
                                        lic_ref.probe_evaluator(R, channels) for larger lattices and long integrations (the
                                        header defines E(q) as what the point probes return), or lic_ref.oracle_evaluator.

tests/test_flowmap_ref.py holds the restatement itself (Jacobi against float64 eigenvalues, a rigid rotation, a saddle's closed
form, the two feeds against each other, the coverage of the GPU test's inputs); tests/test_gpu_flowmap.py holds the module to
it byte for byte."""
import numpy as np

import streamline_ref as sr
from probe_sets import with_field_of_centres

from owlexabrick_amd import scenes

F = np.float32
U = np.uint32
END_MAXSTEPS, END_LEFT, END_NOVALUE, END_STAGNANT = 1, 2, 3, 4
KEYS = ("end", "steps", "reasons", "stretch")
SWEEPS = 5


# ---- the lattice ----
def axis_coords(lo, hi, dims):
    """per axis the coordinates lo + (float(i) + 0.5f) * ((hi - lo) / float(n)) of exa_hip_resample's lattice"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    out = [lo[k] + (np.arange(dims[k], dtype=F) + F(0.5)) * ((hi[k] - lo[k]) / F(dims[k])) for k in range(3)]
    assert all(c.dtype == F for c in out)
    return out


def positions(lo, hi, dims):
    """P(L) [n, 3], L = (k*ny + j)*nx + i"""
    x, y, z = axis_coords(lo, hi, dims)
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1).astype(F)


# ---- the flow map ----
def oracle_flow_map(S, channels, P, hs, num_steps):
    """(end [n, 3], steps [n], reasons [n], seed_ok [n]) from the CPU oracle's line of every point, one direction"""
    ref = sr.StreamRef(S, channels, normalize=False)
    n = len(P)
    end, steps, reasons, seed_ok = np.zeros((n, 3), F), np.zeros(n, U), np.zeros(n, np.int32), np.zeros(n, bool)
    for L, p in enumerate(P):
        verts, _, reason, ok = ref.direction(p, F(hs), num_steps)
        end[L], steps[L], reasons[L], seed_ok[L] = verts[-1], len(verts) - 1, reason, ok
    return end, steps, reasons, seed_ok


def stepper_flow_map(evaluate, P, hs, num_steps):
    """the same from evaluate(q [m, 3]) -> (reason [m] (0: a value), v [m, 3]), all points of a stage side by side: the step of
    exa_hip_streamlines' "One direction" paragraph without EXA_STREAM_NORMALIZE"""
    hs = F(hs)
    n = len(P)
    end, steps, reasons = np.array(P, dtype=F), np.zeros(n, U), np.full(n, END_MAXSTEPS, np.int32)
    r, v = evaluate(end)
    reasons[r != 0] = r[r != 0]
    seed_ok = r == 0
    act = np.nonzero(seed_ok)[0]
    p, d = end[act], v[act].astype(F)

    def stage(q, *state):
        """evaluates q; the lanes that fail end with that reason; the others' state and their d(q)"""
        r, v = evaluate(np.ascontiguousarray(q))
        reasons[act[r != 0]] = r[r != 0]
        return [x[r == 0] for x in (act, v.astype(F)) + state]

    for _ in range(num_steps):
        if not len(act):
            break
        with np.errstate(all="ignore"):
            k1 = hs * d
            act, d2, p, k1 = stage(p + F(.5) * k1, p, k1)
            k2 = hs * d2
            act, d3, p, k1, k2 = stage(p + F(.5) * k2, p, k1, k2)
            k3 = hs * d3
            act, d4, p, k1, k2, k3 = stage(p + k3, p, k1, k2, k3)
            k4 = hs * d4
            pn = p + (F(1) / F(6)) * (((k1 + F(2) * k2) + F(2) * k3) + k4)
            assert pn.dtype == F
        still = (pn.view(U) == p.view(U)).all(axis=1)
        reasons[act[still]] = END_STAGNANT
        act, pn = act[~still], pn[~still]
        act, d, p = stage(pn, pn)
        end[act] = p
        steps[act] += U(1)
    return end, steps, reasons, seed_ok


# ---- the stretch ----
def valid(reasons):
    return (reasons == END_MAXSTEPS) | (reasons == END_STAGNANT)


def stencil_valid(reasons):
    """whether every stencil point of a point is valid: per axis of two points or more (reasons [nz, ny, nx]) the neighbours at
    max(i - 1, 0) and min(i + 1, n - 1)"""
    ok = valid(reasons)
    out = np.ones(ok.shape, bool)
    for ax in range(3):
        n = ok.shape[ax]
        if n >= 2:
            idx = np.arange(n)
            out &= np.take(ok, np.maximum(idx - 1, 0), axis=ax) & np.take(ok, np.minimum(idx + 1, n - 1), axis=ax)
    return out


def _column(end, coords, axis):
    """column `axis` of F at every point ([nz, ny, nx, 3]); axis 0 = x is array axis 2"""
    n = len(coords)
    if n < 2:
        return np.zeros_like(end)
    idx = np.arange(n)
    im, ip = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
    ax = 2 - axis
    shape = [1, 1, 1, 1]
    shape[ax] = n
    with np.errstate(all="ignore"):
        dP = (coords[ip] - coords[im]).reshape(shape)
        col = (np.take(end, ip, axis=ax) - np.take(end, im, axis=ax)) / dP
    assert col.dtype == F
    return col


def tensor(Fx, Fy, Fz):
    """the six entries (00, 11, 22, 01, 02, 12) of C = F^T F from the columns [..., 3] of F"""
    cols = (Fx, Fy, Fz)

    def entry(a, b):
        with np.errstate(all="ignore"):
            return (cols[a][..., 0] * cols[b][..., 0] + cols[a][..., 1] * cols[b][..., 1]) + cols[a][..., 2] * cols[b][..., 2]
    return entry(0, 0), entry(1, 1), entry(2, 2), entry(0, 1), entry(0, 2), entry(1, 2)


def _rotate(app, aqq, apq, arp, arq):
    """one rotation (p, q), r the third index; skipped iff a_pq == 0.0f"""
    with np.errstate(all="ignore"):
        theta = (aqq - app) / (F(2) * apq)
        t = np.copysign(F(1), theta) / (np.abs(theta) + np.sqrt(theta * theta + F(1)))
        c = F(1) / np.sqrt(t * t + F(1))
        s = t * c
        tp = t * apq
        new = (app - tp, aqq + tp, np.zeros_like(apq), c * arp - s * arq, s * arp + c * arq)
    assert all(x.dtype == F for x in new)
    skip = apq == F(0)
    return tuple(np.where(skip, old, x) for old, x in zip((app, aqq, apq, arp, arq), new))


def jacobi_max(a00, a11, a22, a01, a02, a12, sweeps=SWEEPS):
    """the largest diagonal entry after `sweeps` sweeps of cyclic Jacobi, rotations (0,1), (0,2), (1,2); float32 arrays"""
    a00, a11, a22, a01, a02, a12 = (np.asarray(x, F) for x in (a00, a11, a22, a01, a02, a12))
    for _ in range(sweeps):
        a00, a11, a01, a02, a12 = _rotate(a00, a11, a01, a02, a12)
        a00, a22, a02, a01, a12 = _rotate(a00, a22, a02, a01, a12)
        a11, a22, a12, a01, a02 = _rotate(a11, a22, a12, a01, a02)
    m = a00
    with np.errstate(invalid="ignore"):
        m = np.where(a11 > m, a11, m)
        m = np.where(a22 > m, a22, m)
    return m.astype(F)


def stretch(end, reasons, lo, hi, dims, fill=np.nan):
    """stretch [nz, ny, nx] of the flow map end [n, 3], reasons [n]"""
    nx, ny, nz = dims
    end = np.asarray(end, F).reshape(nz, ny, nx, 3)
    reasons = np.asarray(reasons).reshape(nz, ny, nx)
    coords = axis_coords(lo, hi, dims)
    cols = [_column(end, coords[axis], axis) for axis in range(3)]
    return np.where(valid(reasons) & stencil_valid(reasons), jacobi_max(*tensor(*cols)), F(fill)).astype(F)


def ftle(stretch, step, num_steps, fill=np.nan):
    """FTLE = log(stretch) / (2 |T|), T = num_steps * step, formed in double and rounded to float32; fill where stretch is"""
    stretch = np.ascontiguousarray(stretch, dtype=F)
    with np.errstate(all="ignore"):
        out = (np.log(stretch.astype(np.float64)) / (2.0 * num_steps * np.float64(F(step)))).astype(F)
    return np.where(stretch.view(U) == F(fill).view(U), F(fill), out).astype(F)


def flowmap(feed, lo, hi, dims, step, num_steps, backward=False, fill=np.nan):
    """what Renderer.flowmap returns (without ftle), and seed_ok; feed(P, hs, num_steps) is one of the two flow maps"""
    nx, ny, nz = dims
    end, steps, reasons, seed_ok = feed(positions(lo, hi, dims), -F(step) if backward else F(step), num_steps)
    return dict(end=end.reshape(nz, ny, nx, 3), steps=steps.reshape(nz, ny, nx), reasons=reasons.reshape(nz, ny, nx),
                stretch=stretch(end, reasons, lo, hi, dims, fill), seed_ok=seed_ok.reshape(nz, ny, nx))


def oracle_feed(S, channels):
    return lambda P, hs, num_steps: oracle_flow_map(S, channels, P, hs, num_steps)


def stepper_feed(evaluate):
    return lambda P, hs, num_steps: stepper_flow_map(evaluate, P, hs, num_steps)


def with_fill(res, fill):
    """the result with another fill: the flow map does not depend on it"""
    has = valid(res["reasons"]) & stencil_valid(res["reasons"])
    return dict(res, stretch=np.where(has, res["stretch"], F(fill)).astype(F))


def same(got, want, what=""):
    """every array of KEYS byte for byte"""
    for k in KEYS:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.dtype == F:
            a, b = a.view(U), b.view(U)
        assert np.array_equal(a, b), (what, k, np.argwhere(a != b)[:5])


def coverage(res):
    """{what: number of lattice points}: every reason, the failed seeds, the points invalid only through a neighbour, and per
    axis the points with a stretch on a face of the lattice (a one-sided stencil)"""
    r, ok = res["reasons"], valid(res["reasons"])
    has = ok & stencil_valid(r)
    n = {k: int((r == k).sum()) for k in (END_MAXSTEPS, END_LEFT, END_NOVALUE, END_STAGNANT)}
    n["failed_seed"] = int((~res["seed_ok"]).sum())
    n["through_neighbour"] = int((ok & ~has).sum())
    n["stretch"] = int(has.sum())
    for axis, name in enumerate("xyz"):
        ax = 2 - axis
        if r.shape[ax] >= 2:
            n["one_sided_" + name] = int(np.take(has, [0, r.shape[ax] - 1], axis=ax).sum())
    return n


# ---- the scenes of the reference tests ----
def saddle_scene():
    """rotation_scene's volume (one level, 12 x 12 x 8 voxels) with fields 1..3 = (x - 6, -(y - 6), 0): the hat reconstruction of
    a linear field is exact at least half a cell inside, in [0.5, 11.5] x [0.5, 11.5] x [0.5, 7.5]"""
    sc = scenes.amr(levels=1, root=(3, 3, 2), B=4)
    sc = with_field_of_centres(sc, lambda c: c[:, 0] - 6.0)
    sc = with_field_of_centres(sc, lambda c: -(c[:, 1] - 6.0))
    return with_field_of_centres(sc, lambda c: np.zeros(len(c)))


def rk4_growth(h):
    """what one classical RK4 step multiplies the solution of x' = x by"""
    return 1.0 + h + h * h / 2.0 + h ** 3 / 6.0 + h ** 4 / 24.0


def stretch64(end, coords):
    """the stencil, the tensor and numpy's float64 eigenvalues on a flow map end [nz, ny, nx, 3] in float64 (every point valid)"""
    end = np.asarray(end, np.float64)
    cols = []
    for axis in range(3):
        c = np.asarray(coords[axis], np.float64)
        n, ax = len(c), 2 - axis
        if n < 2:
            cols.append(np.zeros_like(end))
            continue
        idx = np.arange(n)
        im, ip = np.maximum(idx - 1, 0), np.minimum(idx + 1, n - 1)
        shape = [1, 1, 1, 1]
        shape[ax] = n
        cols.append((np.take(end, ip, axis=ax) - np.take(end, im, axis=ax)) / (c[ip] - c[im]).reshape(shape))
    Fm = np.stack(cols, axis=-1)                                             # [..., c, a]
    return np.linalg.eigvalsh(np.swapaxes(Fm, -1, -2) @ Fm)[..., -1]


# ---- the inputs the reference tests and the GPU tests share: (name, scene, channels, forms, empty cells, box(dims) -> (lo, hi),
# step); every box but the holes' is wider than the volume on one side at the least, so some seeds fail ----
LATTICES = [(5, 4, 3), (9, 7, 5)]
NUM_STEPS = [1, 12]


def _box(lo, hi):
    return lambda dims: (lo, hi)


def _unit_cells(lo):
    """lattice points at lo + (i + 0.5): the centres of the finest cells, where alone an empty cell leaves no value"""
    return lambda dims: (lo, tuple(float(a + n) for a, n in zip(lo, dims)))


CASES = [
    ("rotation", sr.rotation_scene, (1, 2, 3), (0, 1), False, _box((-3.0, 0.5, 0.75), (12.5, 13.0, 7.5)), 0.125),
    ("amr3", lambda: scenes.amr(levels=3, fields=4), (1, 3, 0), (0, 1), False, _box((-8.0, 1.0, 2.0), (47.0, 50.0, 33.0)), 0.5),
    ("amr3_holes", lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=3), fraction=0.15), (0, 1, 2), (0,), True,
     _unit_cells((8.0, 17.0, 13.0)), 0.5),
    ("zero", sr.zero_fields_scene, (1, 2, 3), (1,), False, _box((-2.0, 3.0, 1.0), (27.0, 30.0, 20.0)), 0.5),
]
# lattices that break a patch map: an axis of one point, fewer points than a patch, one more than a patch
SHAPES = [(1, 1, 1), (2, 1, 1), (1, 2, 1), (1, 1, 2), (67, 1, 1), (3, 2, 1), (4, 4, 4), (5, 5, 5), (65, 3, 2)]

_results = {}


def case_result(idx, form, dims, num_steps, backward):
    """the oracle-fed restatement of CASES[idx] in basis form `form` on the lattice dims, computed once per session"""
    from common import Case
    key = (idx, form, tuple(dims), num_steps, bool(backward))
    if key not in _results:
        name, make, channels, _, empty, box, step = CASES[idx]
        lo, hi = box(dims)
        if ("S", idx, form) not in _results:
            _results[("S", idx, form)] = Case(make(), basis_form=form, allow_empty_cells=empty).oracle_scene()
        _results[key] = flowmap(oracle_feed(_results[("S", idx, form)], channels), lo, hi, dims, step, num_steps, backward)
    return _results[key]
