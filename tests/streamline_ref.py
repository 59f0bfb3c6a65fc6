"""The contract of exa_hip_streamlines (include/exa_hip.h) restated in numpy float32, one scalar operation at a time: the region
of a position from the half-open rule over the region domains (as probe_sets.brute_owner), its three values from the CPU
oracle's sample_point in the scene's basis form, and the RK4 step, the end reasons and the packing exactly as the header
words them.  tests/test_streamline_ref.py holds this restatement itself (against the oracle's tracer, against float64 RK4 of
an analytic field, and the coverage of the end reasons); tests/test_gpu_streamlines.py holds the module to it bit for bit."""
import numpy as np

from probe_sets import domains, with_field_of_centres

from owlexabrick_amd import scenes

F = np.float32
END_NONE, END_MAXSTEPS, END_LEFT, END_NOVALUE, END_STAGNANT = range(5)
NAN3 = np.full(3, np.nan, dtype=F)

# The rotation-field check of tests/test_streamline_ref.py: the largest error of the restatement against float64 RK4 of the
# analytic field, in units of 2^-24 * 12 * stepIndex (the largest coordinate times the number of steps taken), over the 16
# seeds of rotation_seeds(), step 0.125, 60 steps.  Measured on the restatement alone, 2026-10-18: 0.4472 in both
# forms.  The test asserts 4 x the measured value rounded up to a power of two (probe_ref64.bound_from): the
# margin covers other seeds.
ROTATION_K_MEASURED = {0: 0.4472, 1: 0.4472}


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, dtype=F).view(np.uint32), np.asarray(b, dtype=F).view(np.uint32))


class StreamRef:
    """S: an oracle scene (oracle.pyoracle.OracleScene) already set to the basis form of the case"""

    def __init__(self, S, channels=(0, 1, 2), normalize=False):
        self.S, self.channels, self.normalize = S, tuple(int(c) for c in channels), bool(normalize)
        dom = domains(S)
        self.lo, self.hi = dom[:, :3], dom[:, 3:]
        self.root_hi = self.hi.max(axis=0)
        self.evaluations = 0
        self.last = -1

    def owner(self, q):
        """lo <= q < hi per axis; q == hi only on the root box's upper faces; -1 for none (NaN: no comparison holds)"""
        r = self.last          # the domains do not overlap: a position the last owner still holds has no other owner
        if r >= 0 and np.all((q >= self.lo[r]) & ((q < self.hi[r]) | ((q == self.hi[r]) & (self.hi[r] == self.root_hi)))):
            return r
        upper = (q < self.hi) | ((q == self.hi) & (self.hi == self.root_hi))
        own = np.nonzero(np.all((q >= self.lo) & upper, axis=1))[0]
        assert len(own) <= 1, "overlapping region domains"
        self.last = int(own[0]) if len(own) else -1
        return self.last

    def evaluate(self, q):
        """E(q): (0, v, d) or (reason, None, None); order lookup, channels, speed"""
        self.evaluations += 1
        region = self.owner(q)
        if region < 0:
            return END_LEFT, None, None
        v = np.zeros(3, dtype=F)
        novalue = False
        for k, c in enumerate(self.channels):
            ok, value, _ = self.S.sample_point(region, q, c, False)
            novalue |= not ok
            v[k] = value
        if novalue:
            return END_NOVALUE, None, None
        if not self.normalize:
            return 0, v, v
        s = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        assert s.dtype == F
        if not (s > 0) or not np.isfinite(s):
            return END_STAGNANT, None, None
        return 0, v, v / s

    def direction(self, p0, hs, max_steps):
        """(vertices [1 + m, 3], velocities [1 + m, 3], reason, seed_ok): the seed is vertex 0"""
        hs = F(hs)
        p = np.asarray(p0, dtype=F).copy()
        with np.errstate(all="ignore"):
            r, v, d = self.evaluate(p)
            if r:
                return p[None].copy(), NAN3[None].copy(), r, False
            verts, vels = [p.copy()], [v.copy()]
            reason = END_MAXSTEPS
            for _ in range(max_steps):
                k1 = hs * d
                r, _, d2 = self.evaluate(p + F(.5) * k1)
                if r:
                    reason = r
                    break
                k2 = hs * d2
                r, _, d3 = self.evaluate(p + F(.5) * k2)
                if r:
                    reason = r
                    break
                k3 = hs * d3
                r, _, d4 = self.evaluate(p + k3)
                if r:
                    reason = r
                    break
                k4 = hs * d4
                pn = p + (F(1) / F(6)) * (((k1 + F(2) * k2) + F(2) * k3) + k4)
                assert pn.dtype == F
                if _bits_equal(pn, p):
                    reason = END_STAGNANT
                    break
                r, v, d = self.evaluate(pn)
                if r:
                    reason = r
                    break
                p = pn
                verts.append(p.copy())
                vels.append(v.copy())
        return np.stack(verts), np.stack(vels), reason, True

    def line(self, seed, step, max_steps, forward=True, backward=False):
        """(vertices, velocities, seed_vertex, [backward reason, forward reason]) of one seed"""
        assert forward or backward
        reasons = [END_NONE, END_NONE]
        parts_v, parts_w = [], []
        seed_vertex = 0
        if backward:
            bv, bw, reasons[0], _ = self.direction(seed, -F(step), max_steps)
            seed_vertex = len(bv) - 1
            parts_v.append(bv[::-1])
            parts_w.append(bw[::-1])
        if forward:
            fv, fw, reasons[1], _ = self.direction(seed, F(step), max_steps)
            parts_v.append(fv[1:] if backward else fv)      # the seed once
            parts_w.append(fw[1:] if backward else fw)
        return np.concatenate(parts_v), np.concatenate(parts_w), seed_vertex, reasons


def streamlines(S, seeds, channels=(0, 1, 2), step=0.5, max_steps=100, forward=True, backward=False, normalize=False):
    """what Renderer.streamlines(..., velocities=True) returns: (vertices [V,3], offsets [n+1], seed_vertex [n], reasons [n,2],
    velocities [V,3])"""
    ref = StreamRef(S, channels, normalize)
    seeds = np.asarray(seeds, dtype=F).reshape(-1, 3)
    V, W, offsets, seed_vertex, reasons = [], [], [0], [], []
    for s in seeds:
        v, w, sv, rs = ref.line(s, step, max_steps, forward, backward)
        V.append(v)
        W.append(w)
        offsets.append(offsets[-1] + len(v))
        seed_vertex.append(sv)
        reasons.append(rs)
    cat = lambda parts: np.concatenate(parts).astype(F) if parts else np.zeros((0, 3), F)   # noqa: E731
    return (cat(V), np.array(offsets, dtype=np.uint64), np.array(seed_vertex, dtype=np.uint32),
            np.array(reasons, dtype=np.int32).reshape(-1, 2), cat(W))


def joined(back, fwd):
    """the {F,B} result that the {B} and the {F} result of the same seeds imply: per line the {B} line (already farthest
    first), then the {F} line without its seed"""
    bv, bo, _, br, bw = back
    fv, fo, _, fr, fw = fwd
    V, W, offsets, seed_vertex = [], [], [0], []
    for i in range(len(bo) - 1):
        b0, b1, f0, f1 = int(bo[i]), int(bo[i + 1]), int(fo[i]), int(fo[i + 1])
        V += [bv[b0:b1], fv[f0 + 1:f1]]
        W += [bw[b0:b1], fw[f0 + 1:f1]]
        seed_vertex.append(b1 - b0 - 1)
        offsets.append(offsets[-1] + (b1 - b0) + (f1 - f0 - 1))
    reasons = np.stack([br[:, 0], fr[:, 1]], axis=1).astype(np.int32) if len(br) else np.zeros((0, 2), np.int32)
    cat = lambda parts: np.concatenate(parts).astype(F) if parts else np.zeros((0, 3), F)   # noqa: E731
    return cat(V), np.array(offsets, dtype=np.uint64), np.array(seed_vertex, dtype=np.uint32), reasons, cat(W)


# ---- the scenes and seeds the reference tests and the GPU tests share ----
def rotation_scene():
    """one level, 12 x 12 x 8 voxels, 75 regions; fields 1..3 = (-(y-6), x-6, 0.25): a rotation about (6, 6) rising in z.  The
    hat reconstruction of a linear field is exact in the interior."""
    sc = scenes.amr(levels=1, root=(3, 3, 2), B=4)
    sc = with_field_of_centres(sc, lambda c: -(c[:, 1] - 6.0))
    sc = with_field_of_centres(sc, lambda c: c[:, 0] - 6.0)
    return with_field_of_centres(sc, lambda c: np.full(len(c), 0.25))


def rotation_seeds(n=16, seed=3):
    rng = np.random.default_rng(seed)
    r = rng.uniform(0.5, 4.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    z = rng.uniform(1.5, 3.0, n)
    return np.stack([6.0 + r * np.cos(phi), 6.0 + r * np.sin(phi), z], axis=1).astype(F)


def rotation_rk4_64(seeds, step, steps):
    """float64 RK4 of the analytic field (-(y-6), x-6, 0.25): [n, steps + 1, 3]"""
    def f(p):
        return np.stack([-(p[:, 1] - 6.0), p[:, 0] - 6.0, np.full(len(p), 0.25)], axis=1)
    p = np.asarray(seeds, dtype=np.float64)
    out = [p]
    for _ in range(steps):
        k1 = step * f(p)
        k2 = step * f(p + 0.5 * k1)
        k3 = step * f(p + 0.5 * k2)
        k4 = step * f(p + k3)
        p = p + (k1 + 2.0 * k2 + 2.0 * k3 + k4) / 6.0
        out.append(p)
    return np.stack(out, axis=1)


def zero_fields_scene():
    """amr(levels=2) with three all-zero extra fields (channels 1..3): every seed inside stagnates at once"""
    sc = scenes.amr(levels=2)
    for _ in range(3):
        sc = with_field_of_centres(sc, lambda c: np.zeros(len(c)))
    return sc


def uniform_seeds(S, n=48, seed=1, grow=0.05):
    """n seeds uniform in the voxel bounds (S: an oracle scene or a binding.Prep) grown by 5 %"""
    lo, hi = (np.asarray(x, dtype=np.float64) for x in S.voxel_bounds())
    ext = hi - lo
    return np.random.default_rng(seed).uniform(lo - grow * ext, hi + grow * ext, (n, 3)).astype(F)


def reason_counts(reasons, slot):
    return {r: int((np.asarray(reasons)[:, slot] == r).sum()) for r in (END_MAXSTEPS, END_LEFT, END_NOVALUE, END_STAGNANT)}
