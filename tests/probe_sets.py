"""Point sets and scenes shared by the probe tests (tests/test_gpu_sample*.py, tests/test_probe_ref64.py): the mixed bag of
probe_points, the brute-force region owner, points drawn per combination of brick levels, and a scene scaled by a power of
two.  Everything works on a binding.Prep or an oracle scene alike: both expose regions(), bricks() and leaflist()."""
import numpy as np

from owlexabrick_amd import scenes


def domains(prep):
    r = prep.regions()
    return np.concatenate([np.stack(list(r["dom_lo"])), np.stack(list(r["dom_hi"]))], axis=1).astype(np.float32)


def root_box(prep, grow=0.0):
    """the union of the region domains (the root box of the region kd-tree), grown by a share of its extent"""
    dom = domains(prep).astype(np.float64)
    lo, hi = dom[:, :3].min(axis=0), dom[:, 3:].max(axis=0)
    ext = hi - lo
    return (lo - grow * ext).astype(np.float32), (hi + grow * ext).astype(np.float32)


def probe_points(prep, n_uniform=2500, seed=0):
    """uniform in the bounds grown by 10 %, on integer and half-integer planes, on region faces, on brick corners, and a
    few NaN / infinite coordinates"""
    rng = np.random.default_rng(seed)
    dom = domains(prep)
    lo, hi = dom[:, :3].min(axis=0), dom[:, 3:].max(axis=0)     # the root box
    ext = hi - lo
    glo, ghi = lo - 0.1 * ext, hi + 0.1 * ext
    parts = [rng.uniform(glo, ghi, (n_uniform, 3))]
    q = rng.uniform(glo, ghi, (800, 3))
    m = rng.random(q.shape) < 0.6
    q[m] = np.round(q[m] * 2.0) / 2.0                         # cell centres (level 0) and cell faces
    parts.append(q)
    pick = dom[rng.integers(len(dom), size=800)]
    f = rng.uniform(pick[:, :3], pick[:, 3:])
    ax = rng.integers(3, size=800)
    side = rng.integers(2, size=800)
    f[np.arange(800), ax] = pick[np.arange(800), ax + 3 * side]  # on a face of a region: shared, or against a gap
    parts.append(f)
    b = np.asarray(prep.bricks())
    lower = np.stack(list(b["lower"])).astype(np.float32)
    size = np.stack(list(b["size"])).astype(np.float32) * (2.0 ** b["level"].astype(np.float32))[:, None]
    corner = rng.integers(2, size=(len(b), 3))
    parts.append(lower + corner * size)
    parts.append(np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan] * 3], dtype=np.float32))
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


def brute_owner(prep, pts):
    """the region whose domain holds p with the descent's half-open rule (lo <= p < hi; p == hi only on the root box's upper
    faces), -1 for none; asserts there is at most one"""
    dom = domains(prep)
    rlo, rhi = dom[:, :3].min(axis=0), dom[:, 3:].max(axis=0)
    out = np.full(len(pts), -1, dtype=np.int64)
    for s in range(0, len(pts), 512):
        p = pts[s:s + 512, None, :]
        upper = (p < dom[None, :, 3:]) | ((p == dom[None, :, 3:]) & (dom[None, :, 3:] == rhi))
        own = np.all((p >= dom[None, :, :3]) & upper, axis=2)
        cnt = own.sum(axis=1)
        assert cnt.max(initial=0) <= 1, "overlapping region domains"
        out[s:s + 512] = np.where(cnt == 1, own.argmax(axis=1), -1)
    return out


def region_levels(prep):
    """per region, the sorted tuple of the distinct levels of its bricks"""
    r, b, ll = prep.regions(), prep.bricks(), np.asarray(prep.leaflist())
    lev = np.asarray(b["level"])
    return [tuple(sorted(set(int(x) for x in lev[ll[int(s):int(s) + int(n)]])))
            for s, n in zip(r["leafListBegin"], r["leafListSize"])]


def level_class(levels):
    """'single' (all bricks at level 0), 'coarse' (all at one level above 0) or 'mixed' (several levels)"""
    return "mixed" if len(levels) > 1 else ("single" if levels[0] == 0 else "coarse")


def level_points(prep, n=1000, seed=0):
    """n points inside region domains, shared evenly among the combinations of brick levels that occur in the scene (the
    regions of a combination drawn uniformly, the point uniformly in the region's domain)"""
    rng = np.random.default_rng(1000 + seed)
    combos = region_levels(prep)
    kinds = sorted(set(combos))
    dom = domains(prep).astype(np.float64)
    parts = []
    for k, kind in enumerate(kinds):
        ids = np.array([i for i, c in enumerate(combos) if c == kind])
        m = n // len(kinds) + (1 if k < n % len(kinds) else 0)
        pick = dom[ids[rng.integers(len(ids), size=m)]]
        parts.append(rng.uniform(pick[:, :3], pick[:, 3:]))
    return np.ascontiguousarray(np.concatenate(parts).astype(np.float32))


def scaled(scene, k):
    """the same scene with every brick's lower corner multiplied by 2^k and its level raised by k: the same cells, 2^k as wide"""
    b = np.array(scene.bricks7, dtype=np.int32, copy=True).reshape(-1, 7)
    b[:, 3:6] *= 1 << k
    b[:, 6] += k
    return scenes.Scene(b, scene.cellIDs, scene.fields, name=f"{scene.name}_x{1 << k}", value_range=scene.value_range,
                        meta=dict(scene.meta))


def translated(scene, t):
    """the same scene with every brick's lower corner moved by the integer vector t: the same cells somewhere else"""
    t64 = np.asarray(t, dtype=np.int64)
    assert t64.shape == (3,) and np.array_equal(t64, np.asarray(t))
    b = np.array(scene.bricks7, dtype=np.int64, copy=True).reshape(-1, 7)
    b[:, 3:6] += t64
    assert np.abs(b[:, 3:6]).max() < 2 ** 31
    return scenes.Scene(b.astype(np.int32), scene.cellIDs, scene.fields, name=f"{scene.name}_t{'_'.join(str(int(x)) for x in t64)}",
                        value_range=scene.value_range, meta=dict(scene.meta))


# named translations of the amr3 scene (scenes.amr(levels=3): extent 48 x 48 x 32 from the origin)
TRANSLATIONS = [
    ("straddle", (-24, -20, -12)),                 # the origin inside the scene, on cell-centre planes of the coarse level
    ("odd", (-23, -19, -13)),                      # the origin inside, off the coarse planes
    ("negative", (-48, -48, -32)),                 # the upper corner at 0: the root box's closed upper faces at 0
    ("moderate", (-1000, 2000, -52)),
    ("far", (2 ** 20, -2 ** 20, 2 ** 16)),         # float32 positions have an ulp of 0.125 there
]
TRANSLATION = dict(TRANSLATIONS)


def moved(pts, t):
    """pts + t as float32, after asserting that the sum of every finite row is a float32: the same points in the other frame"""
    p64 = np.asarray(pts, dtype=np.float32).astype(np.float64) + np.asarray(t, dtype=np.float64)
    q = p64.astype(np.float32)
    fin = np.isfinite(p64)
    assert np.array_equal(q.astype(np.float64)[fin], p64[fin]), "p + t is not a float32"
    return np.ascontiguousarray(q)


def dyadic_bits(t):
    """g such that a multiple of 2^-g in the (slightly grown) amr3 root box is a float32 before and after adding t"""
    return min(12, 23 - int(np.ceil(np.log2(np.abs(np.asarray(t, dtype=np.float64)).max() + 64))))


def dyadic_points(prep, t, n=1500, seed=0):
    """Points of the untranslated frame (prep is the untranslated scene's) that are float32 in both frames of reference, p
    and p + t: n uniform in the root box grown by 2 %, rounded to multiples of 2^-g (dyadic_bits); points on region faces;
    brick corners; points on the planes that become coordinate 0 after the translation (through the scene or not), among
    them the point that becomes the origin; and the NaN / infinite rows of probe_points.  moved(points, t) is exact."""
    rng = np.random.default_rng(7000 + seed)
    t64 = np.asarray(t, dtype=np.float64)
    g = dyadic_bits(t)
    assert g >= 1                                                  # half-integer planes (region faces) are on the grid
    q = 2.0 ** g
    rnd = lambda a: np.round(np.asarray(a, dtype=np.float64) * q) / q      # noqa: E731
    lo, hi = (x.astype(np.float64) for x in root_box(prep, grow=0.02))
    dom = domains(prep).astype(np.float64)
    parts = [rnd(rng.uniform(lo, hi, (n, 3)))]
    k = 300
    pick = dom[rng.integers(len(dom), size=k)]
    f = rnd(rng.uniform(pick[:, :3], pick[:, 3:]))
    ax, side = rng.integers(3, size=k), rng.integers(2, size=k)
    f[np.arange(k), ax] = pick[np.arange(k), ax + 3 * side]          # on a face of a region
    parts.append(f)
    b = np.asarray(prep.bricks())
    lower = np.stack(list(b["lower"])).astype(np.float64)
    size = np.stack(list(b["size"])).astype(np.float64) * (2.0 ** b["level"].astype(np.float64))[:, None]
    parts.append(lower + rng.integers(2, size=(len(b), 3)) * size)  # brick corners
    zero = rnd(rng.uniform(lo, hi, (240, 3)))
    zero[np.arange(240), np.arange(240) % 3] = -t64[np.arange(240) % 3]    # p + t has a zero component
    zero[:8] = np.where(rng.integers(2, size=(8, 3)) == 1, -t64, zero[:8])  # ... two or three of them
    zero[0] = -t64                                                  # the origin itself
    parts.append(zero)
    pts = np.concatenate(parts)
    assert np.array_equal(pts.astype(np.float32).astype(np.float64), pts)
    assert np.array_equal((pts + t64).astype(np.float32).astype(np.float64), pts + t64)
    pts = np.concatenate([pts.astype(np.float32), np.array([[np.nan, 1, 1], [1, np.inf, 1], [1, 1, -np.inf], [np.nan] * 3], dtype=np.float32)])
    return np.ascontiguousarray(pts)


def translated_boxes(t):
    """histogram boxes in the frame of amr3 translated by t, where the coordinate 0 means something: none; box_lo < 0 < box_hi
    on every axis; upper face exactly 0; degenerate at 0; entirely negative; and one that cuts the scene wherever it lies
    (odd corners, inside the scene's 48 x 48 x 32).  The same box in the untranslated frame is the box minus t."""
    t = [int(x) for x in t]
    return [None, [-7, -5, -3, 9, 11, 5], [-16, -12, -8, 0, 0, 0], [0] * 6, [-15, -13, -9, -1, -3, -2],
            [5 + t[0], 7 + t[1], 3 + t[2], 41 + t[0], 37 + t[1], 27 + t[2]]]


def axis_rays(prep, t, axis, size=(24, 16), n=128):
    """Orthographic rays along +axis through the amr3 scene of the untranslated `prep`, and the same rays in the frame
    translated by t: (rays, rays moved by t), dicts of project_ref.rays.  Origins are dyadic, tmin and dt powers of two:
    every position p_i of exa_hip_project's contract is exact in both frames, which is asserted here in float64."""
    import project_ref as pr
    lo, hi = (x.astype(np.float64) for x in prep.voxel_bounds())
    u, v = [k for k in range(3) if k != axis]
    org = lo + np.array([0.125, 0.375, 0.625])
    org[axis] = lo[axis] - 4.0
    d, du, dv = np.zeros(3), np.zeros(3), np.zeros(3)
    d[axis] = 1.0
    du[u], dv[v] = (hi[u] - lo[u]) / size[0], (hi[v] - lo[v]) / size[1]
    out = []
    for shift in (np.zeros(3), np.asarray(t, dtype=np.float64)):
        r = pr.rays(org + shift, d, size, 0.5, 0.5, n, orgDu=du, orgDv=dv)
        p, has = pr.positions(r)
        o64 = (org + shift)[None, None, :] + (np.arange(size[0]) + 0.5)[None, :, None] * du + (np.arange(size[1]) + 0.5)[:, None, None] * dv
        p64 = o64[:, :, None, :] + (0.5 + (np.arange(n) + 0.5) * 0.5)[None, None, :, None] * d
        assert has.all() and np.array_equal(p.astype(np.float64), p64), "a position rounds"
        out.append(r)
    assert (0.5 + (n - 0.5) * 0.5) - 4.0 > (hi - lo).max()          # the last sample lies behind the scene
    return out


def _amr3_offset():
    sc = scenes.amr(levels=3, fields=3)
    sc.fields[1] = (sc.fields[1].astype(np.float64) + 1000.0).astype(np.float32)   # the sums of the gradient cancel
    return sc


# the scenes held against the float64 reference (tests/probe_ref64.py): (name, make, basis forms, allow_empty_cells)
REF_CASES = [
    ("ex3", lambda: scenes.example("ex3"), (0, 1), False),                  # two levels side by side
    ("ex4", lambda: scenes.example("ex4"), (0, 1), False),
    ("amr3", lambda: scenes.amr(levels=3, fields=3), (0, 1), False),
    ("amr3_offset", _amr3_offset, (0, 1), False),
    ("gen", lambda: scenes.generated(root=(2, 2, 2), B=4, levels=2), (0, 1), False),
    ("amr3_holes", lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=2), fraction=0.15), (0,), True),
]


def ref_points(prep, idx):
    """the points of REF_CASES[idx]: probe_points and 1 000 level_points"""
    return np.ascontiguousarray(np.concatenate([probe_points(prep, n_uniform=1800, seed=100 + idx), level_points(prep, 1000, seed=idx)]))


def grid_positions(lo, hi, dims):
    """the positions of exa_hip_resample's lattice, x fastest, in the float32 operations of the kernel"""
    f = np.float32
    lo, hi = np.asarray(lo, f), np.asarray(hi, f)
    axes = [lo[k] + (np.arange(dims[k], dtype=f) + f(0.5)) * ((hi[k] - lo[k]) / f(dims[k])) for k in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(f)


def cell_centres(scene):
    """the centre of every cell in voxel space, in brick order (x fastest within a brick): [num_cells, 3] float64"""
    out = []
    for sx, sy, sz, x, y, z, level in np.asarray(scene.bricks7, dtype=np.int64).reshape(-1, 7):
        kz, ky, kx = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
        idx = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1).astype(np.float64)
        out.append(np.array([x, y, z], dtype=np.float64) + (idx + 0.5) * float(1 << level))
    return np.concatenate(out)


def with_field_of_centres(scene, fn):
    """the scene with one more field, fn(cell centres) per cell (any scene: the cells are found through bricks7 and cellIDs)"""
    ids = np.asarray(scene.cellIDs)
    field = np.zeros(len(scene.fields[0]), dtype=np.float32)
    field[ids[ids >= 0]] = fn(cell_centres(scene))[ids >= 0].astype(np.float32)
    return scenes.Scene(scene.bricks7, scene.cellIDs, list(scene.fields) + [field], name=scene.name + "_fn",
                        value_range=scene.value_range, meta=dict(scene.meta))
