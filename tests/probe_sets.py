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
