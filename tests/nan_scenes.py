"""Scenes with NaN cell scalars and the transfer function that makes them visible, shared by tests/test_nan_cells.py (CPU:
the inputs are valid by the oracle alone) and tests/test_gpu_nan_cells.py (the module against the oracle on them).

DESIGN.md 2 ("Input domain"): cell scalars are finite or NaN, and a NaN cell poisons the samples that read it exactly as in
the reference.  A NaN sample takes entry 0 of the transfer function (exabrick.cu:135-150: fminf / fmaxf drop the NaN), which
the default ramp leaves transparent; marker_xf() makes it opaque magenta, so a sample that is NaN on one side only moves its
pixel by a whole colour.

Every function returns a new Scene that shares bricks and cell ids with its argument and owns its fields; nothing changes a
scene it is given.  A Case on these scenes states its TF domain (TF_DOMAIN): the default of tests/common.py, the field's own
minimum and maximum, is NaN here."""
import numpy as np

from owlexabrick_amd import harness, scenes

TF_DOMAIN = (-0.25, 1.0)
NAN = np.float32("nan")


def marker_xf():
    """the default ramp with entry 0 — where NaN samples land — replaced by opaque magenta"""
    xf = harness.default_xf()
    xf[0] = (1.0, 0.0, 1.0, 1.0)
    return xf


def _with_fields(scene, fields, tag):
    return scenes.Scene(scene.bricks7, scene.cellIDs, fields, name=f"{scene.name}_{tag}", value_range=scene.value_range,
                        meta=dict(scene.meta))


def _poisoned(scene, cells, channels, tag):
    """`cells`: boolean per cell in brick order (x fastest within a brick); the fields are indexed through cellIDs"""
    ids = np.asarray(scene.cellIDs)[np.asarray(cells, dtype=bool)]
    assert (ids >= 0).all()
    fields = [np.array(f, dtype=np.float32, copy=True) for f in scene.fields]
    for c in channels:
        fields[c][ids] = NAN
    return _with_fields(scene, fields, tag)


def cell_table(scene):
    """per cell in brick order: its centre in voxel space [n, 3] float64, its brick [n], and whether it lies in the outermost
    cell layer of its brick [n] (bricks7 rows are size.xyz, lower.xyz, level)"""
    ctr, brick, face = [], [], []
    for b, (sx, sy, sz, x, y, z, level) in enumerate(np.asarray(scene.bricks7, dtype=np.int64).reshape(-1, 7)):
        kz, ky, kx = np.meshgrid(np.arange(sz), np.arange(sy), np.arange(sx), indexing="ij")
        idx = np.stack([kx.ravel(), ky.ravel(), kz.ravel()], axis=1)
        ctr.append(np.array([x, y, z], dtype=np.float64) + (idx + 0.5) * float(1 << level))
        brick.append(np.full(len(idx), b, dtype=np.int64))
        face.append(np.any((idx == 0) | (idx == np.array([sx, sy, sz]) - 1), axis=1))
    return np.concatenate(ctr), np.concatenate(brick), np.concatenate(face)


def nan_cells(scene, channel=0):
    """boolean per cell in brick order: the cell's scalar of `channel` is NaN"""
    return np.isnan(np.asarray(scene.fields[channel])[np.asarray(scene.cellIDs)])


def _all_channels(scene):
    return range(len(scene.fields))


def sparse(scene, fraction, seed, channels=None):
    """int(fraction * cells) cells drawn without replacement, by their cell id (the index into the fields)"""
    n = len(scene.fields[0])
    assert n == scene.num_cells
    ids = np.random.default_rng(seed).choice(n, size=int(fraction * n), replace=False)
    fields = [np.array(f, dtype=np.float32, copy=True) for f in scene.fields]
    for c in (_all_channels(scene) if channels is None else channels):
        fields[c][ids] = NAN
    return _with_fields(scene, fields, f"sparse{seed}")


def mid_box(scene, share=0.3):
    """the box mid - share * extent .. mid + share * extent of the scene's bounds"""
    lo, hi = (np.asarray(x, dtype=np.float64) for x in scene.bounds())
    mid, ext = 0.5 * (lo + hi), hi - lo
    return mid - share * ext, mid + share * ext


def _in_box(scene, lo, hi):
    ctr = cell_table(scene)[0]
    return np.all((ctr >= np.asarray(lo)) & (ctr <= np.asarray(hi)), axis=1)


def block(scene, lo, hi):
    """NaN where the cell centre lies in the box [lo, hi], in every channel"""
    return _poisoned(scene, _in_box(scene, lo, hi), _all_channels(scene), "block")


def channel_only(scene, k, lo, hi):
    """the block in channel k of a scene of several fields, the other channels untouched"""
    assert len(scene.fields) > 1
    return _poisoned(scene, _in_box(scene, lo, hi), [k], f"block_ch{k}")


def all_nan(scene):
    return _poisoned(scene, np.ones(scene.num_cells, dtype=bool), _all_channels(scene), "all_nan")


def _some_bricks(scene, every, seed, bricks):
    nb = len(np.asarray(scene.bricks7).reshape(-1, 7))
    pick = np.zeros(nb, dtype=bool)
    pick[np.random.default_rng(seed).permutation(nb)[:max(1, nb // every)] if bricks is None else list(bricks)] = True
    return pick


def brick_border(scene, every=4, seed=0, bricks=None):
    """NaN in exactly the outermost cell layer of some bricks (`bricks`, or every `every`-th, drawn by seed), and nowhere
    else: the cells a sampler that clamps its indices to the brick reaches through the clamp"""
    _, brick, face = cell_table(scene)
    return _poisoned(scene, face & _some_bricks(scene, every, seed, bricks)[brick], _all_channels(scene), "border")


def brick_interior(scene, every=4, seed=0, bricks=None):
    """the twin of brick_border: NaN only in cells of the same bricks that lie on no face of their brick"""
    _, brick, face = cell_table(scene)
    cells = ~face & _some_bricks(scene, every, seed, bricks)[brick]
    assert cells.any(), "no brick of the draw has an interior"
    return _poisoned(scene, cells, _all_channels(scene), "interior")


# ---- the base scenes (nothing larger than amr3) and what the tests make of them ----
def amr3(fields=1):
    """scenes.amr(levels=3): 23 552 cells in 4^3 bricks — a cube scene: the one-channel rope march reads the 16-byte cube
    records — 7 066 regions, bounds 48 x 48 x 32"""
    return scenes.amr(levels=3, fields=fields)


def ex3():
    """200 cells, 21 regions; bricks of 4^3 and 2^3 cells, so no cube scene: the 32-byte march headers.  Bricks 0 and 3 are
    the constant 4^3 bricks beside the ramp of the coarse brick 1, which keeps the iso-surface"""
    return scenes.example("ex3")


BASES = {"amr3": lambda: amr3(), "amr3_2f": lambda: amr3(2), "ex3": ex3}

# name -> (base, make(base scene), multi): the clean twin of a scene is its base
SCENES = {
    "amr3_sparse": ("amr3", lambda s: sparse(s, 0.01, 5), True),
    "amr3_block": ("amr3", lambda s: block(s, *mid_box(s)), True),
    "amr3_all_nan": ("amr3", all_nan, True),
    "amr3_border": ("amr3", brick_border, True),
    "amr3_interior": ("amr3", brick_interior, True),
    "amr3_2f_ch0_multi": ("amr3_2f", lambda s: channel_only(s, 0, *mid_box(s)), True),
    "amr3_2f_ch0_single": ("amr3_2f", lambda s: channel_only(s, 0, *mid_box(s)), False),
    "ex3_sparse": ("ex3", lambda s: sparse(s, 0.05, 5), True),
    "ex3_border": ("ex3", lambda s: brick_border(s, bricks=(0, 3)), True),
    "ex3_interior": ("ex3", lambda s: brick_interior(s, bricks=(0, 3)), True),
}
SPARSE = ["amr3_sparse", "ex3_sparse"]
BLOCK = ["amr3_block", "amr3_2f_ch0_single"]                 # regions all of whose cells are NaN: skipping is not neutral
BORDER = ["amr3_border", "ex3_border"]
INTERIOR = ["amr3_interior", "ex3_interior"]

_made = {}


def base(name):
    if ("base", name) not in _made:
        _made[("base", name)] = BASES[name]()
    return _made[("base", name)]


def scene(name):
    """the scene of SCENES[name], made once (nothing changes it)"""
    if name not in _made:
        _made[name] = SCENES[name][1](base(SCENES[name][0]))
    return _made[name]


def case(sc, multi=True, cls=None, **kw):
    """a tests/common.py Case (or the subclass `cls`) on a NaN scene or its clean twin: the marker TF on every channel and the
    stated TF domain"""
    from common import Case
    nf = len(sc.fields)
    kw.setdefault("xf", marker_xf())
    return (cls or Case)(sc, multi=multi, xf_domains=[TF_DOMAIN] * nf, **kw)


# ---- the frames both test files render: variant -> Case settings ----
ISO = 0.4
VARIANTS = {
    "dvr": dict(W=64, H=64, grad=0),
    "grad": dict(W=64, H=64, grad=1),
    "iso": dict(W=64, H=64, grad=1, iso=[(ISO, 0)]),
    "iso_ao": dict(W=64, H=64, grad=0, iso=[(ISO, 0)], ao=1, ao_length=6.0),
    "faint_skip": dict(W=96, H=96, grad=1, opacity_scale=0.05, space_skipping=1),
    "faint_noskip": dict(W=96, H=96, grad=1, opacity_scale=0.05, space_skipping=0),
}


def variants_of(name):
    """at opacity scale 1 saturated rays hide what lies deep in the volume (the block, the interior of a brick): those scenes
    also render faint; the block scenes faint with and without space skipping"""
    v = ["dvr", "grad", "iso", "iso_ao"]
    if name in BLOCK:
        return v + ["faint_skip", "faint_noskip"]
    return v + ["faint_skip"] if name in BORDER + INTERIOR else v


def named_case(name, variant, clean=False, **kw):
    base_name, _, multi = SCENES[name]
    return case(base(base_name) if clean else scene(name), multi=multi, **dict(VARIANTS[variant], **kw))


def empty_range_regions(regions):
    """boolean per region: its value range is still (+inf, -inf) — every cell that contributes to it is NaN"""
    return np.isposinf(regions["vr_lo"]) & np.isneginf(regions["vr_hi"])


# ---- a flow with NaN velocities, for the integrators (exa_hip_streamlines, exa_hip_lic, exa_hip_flowmap) ----
# include/exa_hip.h special-cases nothing: a NaN velocity is a value (status >= 0).  Without EXA_STREAM_NORMALIZE the stage's
# position p + .5f*k1 (or pn) is then NaN, its lookup gives -1 and the direction ends LEFT, the NaN position not appended; with
# the flag, and in exa_hip_lic, !(s > 0) ends it STAGNANT.
FLOW_CHANNELS = (0, 1, 2)
FLOW_STEP, FLOW_MAX_STEPS, FLOW_SEEDS = 0.5, 40, 48
FLOW_PLANE = ((8, 10, 15.5), (1, 0, 0), (0, 1, 0), (14, 10))           # origin, du, dv, size: lic_ref.plane(*FLOW_PLANE)
FLOW_LIC_STEP, FLOW_LIC_HALF_LENGTH = 0.5, 5
FLOW_BOX, FLOW_DIMS, FLOW_NUM_STEPS = ((-8.0, 1.0, 2.0), (47.0, 50.0, 33.0)), (9, 7, 5), 12


def flow_scene():
    """amr(levels=3, fields=3) with 1 % of the cells NaN in channel 1 only (made once)"""
    if "flow" not in _made:
        _made["flow"] = sparse(scenes.amr(levels=3, fields=3), 0.01, 7, channels=[1])
    return _made["flow"]


class CountingNan:
    """an oracle scene that counts the NaN values its sample_point hands out"""

    def __init__(self, S):
        self.S, self.nan = S, 0

    def __getattr__(self, name):
        return getattr(self.S, name)

    def sample_point(self, *args, **kw):
        out = self.S.sample_point(*args, **kw)
        self.nan += int(np.isnan(out[1]))
        return out


def directions_ended_by_nan(S, points, hs, max_steps, normalize=False, channels=FLOW_CHANNELS):
    """boolean per point, from the restatement alone (streamline_ref.StreamRef on the oracle scene S): the direction from the
    point with the signed step hs met a NaN velocity and ended for it, that is before its steps ran out"""
    import streamline_ref as sr
    C = CountingNan(S)
    ref = sr.StreamRef(C, channels, normalize)
    out = np.zeros(len(points), dtype=bool)
    for i, p in enumerate(points):
        before = C.nan
        reason = ref.direction(p, hs, max_steps)[2]
        out[i] = C.nan > before and reason != sr.END_MAXSTEPS
    return out


def counting_evaluator(evaluate):
    """lic_ref's E(q) with a count of the rows that have a value and a NaN in it: evaluate.nan"""
    def counted(q):
        reason, v = evaluate(q)
        counted.nan += int((np.isnan(v).any(axis=1) & (reason == 0)).sum())
        return reason, v
    counted.nan = 0
    return counted
