"""Translation of a scene by an integer vector, on the CPU: the ground the GPU tests of tests/test_gpu_translation.py stand
on.  The host preparation's tables of a translated scene are the tables of the scene, translated; the float32 oracle's
point sample keeps every bit on points that are float32 in both frames of reference (probe_sets.dyadic_points) and stays
within the existing bounds against the float64 reference at general points of the translated frame; the bit-exact
restatements of the histogram and of the projection agree with themselves across frames; and coordinates the float32 tables
cannot hold are refused where a scene enters the module, instead of being partitioned differently without a word."""
import re

import numpy as np
import pytest

import probe_ref64 as r64
import probe_sets as ps
import project_ref as pr
import streamline_ref as sr
import test_probe_ref64 as tp
from common import Case
from histogram_ref import Slots, same_stats
from owlexabrick_amd import binding, scenes

NAMES = [n for n, _ in ps.TRANSLATIONS]
_bits = tp._bits


def amr3():
    return scenes.amr(levels=3, fields=2)


def holes():
    return scenes.with_empty_cells(amr3(), fraction=0.15)


def assert_tables_translate(pa, pb, t):
    """the table equalities of the scaling test with + t in place of * s, and the kd-tree: the same shape, its planes moved"""
    tf = np.asarray(t, dtype=np.float32)
    ra, rb = pa.regions(), pb.regions()
    assert len(ra) == len(rb)
    assert np.array_equal(np.stack(list(ra["dom_lo"])) + tf, np.stack(list(rb["dom_lo"])))
    assert np.array_equal(np.stack(list(ra["dom_hi"])) + tf, np.stack(list(rb["dom_hi"])))
    assert np.array_equal(ra["leafListBegin"], rb["leafListBegin"]) and np.array_equal(ra["leafListSize"], rb["leafListSize"])
    assert np.array_equal(ra["finestLevelCellWidth"], rb["finestLevelCellWidth"])
    assert np.array_equal(pa.leaflist(), pb.leaflist())
    ka, kb = pa.kd_nodes(), pb.kd_nodes()
    assert len(ka) == len(kb) and pa.scene.kdRoot == pb.scene.kdRoot
    for k in ("axis", "left", "right"):
        assert np.array_equal(ka[k], kb[k]), k
    assert np.array_equal(ka["split"] + tf[ka["axis"]], kb["split"])
    for a, b in zip(pa.voxel_bounds(), pb.voxel_bounds()):
        assert np.array_equal(a + tf, b)


def test_the_translations_are_what_their_names_say():
    lo, hi = (x.astype(np.int64) for x in amr3().bounds())
    assert np.array_equal(lo, [0, 0, 0]) and np.array_equal(hi, [48, 48, 32])
    t = {n: np.array(v) for n, v in ps.TRANSLATIONS}
    for n in ("straddle", "odd"):
        assert np.all(lo + t[n] < 0) and np.all(hi + t[n] > 0)
    assert np.all(t["straddle"] % 4 == 0) and np.all(t["odd"] % 2 == 1)          # level 2: centre planes at multiples of 4, + 2
    assert np.array_equal(hi + t["negative"], [0, 0, 0])
    assert np.abs(t["far"]).max() == 2 ** 20


@pytest.mark.parametrize("name", NAMES)
def test_prep_tables_translate_exactly(name):
    t = ps.TRANSLATION[name]
    A = amr3()
    pa, pb = binding.Prep(A), binding.Prep(ps.translated(A, t))
    assert len(pa.regions()) == 7066 and len(pa.kd_nodes()) == 7386
    assert_tables_translate(pa, pb, t)
    pts = ps.dyadic_points(pa, t)
    owner = ps.brute_owner(pa, pts)
    assert np.array_equal(owner, ps.brute_owner(pb, ps.moved(pts, t)))
    assert (owner >= 0).sum() > 1000 and (owner < 0).sum() > 4


def test_dyadic_points_hold_what_they_promise():
    pa = binding.Prep(amr3())
    for name, t in ps.TRANSLATIONS:
        pts = ps.dyadic_points(pa, t)
        q = ps.moved(pts, t)
        assert len(pts) <= 5000 and np.isnan(pts).any() and np.isinf(pts).any()
        fin = np.isfinite(pts).all(axis=1)
        assert np.array_equal(q[fin].astype(np.float64), pts[fin].astype(np.float64) + np.asarray(t, np.float64))
        assert ((q == 0).sum(axis=1) >= 1).sum() >= 200 and (q == 0).all(axis=1).any()     # on the zero planes, and the origin
        dom = ps.domains(pa)
        on_face = (pts[fin][:, None, :] == dom[None, :64, :3]).any(axis=(1, 2))
        assert on_face.sum() >= 10


_frames = {}


def _frame(kind, form):
    """(scene, prep, oracle scene) of the untranslated frame, shared and never changed"""
    if (kind, form) not in _frames:
        scene = holes() if kind == "holes" else amr3()
        empty = kind == "holes"
        _frames[(kind, form)] = (scene, binding.Prep(scene, allow_empty_cells=empty),
                                 Case(scene, basis_form=form, allow_empty_cells=empty).oracle_scene())
    return _frames[(kind, form)]


_untranslated = {}


def _samples_a(kind, form, name):
    key = (kind, form, name)
    if key not in _untranslated:
        scene, pa, S = _frame(kind, form)
        pts = ps.dyadic_points(pa, ps.TRANSLATION[name])
        owner = ps.brute_owner(pa, pts)
        _untranslated[key] = (pts, owner, tp.oracle_samples(S, pts, owner, (0, 1)))
    return _untranslated[key]


@pytest.mark.parametrize("kind,form", [("amr3", 0), ("amr3", 1), ("holes", 0)], ids=["amr3-f0", "amr3-f1", "holes-f0"])
@pytest.mark.parametrize("name", NAMES)
def test_translation_changes_no_bit_of_the_oracle(name, kind, form):
    t = ps.TRANSLATION[name]
    scene, pa, S = _frame(kind, form)
    pts, owner, a = _samples_a(kind, form, name)
    B = ps.translated(scene, t)
    b = tp.oracle_samples(Case(B, basis_form=form, allow_empty_cells=kind == "holes").oracle_scene(), ps.moved(pts, t), owner, (0, 1))
    assert np.array_equal(a[0], b[0])
    assert a[0].sum() > 1000 and (~a[0].all(axis=1)).sum() >= 1                 # samples with a value, points without
    assert np.array_equal(_bits(a[1]), _bits(b[1]))
    assert np.array_equal(_bits(a[2]), _bits(b[2]))
    assert np.abs(a[2][a[0]]).max() > 1e-3
    if kind == "holes":                                                           # owned points whose weights all vanish
        assert (~a[0][owner >= 0]).sum() > (~_samples_a("amr3", 0, name)[2][0][owner >= 0]).sum()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("name", NAMES)
def test_oracle_against_the_reference_in_the_translated_frame(name, form):
    """general float32 points of the translated frame: p - float(lower) is exact for a float32 p, so K_VALUE and K_NUM hold
    as they are"""
    t = ps.TRANSLATION[name]
    scene = ps.translated(amr3(), t)
    prep = binding.Prep(scene)
    lo, hi = ps.root_box(prep, grow=0.02)
    rng = np.random.default_rng(900 + NAMES.index(name))
    pts = np.ascontiguousarray(np.concatenate([rng.uniform(lo, hi, (1500, 3)).astype(np.float32), ps.level_points(prep, 600, seed=3)]))
    owner = ps.brute_owner(prep, pts)
    ref = tp._reference(scene, prep).evaluate(pts, owner, (0, 1))
    ok, v, g = tp.oracle_samples(Case(scene, basis_form=form).oracle_scene(), pts, owner, (0, 1))
    sw = ref["sumW"]
    assert ((sw > 0) & (sw < r64.STATUS_BAND)).sum() == 0, "pick another seed: float32 may round such a sum to either side"
    assert np.array_equal(ok[owner >= 0], sw[owner >= 0] > r64.STATUS_SUMW)
    combos = ps.region_levels(prep)
    cls = np.array([ps.level_class(combos[o]) if o >= 0 else "none" for o in owner])
    kv, kg = r64.scaled_errors(ref, v, g)
    assert ok.all(axis=1).sum() > 1000
    for stratum in ("covered", "all"):
        s = ok & r64.stratum(ref, stratum)
        line = f"K amr3 {name} form {form} {stratum}: n {int(s.sum())} K_value {kv[s].max():.4g} K_num {kg[s].max():.4g} "
        for what in ("coarse", "mixed", "single"):
            m = s & (cls == what)[:, None]
            assert m.sum() >= 100, (stratum, what)
            line += f" [{what} n {int(m.sum())} K_value {kv[m].max():.3g} K_num {kg[m].max():.3g}]"
        print(line)
        assert kv[s].max() <= r64.K_VALUE[stratum][form], (stratum, float(kv[s].max()))
        assert kg[s].max() <= r64.K_NUM[stratum][form], (stratum, float(kg[s].max()))


def test_histogram_restatement_across_frames():
    t = np.array(ps.TRANSLATION["straddle"])
    for scene, allow in ((amr3(), False), (holes(), True)):
        SA, SB = Slots(scene, allow), Slots(ps.translated(scene, t), allow)
        for ch in (0, 1):
            r = SA.histogram(ch, 0, 0, 0)[2]
            assert same_stats(r, SB.histogram(ch, 0, 0, 0)[2])
            for box_b in ps.translated_boxes(t):
                box_a = None if box_b is None else [int(x) for x in np.asarray(box_b) - np.concatenate([t, t])]
                a = SA.histogram(ch, r["min"], r["max"], 128, box=box_a)
                b = SB.histogram(ch, r["min"], r["max"], 128, box=box_b)
                assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and same_stats(a[2], b[2]), box_b
    # the boxes are what they are meant to be: one holds the origin inside, one is empty at 0
    boxes = ps.translated_boxes(t)
    assert all(boxes[1][k] < 0 < boxes[1][k + 3] for k in range(3)) and boxes[3] == [0] * 6
    counts = [SB.histogram(0, 0, 0, 0, box=b)[2]["slots"] for b in boxes]
    assert counts[0] == 23552 and 0 < counts[1] < counts[0] and 0 < counts[2] < counts[0] and counts[3] == 0 and 0 < counts[4] < counts[0]


def test_projection_restatement_across_frames():
    name = "straddle"
    t = ps.TRANSLATION[name]
    scene, pa, SA = _frame("amr3", 1)
    pb = binding.Prep(ps.translated(scene, t))
    SB = Case(ps.translated(scene, t), basis_form=1).oracle_scene()

    def sampler(S, prep):
        def sample(points):
            owner = ps.brute_owner(prep, points)
            ok, v, _ = tp.oracle_samples(S, points, owner, (0,))
            return v[:, 0], np.where(ok[:, 0], owner, np.where(owner >= 0, -2, -1))
        return sample

    valid = 0
    for axis in range(3):
        ra, rb = ps.axis_rays(pa, t, axis, size=(3, 4))
        a, _, sa = pr.project(sampler(SA, pa), ra)
        b, _, sb = pr.project(sampler(SB, pb), rb)
        assert np.array_equal(sa, sb)
        for k in a:
            assert pr.same_bits(a[k], b[k]), (axis, k)
        valid += int((sa >= 0).sum())
        assert (a["count"] > 0).all()
    assert valid >= 3 * 12 * 48                                     # every ray crosses the scene: over 48 samples each


def test_streamline_restatement_reaches_every_end_in_the_translated_frames():
    """what the GPU test of the streamlines asserts about its reference is reached by the restatement alone"""
    for name in ("straddle", "negative"):
        scene = ps.translated(scenes.amr(levels=3, fields=3), ps.TRANSLATION[name])
        S = Case(scene, basis_form=1).oracle_scene()
        seeds = sr.uniform_seeds(S, 48)
        for nm in (False, True):
            for slot, (fw, bw) in ((1, (True, False)), (0, (False, True))):
                n = sr.reason_counts(sr.streamlines(S, seeds, (0, 1, 2), 0.5, 40, fw, bw, nm)[3], slot)
                print(f"{name} normalize {nm} forward {fw}: {n}")
                assert n[sr.END_LEFT] >= 10 and n[sr.END_MAXSTEPS] >= 10, (name, nm, fw, n)


# ---- coordinates the float32 tables cannot hold ----
def _t3(m, sign):
    return (sign * m, -sign * m, sign * m)


@pytest.mark.parametrize("sign", [1, -1])
def test_coordinates_up_to_2_21_are_accepted_and_translate_exactly(sign):
    A = amr3()
    t = _t3(2 ** 21, sign)
    assert_tables_translate(binding.Prep(A), binding.Prep(ps.translated(A, t)), t)


@pytest.mark.parametrize("sign", [1, -1])
@pytest.mark.parametrize("log2", [22, 23])
def test_coordinates_the_float32_tables_cannot_hold_are_refused(log2, sign):
    scene = ps.translated(amr3(), _t3(2 ** log2, sign))
    with pytest.raises(RuntimeError, match=r"exa_prep_create: .*coordinates too large for the cell width") as e:
        binding.Prep(scene)
    msg = str(e.value)
    # it names a brick, an axis and a coordinate of this scene
    assert re.search(r"brick \d+", msg) and re.search(r"\b[xyz]\b", msg) and "float32" in msg, msg
    magnitude = 2 ** log2
    assert any(magnitude - 1 <= abs(float(w)) <= magnitude + 49 for w in re.findall(r"-?\d+(?:\.\d+)?", msg)), msg


def test_a_plane_that_is_no_float32_names_its_brick():
    # one level-0 brick at 2^24 + 1: an odd integer there is no float32
    scene = scenes.Scene(np.array([[2, 2, 2, 0, 0, 0, 0], [2, 2, 2, 0, 2 ** 24 + 1, 0, 0]], np.int32), np.arange(16, dtype=np.int32),
                         [np.linspace(0, 1, 16).astype(np.float32)])
    with pytest.raises(RuntimeError, match=r"exa_prep_create: brick 1 \(lower 0 16777217 0, size 2 2 2, level 0\): its plane y = 16777217 is not a float32"):
        binding.Prep(scene)


def test_scenes_inside_the_representable_range_are_never_refused():
    # coarse bricks far out whose planes are float32 (the scenes of the histogram's 64-bit volume test), every fixture, and a
    # scene moved to the edge of the range along each axis alone
    grids = ("0 0 0 9 10 11 0  0.0 1.0 0.25 0.75 0.5 0.1 0.9 0.3\n16 0 0 3 5 7 2  0.2 0.4 0.6 0.8 1.0 0.0 0.3 0.7\n"
             "0 16 0 1 1 1 3  0.45\n0 12 0 67 1 1 0  0.0 1.0 0.0 1.0 0.0 1.0 0.0 1.0\n")
    for extra in ("0 16777216 0 1 1 1 21  0.35", "0 16777216 0 2 2 2 21  0.35", "0 16777216 0 1 1 1 22  0.35"):
        assert len(binding.Prep(scenes.artificial(scenes.parse_grids(grids + extra), name="odd_coarse")).regions()) == 20
    for name in ("ex0", "ex1", "ex2", "ex3", "ex4"):
        binding.Prep(scenes.example(name))
    A = scenes.amr(levels=2)
    pa = binding.Prep(A)
    for axis in range(3):
        for m in (2 ** 21, -2 ** 21, -2 ** 22):
            t = [0, 0, 0]
            t[axis] = m
            assert_tables_translate(pa, binding.Prep(ps.translated(A, t)), t)
