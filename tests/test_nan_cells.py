"""The inputs of tests/test_gpu_nan_cells.py are valid by the oracle alone (no GPU): every scene of tests/nan_scenes.py
exercises what it is there for, so a scene that stops doing so fails here first.  The floors are conditions on the inputs —
about half of what the oracle gives on these scenes — not tolerances.

Also here: the host preparation against the oracle's regions on the NaN scenes, byte for byte; the NaN entries of the
float64 reconstruction (tests/probe_ref64.py) against the oracle's samplePoint; and one analytic known answer."""
import numpy as np
import pytest

import nan_scenes as ns
import probe_ref64 as r64
import probe_sets as ps
from common import po
from owlexabrick_amd import binding, harness, scenes
from test_probe_ref64 import oracle_samples

FORMS = [0, 1]
_frames = {}


def frame(name, variant, form=1, clean=False):
    key = (name, variant, form, clean)
    if key not in _frames:
        _frames[key] = ns.named_case(name, variant, clean=clean, basis_form=form).run_oracle()
    return _frames[key]


def differing(a, b, tol=1e-3):
    """pixels of which some component of the accumulation buffer differs by more than tol"""
    return int((np.abs(a[1].astype(np.float64) - b[1].astype(np.float64)).max(axis=-1) > tol).sum())


def regions_of(name):
    sc, multi = ns.scene(name), ns.SCENES[name][2]
    S = po.OracleScene(sc.bricks7, sc.cellIDs, sc.fields, num_region_fields=len(sc.fields) if multi else 1)
    return S, S.regions()


def test_the_scene_builders_do_what_they_say():
    b = ns.base("amr3")
    assert b.num_cells == 23552 and np.array_equal(b.bounds()[1], [48, 48, 32])
    for name in ns.SCENES:
        sc, clean = ns.scene(name), ns.base(ns.SCENES[name][0])
        assert sc.fields[0] is not clean.fields[0] and not any(np.isnan(f).any() for f in clean.fields)
        for f, g in zip(sc.fields, clean.fields):                   # NaN or the clean twin's value, nothing else
            assert np.array_equal(f[~np.isnan(f)], g[~np.isnan(f)])
    ctr, brick, face = ns.cell_table(b)
    assert np.array_equal(ctr, ps.cell_centres(b))
    for border, interior in zip(ns.BORDER, ns.INTERIOR):
        nb, ni = ns.nan_cells(ns.scene(border)), ns.nan_cells(ns.scene(interior))
        _, brick, face = ns.cell_table(ns.scene(border))
        assert nb.any() and face[nb].all() and ni.any() and not face[ni].any()
        hit = np.unique(brick[nb])
        assert np.array_equal(hit, np.unique(brick[ni]))              # the same bricks
        assert np.array_equal(nb, face & np.isin(brick, hit))         # exactly the outermost layer of those bricks
    lo, hi = ns.mid_box(b)
    nan = ns.nan_cells(ns.scene("amr3_block"))
    assert nan.sum() == 11388 and np.array_equal(nan, np.all((ctr >= lo) & (ctr <= hi), axis=1))
    two = ns.scene("amr3_2f_ch0_multi")
    assert np.isnan(two.fields[0]).sum() == 11388 and not np.isnan(two.fields[1]).any()
    assert np.isnan(ns.scene("amr3_sparse").fields[0]).sum() == 235 and np.isnan(ns.scene("amr3_all_nan").fields[0]).all()
    xf = ns.marker_xf()
    assert tuple(xf[0]) == (1, 0, 1, 1) and np.array_equal(xf[1:], harness.default_xf()[1:])


def test_the_record_variants_are_covered():
    """amr3 is a cube scene (edge 4: the 16-byte cube records on the one-channel rope march), ex3 with its 4^3 and 2^3 bricks
    is none (the 32-byte march headers); pack_records 0 is an option of the GPU tests"""
    for name, k in (("amr3_border", 2), ("amr3_sparse", 2), ("ex3_border", 0), ("ex3_sparse", 0)):
        P = binding.Prep(ns.scene(name))
        assert binding.cube_records(P.bricks(), P.leaflist())[0] == k, name
        P.close()


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", sorted(ns.SCENES))
def test_no_oracle_frame_has_a_nan_pixel_and_every_scene_shows(name, form):
    shows = 0
    for variant in ns.variants_of(name):
        o = frame(name, variant, form)
        assert not np.isnan(o[1]).any(), variant
        assert o[2]["samples"] > 0 or name == "amr3_all_nan"
        if "iso" in variant and name != "amr3_all_nan":
            assert o[2]["iso_evals"] > 0, "the iso value lies in the field's range"
        shows = max(shows, differing(o, frame(name, variant, form, clean=True)))
    if name in ns.BLOCK:
        shows = max(shows, differing(frame(name, "faint_skip", form), frame(name, "faint_noskip", form)))
    print(f"{name} form {form}: {shows} pixels show the NaN cells in the variant that shows most")
    if name == "amr3_2f_ch0_multi":       # two primary channels: channel 1 is clean and its range keeps every region active
        return
    assert shows >= 300, shows


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ns.SPARSE)
def test_sparse_scenes_differ_from_their_clean_twin(name, form):
    n = differing(frame(name, "grad", form), frame(name, "grad", form, clean=True))
    print(f"{name} form {form}: {n} of 4096 pixels differ from the clean twin by more than 1e-3")       # amr3: 680
    assert n >= 400


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ns.BLOCK)
def test_skipping_is_not_neutral_on_block_scenes(name, form):
    n = differing(frame(name, "faint_skip", form), frame(name, "faint_noskip", form))
    print(f"{name} form {form}: skipping on and off differ in {n} of 9216 pixels")                        # 1 633
    assert n >= 800
    # the marker makes them visible: magenta-dominated pixels with skipping off
    acc = frame(name, "faint_noskip", form)[1]
    assert ((acc[..., 0] > 2 * acc[..., 1]) & (acc[..., 2] > 2 * acc[..., 1])).sum() >= 400


def test_regions_of_empty_range():
    count = {}
    for name in ns.SCENES:
        S, reg = regions_of(name)
        count[name] = int(ns.empty_range_regions(reg).sum())
        assert not np.isnan(reg["vr_lo"]).any() and not np.isnan(reg["vr_hi"]).any()      # s < lo / s > hi skip a NaN
        S.close()
    print(count)
    for name in ns.BLOCK:
        assert count[name] >= 1000, name                                                  # 2 731
    assert count["amr3_sparse"] >= 1                                                      # 4
    assert count["amr3_2f_ch0_multi"] == 0                                                # the range spans both fields
    assert count["amr3_all_nan"] == 7066


def _opaque_xf():
    xf = harness.default_xf()
    xf[:, 3] = 1.0
    return xf


@pytest.mark.parametrize("name", ["amr3_sparse", "amr3_block", "amr3_border", "amr3_2f_ch0_single", "amr3_all_nan", "ex3_border"])
def test_empty_range_regions_are_inactive_under_any_tf(name):
    """+inf > the TF domain's upper end (exabrick.cu:250-281) and no iso value lies in (+inf, -inf) (:373-402)"""
    for xf in (ns.marker_xf(), harness.default_xf(), _opaque_xf()):
        for variant in ("iso", "faint_skip", "faint_noskip"):
            case = ns.named_case(name, variant, xf=xf, iso=[(ns.ISO, 0), (0.7, 0)])
            S = case.oracle_scene()
            fs, P = case.oracle_state(S)
            empty = ns.empty_range_regions(S.regions())
            vol, iso = S.volume_active(fs, P), S.iso_active(fs)
            assert not iso[empty].any()
            if case.space_skipping:
                assert not vol[empty].any()
                if xf[0, 3] == 1.0:       # opaque at entry 0 and everywhere above: what tests/test_gpu_nan_cells.py relies on
                    assert np.array_equal(vol == 0, empty)
            else:
                assert vol.all()
            S.close()


@pytest.mark.parametrize("name", sorted(ns.SCENES))
def test_prep_equals_oracle_bit_for_bit_on_nan_scenes(name):
    """tests/test_host_prep.py on the NaN scenes: valueRangeOf (exa_prep.cpp) skips a NaN as compute_value_range does"""
    sc, multi = ns.scene(name), ns.SCENES[name][2]
    nrf = len(sc.fields) if multi else 1
    S = po.OracleScene(sc.bricks7, sc.cellIDs, sc.fields, num_region_fields=nrf)
    for nt in (1, 5):
        P = binding.Prep(sc, num_threads=nt, num_region_fields=nrf)
        assert P.bricks().tobytes() == S.bricks().tobytes()
        assert P.scalars().tobytes() == S.scalars().tobytes()
        assert P.leaflist().tobytes() == S.leaflist().tobytes()
        pr, sr = P.regions(), S.regions()
        assert pr.tobytes() == sr.tobytes()
        for k in ("vr_lo", "vr_hi"):                                  # the ranges as bits
            assert np.array_equal(pr[k].view(np.uint32), sr[k].view(np.uint32))
        for k in ("dom_lo", "dom_hi"):
            assert np.array_equal(np.stack(list(pr[k])).view(np.uint32), np.stack(list(sr[k])).view(np.uint32))
        P.close()
    S.close()


def _off_the_planes(recon, pts, owner, dist):
    """per point: on every axis either exactly on, or farther than `dist` (voxel units) from, every cell-centre plane of
    every brick of its region — the planes where the low cell index of the reconstruction changes"""
    pts = np.asarray(pts, dtype=np.float64)
    pid, bid = recon.pairs(np.asarray(owner, dtype=np.int64))
    cw = 2.0 ** recon.level[bid].astype(np.float64)
    lp = (pts[pid] - recon.lower[bid]) / cw[:, None] - 0.5
    d = np.abs(lp - np.round(lp)) * cw[:, None]
    near = np.any((d > 0) & (d < dist), axis=1)
    out = np.zeros(len(pts), dtype=bool)
    np.logical_or.at(out, pid, near)
    return ~out


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ns.SPARSE + ns.BORDER)
def test_float64_reconstruction_has_the_oracles_nan_entries(name, form):
    """The oracle reads a corner cell whenever its index lies inside the brick and adds weight * scalar whatever the weight
    (oracle/exa_oracle.c:702-733, the CORNER macro under the index tests; form 1: :786-807, a corner is read iff its three
    per-axis predicates hold and enters fmaf(w, s, ...)): a cell whose hat weight is exactly 0 is still read, and 0 * NaN is
    NaN.  tests/probe_ref64.py does the same (np.where(ok, w, 0) * s with ok the index test).  So value and all three
    components of the numerator are NaN exactly where one of the up to eight cells (l, l + 1 per axis, inside the brick) of
    one of the region's bricks is NaN, on both sides — as long as both take the same l.  float32 rounds (p - lower) / cw - 0.5
    and may land on the other side of a cell-centre plane within a few ulps of it; points exactly on such a plane are exact on
    both sides.  Points nearer than 2^-12 voxels to a plane without lying on it are left out: at most 1 % of the set."""
    idx = 2 if name.startswith("amr3") else 0
    case = ns.named_case(name, "grad", basis_form=form)
    S = case.oracle_scene()
    pts = ps.ref_points(S, idx)
    owner = ps.brute_owner(S, pts)
    recon = r64.Reconstruction(case.scene, S.regions(), S.bricks(), S.leaflist())
    ref = recon.evaluate(pts, owner, (0,))
    ok, v, g = oracle_samples(S, pts, owner, (0,))
    sw = ref["sumW"]
    assert ((sw > 0) & (sw < r64.STATUS_BAND)).sum() == 0
    assert np.array_equal(ok, (owner >= 0)[:, None] & (sw > r64.STATUS_SUMW))     # a NaN cell changes no status
    off = _off_the_planes(recon, pts, owner, 2.0 ** -12)
    assert (~off).mean() <= 0.01
    m = ok & off[:, None]
    nan = np.isnan(v)
    print(f"{name} form {form}: {int(ok.sum())} points with a value, {int((nan & ok).sum())} NaN, {int((~off).sum())} left out")
    assert (nan & m).sum() >= 20 and (~nan & m).sum() >= 200
    assert np.array_equal(np.isnan(ref["value"])[m], nan[m])
    assert np.array_equal(np.isnan(ref["num"])[m], np.isnan(g)[m])
    assert np.array_equal(np.isnan(g).all(axis=-1)[ok], nan[ok]) and np.array_equal(np.isnan(g).any(axis=-1)[ok], nan[ok])
    fin = m & ~nan
    kv, kg = r64.scaled_errors(ref, v, g)
    for stratum in ("covered", "all"):
        s = fin & r64.stratum(ref, stratum)
        print(f"K nan {name} form {form} {stratum}: n {int(s.sum())} K_value {kv[s].max():.4g} K_num {kg[s].max():.4g}")
        assert kv[s].max() <= r64.K_VALUE[stratum][form] and kg[s].max() <= r64.K_NUM[stratum][form], stratum
    S.close()


# ---- known answer: one brick, a constant field, one NaN cell ----
N, CELL, CONST = 8, (3, 4, 2), 0.5


def _one_nan_cell():
    sc = scenes.artificial(scenes.parse_grids(f"0 0 0 {N} {N} {N} 0  {CONST}"), name="const8")
    f = np.array(sc.fields[0], copy=True)
    f[CELL[0] + N * (CELL[1] + N * CELL[2])] = np.nan
    return scenes.Scene(sc.bricks7, sc.cellIDs, [f], name="const8_one_nan")


@pytest.mark.parametrize("form", FORMS)
def test_known_answer_one_nan_cell_in_a_constant_brick(form):
    """The hat function of a cell is positive within one cell width of its centre on every axis (max-norm), and by the
    argument above the cell is read exactly there (on the closed cube, with weight 0 on its surface): samplePoint is NaN
    inside that cube and the constant — to rounding — outside.  Positions at least 1/8 cell away from the cube's surface."""
    sc = _one_nan_cell()
    xf = harness.default_xf()
    xf[:, 3] = 0.0
    xf[0] = (1, 0, 1, 1)                                          # transparent at the constant, the marker at entry 0
    from common import Case
    # (space skipping off: the region's range is the constant alone, which this TF leaves transparent — with skipping on the
    # region is never sampled and the frame is black, asserted below)
    case = Case(sc, W=48, H=48, xf=xf, xf_domains=[ns.TF_DOMAIN], dt=0.25, basis_form=form, space_skipping=0)
    S = case.oracle_scene()
    assert S.num_regions == 1
    centre = np.array(CELL, dtype=np.float64) + 0.5
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(0.0, N, (3000, 3)), centre + rng.uniform(-1.5, 1.5, (4000, 3))]).astype(np.float32)
    d = np.abs(pts.astype(np.float64) - centre).max(axis=1)
    pts, d = pts[np.abs(d - 1.0) >= 0.125], d[np.abs(d - 1.0) >= 0.125]
    ok, v, g = oracle_samples(S, pts, np.zeros(len(pts), dtype=np.int64), (0,))
    assert ok.all() and (d < 1).sum() >= 500 and (d > 1).sum() >= 2000
    assert np.array_equal(np.isnan(v[:, 0]), d < 1) and np.array_equal(np.isnan(g).all(axis=(1, 2)), d < 1)
    assert np.abs(v[d > 1, 0] - CONST).max() <= 4 * 2.0 ** -24
    # the frame: a ray is lit — by the marker alone, pure magenta — only if it meets the cube
    rgba, acc, st = case.run_oracle()
    assert not np.isnan(acc).any()
    lit = acc[..., :3].max(axis=-1) > 0
    assert np.all(acc[..., 1] == 0) and np.array_equal(acc[..., 0], acc[..., 2])
    cam = case.cam(*S.voxel_bounds())
    M = np.stack([cam["dir00"], cam["dirDu"], cam["dirDv"]], axis=1).astype(np.float64)
    corners = centre + np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
    t = np.linalg.solve(M, (np.concatenate([corners, centre[None]]) - cam["pos"].astype(np.float64)).T).T
    u, w = t[:, 1] / t[:, 0], t[:, 2] / t[:, 0]                     # the sample position (sx, sy) in pixels of each point
    ys, xs = np.nonzero(lit)
    assert lit.sum() >= 9
    # a pixel's sample lies in [px, px + 1) x [py, py + 1): a lit pixel lies in the corners' bounding rectangle (1 pixel of slack)
    assert xs.min() >= np.floor(u[:8].min()) - 1 and xs.max() <= np.floor(u[:8].max()) + 1
    assert ys.min() >= np.floor(w[:8].min()) - 1 and ys.max() <= np.floor(w[:8].max()) + 1
    cy, cx = int(np.floor(w[8])), int(np.floor(u[8]))
    assert lit[cy, cx] and np.array_equal(acc[cy, cx, :3], [1, 0, 1])   # through the centre: the first NaN sample is opaque
    case.space_skipping = 1
    assert not case.run_oracle()[1][..., :3].any()
    S.close()
