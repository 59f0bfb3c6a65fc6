"""Point probes on the GPU (exa_hip_sample_points / exa_hip_resample, include/exa_hip.h): values and gradients equal the CPU
oracle's samplePoint bit for bit, the region lookup equals a brute force over the region domains, and nothing a frame sets
(transfer function, activity, iso values, walk, accel, brick order) changes a result."""
import ctypes as C
import math

import numpy as np
import pytest

from analysis_steps import bits as _bits, frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from probe_sets import brute_owner, grid_positions as _grid_positions, probe_points, region_levels, with_field_of_centres

pytestmark = pytest.mark.gpu

FILL = np.float32(-12345.5)


def _cases():
    out = []
    for nm in ["ex0", "ex1", "ex2", "ex3", "ex4"]:
        out += [(nm, lambda nm=nm: scenes.example(nm), form, False) for form in (0, 1)]
    out += [("amr3", lambda: scenes.amr(levels=3, fields=3), form, False) for form in (0, 1)]
    out += [("gen", lambda: scenes.generated(root=(2, 2, 2), B=4, levels=2), form, False) for form in (0, 1)]
    out += [("amr3_holes", lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=2), fraction=0.15), 0, True)]
    return out


CASES = _cases()
_cache = {}


def _run(idx):
    if idx not in _cache:
        name, make, form, empty = CASES[idx]
        case = Case(make(), basis_form=form, allow_empty_cells=empty)
        R = case.hip_renderer()
        S = case.oracle_scene()
        pts = probe_points(R.prep, seed=idx)
        chans = tuple(range(len(case.scene.fields)))
        v, g, st = R.samplePoints(pts, channels=chans, gradient=True, fill=FILL)
        _cache[idx] = (case, R, S, pts, chans, v, g, st)
    return _cache[idx]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{c[0]}-f{c[2]}" for c in CASES])
def test_probe_equals_oracle_bit_for_bit(idx):
    case, R, S, pts, chans, v, g, st = _run(idx)
    assert len(pts) >= 4000
    owner = brute_owner(R.prep, pts)
    n_ok = n_empty = 0
    for i in range(len(pts)):
        for c in chans:
            s = int(st[i, c])
            if s >= 0:
                ok, ov, og = S.sample_point(s, pts[i], c, True)
                assert ok, (i, c, pts[i])
                assert _bits(v[i, c]) == _bits(ov), (i, c, pts[i], v[i, c], ov)
                assert np.array_equal(_bits(g[i, c]), _bits(og)), (i, c, pts[i], g[i, c], og)
                n_ok += 1
            else:
                assert _bits(v[i, c]) == _bits(FILL) and np.all(_bits(g[i, c]) == _bits(FILL)), (i, c, s)
                if s == -2:                                     # the region exists, the oracle's samplePoint says no
                    assert owner[i] >= 0
                    ok, _, _ = S.sample_point(int(owner[i]), pts[i], c, True)
                    assert not ok, (i, c, pts[i])
                    n_empty += 1
                else:
                    assert s == -1, s
    assert n_ok > len(pts) // 4
    if case.allow_empty_cells:
        assert n_empty > 0


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[f"{c[0]}-f{c[2]}" for c in CASES])
def test_probe_lookup_equals_brute_force(idx):
    case, R, S, pts, chans, v, g, st = _run(idx)
    assert R.prep.ropes()["flags"] & 1, "a leaf's box is its region's domain (trees built by exa_prep)"
    owner = brute_owner(R.prep, pts)
    for c in chans:
        got = st[:, c].astype(np.int64)
        region = np.where(got == -2, owner, got)                # -2: the region is there, its weights vanish
        assert np.array_equal(region, owner), np.nonzero(region != owner)[0][:10]
    assert (owner >= 0).sum() > 0 and (owner < 0).sum() > 0


def _renderer(scene, **kw):
    case = Case(scene, **kw)
    return case, case.hip_renderer()


def test_channels_in_one_call_equal_single_calls():
    _, R = _renderer(scenes.amr(levels=3, fields=3))
    pts = probe_points(R.prep, seed=7)
    v, g, st = R.samplePoints(pts, channels=(2, 0, 1), gradient=True, fill=FILL)
    for k, c in enumerate((2, 0, 1)):
        v1, g1, s1 = R.samplePoints(pts, channels=(c,), gradient=True, fill=FILL)
        assert np.array_equal(_bits(v[:, k]), _bits(v1[:, 0])) and np.array_equal(_bits(g[:, k]), _bits(g1[:, 0]))
        assert np.array_equal(st[:, k], s1[:, 0])
    va, _, _ = R.samplePoints(pts, channels=(1, 1))           # a repeated channel
    assert np.array_equal(_bits(va[:, 0]), _bits(va[:, 1]))


def test_results_do_not_depend_on_frame_state_or_options():
    case, R = _renderer(scenes.amr(levels=3, fields=3), W=32, H=32)
    pts = probe_points(R.prep, seed=3)
    want = R.samplePoints(pts, channels=(0, 1, 2), gradient=True)

    def same(what):
        got = R.samplePoints(pts, channels=(0, 1, 2), gradient=True)
        assert np.array_equal(_bits(got[0]), _bits(want[0])), what
        assert np.array_equal(_bits(got[1]), _bits(want[1])), what
        assert np.array_equal(got[2], want[2]), what

    for what in frame_perturbations(case, R):
        same(what)


def _xfm_np(m, w):
    """xfmPoint in numpy float32: x*vx + (y*vy + (z*vz + p)), one rounding per operation"""
    f = np.float32
    vx, vy, vz, p = (np.asarray(m[k], dtype=f) for k in ("vx", "vy", "vz", "p"))
    w = np.asarray(w, dtype=f)
    return (w[:, 0:1] * vx + (w[:, 1:2] * vy + (w[:, 2:3] * vz + p))).astype(f)


XFM = dict(vx=[1.6, 0.5, -0.2], vy=[-0.4, 1.3, 0.3], vz=[0.25, -0.15, 0.9], p=[3.5, -1.25, 2.0])


def test_world_space_equals_voxel_space_at_mapped_positions():
    _, R = _renderer(scenes.amr(levels=3, fields=2))
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lo, hi = R.prep.voxel_bounds()
    L = np.array([XFM["vx"], XFM["vy"], XFM["vz"]], dtype=np.float64).T    # voxel = L @ world + p
    rng = np.random.default_rng(5)
    vox = rng.uniform(lo - 1, hi + 1, (5000, 3))
    world = np.linalg.solve(L, (vox - np.array(XFM["p"])).T).T.astype(np.float32)
    mapped = _xfm_np(XFM, world)
    a = R.samplePoints(world, channels=(0, 1), gradient=True, world=True, fill=FILL)
    b = R.samplePoints(mapped, channels=(0, 1), gradient=True, fill=FILL)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert (a[2] >= 0).sum() > 1000


def test_world_space_without_frame_state_is_refused():
    _, R = _renderer(scenes.example("ex3"))                   # no render yet: the module holds no frame state
    pts = np.zeros((1, 3), np.float32)
    vals = np.zeros(1, np.float32)
    ch = np.zeros(1, np.int32)
    rc = binding.lib().exa_hip_sample_points(R.h, pts.ctypes.data, 1, ch.ctypes.data, 1, binding.SAMPLE_WORLD_SPACE, 0.0,
                                             vals.ctypes.data, None, None, 0, None, 0)
    assert rc != 0 and "frame state" in binding.lib().exa_hip_last_error(R.h).decode()
    lo = (C.c_float * 3)(0, 0, 0)
    hi = (C.c_float * 3)(1, 1, 1)
    dims = (C.c_int32 * 3)(2, 2, 2)
    out = np.zeros(8, np.float32)
    rc = binding.lib().exa_hip_resample(R.h, lo, hi, dims, 0, binding.SAMPLE_WORLD_SPACE, 0.0, out.ctypes.data, 0, None, 0)
    assert rc != 0 and "frame state" in binding.lib().exa_hip_last_error(R.h).decode()


def test_normalized_gradient_of_a_linear_field():
    slope = np.array([0.75, -0.5, 1.25], dtype=np.float64)
    scene = scenes.with_extra_field(scenes.example("ex2"), lambda c: (c.astype(np.float64) @ slope + 2.0))   # one level
    _, R = _renderer(scene)
    lo, hi = R.prep.voxel_bounds()
    rng = np.random.default_rng(11)
    pts = rng.uniform(lo + 0.5, hi - 0.5, (4000, 3)).astype(np.float32)    # between the outermost cell centres
    v, g, st = R.samplePoints(pts, channels=(1,), gradient=True, normalized=True)
    assert np.all(st[:, 0] >= 0)
    exact = pts.astype(np.float64) @ slope + 2.0
    np.testing.assert_allclose(v[:, 0], exact, rtol=1e-5, atol=0)
    np.testing.assert_allclose(g[:, 0], np.broadcast_to(slope, (len(pts), 3)), rtol=1e-4, atol=0)
    # inside, the weights sum to 1 and the numerator is the gradient already; in the outer half cell (x below the first
    # cell centre) they do not, and the normalisation divides the numerator by sumW^2
    edge = pts[:500].copy()
    edge[:, 0] = rng.uniform(lo[0] + 0.01, lo[0] + 0.49, 500).astype(np.float32)
    _, gn, se = R.samplePoints(edge, channels=(1,), gradient=True, normalized=True)
    _, g1, _ = R.samplePoints(edge, channels=(1,), gradient=True)
    assert np.all(se >= 0)
    assert np.all(np.abs(gn[:, 0, 1]) > np.abs(g1[:, 0, 1]))      # sumW < 1: the numerator of d/dy is sumW^2 * slope.y
    np.testing.assert_allclose(gn[:, 0, 1], slope[1], rtol=1e-4)
    R.close()
    # three levels: inside a brick of level L, a cell width and more from the faces of its region, the weights sum to 1
    # and the interpolant of a linear field is that field, whatever the cell width: the normalized gradient is the slope in
    # VOXEL space, where the numerator is the slope per cell, 2^L times as much
    scene = with_field_of_centres(scenes.amr(levels=3), lambda c: c @ slope + 2.0)
    _, R = _renderer(scene)
    combos = region_levels(R.prep)
    dom = np.stack([np.stack(list(R.prep.regions()[k])) for k in ("dom_lo", "dom_hi")], axis=1).astype(np.float64)
    for level in (0, 1, 2):
        cw = float(1 << level)
        ids = np.array([i for i, c in enumerate(combos) if c == (level,) and np.all(dom[i, 1] - dom[i, 0] > 2 * cw)])
        assert len(ids) > 0, level
        pick = dom[ids[rng.integers(len(ids), size=600)]]
        pts = rng.uniform(pick[:, 0] + cw, pick[:, 1] - cw).astype(np.float32)
        pts = pts[np.all((pts >= pick[:, 0] + cw) & (pts <= pick[:, 1] - cw), axis=1)]     # after the rounding to float32
        assert len(pts) >= 500, level
        v, gn, st = R.samplePoints(pts, channels=(1,), gradient=True, normalized=True)
        _, g1, _ = R.samplePoints(pts, channels=(1,), gradient=True)
        assert np.array_equal(st[:, 0], brute_owner(R.prep, pts)) and np.all(np.isin(st[:, 0], ids)), level
        np.testing.assert_allclose(v[:, 0], pts.astype(np.float64) @ slope + 2.0, rtol=1e-5, atol=0)
        np.testing.assert_allclose(gn[:, 0], np.broadcast_to(slope, (len(pts), 3)), rtol=1e-4, atol=0, err_msg=f"level {level}")
        np.testing.assert_allclose(g1[:, 0], np.broadcast_to(slope * cw, (len(pts), 3)), rtol=1e-4, atol=0)
    R.close()


@pytest.mark.parametrize("world", [False, True], ids=["voxel", "world"])
def test_grid_equals_points(world):
    import torch
    _, R = _renderer(scenes.amr(levels=3, fields=2))
    if world:
        R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lo, hi = R.prep.voxel_bounds()
    ext = hi - lo
    boxes = [((lo - 0.1 * ext), (hi + 0.1 * ext), (37, 29, 21)),   # reaching outside the scene
             (lo, hi, (64, 48, 1)),                                # an axis with n = 1
             (lo + 0.3 * ext, hi - 0.2 * ext, (1, 17, 66))]
    if world:
        boxes = [(np.array([-4, -6, -5], np.float32), np.array([30, 24, 26], np.float32), (41, 33, 27))]
    for blo, bhi, dims in boxes:
        blo, bhi = np.asarray(blo, np.float32), np.asarray(bhi, np.float32)
        grid = R.resample(blo, bhi, dims, channel=1, world=world, fill=FILL)
        pos = _grid_positions(blo, bhi, dims)
        v, _, st = R.samplePoints(pos, channels=(1,), world=world, fill=FILL)
        assert np.array_equal(grid.reshape(-1).view(np.uint32), v[:, 0].view(np.uint32)), dims
        assert (st >= 0).sum() > 0
        dev = torch.empty(int(np.prod(dims)), dtype=torch.float32, device="cuda:0")
        R.resample(blo, bhi, dims, channel=1, world=world, fill=FILL, out_ptr=dev)
        assert np.array_equal(dev.cpu().numpy().view(np.uint32), grid.reshape(-1).view(np.uint32))


def test_bad_grid_arguments_are_refused():
    _, R = _renderer(scenes.example("ex3"))
    bad = [((0, 0, 0), (1, 1, 1), (0, 4, 4)), ((0, 0, 0), (1, 0, 1), (4, 4, 4)), ((0, math.nan, 0), (1, 1, 1), (4, 4, 4)),
           ((0, 0, 0), (1, math.inf, 1), (4, 4, 4)), ((0, 0, 0), (1, 1, 1), (4, -1, 4))]
    for lo, hi, dims in bad:
        with pytest.raises(RuntimeError, match="exa_hip_resample"):
            R.resample(lo, hi, dims)
    with pytest.raises(RuntimeError, match="channel"):
        R.resample((0, 0, 0), (1, 1, 1), (2, 2, 2), channel=3)
    lo, hi, dims = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(2, 2, 2)
    out = np.zeros(8, np.float32)
    for flags in (2, 8, 1 << 30):
        assert binding.lib().exa_hip_resample(R.h, lo, hi, dims, 0, flags, 0.0, out.ctypes.data, 0, None, 0) != 0
        assert "flag" in binding.lib().exa_hip_last_error(R.h).decode()
    pts = np.zeros((1, 3), np.float32)
    vals = np.zeros(4, np.float32)
    ch = np.zeros(1, np.int32)
    for flags in (8, 4):                                        # unknown bit; normalized without gradient
        assert binding.lib().exa_hip_sample_points(R.h, pts.ctypes.data, 1, ch.ctypes.data, 1, flags, 0.0, vals.ctypes.data,
                                                   vals.ctypes.data, None, 0, None, 0) != 0
        assert "EXA_SAMPLE" in binding.lib().exa_hip_last_error(R.h).decode() or "flag" in binding.lib().exa_hip_last_error(R.h).decode()
    with pytest.raises(RuntimeError, match="channel"):
        R.samplePoints(pts, channels=(1,))
    with pytest.raises(RuntimeError, match="channels"):
        R.samplePoints(pts, channels=tuple(range(11)))
    v, g, st = R.samplePoints(np.zeros((0, 3), np.float32))    # n == 0 does nothing
    assert v.shape == (0, 1)


def test_grid_beyond_two_to_the_32_points():
    import torch
    _, R = _renderer(scenes.amr(levels=2))
    lo, hi = R.prep.voxel_bounds()
    dims = (2048, 2048, 1025)
    n = dims[0] * dims[1] * dims[2]
    assert n > 2 ** 32
    out = torch.empty(n, dtype=torch.float32, device="cuda:0")
    R.resample(lo, hi, dims, fill=FILL, out_ptr=out)
    pos = _grid_positions(lo, hi, dims[:2] + (1,))
    slice_len = dims[0] * dims[1]
    f = np.float32
    for z in (dims[2] // 2, dims[2] - 1):
        zc = lo[2] + (f(z) + f(0.5)) * ((hi[2] - lo[2]) / f(dims[2]))
        p = pos.copy()
        p[:, 2] = zc
        want, _, st = R.samplePoints(torch.from_numpy(p).cuda(), fill=FILL)
        got = out[z * slice_len:(z + 1) * slice_len]
        assert torch.equal(got.view(torch.int32), want[:, 0].contiguous().view(torch.int32)), z
        assert int((st >= 0).sum()) > 0
    del out
    torch.cuda.empty_cache()


def test_multi_device_handle_equals_single():
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    pts = probe_points(R.prep, seed=9)
    want = R.samplePoints(pts, channels=(0, 1), gradient=True)
    lo, hi = R.prep.voxel_bounds()
    gw = R.resample(lo, hi, (20, 18, 9), channel=1)
    M = multi_handle(R)
    got = M.samplePoints(pts, channels=(0, 1), gradient=True)
    for x, y in zip(want, got):
        assert np.array_equal(np.asarray(x).view(np.uint32), np.asarray(y).view(np.uint32))
    assert np.array_equal(M.resample(lo, hi, (20, 18, 9), channel=1).view(np.uint32), gw.view(np.uint32))
    M.close()


def test_scene_without_kd_tree_is_refused():
    R = binding.Renderer(without_kd_tree(binding.Prep(scenes.amr(levels=3))))
    with pytest.raises(RuntimeError, match="kd-tree"):
        R.samplePoints(np.zeros((4, 3), np.float32))
    with pytest.raises(RuntimeError, match="kd-tree"):
        R.resample((0, 0, 0), (1, 1, 1), (2, 2, 2))
    R.close()


def test_async_on_a_torch_stream_equals_sync():
    import torch
    _, R = _renderer(scenes.amr(levels=3, fields=2))
    pts = probe_points(R.prep, seed=4)
    want = R.samplePoints(pts, channels=(1, 0), gradient=True, normalized=True)
    dpts = torch.from_numpy(pts).cuda()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = R.samplePoints(dpts, channels=(1, 0), gradient=True, normalized=True, stream=s.cuda_stream, async_=True)
    s.synchronize()
    for x, y in zip(want, got):
        assert np.array_equal(x.view(np.uint32), y.cpu().numpy().view(np.uint32))
    lo, hi = R.prep.voxel_bounds()
    gw = R.resample(lo, hi, (33, 17, 12))
    out = torch.empty(33 * 17 * 12, dtype=torch.float32, device="cuda:0")
    with torch.cuda.stream(s):
        R.resample(lo, hi, (33, 17, 12), out_ptr=out, stream=s.cuda_stream, async_=True)
    s.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), gw.reshape(-1).view(np.uint32))
