"""exa_hip_sample_triangles on the GPU (include/exa_hip.h): per triangle the sum and count of the samples, areaNormal and subdiv
equal, bit for bit, the numpy restatement of the contract (tests/surface_ref.py) fed with what the EXISTING point probe
(Renderer.samplePoints) returns at the restated positions — on iso meshes read where they lie, on hand-made meshes with
every group size and every kind of triangle that is not valid, in both basis forms, with empty cells, in world space, packed
and one wave per triangle — and nothing a frame sets changes a byte.  A NaN sum compares as a NaN."""
import ctypes as C

import numpy as np
import pytest

import probe_sets as ps
import surface_ref as sr
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from test_gpu_histogram import ODD_GRIDS

pytestmark = pytest.mark.gpu

f32 = np.float32
KEYS = ("sum", "count", "areaNormal", "subdiv")
XFM = dict(vx=f32([1.6, 0.3, -0.2]), vy=f32([-0.25, 1.9, 0.4]), vz=f32([0.1, -0.35, 2.2]), p=f32([3.0, -1.5, 2.0]))


def holes3():
    """amr3 with cells missing and, in field 1 alone, more cells holding the poison value: the status differs per channel"""
    sc = scenes.with_empty_cells(scenes.amr(levels=3, fields=3), fraction=0.15)
    rng = np.random.default_rng(11)
    f1 = sc.fields[1].copy()
    f1[rng.random(len(f1)) < 0.5] = f32(-1e20)
    return scenes.Scene(sc.bricks7, sc.cellIDs, [sc.fields[0], f1, sc.fields[2]], name="amr3_holes3", value_range=sc.value_range,
                        meta=dict(sc.meta))


SCENES = {
    "ex3": (lambda: scenes.example("ex3"), False),
    "amr3": (lambda: scenes.amr(levels=3, fields=3), False),
    "amr3_holes": (holes3, True),
    "odd": (lambda: scenes.artificial(scenes.parse_grids(ODD_GRIDS), name="odd"), False),
}
_cache = {}


@pytest.fixture(scope="module", autouse=True)
def _release_shared_renderers():
    yield
    for _, R in _cache.values():
        R.close()
    _cache.clear()


def setup(name, form=1):
    """(case, renderer) of a named scene and basis form, made once and shared (its options are left at their defaults)"""
    make, empty = SCENES[name]
    form = 0 if empty else form
    if (name, form) not in _cache:
        case = Case(make(), basis_form=form, allow_empty_cells=empty, W=32, H=32)
        _cache[name, form] = (case, case.hip_renderer())
    return _cache[name, form]


def channels_of(case, k):
    nf = len(case.scene.fields)
    return tuple([0, nf - 1, 0, min(1, nf - 1)][:k]) if nf < 3 else ((0,), (2, 0), (0, 1, 2), (2, 0, 0, 1))[k - 1]


def sampler(R, channels, world=False):
    """the reference's samples: the existing point probe"""
    def sample(points):
        values, _, status = R.samplePoints(points, channels=channels, world=world)
        return values, status
    return sample


def same(got, ref, what=""):
    for k in KEYS:
        a, b = np.asarray(got[k]), ref[k]
        ok = sr.same_sums(a, b) if k in ("sum", "areaNormal") else sr.same_bits(a, b)
        assert ok, (what, k, np.argwhere(np.atleast_2d(a != b))[:5])


def check(R, verts, tris, channels=(0,), spacing=1.0, max_n=64, world=False, what=""):
    """R.sampleTriangles against the restatement; returns (reference dict, values, status of the reference's samples)"""
    ref, values, status = sr.sample_triangles(sampler(R, channels, world), verts, tris, len(channels), spacing, max_n)
    got = R.sampleTriangles(verts, tris, channels=channels, spacing=spacing, max_n=max_n, world=world)
    same(got, ref, what)
    return ref, values, status


def hand_mesh(prep, seed=0):
    """(verts, tris, spacing, expected n per triangle): at `spacing`, triangles of n = 1, 2, 4, 5, 8 (one block of 64 samples),
    9 (two blocks, the last partial) and 64, several of each small one, at random places in the root box; one that spans the
    whole scene and reaches outside the root box; triangles without area; indices out of range; NaN and infinite vertices"""
    rng = np.random.default_rng(100 + seed)
    lo, hi = ps.root_box(prep)
    ext = (hi - lo).astype(np.float64)
    s = float(ext.min()) / 24.0
    verts, tris, want = [], [], []

    def add(v0, v1, v2, n):
        tris.append([len(verts), len(verts) + 1, len(verts) + 2])
        verts.extend([v0, v1, v2])
        want.append(n)

    for n, copies in ((1, 7), (2, 6), (3, 3), (4, 5), (5, 2), (8, 2), (9, 2), (64, 1)):
        for _ in range(copies):
            L = (n - 0.5) * s                                            # the longest edge: q = n - 0.5 -> ceil = n
            d = rng.standard_normal(3)
            d /= np.linalg.norm(d)
            e = np.cross(d, rng.standard_normal(3))
            e /= np.linalg.norm(e)
            v0 = rng.uniform(lo + 0.1 * ext, hi - 0.1 * ext) - (0.5 * L * d if n < 64 else 0)
            add(v0, v0 + L * d, v0 + 0.45 * L * d + 0.3 * L * e, n)
    add(lo - 0.2 * ext, hi + 0.2 * ext, [hi[0] + 0.2 * ext[0], lo[1] - 0.2 * ext[1], 0.5 * (lo[2] + hi[2])], 64)     # clamped at maxN
    c = 0.5 * (lo + hi)
    add(c, c, c, 1)                                                      # a point
    add(c, c + [2.2 * s, 0, 0], c + [1.1 * s, 0, 0], 3)                  # collinear
    verts, tris = np.array(verts, f32), np.array(tris, np.int32)
    nv = len(verts)
    bad = np.array([[0, 1, nv + 4], [-1, 1, 2], [0, 2 ** 31 - 1, 2], [nv + 4, nv + 5, nv + 6]], np.int32)
    poison = np.array([[np.nan, c[1], c[2]], [np.inf, c[1], c[2]], [3e38, c[1], c[2]], [-3e38, c[1], c[2]]], f32)
    verts = np.concatenate([verts, poison])
    odd = np.array([[0, 1, nv], [0, nv + 1, 1], [nv + 2, nv + 3, 0]], np.int32)        # NaN vertex; infinite vertex; an edge that overflows
    tris = np.concatenate([tris, bad, odd])
    want += [0] * 7
    return verts, tris, s, np.array(want, np.int32)


@pytest.mark.parametrize("pack", [1, 0], ids=["packed", "wave-per-triangle"])
@pytest.mark.parametrize("name,form", [("ex3", 0), ("ex3", 1), ("amr3", 0), ("amr3", 1), ("amr3_holes", 0), ("odd", 1)])
def test_hand_made_mesh_equals_the_point_probe_reduced(name, form, pack):
    case, R = setup(name, form)
    verts, tris, s, want = hand_mesh(R.prep)
    nch = min(3, len(case.scene.fields))
    channels = channels_of(case, nch)
    R.setOption("surface_pack", pack)
    try:
        ref, values, status = check(R, verts, tris, channels, s, 64, what=(name, form, pack))
        # on the reference alone: the case is what it says
        assert np.array_equal(ref["subdiv"], want), (ref["subdiv"], want)
        assert np.isnan(ref["areaNormal"][-7:-3]).all() and np.isnan(ref["areaNormal"][-3]).any()
        assert (ref["count"][want == 0] == 0).all() and sr.same_bits(ref["sum"][want == 0], np.zeros(((want == 0).sum(), nch)))
        print(f"{name} form {form} pack {pack}: samples {len(values)} valid {(status >= 0).sum()} outside {(status == -1).sum()} "
              f"no weight {(status == -2).sum()}")
        covered = ref["count"][:, 0] > 0
        if name == "odd":                                    # a few bricks far apart: most of the root box is gaps
            assert (status >= 0).sum() >= 200 and (status == -1).sum() >= 100 and covered[want >= 8].any()
        else:
            assert (status >= 0).sum() >= 1000 and (status == -1).sum() >= 100
            assert covered[want == 1].any() and covered[want == 2].any() and covered[want == 4].any() and covered[want == 64].all()
        partial = (ref["count"][:, 0] > 0) & (ref["count"][:, 0] < want.astype(np.int64) ** 2)
        assert partial.any()
        if name == "amr3_holes":
            assert (status == -2).sum() >= 10 and ((status[:, 0] >= 0) != (status[:, 1] >= 0)).sum() >= 10
            assert (ref["count"][:, 0] != ref["count"][:, 1]).any()
        # the same triangles in another order: packed groups mix other n, every triangle keeps its bytes
        order = np.random.default_rng(5).permutation(len(tris))
        got = R.sampleTriangles(verts, tris[order], channels=channels, spacing=s, max_n=64)
        same(got, {k: ref[k][order] for k in KEYS}, (name, form, pack, "shuffled"))
        assert R.sampleTrianglesMs() > 0.0
    finally:
        R.setOption("surface_pack", 1)


def small_mesh(prep, m, seed=1):
    """m random small triangles inside the root box grown by 5 %: at spacing 1, n mostly 1 .. 4, now and then up to 9"""
    rng = np.random.default_rng(200 + seed)
    lo, hi = ps.root_box(prep, 0.05)
    v0 = rng.uniform(lo, hi, (m, 3))
    size = np.where(rng.random(m) < 0.1, rng.uniform(4, 8.9, m), rng.uniform(0.2, 3.9, m))
    e1, e2 = rng.standard_normal((m, 3)), rng.standard_normal((m, 3))
    e1 *= (size / np.linalg.norm(e1, axis=1))[:, None]
    e2 *= (0.7 * size / np.linalg.norm(e2, axis=1))[:, None]
    verts = np.concatenate([v0, v0 + e1, v0 + e2]).astype(f32)
    tris = np.stack([np.arange(m), np.arange(m) + m, np.arange(m) + 2 * m], axis=1).astype(np.int32)
    return verts, tris


def test_numbers_of_triangles_around_a_wave():
    case, R = setup("amr3")
    verts, tris = small_mesh(R.prep, 257)
    ref, values, status = check(R, verts, tris, (0, 1), 1.0, 64, what="257")
    ns = set(ref["subdiv"].tolist())
    assert {1, 2, 3, 4} <= ns and max(ns) >= 5 and (status >= 0).sum() >= 500
    for pack in (1, 0):
        R.setOption("surface_pack", pack)
        for m in (1, 63, 64, 65):
            got = R.sampleTriangles(verts, tris[:m], channels=(0, 1), spacing=1.0, max_n=64)
            same(got, {k: ref[k][:m] for k in KEYS}, (pack, m))
    R.setOption("surface_pack", 1)
    # no triangles: nothing happens
    got = R.sampleTriangles(verts, tris[:0], channels=(0, 1))
    assert got["sum"].shape == (0, 2) and got["subdiv"].shape == (0,)


def test_more_triangles_than_one_chunk_of_the_staging_buffer():
    """host arrays go through the 64 MiB staging buffer in chunks: with four channels and every output a triangle takes 80 bytes
    of it, so 900 000 triangles are a whole chunk of 838 860 and a partial one (one sample each: spacing 0, maxN 1)"""
    case, R = setup("amr3")
    rng = np.random.default_rng(12)
    lo, hi = ps.root_box(R.prep, 0.05)
    verts = rng.uniform(lo, hi, (5000, 3)).astype(f32)
    m = 900000
    tris = rng.integers(0, len(verts), (m, 3)).astype(np.int32)
    tris[::1000, 1] = len(verts)                              # now and then a bad index
    assert m * 80 > 64 << 20
    ref, _, status = check(R, verts, tris, (2, 0, 0, 1), 0.0, 1, what="two chunks")
    assert (ref["subdiv"][::1000] == 0).all() and (np.delete(ref["subdiv"], np.s_[::1000]) == 1).all()
    assert (status[-50000:] >= 0).sum() >= 10000 and (ref["count"][-50000:] > 0).any()


@pytest.mark.parametrize("name", ["ex3", "amr3", "amr3_holes"])
def test_iso_mesh_three_ways(name):
    """the mesh of a 12^3 lattice through the flag, read back and passed as host arrays, and as device arrays: the same bytes"""
    import torch
    case, R = setup(name)
    lo, hi = ps.root_box(R.prep)
    V = R.resample(lo, hi, (12, 12, 12), channel=0)
    iso = float(np.median(V[np.isfinite(V)]))
    nch = min(3, len(case.scene.fields))
    channels = channels_of(case, nch)
    spacing = float((hi - lo).min()) / 40.0
    nv, nt = R.extractIsoSurface(lo, hi, (12, 12, 12), iso)
    try:
        assert nt >= 50
        flagged = R.sampleTriangles(channels=channels, spacing=spacing, max_n=64)
        verts, tris, _ = R.readIsoSurface()
        ref, values, status = check(R, verts, tris, channels, spacing, 64, what=(name, "host arrays"))
        same(flagged, ref, (name, "flag"))
        assert (status >= 0).sum() >= 100 and len(set(ref["subdiv"].tolist())) >= 3
        dev = torch.device("cuda:0")
        got = R.sampleTriangles(torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev), channels=channels, spacing=spacing, max_n=64)
        torch.cuda.synchronize()
        same({k: got[k].cpu().numpy().view(ref[k].dtype) for k in KEYS}, ref, (name, "device arrays"))
        # the flag wants no arrays, and a mesh
        L = binding.lib()
        ch = (C.c_int32 * 1)(0)
        rc = L.exa_hip_sample_triangles(R.h, verts.ctypes.data, len(verts), tris.ctypes.data, len(tris), ch, 1, 1.0, 4,
                                        binding.SURFACE_FROM_ISOSURFACE, None, None, None, None, 0, None)
        assert rc != 0 and L.exa_hip_last_error(R.h).decode().startswith("exa_hip_sample_triangles: ")
    finally:
        R.releaseIsoSurface()
    with pytest.raises(RuntimeError, match="exa_hip_sample_triangles: no mesh"):
        R.sampleTriangles(channels=(0,))


def test_spacing_zero_and_exact_quotients():
    case, R = setup("amr3")
    verts, tris = small_mesh(R.prep, 9, seed=2)
    for max_n in (1, 7, 64):
        ref, _, status = check(R, verts, tris, (1,), 0.0, max_n, what=("spacing 0", max_n))
        assert (ref["subdiv"] == max_n).all() and (status >= 0).any()
    # L / spacing exactly an integer: n is that integer; one ulp more of L: the next
    lo, _ = ps.root_box(R.prep)
    v0 = f32([0, lo[1] + 2, lo[2] + 2])                      # x = 0: the float32 sums below are exact
    up = np.nextafter(f32(3), f32(4))
    verts = np.array([v0, v0 + f32([3, 0, 0]), v0 + f32([1, 1, 0]), v0 + f32([up, 0, 0])], f32)
    tris = np.array([[0, 1, 2], [0, 3, 2]], np.int32)
    assert (verts[1] - verts[0])[0] == 3 and (verts[3] - verts[0])[0] == up
    for spacing, n in ((0.75, 4), (0.5, 6), (3.0, 1), (1.0, 3)):
        ref, _, _ = check(R, verts, tris, (0,), spacing, 64, what=("exact", spacing))
        assert ref["subdiv"].tolist() == [n, n + 1], (spacing, ref["subdiv"])
    ref, _, _ = check(R, verts, tris, (0,), 0.75, 4, what="clamped")
    assert ref["subdiv"].tolist() == [4, 4]


@pytest.mark.parametrize("k", [1, 3, 4])
def test_channels(k):
    case, R = setup("amr3")
    verts, tris, s, _ = hand_mesh(R.prep, seed=3)
    channels = channels_of(case, k)
    ref, _, _ = check(R, verts, tris, channels, s, 16, what=("channels", channels))
    if k == 4:                                               # (2, 0, 0, 1): the repeat holds the same bytes
        assert sr.same_sums(ref["sum"][:, 1], ref["sum"][:, 2]) and not sr.same_sums(ref["sum"][:, 0], ref["sum"][:, 1])


def _world(R, verts):
    """voxel-space vertices as world-space ones under XFM (voxel = M world + p), and the transform set on R"""
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    M = np.stack([XFM["vx"], XFM["vy"], XFM["vz"]], axis=1).astype(np.float64)
    with np.errstate(all="ignore"):
        return (np.linalg.inv(M) @ (verts.astype(np.float64) - XFM["p"]).T).T.astype(f32)


@pytest.mark.parametrize("uniform", [0, 1])
def test_world_space_goes_through_the_transform_like_the_point_probe(uniform):
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    verts, tris, s, want = hand_mesh(R.prep, seed=4)
    wverts = _world(R, verts)
    R.setOption("sample_uniform", uniform)
    for pack in (1, 0):
        R.setOption("surface_pack", pack)
        ref, values, status = check(R, wverts, tris, (0, 2), s / 2.0, 64, world=True, what=("world", uniform, pack))
    assert (status >= 0).sum() >= 1000 and (status == -1).sum() >= 100
    # not the voxel-space result
    got = R.sampleTriangles(wverts, tris, channels=(0, 2), spacing=s / 2.0, max_n=64, world=False)
    assert not sr.same_sums(got["sum"], ref["sum"]) and sr.same_sums(got["areaNormal"], ref["areaNormal"])
    # an iso mesh extracted in world space, read where it lies
    lo, hi = wverts[:60].min(axis=0), wverts[:60].max(axis=0)
    V = R.resample(lo, hi, (12, 12, 12), channel=0, world=True)
    nv, nt = R.extractIsoSurface(lo, hi, (12, 12, 12), float(np.median(V[np.isfinite(V)])), world=True)
    assert nt >= 50
    flagged = R.sampleTriangles(channels=(0, 2), spacing=s, max_n=64, world=True)
    v, t, _ = R.readIsoSurface()
    ref, _, _ = check(R, v, t, (0, 2), s, 64, world=True, what="world iso mesh")
    same(flagged, ref, "world iso mesh through the flag")
    R.close()


def test_bytes_do_not_depend_on_the_frame_state_or_options():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    verts, tris, s, _ = hand_mesh(R.prep, seed=6)
    first, _, status = check(R, verts, tris, (0, 1, 2), s, 64, what="first")
    assert (status >= 0).sum() >= 1000

    def again(what):
        same(R.sampleTriangles(verts, tris, channels=(0, 1, 2), spacing=s, max_n=64), first, what)

    again("two calls")
    R.render()
    again("after a frame")
    for what in frame_perturbations(case, R):
        again(what)
    for uniform in (0, 1):
        R.setOption("sample_uniform", uniform)
        for pack in (0, 1):
            R.setOption("surface_pack", pack)
            again(f"sample_uniform {uniform} surface_pack {pack}")
        for patch in range(4):
            R.setOption("sample_patch", patch)
            again(f"sample_patch {patch}")
    R.close()


def test_multi_device_handle_equals_single():
    case, R = setup("amr3")
    verts, tris, s, _ = hand_mesh(R.prep, seed=7)
    want = R.sampleTriangles(verts, tris, channels=(0, 1), spacing=s, max_n=64)
    M = multi_handle(R, 1)
    for pack in (1, 0):
        M.setOption("surface_pack", pack)
        same(M.sampleTriangles(verts, tris, channels=(0, 1), spacing=s, max_n=64), want, ("multi", pack))
    M.close()


def test_constant_field_sums_to_the_count():
    """the one check of meaning: where the field is 1 everywhere, every valid sample is exactly 1.0f in basis form 0 (there sumWV
    is the sum of the very products w * 1.0f whose sum is sumW, in the same order), so the sum of a triangle is its count.
    Form 1 forms the two sums in different associations (products of per-axis sums against fused multiply-adds), its
    constant is 1 within rounding only: that is the point probe's, and every other test here holds form 1 to it bit for bit."""
    sc = scenes.amr(levels=3, fields=1)
    sc = scenes.Scene(sc.bricks7, sc.cellIDs, [np.ones_like(sc.fields[0])], name="amr3_one", value_range=(0.0, 1.0), meta=dict(sc.meta))
    R = Case(sc, basis_form=0, W=32, H=32, xf_domains=[(0.0, 1.0)]).hip_renderer()
    verts, tris, s, want = hand_mesh(R.prep, seed=8)
    for pack in (1, 0):
        R.setOption("surface_pack", pack)
        got = R.sampleTriangles(verts, tris, channels=(0,), spacing=s, max_n=64)
        assert (got["count"] > 0).sum() >= 20 and got["count"].max() > 1000
        assert np.array_equal(got["sum"], got["count"].astype(np.float64)), pack
    # ... and what a caller forms of it: the integral of a triangle that lies inside is its area
    I = binding.surface_integrals(got)
    inside = (got["count"][:, 0].astype(np.int64) == want.astype(np.int64) ** 2) & (want > 0)
    assert inside.sum() >= 10 and np.array_equal(I["integral"][inside, 0], I["area"][inside])
    assert I["invalid_triangles"] == 7 and I["uncovered_triangles"][0] == ((got["count"][:, 0] == 0) & (want > 0)).sum()
    R.close()


def test_device_outputs_and_null_outputs():
    import torch
    case, R = setup("amr3")
    L = binding.lib()
    verts, tris, s, _ = hand_mesh(R.prep, seed=9)
    want = R.sampleTriangles(verts, tris, channels=(0, 1), spacing=s, max_n=64)
    m = len(tris)
    ch = (C.c_int32 * 2)(0, 1)
    dev = torch.device("cuda:0")
    dv, dt = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
    count = torch.full((m, 2), 77, dtype=torch.int32, device=dev)
    normal = torch.full((m, 3), 77, dtype=torch.float32, device=dev)
    rc = L.exa_hip_sample_triangles(R.h, dv.data_ptr(), len(verts), dt.data_ptr(), m, ch, 2, s, 64, 0, None, count.data_ptr(), normal.data_ptr(),
                                    None, 1, None)
    assert rc == 0, L.exa_hip_last_error(R.h).decode()
    torch.cuda.synchronize()
    assert sr.same_bits(count.cpu().numpy().view(np.uint32), want["count"]) and sr.same_sums(normal.cpu().numpy(), want["areaNormal"])
    # on the host: the sums alone; subdiv alone; nothing at all
    total, sub = np.full((m, 2), 77.0), np.full(m, 77, np.int32)
    assert L.exa_hip_sample_triangles(R.h, verts.ctypes.data, len(verts), tris.ctypes.data, m, ch, 2, s, 64, 0, total.ctypes.data, None, None,
                                      None, 0, None) == 0
    assert sr.same_sums(total, want["sum"])
    assert L.exa_hip_sample_triangles(R.h, verts.ctypes.data, len(verts), tris.ctypes.data, m, ch, 2, s, 64, 0, None, None, None,
                                      sub.ctypes.data, 0, None) == 0
    assert sr.same_bits(sub, want["subdiv"])
    assert L.exa_hip_sample_triangles(R.h, verts.ctypes.data, len(verts), tris.ctypes.data, m, ch, 2, s, 64, 0, None, None, None, None, 0, None) == 0


def test_bad_arguments_are_refused_and_the_handle_stays_usable():
    case, R = setup("amr3")
    L = binding.lib()
    verts, tris, s, _ = hand_mesh(R.prep, seed=10)
    want = R.sampleTriangles(verts, tris, channels=(0, 1), spacing=s, max_n=16)
    assert want["count"].sum() > 0
    m = len(tris)
    buf = dict(sum=np.zeros((m, 2)), count=np.zeros((m, 2), np.uint32), areaNormal=np.zeros((m, 3), f32), subdiv=np.zeros(m, np.int32))

    def call(v=verts.ctypes.data, nv=len(verts), t=tris.ctypes.data, nt=m, channels=(0, 1), nch=None, spacing=s, max_n=16, flags=0):
        ch = (C.c_int32 * max(len(channels), 1))(*channels) if channels is not None else None
        rc = L.exa_hip_sample_triangles(R.h, v, nv, t, nt, ch, len(channels) if nch is None else nch, spacing, max_n, flags,
                                        *[buf[k].ctypes.data for k in KEYS], 0, None)
        return rc, L.exa_hip_last_error(R.h).decode()

    R.releaseIsoSurface()
    nan, inf = float("nan"), float("inf")
    bad = [(dict(channels=(), nch=0), "channels"), (dict(channels=(0, 1, 2, 0, 1), nch=5), "channels"), (dict(channels=None, nch=1), "channels"),
           (dict(channels=(0, 3)), "channel"), (dict(channels=(-1,)), "channel"),
           (dict(max_n=0), "maxN"), (dict(max_n=65), "maxN"), (dict(max_n=-4), "maxN"),
           (dict(spacing=-1.0), "spacing"), (dict(spacing=nan), "spacing"), (dict(spacing=inf), "spacing"),
           (dict(flags=2), "flag"), (dict(flags=4), "flag"), (dict(flags=16), "flag"), (dict(flags=1 << 30), "flag"),
           (dict(v=None), "null"), (dict(t=None), "null"),
           (dict(flags=binding.SURFACE_FROM_ISOSURFACE), "NULL"),
           (dict(v=None, t=None, flags=binding.SURFACE_FROM_ISOSURFACE), "no mesh"),
           (dict(nv=2 ** 31), "INT32_MAX"), (dict(nt=2 ** 31), "INT32_MAX")]
    for kw, match in bad:
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith("exa_hip_sample_triangles: ") and match in msg, (kw, rc, msg)
        assert R.sampleTrianglesMs() == 0.0
        rc, msg = call()                                        # ... and the handle still does it
        assert rc == 0, msg
        same(buf, want, kw)


def test_world_space_needs_a_frame_state():
    case, R0 = setup("amr3")
    R = binding.Renderer(R0.prep)                               # no frame state yet
    L = binding.lib()
    verts, tris = small_mesh(R.prep, 20)
    ch = (C.c_int32 * 1)(0)
    count = np.zeros((20, 1), np.uint32)
    args = (verts.ctypes.data, len(verts), tris.ctypes.data, 20, ch, 1, 1.0, 8)
    rc = L.exa_hip_sample_triangles(R.h, *args, binding.SAMPLE_WORLD_SPACE, None, count.ctypes.data, None, None, 0, None)
    msg = L.exa_hip_last_error(R.h).decode()
    assert rc != 0 and msg.startswith("exa_hip_sample_triangles: ") and "frame state" in msg, msg
    rc = L.exa_hip_sample_triangles(R.h, *args, 0, None, count.ctypes.data, None, None, 0, None)          # voxel space works
    assert rc == 0 and count.sum() > 0
    R.close()


def test_scene_without_kd_tree_is_refused():
    R = binding.Renderer(without_kd_tree(binding.Prep(scenes.amr(levels=3, fields=3))))
    verts, tris = small_mesh(R.prep, 20)
    with pytest.raises(RuntimeError, match="exa_hip_sample_triangles: .*kd-tree"):
        R.sampleTriangles(verts, tris)
    R.close()
