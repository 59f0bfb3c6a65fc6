"""exa_hip_raycast_iso on the GPU (include/exa_hip.h): per pixel the depth, position, value and gradient of the first crossing
of a value along a ray, its sample index and side and the number of crossings equal, bit for bit, the numpy restatement of
the contract (tests/raycast_ref.py) fed with what the EXISTING point probe (Renderer.samplePoints) returns at the restated
positions — the samples of the march, the midpoints of every round of the refinement and the hit — in both basis forms, with
empty cells, with gaps in the domain, with NaN cells, in world space, across tiles of the image, with any subset of the
outputs — and nothing a frame sets changes a byte.  There is no tolerance in this file.

The rays, the small AMR scene and the world-space case are those of tests/test_gpu_project.py, at 24 x 16 pixels of 48
samples.  Every family asserts, on the reference alone, that it is not vacuous: a quarter of the pixels have a crossing, some
pixel has two, and some refinement ends early (on a bracket that cannot be halved, or on an unusable midpoint)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import probe_sets as ps
import project_ref as pr
import raycast_ref as rr
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from fuzz_cases import random_case
from owlexabrick_amd import binding, scenes
from test_gpu_project import CAMERAS, _struct, _to_world, _world_case, amr3

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, N = 24, 16, 48
SIZE = (W, H)
KEYS = rr.KEYS


def sampler(R, channel=0, world=False):
    """the reference's samples: the existing point probe; with gradient=True its voxel-space gradient"""
    def sample(points, gradient=False):
        values, grads, status = R.samplePoints(points, channels=(channel,), gradient=gradient, normalized=gradient, world=world)
        if gradient:
            return values[:, 0], grads[:, 0, :], status[:, 0]
        return values[:, 0], status[:, 0]
    return sample


def check(R, rays, iso, refine, normalize=False, channel=0, world=False, fill=np.nan, what=""):
    """R.raycast_iso against the restatement; returns (reference dict, its info, what the call returned)"""
    ref, info = rr.raycast(sampler(R, channel, world), rays, iso, refine, normalize, fill)
    got = R.raycast_iso(**rays, iso=iso, refine=refine, channel=channel, world=world, normalize=normalize, fill=fill)
    for k in KEYS:
        assert rr.same_bits(got[k], ref[k]), (what, k, np.argwhere(got[k] != ref[k])[:5])
    return ref, info, got


def shares(ref, info):
    """(pixels with a crossing, pixels with two or more, refinements that ended early)"""
    return (int((ref["index"] >= 0).sum()), int((ref["crossings"] >= 2).sum()),
            int((info["ended_collapsed"] | info["ended_unusable"]).sum()))


def middle_iso(R, rays, normalize=False, channel=0, world=False):
    """an iso value inside the range: the median of the usable samples of these rays (a float32)"""
    p, _ = pr.positions(rays, normalize)
    v, st = sampler(R, channel, world)(np.ascontiguousarray(p.reshape(-1, 3)))
    return f32(np.median(v[rr.usable(v, st)]))


_cache = {}


def setup(form, empty=False):
    key = (form, empty)
    if key not in _cache:
        scene = scenes.with_empty_cells(amr3(), fraction=0.15) if empty else amr3()
        case = Case(scene, basis_form=form, allow_empty_cells=empty, W=32, H=32)
        _cache[key] = (case, case.hip_renderer())
    return _cache[key]


@pytest.mark.parametrize("refine", [0, 1, 7, 32])
@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("form", [0, 1])
def test_crossings_equal_the_point_probe_restated(form, camera, normalize, refine):
    case, R = setup(form)
    rays = CAMERAS[camera](R.prep, normalize, SIZE, N)
    iso = middle_iso(R, rays, normalize)
    ref, info, _ = check(R, rays, iso, refine, normalize, what=(form, camera, normalize, refine))
    hit, multi, early = shares(ref, info)
    print(f"form {form} {camera} normalize {normalize} refine {refine}: iso {iso} hit {hit} of {W * H} multi {multi} early {early}")
    assert 4 * hit >= W * H and multi >= 1
    # a bracket of float32 t cannot be halved 32 times; fewer rounds end early only on an unusable midpoint
    assert early == hit if refine == 32 else early <= hit
    assert np.array_equal(ref["index"] >= 0, ref["crossings"] > 0) and np.array_equal(ref["side"] != 0, ref["index"] >= 0)
    assert set(np.unique(ref["side"])) == {-1, 0, 1}
    # the hit is a valid sample of the field, a float32 rounding or so off the value
    v = ref["value"][ref["index"] >= 0]
    assert np.isfinite(v).all() and np.isfinite(ref["gradient"][ref["index"] >= 0]).all()
    if refine:
        first, _ = rr.raycast(sampler(R), rays, iso, 0, normalize)
        assert np.abs(v - iso).mean() < np.abs(first["value"][ref["index"] >= 0] - iso).mean()
    # the channel is an argument
    check(R, rays, middle_iso(R, rays, normalize, channel=1), refine, normalize, channel=1, what=(form, camera, normalize, refine, "channel 1"))


@pytest.mark.parametrize("form", [0, 1])
def test_iso_below_the_range_and_equal_to_a_sample(form):
    case, R = setup(form)
    rays = CAMERAS["ortho"](R.prep, False, SIZE, N)
    p, _ = pr.positions(rays)
    values, status = sampler(R)(np.ascontiguousarray(p.reshape(-1, 3)))
    ok = rr.usable(values, status)
    # below the minimum: every usable sample is inside, no pixel has a crossing, every float output is the fill
    ref, info, got = check(R, rays, values[ok].min() - f32(1), 7, fill=-3.5, what="below")
    assert shares(ref, info) == (0, 0, 0) and (got["index"] == -1).all() and (got["side"] == 0).all() and (got["crossings"] == 0).all()
    for k in ("t", "position", "value", "gradient"):
        assert (got[k] == f32(-3.5)).all(), k
    # the bits of actual samples: usable ones whose predecessor on the ray is usable and smaller — `>=` puts the sample itself
    # inside, so that pair is a crossing whose interpolation weight is exactly 1
    v3, ok3 = values.reshape(H, W, N), ok.reshape(H, W, N)
    t = pr.times(rays)
    rising = np.argwhere(ok3[..., 1:] & ok3[..., :-1] & (v3[..., 1:] > v3[..., :-1]))
    assert len(rising) >= 100
    for y, x, i0 in rising[:: len(rising) // 5][:5]:
        iso = v3[y, x, i0 + 1]
        ref, info, got = check(R, rays, iso, 0, what=("sample bits", y, x, i0))
        assert ref["crossings"][y, x] >= 1 and ref["index"][y, x] <= i0 + 1
        if ref["index"][y, x] == i0 + 1:
            assert ref["side"][y, x] == 1 and ref["t"][y, x] == t[i0] + f32(1) * (t[i0 + 1] - t[i0])
        hit, multi, _ = shares(ref, info)
        assert hit >= 1
        check(R, rays, iso, 32, what=("sample bits, refined", y, x, i0))


def test_rays_inside_missing_and_of_one_sample():
    case, R = setup(1)
    lo, hi = ps.root_box(R.prep)
    ext = hi - lo
    # origins inside the volume: sample 0 is usable, and whatever side it is on, no crossing is invented at index 0
    rays = pr.rays(lo + 1, (1, 0.25, 0.125), SIZE, 0.0, 0.75, N, orgDu=(0, ext[1] / 32, 0), orgDv=(0, 0, ext[2] / 32))
    iso = middle_iso(R, rays)
    ref, info, _ = check(R, rays, iso, 7, what="origins inside")
    assert (info["status"][..., 0] >= 0).all() and (info["values"][..., 0] >= iso).any() and (ref["index"] != 0).all()
    assert shares(ref, info)[0] >= W * H // 4
    # rays that miss the root box entirely; a direction of zero length, normalised: no samples at all
    for what, r, normalize in (("beside the box", pr.rays((hi[0] + 5, lo[1], lo[2] - 3), (0.1, 0, 1), SIZE, 0.0, 1.0, N, orgDu=(0.5, 0, 0), orgDv=(0, 0.5, 0)), False),
                               ("behind the box", pr.rays(hi + 2, (1, 1, 1), SIZE, 0.0, 1.0, N, orgDu=(0.5, 0, 0), orgDv=(0, 0.5, 0)), True),
                               ("zero direction", pr.rays(lo + 1, (0, 0, 0), SIZE, 0.0, 0.5, N, orgDu=(0, ext[1] / 32, 0)), True)):
        ref, info, got = check(R, r, iso, 7, normalize, what=what)
        assert (info["status"] < 0).all() and (got["index"] == -1).all() and np.isnan(got["t"]).all()
    # one sample per ray: usable samples, and no pair to form a crossing
    one = pr.rays((lo[0] + 0.5, lo[1], lo[2]), (0, 0, 1), SIZE, 0.0, float(ext[2]), 1, orgDu=(0, ext[1] / W, 0))
    ref, info, got = check(R, one, iso, 7, what="one sample")
    assert (info["status"] >= 0).any() and (got["crossings"] == 0).all() and (got["index"] == -1).all()
    # two samples: the smallest ray that can have one
    two = pr.rays((lo[0] + 0.5, lo[1], lo[2]), (0, 0, 1), SIZE, 0.0, float(ext[2]) / 2, 2, orgDu=(ext[0] / W, 0, 0), orgDv=(0, ext[1] / H, 0))
    ref, info, _ = check(R, two, middle_iso(R, two), 32, what="two samples")
    assert shares(ref, info)[0] >= 10 and set(np.unique(ref["index"])) == {-1, 1}


def _gaps(info, iso):
    """(unusable samples between two usable ones of a ray, those whose neighbours lie on different sides of iso)"""
    ok = rr.usable(info["values"], info["status"])
    with np.errstate(invalid="ignore"):
        inside = info["values"] >= iso
    between = ~ok[..., 1:-1] & ok[..., :-2] & ok[..., 2:]
    return int(between.sum()), int((between & (inside[..., :-2] != inside[..., 2:])).sum())


def test_empty_cells_and_gaps_in_the_domain():
    """a pair of usable samples with an unusable one between them is no crossing: cells missing from the bricks (status -2
    where every corner is missing) and bricks missing from the domain (status -1 inside the root box)"""
    case, R = setup(0, empty=True)
    between = across = 0
    for camera in sorted(CAMERAS):
        rays = CAMERAS[camera](R.prep, True, SIZE, N)
        iso = middle_iso(R, rays, True)
        for refine in (0, 7, 32):
            ref, info, _ = check(R, rays, iso, refine, True, what=("empty cells", camera, refine))
        hit, multi, early = shares(ref, info)
        assert 4 * hit >= W * H and multi >= 1 and early == hit
        b, a = _gaps(info, iso)
        between, across = between + b, across + a
    print(f"empty cells: gaps between usable samples {between}, of which across iso {across}")
    assert between >= 1 and across >= 1
    # the `--holes` family of tests/gpu_fuzz.py on random partitions that leave bricks out: seeds whose domain has gaps
    between = across = 0
    for seed in (0, 4):
        fuzz, _ = random_case(seed, grids=True)
        scene = scenes.with_empty_cells(fuzz.scene, fraction=0.1, seed=seed)
        Rg = Case(scene, basis_form=0, allow_empty_cells=True, W=32, H=32).hip_renderer()
        for camera in sorted(CAMERAS):
            rays = CAMERAS[camera](Rg.prep, False, SIZE, N)
            iso = middle_iso(Rg, rays)
            for refine in (1, 32):
                ref, info, _ = check(Rg, rays, iso, refine, what=("grids with holes", seed, camera, refine))
            hit, multi, early = shares(ref, info)
            b, a = _gaps(info, iso)
            between, across = between + b, across + a
            print(f"grids {seed} {camera}: hit {hit} multi {multi} early {early} gaps {b} across iso {a}")
            assert 4 * hit >= W * H and early == hit
        Rg.close()
    assert between >= 10 and across >= 1


def test_nan_cells_are_unusable_samples():
    scene = amr3()
    rng = np.random.default_rng(5)
    field = scene.fields[0].copy()
    field[rng.choice(len(field), size=len(field) // 300, replace=False)] = np.nan
    scene = scenes.Scene(scene.bricks7, scene.cellIDs, [field, scene.fields[1]], name="amr3_nan", value_range=scene.value_range,
                         meta=dict(scene.meta))
    case = Case(scene, W=32, H=32, xf_domains=[(0.0, 1.0), (0.0, 1.0)])
    R = case.hip_renderer()
    clean = setup(1)[1]
    for camera in sorted(CAMERAS):
        rays = CAMERAS[camera](R.prep, True, SIZE, N)
        iso = middle_iso(R, rays, True)
        for refine in (0, 7, 32):
            ref, info, _ = check(R, rays, iso, refine, True, what=("nan", camera, refine))
        hit, multi, early = shares(ref, info)
        nan = np.isnan(info["values"]) & (info["status"] >= 0)
        print(f"nan {camera}: hit {hit} multi {multi} early {early} NaN samples {int(nan.sum())}")
        assert 4 * hit >= W * H and multi >= 1 and early == hit and nan.sum() >= 20
        # the NaN cells take crossings away from the clean scene's image, or move them
        want, _ = rr.raycast(sampler(clean), rays, iso, 0, True)
        assert not np.array_equal(want["crossings"], ref["crossings"])
    R.close()


def _raw_call(R, rays, iso, refine, flags, ptrs, fill=np.nan, device=0):
    L = binding.lib()
    rc = L.exa_hip_raycast_iso(R.h, C.byref(_struct(rays)), 0, float(iso), refine, flags, float(fill), *ptrs, device, None)
    return rc, L.exa_hip_last_error(R.h).decode()


_SHAPES = dict(t=((), f32), position=((3,), f32), value=((), f32), gradient=((3,), f32), index=((), np.int32),
               side=((), np.int32), crossings=((), np.uint32))


def test_null_outputs_change_no_other_array():
    case, R = setup(1)
    rays = CAMERAS["pinhole"](R.prep, True, SIZE, N)
    iso = middle_iso(R, rays, True)
    want, info, _ = check(R, rays, iso, 7, True, what="all outputs")
    assert shares(want, info)[1] >= 1
    # without the counts a ray may stop at its first crossing: the same bytes in every other array
    got = R.raycast_iso(**rays, iso=iso, refine=7, normalize=True, outputs=[k for k in KEYS if k != "crossings"])
    assert sorted(got) == sorted(k for k in KEYS if k != "crossings")
    for k in got:
        assert rr.same_bits(got[k], want[k]), k
    # every subset of the seven outputs, through the C ABI: a skipped array is not touched
    for mask in itertools.product((False, True), repeat=len(KEYS)):
        buf = {k: np.full((H, W) + _SHAPES[k][0], 77, _SHAPES[k][1]) for k in KEYS}
        rc, msg = _raw_call(R, rays, iso, 7, binding.PROJECT_NORMALIZE, [buf[k].ctypes.data if m else None for k, m in zip(KEYS, mask)])
        assert rc == 0, msg
        for k, m in zip(KEYS, mask):
            assert rr.same_bits(buf[k], want[k]) if m else (buf[k] == 77).all(), (mask, k)


def test_device_pointers():
    import torch
    case, R = setup(1)
    rays = CAMERAS["pinhole"](R.prep, True, SIZE, N)
    iso = middle_iso(R, rays, True)
    want = R.raycast_iso(**rays, iso=iso, refine=7, normalize=True)
    dev = torch.device("cuda:0")
    dtypes = dict(t=torch.float32, position=torch.float32, value=torch.float32, gradient=torch.float32, index=torch.int32,
                  side=torch.int32, crossings=torch.int32)
    for skip in ((), ("crossings",), ("t", "gradient", "side")):
        out = {k: torch.full((H, W) + _SHAPES[k][0], 77, dtype=dtypes[k], device=dev) for k in KEYS}
        rc, msg = _raw_call(R, rays, iso, 7, binding.PROJECT_NORMALIZE,
                            [None if k in skip else C.c_void_p(out[k].data_ptr()) for k in KEYS], device=1)
        assert rc == 0, msg
        torch.cuda.synchronize()
        for k in KEYS:
            if k in skip:
                assert bool((out[k] == 77).all()), k
            else:
                assert rr.same_bits(out[k].cpu().numpy().view(want[k].dtype), want[k]), (skip, k)
    assert R.raycastIsoMs() > 0.0


def test_an_image_of_several_tiles():
    """wider than a tile and more pixels than the staging buffer holds with all seven outputs: 2 x 2 tiles, the last column
    of patches 4 pixels wide (host outputs of 44 bytes per pixel: tiles of 4096 x 368).  Two samples per ray, the smallest
    that can cross — one just inside the volume, one at mid-depth — over two voxels square where the field peaks
    (scenes.amr), and the iso value halfway between the two samples of the ray through the middle: every tile has crossings"""
    case, R = setup(1)
    lo, hi = ps.root_box(R.prep)
    ext = hi - lo
    size = (4100, 700)
    corner = (lo[0] + 0.45 * ext[0] - 1, lo[1] + 0.55 * ext[1] - 1, lo[2])
    rays = pr.rays(corner, (0, 0, 1), size, -0.16 * ext[2], 0.44 * ext[2], 2, orgDu=(2.0 / size[0], 0, 0), orgDv=(0, 2.0 / size[1], 0))
    middle = dict(rays, size=(1, 1), orgDu=f32(size[0]) * rays["orgDu"], orgDv=f32(size[1]) * rays["orgDv"])
    p, _ = pr.positions(middle)
    v, st = sampler(R)(np.ascontiguousarray(p.reshape(-1, 3)))
    assert (st >= 0).all() and abs(float(v[1]) - float(v[0])) > 0.05, (v, st)
    ref, info, _ = check(R, rays, f32(0.5) * (v[0] + v[1]), 2, what="tiles")
    hit = ref["index"] == 1
    print(f"tiles: hit share {hit.mean():.3f}, per tile {[float(hit[ys, xs].mean()) for ys in (slice(0, 368), slice(368, None)) for xs in (slice(0, 4096), slice(4096, None))]}")
    assert hit.mean() > 0.5
    assert hit[:368, :4096].any() and hit[:368, 4096:].any() and hit[368:, :4096].any() and hit[368:, 4096:].any()
    assert len(np.unique(ref["t"][hit])) > 1000                                # not one answer repeated


def test_world_space_goes_through_the_transform_like_the_point_probe():
    case, Minv, p = _world_case()
    R = case.hip_renderer()
    for camera in sorted(CAMERAS):
        for normalize in (False, True):
            rays = _to_world(CAMERAS[camera](R.prep, False, SIZE, N), Minv, p)
            if normalize:                                   # M doubles lengths: a world-space unit is two voxels
                unit = float(np.linalg.norm(rays["dir"] + f32(12) * rays["dirDu"] + f32(8) * rays["dirDv"]))
                rays["tmin"], rays["dt"] = f32(rays["tmin"] * unit), f32(rays["dt"] * unit)
            iso = middle_iso(R, rays, normalize, world=True)
            for refine in (0, 7, 32):
                ref, info, got = check(R, rays, iso, refine, normalize, world=True, what=("world", camera, normalize, refine))
            hit, multi, early = shares(ref, info)
            assert 4 * hit >= W * H and multi >= 1 and early == hit, (camera, normalize, hit, multi, early)
            # the position is the caller's: on the world-space ray, not put through the transform
            o, d, _ = pr.origins_and_directions(rays, normalize)
            rows = ref["index"] >= 0
            assert rr.same_bits(got["position"][rows], (o[rows] + got["t"][rows][:, None] * d[rows]).astype(f32))
    # sample_uniform only selects how the lookup is shared
    R.setOption("sample_uniform", 0)
    got = R.raycast_iso(**rays, iso=iso, refine=32, world=True, normalize=True)
    for k in KEYS:
        assert rr.same_bits(got[k], ref[k]), k
    R.close()


def test_world_space_needs_a_frame_state():
    case, R0 = setup(1)
    R = binding.Renderer(R0.prep)                               # no frame state yet
    rays = CAMERAS["pinhole"](R.prep, True, SIZE, N)
    index = np.zeros((H, W), np.int32)
    ptrs = [None, None, None, None, index.ctypes.data, None, None]
    rc, msg = _raw_call(R, rays, 0.5, 7, binding.SAMPLE_WORLD_SPACE | binding.PROJECT_NORMALIZE, ptrs)
    assert rc != 0 and msg.startswith("exa_hip_raycast_iso") and "frame state" in msg, msg
    rc, msg = _raw_call(R, rays, middle_iso(R0, rays, True), 7, binding.PROJECT_NORMALIZE, ptrs)      # voxel space works
    assert rc == 0 and (index >= 0).sum() > 0
    R.close()


def test_bytes_do_not_depend_on_the_frame_state_or_options():
    case = Case(amr3(), W=32, H=32)
    R = case.hip_renderer()
    rays = CAMERAS["pinhole"](R.prep, True, SIZE, N)
    iso = middle_iso(R, rays, True)
    first, info, _ = check(R, rays, iso, 32, True, what="first")
    hit, multi, early = shares(first, info)
    assert 4 * hit >= W * H and multi >= 1 and early == hit

    def same(what):
        got = R.raycast_iso(**rays, iso=iso, refine=32, normalize=True)
        for k in KEYS:
            assert rr.same_bits(got[k], first[k]), (what, k)

    same("two calls")
    R.render()
    same("after a frame")
    for what in frame_perturbations(case, R):
        same(what)
    for uniform in (0, 1):
        R.setOption("sample_uniform", uniform)
        same(f"sample_uniform {uniform}")
        for patch in range(4):
            R.setOption("sample_patch", patch)
            same(f"sample_patch {patch}")
    R.close()


def test_multi_device_handle_equals_single():
    case, R = setup(1)
    rays = CAMERAS["pinhole"](R.prep, True, SIZE, N)
    iso = middle_iso(R, rays, True)
    want = R.raycast_iso(**rays, iso=iso, refine=7, normalize=True)
    assert (want["index"] >= 0).sum() >= W * H // 4
    M = multi_handle(R, 1)
    got = M.raycast_iso(**rays, iso=iso, refine=7, normalize=True)
    for k in KEYS:
        assert rr.same_bits(got[k], want[k]), k
    assert M.raycastIsoMs() > 0.0
    M.close()


def test_scene_without_kd_tree_is_refused():
    R = binding.Renderer(without_kd_tree(binding.Prep(amr3())))
    with pytest.raises(RuntimeError, match="kd-tree"):
        R.raycast_iso(**CAMERAS["pinhole"](R.prep, True, SIZE, N), iso=0.5, normalize=True)
    R.close()


def test_bad_arguments_are_refused_and_the_handle_stays_usable():
    case, R = setup(1)
    L = binding.lib()
    rays = CAMERAS["pinhole"](R.prep, True, SIZE, N)
    iso = middle_iso(R, rays, True)
    want = R.raycast_iso(**rays, iso=iso, refine=7, normalize=True)
    assert (want["index"] >= 0).sum() > 0 and R.raycastIsoMs() > 0.0
    buf = {k: np.zeros((H, W) + _SHAPES[k][0], _SHAPES[k][1]) for k in KEYS}

    def call(s, channel=0, iso=float(iso), refine=7, flags=binding.PROJECT_NORMALIZE):
        rc = L.exa_hip_raycast_iso(R.h, s, channel, iso, refine, flags, float("nan"), *[buf[k].ctypes.data for k in KEYS], 0, None)
        return rc, L.exa_hip_last_error(R.h).decode()

    def edited(**kw):
        s = _struct(rays)
        for k, v in kw.items():
            if isinstance(v, tuple):                        # (index, value) of a vector
                getattr(s, k)[v[0]] = v[1]
            else:
                setattr(s, k, v)
        return C.byref(s)

    nan, inf = float("nan"), float("inf")
    bad = [((None,), {}, "null"),
           ((edited(org=(1, nan)),), {}, "finite"), ((edited(dirDv=(2, inf)),), {}, "finite"), ((edited(orgDu=(0, -inf)),), {}, "finite"),
           ((edited(tmin=nan),), {}, "finite"), ((edited(dt=inf),), {}, "finite"),
           ((edited(dt=0.0),), {}, "dt"), ((edited(dt=-1.0),), {}, "dt"),
           ((edited(numSamples=0),), {}, "numSamples"), ((edited(numSamples=-3),), {}, "numSamples"),
           ((edited(numSamples=binding.PROJECT_MAX_SAMPLES + 1),), {}, "numSamples"),
           ((edited(tmin=3.4e38, dt=1e33, numSamples=binding.PROJECT_MAX_SAMPLES),), {}, "not finite"),
           ((edited(width=0),), {}, "width"), ((edited(height=0),), {}, "width"), ((edited(width=-1),), {}, "width"),
           ((edited(width=65536, height=32768),), {}, "width"),
           ((edited(),), dict(channel=-1), "channel"), ((edited(),), dict(channel=2), "channel"),
           ((edited(),), dict(flags=2), "flag"), ((edited(),), dict(flags=binding.PROJECT_NORMALIZE | 8), "flag"),
           ((edited(),), dict(flags=1 << 30), "flag"),
           ((edited(),), dict(iso=nan), "iso"), ((edited(),), dict(iso=inf), "iso"), ((edited(),), dict(iso=-inf), "iso"),
           ((edited(),), dict(refine=-1), "refine"), ((edited(),), dict(refine=binding.CROSS_MAX_REFINE + 1), "refine")]
    for args, kw, match in bad:
        rc, msg = call(*args, **kw)
        assert rc != 0 and msg.startswith("exa_hip_raycast_iso") and match in msg, (match, kw, rc, msg)
        assert R.raycastIsoMs() == 0.0
        rc, msg = call(edited())                                # ... and the handle still casts
        assert rc == 0, msg
        assert R.raycastIsoMs() > 0.0
        for k in KEYS:
            assert rr.same_bits(buf[k], want[k]), (match, k)
    assert call(edited(), refine=0)[0] == 0 and call(edited(), refine=binding.CROSS_MAX_REFINE)[0] == 0
