"""exa_hip_project on the GPU (include/exa_hip.h): per pixel the sum, count, maximum, minimum and index of the maximum of the
samples along a ray equal, bit for bit, the numpy restatement of the contract (tests/project_ref.py) fed with what the
EXISTING point probe (Renderer.samplePoints) returns at the restated positions — in both basis forms, with empty cells, with
NaN cells, in world space, at the edges of the index range the kernel skips, across tiles of the image — and nothing a frame
sets changes a byte.

The loop guard of the kd descent (return code 3) cannot be reached from here: a tree that could trip it is refused where it
enters the module (tests/test_gpu_streamlines.py::test_a_cyclic_kd_tree_never_reaches_the_descent holds that)."""
import ctypes as C

import numpy as np
import pytest

import probe_sets as ps
import project_ref as pr
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, harness, scenes

pytestmark = pytest.mark.gpu

f32 = np.float32
W, H, N = 20, 13, 96                      # partial 8 x 8 patches on both axes
KEYS = ("sum", "count", "max", "min", "max_index")


def amr3():
    return scenes.amr(levels=3, fields=2)


def ortho_rays(prep, normalize, size=(W, H), n=N):
    """parallel rays, slightly tilted against z, whose origins cover the root box grown by 10 % in x and y and whose samples
    span more than its depth"""
    glo, ghi = ps.root_box(prep, 0.1)
    ext = ghi - glo
    d = np.array([0.15, -0.1, 1.0], f32)
    length = float(np.sqrt(np.dot(d.astype(np.float64), d.astype(np.float64))))
    unit = length if normalize else 1.0                  # t per unit of |d|
    org = glo - f32(0.5) * ext[2] * np.array([0.15, -0.1, 0.0], f32)
    return pr.rays(org, d, size, -1.0 * unit, 1.15 * float(ext[2]) * unit / n, n,
                   orgDu=(ext[0] / size[0], 0, 0), orgDv=(0, ext[1] / size[1], 0))


def pinhole_rays(prep, normalize, size=(W, H), n=N):
    """a pinhole camera off a corner of the grown root box, looking at its centre"""
    glo, ghi = ps.root_box(prep, 0.1)
    ext = (ghi - glo).astype(np.float64)
    centre = 0.5 * (glo + ghi)
    origin = (centre + np.array([-.9, .7, 1.3]) * ext).astype(f32)
    cam = harness.camera(origin, centre, [0, 1, 0], 30.0, size[0], size[1])
    dist, diag = float(np.linalg.norm(origin - centre)), float(np.linalg.norm(ext))
    mid = cam["dir00"] + f32(0.5 * size[0]) * cam["dirDu"] + f32(0.5 * size[1]) * cam["dirDv"]
    unit = 1.0 if normalize else 1.0 / float(np.linalg.norm(mid))          # t per voxel
    t0, t1 = (dist - 0.62 * diag) * unit, (dist + 0.62 * diag) * unit
    return pr.rays(cam["pos"], cam["dir00"], size, t0, (t1 - t0) / n, n, dirDu=cam["dirDu"], dirDv=cam["dirDv"])


CAMERAS = {"ortho": ortho_rays, "pinhole": pinhole_rays}


def sampler(R, channel=0, world=False):
    """the reference's samples: the existing point probe"""
    def sample(points):
        values, _, status = R.samplePoints(points, channels=(channel,), world=world)
        return values[:, 0], status[:, 0]
    return sample


def check(R, rays, normalize=False, channel=0, world=False, what="", nan_sum=False):
    """R.project against the restatement; returns (reference dict, values, status) of the reference"""
    ref, values, status = pr.project(sampler(R, channel, world), rays, normalize)
    got = R.project(**rays, channel=channel, world=world, normalize=normalize)
    for k in KEYS:
        a, b = got[k], ref[k]
        if k == "sum" and nan_sum:            # which NaN a sum of several NaNs is, IEEE leaves open: NaN where the reference is
            assert np.array_equal(np.isnan(a), np.isnan(b)), (what, k)
            a, b = np.where(np.isnan(a), 0.0, a), np.where(np.isnan(b), 0.0, b)
        assert pr.same_bits(a, b), (what, k, np.argwhere(a != b)[:5])
    return ref, values, status


_cache = {}


def setup(form, empty=False):
    key = (form, empty)
    if key not in _cache:
        scene = scenes.with_empty_cells(amr3(), fraction=0.15) if empty else amr3()
        case = Case(scene, basis_form=form, allow_empty_cells=empty, W=32, H=32)
        _cache[key] = (case, case.hip_renderer())
    return _cache[key]


@pytest.mark.parametrize("normalize", [False, True], ids=["raw", "normalized"])
@pytest.mark.parametrize("camera", sorted(CAMERAS))
@pytest.mark.parametrize("form", [0, 1])
def test_projection_equals_the_point_probe_reduced(form, camera, normalize):
    case, R = setup(form)
    rays = CAMERAS[camera](R.prep, normalize)
    ref, values, status = check(R, rays, normalize, what=(form, camera, normalize))
    # on the reference alone: the case is not vacuous
    valid = status >= 0
    count = ref["count"]
    print(f"form {form} {camera} normalize {normalize}: valid {valid.sum()} empty px {(count == 0).sum()} "
          f"partial px {((count > 0) & (count < N)).sum()}")
    assert valid.sum() >= 2000
    assert (count == 0).sum() >= 20
    assert ((count > 0) & (count < N)).sum() >= 20
    levels = ps.region_levels(R.prep)
    classes = {ps.level_class(levels[r]) for r in np.unique(status[valid])}
    assert classes == {"single", "coarse", "mixed"}, classes
    # the channel is an argument
    check(R, rays, normalize, channel=1, what=(form, camera, normalize, "channel 1"))


def test_edges_of_the_skipped_index_range():
    """orthographic rays of exactly representable numbers against the integer root box: where the bisection's two ends fall
    on, next to and outside the box's faces"""
    case, R = setup(1)
    lo, hi = ps.root_box(R.prep)
    assert np.all(lo == np.round(lo)) and np.all(hi == np.round(hi))
    size = (9, 10)
    ext = hi - lo
    du, dv = (0, ext[1] / 8, 0), (0, 0, ext[2] / 8)                    # pixel centres from lo + ext/16 on, the last ones outside

    def along_x(x):
        # rays along z in the plane of constant x (the image's axes: y and nothing)
        return pr.rays((x, lo[1], lo[2]), (0, 0, 1), size, -4.0, 0.5, 96, orgDu=du)

    # in the closed upper face x = hi.x and one ulp outside it, and the same on the lower face.  A position in a face of the
    # root box is inside the box and inside a region's closed domain, but the hat weights of the outermost cells end there:
    # its status is -2, not -1 — no image can tell the two apart, so the reference's status says which case this is
    for face, out in ((hi[0], np.inf), (lo[0], -np.inf)):
        ref, _, status = check(R, along_x(face), what=("in the face", face))
        assert (status == -2).any()
        ref, _, status = check(R, along_x(np.nextafter(face, f32(out))), what=("one ulp outside the face", face))
        assert (status == -1).all()
    # samples that land exactly on the faces z = lo.z and z = hi.z: the first and the last index inside the root box
    dom = ps.domains(R.prep)
    for upper in (False, True):
        touching = dom[dom[:, 5] == hi[2]] if upper else dom[dom[:, 2] == lo[2]]
        x, y = 0.5 * (touching[0, 0] + touching[0, 3]), 0.5 * (touching[0, 1] + touching[0, 4])      # through a region on that face
        rays = pr.rays((x, y, lo[2] - 4.25), (0, 0, 1), size, 0.0, 0.5, 96, orgDu=(0, 2.0 ** -6, 0))
        ref, _, status = check(R, rays, what=("on the z faces", upper))
        p, _ = pr.positions(rays)
        k = int(np.flatnonzero(p[0, 0, :, 2] == (hi[2] if upper else lo[2]))[0])
        assert status[0, 0, k] == -2 and status[0, 0, k + (1 if upper else -1)] == -1 and status[0, 0, k - (1 if upper else -1)] >= 0
    # one zero component; two negative components and a zero one; all negative from beyond the upper corner
    check(R, pr.rays((lo[0] - 3, lo[1] + 0.5, lo[2] - 1), (1, 0, 0.5), size, 0.0, 0.75, 96, orgDu=du, orgDv=dv), what="one zero component")
    check(R, pr.rays((hi[0] + 3, hi[1] + 2, lo[2]), (-1, -0.5, 0), size, 0.0, 0.75, 96, orgDu=(0, -ext[1] / 8, 0), orgDv=dv),
          what="negative directions")
    ref, _, _ = check(R, pr.rays(hi + 4, (-1, -0.5, -0.25), size, 0.0, 0.75, 96, orgDu=(0, -ext[1] / 8, 0), orgDv=(0, 0, -ext[2] / 8)),
                      what="all negative")
    assert ref["count"].max() > 0
    # -0.0 as a direction component is a zero
    check(R, pr.rays((lo[0] - 3, lo[1] + 0.5, lo[2] + 0.5), (1, -0.0, -0.0), size, 0.0, 0.75, 96, orgDu=du, orgDv=dv), what="negative zeros")
    # origins inside the box: the range begins at index 0; and ends at the last index where the rays stay inside
    ref, _, status = check(R, pr.rays(lo + 1, (1, 0.25, 0.125), size, 0.0, 0.75, 96, orgDu=(0, ext[1] / 16, 0), orgDv=(0, 0, ext[2] / 16)),
                           what="origins inside")
    assert (status[..., 0] >= 0).any()
    ref, _, status = check(R, pr.rays(lo + 1, (1, 0.25, 0.125), size, 0.0, 0.125, 96, orgDu=(0, ext[1] / 16, 0), orgDv=(0, 0, ext[2] / 16)),
                           what="rays that end inside")
    assert (status[..., -1] >= 0).any() and (ref["count"] == 96).any()
    # tmin beyond the box
    ref, _, _ = check(R, pr.rays((lo[0] - 3, lo[1] + 0.5, lo[2] + 0.5), (1, 0, 0), size, 2 * ext[0] + 10, 0.75, 96, orgDu=du, orgDv=dv),
                      what="tmin beyond the box")
    assert ref["count"].max() == 0
    # a far origin, 10^4 box sizes away: t_i is spaced wider than dt, so positions repeat
    far = pr.rays((lo[0] - 1e4 * ext[0], lo[1] + 0.5, lo[2] + 0.5), (1, 0, 0), size, 1e4 * ext[0] - 1, 0.01, 4096, orgDu=du, orgDv=dv)
    t = pr.times(far)
    assert (np.diff(t) == 0).sum() > 1000 and np.all(np.diff(t) >= 0)
    ref, _, _ = check(R, far, what="far origin")
    assert ref["count"].max() > 0
    # 4096 samples of which under 5 % lie inside
    ref, _, status = check(R, pr.rays((lo[0] - 1000, lo[1] + 0.5, lo[2] + 0.5), (1, 0, 0), size, 0.0, 0.5, 4096, orgDu=du, orgDv=dv),
                           what="4096 samples")
    share = (status >= 0).mean()
    assert 0 < share < 0.05, share
    # one sample
    ref, _, _ = check(R, pr.rays((lo[0] + 0.5, lo[1], lo[2]), (0, 0, 1), size, 0.0, 20.0, 1, orgDu=du), what="one sample")
    assert 0 < (ref["count"] == 1).sum() < size[0] * size[1]
    assert set(np.unique(ref["max_index"])) == {-1, 0}
    # a direction of zero length, raw (every sample at the origin) and normalised (no samples)
    ref, _, _ = check(R, pr.rays(lo + 1, (0, 0, 0), size, 0.0, 0.5, 8, orgDu=(0, ext[1] / 16, 0)), what="zero direction")
    assert (ref["count"] == 8).any()
    ref, _, _ = check(R, pr.rays(lo + 1, (0, 0, 0), size, 0.0, 0.5, 8, orgDu=(0, ext[1] / 16, 0)), normalize=True, what="zero direction, normalised")
    assert ref["count"].max() == 0
    # directions that overflow float32 (finite inputs): infinite or NaN positions, no samples
    ref, _, _ = check(R, pr.rays(lo + 1, (3e38, 0, 0), size, 0.0, 0.5, 8, dirDu=(3e38, 0, 0), dirDv=(-3e38, 0, 0)), what="overflow")
    assert ref["count"].max() == 0


def test_empty_cells():
    case, R = setup(0, empty=True)
    seen = 0
    for camera in sorted(CAMERAS):
        ref, values, status = check(R, CAMERAS[camera](R.prep, True), True, what=("empty cells", camera))
        seen += int((status == -2).sum())
        assert (status >= 0).sum() >= 1000
    assert seen >= 1


def test_nan_cells_poison_the_sum_only():
    scene = amr3()
    rng = np.random.default_rng(5)
    field = scene.fields[0].copy()
    field[rng.choice(len(field), size=len(field) // 300, replace=False)] = np.nan
    scene = scenes.Scene(scene.bricks7, scene.cellIDs, [field, scene.fields[1]], name="amr3_nan", value_range=scene.value_range,
                         meta=dict(scene.meta))
    case = Case(scene, W=32, H=32, xf_domains=[(0.0, 1.0), (0.0, 1.0)])
    R = case.hip_renderer()
    for camera in sorted(CAMERAS):
        ref, values, status = check(R, CAMERAS[camera](R.prep, True), True, what=("nan", camera), nan_sum=True)
        poisoned = np.isnan(ref["sum"])
        print(f"nan {camera}: poisoned px {poisoned.sum()} clean px {(~poisoned & (ref['count'] > 0)).sum()}")
        assert poisoned.sum() >= 5 and (~poisoned & (ref["count"] > 0)).sum() >= 1
        # a NaN counts, and never becomes max or min
        assert np.array_equal(ref["count"], (status >= 0).sum(axis=2).astype(np.uint32))
        assert not np.isnan(ref["max"]).any() and not np.isnan(ref["min"]).any()
        some = poisoned & (np.where(status >= 0, ~np.isnan(values), False).sum(axis=2) > 0)
        assert some.sum() >= 5 and np.isfinite(ref["max"][some]).all() and np.isfinite(ref["min"][some]).all()
    R.close()


def _world_case():
    """voxel = M world + p with M a rotation about a skew axis times 2: no axis of the world is an axis of the voxel grid"""
    axis = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    ang = 0.7
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    M = 2.0 * (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K)
    p = np.array([3.0, -1.5, 2.0])
    xfm = dict(vx=M[:, 0].astype(f32), vy=M[:, 1].astype(f32), vz=M[:, 2].astype(f32), p=p.astype(f32))
    cam = dict(pos=np.array([0, 0, -100], f32), dir00=np.array([-1, -1, 1], f32), dirDu=np.array([.06, 0, 0], f32),
               dirDv=np.array([0, .06, 0], f32))
    return Case(amr3(), W=32, H=32, xfm=xfm, camera=cam), np.linalg.inv(M), p


def _to_world(rays, Minv, p):
    out = dict(rays)
    out["org"] = (Minv @ (rays["org"].astype(np.float64) - p)).astype(f32)
    for k in ("orgDu", "orgDv", "dir", "dirDu", "dirDv"):
        out[k] = (Minv @ rays[k].astype(np.float64)).astype(f32)
    return out


def test_world_space_goes_through_the_transform_like_the_point_probe():
    case, Minv, p = _world_case()
    R = case.hip_renderer()
    for camera in sorted(CAMERAS):
        for normalize in (False, True):
            rays = _to_world(CAMERAS[camera](R.prep, False), Minv, p)
            if normalize:                                   # M doubles lengths: a world-space unit is two voxels
                unit = float(np.linalg.norm(rays["dir"] + f32(10) * rays["dirDu"] + f32(6.5) * rays["dirDv"]))
                rays["tmin"], rays["dt"] = f32(rays["tmin"] * unit), f32(rays["dt"] * unit)
            ref, values, status = check(R, rays, normalize, world=True, what=("world", camera, normalize))
            assert (status >= 0).sum() >= 1500 and (ref["count"] == 0).sum() >= 10, (camera, normalize, (status >= 0).sum())
    R.close()


def test_bytes_do_not_depend_on_the_frame_state_or_options():
    case = Case(amr3(), W=32, H=32)
    R = case.hip_renderer()
    rays = pinhole_rays(R.prep, True)
    first, _, status = check(R, rays, True, what="first")
    assert (status >= 0).sum() >= 2000

    def same(what):
        got = R.project(**rays, normalize=True)
        for k in KEYS:
            assert pr.same_bits(got[k], first[k]), (what, k)

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


def test_sample_uniform_does_not_change_world_space_bytes():
    case, Minv, p = _world_case()
    R = case.hip_renderer()
    rays = _to_world(ortho_rays(R.prep, False), Minv, p)
    R.setOption("sample_uniform", 0)
    ref, _, _ = check(R, rays, world=True, what="per lane")
    R.setOption("sample_uniform", 1)
    got = R.project(**rays, world=True)
    for k in KEYS:
        assert pr.same_bits(got[k], ref[k]), k
    R.close()


def test_an_image_of_several_tiles():
    """wider than a tile and more pixels than the staging buffer holds: 2 x 2 tiles, the last column of patches 4 pixels wide"""
    case, R = setup(1)
    lo, hi = ps.root_box(R.prep)
    ext = hi - lo
    size = (4100, 700)
    # over the root box less a margin, one sample each, at mid-depth
    rays = pr.rays((lo[0] + 1, lo[1] + 1, lo[2]), (0, 0, 1), size, 0.0, ext[2], 1,
                   orgDu=((ext[0] - 2) / size[0], 0, 0), orgDv=(0, (ext[1] - 2) / size[1], 0))
    ref, _, status = check(R, rays, what="tiles")
    assert (status >= 0).mean() > 0.3
    assert (ref["count"][:, 4096:] == 1).any() and (ref["count"][680:, :] == 1).any() and (ref["count"][680:, 4096:] == 1).any()


def test_multi_device_handle_equals_single():
    case, R = setup(1)
    rays = pinhole_rays(R.prep, True)
    want = R.project(**rays, normalize=True)
    M = multi_handle(R, 1)
    got = M.project(**rays, normalize=True)
    for k in KEYS:
        assert pr.same_bits(got[k], want[k]), k
    M.close()


def _struct(rays):
    s = binding.ExaHipRays()
    for k in ("org", "orgDu", "orgDv", "dir", "dirDu", "dirDv"):
        setattr(s, k, (C.c_float * 3)(*[float(c) for c in rays[k]]))
    s.width, s.height = rays["size"]
    s.tmin, s.dt, s.numSamples = float(rays["tmin"]), float(rays["dt"]), rays["num_samples"]
    return s


def test_device_pointers_and_null_outputs():
    import torch
    case, R = setup(1)
    L = binding.lib()
    rays = pinhole_rays(R.prep, True)
    want = R.project(**rays, normalize=True)
    s = _struct(rays)
    dev = torch.device("cuda:0")
    dtypes = dict(sum=torch.float64, count=torch.int32, max=torch.float32, min=torch.float32, max_index=torch.int32)
    out = {k: torch.full((H, W), 77, dtype=t, device=dev) for k, t in dtypes.items()}
    ptr = lambda k: C.c_void_p(out[k].data_ptr())                           # noqa: E731
    rc = L.exa_hip_project(R.h, C.byref(s), 0, binding.PROJECT_NORMALIZE, ptr("sum"), ptr("count"), ptr("max"), ptr("min"),
                           ptr("max_index"), 1, None)
    assert rc == 0, L.exa_hip_last_error(R.h).decode()
    torch.cuda.synchronize()
    for k in KEYS:
        assert pr.same_bits(out[k].cpu().numpy().view(want[k].dtype), want[k]), k
    assert R.projectMs() > 0.0
    # NULL outputs are skipped: on the device ...
    out = {k: torch.full((H, W), 77, dtype=t, device=dev) for k, t in dtypes.items()}
    rc = L.exa_hip_project(R.h, C.byref(s), 0, binding.PROJECT_NORMALIZE, None, ptr("count"), None, ptr("min"), None, 1, None)
    assert rc == 0, L.exa_hip_last_error(R.h).decode()
    torch.cuda.synchronize()
    for k in KEYS:
        if k in ("count", "min"):
            assert pr.same_bits(out[k].cpu().numpy().view(want[k].dtype), want[k]), k
        else:
            assert bool((out[k] == 77).all()), k
    # ... and on the host; and all five
    vmax, index = np.full((H, W), 77, f32), np.full((H, W), 77, np.int32)
    rc = L.exa_hip_project(R.h, C.byref(s), 0, binding.PROJECT_NORMALIZE, None, None, vmax.ctypes.data, None, index.ctypes.data, 0, None)
    assert rc == 0 and pr.same_bits(vmax, want["max"]) and pr.same_bits(index, want["max_index"])
    assert L.exa_hip_project(R.h, C.byref(s), 0, binding.PROJECT_NORMALIZE, None, None, None, None, None, 0, None) == 0


def test_bad_arguments_are_refused_and_the_handle_stays_usable():
    case, R = setup(1)
    L = binding.lib()
    rays = pinhole_rays(R.prep, True)
    want = R.project(**rays, normalize=True)
    assert want["count"].sum() > 0
    buf = {k: np.zeros((H, W), want[k].dtype) for k in KEYS}

    def call(s, channel=0, flags=binding.PROJECT_NORMALIZE):
        rc = L.exa_hip_project(R.h, s, channel, flags, *[buf[k].ctypes.data for k in KEYS], 0, None)
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
           ((edited(),), dict(flags=1 << 30), "flag")]
    for args, kw, match in bad:
        rc, msg = call(*args, **kw)
        assert rc != 0 and "exa_hip_project" in msg and match in msg, (match, kw, rc, msg)
        assert R.projectMs() == 0.0
        rc, msg = call(edited())                                # ... and the handle still projects
        assert rc == 0, msg
        for k in KEYS:
            assert pr.same_bits(buf[k], want[k]), (match, k)


def test_world_space_needs_a_frame_state():
    case, R0 = setup(1)
    R = binding.Renderer(R0.prep)                               # no frame state yet
    L = binding.lib()
    s = _struct(pinhole_rays(R.prep, True))
    count = np.zeros((H, W), np.uint32)
    rc = L.exa_hip_project(R.h, C.byref(s), 0, binding.SAMPLE_WORLD_SPACE | binding.PROJECT_NORMALIZE, None, count.ctypes.data, None, None, None, 0, None)
    msg = L.exa_hip_last_error(R.h).decode()
    assert rc != 0 and "exa_hip_project" in msg and "frame state" in msg, msg
    rc = L.exa_hip_project(R.h, C.byref(s), 0, binding.PROJECT_NORMALIZE, None, count.ctypes.data, None, None, None, 0, None)     # voxel space works
    assert rc == 0 and count.sum() > 0
    R.close()


def test_scene_without_kd_tree_is_refused():
    R = binding.Renderer(without_kd_tree(binding.Prep(amr3())))
    with pytest.raises(RuntimeError, match="kd-tree"):
        R.project(**pinhole_rays(R.prep, True), normalize=True)
    R.close()
