"""Contour lines on a plane lattice on the GPU (exa_hip_isolines, include/exa_hip.h): the kept lattice values equal the
points probe at the restated positions, and vertices, uv, segments and both offset arrays equal the numpy restatement of the
contract (tests/isolines_ref.py) applied to those values, byte for byte; gradients equal the points probe at the vertices;
the derived call does the same against sampleDerived; nothing a frame or a tuning knob sets changes a byte; the iso-surface's
mesh and the lines do not drop each other; bad arguments are refused with a message and leave the handle usable."""
import ctypes as C
import math

import numpy as np
import pytest

import isolines_ref as ref
import probe_sets as ps
from analysis_steps import bits as _bits, frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes

pytestmark = pytest.mark.gpu

NAN = float("nan")
XFM = dict(vx=[1.6, 0.5, -0.2], vy=[-0.4, 1.3, 0.3], vz=[0.25, -0.15, 0.9], p=[3.5, -1.25, 2.0])
# the smallest lattices at which each mechanism can go wrong: a single square; a row of two; odd sizes; a 256-point block
# that ends inside a row; whole waves per row; more than 2048 blocks, so more than one scan chunk
SHAPES = [(2, 2), (3, 2), (17, 5), (257, 3), (64, 9), (1025, 513)]
assert (1025 * 513 + 255) // 256 > 2048

SCENES = {
    "ex3": (lambda: scenes.example("ex3"), False),
    "ex4": (lambda: scenes.example("ex4"), False),
    "amr3": (lambda: scenes.amr(levels=3, fields=3), False),
    "amr3_holes": (lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=3), fraction=0.15), True),
    "amr3_moved": (lambda: ps.translated(scenes.amr(levels=3, fields=3), ps.TRANSLATION["moderate"]), False),
}


def _box(R):
    lo, hi = R.prep.voxel_bounds()
    return np.asarray(lo, np.float64), np.asarray(hi, np.float64)


def _boundary_x(scene, lo, hi):
    """an x inside the volume that is a face of bricks of two levels (a coarse-fine boundary lies on it), else any brick face"""
    b = np.asarray(scene.bricks7, dtype=np.int64).reshape(-1, 7)
    faces = {}
    for sx, x, level in zip(b[:, 0], b[:, 3], b[:, 6]):
        for f in (x, x + (sx << level)):
            if lo[0] < f < hi[0]:
                faces.setdefault(int(f), set()).add(int(level))
    assert faces, "a scene of one brick along x"
    mixed = sorted(f for f, levels in faces.items() if len(levels) > 1)
    return float(mixed[len(mixed) // 2]) if mixed else float(sorted(faces)[len(faces) // 2])


def _planes(scene, lo, hi, size):
    """name -> (origin, du, dv) of a voxel-space plane lattice of `size` points over the volume lo .. hi"""
    nu, nv = size
    ext = hi - lo
    z = math.floor(lo[2] + 0.5 * ext[2]) + 0.5                    # a plane of finest-level cell centres
    return {
        "centres": ((lo[0], lo[1], z), (ext[0] / nu, 0, 0), (0, ext[1] / nv, 0)),
        "boundary": ((_boundary_x(scene, lo, hi), lo[1], lo[2]), (0, ext[1] / nu, 0), (0, 0, ext[2] / nv)),
        "oblique": (lo + ext * (0.05, 0.02, 0.01), ext * (0.9, 0.55, 0.08) / nu, ext * (-0.04, 0.4, 0.9) / nv),
        # leaves the volume on both sides of u: columns of NaN, so invalid squares
        "leaving": ((lo[0] - 0.3 * ext[0], lo[1], z - 0.25), (1.6 * ext[0] / nu, 0, 0), (0, ext[1] / nv, 0.3 / nv)),
    }


def _levels(V):
    """from the kept lattice values: three quartiles of the distinct finite values in descending order with the middle one
    repeated, one lattice value exactly (a vertex with t == 0), and a level above every value (an empty level)"""
    fin = np.unique(V[np.isfinite(V)])
    if fin.size > 1:
        fin = fin[1:]                                              # a background at the minimum holds no line
    q = [fin[(k * (fin.size - 1)) // 4] for k in (3, 2, 1)]
    mid = np.float32(0.5 * (float(q[1]) + float(fin[min(fin.size - 1, (fin.size - 1) // 2 + 1)])))     # between two lattice values
    exact = fin[(2 * fin.size) // 5]
    return np.array([q[0], mid, q[2], mid, exact, np.float32(float(fin[-1]) + 1.0)], np.float32)


def _check(R, plane, size, isos, channel, world, what, derived=None):
    """one extraction against the probes and the restatement; returns (result, restatement)"""
    nu, nv = size
    if derived is None:
        got = R.isolines(*plane, size, isos, channel=channel, world=world, gradients=True, values=True)
    else:
        got = R.isolinesDerived(*plane, size, isos, derived, world=world, values=True)
    P = ref.positions(*plane, nu, nv).reshape(-1, 3)
    if derived is None:
        want_v = R.samplePoints(P, channels=(channel,), world=world, fill=NAN)[0][:, 0]
    else:
        want_v = R.sampleDerived(P, derived, world=world, fill=NAN)[0]
    V = got["values"]
    assert V.shape == (nv, nu) and V.dtype == np.float32, what
    assert np.array_equal(_bits(V).reshape(-1), _bits(want_v).reshape(-1)), what
    want = ref.extract(V, *plane, isos)
    for k in ref.ABI_KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, np.nonzero(got[k].reshape(-1) != want[k].reshape(-1))[0][:10])
    if derived is None:
        _, g, _ = R.samplePoints(got["vertices"], channels=(channel,), gradient=True, normalized=True, world=world, fill=NAN)
        assert got["gradients"].shape == got["vertices"].shape and np.array_equal(_bits(got["gradients"]), _bits(g[:, 0])), what
    return got, want


def _values(R, plane, size, channel=0, world=False, derived=None):
    """the lattice values alone: an extraction at a level nothing reaches, with the values kept"""
    if derived is None:
        return R.isolines(*plane, size, [np.float32(3e38)], channel=channel, world=world, values=True)["values"]
    return R.isolinesDerived(*plane, size, [np.float32(3e38)], derived, world=world, values=True)["values"]


@pytest.mark.parametrize("name", sorted(SCENES))
def test_lines_equal_the_restatement_byte_for_byte(name):
    make, empty = SCENES[name]
    case = Case(make(), allow_empty_cells=empty)
    R = case.hip_renderer()
    lo, hi = _box(R)
    channel = len(case.scene.fields) - 1
    # every shape on the oblique plane, every plane at two shapes
    combos = [("oblique", s) for s in SHAPES] + [(p, s) for p in ("centres", "boundary", "leaving") for s in ((17, 5), (64, 9))]
    segments = 0
    for pname, size in combos:
        plane = _planes(case.scene, lo, hi, size)[pname]
        what = f"{name} {pname} {size[0]}x{size[1]}"
        V = _values(R, plane, size, channel)
        assert np.isfinite(V).any(), what
        valid = ref.valid_squares(V)
        if pname == "leaving":
            assert 0 < valid.sum() < valid.size, what                 # squares that must stay silent
        isos = _levels(V)
        assert (V == isos[4]).any(), what                             # a level equal to a lattice value
        got, want = _check(R, plane, size, isos, channel, False, what)
        assert got["vertex_offsets"][-1] == got["vertex_offsets"][-2], what          # the level above every value: empty
        print(f"{what}: vertices {len(got['vertices'])} segments {len(got['segments'])} valid squares {int(valid.sum())}/{valid.size}")
        if size[0] >= 64:
            assert len(got["segments"]) > 0, what
            segments += len(got["segments"])
            one, _ = _check(R, plane, size, isos[1:2], channel, False, what + " one level")
            n0, n1 = (int(x) for x in got["vertex_offsets"][1:3])
            assert one["vertices"].tobytes() == got["vertices"][n0:n1].tobytes(), what       # the levels are independent
            nothing = R.isolines(*plane, size, isos[5:], channel=channel, gradients=True)
            assert nothing["vertices"].shape == (0, 3) and nothing["segments"].shape == (0, 2) and nothing["gradients"].shape == (0, 3), what
            assert np.array_equal(nothing["vertex_offsets"], [0, 0]) and np.array_equal(nothing["segment_offsets"], [0, 0]), what
    assert segments > 1000, (name, segments)
    R.close()


def test_lines_in_world_space_equal_the_restatement():
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    size = (67, 41)
    plane = ((-4.0, -6.0, 9.5), (34.0 / size[0], 0.1, 0.02), (0.05, 30.0 / size[1], 0.3))      # in the world box of the iso-mesh test
    V = _values(R, plane, size, 1, world=True)
    assert np.isfinite(V).sum() > 100
    got, _ = _check(R, plane, size, _levels(V), 1, True, "amr3 world")
    assert len(got["segments"]) > 0
    # positions stay in the caller's space: on the world plane, and different from the voxel-space extraction
    uv = got["uv"].astype(np.float64)
    on_plane = np.asarray(plane[0]) + uv[:, :1] * np.asarray(plane[1]) + uv[:, 1:] * np.asarray(plane[2])
    assert np.allclose(got["vertices"], on_plane, atol=1e-3)
    V2 = _values(R, plane, size, 1, world=False)
    assert not np.array_equal(_bits(V2), _bits(V))
    R.close()


@pytest.mark.parametrize("quantity", ["q", "vorticity_magnitude"])
def test_derived_lines_equal_the_restatement(quantity):
    case = Case(scenes.amr(levels=3, fields=3))
    R = case.hip_renderer()
    lo, hi = _box(R)
    for size in ((64, 9), (257, 3)):
        plane = _planes(case.scene, lo, hi, size)["oblique"]
        V = _values(R, plane, size, derived=quantity)
        got, _ = _check(R, plane, size, _levels(V), None, False, f"{quantity} {size}", derived=quantity)
        assert len(got["segments"]) > 0 and "gradients" not in got
    R.close()


def _same(got, want, what):
    assert sorted(got) == sorted(want), what
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def test_lines_do_not_depend_on_frame_state_or_options():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    lo, hi = _box(R)
    size = (64, 9)
    plane = _planes(case.scene, lo, hi, size)["oblique"]
    isos = _levels(_values(R, plane, size, 1))
    call = lambda H: H.isolines(*plane, size, isos, channel=1, gradients=True, values=True)        # noqa: E731
    want = call(R)
    assert len(want["segments"]) > 20
    _same(call(R), want, "two consecutive calls")
    for what in frame_perturbations(case, R):
        _same(call(R), want, what)
    for patch in range(4):
        R.setOption("sample_patch", patch)
        _same(call(R), want, f"sample_patch {patch}")
    R.setOption("sample_uniform", 0)
    _same(call(R), want, "sample_uniform 0")
    M = multi_handle(R)
    _same(call(M), want, "a multi-device handle")
    M.close()
    R.close()


def test_lines_and_iso_surface_do_not_drop_each_other():
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    lo, hi = _box(R)
    size = (64, 9)
    plane = _planes(case.scene, lo, hi, size)["oblique"]
    isos = _levels(_values(R, plane, size, 1))
    want_lines = R.isolines(*plane, size, isos, channel=1)
    want_mesh = R.isosurface(lo, hi, (19, 17, 13), float(isos[1]), channel=1)
    assert len(want_mesh[1]) > 0 and len(want_lines["segments"]) > 0
    R.extractIsoSurface(lo, hi, (19, 17, 13), float(isos[1]), channel=1)
    R.extractIsolines(*plane, size, isos, channel=1)
    mesh = R.readIsoSurface()                                        # extracted before the lines: still there
    assert mesh[0].tobytes() == want_mesh[0].tobytes() and mesh[1].tobytes() == want_mesh[1].tobytes()
    R.extractIsoSurface(lo, hi, (9, 9, 9), float(isos[1]), channel=1)
    R.releaseIsoSurface()
    _same(R.readIsolines(), want_lines, "the lines behind a later iso-surface and its release")
    R.releaseIsolines()
    with pytest.raises(RuntimeError, match="exa_hip_isolines_read"):
        R.readIsolines()
    # the device read, and the stage times
    import torch
    nv, ns = R.extractIsolines(*plane, size, isos, channel=1, gradients=True, values=True)
    host = R.readIsolines()
    dev = dict(vertices=torch.empty((nv, 3), dtype=torch.float32, device="cuda:0"), uv=torch.empty((nv, 2), dtype=torch.float32, device="cuda:0"),
               gradients=torch.empty((nv, 3), dtype=torch.float32, device="cuda:0"), segments=torch.empty((ns, 2), dtype=torch.int32, device="cuda:0"),
               values=torch.empty(size[::-1], dtype=torch.float32, device="cuda:0"))
    off = [torch.empty(2 * (len(isos) + 1), dtype=torch.int32, device="cuda:0") for _ in range(2)]      # uint64 as pairs of int32
    R._check(binding.lib().exa_hip_isolines_read(R.h, *(binding._dev_ptr(dev[k]) for k in ("vertices", "uv", "gradients", "segments")),
                                                 binding._dev_ptr(off[0]), binding._dev_ptr(off[1]), binding._dev_ptr(dev["values"]), 1, None))
    for k, x in dev.items():
        assert x.cpu().numpy().tobytes() == host[k].tobytes(), k
    assert off[0].cpu().numpy().tobytes() == host["vertex_offsets"].tobytes()
    assert off[1].cpu().numpy().tobytes() == host["segment_offsets"].tobytes()
    ms = R.isolinesStageMs()
    assert len(ms) == 6 and all(m >= 0 for m in ms) and ms[0] > 0 and ms[4] > 0
    R.close()


def _raw(R, fn="exa_hip_isolines", origin=(0, 0, 4.5), du=(0.5, 0, 0), dv=(0, 0.5, 0), nu=16, nv=16, channel=0, isos=(0.5,), flags=0,
         plane=True, num=None, quantity=None):
    p = binding.ExaHipPlane((C.c_float * 3)(*origin), (C.c_float * 3)(*du), (C.c_float * 3)(*dv), nu, nv)
    levels = (C.c_float * max(len(isos), 1))(*isos) if isos is not None else None
    num = (len(isos) if isos is not None else 1) if num is None else num
    nvert, nseg = C.c_uint64(77), C.c_uint64(77)
    L = binding.lib()
    if quantity is None:
        rc = L.exa_hip_isolines(R.h, C.byref(p) if plane else None, channel, levels, num, flags, C.byref(nvert), C.byref(nseg), None)
    else:
        ch = (C.c_int32 * 3)(*channel)
        rc = L.exa_hip_isolines_derived(R.h, C.byref(p) if plane else None, ch, quantity, levels, num, flags, C.byref(nvert), C.byref(nseg), None)
    return rc, int(nvert.value), int(nseg.value), L.exa_hip_last_error(R.h).decode()


def test_refused_arguments_leave_the_handle_usable():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()                                    # no render yet: the module holds no frame state
    L = binding.lib()
    buf = np.zeros(64, np.float32)
    assert L.exa_hip_isolines_read(R.h, buf.ctypes.data, None, None, None, None, None, None, 0, None) != 0       # before any extraction
    assert L.exa_hip_last_error(R.h).decode().startswith("exa_hip_isolines_read: ")
    rc, nv, ns, msg = _raw(R, flags=binding.SAMPLE_WORLD_SPACE)
    assert rc != 0 and msg.startswith("exa_hip_isolines: ") and "frame state" in msg, msg
    frame = R.render()
    level = float(_levels(_values(R, ((0, 0, 4.5), (0.5, 0, 0), (0, 0.5, 0)), (16, 16)))[1])       # _raw's plane: a level that crosses it
    rc, nv, ns, _ = _raw(R, isos=(level,))
    assert rc == 0 and nv > 0 and ns > 0
    nf = len(case.scene.fields)
    bad = [dict(plane=False), dict(isos=None), dict(origin=(math.nan, 0, 0)), dict(du=(math.inf, 0, 0)), dict(dv=(0, -math.inf, 0)),
           dict(isos=(0.5, math.nan)), dict(isos=(math.inf,)), dict(nu=1), dict(nv=1), dict(nu=0), dict(nv=-5), dict(nu=65536, nv=65536),
           dict(num=0), dict(num=-1), dict(isos=(0.5,) * 257), dict(channel=nf), dict(channel=-1), dict(flags=4), dict(flags=8),
           dict(flags=32), dict(flags=1 << 30)]
    for kw in bad:
        rc, nv, ns, msg = _raw(R, **kw)
        assert rc != 0 and (nv, ns) == (0, 0) and msg.startswith("exa_hip_isolines: "), (kw, rc, msg)
        # a failed extraction drops the result
        assert L.exa_hip_isolines_read(R.h, buf.ctypes.data, None, None, None, None, None, None, 0, None) != 0, kw
    assert R.render().shape == frame.shape                     # the handle still renders
    bad = [dict(quantity=-1), dict(quantity=binding.DERIVED["vorticity"]), dict(quantity=99), dict(flags=binding.SAMPLE_GRADIENT),
           dict(flags=4), dict(channel=(0, 1, nf)), dict(plane=False), dict(isos=(math.nan,)), dict(nu=1)]
    for kw in bad:
        kw = dict(dict(quantity=binding.DERIVED["q"], channel=(0, 1, 2)), **kw)
        rc, nv, ns, msg = _raw(R, **kw)
        assert rc != 0 and (nv, ns) == (0, 0) and msg.startswith("exa_hip_isolines_derived: "), (kw, rc, msg)
    # the next valid calls succeed
    rc, nv, ns, _ = _raw(R, isos=(level, level), flags=binding.SAMPLE_WORLD_SPACE | binding.SAMPLE_GRADIENT)
    assert rc == 0 and nv % 2 == 0 and ns % 2 == 0
    # arrays the extraction did not keep
    vals, g = np.zeros(256, np.float32), np.zeros((nv, 3), np.float32)
    assert L.exa_hip_isolines_read(R.h, None, None, None, None, None, None, vals.ctypes.data, 0, None) != 0
    assert "EXA_ISOLINES_KEEP_VALUES" in L.exa_hip_last_error(R.h).decode()
    assert L.exa_hip_isolines_read(R.h, None, None, g.ctypes.data, None, None, None, None, 0, None) == 0
    rc, nv, ns, _ = _raw(R, quantity=binding.DERIVED["q"], channel=(0, 1, 2), isos=(0.0,), flags=binding.ISOLINES_KEEP_VALUES)
    assert rc == 0
    assert L.exa_hip_isolines_read(R.h, None, None, g.ctypes.data, None, None, None, None, 0, None) != 0
    assert "EXA_SAMPLE_GRADIENT" in L.exa_hip_last_error(R.h).decode()
    assert L.exa_hip_isolines_read(R.h, None, None, None, None, None, None, vals.ctypes.data, 0, None) == 0
    assert R.render().shape == frame.shape
    R.close()


def test_scene_without_kd_tree_is_refused():
    R = without_kd_tree(Case(scenes.amr(levels=3), W=32, H=32)).hip_renderer()
    rc, nv, ns, msg = _raw(R)
    assert rc != 0 and (nv, ns) == (0, 0) and msg.startswith("exa_hip_isolines: ") and "kd-tree" in msg, msg
    assert R.render().shape == (32, 32)                        # the handle still renders (through its LBVH)
    R.close()
