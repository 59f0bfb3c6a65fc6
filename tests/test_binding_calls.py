"""What owlexabrick_amd/binding.py sends through the C ABI, held against a recording (tests/golden/binding_calls.json) made
from the binding before its analysis half was folded.  A stub stands in for libexa_hip.so, so neither the module nor a GPU
is needed: every exa_hip_* call is logged with its arguments normalised by the argtypes of binding._ABI, the stub writes
fixed counts into the out-parameters so that the read methods allocate something, and every return value is summarised.

Left out: the torch CUDA tensor branches of samplePoints, sampleDerived and sampleTriangles cannot run without a device;
they stay with tests/test_gpu_sample.py, tests/test_gpu_derived.py and tests/test_gpu_surface.py.  A CPU tensor that
answers is_cuda = True gets as far here as a CPU can: the TypeError texts of all three, and the call of sampleTriangles
(whose outputs, unlike those of the other two, do not pass through _dev_ptr, which refuses a tensor not on a device).

`python tests/test_binding_calls.py FILE` writes a recording of the current binding to FILE."""
import ctypes as C
import hashlib
import inspect
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from owlexabrick_amd import binding as B  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "binding_calls.json")
# what the stub writes by reference: the handle, and per out-parameter a small number that differs with the slot
HANDLE, COUNT, VALUE = 0x1000, 2, 20
# the underscore names other files use
KEPT = ("__init__", "_check", "_ms", "_push_state", "_dev_ptr", "_f3", "_i3")
# Renderer's frame side, which the recording leaves alone; every other public method must appear in the case list
FRAME_METHODS = {"close", "setVoxelSpaceTransform", "resizeFrameBuffer", "updateIsoValues", "resetTracer", "setTracerEnabled",
                 "advanceTracer", "readTraces", "setTriangles", "updateContourPlanes", "updateCamera", "updateXF",
                 "updateFrameID", "updateDt", "setSpaceSkipping", "setGradientShadingDVR", "setGradientShadingISO", "setShard",
                 "setOption", "outputPixels", "render", "renderStats", "stats", "readAccum", "writeAccum", "readActivity",
                 "untile"}


def _mask_pointers(ctype, at, buf):
    """replace every c_void_p inside a struct or array by 0 / 1: an address is no part of a recording"""
    if issubclass(ctype, C.Structure):
        for name, ft in ctype._fields_:
            _mask_pointers(ft, at + getattr(ctype, name).offset, buf)
    elif issubclass(ctype, C.Array):
        if issubclass(ctype._type_, (C.Structure, C.Array, C.c_void_p)):
            for i in range(ctype._length_):
                _mask_pointers(ctype._type_, at + i * C.sizeof(ctype._type_), buf)
    elif ctype is C.c_void_p:
        buf[at:at + 8] = int(any(buf[at:at + 8])).to_bytes(8, "little")


def _bytes(obj):
    buf = bytearray(bytes(obj))
    _mask_pointers(type(obj), 0, buf)
    return buf.hex()


def _arg(a, t):
    pointer_slot = t is C.c_void_p or issubclass(t, C._Pointer)
    if hasattr(a, "_obj"):                                      # byref(...)
        assert pointer_slot and (t is C.c_void_p or type(a._obj) is t._type_), (a._obj, t)
        return [type(a._obj).__name__, _bytes(a._obj)]
    if isinstance(a, (C.Structure, C.Array)):
        assert pointer_slot, (a, t)
        return _bytes(a)
    if t is C.c_float:
        return "f" + bytes(C.c_float(a)).hex()
    if t is C.c_char_p:
        return a.decode()
    if not pointer_slot:
        assert type(a) is int, (a, t)
        return a
    if isinstance(a, C.c_void_p):
        a = a.value
    assert a is None or type(a) is int, (a, t)
    return "ptr" if a else "null"


class Stub:
    """stands in for the loaded library: every symbol of _ABI logs its call and returns 0 (b"" for the last_error getters),
    or 1 for the one function named in `fail`, which then writes nothing"""

    def __init__(self):
        self.log, self.fail = [], None

    def __getattr__(self, name):
        if name not in B._ABI:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        restype, argtypes = B._ABI[name]
        assert len(args) == len(argtypes or []), (name, len(args))
        self.log.append([name] + [_arg(a, t) for a, t in zip(args, argtypes or [])])
        if restype is C.c_char_p:
            return b""
        if name == self.fail:
            return 1
        for i, a in enumerate(args):
            out = getattr(a, "_obj", None)
            if isinstance(out, C.c_uint64):
                out.value = COUNT + i
            elif isinstance(out, C.c_int32):
                out.value = VALUE + i
            elif isinstance(out, C.c_void_p):
                out.value = HANDLE
        return 0


class _Prep:
    """as much of binding.Prep as Renderer.__init__ reads"""
    num_fields = 3

    def __init__(self):
        self.scene = B.ExaHipScene()

    def voxel_bounds(self):
        return np.zeros(3, np.float32), np.ones(3, np.float32)


class _OnDevice:
    """a CPU torch tensor that says it lives on a device (see the top of the file)"""
    is_cuda = True

    def __init__(self, tensor):
        self._tensor = tensor

    def __getattr__(self, name):
        return getattr(self._tensor, name)


def _summary(v, zeros=()):
    """type, shape and dtype of an array, the value of a scalar, recursively through tuples, lists and dicts; under the keys
    or indices of `zeros`, where the binding hands out zero-filled arrays, the content too"""
    if isinstance(v, np.ndarray):
        return ["ndarray", list(v.shape), str(v.dtype)]
    if type(v).__name__ == "Tensor":
        return ["Tensor", list(v.shape), str(v.dtype), v.device.type]
    if isinstance(v, (tuple, list, dict)):
        items = list(v.items()) if isinstance(v, dict) else list(enumerate(v))
        out, seen = [], {}
        for k, x in items:
            if isinstance(x, np.ndarray) and id(x) in seen:
                s = ["same array as", seen[id(x)]]
            else:
                s = _summary(x)
                if k in zeros and x is not None:
                    s.append(hashlib.sha256(x.tobytes()).hexdigest())
            seen[id(x)] = k
            out.append([k, s])
        return [type(v).__name__, out]
    if isinstance(v, np.generic):
        return [type(v).__name__, repr(v.item())]
    return [type(v).__name__, repr(v)]


def _unordered(summary):
    """the summary with the entries of every dict sorted by key: the order of a result's keys is not held"""
    if isinstance(summary, list) and len(summary) == 2 and summary[0] in ("dict", "tuple", "list"):
        entries = [[k, _unordered(s)] for k, s in summary[1]]
        return [summary[0], sorted(entries) if summary[0] == "dict" else entries]
    return summary


def c(method, *args, zeros=(), **kw):
    return method, args, kw, zeros


def fail(name):
    """from here on the stub's function `name` returns 1 (None: none does)"""
    return "!fail", name


def _cases():
    """[(group, [case, ...])]: every group runs on a renderer of its own"""
    import torch
    lo, hi, dims, bad_dims = (0.0, 0.5, 1.0), (8.0, 6.0, 4.0), (4, 3, 2), (4, -3, 2)
    pts = np.arange(15, dtype=np.float32).reshape(5, 3)
    verts = np.arange(12, dtype=np.float64).reshape(4, 3)
    tris = [[0, 1, 2], [1, 2, 3], [0, 2, 3]]
    plane = ((0.0, 0.0, 1.0), (1.0, 0.0, 0.0), (0.0, 0.5, 0.0), (6, 5))
    rays = ((0, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.1, 0, 0), (0, 0.1, 0))
    march = (0.25, 0.5, 7)                                                  # tmin, dt, num_samples
    huge = (65536, 32768)                                                   # 2^31 pixels: one more than the module takes
    seeds = pts[:3]
    iso_args, line_args = (lo, hi, dims, 0.5), plane + ([0.25, 0.5, 0.75],)
    basin_args = iso_args + (0.125,)
    dev = lambda a: _OnDevice(torch.from_numpy(a))                          # noqa: E731
    groups = [
        ("probes", [
            c("samplePoints", pts),
            c("samplePoints", pts, channels=(0, 2), gradient=True),
            c("samplePoints", pts.tolist(), channels=[1], normalized=True, world=True, fill=0.0, stream=0x30, async_=True),
            c("resample", lo, hi, dims),
            c("resample", lo, hi, bad_dims, channel=1, world=True, fill=-1.0),
            c("resample", lo, hi, dims, out_ptr=0x2000, stream=0x30, async_=True),
            c("resample", lo, hi, dims, out_ptr=np.zeros(24, np.float32)),
            c("sampleDerived", pts, "vorticity"),
            c("sampleDerived", pts, "Q", channels=(2, 1, 0), world=True, fill=0.0, stream=0x30, async_=True),
            c("sampleDerived", pts, 7),
            c("sampleDerived", pts, "nope", world=True),
            c("resampleDerived", lo, hi, dims, "vorticity"),
            c("resampleDerived", lo, hi, bad_dims, "speed", channels=(2, 1, 0), world=True, fill=0.0),
            c("resampleDerived", lo, hi, dims, 2, out_ptr=0x2000, stream=0x30, async_=True),
            c("resampleDerived", lo, hi, dims, "q", out_ptr="0x2000"),
            c("derivedMs"),
        ]),
        ("tensors", [
            c("samplePoints", dev(pts.astype(np.float64))),
            c("samplePoints", dev(pts.reshape(-1)[:14])),
            c("sampleDerived", dev(pts.T), "speed"),
            c("sampleTriangles", dev(verts.astype(np.float32)), dev(np.array(tris, np.int32)), channels=(0, 1), stream=0x30),
            c("sampleTriangles", dev(verts.astype(np.float32)), dev(np.array(tris, np.int64))),
            c("resample", lo, hi, dims, out_ptr=dev(np.zeros(24, np.float32))),
            c("resample", lo, hi, dims, out_ptr=dev(np.zeros(24, np.float64))),
            c("profile", lo, hi, dims, (B.labels(dev(np.zeros(24, np.int32)), 4),), zeros=("count", "sums", "mins", "maxs")),
        ]),
        ("isosurface", [
            c("readIsoSurface"),
            c("sampleTriangles", zeros=B.SURFACE_KEYS),
            c("extractIsoSurface", *iso_args),
            c("readIsoSurface"),
            c("extractIsoSurface", *iso_args, channel=1, world=True, gradients=True, stream=0x30),
            c("readIsoSurface"),
            c("sampleTriangles", zeros=B.SURFACE_KEYS),
            c("sampleTriangles", channels=(0, 1), spacing=0, max_n=8, world=True, stream=0x30, zeros=B.SURFACE_KEYS),
            c("surfaceIntegrals", channels=(0, 1, 2)),
            c("isoSurfaceStageMs"),
            c("releaseIsoSurface"),
            c("readIsoSurface"),
            c("isosurface", *iso_args),
            c("isosurface", *iso_args, channel=2, world=True, gradients=True),
            c("extractIsoSurfaceDerived", *iso_args, "q", world=True, gradients=True, stream=0x30),
            c("readIsoSurface"),
            c("extractIsoSurfaceDerived", *iso_args, "nope"),
            c("isosurfaceDerived", *iso_args, "speed"),
            c("isosurfaceDerived", *iso_args, 3, channels=(2, 1, 0), world=True),
        ]),
        ("isolines", [
            c("readIsolines"),
            c("extractIsolines", *line_args),
            c("readIsolines"),
            c("extractIsolines", *line_args, channel=1, world=True, gradients=True, values=True, stream=0x30),
            c("readIsolines"),
            c("extractIsolines", *line_args, quantity="divergence", channels=(2, 1, 0), values=True),
            c("readIsolines"),
            c("isolinesStageMs"),
            c("releaseIsolines"),
            c("readIsolines"),
            c("isolines", *line_args),
            c("isolines", plane[0], plane[1], plane[2], plane[3], 0.5, channel=2, world=True, gradients=True, values=True),
            c("isolinesDerived", *line_args, "speed"),
            c("isolinesDerived", *line_args, 4, channels=(2, 1, 0), world=True, values=True),
            c("readIsolines"),
        ]),
        ("regions", [
            c("readRegions"),
            c("extractRegions", *iso_args),
            c("readRegions", zeros=("regions",)),
            c("extractRegions", *iso_args, channel=1, world=True, below=True, stream=0x30),
            c("extractRegions", *iso_args, faces=True, keep_values=True),
            c("readRegions", zeros=("regions",)),
            c("extractRegions", *iso_args, quantity="helicity", channels=(2, 1, 0), below=True, faces=True, keep_values=True),
            c("readRegions", zeros=("regions",)),
            c("regionsStageMs"),
            c("releaseRegions"),
            c("readRegions"),
            c("regions", *iso_args, zeros=("regions",)),
            c("regions", *iso_args, channel=2, world=True, below=True, faces=True, keep_values=True, zeros=("regions",)),
            c("regionsDerived", *iso_args, "speed", zeros=("regions",)),
            c("regionsDerived", *iso_args, 1, channels=(2, 1, 0), world=True, below=True, faces=True, keep_values=True,
              zeros=("regions",)),
            c("readRegions"),
        ]),
        ("basins", [
            c("readBasins"),
            c("extractBasins", *basin_args),
            c("readBasins", zeros=("regions",)),
            c("extractBasins", *basin_args, channel=1, world=True, below=True, stream=0x30),
            c("extractBasins", *basin_args, faces=True, keep_values=True),
            c("readBasins", zeros=("regions",)),
            c("extractBasins", *basin_args, quantity="helicity", channels=(2, 1, 0), below=True, faces=True, keep_values=True),
            c("readBasins", zeros=("regions",)),
            c("basinsStageMs"),
            c("releaseBasins"),
            c("readBasins"),
            c("basins", *basin_args, zeros=("regions",)),
            c("basins", *basin_args, channel=2, world=True, below=True, faces=True, keep_values=True, zeros=("regions",)),
            c("basinsDerived", *basin_args, "speed", zeros=("regions",)),
            c("basinsDerived", *basin_args, 1, channels=(2, 1, 0), world=True, below=True, faces=True, keep_values=True,
              zeros=("regions",)),
            c("readBasins"),
        ]),
        ("critical points", [
            c("readCriticalPoints"),
            c("extractCriticalPoints", lo, hi, dims),
            c("readCriticalPoints", zeros=(0,)),
            c("extractCriticalPoints", lo, hi, dims, channels=(2, 1, 0), iterations=5, tolerance=0.25, world=True, probe=True,
              stream=0x30),
            c("readCriticalPoints", zeros=(0,)),
            c("criticalPointsStageMs"),
            c("releaseCriticalPoints"),
            c("readCriticalPoints"),
            c("criticalPoints", lo, hi, dims, zeros=(0,)),
            c("criticalPoints", lo, hi, dims, channels=(2, 1, 0), iterations=5, tolerance=0.25, world=True, probe=True,
              zeros=(0,)),
            c("readCriticalPoints"),
        ]),
        ("streamlines", [
            c("readStreamlines"),
            c("extractStreamlines", seeds),
            c("readStreamlines"),
            c("extractStreamlines", seeds.tolist(), channels=(2, 1, 0), step=0.25, max_steps=9, forward=False, backward=True,
              normalize=True, velocities=True, stream=0x30),
            c("readStreamlines"),
            c("streamlinesMs"),
            c("releaseStreamlines"),
            c("readStreamlines"),
            c("streamlines", seeds),
            c("streamlines", seeds, channels=(2, 1, 0), step=0.25, max_steps=9, backward=True, normalize=True, velocities=True),
            c("readStreamlines"),
        ]),
        ("histogram", [
            c("histogram", 0, 0.0, 1.0, 16),
            c("histogram", 1, -1, 2, B.HIST_MAX_BINS + 5, box=(0, 1, 2, 3, 4, 5), volume=False, stream=0x30),
            c("histogram", 0, 0.0, 1.0, -3),
            c("histogramMs"),
            c("fieldStats", 2),
            c("fieldStats", 1, box=(0, 1, 2, 3, 4, 5)),
        ]),
        ("profile", [
            c("profile", lo, hi, dims, B.uniform(B.channel(0), 0.0, 1.0, 6), zeros=("count", "sum_weight", "sums", "mins", "maxs")),
            c("profile", lo, hi, dims, [B.uniform(B.radius((1, 2, 3)), 0.0, 9.0, 6)], values=[B.channel(1)], minmax=False,
              zeros=("count", "sums")),
            c("profile", lo, hi, dims, (B.edges(B.coordinate(2), [0, 1, 2, 4, 8]), B.uniform(B.derived("q", (2, 1, 0)), -1.0, 1.0, 3)),
              values=(B.channel(0), B.derived("speed"), B.radius((1, 2, 3)), B.coordinate(1)), weight=B.channel(2), world=True,
              stream=0x30, zeros=("count", "sum_weight", "sums", "mins", "maxs")),
            c("profile", lo, hi, dims, (B.labels(np.arange(24, dtype=np.int32) % 5 - 1, 4),), values=(B.channel(0),),
              zeros=("count", "sums", "mins", "maxs")),
            c("profile", lo, hi, dims, (B.labels(0x2000, 4), B.uniform(B.channel(1), 0.0, 1.0, 2)), weight=B.coordinate(0),
              zeros=("count", "sum_weight", "sums", "mins", "maxs")),
            c("profile", lo, hi, dims, (B.uniform(B.channel(0), 0.0, 1.0, B.PROFILE_MAX_BINS), B.uniform(B.channel(1), 0.0, 1.0, 2)),
              values=(B.channel(0),)),
            c("profile", lo, hi, dims, (B.uniform(B.channel(0), 0.0, 1.0, -2),)),
            c("profile", lo, hi, dims, ()),
            c("profileStageMs"),
        ]),
        ("images", [
            c("lic", plane),
            c("lic", plane, channels=(2, 1, 0), step=0.25, half_length=9, noise=np.arange(30) % 7, seed=-1, fill=0.0, stream=0x30),
            c("lic", plane, noise=np.zeros(29, np.uint8)),
            c("lic", plane[:3] + ((-6, 5),)),
            c("licMs"),
            c("flowmap", lo, hi, dims),
            c("flowmap", lo, hi, bad_dims, channels=(2, 1, 0), step=0.25, num_steps=9, backward=True, fill=0.0, stream=0x30),
            c("flowmapMs"),
            c("project", *rays, (6, 5), *march),
            c("project", *rays, (6, -5), *march, channel=1, world=True, normalize=True, stream=0x30),
            c("project", *rays, huge, *march),
            c("projectMs"),
            c("raycast_iso", *rays, (6, 5), *march, 0.5),
            c("raycast_iso", *rays, (6, 5), *march, 0.5, refine=3, channel=1, world=True, normalize=True, fill=0.0,
              outputs=("position", "t", "crossings"), stream=0x30),
            c("raycast_iso", *rays, (6, 5), *march, 0.5, outputs=("t", "depth"), world=True),
            c("raycast_iso", *rays, (6, 5), *march, 0.5, outputs=()),
            c("raycast_iso", *rays, huge, *march, 0.5, outputs=["gradient"]),
            c("raycastIsoMs"),
        ]),
        ("surface", [
            c("sampleTriangles", verts, tris, zeros=B.SURFACE_KEYS),
            c("sampleTriangles", verts, tris, channels=(0, 1, 2, 0, 1), spacing=0.5, max_n=4, world=True, stream=0x30,
              zeros=B.SURFACE_KEYS),
            c("sampleTrianglesMs"),
            c("surfaceIntegrals", verts, tris, channels=(0, 1, 2), spacing=0.5, max_n=4, world=True),
            c("surfaceIntegrals", verts, tris),
        ]),
    ]
    # one function fails: what is raised, what a one-shot still sends, and what the next read of the family then sends
    families = [
        ("IsoSurface", "isosurface", ("exa_hip_isosurface", c("extractIsoSurface", *iso_args, gradients=True)),
         ("exa_hip_isosurface_derived", c("extractIsoSurfaceDerived", *iso_args, "q")), c("isosurface", *iso_args)),
        ("Isolines", "isolines", ("exa_hip_isolines", c("extractIsolines", *line_args, values=True)),
         ("exa_hip_isolines_derived", c("extractIsolines", *line_args, quantity="q")), c("isolines", *line_args)),
        ("Regions", "regions", ("exa_hip_regions", c("extractRegions", *iso_args, keep_values=True)),
         ("exa_hip_regions_derived", c("extractRegions", *iso_args, quantity="q")), c("regions", *iso_args)),
        ("Basins", "basins", ("exa_hip_basins", c("extractBasins", *basin_args, keep_values=True)),
         ("exa_hip_basins_derived", c("extractBasins", *basin_args, quantity="q")), c("basins", *basin_args)),
        ("CriticalPoints", "critical_points", ("exa_hip_critical_points", c("extractCriticalPoints", lo, hi, dims, probe=True)),
         None, c("criticalPoints", lo, hi, dims, probe=True)),
        ("Streamlines", "streamlines", ("exa_hip_streamlines", c("extractStreamlines", seeds, velocities=True)),
         None, c("streamlines", seeds)),
    ]
    for family, symbol, plain, from_derived, one_shot in families:
        for name, extract in filter(None, (plain, from_derived)):
            groups.append((f"{name} fails", [plain[1], fail(name), extract, c("read" + family), one_shot, fail(None),
                                              c("read" + family)]))
        groups.append((f"exa_hip_{symbol}_read fails", [plain[1], fail(f"exa_hip_{symbol}_read"), c("read" + family), one_shot,
                                                         fail(None), c("read" + family)]))
    return groups


def record():
    """the case list run against the current binding: one entry per call of a Renderer method"""
    records, stub, saved = [], Stub(), B._lib
    B._lib = stub
    try:
        for group, cases in _cases():
            R = B.Renderer(_Prep())
            stub.log = []
            try:
                for i, case in enumerate(cases):
                    if case[0] == "!fail":
                        stub.fail = case[1]
                        continue
                    method, args, kw, zeros = case
                    rec = {"case": f"{group} [{i}] {method}({', '.join(kw)})"}
                    try:
                        rec["result"] = _summary(getattr(R, method)(*args, **kw), zeros)
                    except Exception as e:  # noqa: BLE001
                        rec["error"] = [type(e).__name__, str(e)]
                    rec["sent"], stub.log = stub.log, []
                    records.append(rec)
            finally:
                stub.fail = None
                R.close()                                       # while the stub is in place: close() calls lib()
    finally:
        B._lib = saved
    return records


def api():
    """signature and docstring hash of every public callable of the module, of Renderer and of Prep, and of KEPT"""
    out = {}
    for owner, names in (("", vars(B)), ("Renderer.", vars(B.Renderer)), ("Prep.", vars(B.Prep))):
        for name, f in names.items():
            if callable(f) and (not name.startswith("_") or name in KEPT) and getattr(f, "__module__", None) == B.__name__:
                try:
                    sig = str(inspect.signature(f))
                except (TypeError, ValueError):                 # a ctypes structure
                    sig = None
                out[owner + name] = [sig, hashlib.sha256((inspect.getdoc(f) or "").encode()).hexdigest()]
    return out


def whole_recording():
    return json.loads(json.dumps({"api": api(), "names": sorted(n for n in vars(B) if not n.startswith("__")), "calls": record()}))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    saved = B._lib
    try:
        return whole_recording()
    finally:
        assert B._lib is saved                                  # no other test sees the stub


def test_case_list_reaches_every_analysis_method():
    wanted = {n for n, f in vars(B.Renderer).items() if callable(f) and not n.startswith("_")} - FRAME_METHODS
    reached = {case[0] for _, cases in _cases() for case in cases}
    assert wanted <= reached, sorted(wanted - reached)


def test_calls_match_the_recording(golden, current):
    assert [r["case"] for r in current["calls"]] == [r["case"] for r in golden["calls"]]
    for got, want in zip(current["calls"], golden["calls"]):
        assert got.get("error") == want.get("error"), got["case"]
        assert len(got["sent"]) == len(want["sent"]) and [s[0] for s in got["sent"]] == [s[0] for s in want["sent"]], got["case"]
        for sent, recorded in zip(got["sent"], want["sent"]):
            assert sent == recorded, (got["case"], sent[0])
        assert _unordered(got.get("result")) == _unordered(want.get("result")), got["case"]


def test_signatures_and_docstrings_match_the_recording(golden, current):
    assert not set(golden["names"]) - set(current["names"])
    for name, want in golden["api"].items():
        assert current["api"].get(name) == want, name
    assert set(current["api"]) == set(golden["api"])


if __name__ == "__main__":
    rec = whole_recording()
    with open(sys.argv[1], "w") as f:
        f.write('{"api": {\n' + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in rec["api"].items()) + "},\n")
        f.write('"names": ' + json.dumps(rec["names"]) + ",\n")
        f.write('"calls": [\n' + ",\n".join(" " + json.dumps(r) for r in rec["calls"]) + "]}\n")
