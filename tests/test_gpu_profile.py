"""Profiles and phase plots on the GPU (exa_hip_profile, include/exa_hip.h): count, sumWeight, sums, mins, maxs and every
field of the stats but ldsTable equal the numpy restatement of the contract (tests/profile_ref.py) byte for byte when that is
fed the lattices exa_hip_resample[_derived] return — on four scenes, on lattice shapes that trip indexing mistakes, with
uniform, edges and label axes from 1 to 2^20 bins on both sides of the LDS / HBM choice, on the shapes that put a whole wave
into one bin or every lane into its own, with every kind of source as key, value and weight; the labels of exa_hip_regions
and exa_hip_basins as the axis give those calls' own tables; nothing a frame or a tuning knob sets changes a byte; bad
arguments are refused with a message and leave the handle usable.  The failed allocation has no test."""
import ctypes as C
import math

import numpy as np
import pytest

import profile_ref as ref
from analysis_steps import frame_perturbations, multi_handle, without_kd_tree
from common import Case
from owlexabrick_amd import binding, scenes
from owlexabrick_amd.binding import channel, coordinate, derived, radius
from test_gpu_isomesh import XFM, _root_box

pytestmark = pytest.mark.gpu

NAN = float("nan")
LATTICES = [(1, 1, 1), (67, 1, 1), (257, 1, 1), (9, 8, 7), (17, 16, 16)]        # the last: 17 tiles, beyond one launch block of 16


# ---- a source is a tuple: ("c", channel) | ("d", quantity, channels) | ("r", centre) | ("x", axis); an axis is
# ("uniform", source, lo, hi, n) | ("edges", source, array) | ("labels", array, n) | ("labels_device", array, n) ----
def _bind_source(s):
    return {"c": lambda: channel(s[1]), "d": lambda: derived(s[1], s[2]), "r": lambda: radius(s[1]), "x": lambda: coordinate(s[1])}[s[0]]()


def _bind_axis(a, keep):
    if a[0] == "uniform":
        return binding.uniform(_bind_source(a[1]), a[2], a[3], a[4])
    if a[0] == "edges":
        return binding.edges(_bind_source(a[1]), a[2])
    if a[0] == "labels":
        return binding.labels(np.ascontiguousarray(a[1], np.int32), a[2])
    import torch
    keep.append(torch.from_numpy(np.ascontiguousarray(a[1], np.int32).reshape(-1)).to("cuda:0"))
    return binding.labels(keep[-1], a[2])


class Lattice:
    """a renderer's lattice: the restatement's inputs, every resampled source once"""

    def __init__(self, R, lo, hi, dims, world=False):
        self.R, self.lo, self.hi, self.dims, self.world, self.cache = R, lo, hi, dims, world, {}

    def source(self, s):
        key = repr(s)
        if key not in self.cache:
            if s[0] == "c":
                v = self.R.resample(self.lo, self.hi, self.dims, channel=s[1], world=self.world, fill=NAN)
            elif s[0] == "d":
                v = self.R.resampleDerived(self.lo, self.hi, self.dims, s[1], channels=s[2], world=self.world, fill=NAN)
            elif s[0] == "r":
                v = ref.radius(self.lo, self.hi, self.dims, s[1])
            else:
                v = ref.coordinate(self.lo, self.hi, self.dims, s[1])
            self.cache[key] = np.ascontiguousarray(v, np.float32).reshape(-1)
        return self.cache[key]

    def axis(self, a):
        if a[0] == "uniform":
            return ref.uniform(self.source(a[1]), a[2], a[3], a[4])
        if a[0] == "edges":
            return ref.edges(self.source(a[1]), a[2])
        return ref.labels(a[1], a[2])

    def want(self, axes, values=(), weight=None, minmax=True):
        return ref.profile([self.axis(a) for a in axes], [self.source(v) for v in values],
                           None if weight is None else self.source(weight), minmax=minmax)

    def got(self, axes, values=(), weight=None, minmax=True, R=None):
        keep = []
        return (R or self.R).profile(self.lo, self.hi, self.dims, [_bind_axis(a, keep) for a in axes], [_bind_source(v) for v in values],
                                     None if weight is None else _bind_source(weight), world=self.world, minmax=minmax)

    def check(self, axes, values=(), weight=None, minmax=True, what="", binned=True):
        got, want = self.got(axes, values, weight, minmax), self.want(axes, values, weight, minmax)
        _same(got, want, what)
        assert (got["stats"]["binned"] > 0) == binned, (what, got["stats"])
        return got


def _same(got, want, what):
    stats = {k: v for k, v in got["stats"].items() if k != "ldsTable"}
    print(what, got["stats"])
    assert stats == want["stats"], (what, stats, want["stats"])
    for k in ("count", "sum_weight", "sums", "mins", "maxs"):
        if want[k] is None:
            assert got[k] is None, (what, k)
            continue
        g = got[k].reshape(want[k].shape)
        assert g.dtype == want[k].dtype and g.tobytes() == want[k].tobytes(), (what, k, np.argwhere(g.view(np.uint8) != want[k].view(np.uint8))[:5])
    st = got["stats"]
    assert st["points"] == st["outside"] + st["invalid"] + sum(st["under"]) + sum(st["over"]) + st["binned"], what


def _bytes(got):
    return [None if got[k] is None else got[k].tobytes() for k in ("count", "sum_weight", "sums", "mins", "maxs")] + [got["stats"]]


def _range(v):
    fin = v[np.isfinite(v)]
    return float(fin.min()), float(fin.max())


def _span(v):
    """a uniform range around the finite values of v that is valid also where they are all the same"""
    lo, hi = _range(v)
    return (lo, hi) if lo < hi else (lo - 1.0, hi + 1.0)


SCENES = [("ex0", lambda: scenes.example("ex0"), 0, False), ("ex3", lambda: scenes.example("ex3"), 1, False),
          ("amr3", lambda: scenes.amr(levels=3, fields=3), 1, False), ("amr3", lambda: scenes.amr(levels=3, fields=3), 0, False),
          ("amr3_holes", lambda: scenes.with_empty_cells(scenes.amr(levels=3, fields=2), fraction=0.15), 0, True)]


@pytest.mark.parametrize("idx", range(len(SCENES)), ids=[f"{s[0]}-f{s[2]}" for s in SCENES])
def test_profiles_equal_the_restatement_byte_for_byte(idx):
    name, make, form, empty = SCENES[idx]
    case = Case(make(), basis_form=form, allow_empty_cells=empty)
    R = case.hip_renderer()
    nf = len(case.scene.fields)
    lo, hi = _root_box(R.prep)                                 # grown: the box overhangs the scene, NaN there
    centre = tuple(0.5 * (np.asarray(lo) + np.asarray(hi)))
    for dims in LATTICES + [(37, 29, 23)]:
        lat = Lattice(R, lo, hi, dims)
        key, val = ("c", nf - 1), ("c", 0)
        a, b = _span(lat.source(key)) if np.isfinite(lat.source(key)).any() else (0.0, 1.0)
        some = bool(np.isfinite(lat.source(key) + lat.source(val)).any())      # a point at which both are finite
        what = f"{name} form {form} {dims}"
        for n in (1, 7, 64, 4096):
            lat.check([("uniform", key, a, b, n)], [val, ("r", centre)], what=f"{what} uniform {n}", binned=some)
            lat.check([("edges", key, np.unique(np.linspace(a, b, n + 1, dtype=np.float32)))],
                      [val], ("x", 2), what=f"{what} edges {n}", binned=some)
        got = lat.check([("uniform", ("r", centre), 0.0, float(np.linalg.norm(np.asarray(hi) - np.asarray(lo))), 16)], [key], what=f"{what} radial",
                        binned=bool(np.isfinite(lat.source(key)).any()))
        if dims == (37, 29, 23):
            assert got["stats"]["invalid"] > 0, what              # the overhang
    R.close()


@pytest.fixture(scope="module")
def amr3():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()
    yield case, R
    R.close()


@pytest.fixture(scope="module")
def inner(amr3):
    """a lattice inside amr3 (every value finite), 17 tiles"""
    case, R = amr3
    lo, hi = R.prep.voxel_bounds()
    return Lattice(R, np.asarray(lo, np.float32), np.asarray(hi, np.float32), (17, 16, 16))


def test_two_axes(inner):
    k0, k1 = ("c", 0), ("d", "q", (0, 1, 2))
    a0, b0 = _range(inner.source(k0))
    a1, b1 = _range(inner.source(k1))
    for n0, n1 in ((7, 5), (64, 64), (1024, 1024)):
        got = inner.check([("uniform", k0, a0, b0, n0), ("uniform", k1, a1, b1, n1)], [("c", 1), ("c", 2)], ("c", 2), what=f"2-D {n0}x{n1}")
        assert got["count"].shape == (n1, n0) and got["sums"].shape == (2, n1, n0)
        assert got["stats"]["ldsTable"] == (1 if (n0, n1) == (7, 5) else 0)
    e0 = np.quantile(inner.source(k0), np.linspace(0, 1, 8)).astype(np.float32)
    inner.check([("edges", k0, np.unique(e0)), ("edges", k1, np.array([a1, 0.5 * (a1 + b1), b1], np.float32))], [("c", 1)], what="2-D edges")


def test_bin_count_sweep_crosses_the_lds_choice(inner):
    key = ("c", 1)
    a, b = _range(inner.source(key))
    seen = set()
    for p in range(17):
        got = inner.check([("uniform", key, a, b, 1 << p)], [("c", 0), ("c", 2)], ("c", 0), what=f"B = 2^{p}")
        seen.add(got["stats"]["ldsTable"])
    assert seen == {0, 1}


def test_ranges_and_edges_on_data_values(inner):
    k0, k1 = ("c", 0), ("c", 1)
    v0, v1 = (np.sort(v[np.isfinite(v)]) for v in (inner.source(k0), inner.source(k1)))
    n = min(v0.size, v1.size)
    assert n > 4000
    # a narrow range: under and over on the first axis, and on the second among those the first lets through
    got = inner.check([("uniform", k0, float(v0[n // 4]), float(v0[3 * n // 4]), 9), ("uniform", k1, float(v1[n // 3]), float(v1[2 * n // 3]), 5)],
                      [("c", 2)], what="narrow")
    st = got["stats"]
    assert st["under"][0] > 0 and st["over"][0] > 0 and st["under"][1] + st["over"][1] > 0
    # lo and hi exactly data values (the extremes: nothing is under or over), and edges that are data values, the last too
    got = inner.check([("uniform", k0, float(v0[0]), float(v0[-1]), 13)], [k1], what="lo, hi = min, max")
    assert got["stats"]["under"][0] == got["stats"]["over"][0] == 0 and got["count"][-1] > 0
    e = np.unique(v0[[0, n // 7, n // 3, n // 2, (4 * n) // 5, n - 1]])
    got = inner.check([("edges", k0, e)], [k1], k1, what="edges = data values")
    assert got["stats"]["under"][0] == got["stats"]["over"][0] == 0 and got["count"].sum() == got["stats"]["binned"] >= n - 1
    got = inner.check([("edges", k0, e[1:-1])], [k1], what="inner edges = data values")
    assert got["stats"]["under"][0] > 0 and got["stats"]["over"][0] > 0


@pytest.fixture(scope="module")
def rich():
    """amr3 with three fields and three more: a constant (3), +-3e38 (4), and field 0 with one Inf cell (5)"""
    scene = scenes.amr(levels=3, fields=3)
    f = np.array(scene.fields[0], np.float32, copy=True)          # the fields are indexed by cell id: these follow field 0's
    scene.fields.append(np.full(len(f), 2.5, np.float32))
    scene.fields.append(np.where(f > np.median(f), 3e38, -3e38).astype(np.float32))
    f[len(f) // 2] = np.inf
    scene.fields.append(f)
    case = Case(scene, W=32, H=32, xf_domains=[(0.0, 1.0)] * 6)
    R = case.hip_renderer()
    lo, hi = R.prep.voxel_bounds()
    yield Lattice(R, np.asarray(lo, np.float32), np.asarray(hi, np.float32), (64, 9, 8))
    R.close()


def test_contention_shapes(rich):
    lat = rich
    n = int(np.prod(lat.dims))
    L = np.arange(n)
    vals = [("c", 0), ("c", 1)]
    got = lat.check([("uniform", ("c", 3), 0.0, 6.0, 3)], vals, ("c", 2), what="a constant key")
    assert np.count_nonzero(got["count"]) == 1 and got["count"].sum() == got["stats"]["binned"] > n // 2
    x = lat.source(("x", 0))
    got = lat.check([("uniform", ("x", 0), float(lat.lo[0]), float(lat.hi[0]), 64)], vals, what="64 bins in every wave")
    assert np.count_nonzero(got["count"]) == 64 and got["count"].sum() == got["stats"]["binned"] and np.unique(x).size == 64
    lat.check([("labels", (L % 64).astype(np.int32), 64)], vals, ("c", 2), what="labels L % 64")
    lat.check([("labels", np.zeros(n, np.int32), 1)], vals, ("c", 2), what="labels all 0")
    got = lat.check([("labels", np.full(n, -1, np.int32), 3)], vals, ("c", 2), what="labels all -1", binned=False)
    assert got["stats"]["outside"] == n == got["stats"]["points"]
    assert np.isposinf(got["mins"]).all() and np.isneginf(got["maxs"]).all() and not got["count"].any()
    got = lat.check([("labels", (L % 100003).astype(np.int32), 100003)], vals, ("c", 2), what="labels L % 100003")
    assert got["stats"]["ldsTable"] == 0
    lat.check([("labels_device", (L % 5 - 1).astype(np.int32), 4), ("uniform", ("c", 1), *_range(lat.source(("c", 1))), 6)], vals, what="device labels, two axes")


def test_every_kind_of_source_as_key_value_and_weight(rich):
    lat = rich
    centre = (10.0, 12.5, 7.0)
    kinds = [("c", 1), ("d", "q", (0, 1, 2)), ("r", centre), ("x", 1)]
    for key in kinds:
        a, b = _span(lat.source(key))
        for value in kinds:
            for weight in kinds + [None]:
                lat.check([("uniform", key, a, b, 11)], [value], weight, what=f"key {key[0]} value {value[0]} weight {weight and weight[0]}")
    a, b = _span(lat.source(("c", 0)))
    axis = [("uniform", ("c", 0), a, b, 11)]
    lat.check(axis, [("c", 1), ("c", 1), ("c", 0), ("r", centre)], ("c", 1), what="repeated sources, four values")
    lat.check(axis, [("c", 1)], ("d", "divergence", (0, 1, 2)), what="a weight of both signs")
    assert (lat.source(("d", "divergence", (0, 1, 2))) < 0).any()
    lat.check(axis, [("c", 1), ("c", 2)], minmax=False, what="no min / max")
    lat.check(axis, what="counts only")
    got = lat.check(axis, [("c", 4)], ("c", 3), what="w * v overflows")           # 2.5 * 3e38
    assert got["stats"]["invalid"] > 0
    got = lat.check(axis, [("c", 5)], what="an Inf cell")
    assert got["stats"]["invalid"] > 0
    got = lat.check([("uniform", ("c", 5), a, b, 11)], [("c", 1)], what="an Inf cell in the key")
    assert got["stats"]["invalid"] + got["stats"]["over"][0] > 0


def test_profiles_in_world_space():
    case = Case(scenes.amr(levels=3, fields=2))
    R = case.hip_renderer()
    R.setVoxelSpaceTransform(XFM["vx"], XFM["vy"], XFM["vz"], XFM["p"])
    lat = Lattice(R, np.array([-4, -6, -5], np.float32), np.array([30, 24, 26], np.float32), (41, 33, 27), world=True)
    a, b = _span(lat.source(("c", 1)))
    got = lat.check([("uniform", ("c", 1), a, b, 32), ("uniform", ("r", (10.0, 8.0, 9.0)), 0.0, 30.0, 8)], [("c", 0), ("x", 2)], what="world")
    assert got["stats"]["invalid"] > 0
    R.close()


def test_labels_of_regions_and_basins_give_their_tables(amr3):
    import torch
    case, R = amr3
    lo, hi = _root_box(R.prep)
    dims = (37, 29, 23)
    V = R.resample(lo, hi, dims, channel=1, fill=NAN)
    iso = float(np.median(V[np.isfinite(V)]))
    for what in ("regions", "basins", "derived"):
        if what == "regions":
            res, src = R.regions(lo, hi, dims, iso, channel=1, keep_values=True), channel(1)
        elif what == "basins":
            res, src = R.basins(lo, hi, dims, iso, 0.05, channel=1, keep_values=True), channel(1)
        else:
            res, src = R.regionsDerived(lo, hi, dims, 0.0, "q", channels=(0, 1, 2), keep_values=True), derived("q", (0, 1, 2))
        table = res["regions"]
        assert len(table) > 1
        dev = torch.from_numpy(res["labels"].reshape(-1)).to("cuda:0")
        for lab in (res["labels"], dev):
            got = R.profile(lo, hi, dims, binding.labels(lab, len(table)), [src])
            assert got["count"].tobytes() == table["points"].tobytes(), what
            assert got["sums"][0].tobytes() == table["sumFixed"].tobytes(), what
            assert got["stats"]["valueExponent"][0] == res["sum_exponent"], what
            assert got["mins"][0].tobytes() == table["min"].tobytes() and got["maxs"][0].tobytes() == table["max"].tobytes(), what
            assert got["stats"]["outside"] == int((res["labels"] < 0).sum()) and got["stats"]["binned"] == res["num_inside"], what
        m = binding.profile_measures(got, lo, hi, dims)
        r = binding.region_measures(table, res["sum_exponent"], lo, hi, dims)
        assert np.array_equal(m["sums"][0], r["sum"]) and np.array_equal(m["means"][0], r["mean"]) and np.array_equal(m["volume"], r["volume"])


def test_profiles_do_not_depend_on_frame_state_or_options(amr3):
    case, R = amr3
    lo, hi = _root_box(R.prep)
    dims = (37, 29, 23)
    lat = Lattice(R, lo, hi, dims)
    a, b = _span(lat.source(("c", 1)))
    args = ([("uniform", ("c", 1), a, b, 50), ("uniform", ("r", (10.0, 12.0, 8.0)), 0.0, 40.0, 9)], [("c", 0), ("d", "q", (0, 1, 2))], ("c", 2))
    want = _bytes(lat.check(*args, what="before"))
    call = lambda H=None: _bytes(lat.got(*args, R=H))              # noqa: E731
    assert call() == want, "two consecutive calls"
    M = multi_handle(R)
    assert call(M) == want, "a multi-device handle"
    M.close()
    for what in frame_perturbations(case, R):
        assert call() == want, what
    for patch in range(4):
        R.setOption("sample_patch", patch)
        assert call() == want, f"sample_patch {patch}"
    R.setOption("sample_uniform", 0)
    assert call() == want, "sample_uniform 0"
    R.setOption("sample_uniform", 1)
    R.setOption("sample_patch", 0)
    ms = R.profileStageMs()
    assert len(ms) == 4 and all(m > 0 for m in ms), ms
    for form in (0, 1):                                          # each form against the restatement fed that form's lattices
        R.setOption("basis_form", form)
        Lattice(R, lo, hi, dims).check(*args, what=f"basis_form {form}")
    R.setOption("basis_form", case.basis_form)


# ---- errors ----
def _raw(R, lo=(0, 0, 0), hi=(8, 8, 8), dims=(9, 9, 9), flags=0, axes=None, num_axes=None, values=(channel(0),), num_values=None,
         weight=None, null=(), only=None):
    """the C entry point with one thing wrong; `null`: names of pointers passed as NULL; `only`: "mins" / "maxs" alone"""
    axes = [binding.uniform(channel(0), 0.0, 1.0, 4)] if axes is None else axes
    ax = (binding.ExaHipProfileAxis * max(1, len(axes)))(*[a.struct for a in axes])
    nv = len(values) if num_values is None else num_values
    vals = (binding.ExaHipSource * max(1, len(values)))(*values)
    room = 1 << 16
    count, sw, sums = np.full(room, 77, np.uint64), np.full(room, 77, np.int64), np.full(4 * room, 77, np.int64)
    mins, maxs = np.full(4 * room, 77, np.float32), np.full(4 * room, 77, np.float32)
    st = binding.ExaHipProfileStats()
    p = lambda name, obj: None if name in null else obj            # noqa: E731
    rc = binding.lib().exa_hip_profile(
        R.h, p("lo", (C.c_float * 3)(*lo)), p("hi", (C.c_float * 3)(*hi)), p("dims", (C.c_int32 * 3)(*dims)), flags, p("axes", ax),
        len(axes) if num_axes is None else num_axes, p("values", vals), nv, C.byref(weight) if weight is not None else None,
        p("count", count.ctypes.data), sw.ctypes.data if (weight is not None) != ("sumWeight" in null) else None, p("sums", sums.ctypes.data),
        None if only == "maxs" else mins.ctypes.data, None if only == "mins" else maxs.ctypes.data, C.byref(st), None)
    untouched = all(np.all(a == 77) for a in (count, sw, sums, mins, maxs))
    return rc, untouched, binding.lib().exa_hip_last_error(R.h).decode()


def test_refused_arguments():
    case = Case(scenes.amr(levels=3, fields=3), W=32, H=32)
    R = case.hip_renderer()                                    # no render yet: the module holds no frame state
    lat = Lattice(R, (0, 0, 0), (8, 8, 8), (9, 9, 9))
    good = ([("uniform", ("c", 0), *_span(lat.source(("c", 0))), 4)], [("c", 0)])
    nf = len(case.scene.fields)
    u = lambda **kw: binding.uniform(channel(0), kw.get("lo", 0.0), kw.get("hi", 1.0), kw.get("n", 4))      # noqa: E731
    lab = np.zeros(729, np.int32)
    bad_lab = lab.copy()
    bad_lab[[100, 50, 700]] = [4, 9, 3]
    ascending = np.array([0.0, 1.0, 2.0], np.float32)
    bad = [dict(flags=binding.SAMPLE_WORLD_SPACE),               # world space before a frame state
           dict(null=("lo",)), dict(null=("hi",)), dict(null=("dims",)), dict(null=("axes",)), dict(null=("count",)),
           dict(lo=(math.nan, 0, 0)), dict(hi=(8, math.inf, 8)), dict(hi=(8, 0, 8)), dict(dims=(0, 9, 9)), dict(dims=(9, 9, -1)),
           dict(dims=(2 ** 11, 2 ** 11, 2 ** 9)), dict(num_axes=0), dict(num_axes=3), dict(axes=[u(), binding.labels(lab, 3)]),
           dict(num_values=-1), dict(num_values=5), dict(null=("values",)), dict(null=("sums",)),
           dict(values=(derived("vorticity"),)), dict(values=(derived(99),)), dict(values=(channel(nf),)), dict(values=(channel(-1),)),
           dict(values=(derived("q", (0, 1, nf)),)), dict(values=(coordinate(3),)), dict(values=(radius((0, math.nan, 0)),)),
           dict(values=(binding.ExaHipSource(9, (C.c_int32 * 3)(), 0, (C.c_float * 3)()),)), dict(weight=channel(nf)),
           dict(axes=[u(n=0)]), dict(axes=[u(n=-3)]), dict(axes=[u(lo=1.0, hi=1.0)]), dict(axes=[u(lo=2.0, hi=1.0)]), dict(axes=[u(lo=math.nan)]),
           dict(axes=[u(hi=math.inf)]), dict(axes=[u(lo=-3e38, hi=3e38)]), dict(axes=[u(lo=0.0, hi=1e-45, n=1 << 20)]),
           dict(axes=[binding.edges(channel(0), ascending[::-1])]), dict(axes=[binding.edges(channel(0), [0.0, 1.0, 1.0])]),
           dict(axes=[binding.edges(channel(0), [0.0, math.nan, 2.0])]), dict(axes=[binding.edges(channel(0), [0.0, 1.0, math.inf])]),
           dict(axes=[u(n=(1 << 24) + 1)]), dict(axes=[u(n=1 << 13), u(n=1 << 12)]), dict(axes=[u(n=1 << 30), u(n=1 << 30)]),
           dict(weight=channel(0), null=("sumWeight",)), dict(null=("sumWeight",)), dict(only="mins"), dict(only="maxs"),
           dict(flags=2), dict(flags=4), dict(flags=32), dict(flags=1 << 30),
           dict(axes=[binding.labels(bad_lab, 3)]), dict(axes=[binding.labels(bad_lab, 3), u()])]
    for kw in bad:
        rc, untouched, msg = _raw(R, **kw)
        assert rc != 0 and untouched and msg.startswith("exa_hip_profile: "), (kw, rc, msg)
        lat.check(*good, what=f"after {sorted(kw)}")            # the handle still works, and rightly
    rc, _, msg = _raw(R, axes=[binding.labels(bad_lab, 3)])
    assert "L = 50" in msg, msg                                # the first such point
    rc, _, msg = _raw(R, flags=binding.SAMPLE_WORLD_SPACE)
    assert "frame state" in msg, msg
    # sources that need no lattice in memory need no frame state's transform either way, and the valid raw call passes
    assert _raw(R)[0] == 0 and _raw(R, weight=channel(1))[0] == 0 and _raw(R, values=(), null=("values", "sums"))[0] == 0
    frame = R.render()
    assert _raw(R, flags=binding.SAMPLE_WORLD_SPACE)[0] == 0
    assert R.render().shape == frame.shape
    R.close()


def test_scene_without_kd_tree_is_refused_for_a_channel_only():
    R = without_kd_tree(Case(scenes.amr(levels=3), W=32, H=32)).hip_renderer()
    rc, untouched, msg = _raw(R)
    assert rc != 0 and untouched and msg.startswith("exa_hip_profile: ") and "kd-tree" in msg, msg
    lo, hi, dims = (0, 0, 0), (8, 8, 8), (9, 9, 9)
    got = R.profile(lo, hi, dims, binding.uniform(radius((4, 4, 4)), 0.0, 8.0, 8), [coordinate(0)], coordinate(2))
    want = ref.profile([ref.uniform(ref.radius(lo, hi, dims, (4, 4, 4)), 0.0, 8.0, 8)], [ref.coordinate(lo, hi, dims, 0)], ref.coordinate(lo, hi, dims, 2))
    _same(got, want, "no kd tree, no lattice in memory")
    assert R.render().shape == (32, 32)                        # the handle still renders (through its LBVH)
    R.close()
