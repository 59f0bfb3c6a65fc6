"""ctypes binding of the C ABI in include/exa_hip.h (libexa_hip.so) and a
`Renderer` that keeps the method names of the reference's exa::OptixRenderer
(exa/OptixRenderer.h:32-97) so tests read like calls into the reference.

There is no CPU fallback: if the HIP module is missing or no GPU is present,
loading / creating fails loudly.
"""
import ctypes as C
import os
from collections import namedtuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# EXA_HIP_LIB: another build of the same module (A/B timing of kernel variants, tools/ab_variants.sh)
LIB_PATH = os.environ.get("EXA_HIP_LIB") or os.path.join(_HERE, "libexa_hip.so")

NUM_XF_VALUES, MAX_CHANNELS, MAX_ISO, MAX_CONTOUR = 128, 10, 2, 3
# the module's default of option "basis_form" (exa_module.cpp): association of the eight-corner basis sums
DEFAULT_BASIS_FORM = 1


class _Iso(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("value", C.c_float), ("channel", C.c_int32)]


class _Contour(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("normal", C.c_float * 3), ("channel", C.c_int32), ("offset", C.c_float)]


class _Clip(C.Structure):
    _fields_ = [("lo", C.c_float * 3), ("hi", C.c_float * 3), ("enabled", C.c_int32)]


class _AO(C.Structure):
    _fields_ = [("length", C.c_float), ("enabled", C.c_int32)]


class ExaHipFrameState(C.Structure):
    _fields_ = [("cam_pos", C.c_float * 3), ("cam_dir00", C.c_float * 3),
                ("cam_dirDu", C.c_float * 3), ("cam_dirDv", C.c_float * 3),
                ("iso", _Iso * MAX_ISO), ("contour", _Contour * MAX_CONTOUR),
                ("clipBox", _Clip), ("ao", _AO), ("clockScale", C.c_float),
                ("xfm_vx", C.c_float * 3), ("xfm_vy", C.c_float * 3),
                ("xfm_vz", C.c_float * 3), ("xfm_p", C.c_float * 3),
                ("frameID", C.c_int32), ("xfDomain", (C.c_float * 2) * MAX_CHANNELS),
                ("xfOpacityScale", C.c_float)]


class ExaHipParams(C.Structure):
    _fields_ = [("dt", C.c_float), ("numPrimaryChannels", C.c_int32), ("colormapChannel", C.c_int32),
                ("gradientShadingDVR", C.c_int32), ("gradientShadingISO", C.c_int32),
                ("numChannels", C.c_int32), ("spaceSkippingEnabled", C.c_int32)]


class ExaHipTracer(C.Structure):
    _fields_ = [("enabled", C.c_int32), ("channels", C.c_int32 * 3), ("numTraces", C.c_int32),
                ("numTimesteps", C.c_int32), ("steplen", C.c_float)]


class ExaHipScene(C.Structure):
    _fields_ = [("bricks", C.c_void_p), ("numBricks", C.c_uint64),
                ("regions", C.c_void_p), ("numRegions", C.c_uint64),
                ("leafList", C.c_void_p), ("leafListSize", C.c_uint64),
                ("scalars", C.c_void_p), ("channelOffset", C.c_void_p),
                ("totalCells", C.c_uint64), ("numFields", C.c_int32),
                ("voxelBounds_lo", C.c_float * 3), ("voxelBounds_hi", C.c_float * 3),
                ("kdNodes", C.c_void_p), ("numKdNodes", C.c_uint64), ("kdRoot", C.c_int32), ("allowEmptyCells", C.c_int32)]


class ExaHipStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("segments", "sample_evals", "samples", "brick_visits", "corner_loads",
                                          "iso_segments", "iso_evals", "nodes_visited", "node_bytes", "pixels")] + \
               [("diag", C.c_uint64 * 9), ("phase_cycles", C.c_uint64 * 5), ("kernel_ms", C.c_float), ("rebuild_ms", C.c_float),
                ("walk_restarts", C.c_uint64), ("walk_union_nodes", C.c_uint64), ("walk_probe_overflow", C.c_uint64),
                ("wave_iters", C.c_uint64), ("tile_iters", C.c_uint64), ("walk_leaf_visits", C.c_uint64)]

    def asdict(self):
        d = {}
        for n, t in self._fields_:
            v = getattr(self, n)
            d[n] = int(v) if t is C.c_uint64 else (float(v) if t is C.c_float else [int(x) for x in v])
        return d


# exa_hip_histogram (include/exa_hip.h)
HIST_MAX_BINS = 4096
HIST_MAX_LEVELS = 32


class ExaHipFieldStats(C.Structure):
    _fields_ = [("slots", C.c_uint64), ("empty", C.c_uint64), ("nan", C.c_uint64), ("under", C.c_uint64), ("over", C.c_uint64),
                ("binned", C.c_uint64), ("levelCells", C.c_uint64 * HIST_MAX_LEVELS), ("min", C.c_float), ("max", C.c_float)]

    def asdict(self):
        """counts as ints, levelCells as a uint64 array, min / max as numpy float32 (their bits are part of the result)"""
        d = {k: int(getattr(self, k)) for k in ("slots", "empty", "nan", "under", "over", "binned")}
        d["levelCells"] = np.array(self.levelCells, dtype=np.uint64)
        d["min"], d["max"] = np.float32(self.min), np.float32(self.max)
        return d


BRICK_DTYPE = np.dtype([("lower", "<i4", 3), ("size", "<i4", 3), ("level", "<i4"), ("begin", "<u4")])
REGION_DTYPE = np.dtype([("dom_lo", "<f4", 3), ("dom_hi", "<f4", 3), ("vr_lo", "<f4"), ("vr_hi", "<f4"),
                         ("leafListBegin", "<i4"), ("leafListSize", "<i4"), ("finestLevelCellWidth", "<f4")])
KDNODE_DTYPE = np.dtype([("split", "<f4"), ("axis", "<i4"), ("left", "<i4"), ("right", "<i4")])
KD_EMPTY = -2 ** 31

# exa_hip_sample_points / exa_hip_resample flags (include/exa_hip.h)
SAMPLE_WORLD_SPACE = 1
SAMPLE_GRADIENT = 2
SAMPLE_GRADIENT_NORMALIZED = 4

# exa_hip_streamlines flags and end reasons (include/exa_hip.h)
STREAM_FORWARD = 1
STREAM_BACKWARD = 2
STREAM_NORMALIZE = 4
STREAM_VELOCITIES = 8
STREAM_MAX_STEPS = 1 << 20
STREAM_END_NONE, STREAM_END_MAXSTEPS, STREAM_END_LEFT, STREAM_END_NOVALUE, STREAM_END_STAGNANT = range(5)
# exa_hip_lic (include/exa_hip.h): the cap of half_length, and the end reason it adds to the STREAM_END_* ones
LIC_MAX_STEPS = 4096
LIC_END_IMAGE = 5
# exa_hip_flowmap (include/exa_hip.h): exactly one of the two directions
FLOWMAP_FORWARD = 1
FLOWMAP_BACKWARD = 2

# exa_hip_project (include/exa_hip.h)
PROJECT_NORMALIZE = 4
PROJECT_MAX_SAMPLES = 1 << 20

# exa_hip_sample_triangles (include/exa_hip.h)
SURFACE_FROM_ISOSURFACE = 8
SURFACE_MAX_N = 64
SURFACE_MAX_CHANNELS = 4

# exa_hip_isolines (include/exa_hip.h)
ISOLINES_KEEP_VALUES = 16
ISOLINES_MAX_LEVELS = 256

# exa_hip_regions (include/exa_hip.h)
REGIONS_KEEP_VALUES = 16
REGIONS_BELOW = 32
REGIONS_FACES = 64
# ExaHipRegion (a connected region of exa_hip_regions, not a region of the scene: REGION_DTYPE above): 84 bytes of fields, padded to 88
LABELLED_REGION_DTYPE = np.dtype(dict(names=["points", "sumFixed", "sumIndex", "lo", "hi", "first", "argMin", "argMax", "min", "max"],
                             formats=["<u8", "<i8", ("<u8", 3), ("<i4", 3), ("<i4", 3), "<u4", "<u4", "<u4", "<f4", "<f4"],
                             offsets=[0, 8, 16, 40, 52, 64, 68, 72, 76, 80], itemsize=88))
# ExaHipBasin (a basin of exa_hip_basins): the fields of ExaHipRegion, then the highest pass; 96 bytes, no padding
BASIN_DTYPE = np.dtype([("points", "<u8"), ("sumFixed", "<i8"), ("sumIndex", "<u8", 3), ("lo", "<i4", 3), ("hi", "<i4", 3),
                        ("first", "<u4"), ("argMin", "<u4"), ("argMax", "<u4"), ("min", "<f4"), ("max", "<f4"),
                        ("neighbour", "<i4"), ("saddle", "<f4"), ("depth", "<f4")])
assert BASIN_DTYPE.itemsize == 96

# exa_hip_critical_points (include/exa_hip.h): the flag, the bits of a point's type beside n+ (bits 0-1), ExaHipCriticalPoint
# (104 bytes, no padding) and the fields of ExaHipCriticalStats
CRITICAL_PROBE = 16
CRITICAL_MAX_ITERATIONS = 32
CRITICAL = {"n_plus_mask": 3, "sink": 0, "saddle_1": 1, "saddle_2": 2, "source": 3, "spiral": 4, "degenerate": 8}
CRITICAL_POINT_DTYPE = np.dtype(dict(names=["cell", "type", "local", "position", "lastStep", "jacobian", "invariants", "discriminant"],
                                     formats=["<u4", "<i4", ("<f4", 3), ("<f4", 3), "<f4", ("<f4", 9), ("<f8", 3), "<f8"],
                                     offsets=[0, 4, 8, 20, 32, 36, 72, 96], itemsize=104))
CRITICAL_STATS = ("cells", "invalidCells", "candidates", "found", "nonFinite", "leftCell", "notConverged")

# exa_hip_profile (include/exa_hip.h): the source kinds, the flag, the caps and the structs
SOURCE_CHANNEL, SOURCE_DERIVED, SOURCE_RADIUS, SOURCE_COORDINATE = range(4)
PROFILE_LABELS_DEVICE = 16
PROFILE_MAX_VALUES = 4
PROFILE_MAX_BINS = 1 << 24


class ExaHipSource(C.Structure):
    _fields_ = [("kind", C.c_int32), ("channels", C.c_int32 * 3), ("quantity", C.c_int32), ("centre", C.c_float * 3)]


class ExaHipProfileAxis(C.Structure):
    _fields_ = [("source", ExaHipSource), ("numBins", C.c_int32), ("lo", C.c_float), ("hi", C.c_float),
                ("edges", C.c_void_p), ("labels", C.c_void_p)]


class ExaHipProfileStats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("outside", C.c_uint64), ("invalid", C.c_uint64), ("under", C.c_uint64 * 2),
                ("over", C.c_uint64 * 2), ("binned", C.c_uint64), ("weightExponent", C.c_int32),
                ("valueExponent", C.c_int32 * 4), ("ldsTable", C.c_int32)]

    def asdict(self):
        d = {k: int(getattr(self, k)) for k in ("points", "outside", "invalid", "binned", "weightExponent", "ldsTable")}
        d["under"], d["over"] = [int(v) for v in self.under], [int(v) for v in self.over]
        d["valueExponent"] = [int(v) for v in self.valueExponent]
        return d


# exa_hip_raycast_iso (include/exa_hip.h)
CROSS_MAX_REFINE = 32
RAYCAST_KEYS = ("t", "position", "value", "gradient", "index", "side", "crossings")

# exa_hip_*_derived quantities (include/exa_hip.h: EXA_DERIVED_*), by name, and the number of components of each
DERIVED = {"speed": 0, "divergence": 1, "vorticity": 2, "vorticity_magnitude": 3, "q": 4, "helicity": 5}
DERIVED_COMPONENTS = {0: 1, 1: 1, 2: 3, 3: 1, 4: 1, 5: 1}


def derived_quantity(q):
    """the number of a derived quantity given by name (a key of DERIVED, any letter case) or by number; an unknown number
    passes through for the module to refuse, an unknown name is a ValueError"""
    if isinstance(q, str):
        if q.lower() not in DERIVED:
            raise ValueError(f"unknown derived quantity {q!r} (one of {', '.join(DERIVED)})")
        return DERIVED[q.lower()]
    return int(q)


SURFACE_KEYS = ("sum", "count", "areaNormal", "subdiv")


def surface_integrals(samples):
    """From the dict of Renderer.sampleTriangles (numpy), in float64 and sequentially in ascending triangle order (no pairwise
    sums: the same operations as exa::Renderer::surfaceIntegrals).  Per triangle: area [m] = |areaNormal|, mean [m, C] = sum /
    count (NaN where count == 0), integral [m, C] = mean * area.  Totals over the valid triangles (subdiv > 0; the others are
    counted in invalid_triangles), per channel: covered_area [C], uncovered_area [C] and uncovered_triangles [C] (count == 0),
    total_integral [C] = the sum of mean * area and force [C, 3] = the sum of mean * areaNormal over the covered ones; with three
    channels flux = the sum of (mean0 * n.x + mean1 * n.y) + mean2 * n.z over the triangles all three cover (else NaN).  The
    samples ride along under "samples"."""
    total, count = samples["sum"], samples["count"]
    normal = samples["areaNormal"].astype(np.float64)
    subdiv = samples["subdiv"]
    m, nc = total.shape
    with np.errstate(all="ignore"):
        area = np.sqrt((normal[:, 0] * normal[:, 0] + normal[:, 1] * normal[:, 1]) + normal[:, 2] * normal[:, 2])
        mean = np.where(count > 0, total / np.where(count > 0, count, 1).astype(np.float64), np.nan)
        integral = mean * area[:, None]
        valid = subdiv > 0
        covered = valid[:, None] & (count > 0)
        # np.cumsum adds along the axis in order, from +0.0
        seq = lambda terms: np.concatenate([np.zeros((1,) + terms.shape[1:]), terms]).cumsum(axis=0)[-1]        # noqa: E731
        covered_area = seq(np.where(covered, area[:, None], 0.0))
        uncovered = valid[:, None] & (count == 0)
        uncovered_area = seq(np.where(uncovered, area[:, None], 0.0))
        total_integral = seq(np.where(covered, integral, 0.0))
        force = seq(np.where(covered[:, :, None], mean[:, :, None] * normal[:, None, :], 0.0))
        flux = float("nan")
        if nc == 3:
            every = covered.all(axis=1)
            flux = float(seq(np.where(every, (mean[:, 0] * normal[:, 0] + mean[:, 1] * normal[:, 1]) + mean[:, 2] * normal[:, 2], 0.0)))
    return dict(samples=samples, area=area, mean=mean, integral=integral, covered_area=covered_area, uncovered_area=uncovered_area,
                uncovered_triangles=uncovered.sum(axis=0).astype(np.uint64), total_integral=total_integral, force=force, flux=flux,
                invalid_triangles=int((~valid).sum()))


class ExaHipRays(C.Structure):
    _fields_ = [("org", C.c_float * 3), ("orgDu", C.c_float * 3), ("orgDv", C.c_float * 3),
                ("dir", C.c_float * 3), ("dirDu", C.c_float * 3), ("dirDv", C.c_float * 3),
                ("width", C.c_int32), ("height", C.c_int32), ("tmin", C.c_float), ("dt", C.c_float), ("numSamples", C.c_int32)]


class ExaHipPlane(C.Structure):
    _fields_ = [("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("nu", C.c_int32), ("nv", C.c_int32)]


_vp, _i32, _u64, _f32, _P = C.c_void_p, C.c_int32, C.c_uint64, C.c_float, C.POINTER

# every symbol include/exa_hip.h declares: name -> (restype, None = the int return code; argtypes, None = takes none).  lib()
# sets the prototypes from it
_ABI = {
    "exa_prep_create": (None, [_vp, _u64, _vp, _u64, _P(_vp), _P(_u64), _i32, _i32, _i32, _P(_vp)]),
    "exa_prep_create_ex": (None, [_vp, _u64, _vp, _u64, _P(_vp), _P(_u64), _i32, _i32, _i32, _i32, _P(_vp)]),
    "exa_prep_destroy": (None, [_vp]),
    "exa_prep_ropes": (None, [_vp, _P(_u64), _P(_u64), _vp, _vp, _vp, _vp, _P(_i32)]),
    "exa_prep_cube_records": (None, [_vp, _u64, _vp, _u64, _vp, _P(_i32), _vp]),
    "exa_prep_scene": (None, [_vp, _P(ExaHipScene)]),
    "exa_prep_set_kd_tree": (None, [_vp, _vp, _u64, _i32]),
    "exa_prep_last_error": (C.c_char_p, None),
    "exa_hip_create": (None, [_P(ExaHipScene), _i32, _P(_vp)]),
    "exa_hip_create_multi": (None, [_P(ExaHipScene), _P(_i32), _i32, _P(_vp)]),
    "exa_hip_destroy": (None, [_vp]),
    "exa_hip_resize": (None, [_vp, _i32, _i32]),
    "exa_hip_set_frame_state": (None, [_vp, _P(ExaHipFrameState)]),
    "exa_hip_set_xf": (None, [_vp, _i32, _vp]),
    "exa_hip_set_params": (None, [_vp, _P(ExaHipParams)]),
    "exa_hip_set_triangles": (None, [_vp, _vp, _u64, _vp, _u64]),
    "exa_hip_reset_tracer": (None, [_vp, _P(ExaHipTracer), _vp]),
    "exa_hip_set_tracer_enabled": (None, [_vp, _i32]),
    "exa_hip_advance_tracer": (None, [_vp, _P(_i32)]),
    "exa_hip_read_traces": (None, [_vp, _vp]),
    "exa_hip_set_shard": (None, [_vp, _i32, _i32]),
    "exa_hip_output_pixels": (C.c_uint64, [_vp]),
    "exa_hip_untile": (None, [_vp, _vp, _u64, _i32, _vp, _vp]),
    "exa_hip_render": (None, [_vp, _vp, _i32, _vp, _i32]),
    "exa_hip_render_stats": (None, [_vp, _vp, _i32, _P(ExaHipStats)]),
    "exa_hip_get_stats": (None, [_vp, _P(ExaHipStats)]),
    "exa_hip_read_accum": (None, [_vp, _vp]),
    "exa_hip_write_accum": (None, [_vp, _vp]),
    "exa_hip_read_activity": (None, [_vp, _i32, _vp]),
    "exa_hip_set_option": (None, [_vp, C.c_char_p, _i32]),
    "exa_hip_last_error": (C.c_char_p, [_vp]),
    "exa_hip_sample_points": (None, [_vp, _vp, _u64, _vp, _i32, _i32, _f32, _vp, _vp, _vp, _i32, _vp, _i32]),
    "exa_hip_resample": (None, [_vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _i32, _vp, _i32]),
    "exa_hip_isosurface": (None, [_vp, _vp, _vp, _vp, _i32, _f32, _i32, _P(_u64), _P(_u64), _vp]),
    "exa_hip_isosurface_read": (None, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_isosurface_release": (None, [_vp]),
    "exa_hip_isosurface_stage_ms": (None, [_vp, _vp]),
    "exa_hip_sample_derived": (None, [_vp, _vp, _u64, _vp, _i32, _i32, _f32, _vp, _vp, _i32, _vp, _i32]),
    "exa_hip_resample_derived": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _i32, _vp, _i32]),
    "exa_hip_isosurface_derived": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _P(_u64), _P(_u64), _vp]),
    "exa_hip_derived_ms": (None, [_vp, _P(_f32)]),
    "exa_hip_isolines": (None, [_vp, _P(ExaHipPlane), _i32, _vp, _i32, _i32, _P(_u64), _P(_u64), _vp]),
    "exa_hip_isolines_derived": (None, [_vp, _P(ExaHipPlane), _vp, _i32, _vp, _i32, _i32, _P(_u64), _P(_u64), _vp]),
    "exa_hip_isolines_read": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_isolines_release": (None, [_vp]),
    "exa_hip_isolines_stage_ms": (None, [_vp, _vp]),
    "exa_hip_regions": (None, [_vp, _vp, _vp, _vp, _i32, _f32, _i32, _P(_u64), _P(_u64), _P(_i32), _vp]),
    "exa_hip_regions_derived": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _P(_u64), _P(_u64), _P(_i32), _vp]),
    "exa_hip_regions_read": (None, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_regions_release": (None, [_vp]),
    "exa_hip_regions_stage_ms": (None, [_vp, _vp]),
    "exa_hip_basins": (None, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _i32, _P(_u64), _P(_u64), _P(_u64), _P(_i32), _P(_i32), _vp]),
    "exa_hip_basins_derived": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _f32, _i32, _P(_u64), _P(_u64), _P(_u64), _P(_i32),
                                      _P(_i32), _vp]),
    "exa_hip_basins_read": (None, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_basins_release": (None, [_vp]),
    "exa_hip_basins_stage_ms": (None, [_vp, _vp]),
    "exa_hip_critical_points": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _P(_u64), _vp, _vp]),
    "exa_hip_critical_points_read": (None, [_vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_critical_points_release": (None, [_vp]),
    "exa_hip_critical_points_stage_ms": (None, [_vp, _vp]),
    "exa_hip_profile": (None, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp,
                               _P(ExaHipProfileStats), _vp]),
    "exa_hip_profile_stage_ms": (None, [_vp, _vp]),
    "exa_hip_distance": (None, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_distance_derived": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_distance_mask": (None, [_vp, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_distance_stage_ms": (None, [_vp, _vp]),
    "exa_hip_histogram_ms": (None, [_vp, _P(_f32)]),
    "exa_hip_histogram": (None, [_vp, _i32, _f32, _f32, _i32, _vp, _vp, _vp, _P(ExaHipFieldStats), _vp]),
    "exa_hip_streamlines": (None, [_vp, _vp, _u64, _vp, _f32, _i32, _i32, _P(_u64), _vp]),
    "exa_hip_streamlines_read": (None, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_streamlines_release": (None, [_vp]),
    "exa_hip_streamlines_ms": (None, [_vp, _P(_f32)]),
    "exa_hip_lic": (None, [_vp, _P(ExaHipPlane), _vp, _f32, _i32, _vp, C.c_uint32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_lic_ms": (None, [_vp, _P(_f32)]),
    "exa_hip_flowmap": (None, [_vp, _vp, _vp, _vp, _vp, _f32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_flowmap_ms": (None, [_vp, _vp]),
    "exa_hip_project": (None, [_vp, _P(ExaHipRays), _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_project_ms": (None, [_vp, _P(_f32)]),
    "exa_hip_raycast_iso": (None, [_vp, _P(ExaHipRays), _i32, _f32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_raycast_iso_ms": (None, [_vp, _P(_f32)]),
    "exa_hip_sample_triangles": (None, [_vp, _vp, _u64, _vp, _u64, _vp, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp]),
    "exa_hip_sample_triangles_ms": (None, [_vp, _P(_f32)]),
}
ABI_SYMBOLS = list(_ABI)

_lib = None


def lib():
    """load libexa_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            # not built yet: try to build the HIP module (hipcc cross-compiles without a GPU); never a CPU fallback
            import subprocess
            try:
                subprocess.check_call(["make", "-C", os.path.join(_HERE, "csrc"), "-s", "-j6"])
            except Exception as e:  # noqa: BLE001
                raise RuntimeError(f"{LIB_PATH} not found and building it failed ({e}); run "
                                   "__graft_entry__.build(); there is no CPU fallback") from e
        L = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in _ABI.items():
            fn = getattr(L, name)
            if restype is not None:
                fn.restype = restype
            if argtypes is not None:
                fn.argtypes = argtypes
        _lib = L
    return _lib


def cube_records(bricks, leaflist, begin_alt=None):
    """the cube records the module builds for a scene whose bricks are all cubes of one power-of-two edge
    (exa_prep_cube_records, a diagnostic): (k, records [n,4] uint32) with k = log2 of the edge, or (0, None) when the scene
    is no cube scene.  bricks: BRICK_DTYPE array; leaflist: int32 brick indices; begin_alt: the `begin` values of the other
    brick order, held to the same conditions."""
    bricks = np.ascontiguousarray(bricks, dtype=BRICK_DTYPE)
    leaflist = np.ascontiguousarray(leaflist, dtype=np.int32)
    alt = None if begin_alt is None else np.ascontiguousarray(begin_alt, dtype=np.uint32)
    assert alt is None or alt.size == bricks.size
    k = C.c_int32(-1)
    rec = np.zeros((leaflist.size, 4), dtype=np.uint32)
    if lib().exa_prep_cube_records(bricks.ctypes.data, bricks.size, leaflist.ctypes.data if leaflist.size else None, leaflist.size,
                                   None if alt is None else alt.ctypes.data, C.byref(k), rec.ctypes.data if rec.size else None):
        raise RuntimeError(lib().exa_prep_last_error().decode())
    return (int(k.value), rec) if k.value else (0, None)


class Prep:
    """host data preparation of the OptixRenderer constructor (exa_prep_*)."""

    def __init__(self, scene, num_region_fields=None, num_threads=0, allow_empty_cells=False):
        """allow_empty_cells: the reference's build option ALLOW_EMPTY_CELLS (cell id -1 = no cell, EXA_PREP_ALLOW_EMPTY_CELLS)"""
        L = lib()
        self.bricks7 = np.ascontiguousarray(scene.bricks7, dtype=np.int32).reshape(-1, 7)
        self.cellIDs = np.ascontiguousarray(scene.cellIDs, dtype=np.int32)
        self.fields = [np.ascontiguousarray(f, dtype=np.float32) for f in scene.fields]
        nf = len(self.fields)
        ptrs = (C.c_void_p * max(nf, 1))(*[f.ctypes.data for f in self.fields])
        lens = (C.c_uint64 * max(nf, 1))(*[f.size for f in self.fields])
        self.h = C.c_void_p()
        rc = L.exa_prep_create_ex(self.bricks7.ctypes.data, self.bricks7.shape[0], self.cellIDs.ctypes.data,
                                  self.cellIDs.size, ptrs, lens, nf,
                                  nf if num_region_fields is None else num_region_fields, num_threads,
                                  1 if allow_empty_cells else 0, C.byref(self.h))
        if rc:
            raise RuntimeError(L.exa_prep_last_error().decode())
        self.scene = ExaHipScene()
        L.exa_prep_scene(self.h, C.byref(self.scene))
        self.num_fields = nf

    def _arr(self, ptr, count, dtype):
        if count == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype)

    def bricks(self):
        return self._arr(self.scene.bricks, self.scene.numBricks, BRICK_DTYPE)

    def regions(self):
        return self._arr(self.scene.regions, self.scene.numRegions, REGION_DTYPE)

    def leaflist(self):
        return self._arr(self.scene.leafList, self.scene.leafListSize, np.int32)

    def scalars(self):
        return self._arr(self.scene.scalars, self.scene.numFields * self.scene.totalCells, np.float32)

    def kd_nodes(self):
        return self._arr(self.scene.kdNodes, self.scene.numKdNodes, KDNODE_DTYPE)

    def ropes(self):
        """leaves and neighbour links of the rope walk as the module builds them (exa_prep_ropes, a diagnostic):
        dict(boxes [n,6], links [n,6], region [n], nodes (KDNODE_DTYPE), flags)"""
        nl, nn, flags = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        if lib().exa_prep_ropes(self.h, C.byref(nl), C.byref(nn), None, None, None, None, None):
            raise RuntimeError(lib().exa_prep_last_error().decode())
        boxes = np.zeros((nl.value, 6), dtype=np.float32)
        links = np.zeros((nl.value, 6), dtype=np.int32)
        region = np.zeros(nl.value, dtype=np.int32)
        nodes = np.zeros(max(1, nn.value), dtype=KDNODE_DTYPE)
        if lib().exa_prep_ropes(self.h, C.byref(nl), C.byref(nn), boxes.ctypes.data, links.ctypes.data, region.ctypes.data,
                                nodes.ctypes.data, C.byref(flags)):
            raise RuntimeError(lib().exa_prep_last_error().decode())
        return dict(boxes=boxes, links=links, region=region, nodes=nodes[:nn.value], flags=int(flags.value))

    def set_kd_tree(self, nodes, root):
        """replace the region kd-tree (KDNODE_DTYPE array, root reference) by a caller's own, as a caller may hand the module its
        own tree in ExaHipScene.kdNodes: ropes() and a Renderer made from this prep then see it"""
        nodes = np.ascontiguousarray(nodes, dtype=KDNODE_DTYPE)
        if lib().exa_prep_set_kd_tree(self.h, nodes.ctypes.data if len(nodes) else None, len(nodes), int(root)):
            raise RuntimeError(lib().exa_prep_last_error().decode())
        lib().exa_prep_scene(self.h, C.byref(self.scene))

    def voxel_bounds(self):
        return (np.array(self.scene.voxelBounds_lo, dtype=np.float32),
                np.array(self.scene.voxelBounds_hi, dtype=np.float32))

    def close(self):
        if getattr(self, "h", None):
            lib().exa_prep_destroy(self.h)
            self.h = None

    __del__ = close


class Renderer:
    """Python mirror of exa::OptixRenderer's public methods over the C ABI."""

    def __init__(self, prep, device=0, multiFieldDvr=True, devices=None):
        """devices: a list of device indices -> one handle that drives all of them (exa_hip_create_multi)"""
        L = lib()
        self.prep = prep
        self.h = C.c_void_p()
        if devices is not None:
            arr = (C.c_int32 * len(devices))(*devices)
            rc = L.exa_hip_create_multi(C.byref(prep.scene), arr, len(devices), C.byref(self.h))
        else:
            rc = L.exa_hip_create(C.byref(prep.scene), device, C.byref(self.h))
        if rc:
            raise RuntimeError(L.exa_hip_last_error(None).decode())
        self.numFields = prep.num_fields
        self.frameState = ExaHipFrameState()
        self.frameState.xfm_vx[0] = self.frameState.xfm_vy[1] = self.frameState.xfm_vz[2] = 1.0
        self.frameState.ao.length, self.frameState.ao.enabled = 1e20, 1   # FrameState.h:55-58 defaults
        self.frameState.xfOpacityScale = 1.0
        for i in range(MAX_CONTOUR):
            self.frameState.contour[i].normal[0] = 1.0
            self.frameState.contour[i].offset = 0.5
        nprim = self.numFields if multiFieldDvr else 1
        self.params = ExaHipParams(0.5, nprim, 0 if (multiFieldDvr or self.numFields < 2) else 1, 1, 1, nprim, 1)
        self.doSpaceSkipping = True
        self.fbSize = (0, 0)
        self.voxelSpaceBounds = prep.voxel_bounds()
        # the last extraction of each family, for the read that follows it
        self._iso_counts, self._stream_counts = _IsoMesh(0, 0, False), _StreamLines(0, 0, False)
        self._isolines = self._regions = self._basins = self._critical = None

    def _check(self, rc):
        if rc:
            raise RuntimeError(lib().exa_hip_last_error(self.h).decode())

    def _ms(self, getter):
        """the float that one of the `float *ms` getters reports"""
        ms = C.c_float(0)
        self._check(getter(self.h, C.byref(ms)))
        return float(ms.value)

    def _stage_ms(self, getter, n):
        """the n floats that one of the `float ms[n]` getters reports"""
        ms = (C.c_float * n)()
        self._check(getter(self.h, ms))
        return [float(v) for v in ms]

    def _field_call(self, of_channel, of_derived, head, channel, quantity, channels, tail):
        """the return code of of_channel(handle, *head, channel, *tail) or, with a quantity, of its _derived form
        of_derived(handle, *head, channels, quantity, *tail)"""
        if quantity is None:
            return of_channel(self.h, *head, int(channel), *tail)
        return of_derived(self.h, *head, _i3(channels), derived_quantity(quantity), *tail)

    def _refused_read(self, read, pointers, method):
        """a read with no extraction of this renderer behind it: all null, for the module to refuse"""
        self._check(read(self.h, *[None] * pointers, 0, None))
        raise RuntimeError(f"{method}: no extraction of this renderer to read")

    @staticmethod
    def _one_shot(read, release):
        """what read() returns of the extraction just made, which is released even if the read raises"""
        try:
            return read()
        finally:
            release()

    def close(self):
        if getattr(self, "h", None):
            lib().exa_hip_destroy(self.h)
            self.h = None

    __del__ = close

    # ---- OptixRenderer method set (exa/OptixRenderer.h:38-79) ----
    def setVoxelSpaceTransform(self, vx, vy, vz, p):
        for i in range(3):
            self.frameState.xfm_vx[i], self.frameState.xfm_vy[i] = float(vx[i]), float(vy[i])
            self.frameState.xfm_vz[i], self.frameState.xfm_p[i] = float(vz[i]), float(p[i])

    def resizeFrameBuffer(self, fbSize):
        self.fbSize = (int(fbSize[0]), int(fbSize[1]))
        self._check(lib().exa_hip_resize(self.h, *self.fbSize))

    def updateIsoValues(self, isoValues, channels, enabled):
        for i in range(MAX_ISO):
            self.frameState.iso[i].value = float(isoValues[i])
            self.frameState.iso[i].channel = int(channels[i])
            self.frameState.iso[i].enabled = int(enabled[i])

    # ---- streamline tracer (OptixRenderer::setTracerEnabled / resetTracer / advanceTracer) ----
    def resetTracer(self, seeds, channels=(0, 1, 2), numTimesteps=100, steplen=1e-6, enabled=True):
        sd = np.ascontiguousarray(seeds, dtype=np.float32).reshape(-1, 3)
        self._tracer = ExaHipTracer(int(enabled), _i3(channels), sd.shape[0], int(numTimesteps), float(steplen))
        self._check(lib().exa_hip_reset_tracer(self.h, C.byref(self._tracer), sd.ctypes.data))

    def setTracerEnabled(self, enable):
        self._check(lib().exa_hip_set_tracer_enabled(self.h, int(bool(enable))))

    def advanceTracer(self):
        r = C.c_int32(0)
        self._check(lib().exa_hip_advance_tracer(self.h, C.byref(r)))
        return bool(r.value)

    def readTraces(self):
        out = np.zeros((self._tracer.numTraces, self._tracer.numTimesteps, 3), dtype=np.float32)
        self._check(lib().exa_hip_read_traces(self.h, out.ctypes.data))
        return out

    def setTriangles(self, verts, tris):
        """the `surfaces` argument of the OptixRenderer constructor, all meshes concatenated"""
        v = np.ascontiguousarray(verts, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(tris, dtype=np.int32).reshape(-1, 3)
        self._check(lib().exa_hip_set_triangles(self.h, v.ctypes.data, v.shape[0], t.ctypes.data, t.shape[0]))

    def updateContourPlanes(self, normals, offsets, channels, enabled):
        for i in range(MAX_CONTOUR):
            n = np.asarray(normals[i], dtype=np.float32)
            n = (n * (np.float32(1.0) / np.sqrt(np.dot(n, n), dtype=np.float32))).astype(np.float32)   # normalize() (:511)
            for k in range(3):
                self.frameState.contour[i].normal[k] = float(n[k])
            self.frameState.contour[i].offset = float(offsets[i])
            self.frameState.contour[i].channel = int(channels[i])
            self.frameState.contour[i].enabled = int(enabled[i])

    def updateCamera(self, pos, dir00, dirDu, dirDv):
        for i in range(3):
            self.frameState.cam_pos[i], self.frameState.cam_dir00[i] = float(pos[i]), float(dir00[i])
            self.frameState.cam_dirDu[i], self.frameState.cam_dirDv[i] = float(dirDu[i]), float(dirDv[i])

    def updateXF(self, chan, opacities, colorMap, xfDomain, xfOpacityScale=0.1):
        colorMap = np.asarray(colorMap, dtype=np.float32)
        if colorMap.shape[0] != NUM_XF_VALUES:
            raise RuntimeError("mismatching xf size!?")          # OptixRenderer.cpp:382-383
        lut = np.concatenate([colorMap[:, :3], np.asarray(opacities, dtype=np.float32).reshape(-1, 1)], axis=1)
        lut = np.ascontiguousarray(lut, dtype=np.float32)
        self.frameState.xfDomain[chan][0], self.frameState.xfDomain[chan][1] = float(xfDomain[0]), float(xfDomain[1])
        self.frameState.xfOpacityScale = float(xfOpacityScale)
        self._check(lib().exa_hip_set_xf(self.h, chan, lut.ctypes.data))

    def updateFrameID(self, frameID):
        self.frameState.frameID = int(frameID)

    def updateDt(self, dt):
        self.params.dt = float(dt)

    def setSpaceSkipping(self, enable):
        self.doSpaceSkipping = bool(enable)

    def setGradientShadingDVR(self, enable):
        self.params.gradientShadingDVR = int(bool(enable))

    def setGradientShadingISO(self, enable):
        self.params.gradientShadingISO = int(bool(enable))

    def setShard(self, rank, world):
        self._check(lib().exa_hip_set_shard(self.h, rank, world))

    def setOption(self, key, value):
        self._check(lib().exa_hip_set_option(self.h, key.encode(), int(value)))

    def _push_state(self):
        contour = any(self.frameState.contour[i].enabled for i in range(MAX_CONTOUR))
        self.params.spaceSkippingEnabled = int((not contour) and self.doSpaceSkipping)  # OptixRenderer.cpp:418-432
        self._check(lib().exa_hip_set_frame_state(self.h, C.byref(self.frameState)))
        self._check(lib().exa_hip_set_params(self.h, C.byref(self.params)))

    def outputPixels(self):
        return int(lib().exa_hip_output_pixels(self.h))

    def render(self, device_ptr=None, stream=None, async_=False):
        """OptixRenderer::render().  Without device_ptr returns the colour buffer as a
        numpy array ([H,W] uint32 for a whole frame, flat tile-major for a shard)."""
        self._push_state()
        if device_ptr is not None:
            self._check(lib().exa_hip_render(self.h, C.c_void_p(device_ptr), 1, C.c_void_p(stream or 0), int(async_)))
            return None
        n = self.outputPixels()
        out = np.zeros(n, dtype=np.uint32)
        self._check(lib().exa_hip_render(self.h, out.ctypes.data, 0, None, 0))
        W, H = self.fbSize
        return out.reshape(H, W) if n == W * H else out

    def renderStats(self):
        self._push_state()
        n = self.outputPixels()
        out = np.zeros(n, dtype=np.uint32)
        st = ExaHipStats()
        self._check(lib().exa_hip_render_stats(self.h, out.ctypes.data, 0, C.byref(st)))
        W, H = self.fbSize
        return (out.reshape(H, W) if n == W * H else out), st.asdict()

    def stats(self):
        st = ExaHipStats()
        self._check(lib().exa_hip_get_stats(self.h, C.byref(st)))
        return st.asdict()

    def readAccum(self):
        n = self.outputPixels()
        out = np.zeros((n, 4), dtype=np.float32)
        self._check(lib().exa_hip_read_accum(self.h, out.ctypes.data))
        W, H = self.fbSize
        return out.reshape(H, W, 4) if n == W * H else out

    def writeAccum(self, accum):
        a = np.ascontiguousarray(accum, dtype=np.float32)
        self._check(lib().exa_hip_write_accum(self.h, a.ctypes.data))

    def readActivity(self, which=0):
        self._push_state()
        out = np.zeros(self.prep.scene.numRegions, dtype=np.uint8)
        self._check(lib().exa_hip_read_activity(self.h, which, out.ctypes.data))
        return out

    def untile(self, gathered_ptr, shard_stride, world, out_ptr, stream=None):
        self._check(lib().exa_hip_untile(self.h, C.c_void_p(gathered_ptr), shard_stride, world,
                                         C.c_void_p(out_ptr), C.c_void_p(stream or 0)))

    # ---- point probes (exa_hip_sample_points / exa_hip_resample; include/exa_hip.h states the contract) ----
    def _probe_world(self, world):
        if world:                       # the voxelSpaceTransform lives in the frame state the module holds
            self._push_state()
        return SAMPLE_WORLD_SPACE if world else 0

    def samplePoints(self, points, channels=(0,), gradient=False, normalized=False, world=False, fill=float("nan"),
                     stream=None, async_=False):
        """the reconstructed field at points [n,3] (voxel space, or world space with world=True).  Returns
        (values [n, len(channels)], gradients [n, len(channels), 3] or None, status [n, len(channels)]): status = region id,
        -1 outside every region, -2 where the basis weights vanish; value and gradient are `fill` where status < 0.
        gradient: the reference's numerator sumW*sumD - sumWV*sumDC, its derivative weights in each brick's own cell units
        (no voxel-space vector where bricks are coarse or of several levels); normalized: the gradient of sumWV/sumW with
        respect to the voxel-space position (derivative weights times each brick's 2^-level, divided by sumW^2),
        both with respect to voxel-space coordinates.  A numpy array takes the host path; a contiguous float32 torch CUDA
        tensor (memory of the handle's first device) the device path, with torch tensors out (async_ on `stream`)."""
        chans = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
        flags = self._probe_world(world) | (SAMPLE_GRADIENT if gradient or normalized else 0)
        flags |= SAMPLE_GRADIENT_NORMALIZED if normalized else 0
        k = chans.size
        empty, ptr, device = _like(points)
        pts, n = _rows3(points, np.float32, device, "points: a contiguous float32 tensor [n, 3]")
        values = empty((n, k), np.float32)
        grads = empty((n, k, 3), np.float32) if flags & SAMPLE_GRADIENT else None
        status = empty((n, k), np.int32)
        self._check(lib().exa_hip_sample_points(self.h, ptr(pts), n, chans.ctypes.data, k, flags, float(fill), ptr(values),
                                                ptr(grads), ptr(status), *_target(device, stream, async_)))
        return values, grads, status

    def resample(self, lo, hi, dims, channel=0, world=False, fill=float("nan"), out_ptr=None, stream=None, async_=False):
        """the field at the cell centres of a uniform dims[0] x dims[1] x dims[2] grid over the box [lo, hi] (voxel space, or
        world space with world=True).  Without out_ptr returns a float32 array [nz, ny, nx] (x fastest); out_ptr (a device
        pointer or a contiguous float32 torch CUDA tensor) takes the device path and returns None."""
        flags = self._probe_world(world)
        out, dest = _lattice_out(dims, (), out_ptr, stream, async_)
        self._check(lib().exa_hip_resample(self.h, _f3(lo), _f3(hi), _i3(dims), int(channel), flags, float(fill), *dest))
        return out

    # ---- iso-surface extraction (exa_hip_isosurface*; include/exa_hip.h states the contract) ----
    def extractIsoSurface(self, lo, hi, dims, iso, channel=0, world=False, gradients=False, stream=None):
        """extract the surface field == iso on the lattice of resample(lo, hi, dims) into module-owned device memory;
        returns (numVertices, numTriangles).  readIsoSurface copies it out, releaseIsoSurface frees it."""
        return self._extract_iso(lo, hi, dims, iso, channel, None, None, world, gradients, stream)

    def _extract_iso(self, lo, hi, dims, iso, channel, quantity, channels, world, gradients, stream):
        """extractIsoSurface of a channel or of a derived quantity, whose mesh has no gradients.  A call that fails leaves
        the state as it was: the module then has no mesh, and refuses the read that state asks for"""
        flags = self._probe_world(world) | (SAMPLE_GRADIENT if gradients else 0)
        nv, nt = C.c_uint64(0), C.c_uint64(0)
        self._check(self._field_call(lib().exa_hip_isosurface, lib().exa_hip_isosurface_derived, (_f3(lo), _f3(hi), _i3(dims)),
                                     channel, quantity, channels,
                                     (float(iso), flags, C.byref(nv), C.byref(nt), C.c_void_p(stream or 0))))
        self._iso_counts = _IsoMesh(int(nv.value), int(nt.value), bool(gradients) and quantity is None)
        return self._iso_counts[:2]

    def readIsoSurface(self):
        """(verts float32 [n,3], tris int32 [m,3], grads float32 [n,3] or None) of the last extractIsoSurface"""
        mesh = self._iso_counts
        verts = np.empty((mesh.vertices, 3), dtype=np.float32)
        tris = np.empty((mesh.triangles, 3), dtype=np.int32)
        grads = np.empty((mesh.vertices, 3), dtype=np.float32) if mesh.gradients else None
        self._check(lib().exa_hip_isosurface_read(self.h, verts.ctypes.data, _host_ptr(grads), tris.ctypes.data, 0, None))
        return verts, tris, grads

    def releaseIsoSurface(self):
        self._check(lib().exa_hip_isosurface_release(self.h))
        self._iso_counts = _IsoMesh(0, 0, False)

    def isoSurfaceStageMs(self):
        """device ms of the last extraction's stages: lattice values, cube pass, point pass, scans, emit, gradients"""
        return self._stage_ms(lib().exa_hip_isosurface_stage_ms, 6)

    def isosurface(self, lo, hi, dims, iso, channel=0, world=False, gradients=False):
        """the iso-surface field == iso of `channel` on the lattice of resample(lo, hi, dims), by marching tetrahedra:
        (verts float32 [n,3] in the space of lo / hi, tris int32 [m,3], grads float32 [n,3] or None).  grads: what
        samplePoints(verts, gradient=True, normalized=True) gives; the shading normal is -grad/|grad|.  The device copy
        is released before returning."""
        self.extractIsoSurface(lo, hi, dims, iso, channel=channel, world=world, gradients=gradients)
        return self._one_shot(self.readIsoSurface, self.releaseIsoSurface)

    # ---- derived flow quantities (exa_hip_*_derived; include/exa_hip.h states the contract) ----
    def sampleDerived(self, points, quantity, channels=(0, 1, 2), world=False, fill=float("nan"), stream=None, async_=False):
        """a quantity of the velocity gradient tensor of the vector field `channels` at points [n,3]: `quantity` by name (a
        key of DERIVED) or number.  Returns (out [n], or [n, 3] for vorticity; status [n]).  Voxel-space quantities, also
        for world-space positions.  A numpy array takes the host path, a contiguous float32 torch CUDA tensor the device
        path with torch tensors out (async_ on `stream`), as samplePoints."""
        q = derived_quantity(quantity)
        k = DERIVED_COMPONENTS.get(q, 1)                                       # the module checks the quantity
        flags, ch3 = self._probe_world(world), _i3(channels)
        empty, ptr, device = _like(points)
        pts, n = _rows3(points, np.float32, device, "points: a contiguous float32 tensor [n, 3]")
        out = empty((n, k), np.float32)
        status = empty((n,), np.int32)
        self._check(lib().exa_hip_sample_derived(self.h, ptr(pts), n, ch3, q, flags, float(fill), ptr(out), ptr(status),
                                                 *_target(device, stream, async_)))
        return (out if k == 3 else out.reshape(n)), status

    def resampleDerived(self, lo, hi, dims, quantity, channels=(0, 1, 2), world=False, fill=float("nan"), out_ptr=None,
                        stream=None, async_=False):
        """the quantity on the lattice of resample(lo, hi, dims): a float32 array [nz, ny, nx], or [nz, ny, nx, 3] for
        vorticity; out_ptr (a device pointer or a contiguous float32 torch CUDA tensor) takes the device path and returns
        None."""
        q = derived_quantity(quantity)
        k = DERIVED_COMPONENTS.get(q, 1)
        flags = self._probe_world(world)
        out, dest = _lattice_out(dims, (3,) if k == 3 else (), out_ptr, stream, async_)
        self._check(lib().exa_hip_resample_derived(self.h, _f3(lo), _f3(hi), _i3(dims), _i3(channels), q, flags, float(fill), *dest))
        return out

    def extractIsoSurfaceDerived(self, lo, hi, dims, iso, quantity, channels=(0, 1, 2), world=False, gradients=False,
                                 stream=None):
        """extractIsoSurface on the lattice of resampleDerived(lo, hi, dims, quantity, channels): (numVertices, numTriangles).
        One-component quantities only; gradients=True is refused by the module."""
        return self._extract_iso(lo, hi, dims, iso, None, quantity, channels, world, gradients, stream)

    def isosurfaceDerived(self, lo, hi, dims, iso, quantity, channels=(0, 1, 2), world=False):
        """the iso-surface quantity == iso on the lattice of resampleDerived(lo, hi, dims, quantity, channels), as isosurface:
        (verts float32 [n,3], tris int32 [m,3]).  The device copy is released before returning."""
        self.extractIsoSurfaceDerived(lo, hi, dims, iso, quantity, channels=channels, world=world)
        return self._one_shot(self.readIsoSurface, self.releaseIsoSurface)[:2]

    # ---- contour lines on a plane lattice (exa_hip_isolines*; include/exa_hip.h states the contract) ----
    def extractIsolines(self, origin, du, dv, size, isos, channel=0, world=False, gradients=False, values=False, quantity=None,
                        channels=(0, 1, 2), stream=None):
        """extract the lines field == iso, for every iso of `isos`, on the plane lattice of size = (nu, nv) whose point (i, j)
        lies at origin + (i + 0.5) du + (j + 0.5) dv, into module-owned device memory; with a `quantity` the lines of that
        derived quantity of `channels`.  Returns (numVertices, numSegments).  readIsolines copies the result out,
        releaseIsolines frees it."""
        flags = self._probe_world(world) | (SAMPLE_GRADIENT if gradients else 0) | (ISOLINES_KEEP_VALUES if values else 0)
        plane = ExaHipPlane(_f3(origin), _f3(du), _f3(dv), int(size[0]), int(size[1]))
        levels = np.ascontiguousarray(isos, dtype=np.float32).reshape(-1)
        nv, ns = C.c_uint64(0), C.c_uint64(0)
        self._isolines = None
        self._check(self._field_call(lib().exa_hip_isolines, lib().exa_hip_isolines_derived, (C.byref(plane),), channel, quantity,
                                     channels, (levels.ctypes.data, len(levels), flags, C.byref(nv), C.byref(ns),
                                                C.c_void_p(stream or 0))))
        self._isolines = _Isolines(int(nv.value), int(ns.value), len(levels), bool(gradients),
                                   (int(size[1]), int(size[0])) if values else None)
        return self._isolines[:2]

    def readIsolines(self):
        """the last extractIsolines as a dict: vertices float32 [V,3], uv float32 [V,2], segments int32 [S,2] (global vertex
        indices), vertex_offsets and segment_offsets uint64 [levels + 1], and gradients float32 [V,3] / values float32
        [nv,nu] where the extraction kept them"""
        kept = self._isolines
        if kept is None:
            self._refused_read(lib().exa_hip_isolines_read, 7, "readIsolines")
        table = (("vertices", (kept.vertices, 3), np.float32), ("uv", (kept.vertices, 2), np.float32),
                 ("gradients", (kept.vertices, 3) if kept.gradients else None, np.float32),
                 ("segments", (kept.segments, 2), np.int32), ("vertex_offsets", (kept.levels + 1,), np.uint64),
                 ("segment_offsets", (kept.levels + 1,), np.uint64), ("values", kept.values_shape, np.float32))
        out = _outputs(table)
        self._check(lib().exa_hip_isolines_read(self.h, *_pointers(table, out), 0, None))
        return out

    def releaseIsolines(self):
        self._check(lib().exa_hip_isolines_release(self.h))
        self._isolines = None

    def isolinesStageMs(self):
        """device ms of the last extraction's stages, summed over the levels: positions and values, square pass, point pass,
        scans, emit, gradients"""
        return self._stage_ms(lib().exa_hip_isolines_stage_ms, 6)

    def isolines(self, origin, du, dv, size, isos, channel=0, world=False, gradients=False, values=False):
        """the contour lines field == iso of `channel`, for every iso of `isos`, on the plane lattice of extractIsolines, by
        marching triangles: the dict of readIsolines.  The >= iso side lies to the left of every segment (u right, v up);
        level l owns vertices[vertex_offsets[l]:vertex_offsets[l+1]] and segments[segment_offsets[l]:segment_offsets[l+1]].
        The device copy is released before returning."""
        self.extractIsolines(origin, du, dv, size, isos, channel=channel, world=world, gradients=gradients, values=values)
        return self._one_shot(self.readIsolines, self.releaseIsolines)

    def isolinesDerived(self, origin, du, dv, size, isos, quantity, channels=(0, 1, 2), world=False, values=False):
        """isolines of a one-component derived quantity (a key of DERIVED, or its number) of the vector field `channels`"""
        self.extractIsolines(origin, du, dv, size, isos, world=world, values=values, quantity=quantity, channels=channels)
        return self._one_shot(self.readIsolines, self.releaseIsolines)

    # ---- connected regions of field >= iso on a lattice (exa_hip_regions*; include/exa_hip.h states the contract) ----
    def extractRegions(self, lo, hi, dims, iso, channel=0, world=False, below=False, faces=False, keep_values=False,
                       quantity=None, channels=(0, 1, 2), stream=None):
        """label the connected regions of field >= iso (below: < iso) on the lattice of resample(lo, hi, dims), joined along
        the Kuhn edges (faces: the axis edges only), into module-owned device memory; with a `quantity` the regions of that
        derived quantity of `channels`.  Returns (numRegions, numInside, sum_exponent).  readRegions copies the result out,
        releaseRegions frees it."""
        flags = self._labelled_flags(world, below, faces, keep_values)
        nr, ni, se = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        self._regions = None
        self._check(self._field_call(lib().exa_hip_regions, lib().exa_hip_regions_derived, (_f3(lo), _f3(hi), _i3(dims)), channel,
                                     quantity, channels, (float(iso), flags, C.byref(nr), C.byref(ni), C.byref(se),
                                                          C.c_void_p(stream or 0))))
        self._regions = _Labelled(int(nr.value), tuple(int(d) for d in dims[::-1]), bool(keep_values),
                                  dict(sum_exponent=int(se.value), num_inside=int(ni.value)))
        return int(nr.value), int(ni.value), int(se.value)

    def _labelled_flags(self, world, below, faces, keep_values):
        """the flags of extractRegions and extractBasins"""
        return (self._probe_world(world) | (REGIONS_BELOW if below else 0) | (REGIONS_FACES if faces else 0)
                | (REGIONS_KEEP_VALUES if keep_values else 0))

    def _read_labelled(self, kept, read, method, dtype, tables):
        """the dict of readRegions and readBasins: labels, one zero-filled table of `dtype` under each key of `tables`, the
        numbers the extraction returned, and the values where it kept them"""
        if kept is None:
            self._refused_read(read, 3, method)
        table = np.zeros(kept.count, dtype)
        out = dict(labels=np.empty(kept.shape, np.int32), **dict.fromkeys(tables, table), **kept.numbers)
        if kept.keep_values:
            out["values"] = np.empty(kept.shape, np.float32)
        self._check(read(self.h, out["labels"].ctypes.data, table.ctypes.data if kept.count else None, _host_ptr(out.get("values")),
                         0, None))
        return out

    def readRegions(self):
        """the last extractRegions as a dict: labels int32 [nz, ny, nx] (the region's number, -1 outside), regions (a
        structured array of LABELLED_REGION_DTYPE, numbered by ascending `first`), sum_exponent, num_inside, and values float32
        [nz, ny, nx] where the extraction kept them"""
        return self._read_labelled(self._regions, lib().exa_hip_regions_read, "readRegions", LABELLED_REGION_DTYPE, ("regions",))

    def releaseRegions(self):
        self._check(lib().exa_hip_regions_release(self.h))
        self._regions = None

    def regionsStageMs(self):
        """device ms of the last extractRegions' stages: values, init, merge, flatten, rank, stats"""
        return self._stage_ms(lib().exa_hip_regions_stage_ms, 6)

    def regions(self, lo, hi, dims, iso, channel=0, world=False, below=False, faces=False, keep_values=False):
        """the connected regions of field >= iso of `channel` on the lattice of resample(lo, hi, dims): the dict of
        readRegions (region_measures turns its table into sums, means, volumes, integrals and centroids).  The device copy
        is released before returning."""
        self.extractRegions(lo, hi, dims, iso, channel=channel, world=world, below=below, faces=faces, keep_values=keep_values)
        return self._one_shot(self.readRegions, self.releaseRegions)

    def regionsDerived(self, lo, hi, dims, iso, quantity, channels=(0, 1, 2), world=False, below=False, faces=False,
                       keep_values=False):
        """regions of a one-component derived quantity (a key of DERIVED, or its number) of the vector field `channels`"""
        self.extractRegions(lo, hi, dims, iso, world=world, below=below, faces=faces, keep_values=keep_values,
                            quantity=quantity, channels=channels)
        return self._one_shot(self.readRegions, self.releaseRegions)

    # ---- profiles and phase plots on a lattice (exa_hip_profile; include/exa_hip.h states the contract) ----
    def profile(self, lo, hi, dims, axes, values=(), weight=None, world=False, minmax=True, stream=None):
        """the points of the lattice of resample(lo, hi, dims) binned by one or two `axes` (uniform(), edges() or, first
        axis only, labels()), with `values` (up to four sources: channel(), derived(), radius(), coordinate()) accumulated
        per bin, weighted by the source `weight` if given.  Returns a dict: count uint64 [B...], sum_weight int64 [B...] or
        None, sums int64 [numValues, B...], mins / maxs float32 [numValues, B...] or None (minmax=False), stats (the dict of
        ExaHipProfileStats) — B... is (numBins,) or (numBins1, numBins0), the first axis fastest.  profile_measures turns
        the fixed-point sums into sums, means and volumes."""
        if isinstance(axes, ProfileAxis):
            axes = (axes,)
        axes, values = tuple(axes), tuple(values)
        ax = (ExaHipProfileAxis * max(1, len(axes)))(*[a.struct for a in axes])
        flags = self._probe_world(world) | (PROFILE_LABELS_DEVICE if any(a.device for a in axes) else 0)
        shape = tuple(int(a.struct.numBins) for a in axes[:2])[::-1]
        bins = int(np.prod(shape, dtype=np.int64)) if shape else 0
        nv = len(values)
        room = bins if 0 < bins <= PROFILE_MAX_BINS and all(n > 0 for n in shape) else 0     # a refused call writes nothing
        vals = (ExaHipSource * max(1, nv))(*values)
        count = np.zeros(room, np.uint64)
        sum_weight = np.zeros(room, np.int64) if weight is not None else None
        sums = np.zeros((nv, room), np.int64)
        mins, maxs = (np.zeros((nv, room), np.float32), np.zeros((nv, room), np.float32)) if minmax else (None, None)
        st, ptr = ExaHipProfileStats(), _host_ptr
        self._check(lib().exa_hip_profile(self.h, _f3(lo), _f3(hi), _i3(dims), flags, ax, len(axes), vals if nv else None, nv,
                                          C.byref(weight) if weight is not None else None, ptr(count), ptr(sum_weight),
                                          ptr(sums) if nv else None, ptr(mins), ptr(maxs), C.byref(st), C.c_void_p(stream or 0)))
        grid = lambda a: a.reshape(a.shape[:-1] + shape) if a is not None else None           # noqa: E731
        return dict(count=grid(count), sum_weight=grid(sum_weight), sums=grid(sums), mins=grid(mins), maxs=grid(maxs),
                    stats=st.asdict(), weighted=weight is not None)

    def profileStageMs(self):
        """device ms of the last profile's stages: values, classify, accumulate, finish"""
        return self._stage_ms(lib().exa_hip_profile_stage_ms, 4)

    # ---- basins: one per peak of field >= iso, merged by depth (exa_hip_basins*; include/exa_hip.h states the contract) ----
    def extractBasins(self, lo, hi, dims, iso, min_depth, channel=0, world=False, below=False, faces=False, keep_values=False,
                      quantity=None, channels=(0, 1, 2), stream=None):
        """the basins of field >= iso (below: of the minima of < iso) on the lattice of resample(lo, hi, dims): every inside
        point goes to the peak it climbs to, peaks that stand out of their highest pass by less than min_depth are merged
        across it; into module-owned device memory.  With a `quantity` the basins of that derived quantity of `channels`.
        Returns (numBasins, numRawBasins, numInside, sum_exponent, rounds).  readBasins copies the result out, releaseBasins
        frees it."""
        flags = self._labelled_flags(world, below, faces, keep_values)
        nb, nr, ni, se, rounds = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0), C.c_int32(0)
        self._basins = None
        self._check(self._field_call(lib().exa_hip_basins, lib().exa_hip_basins_derived, (_f3(lo), _f3(hi), _i3(dims)), channel,
                                     quantity, channels, (float(iso), float(min_depth), flags, C.byref(nb), C.byref(nr), C.byref(ni),
                                                          C.byref(se), C.byref(rounds), C.c_void_p(stream or 0))))
        self._basins = _Labelled(int(nb.value), tuple(int(d) for d in dims[::-1]), bool(keep_values),
                                 dict(sum_exponent=int(se.value), num_inside=int(ni.value), num_raw=int(nr.value),
                                      rounds=int(rounds.value)))
        return int(nb.value), int(nr.value), int(ni.value), int(se.value), int(rounds.value)

    def readBasins(self):
        """the last extractBasins as a dict: the keys of readRegions (labels int32 [nz, ny, nx], the basin's number or -1;
        sum_exponent; num_inside; values where kept) with the table under `regions` and under `basins` (a structured array of
        BASIN_DTYPE, numbered by ascending lattice index of the peak), num_raw and rounds"""
        return self._read_labelled(self._basins, lib().exa_hip_basins_read, "readBasins", BASIN_DTYPE, ("regions", "basins"))

    def releaseBasins(self):
        self._check(lib().exa_hip_basins_release(self.h))
        self._basins = None

    def basinsStageMs(self):
        """device ms of the last extractBasins' stages: values, ascent, passes, links, rank, stats"""
        return self._stage_ms(lib().exa_hip_basins_stage_ms, 6)

    def basins(self, lo, hi, dims, iso, min_depth, channel=0, world=False, below=False, faces=False, keep_values=False):
        """the basins of field >= iso of `channel` on the lattice of resample(lo, hi, dims): the dict of readBasins
        (region_measures reads its table as it reads that of regions).  The device copy is released before returning."""
        self.extractBasins(lo, hi, dims, iso, min_depth, channel=channel, world=world, below=below, faces=faces,
                           keep_values=keep_values)
        return self._one_shot(self.readBasins, self.releaseBasins)

    def basinsDerived(self, lo, hi, dims, iso, min_depth, quantity, channels=(0, 1, 2), world=False, below=False, faces=False,
                      keep_values=False):
        """basins of a one-component derived quantity (a key of DERIVED, or its number) of the vector field `channels`"""
        self.extractBasins(lo, hi, dims, iso, min_depth, world=world, below=below, faces=faces, keep_values=keep_values,
                           quantity=quantity, channels=channels)
        return self._one_shot(self.readBasins, self.releaseBasins)

    # ---- critical points of a flow on a lattice (exa_hip_critical_points*; include/exa_hip.h states the contract) ----
    def extractCriticalPoints(self, lo, hi, dims, channels=(0, 1, 2), iterations=8, tolerance=2.0 ** -10, world=False, probe=False,
                              stream=None):
        """find and classify the zeros of the vector field `channels` on the lattice of resample(lo, hi, dims), one per cell at
        the most, into module-owned device memory.  Returns (numPoints, stats dict of CRITICAL_STATS).  readCriticalPoints
        copies the result out, releaseCriticalPoints frees it."""
        flags = self._probe_world(world) | (CRITICAL_PROBE if probe else 0)
        n, st = C.c_uint64(0), (C.c_uint64 * len(CRITICAL_STATS))()
        self._critical = None
        self._check(lib().exa_hip_critical_points(self.h, _f3(lo), _f3(hi), _i3(dims), _i3(channels), int(iterations), float(tolerance),
                                                  flags, C.byref(n), st, C.c_void_p(stream or 0)))
        self._critical = _Critical(int(n.value), bool(probe))
        return int(n.value), dict(zip(CRITICAL_STATS, (int(v) for v in st)))

    def readCriticalPoints(self):
        """the last extractCriticalPoints: (points, a structured array of CRITICAL_POINT_DTYPE in ascending cell number; probe
        float32 [n, 3, 4] = value and voxel-space gradient of each channel at each position, or None; probe_status int32 [n, 3]
        or None)"""
        kept = self._critical
        if kept is None:
            self._refused_read(lib().exa_hip_critical_points_read, 3, "readCriticalPoints")
        n = kept.points
        points = np.zeros(n, CRITICAL_POINT_DTYPE)
        probe = np.empty((n, 3, 4), np.float32) if kept.probe else None
        status = np.empty((n, 3), np.int32) if kept.probe else None
        self._check(lib().exa_hip_critical_points_read(self.h, *[_host_ptr(a) if n else None for a in (points, probe, status)],
                                                       0, None))
        return points, probe, status

    def releaseCriticalPoints(self):
        self._check(lib().exa_hip_critical_points_release(self.h))
        self._critical = None

    def criticalPointsStageMs(self):
        """device ms of the last extractCriticalPoints' stages: values, cells, scans, refine, emit, probe"""
        return self._stage_ms(lib().exa_hip_critical_points_stage_ms, 6)

    def criticalPoints(self, lo, hi, dims, channels=(0, 1, 2), iterations=8, tolerance=2.0 ** -10, world=False, probe=False):
        """the critical points of the vector field `channels` on the lattice of resample(lo, hi, dims): (points, stats), with
        probe=True (points, stats, probe, probe_status) as readCriticalPoints gives them.  type & 3 is n+, the eigenvalues with
        a positive real part; CRITICAL names the other bits.  The device copy is released before returning."""
        _, stats = self.extractCriticalPoints(lo, hi, dims, channels=channels, iterations=iterations, tolerance=tolerance,
                                              world=world, probe=probe)
        points, values, status = self._one_shot(self.readCriticalPoints, self.releaseCriticalPoints)
        return (points, stats, values, status) if probe else (points, stats)

    def derivedMs(self):
        """device ms of the kernels of the last sampleDerived / resampleDerived call, summed"""
        return self._ms(lib().exa_hip_derived_ms)

    # ---- histogram and value range of a channel's cells (exa_hip_histogram; include/exa_hip.h states the contract) ----
    def histogram(self, channel, lo, hi, bins, box=None, volume=True, stream=None):
        """the exact histogram of the cell values of `channel` over [lo, hi] in `bins` bins: (cells uint64 [bins], volume
        uint64 [bins] or None, stats dict).  cells counts cell slots, volume weights a level-L cell with 8^L finest voxels;
        box = (lo.xyz, hi.xyz) in integer voxel coordinates restricts both to the cells whose centre lies in it.  bins = 0
        is the range-only pass (fieldStats)."""
        bins = int(bins)
        n = min(max(bins, 0), HIST_MAX_BINS)                                   # the module checks bins
        cells = np.zeros(n, dtype=np.uint64)
        vol = np.zeros(n, dtype=np.uint64) if volume else None
        b6 = (C.c_int32 * 6)(*[int(v) for v in box]) if box is not None else None
        st = ExaHipFieldStats()
        self._check(lib().exa_hip_histogram(self.h, int(channel), float(lo), float(hi), bins, b6, cells.ctypes.data,
                                            vol.ctypes.data if volume else None, C.byref(st), C.c_void_p(stream or 0)))
        return cells, vol, st.asdict()

    def histogramMs(self):
        """device ms of the last histogram / fieldStats call's kernel"""
        return self._ms(lib().exa_hip_histogram_ms)

    def fieldStats(self, channel, box=None):
        """value range (min, max), cell counts per level and the NaN / empty counts of `channel`, optionally inside a box: the
        stats dict of the range-only pass"""
        return self.histogram(channel, 0.0, 0.0, 0, box=box, volume=False)[2]

    # ---- streamlines (exa_hip_streamlines*; include/exa_hip.h states the contract) ----
    def extractStreamlines(self, seeds, channels=(0, 1, 2), step=0.5, max_steps=1000, forward=True, backward=False,
                           normalize=False, velocities=False, stream=None):
        """integrate the field lines of the vector field `channels` from seeds [n,3] (voxel space) into module-owned device
        memory; returns the number of vertices.  readStreamlines copies them out, releaseStreamlines frees them."""
        pts = np.ascontiguousarray(seeds, dtype=np.float32).reshape(-1, 3)
        ch3 = _i3(channels)
        flags = (STREAM_FORWARD if forward else 0) | (STREAM_BACKWARD if backward else 0)
        flags |= (STREAM_NORMALIZE if normalize else 0) | (STREAM_VELOCITIES if velocities else 0)
        nv = C.c_uint64(0)
        self._stream_counts = _StreamLines(0, 0, False)
        self._check(lib().exa_hip_streamlines(self.h, pts.ctypes.data, pts.shape[0], ch3, float(step), int(max_steps), flags,
                                              C.byref(nv), C.c_void_p(stream or 0)))
        self._stream_counts = _StreamLines(pts.shape[0], int(nv.value), bool(velocities))
        return int(nv.value)

    def readStreamlines(self):
        """(vertices float32 [V,3], offsets uint64 [n+1], seed_vertex uint32 [n], reasons int32 [n,2] (backward, forward),
        velocities float32 [V,3] or None) of the last extractStreamlines"""
        n, nv = self._stream_counts.seeds, self._stream_counts.vertices
        verts = np.empty((nv, 3), dtype=np.float32)
        vels = np.empty((nv, 3), dtype=np.float32) if self._stream_counts.velocities else None
        offsets = np.empty(n + 1, dtype=np.uint64)
        seed_vertex = np.empty(n, dtype=np.uint32)
        reasons = np.empty((n, 2), dtype=np.int32)
        self._check(lib().exa_hip_streamlines_read(self.h, verts.ctypes.data, _host_ptr(vels), offsets.ctypes.data,
                                                   seed_vertex.ctypes.data, reasons.ctypes.data, 0, None))
        return verts, offsets, seed_vertex, reasons, vels

    def releaseStreamlines(self):
        self._check(lib().exa_hip_streamlines_release(self.h))
        self._stream_counts = _StreamLines(0, 0, False)

    def streamlinesMs(self):
        """device ms of the last extraction's two kernels (count and emit), summed"""
        return self._ms(lib().exa_hip_streamlines_ms)

    def streamlines(self, seeds, channels=(0, 1, 2), step=0.5, max_steps=1000, forward=True, backward=False, normalize=False,
                    velocities=False):
        """field lines of the vector field formed by three channels, by fixed-step RK4 from seeds [n,3] in voxel space:
        (vertices [V,3], offsets [n+1], seed_vertex [n], reasons [n,2], velocities [V,3] or None).  Line i is
        vertices[offsets[i]:offsets[i+1]]: the backward part reversed, the seed at seed_vertex[i], the forward part.
        normalize: step along v/|v| (step is an arc length in voxels).  reasons: STREAM_END_* per direction (backward,
        forward).  The device copy is released before returning."""
        self.extractStreamlines(seeds, channels=channels, step=step, max_steps=max_steps, forward=forward, backward=backward,
                                normalize=normalize, velocities=velocities)
        return self._one_shot(self.readStreamlines, self.releaseStreamlines)

    # ---- line integral convolution on a cut plane (exa_hip_lic; include/exa_hip.h states the contract) ----
    def lic(self, plane, channels=(0, 1, 2), step=0.5, half_length=20, noise=None, seed=0, fill=float("nan"), stream=None):
        """the dense picture of the in-plane direction of the vector field `channels` on plane = (origin, du, dv, (nu, nv)),
        the lattice of isolines: per pixel the noise along its field line, `half_length` steps of `step` pixels backward and
        forward, averaged.  noise: uint8 [nv, nu], or None for the built-in hash of (ix, iy, seed).  Returns a dict of arrays
        [nv, nu]: lic (float32: sum / count; `fill` where the centre has no value), sum and count (uint32), speed (float32:
        |v| at the centre) and reasons (int32 [nv, nu, 2]: STREAM_END_* or LIC_END_IMAGE, backward and forward)."""
        origin, du, dv, size = plane
        nu, nv = int(size[0]), int(size[1])
        s = ExaHipPlane(_f3(origin), _f3(du), _f3(dv), nu, nv)
        if noise is not None:
            noise = np.ascontiguousarray(noise, dtype=np.uint8)
            if noise.size != nu * nv:
                raise ValueError("lic: the noise must hold nu * nv bytes")
        out = _outputs(_LIC_OUT, (max(nv, 0), max(nu, 0)))
        self._check(lib().exa_hip_lic(self.h, C.byref(s), _i3(channels), float(step), int(half_length), _host_ptr(noise),
                                      int(seed) & 0xFFFFFFFF, 0, float(fill), *_pointers(_LIC_OUT, out), 0,
                                      C.c_void_p(stream or 0)))
        return out

    def licMs(self):
        """device ms of the last lic call's kernels, summed"""
        return self._ms(lib().exa_hip_lic_ms)

    # ---- flow map and FTLE stretch on a lattice (exa_hip_flowmap; include/exa_hip.h states the contract) ----
    def flowmap(self, lo, hi, dims, channels=(0, 1, 2), step=0.5, num_steps=20, backward=False, fill=float("nan"), stream=None):
        """where a particle released at every point of the lattice of resample (lo, hi, dims; voxel space) is after num_steps
        RK4 steps of the time `step` through the vector field `channels`, forward or backward, and how much the map stretches.
        Returns a dict of arrays [nz, ny, nx]: end (float32 [nz, ny, nx, 3]), steps (uint32), reasons (int32, STREAM_END_*),
        stretch (float32: the largest eigenvalue of the Cauchy-Green tensor; `fill` where the point or a stencil neighbour did
        not last the time) and ftle (float32: log(stretch) / (2 |T|), T = num_steps * step, formed in float64; `fill` where
        stretch is)."""
        out = _outputs(_FLOWMAP_OUT, _lattice_shape(dims))
        self._check(lib().exa_hip_flowmap(self.h, _f3(lo), _f3(hi), _i3(dims), _i3(channels), float(step), int(num_steps),
                                          FLOWMAP_BACKWARD if backward else FLOWMAP_FORWARD, float(fill),
                                          *_pointers(_FLOWMAP_OUT, out), 0, C.c_void_p(stream or 0)))
        out["ftle"] = ftle_of_stretch(out["stretch"], step, num_steps, fill)
        return out

    def flowmapMs(self):
        """device ms of the last flowmap call's two stages: (integrate, stretch)"""
        return tuple(self._stage_ms(lib().exa_hip_flowmap_ms, 2))

    # ---- projections along rays (exa_hip_project; include/exa_hip.h states the contract) ----
    def project(self, org, orgDu, orgDv, dir, dirDu, dirDv, size, tmin, dt, num_samples, channel=0, world=False,
                normalize=False, stream=None):
        """the field of `channel` reduced along one ray per pixel of a size = (width, height) image: pixel (x, y) has the origin
        org + (x+.5)*orgDu + (y+.5)*orgDv and the direction dir + (x+.5)*dirDu + (y+.5)*dirDv (normalize: divided by its
        length), its samples lie at tmin + (i+.5)*dt, i < num_samples, in voxel space or (world=True) in world space.
        Returns a dict of arrays [height, width]: sum (float64: the valid samples added up; sum*dt is the line integral,
        sum/count the mean), count (uint32), max, min (float32; -inf / +inf where count is 0) and max_index (int32: the
        sample index of the first maximum, -1 for none)."""
        flags = self._probe_world(world) | (PROJECT_NORMALIZE if normalize else 0)
        rays, shape = _rays(org, orgDu, orgDv, dir, dirDu, dirDv, size, tmin, dt, num_samples)
        out = _outputs(_PROJECT_OUT, shape)
        self._check(lib().exa_hip_project(self.h, C.byref(rays), int(channel), flags, *_pointers(_PROJECT_OUT, out), 0,
                                          C.c_void_p(stream or 0)))
        return out

    def projectMs(self):
        """device ms of the last project call's kernel launches, summed"""
        return self._ms(lib().exa_hip_project_ms)

    # ---- the field on a triangle mesh (exa_hip_sample_triangles; include/exa_hip.h states the contract) ----
    def sampleTriangles(self, vertices=None, triangles=None, channels=(0,), spacing=1.0, max_n=SURFACE_MAX_N, world=False,
                        stream=None):
        """up to four channels of the field on the triangles of a mesh: every triangle is cut into n x n congruent parts, n =
        its longest edge over `spacing` rounded up, at most max_n (spacing 0: n = max_n), and sampled at their centroids.
        Returns a dict: sum float64 [m, C] of the valid samples, count uint32 [m, C], areaNormal float32 [m, 3] (half the
        cross product of the edges) and subdiv int32 [m] (n; 0: a bad index or a non-finite vertex, no samples).  vertices
        [nv, 3] and triangles [m, 3] in voxel space (world=True: world space): numpy arrays take the host path, contiguous
        float32 / int32 torch CUDA tensors the device path with torch tensors out; both None: the mesh the last
        extractIsoSurface left in the module (world as the extraction had it), read on the device."""
        ch = np.ascontiguousarray(channels, dtype=np.int32).reshape(-1)
        nc = min(len(ch), SURFACE_MAX_CHANNELS)                                 # the module checks the number
        flags = self._probe_world(world)
        args = (ch.ctypes.data, len(ch), float(spacing), int(max_n))
        empty, ptr, device = _like(vertices)
        if vertices is None and triangles is None:
            nt, mesh, flags = self._iso_counts.triangles, (None, 0, None, 0), flags | SURFACE_FROM_ISOSURFACE
        else:
            text = "vertices: a contiguous float32 tensor [nv, 3]; triangles: a contiguous int32 tensor [m, 3]"
            (verts, nv), (tris, nt) = _rows3(vertices, np.float32, device, text), _rows3(triangles, np.int32, device, text)
            mesh = (ptr(verts), nv, ptr(tris), nt)
        # the host path hands out zero-filled arrays and a uint32 count; tensors come uninitialised, their count as int32
        table = (("sum", (nc,), np.float64), ("count", (nc,), np.int32 if device else np.uint32),
                 ("areaNormal", (3,), np.float32), ("subdiv", (), np.int32))
        out = _outputs(table, (nt,), empty if device else np.zeros)
        self._check(lib().exa_hip_sample_triangles(self.h, *mesh, *args, flags, *_pointers(table, out, ptr), int(device),
                                                   C.c_void_p(stream or 0)))
        return out

    def sampleTrianglesMs(self):
        """device ms of the last sampleTriangles call's kernels, summed"""
        return self._ms(lib().exa_hip_sample_triangles_ms)

    def surfaceIntegrals(self, vertices=None, triangles=None, channels=(0,), spacing=1.0, max_n=SURFACE_MAX_N, world=False):
        """sampleTriangles (host path, or the module's iso mesh) and what a caller forms of it: surface_integrals(samples)"""
        return surface_integrals(self.sampleTriangles(vertices, triangles, channels, spacing, max_n, world))

    # ---- iso-crossings along rays (exa_hip_raycast_iso; include/exa_hip.h states the contract) ----
    def raycast_iso(self, org, orgDu, orgDv, dir, dirDu, dirDv, size, tmin, dt, num_samples, iso, refine=8, channel=0,
                    world=False, normalize=False, fill=float("nan"), outputs=RAYCAST_KEYS, stream=None):
        """where the field of `channel` first crosses `iso` along the rays of project (same arguments, same sample positions):
        a dict of arrays [height, width] — t (float32: the depth of the first crossing after `refine` rounds of bisection
        and a linear interpolation), position [.., 3] (in the caller's space), value and gradient [.., 3] (the point probe's
        value and voxel-space gradient at position), index (int32: the sample index behind the first crossing, -1 for none),
        side (int32: +1 entering the >= iso side, -1 leaving it, 0 for none), crossings (uint32: crossings of the whole ray).
        t, position, value and gradient are `fill` without a crossing.  outputs: the keys wanted; the others are skipped."""
        unknown = [k for k in outputs if k not in RAYCAST_KEYS]
        if unknown:
            raise ValueError(f"unknown outputs {unknown} (of {', '.join(RAYCAST_KEYS)})")
        flags = self._probe_world(world) | (PROJECT_NORMALIZE if normalize else 0)
        rays, shape = _rays(org, orgDu, orgDv, dir, dirDu, dirDv, size, tmin, dt, num_samples)
        table = [(k, tail if k in outputs else None, dtype) for k, tail, dtype in _RAYCAST_OUT]
        out = _outputs(table, shape)
        self._check(lib().exa_hip_raycast_iso(self.h, C.byref(rays), int(channel), float(iso), int(refine), flags, float(fill),
                                              *_pointers(table, out), 0, C.c_void_p(stream or 0)))
        return out

    def raycastIsoMs(self):
        """device ms of the last raycast_iso call's kernel launches, summed"""
        return self._ms(lib().exa_hip_raycast_iso_ms)


# what a Renderer keeps of its last extraction, per family, for the read that follows
_IsoMesh = namedtuple("_IsoMesh", "vertices triangles gradients")
_StreamLines = namedtuple("_StreamLines", "seeds vertices velocities")
_Isolines = namedtuple("_Isolines", "vertices segments levels gradients values_shape")
_Labelled = namedtuple("_Labelled", "count shape keep_values numbers")          # regions and basins; numbers: those the read repeats
_Critical = namedtuple("_Critical", "points probe")

# the output arrays of a call in the order of its pointer arguments: (key, the shape behind the image's or lattice's, dtype)
_LIC_OUT = (("lic", (), np.float32), ("sum", (), np.uint32), ("count", (), np.uint32), ("speed", (), np.float32),
            ("reasons", (2,), np.int32))
_FLOWMAP_OUT = (("end", (3,), np.float32), ("steps", (), np.uint32), ("reasons", (), np.int32), ("stretch", (), np.float32))
_PROJECT_OUT = (("sum", (), np.float64), ("count", (), np.uint32), ("max", (), np.float32), ("min", (), np.float32),
                ("max_index", (), np.int32))
_RAYCAST_OUT = (("t", (), np.float32), ("position", (3,), np.float32), ("value", (), np.float32), ("gradient", (3,), np.float32),
                ("index", (), np.int32), ("side", (), np.int32), ("crossings", (), np.uint32))
assert tuple(k for k, _, _ in _RAYCAST_OUT) == RAYCAST_KEYS


def _outputs(table, shape=(), empty=np.empty):
    """the arrays such a table describes, over `shape`, by key; a row whose trailing shape is None is an output not wanted"""
    return {k: empty(shape + tail, dtype) for k, tail, dtype in table if tail is not None}


def _host_ptr(a):
    """the pointer argument of a numpy array, null for None"""
    return None if a is None else a.ctypes.data


def _pointers(table, out, ptr=_host_ptr):
    """the pointer arguments of the table's call: null for an output not wanted"""
    return [ptr(out.get(k)) for k, _, _ in table]


def _like(x):
    """for the outputs of a call whose input x is a torch CUDA tensor or (anything else) host memory: (empty(shape, dtype),
    uninitialised arrays of x's library, tensors on x's device; ptr(array or None), their pointer argument; whether it is
    the device path)"""
    if not getattr(x, "is_cuda", False):
        return np.empty, _host_ptr, False
    import torch
    return (lambda shape, dtype: torch.empty(shape, dtype=getattr(torch, np.dtype(dtype).name), device=x.device),
            lambda a: None if a is None else C.c_void_p(a.data_ptr()), True)


def _rows3(x, dtype, device, text):
    """x as rows of three `dtype` values, and their number.  On the device path x is taken as it is, a contiguous tensor of
    that dtype (else TypeError(text)); on the host path numpy converts it"""
    if device:
        import torch
        if x.dtype != getattr(torch, np.dtype(dtype).name) or not x.is_contiguous() or x.numel() % 3:
            raise TypeError(text)
        return x, x.numel() // 3
    a = np.ascontiguousarray(x, dtype=dtype).reshape(-1, 3)
    return a, a.shape[0]


def _target(device, stream, async_):
    """the last three arguments of a call that writes host or device memory: only the device path has a stream to wait on"""
    return (1, C.c_void_p(stream or 0), int(async_)) if device else (0, None, 0)


def _lattice_shape(dims):
    """the shape of an array over the lattice of resample, x fastest; the module checks the dims"""
    return tuple(max(int(d), 0) for d in tuple(dims)[::-1])


def _lattice_out(dims, tail, out_ptr, stream, async_):
    """where a resample writes: (the float32 host array over the lattice it returns, or None with an out_ptr; the last four
    arguments of its call)"""
    if out_ptr is not None:
        return None, (_dev_ptr(out_ptr),) + _target(True, stream, async_)
    out = np.empty(_lattice_shape(dims) + tail, np.float32)
    return out, (out.ctypes.data,) + _target(False, stream, async_)


def _rays(org, orgDu, orgDv, dir, dirDu, dirDv, size, tmin, dt, num_samples):
    """(the ExaHipRays of these arguments, the shape (height, width) of a per-pixel output — (0, 0) for a size the module
    refuses)"""
    rays = ExaHipRays()
    for name, v in (("org", org), ("orgDu", orgDu), ("orgDv", orgDv), ("dir", dir), ("dirDu", dirDu), ("dirDv", dirDv)):
        setattr(rays, name, _f3(v))
    rays.width, rays.height = int(size[0]), int(size[1])
    rays.tmin, rays.dt, rays.numSamples = float(tmin), float(dt), int(num_samples)
    shape = (max(rays.height, 0), max(rays.width, 0))                      # the module checks the size
    if shape[0] * shape[1] > 2 ** 31 - 1:
        shape = (0, 0)
    return rays, shape


def region_measures(regions, sum_exponent, lo, hi, dims):
    """what follows from the table of Renderer.regions over the lattice (lo, hi, dims), per region, in float64: `sum` of the
    values (sumFixed * 2^-sum_exponent, exact up to the double's 53 bits), `mean`, `volume` (points times the volume of a
    lattice cell), `integral` (sum times that volume), and `centroid` [n, 3], the mean position of the region's points in the
    space of lo / hi (lattice point i on an axis lies at lo + (i + 0.5) * (hi - lo) / dims)"""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    step = (hi - lo) / np.asarray(dims, np.float64).reshape(3)
    points = regions["points"].astype(np.float64)
    total = np.ldexp(regions["sumFixed"].astype(np.float64), -int(sum_exponent))
    cell = float(np.prod(step))
    return dict(sum=total, mean=total / points, volume=points * cell, integral=total * cell,
                centroid=lo + (regions["sumIndex"].astype(np.float64) / points[:, None] + 0.5) * step)


def ftle_of_stretch(stretch, step, num_steps, fill=float("nan")):
    """FTLE = log(stretch) / (2 |T|), T = num_steps * float32(step), formed in float64 and rounded to float32; `fill` where
    stretch holds the bits of float32(fill) (include/exa_hip.h, exa_hip_flowmap)"""
    stretch = np.ascontiguousarray(stretch, dtype=np.float32)
    with np.errstate(all="ignore"):
        ftle = (np.log(stretch.astype(np.float64)) / (2.0 * num_steps * np.float64(np.float32(step)))).astype(np.float32)
    filled = stretch.view(np.uint32) == np.float32(fill).view(np.uint32)
    return np.where(filled, np.float32(fill), ftle).astype(np.float32)


# ---- the sources and axes of Renderer.profile ----
def channel(c):
    """the source `channel c` on the lattice: what resample returns with a NaN fill"""
    return ExaHipSource(SOURCE_CHANNEL, (C.c_int32 * 3)(int(c), 0, 0), 0, (C.c_float * 3)())


def derived(quantity, channels=(0, 1, 2)):
    """the source `derived quantity of the vector field channels` (one component): what resampleDerived returns"""
    return ExaHipSource(SOURCE_DERIVED, _i3(channels), derived_quantity(quantity), (C.c_float * 3)())


def radius(centre):
    """the source `distance of the lattice position from centre`, in the space of lo / hi"""
    return ExaHipSource(SOURCE_RADIUS, (C.c_int32 * 3)(), 0, _f3(centre))


def coordinate(axis):
    """the source `component axis (0, 1, 2) of the lattice position`"""
    return ExaHipSource(SOURCE_COORDINATE, (C.c_int32 * 3)(int(axis), 0, 0), 0, (C.c_float * 3)())


class ProfileAxis:
    """an axis of Renderer.profile: the struct, and what it points to kept alive"""

    def __init__(self, struct, keep=None, device=False):
        self.struct, self.keep, self.device = struct, keep, device


def uniform(src, lo, hi, n):
    """n uniform bins of the source over [lo, hi], by exa_hip_histogram's rule"""
    return ProfileAxis(ExaHipProfileAxis(src, int(n), float(lo), float(hi), None, None))


def edges(src, array):
    """bins between the strictly ascending float32 `array` of numBins + 1 edges, the last bin closed"""
    e = np.ascontiguousarray(array, np.float32).reshape(-1)
    return ProfileAxis(ExaHipProfileAxis(src, e.size - 1, 0.0, 0.0, e.ctypes.data, None), keep=e)


def labels(array_or_device_ptr, n):
    """the bin of every lattice point given directly, n of them: an int32 array of numPoints labels (what Renderer.regions /
    basins return under `labels`; < 0: outside), or a device pointer (an int, or an int32 torch CUDA tensor) to them"""
    if isinstance(array_or_device_ptr, np.ndarray):
        a = np.ascontiguousarray(array_or_device_ptr, np.int32).reshape(-1)
        return ProfileAxis(ExaHipProfileAxis(ExaHipSource(), int(n), 0.0, 0.0, None, a.ctypes.data), keep=a)
    ptr = _dev_ptr(array_or_device_ptr)
    return ProfileAxis(ExaHipProfileAxis(ExaHipSource(), int(n), 0.0, 0.0, None, ptr), keep=array_or_device_ptr, device=True)


def profile_measures(result, lo, hi, dims):
    """what follows from the dict of Renderer.profile over the lattice (lo, hi, dims), per bin, in float64: `sums`
    [numValues, B...] (fixed * 2^-exponent of the series), `sum_weight` (or None), `means` (sum of w*v over sum of w, or sum
    of v over count; NaN in an empty bin) and `volume` (count times the volume of a lattice cell), as region_measures does"""
    st = result["stats"]
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    cell = float(np.prod((hi - lo) / np.asarray(dims, np.float64).reshape(3)))
    count = result["count"].astype(np.float64)
    sums = np.stack([np.ldexp(s.astype(np.float64), -int(st["valueExponent"][f])) for f, s in enumerate(result["sums"])]) \
        if len(result["sums"]) else np.zeros(result["sums"].shape, np.float64)
    sum_weight = None if result["sum_weight"] is None else np.ldexp(result["sum_weight"].astype(np.float64), -int(st["weightExponent"]))
    with np.errstate(all="ignore"):
        means = sums / (count if sum_weight is None else sum_weight)
    return dict(sums=sums, sum_weight=sum_weight, means=means, volume=count * cell)


def _f3(v):
    return (C.c_float * 3)(*[float(c) for c in v])


def _i3(v):
    return (C.c_int32 * 3)(*[int(c) for c in v])


def _dev_ptr(x):
    """a device pointer from an int, None, or a contiguous torch CUDA tensor of 4-byte elements"""
    if x is None:
        return None
    if isinstance(x, int):
        return C.c_void_p(x)
    if not (getattr(x, "is_cuda", False) and x.is_contiguous() and x.element_size() == 4):
        raise TypeError("a device pointer or a contiguous float32 / int32 torch CUDA tensor is expected")
    return C.c_void_p(x.data_ptr())
