"""exa_hip_distance: the exact Euclidean distance transform of a set of lattice points (include/exa_hip.h states the
contract).  Functions of a binding.Renderer `R`:

    distance(R, lo, hi, dims, iso, ...)         the set is field >= iso (or < iso, or its complement, or both, signed)
    distance_mask(R, lo, hi, dims, labels, ...) the set is given by labels (Renderer.regions / basins), host or device
    distance_stage_ms(R)                        device ms of the last call's stages
    distance_bands(dist, width, n)              distances to band labels, for binding.labels(...) and Renderer.profile
"""
import ctypes as C

import numpy as np

from . import binding
from .binding import lib

DISTANCE_BELOW = 32
DISTANCE_TO_OUTSIDE = 64
DISTANCE_SIGNED = 128
DISTANCE_LABELS_DEVICE = 256


class ExaHipDistanceStats(C.Structure):
    _fields_ = [("points", C.c_uint64), ("inside", C.c_uint64), ("reached", C.c_uint64), ("maxDistance", C.c_float),
                ("pad", C.c_int32)]

    def asdict(self):
        return dict(points=int(self.points), inside=int(self.inside), reached=int(self.reached),
                    maxDistance=float(self.maxDistance))


def _flags(below, to_outside, signed):
    return (DISTANCE_BELOW if below else 0) | (DISTANCE_TO_OUTSIDE if to_outside else 0) | (DISTANCE_SIGNED if signed else 0)


def _call(R, fn, head, tail_args, dims, nearest, out, stream):
    """fn(handle, *head, *tail_args, dist, nearest, stats, pointersAreDevice, stream) into new host arrays over the lattice,
    or (out = (dist, nearest or None): device pointers or torch CUDA tensors) into the caller's device memory"""
    stats = ExaHipDistanceStats()
    if out is None:
        shape = binding._lattice_shape(dims)
        dist = np.empty(shape, np.float32)
        near = np.empty(shape, np.int32) if nearest else None
        pointers = (dist.ctypes.data, binding._host_ptr(near), C.byref(stats), 0)
    else:
        dist, near = out
        pointers = (binding._dev_ptr(dist), binding._dev_ptr(near), C.byref(stats), 1)
    R._check(fn(R.h, *head, *tail_args, *pointers, C.c_void_p(stream or 0)))
    result = dict(dist=dist, stats=stats.asdict())
    if near is not None:
        result["nearest"] = near
    return result


def distance(R, lo, hi, dims, iso, channel=0, quantity=None, channels=(0, 1, 2), max_distance=float("inf"), below=False,
             to_outside=False, signed=False, nearest=False, world=False, stream=None, out=None):
    """per point of the lattice of resample (lo, hi, dims) the distance to the nearest point where the field of `channel`
    (with a `quantity`: that derived quantity of `channels`) is inside — finite and >= iso, `below`: finite and < iso;
    `to_outside`: to the nearest point that is not inside; `signed`: + the distance to the inside set at the other points,
    - the distance to the others at inside points.  Distances are in the space of lo / hi; beyond max_distance, or with no
    target, +INF (-INF).  Returns a dict: dist float32 [nz, ny, nx], nearest int32 (the linear index of the nearest target,
    -1 for none; only with nearest=True), stats (points, inside, reached, maxDistance).  out = (dist, nearest or None) as
    device pointers or torch CUDA tensors writes there instead."""
    head = (binding._f3(lo), binding._f3(hi), binding._i3(dims))
    tail = (float(iso), float(max_distance), R._probe_world(world) | _flags(below, to_outside, signed))
    if quantity is None:
        return _call(R, lib().exa_hip_distance, head, (int(channel),) + tail, dims, nearest, out, stream)
    return _call(R, lib().exa_hip_distance_derived, head, (binding._i3(channels), binding.derived_quantity(quantity)) + tail, dims,
                 nearest, out, stream)


def distance_mask(R, lo, hi, dims, labels, label=-1, max_distance=float("inf"), to_outside=False, signed=False, nearest=False,
                  stream=None, out=None):
    """as distance, of the set labels == label (label == -1: labels >= 0); lo, hi and dims give only the spacing.  `labels`:
    an int32 numpy array of numPoints labels, or a device pointer (an int, or an int32 torch CUDA tensor) to them"""
    flags = _flags(False, to_outside, signed)
    if isinstance(labels, np.ndarray):
        keep = np.ascontiguousarray(labels, np.int32).reshape(-1)
        ptr = keep.ctypes.data
    else:
        keep, ptr = labels, binding._dev_ptr(labels)
        flags |= DISTANCE_LABELS_DEVICE
    head = (binding._f3(lo), binding._f3(hi), binding._i3(dims))
    return _call(R, lib().exa_hip_distance_mask, head, (ptr, int(label), float(max_distance), flags), dims, nearest, out, stream)


def distance_stage_ms(R):
    """device ms of the last distance call's stages: (values, rows, columns, finish)"""
    return tuple(R._stage_ms(lib().exa_hip_distance_stage_ms, 4))


def distance_bands(dist, width, n):
    """int32 labels floor(|dist| / width) (formed in float64), -1 where that is >= n or dist is not finite: the shells of
    width `width` about the target set, for binding.labels(bands, n) as the label axis of Renderer.profile"""
    d = np.abs(np.asarray(dist, np.float32).astype(np.float64))
    with np.errstate(invalid="ignore"):
        q = np.floor(d / float(width))
    return np.where(np.isfinite(d) & (q < int(n)), q, -1).astype(np.int32)
