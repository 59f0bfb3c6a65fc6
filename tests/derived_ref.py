"""The table of derived flow quantities of include/exa_hip.h (exa_hip_sample_derived) in numpy float32: not a test module.

derived(q, v, J) takes the values v [n, 3] and the Jacobian J [n, 3, 3] (J[:, c, k] = component k of the gradient of channel
c: what samplePoints(..., gradient=True, normalized=True) returns) and gives [n], or [n, 3] for the vorticity.  Every array
operation of numpy on float32 arrays is one correctly rounded float32 operation per element, so the expressions below are
the contract's: rounded separately, nothing contracted, associated as written.  With dtype=np.float64 the same expressions
are the float64 reference of tests/test_gpu_derived.py."""
import numpy as np

SPEED, DIVERGENCE, VORTICITY, VORTICITY_MAGNITUDE, Q, HELICITY = range(6)
QUANTITIES = {"speed": SPEED, "divergence": DIVERGENCE, "vorticity": VORTICITY, "vorticity_magnitude": VORTICITY_MAGNITUDE,
              "q": Q, "helicity": HELICITY}
COMPONENTS = {SPEED: 1, DIVERGENCE: 1, VORTICITY: 3, VORTICITY_MAGNITUDE: 1, Q: 1, HELICITY: 1}


def vorticity(J):
    return J[:, 2, 1] - J[:, 1, 2], J[:, 0, 2] - J[:, 2, 0], J[:, 1, 0] - J[:, 0, 1]


def derived(q, v, J, dtype=np.float32):
    v = np.ascontiguousarray(v, dtype=dtype).reshape(-1, 3)
    J = np.ascontiguousarray(J, dtype=dtype).reshape(-1, 3, 3)
    with np.errstate(all="ignore"):                              # NaN and infinities propagate by the formulas
        wx, wy, wz = vorticity(J)
        if q == SPEED:
            return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        if q == DIVERGENCE:
            return (J[:, 0, 0] + J[:, 1, 1]) + J[:, 2, 2]
        if q == VORTICITY:
            return np.stack([wx, wy, wz], axis=1)
        if q == VORTICITY_MAGNITUDE:
            return np.sqrt((wx * wx + wy * wy) + wz * wz)
        if q == Q:
            d = (J[:, 0, 0] * J[:, 0, 0] + J[:, 1, 1] * J[:, 1, 1]) + J[:, 2, 2] * J[:, 2, 2]
            o = (J[:, 0, 1] * J[:, 1, 0] + J[:, 0, 2] * J[:, 2, 0]) + J[:, 1, 2] * J[:, 2, 1]
            return dtype(-0.5) * d - o
        if q == HELICITY:
            return (v[:, 0] * wx + v[:, 1] * wy) + v[:, 2] * wz
    raise ValueError(f"unknown quantity {q}")


def from_probe(q, values, gradients, status, fill):
    """the contract's composition: derived() of samplePoints' values [n, 3], gradients [n, 3, 3] and status [n, 3] (normalized
    gradient); returns (out, status [n]) with status -2 where any channel has -2, and `fill` in every component where it is < 0"""
    st = np.where((status == -2).any(axis=1), -2, status[:, 0]).astype(np.int32)
    st = np.where((status == -1).any(axis=1), -1, st).astype(np.int32)
    out = derived(q, values, gradients).astype(np.float32)
    bad = st < 0
    out[bad] = np.float32(fill)
    return out, st
