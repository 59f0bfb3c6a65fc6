"""The kernels of exa_hip_critical_points in the gfx950 code object of the iso-mesh unit (no GPU needed; tests/code_objects.py
is the reader): each is there exactly once, without scratch and without spilled registers, within the 64 vector registers
that leave these passes their full occupancy — the refine and the emit kernel accumulate the interpolant and its derivative
corner by corner instead of holding a cell's 24 corner values."""
import pytest

from code_objects import kernels

UNIT = "exa_isomesh.o"
KERNELS = ["isoCriticalCellKernel", "isoCriticalCompactKernel", "isoCriticalRefineKernel", "isoCriticalEmitKernel",
           "isoCriticalPackKernel"]


def _waves(vgprs):
    """waves per SIMD that a kernel's vector registers allow on gfx950: 512 per lane, allocated in steps of 8, at most 8"""
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


@pytest.mark.parametrize("want", KERNELS)
def test_critical_kernel_is_there_once_within_its_budget(want):
    found = [r for name, r in kernels(UNIT).items() if want in name]
    assert len(found) == 1, (want, sorted(kernels(UNIT)))
    r = found[0]
    print(f"{want}: {r.vgpr} VGPRs, {_waves(r.vgpr)} waves, LDS {r.lds} bytes")
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0 and r.vgpr <= 64, (want, r)


def test_the_unit_holds_no_other_critical_kernel():
    names = [name for name in kernels(UNIT) if "isoCritical" in name]
    assert len(names) == len(KERNELS), names
