"""The kernels of exa_hip_distance in the gfx950 code object of exa_isomesh.o (no GPU needed; tests/code_objects.py is the
reader): each is there exactly once, without scratch and without spilled registers, within the 64 vector registers that
leave the memory-bound passes of the unit their full occupancy; the column pass is one template, built for y and for z."""
import pytest

from code_objects import kernels

UNIT = "exa_isomesh.o"
DISTANCE = ["isoDistanceInsideKernel", "isoDistanceRowKernel", "isoDistanceColumnKernelILi1E", "isoDistanceColumnKernelILi2E",
            "isoDistanceFinishKernel"]


@pytest.mark.parametrize("want", DISTANCE)
def test_distance_kernel_is_there_once_within_its_registers(want):
    found = [r for name, r in kernels(UNIT).items() if want in name]
    assert len(found) == 1, (want, sorted(kernels(UNIT)))
    r = found[0]
    assert r.vgpr <= 64 and r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0, (want, r)


def test_the_unit_holds_no_other_distance_kernel():
    names = [name for name in kernels(UNIT) if "Distance" in name]
    assert len(names) == len(DISTANCE) and all("isoDistance" in name for name in names), names
