"""The kernels of exa_hip_basins in the gfx950 code object of the iso-mesh unit (no GPU needed; tests/code_objects.py is the
reader): each is there exactly once, without scratch and without spilled registers, within the 64 vector registers that
leave these memory-bound passes their full occupancy."""
import pytest

from code_objects import kernels

UNIT = "exa_isomesh.o"
KERNELS = ["isoBasinUpKernel", "isoBasinJumpKernel", "isoBasinCountKernel", "isoBasinRankKernel", "isoBasinLabelKernel",
           "isoBasinPassKernel", "isoBasinLinkKernel", "isoBasinMergeKernel", "isoBasinFinalKernel", "isoBasinStatsKernel",
           "isoBasinFirstKernel", "isoBasinFinishKernel"]


@pytest.mark.parametrize("want", KERNELS)
def test_basin_kernel_is_there_once_within_its_budget(want):
    found = [r for name, r in kernels(UNIT).items() if want in name]
    assert len(found) == 1, (want, sorted(kernels(UNIT)))
    r = found[0]
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0 and r.vgpr <= 64, (want, r)


def test_the_unit_holds_no_other_basin_kernel():
    names = [name for name in kernels(UNIT) if "isoBasin" in name]
    assert len(names) == len(KERNELS), names
