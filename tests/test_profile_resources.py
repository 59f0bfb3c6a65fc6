"""The kernels of exa_hip_profile in the gfx950 code object of exa_isomesh.o (no GPU needed; tests/code_objects.py is the
reader): each is there exactly once, without scratch and without spilled registers, within the 64 vector registers that
leave the memory-bound passes of the unit their full occupancy; the LDS variant of the accumulate pass holds its table in
dynamic shared memory, so the static size says nothing about the workgroups per CU."""
import pytest

from code_objects import kernels

UNIT = "exa_isomesh.o"
PROFILE = ["isoProfileClassifyKernel", "isoProfileAccumulateKernelILb1E", "isoProfileAccumulateKernelILb0E", "isoProfileFinishKernel"]


@pytest.mark.parametrize("want", PROFILE)
def test_profile_kernel_is_there_once_within_its_registers(want):
    found = [r for name, r in kernels(UNIT).items() if want in name]
    assert len(found) == 1, (want, sorted(kernels(UNIT)))
    r = found[0]
    assert r.vgpr <= 64 and r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0, (want, r)


def test_the_unit_holds_no_other_profile_kernel():
    names = [name for name in kernels(UNIT) if "Profile" in name]
    assert len(names) == len(PROFILE) and all("iso" in name for name in names), names


def test_the_lds_table_is_dynamic_shared_memory():
    (lds,) = [r for name, r in kernels(UNIT).items() if "isoProfileAccumulateKernelILb1E" in name]
    assert lds.lds == 0, lds
