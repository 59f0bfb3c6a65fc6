"""The kernels of exa_hip_sample_triangles in the gfx950 code objects the build left in csrc/ (no GPU needed;
tests/code_objects.py is the reader): every instance is there exactly once in each of the three units of the probes, without
scratch and without spilled vector or scalar registers — the sampling kernel holds the voxelSpaceTransform in LDS for that —,
and no other kernel of a unit carries the name."""
import pytest

from code_objects import kernels

FORMS = {"f0": "form0", "f1": "form1", "f0e": "form0e"}          # the unit's suffix -> the namespace of its kernels


def _instances(ns):
    return ([f"_ZN3exa{len(ns)}{ns}25sampleTrianglesPrepKernelENS_7TriArgsE"]
            + [f"_ZN3exa{len(ns)}{ns}21sampleTrianglesKernelILb{u}EEEvNS_7TriArgsE" for u in (0, 1)])


@pytest.mark.parametrize("unit,want", [(f"exa_sample_{f}.o", w) for f, ns in sorted(FORMS.items()) for w in _instances(ns)])
def test_instance_is_there_once_without_scratch_and_spills(unit, want):
    found = [r for name, r in kernels(unit).items() if name == want]
    assert len(found) == 1, (unit, want, sorted(kernels(unit)))
    r = found[0]
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0, (unit, want, r)


@pytest.mark.parametrize("f", sorted(FORMS))
def test_no_other_kernel_of_the_unit_is_about_triangles(f):
    names = [n for n in kernels(f"exa_sample_{f}.o") if "Triangles" in n]
    assert sorted(names) == sorted(_instances(FORMS[f])), names
    assert all("sampleTriangles" in n for n in names)
