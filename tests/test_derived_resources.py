"""The kernels of the derived flow quantities (sampleDerivedPointsKernel, sampleDerivedGridKernel; exa_sample_kernels.h) in the
gfx950 code objects of the probes' units (no GPU needed; tests/code_objects.py is the reader): the quantity is a runtime
argument, so each unit holds one points instance and the eight grid instances <patch shape, UNIFORM>, each exactly once; they
keep the three channels' values and Jacobian in registers: no scratch, no spilled vector or scalar register, no LDS."""
import pytest

from code_objects import kernels

FORMS = {"f0": "form0", "f1": "form1", "f0e": "form0e"}          # the unit's suffix -> the namespace of its kernels
SHAPES = [(64, 1, 1), (16, 4, 1), (8, 8, 1), (4, 4, 4)]


def _names(ns):
    return ([f"_ZN3exa{len(ns)}{ns}25sampleDerivedPointsKernelENS_10SampleArgsE"]
            + [f"_ZN3exa{len(ns)}{ns}23sampleDerivedGridKernelILi{x}ELi{y}ELi{z}ELb{u}EEEvNS_10SampleArgsE"
               for x, y, z in SHAPES for u in (0, 1)])


@pytest.mark.parametrize("form", sorted(FORMS))
def test_the_nine_instances_are_there_once_in_registers(form):
    unit = f"exa_sample_{form}.o"
    k = kernels(unit)
    want = _names(FORMS[form])
    assert len(want) == 9
    assert sorted(name for name in k if "Derived" in name) == sorted(want), (unit, sorted(k))
    for name in want:
        r = k[name]
        print(f"{unit} vgpr {r.vgpr:3d} sgpr {r.sgpr:3d}  {name}")
        assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0 and r.lds == 0, (unit, name, r)
