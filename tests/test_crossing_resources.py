"""The kernel of exa_hip_raycast_iso (sampleCrossingsKernel, exa_sample_kernels.h) in the gfx950 code objects of the probes'
units (no GPU needed; tests/code_objects.py is the reader): every instance — wave-uniform or per-lane lookup, with or without
the skipping of indices — is there exactly once per unit, and keeps the march, the bracket of the first crossing, the
refinement and the gradient sample at the hit in registers: no scratch, no spilled vector or scalar register and no LDS under
its launch bound of 256."""
import pytest

from code_objects import kernels

FORMS = {"f0": "form0", "f1": "form1", "f0e": "form0e"}          # the unit's suffix -> the namespace of its kernels
INSTANCES = [(u, s) for u in (0, 1) for s in (0, 1)]            # <UNIFORM, SKIP>


def _name(ns, uniform, skip):
    return f"_ZN3exa{len(ns)}{ns}21sampleCrossingsKernelILb{uniform}ELb{skip}EEEvNS_9CrossArgsE"


@pytest.mark.parametrize("uniform,skip", INSTANCES)
@pytest.mark.parametrize("form", sorted(FORMS))
def test_crossing_kernel_is_there_once_without_scratch_spills_and_lds(form, uniform, skip):
    unit = f"exa_sample_{form}.o"
    k = kernels(unit)
    want = _name(FORMS[form], uniform, skip)
    found = [r for name, r in k.items() if name == want]
    assert len(found) == 1, (unit, want, sorted(k))
    r = found[0]
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0 and r.lds == 0, (unit, want, r)


@pytest.mark.parametrize("form", sorted(FORMS))
def test_unit_holds_no_other_crossing_kernel(form):
    k = kernels(f"exa_sample_{form}.o")
    crossings = sorted(name for name in k if "Crossings" in name)
    assert crossings == sorted(_name(FORMS[form], u, s) for u, s in INSTANCES), crossings
