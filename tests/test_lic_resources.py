"""The kernel of exa_hip_lic (streamlinesKernelLic, exa_lic_kernels.h) in the gfx950 code objects of the streamline units (no
GPU needed; tests/code_objects.py is the reader): it is there exactly once per unit, keeps its line's state in registers — no
scratch, no spilled vector or scalar register — and leaves a SIMD at least as many waves as the streamline integrator of the
same unit, whose evaluation it shares."""
import pytest

from code_objects import kernels

FORMS = {"f0": "form0", "f1": "form1", "f0e": "form0e"}          # the unit's suffix -> the namespace of its kernels


def _waves(vgprs):
    """waves per SIMD that a kernel's vector registers allow on gfx950: 512 per lane, allocated in steps of 8, at most 8"""
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_lic_kernel_is_there_once_in_registers_at_the_integrators_occupancy(form):
    ns, k = FORMS[form], kernels(f"exa_stream_{form}.o")
    found = [r for name, r in k.items() if "Lic" in name]
    assert len(found) == 1 and f"_ZN3exa{len(ns)}{ns}20streamlinesKernelLicENS_7LicArgsE" in k, sorted(k)
    r = found[0]
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0 and r.lds == 0, r
    count = k[f"_ZN3exa{len(ns)}{ns}17streamlinesKernelILb0ELb1EEEvNS_10StreamArgsE"]        # <EMIT = false, NORM = true>
    print(f"{form}: lic {r.vgpr} VGPRs, {_waves(r.vgpr)} waves; streamlinesKernel<false,true> {count.vgpr} VGPRs, {_waves(count.vgpr)} waves")
    assert _waves(r.vgpr) >= _waves(count.vgpr), (r, count)


def test_waves_from_registers():
    assert [_waves(v) for v in (64, 65, 72, 73, 80, 88, 96, 128, 129, 512)] == [8, 7, 7, 6, 6, 5, 5, 4, 3, 1]
