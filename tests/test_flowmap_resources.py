"""The kernels of exa_hip_flowmap in the gfx950 code objects (no GPU needed; tests/code_objects.py is the reader).  The
integrator (streamlinesKernelFlowmap, exa_flowmap_kernels.h) is there exactly once per streamline unit, keeps its line's state
in registers — no scratch, no spilled vector or scalar register, no LDS — and leaves a SIMD at least as many waves as the
streamline integrator of the same unit, whose evaluation and stage machine it shares.  The stretch kernel
(isoLatticeStretchKernel) is there once, in the iso-mesh unit, with its 3 x 3 matrix in registers: no scratch, no spills."""
import pytest

from code_objects import kernels

FORMS = {"f0": "form0", "f1": "form1", "f0e": "form0e"}          # the unit's suffix -> the namespace of its kernels


def _waves(vgprs):
    """waves per SIMD that a kernel's vector registers allow on gfx950: 512 per lane, allocated in steps of 8, at most 8"""
    return min(8, 512 // (8 * ((vgprs + 7) // 8)))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_integrator_is_there_once_in_registers_at_the_streamlines_occupancy(form):
    ns, k = FORMS[form], kernels(f"exa_stream_{form}.o")
    found = [r for name, r in k.items() if "Flowmap" in name]
    assert len(found) == 1 and f"_ZN3exa{len(ns)}{ns}24streamlinesKernelFlowmapENS_11FlowmapArgsE" in k, sorted(k)
    r = found[0]
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0 and r.lds == 0, r
    count = k[f"_ZN3exa{len(ns)}{ns}17streamlinesKernelILb0ELb0EEEvNS_10StreamArgsE"]        # <EMIT = false, NORM = false>
    print(f"{form}: flow map {r.vgpr} VGPRs, {_waves(r.vgpr)} waves; streamlinesKernel<false,false> {count.vgpr} VGPRs, {_waves(count.vgpr)} waves")
    assert _waves(r.vgpr) >= _waves(count.vgpr), (r, count)


def test_stretch_kernel_is_there_once_without_scratch_and_spills():
    k = kernels("exa_isomesh.o")
    found = [(name, r) for name, r in k.items() if "Stretch" in name]
    assert len(found) == 1 and "isoLatticeStretchKernel" in found[0][0], sorted(k)
    r = found[0][1]
    print(f"stretch: {r.vgpr} VGPRs, {_waves(r.vgpr)} waves")
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0 and r.lds == 0, r


def test_waves_from_registers():
    assert [_waves(v) for v in (64, 65, 72, 73, 80, 88, 96, 128, 129, 512)] == [8, 7, 7, 6, 6, 5, 5, 4, 3, 1]
