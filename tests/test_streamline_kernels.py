"""The streamline integrator's kernels (exa_hip_streamlines), read from the gfx950 code objects the build left in csrc/ (no
GPU needed): every sampler variant — basis form 0, form 1, form 0 with empty cells — has its translation unit, its count and
emit kernels (plain and normalised) run without scratch and without spilled registers, and the units hold nothing else.  A
missing object is a failure: build() makes them."""
import pytest

from test_sample_kernels import _kernels

VARIANTS = {"exa_stream_f0.o": "form0", "exa_stream_f1.o": "form1", "exa_stream_f0e.o": "form0e"}


def _name(ns, emit, norm):
    return f"_ZN3exa{len(ns)}{ns}17streamlinesKernelILb{int(emit)}ELb{int(norm)}EEEvNS_10StreamArgsE"


@pytest.mark.parametrize("obj", sorted(VARIANTS))
def test_streamline_kernels_have_no_scratch_and_no_spills(obj):
    ns = VARIANTS[obj]
    k = _kernels(obj)
    want = [_name(ns, emit, norm) for emit in (False, True) for norm in (False, True)]
    missing = [w for w in want if w not in k]
    assert not missing, (missing, sorted(k))
    for name in want:
        vgpr, scratch, vspill, sspill = k[name]
        print(name, "vgprs", vgpr)
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, vgpr, scratch, vspill, sspill)


@pytest.mark.parametrize("obj", sorted(VARIANTS))
def test_streamline_units_hold_only_the_streamline_kernels(obj):
    # the renderer's and the probes' kernels stay in their own units: compiling them again here would double the build
    k = _kernels(obj)
    assert k and all("streamlinesKernel" in name for name in k), sorted(k)
