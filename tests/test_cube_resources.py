"""Registers, scratch and spills of the cube instantiations of the one-channel rope march (NCH == 1: the 16-byte cube
records, owlexabrick_amd/csrc/exa_cube.h), read from the gfx950 code object the build left in csrc/ (no GPU needed;
tests/code_objects.py is the reader).  They are compiled for seven waves per SIMD like the variants they replace in a cube
scene: 72 vector registers, no scratch — tests/test_kernel_resources.py says what the occupancy is worth."""
import re

import pytest

from code_objects import kernels
from test_kernel_resources import _march

UNIT = "exa_kernels_f1r.o"
CASES = [(grad, surf) for grad in (False, True) for surf in (False, True)]


@pytest.mark.parametrize("grad,surf", CASES, ids=[f"{'gradient' if g else 'plain'}-{'surfaces' if s else 'dvr'}" for g, s in CASES])
def test_cube_march_keeps_seven_waves_without_scratch(grad, surf):
    name = _march("form1", grad, True, 0, surf, 0, True, 1, True)
    k = kernels(UNIT)
    assert name in k, (name, sorted(n for n in k if "renderFrameKdKernel" in n))
    r = k[name]
    print(f"RESOURCES {name}: {r}")
    # (what tests/test_kernel_resources.py holds the variants on the march headers to: these, like those, park a few scalar
    # registers in lanes of a vector register around the march — sgpr_spill, no memory involved)
    assert r.vgpr <= 72 and r.scratch == 0 and r.vgpr_spill == 0, (name, r)


def test_the_cube_form_exists_for_the_shipped_one_channel_rope_march_only():
    """four instantiations in the form-1 rope unit, none in any other unit"""
    # <GRAD, FAST, MULTI, SURF, STATS, SMALL, NCH, ROPE>: NCH == 1 is the second-to-last argument
    cube = lambda unit: sorted(n for n in kernels(unit) if re.search(r"renderFrameKdKernelI.*Li1ELb[01]EEEvNS_10RenderArgsE$", n))   # noqa: E731
    want = sorted(_march("form1", g, True, 0, s, 0, True, 1, True) for g, s in CASES)
    assert cube(UNIT) == want
    for unit in ("exa_kernels_f1.o", "exa_kernels_f0.o", "exa_kernels_f0r.o", "exa_kernels_f0e.o", "exa_kernels_f0er.o"):
        assert kernels(unit) and not cube(unit), unit
