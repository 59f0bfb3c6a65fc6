"""Registers, scratch and spills of the module's kernels, read from the gfx950 code objects the build left in csrc/ (no GPU
needed; tests/code_objects.py is the reader).  Every object that holds device code has its expectations here, and the
build's own list of them (`make print-device-objs`) is held against this file, so a new unit cannot arrive without any.

The march's speed hangs on its occupancy: a variant compiled for seven waves per SIMD must fit 72 vector registers and one
for six waves 80 — and must do so WITHOUT scratch: the same kernel with the pixel's colour spilled inside the march loop takes
22.1 instead of 17.1 ms on the bench scene (profiles/r05_experiments.txt 15), and nothing else in the suite would notice.
Checked for the variants the default frame of every BASELINE configuration launches (form 1, not instrumented); the
instrumented instances of the same units do use scratch and spill scalar registers, and are not held to anything.

The probes, the streamlines, the iso-surface and the histogram each have units of their own, which hold their kernels and
nothing else (compiling the renderer's again there would double the build), without scratch and without spilled registers;
the memory-bound passes of the last two at a register count that leaves them their full occupancy."""
import collections
import subprocess

import pytest

from code_objects import CSRC, kernels

FORMS = {"f0": "form0", "f1": "form1", "f0e": "form0e"}          # the unit's suffix -> the namespace of its kernels


def _march(ns, grad, fast, multi, surf, stats, small, nch, rope):
    b = lambda v: "Lb1E" if v else "Lb0E"                                    # noqa: E731
    return (f"_ZN3exa{len(ns)}{ns}19renderFrameKdKernelI{b(grad)}{b(fast)}Li{multi}E{b(surf)}Li{stats}E{b(small)}Li{nch}E{b(rope)}"
            "EEvNS_10RenderArgsE")


def _march_cases():
    """(test id, unit, kernel, VGPR budget) of the shipped march variants"""
    for surf in (False, True):
        s = "surfaces" if surf else "dvr"
        for grad in (False, True):
            g = "gradient" if grad else "plain"
            # one channel on the rope walk.  32-bit address form (every BASELINE configuration): seven waves per SIMD = 72
            # VGPRs; fields beyond 4 GiB: six waves = 80
            yield f"rope-{g}-{s}-small", "exa_kernels_f1r.o", _march("form1", grad, True, 0, surf, 0, True, 0, True), 72
            yield f"rope-{g}-{s}-large", "exa_kernels_f1r.o", _march("form1", grad, True, 0, surf, 0, False, 0, True), 80
        for small in (True, False):                                                              # the stack walk: six waves
            yield (f"stack-{s}-{'small' if small else 'large'}", "exa_kernels_f1.o",
                   _march("form1", True, True, 0, surf, 0, small, 0, False), 80)
        for nch, budget in ((2, 96), (3, 128), (4, 128)):                                        # interleaved channels: five / four / four waves
            yield f"rope-{nch}ch-{s}", "exa_kernels_f1r.o", _march("form1", True, True, 2, surf, 0, True, nch, True), budget


MARCH = list(_march_cases())


def _sample(ns):
    shapes = [(64, 1, 1), (16, 4, 1), (8, 8, 1), (4, 4, 4)]
    return ([f"_ZN3exa{len(ns)}{ns}18samplePointsKernelILb{g}EEEvNS_10SampleArgsE" for g in (0, 1)]
            + [f"_ZN3exa{len(ns)}{ns}22samplePointsNormKernelENS_10SampleArgsE"]
            + [f"_ZN3exa{len(ns)}{ns}16sampleGridKernelILi{x}ELi{y}ELi{z}ELb{u}EEEvNS_10SampleArgsE" for x, y, z in shapes for u in (0, 1)])


def _stream(ns):
    return [f"_ZN3exa{len(ns)}{ns}17streamlinesKernelILb{emit}ELb{norm}EEEvNS_10StreamArgsE" for emit in (0, 1) for norm in (0, 1)]


# A unit of one concern: `kernels` are there, each exactly once (a mangled name, or a part of one); every kernel name of the
# unit contains `word` — so no unit holds another's kernels, which is what the older "the other units are unchanged by the
# iso-mesh / histogram unit" tests asked; `exact`: it holds nothing but `kernels`; every kernel of it stays within `vgprs`.
Unit = collections.namedtuple("Unit", "word kernels exact vgprs")
OWN = {}
for f, ns in FORMS.items():
    OWN[f"exa_sample_{f}.o"] = Unit("sample", _sample(ns), False, None)
    OWN[f"exa_stream_{f}.o"] = Unit("streamlinesKernel", _stream(ns), False, None)
OWN["exa_isomesh.o"] = Unit("iso", ["isoCubeKernel", "isoPointKernel", "isoScanChunksKernel", "isoScanTopKernel",
                                    "isoEmitVerticesKernel", "isoEmitTrianglesKernel"], False, 64)
OWN["exa_histogram.o"] = Unit("histKernel", ["histKernelILb1E", "histKernelILb0E"], True, 64)     # <true>: bins, <false>: range only
# ... and the units of which only a gfx950 kernel is asked: the forms no BASELINE configuration renders with, the LBVH build
ANY = ["exa_kernels_f0.o", "exa_kernels_f0e.o", "exa_kernels_f0r.o", "exa_kernels_f0er.o", "exa_lbvh.o"]
UNITS = sorted({unit for _, unit, _, _ in MARCH} | set(OWN) | set(ANY))


@pytest.mark.parametrize("unit,kernel,budget", [c[1:] for c in MARCH], ids=[c[0] for c in MARCH])
def test_march_kernel_keeps_its_occupancy_without_scratch(unit, kernel, budget):
    r = kernels(unit)[kernel]
    assert r.vgpr <= budget and r.scratch == 0 and r.vgpr_spill == 0, (unit, kernel, r)


@pytest.mark.parametrize("unit,want", [(u, w) for u in sorted(OWN) for w in OWN[u].kernels])
def test_kernel_is_there_without_scratch_and_spills(unit, want):
    found = [r for name, r in kernels(unit).items() if want in name]
    assert len(found) == 1, (unit, want, sorted(kernels(unit)))
    r = found[0]
    assert r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0, (unit, want, r)


@pytest.mark.parametrize("unit", sorted(OWN))
def test_unit_holds_only_its_own_kernels(unit):
    u, k = OWN[unit], kernels(unit)
    assert k and all(u.word in name for name in k), (unit, sorted(k))
    if u.exact:
        assert len(k) == len(u.kernels), (unit, sorted(k))
    if u.vgprs is not None:                 # every kernel of the unit, also one that `kernels` does not name
        for name, r in k.items():
            assert r.vgpr <= u.vgprs and r.scratch == 0 and r.vgpr_spill == 0 and r.sgpr_spill == 0, (unit, name, r)


def _make(*args):
    return subprocess.run(["make", "-C", CSRC, *args], check=True, capture_output=True, text=True).stdout


def test_every_device_object_of_the_build_has_expectations_here():
    assert UNITS == sorted(_make("-s", "print-device-objs").split())
    for unit in UNITS:
        assert kernels(unit), unit + " holds no gfx950 kernel"


def test_variant_build_compiles_every_object_once_with_its_defines(tmp_path):
    """`make O=dir OUT=lib DEFS=... lib` (tools/ab_variants.sh) is the default build's recipe: nothing is compiled, the
    command lines are read"""
    d, probe = str(tmp_path), "-DEXA_PROBE_DEFINE"
    lines = [ln.split() for ln in _make("-n", "-B", f"O={d}", f"OUT={d}/l.so", f"DEFS={probe}", "lib").splitlines() if " -o " in ln]
    host = ["exa_create.o", "exa_frame.o", "exa_probe.o", "exa_streamlines.o", "exa_stats.o", "exa_module.o"]
    compiles = {ln[ln.index("-o") + 1]: ln for ln in lines if "-c" in ln}
    links = [ln for ln in lines if "-c" not in ln]
    assert len(compiles) + len(links) == len(lines) and len(links) == 1, lines
    assert sorted(compiles) == sorted(f"{d}/{o}" for o in UNITS + host + ["exa_prep.o"])
    for out, ln in compiles.items():
        assert (probe in ln) == (not out.endswith("/exa_prep.o")), ln
        assert ("--offload-arch=gfx950" in ln) == (probe in ln), ln
    assert links[0][links[0].index("-o") + 1] == f"{d}/l.so" and set(compiles) <= set(links[0]), links[0]
