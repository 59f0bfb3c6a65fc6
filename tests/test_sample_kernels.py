"""The point probes' kernels (exa_hip_sample_points / exa_hip_resample), read from the gfx950 code objects the build left in
csrc/ (no GPU needed): every sampler variant — basis form 0, form 1, form 0 with empty cells — has its translation unit, and
its points and grid kernels run without scratch and without spilled registers.  A missing object is a failure: build()
makes them."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "owlexabrick_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"

VARIANTS = {"exa_sample_f0.o": "form0", "exa_sample_f1.o": "form1", "exa_sample_f0e.o": "form0e"}
SHAPES = [(64, 1, 1), (16, 4, 1), (8, 8, 1), (4, 4, 4)]


def _kernels(obj):
    """{mangled name: (vgprs, scratch bytes, spilled vgprs, spilled sgprs)} of the gfx950 code object in a host object file"""
    path = os.path.join(CSRC, obj)
    assert os.path.exists(path), f"{obj} was not built (run __graft_entry__.build())"
    assert os.path.exists(os.path.join(LLVM, "llvm-objdump")), "the ROCm llvm tools are needed to read the code objects"
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(path, os.path.join(d, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = [f for f in os.listdir(d) if "gfx950" in f]
        assert co, "no gfx950 code object in " + obj
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co[0]], cwd=d, check=True, capture_output=True,
                               text=True).stdout
    out = {}
    for block in notes.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        if not name or name.group(1).endswith(".kd"):
            continue
        get = lambda key: int(re.search(r"\." + key + r":\s+(\d+)", block).group(1))   # noqa: E731
        out[name.group(1)] = (get("vgpr_count"), get("private_segment_fixed_size"), get("vgpr_spill_count"),
                              get("sgpr_spill_count"))
    return out


def _points(ns, grad):
    return f"_ZN3exa{len(ns)}{ns}18samplePointsKernelILb{int(grad)}EEEvNS_10SampleArgsE"


def _grid(ns, shape, uniform):
    x, y, z = shape
    return f"_ZN3exa{len(ns)}{ns}16sampleGridKernelILi{x}ELi{y}ELi{z}ELb{int(uniform)}EEEvNS_10SampleArgsE"


@pytest.mark.parametrize("obj", sorted(VARIANTS))
def test_probe_kernels_have_no_scratch_and_no_spills(obj):
    ns = VARIANTS[obj]
    k = _kernels(obj)
    want = [_points(ns, g) for g in (False, True)] + [f"_ZN3exa{len(ns)}{ns}22samplePointsNormKernelENS_10SampleArgsE"]
    want += [_grid(ns, s, u) for s in SHAPES for u in (False, True)]
    missing = [w for w in want if w not in k]
    assert not missing, (missing, sorted(k))
    for name in want:
        vgpr, scratch, vspill, sspill = k[name]
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, vgpr, scratch, vspill, sspill)


@pytest.mark.parametrize("obj", sorted(VARIANTS))
def test_probe_units_hold_only_the_probe_kernels(obj):
    # the renderer's kernels stay in exa_kernels_*.o: a probe unit that compiled them again would double the build
    k = _kernels(obj)
    assert all("sample" in name for name in k), sorted(k)
