"""The kernels of exa_hip_isosurface (csrc/exa_isomesh.hip), read from the gfx950 code object the build left in csrc/ (no GPU
needed): the unit exists, holds the cube pass, the point pass, the scans and the emit kernels, and every kernel in it runs
without scratch and without spilled registers.  A missing object is a failure: build() makes it."""
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "owlexabrick_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
OBJ = "exa_isomesh.o"
KERNELS = ["isoCubeKernel", "isoPointKernel", "isoScanChunksKernel", "isoScanTopKernel", "isoEmitVerticesKernel",
           "isoEmitTrianglesKernel"]


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


def test_isomesh_unit_holds_its_kernels_for_gfx950():
    k = _kernels(OBJ)
    for want in KERNELS:
        assert sum(1 for name in k if want in name) == 1, (want, sorted(k))
    assert all("iso" in name for name in k), sorted(k)          # nothing of the renderer or of the probes is compiled here


def test_isomesh_kernels_have_no_scratch_and_no_spills():
    k = _kernels(OBJ)
    assert len(k) >= len(KERNELS)
    for name, (vgpr, scratch, vspill, sspill) in k.items():
        assert scratch == 0 and vspill == 0 and sspill == 0, (name, vgpr, scratch, vspill, sspill)
        assert vgpr <= 64, (name, vgpr)                          # memory-bound passes: full occupancy


def test_probe_units_are_unchanged_by_the_isomesh_unit():
    # the iso kernels live in their own unit: tests/test_sample_kernels.py requires the probe units to hold only sample* kernels
    for obj in ("exa_sample_f0.o", "exa_sample_f1.o", "exa_sample_f0e.o"):
        assert not any(want in name for name in _kernels(obj) for want in KERNELS), obj
