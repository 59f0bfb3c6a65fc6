"""Registers, scratch and LDS of the kernels in the gfx950 code objects the build left in csrc/ (no GPU needed): the one reader
of them, for tests/test_kernel_resources.py and for the command line:

    python tests/code_objects.py [--obj exa_kernels_f1r.o] [regex]      (after `make -C owlexabrick_amd/csrc`)
"""
import argparse
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "owlexabrick_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"

# of the kernel's entry in the code object's metadata: .vgpr_count, .sgpr_count, .private_segment_fixed_size (bytes per
# lane), .vgpr_spill_count, .sgpr_spill_count, .group_segment_fixed_size (bytes)
Resources = collections.namedtuple("Resources", "vgpr sgpr scratch vgpr_spill sgpr_spill lds")
_KEYS = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
         "group_segment_fixed_size")


def kernels(obj, csrc=CSRC):
    """{mangled name: Resources} of the gfx950 code object embedded in the host object file csrc/obj.  A missing object is a
    failure, never a skip: build() makes them all."""
    path = os.path.join(csrc, obj)
    assert os.path.exists(path), f"{path} was not built (run __graft_entry__.build())"
    return _read(path, os.stat(path).st_mtime_ns)


@functools.lru_cache(maxsize=None)
def _read(path, mtime):
    tools = [os.path.join(LLVM, t) for t in ("llvm-objdump", "llvm-readelf")]
    assert all(map(os.path.exists, tools)), f"the ROCm llvm tools ({LLVM}) are needed to read {path}"
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(path, os.path.join(d, "k.o"))
        subprocess.run([tools[0], "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = [f for f in os.listdir(d) if "gfx950" in f]
        assert co, "no gfx950 code object in " + path
        notes = subprocess.run([tools[1], "--notes", co[0]], cwd=d, check=True, capture_output=True, text=True).stdout
    out = {}
    for entry in notes.split("\n  - ")[1:]:                     # amdhsa.kernels: one list item per kernel
        keys = dict(re.findall(r"^    \.(\w+): +(\S+)$", entry, re.M))          # its own keys, not those of its .args
        if "name" in keys:
            out[keys["name"]] = Resources(*(int(keys[k]) for k in _KEYS))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--obj", default="exa_kernels_f0.o")
    ap.add_argument("regex", nargs="?", default="")
    a = ap.parse_args()
    for name, r in kernels(a.obj).items():
        if re.search(a.regex, name):
            print(f"vgpr {r.vgpr:3d} sgpr {r.sgpr:3d} scratch {r.scratch:4d} spill {r.vgpr_spill:3d} lds {r.lds:5d}  {name}")
