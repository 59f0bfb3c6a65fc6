#!/usr/bin/env python3
"""sha256 (first 16 hex digits) of the instructions of every gfx950 kernel in the objects of a csrc/ build, kernel by
kernel, where tools/text_sha.sh hashes an object's whole .text: a change that adds kernels to a unit, or members at the end
of a kernel's argument struct, shows the same hashes for the kernels it is meant to leave alone.

    tools/kernel_sha.py [--csrc DIR] [--obj exa_kernels_f1r.o ...] [regex]          one line per kernel
    tools/kernel_sha.py --against OTHER_CSRC [--obj ...] [regex]                   compares with another build's objects

What is hashed is the disassembly of the kernel's symbol without addresses and encodings (branches are relative: they print
as offsets from the symbol)."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def kernel_hashes(path):
    """{mangled kernel name: (hash, instructions)} of the gfx950 code object in the host object `path`"""
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(path, os.path.join(d, "k.o"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "k.o"], cwd=d, check=True, capture_output=True)
        co = [f for f in os.listdir(d) if "gfx950" in f]
        if not co:
            return {}
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co[0]], cwd=d, check=True, capture_output=True, text=True).stdout
        names = set(re.findall(r"^    \.name: +(\S+)$", notes, re.M))
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co[0]],
                             cwd=d, check=True, capture_output=True, text=True).stdout
    out, name, lines = {}, None, []
    for ln in dis.splitlines() + ["<end>:"]:
        m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", ln.strip())
        if m:
            if name in names:
                out[name] = (hashlib.sha256("\n".join(lines).encode()).hexdigest()[:16], len(lines))
            name, lines = m.group(1), []
        elif ln.strip():
            lines.append(re.sub(r"\s*//.*$", "", ln.strip()))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--csrc", default=os.path.join(ROOT, "owlexabrick_amd", "csrc"))
    ap.add_argument("--against", default=None, help="csrc directory of another build: report kernels that differ, are new or are gone")
    ap.add_argument("--obj", action="append", default=[])
    ap.add_argument("regex", nargs="?", default="")
    a = ap.parse_args()
    objs = a.obj or sorted(f for f in os.listdir(a.csrc) if f.endswith(".o"))
    differ = 0
    for o in objs:
        mine = {k: v for k, v in kernel_hashes(os.path.join(a.csrc, o)).items() if re.search(a.regex, k)}
        if a.against is None:
            for k, (h, n) in sorted(mine.items()):
                print(f"{h}  {n:6d} instructions  {o}  {k}")
            continue
        other_path = os.path.join(a.against, o)
        other = {k: v for k, v in kernel_hashes(other_path).items() if re.search(a.regex, k)} if os.path.exists(other_path) else {}
        same = sum(1 for k in mine if k in other and mine[k] == other[k])
        changed = sorted(k for k in mine if k in other and mine[k] != other[k])
        print(f"{o}: {same} kernels identical, {len(changed)} differ, {len(set(mine) - set(other))} new, {len(set(other) - set(mine))} gone")
        for k in changed:
            print(f"  differs  {k}  {other[k][0]} ({other[k][1]} instructions) -> {mine[k][0]} ({mine[k][1]})")
        for k in sorted(set(mine) - set(other)):
            print(f"  new      {k}  {mine[k][0]} ({mine[k][1]} instructions)")
        for k in sorted(set(other) - set(mine)):
            print(f"  gone     {k}")
        differ += len(changed) + len(set(other) - set(mine))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
