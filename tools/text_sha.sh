#!/bin/bash
# sha256 (first 16 hex digits) and size of the gfx950 .text of every object in csrc/ whose gfx950 code object has one
# (after `make -C owlexabrick_amd/csrc`): the march, sample, iso-mesh and LBVH kernels; the host objects hold no device
# code and print nothing.  A refactoring that is meant to leave the machine code alone shows the same hashes before and
# after.  usage: tools/text_sha.sh [csrc directory]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CS=$(cd "${1:-$ROOT/owlexabrick_amd/csrc}" && pwd)
for f in "$CS"/*.o; do
  TMP=$(mktemp -d)
  ( cd "$TMP" && cp "$f" k.o && /opt/rocm/lib/llvm/bin/llvm-objdump --offloading k.o > /dev/null 2>&1 \
    && CO=$(ls | grep gfx950) && [ -n "$CO" ] \
    && /opt/rocm/lib/llvm/bin/llvm-objcopy -O binary --only-section=.text "$CO" text.bin 2> /dev/null && [ -s text.bin ] \
    && printf "%s  %s bytes  %s\n" "$(sha256sum text.bin | cut -c1-16)" "$(stat -c %s text.bin)" "$(basename "$f")" ) || true
  rm -rf "$TMP"
done
