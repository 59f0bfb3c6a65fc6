#!/bin/bash
# Builds libexa_hip variants with different -D... build-time constants (exa_device.h: EXA_MARCH_WAVES, EXA_KD_STACK, EXA_SEG_QUEUE ...) (here, no GPU needed) into build/variants/ (git-ignored,
# travels to the GPU box), and on the GPU box times each with bench.py on C4, twice, interleaved.
#   tools/ab_variants.sh build  base:"" name1:"-DEXA_KD_STACK=3 -DEXA_SEG_QUEUE=5 ..." name2:"..."
#       each by the module's own recipe (csrc/Makefile); KFLAGS=... in front: other flags for the kernel translation units than the Makefile's, KFLAGS= none
#   tools/ab_variants.sh run [bench args]      -> gpurun_out/variants/results.txt
#       ends at the first run that fails, with that run's exit status
set -u -o pipefail
ROOT=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
LIBS="$ROOT/build/variants"
OUT="$ROOT/gpurun_out/variants"
mode=$1; shift
if [ "$mode" = build ]; then
  mkdir -p "$LIBS"
  for spec in "$@"; do
    name=${spec%%:*}; defs=${spec#*:}
    mkdir -p "$OUT/obj_$name"
    # the module's own recipe (csrc/Makefile), with this variant's objects and library beside the default build's
    make -C "$ROOT/owlexabrick_amd/csrc" -s -j16 O="$OUT/obj_$name" OUT="$LIBS/libexa_hip_$name.so" DEFS="$defs" ${KFLAGS+"KFLAGS=$KFLAGS"} lib || exit
    echo "built $name ($defs)"
  done
  ls -la "$LIBS"/*.so
else
  mkdir -p "$OUT"
  : > "$OUT/results.txt"
  for rep in 1 2; do
    for so in "$LIBS"/libexa_hip_*.so; do
      name=$(basename "$so" .so); name=${name#libexa_hip_}
      EXA_HIP_LIB="$so" timeout -k 10 120 python3 "$ROOT/bench.py" --full --cpu-baseline off --pmc off --in-flight 1 --steps 20 --warmup 3 "$@" > "$OUT/$name.$rep.json" 2> "$OUT/$name.$rep.err"
      status=$?
      if [ $status -ne 0 ]; then        # nothing more is started on a GPU that a run has failed or hung on
        echo "$name rep $rep failed (exit status $status)" | tee -a "$OUT/results.txt"; tail -3 "$OUT/$name.$rep.err"
        exit $status
      fi
      python3 -c "import json,sys; d=json.loads(open('$OUT/$name.$rep.json').read().strip().splitlines()[-1]); print('%-12s rep $rep  %.3f ms/frame  kernel %.3f ms  %.2f fps' % ('$name', d['ms_per_step'], d['roofline']['kernel_ms'], d['value']))" | tee -a "$OUT/results.txt" || exit
    done
  done
fi
