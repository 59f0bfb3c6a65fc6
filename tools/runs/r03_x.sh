O=${1:?usage: r03_x.sh <outdir>}
for c in 32 256 1024 4096 256 32; do
  EXA_COST_CLASSES=$c python bench.py --full --steps 20 --cpu-baseline off --pmc off > $O/r03_x_cls$c.json 2>/dev/null
  python -c "
import json; d=json.loads(open('$O/r03_x_cls$c.json').read().strip().splitlines()[-1]); print('classes $c: %.3f ms/frame kernel %.3f' % (d['ms_per_step'], d['roofline']['kernel_ms']))"
done
