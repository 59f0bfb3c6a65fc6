#!/bin/bash
# round 3, final reference measurements (burst priority, 256 cost classes)
set -o pipefail
O=gpurun_out
python bench.py --full > $O/r03_z_bench.json 2> $O/r03_z_bench.err; tail -c 300 $O/r03_z_bench.json; echo
bash tools/config_timeline.sh $O/r03_z_tl_c4 --steps 10 --pmc off
bash tools/pmc_run.sh $O/r03_z_pmc_c4 > $O/r03_z_pmc_c4.txt 2>&1; grep -E "^==|SQ_INSTS_VALU |lane util|WAVE_CYCLES|FETCH_SIZE .*GB|L2 hit|L1 miss" $O/r03_z_pmc_c4.txt | head -24
b() { name=$1; shift; python bench.py --full --cpu-baseline off --pmc on "$@" > $O/r03_z_$name.json 2> $O/r03_z_$name.err || tail -3 $O/r03_z_$name.err; }
b c2 --config c2_lanl --size 1024 --steps 50
b c3iso --config c3_gear --iso 0.5 --steps 20
b c3 --config c3_gear --steps 20
b f3 --fields 3 --steps 10
b s125 --scale 1.25 --steps 10
b closeup --camera closeup --steps 10
b c5 --size 4096 --iso 0.5 --ao --spp 16 --steps 3 --warmup 1
python - <<'PY'
import json,glob
for f in sorted(glob.glob("gpurun_out/r03_z_*.json")):
    try:
        d=json.loads(open(f).read().strip().splitlines()[-1]); r=d["roofline"]
        print("%-34s fps %.3f ms %.3f Msamples/s %.0f valu %.3f hbm %.3f traffic %.2f GB" % (f.split('/')[-1], d["value"], d["ms_per_step"], d["msamples_per_s"], r.get("frac") or 0, (r.get("hbm_measured") or {}).get("frac",0), (r.get("traffic") or 0)/1e9))
    except Exception as e: print(f, "ERR", e)
PY
echo done
