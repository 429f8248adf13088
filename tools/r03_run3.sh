#!/bin/bash
# round 3: secondary bench lines (bf16 mode, configs[3] shape, train modes, iter) -> gpurun_out/r03_bench_*.json
cd "$GRAFT_REPO_ROOT"
mkdir -p gpurun_out
OUT=${OUT:-out}; mkdir -p "$OUT"
run() { name=$1; shift; timeout -k 10 400 python bench.py --full "$@" > "$OUT"/r03_bench_$name.json 2> "$OUT"/r03_bench_$name.err; echo "$name rc=$?"; python - <<EOF2
import json
try:
    d=json.loads(open("$OUT/r03_bench_$name.json").read().strip().splitlines()[-1]); r=d.get("roofline",{})
    print("   ", round(d["value"],1), d["unit"], round(d["ms_per_step"],3), "ms; frac", round(r.get("frac",0),3), r.get("bound"), "path", round(r.get("path",0),3), "pipelined", (d.get("pipelined") or {}).get("value"))
except Exception as e: print("   ERR", e)
EOF2
}
run c1_bf16 --dtype bf16 --steps 20 --warmup 3 --no-cpu-baseline
run c3_bf16 --workload c3 --steps 10 --warmup 2 --no-cpu-baseline
run c3_f32 --workload c3 --dtype f32 --steps 10 --warmup 2 --no-cpu-baseline
run train_f32 --mode train --steps 20 --warmup 3
run train_bf16 --mode train --dtype bf16 --steps 20 --warmup 3
run train_geo_40960 --mode train-geo --steps 5 --warmup 2
run train_geo_65536 --mode train-geo --num-pt 65536 --steps 5 --warmup 2
run iter_f32 --mode iter --steps 10 --warmup 2
