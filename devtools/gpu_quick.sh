#!/bin/bash
# quick GPU check: model/train/pipeline parity tests, then one bench --full run (prints the kernel table); logs in
# $SIR_OUT_DIR (default out/)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$(realpath -m "${SIR_OUT_DIR:-$R/out}")
cd $R; mkdir -p $O
timeout -k 10 600 python -m pytest tests/test_features_gpu.py tests/test_model_gpu.py tests/test_train_gpu.py tests/test_pipeline_gpu.py -q -x > $O/quick_tests.log 2>&1; rc=$?
tail -3 $O/quick_tests.log
if [ $rc -ne 0 ]; then grep -E "Error|assert|FAILED" $O/quick_tests.log | head -20; exit $rc; fi
timeout -k 10 300 python bench.py --full --steps 100 --warmup 20 --no-cpu-baseline $BENCH_ARGS > $O/quick_bench.json 2> $O/quick_bench.err || { tail -5 $O/quick_bench.err; exit 1; }
python - <<PY
import json
d=json.loads(open("$O/quick_bench.json").read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], {k: round(x*1e3,1) for k,x in d["kernels_avg_ms"].items()}, "train", d.get("train",{}).get("value"), d.get("train",{}).get("ms_per_step"))
PY
