#!/bin/bash
# kernel trace (timeline) of a few training steps: $SIR_OUT_DIR/trt/tr_kernel_trace.csv (default out/), analysed by
# devtools/trace_gaps.py
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$(realpath -m "${SIR_OUT_DIR:-$R/out}")
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
rm -rf $O/trt
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trt -o tr -- python3 $R/bench.py --full --steps 3 --warmup 2 --train-steps ${TRAIN_STEPS:-12} --no-cpu-baseline --streams 1 > $O/trt.log 2>&1 || { tail -20 $O/trt.log; exit 1; }
ls $O/trt
cd $R && python devtools/trace_gaps.py $O/trt/tr_kernel_trace.csv
