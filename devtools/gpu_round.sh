#!/bin/bash
# one GPU-box session: parity tests, smoke, bench --full, rocprofv3 kernel traces of the inference and the training leg;
# logs and traces go to $SIR_OUT_DIR (default out/ in the repository root)
set -o pipefail
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$(realpath -m "${SIR_OUT_DIR:-$R/out}")
mkdir -p $O
cd $R
timeout -k 10 900 python -m pytest tests -q -m gpu -s > $O/gpu_tests.log 2>&1; rc=$?
tail -5 $O/gpu_tests.log
if [ $rc -ne 0 ]; then grep -E "^(FAILED|ERROR)|Error|assert " $O/gpu_tests.log | head -40; fi
if [ $rc -gt 1 ]; then echo "pytest crashed rc=$rc"; exit $rc; fi
timeout -k 10 300 python __graft_entry__.py smoke > $O/smoke.log 2>&1 || { tail -20 $O/smoke.log; exit 1; }
tail -2 $O/smoke.log
timeout -k 10 600 python bench.py --full --steps ${STEPS:-100} --warmup 20 > $O/bench.log 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cat $O/bench.log
if [ "${PROF:-1}" = "1" ]; then
cd /tmp && export TMPDIR=/tmp
# inference leg alone, strictly serial (one stream) so that per-kernel averages are the kernels' own durations
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o infer -- python3 $R/bench.py --steps 30 --warmup 5 --repeats 1 --streams 1 > $O/prof.log 2>&1 || { tail -20 $O/prof.log; exit 1; }
# training legs (plain + augmented) with a short inference part
timeout -k 10 600 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o train -- python3 $R/bench.py --full --steps 2 --warmup 1 --repeats 1 --train-steps 30 --no-cpu-baseline --no-dist-leg --no-dropin --sustain-seconds 0 --streams 1 > $O/prof_train.log 2>&1 || { tail -20 $O/prof_train.log; exit 1; }
ls -R $O/prof | head -20
fi
