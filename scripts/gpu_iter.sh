#!/bin/bash
# Iteration loop on the GPU box: parity tests (stop at first failure), then a short C3 bench line.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
RESULTS=${RESULTS:-results}  # where this script writes its logs and result lines
export TMPDIR=/tmp
mkdir -p $RESULTS
timeout -k 10 400 python3 -u -m pytest tests -m "gpu and not slow" -x -q --timeout 120 --timeout-method thread > $RESULTS/tests.log 2>&1
rc=$?; tail -3 $RESULTS/tests.log; [ $rc -eq 0 ] || { grep -E "FAIL|Error|assert" $RESULTS/tests.log | head -30; exit $rc; }
timeout -k 10 300 python3 -u bench.py --full --steps ${STEPS:-3} --no-cpu-baseline --kernel-iters 20 ${BENCH_ARGS:-} > $RESULTS/iter_bench.json 2> $RESULTS/iter_bench.err
rc=$?; tail -2 $RESULTS/iter_bench.err; [ $rc -eq 0 ] || exit $rc
python3 -c "
import json; d=json.loads(open('$RESULTS/iter_bench.json').read().strip().splitlines()[-1])
print('pods/s', round(d['value']), 'ms/step', round(d['ms_per_step'],2), 'rounds', d['device_rounds'], {k: round(v*1e3,2) for k,v in d['roofline']['kernels_ms'].items()})"
