#!/bin/bash
# C4 (NodeNUMAResource) evidence: geometry sweep, bench line with oracle check + CPU baseline, rocprof trace.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
RESULTS=${RESULTS:-results}  # where this script writes its logs and result lines
export TMPDIR=/tmp
mkdir -p $RESULTS/c4
SWEEP="${SWEEP:-32:8 32:2 32:1 16:4}" bash scripts/gpu_c4_sweep.sh || exit $?
echo "== bench c4 (check + cpu baseline)"
timeout -k 10 400 python3 -u bench.py --full --workload c4 ${C4_ARGS:-} --check 2000 > $RESULTS/c4/bench.json 2> $RESULTS/c4/bench.err
rc=$?; echo "bench rc=$rc"; tail -3 $RESULTS/c4/bench.err; cat $RESULTS/c4/bench.json; [ $rc -eq 0 ] || exit $rc
echo "== rocprof trace c4"
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $RESULTS/c4/trace -o run --output-format csv -- python3 -u bench.py --full --workload c4 ${C4_ARGS:-} --no-cpu-baseline > $RESULTS/c4/trace.log 2>&1
rc=$?; echo "trace rc=$rc"; tail -2 $RESULTS/c4/trace.log; exit $rc
