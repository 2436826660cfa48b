#!/bin/bash
# Default bench line (the judged configuration) then the rocprof trace + PMC passes (gpu_prof.sh).
set -o pipefail
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
RESULTS=${RESULTS:-results}  # where this script writes its logs and result lines
export TMPDIR=/tmp
mkdir -p $RESULTS
echo "== bench (default)"
timeout -k 10 600 python3 -u bench.py --full ${BENCH_ARGS:-} > $RESULTS/bench.json 2> $RESULTS/bench.err
rc=$?; echo "bench rc=$rc"; tail -3 $RESULTS/bench.err; cat $RESULTS/bench.json; [ $rc -eq 0 ] || exit $rc
[ -n "$NO_PROF" ] && exit 0
bash scripts/gpu_prof.sh
