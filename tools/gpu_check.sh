#!/bin/bash
# One GPU-box call: parity tests, the full bench, kernel-trace stats (dev tool).
# usage: OUT_DIR=<folder for the logs> tools/gpu_check.sh TAG [pytest-args...]
set -o pipefail
TAG=${1:-chk}; shift
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
O=${OUT_DIR:?set OUT_DIR to the folder for the logs}/$TAG
mkdir -p $O
timeout -k 10 600 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread "$@" \
  > $O/pytest.log 2>&1 || { tail -30 $O/pytest.log; exit 1; }
tail -3 $O/pytest.log
timeout -k 10 300 python -u bench.py --full > $O/bench.log 2>&1 || { tail -30 $O/bench.log; exit 1; }
tail -1 $O/bench.log
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof -o run -- \
  python3 bench.py --full --no-cpu-baseline > $O/bench_prof.log 2>&1 || { tail -30 $O/bench_prof.log; exit 1; }
echo done
