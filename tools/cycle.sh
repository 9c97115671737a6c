#!/bin/bash
# GPU cycle: smoke, a bench line, a rocprofv3 kernel-stats profile + idle gaps, then the GPU suite.
#   usage: bash tools/cycle.sh TAG
set -o pipefail
TAG=${1:-r05}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT" || exit 1
timeout -k 10 200 python -u -c 'import __graft_entry__ as g; g.smoke()' > $OUT/${TAG}_smoke.log 2>&1 || { tail -30 $OUT/${TAG}_smoke.log; exit 1; }
tail -2 $OUT/${TAG}_smoke.log
timeout -k 10 400 python3 bench.py --full > $OUT/${TAG}_bench.log 2>&1 || { tail -20 $OUT/${TAG}_bench.log; exit 1; }
tail -1 $OUT/${TAG}_bench.log | cut -c1-600
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/${TAG}_prof -o run --output-format csv -- python3 bench.py --no-cpu-baseline --no-extra > $OUT/${TAG}_prof.log 2>&1 || { tail -20 $OUT/${TAG}_prof.log; exit 1; }
python tools/prof_summary.py $OUT/${TAG}_prof 13 40 > $OUT/${TAG}_summary.txt 2>&1
python tools/gaps.py $OUT/${TAG}_prof > $OUT/${TAG}_gaps.txt 2>&1
head -30 $OUT/${TAG}_summary.txt
timeout -k 10 500 python -u -m pytest tests -m gpu -q --timeout 200 --timeout-method thread > $OUT/${TAG}_gputest.log 2>&1; echo "gputest rc=$?"
tail -15 $OUT/${TAG}_gputest.log
