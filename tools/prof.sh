#!/bin/bash
# usage (on the GPU box, from the repo root): bash tools/prof.sh <tag> [bench args...]
# runs rocprofv3 --kernel-trace --stats on bench.py and prints a per-kernel summary (also saved under $OUT, default prof_out/ in the repo root)
TAG=$1; shift
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=${OUT:-$R/prof_out}
mkdir -p $O
cd /tmp && export TMPDIR=/tmp
# (a plain run, without --full: one timed region and nothing beside it that would be averaged into the profile.  The divisor is what bench.py
#  says it executed: "steps_executed")
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$TAG -- python $R/bench.py "$@" > $O/prof_$TAG.log 2>&1
grep '"metric"' $O/prof_$TAG.log
NST=$(grep '"metric"' $O/prof_$TAG.log | python -c "import sys, json; print(json.loads(sys.stdin.read())['steps_executed']['steps'])")
python $R/tools/prof_summary.py $(find $O/prof_$TAG -name "*kernel_stats.csv" | head -1) $NST | tee $O/prof_${TAG}_summary.txt
