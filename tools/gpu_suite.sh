#!/bin/bash
# the whole GPU suite (incl. the configs[2]/[4] scale tests), then the bench line with every leg (bench.py --full)
# usage: tools/gpu_suite.sh <output dir>; each step has a time limit, and nothing runs behind one that failed
export TMPDIR=/tmp
out=${1:?usage: tools/gpu_suite.sh <output dir>}
mkdir -p "$out"
( time timeout -k 10 1500 python -m pytest tests -m gpu -x -q --durations=8 ) > "$out/tests.log" 2>&1
rc=$?
tail -25 "$out/tests.log"
[ $rc -eq 0 ] || exit $rc
( time timeout -k 10 900 python bench.py --full ) > "$out/bench.json" 2> "$out/bench.err"
rc=$?
tail -5 "$out/bench.err"
cat "$out/bench.json"
exit $rc
