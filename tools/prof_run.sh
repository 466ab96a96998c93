#!/bin/bash
# rocprofv3 kernel-trace + stats of a short bench run into bench_out/$1 (extra bench args after it).
set -u
ROOT=$(pwd); export TMPDIR=/tmp
name=$1; shift
mkdir -p bench_out
timeout -k 10 ${PROF_TIMEOUT:-400} rocprofv3 --kernel-trace --stats --output-format csv \
    -d "$ROOT/bench_out/$name" -o run -- python "$ROOT/bench.py" --full --steps 5 --warmup 2 --no-cpu-baseline "$@" \
    > bench_out/$name.log 2>&1
rc=$?; echo "prof $name rc=$rc"; grep '^{' bench_out/$name.log | cut -c1-300
exit $rc
