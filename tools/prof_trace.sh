#!/bin/bash
# rocprofv3 kernel trace + stats of bench.py (run on the GPU machine from the repo root).  Output: $PROF_OUT/<tag>_kt_<workload>/
# (PROF_OUT: prof_out/)
# usage: tools/prof_trace.sh <tag> <workload> [extra bench args]
set -u
TAG=${1:-rXX}; W=${2:-4k10-gop}; shift 2
ROOT=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=$(realpath -m ${PROF_OUT:-$ROOT/prof_out}); mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_kt_$W -- python3 $ROOT/bench.py --workload $W --steps 3 --warmup 1 --full --no-cpu-baseline --no-e2e "$@" \
  > $OUT/${TAG}_bench_${W}_under_rocprof.json 2> $OUT/${TAG}_kt_$W.err || { tail -5 $OUT/${TAG}_kt_$W.err; exit 1; }
ls -la $OUT/${TAG}_kt_$W/*/ | head
