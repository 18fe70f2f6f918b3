#!/bin/bash
# Runs on an MI355X: the three rocprofv3 passes behind profiles/ (kernel trace + stats; PMC FETCH_SIZE; PMC
# WRITE_SIZE in separate runs, as MI355X_MICROARCH.md prescribes).  Raw outputs land in $OUT/prof/{stats,fetch,write}, the
# condensed files in $OUT/profiles (OUT defaults to profile_out).  bench.py runs with --full: the per-kernel measurements
# and the whole result line are part of what is profiled and kept.
set -e
export ROUND=${ROUND:-r06}
OUT=${OUT:-profile_out}
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
rm -rf $OUT/prof && mkdir -p $OUT/prof
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof/stats -o run -- python3 bench.py --full --steps 30 --warmup 3 --no-cpu-baseline --no-shapes --no-dp-probe --no-other-configs > $OUT/prof/stats.log 2>&1
# the two counter passes run with the filler roles off (a launch's bytes are then its own role's: with them on, the narrow sites'
# launches also read the slabs of earlier sites / convolutions, bytes that the closing reductions read otherwise)
export ALIGNQ_FILL=0
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $OUT/prof/fetch -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-shapes --no-dp-probe --no-other-configs > $OUT/prof/fetch.log 2>&1
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $OUT/prof/write -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-shapes --no-dp-probe --no-other-configs > $OUT/prof/write.log 2>&1
unset ALIGNQ_FILL
find $OUT/prof -name "*.csv" | head -20
# keep the merge-back under the 64 MiB cap: drop the per-dispatch traces of the PMC runs except the counter tables
find $OUT/prof/fetch $OUT/prof/write -name "*kernel_trace.csv" -delete
du -sh $OUT/prof
python3 tools/summarise_profiles.py $OUT/prof $OUT/profiles
grep "^{\"metric" $OUT/prof/stats.log > $OUT/profiles/bench_under_rocprof.json || true
rm -rf $OUT/prof
python3 bench.py --full --steps 200 --warmup 20 > $OUT/profiles/bench_n1.json 2> $OUT/profiles/bench_n1.err
tail -c 600 $OUT/profiles/bench_n1.json
