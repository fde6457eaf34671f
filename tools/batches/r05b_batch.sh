#!/usr/bin/env bash
# round 5, second batch: the whole GPU suite again (after the K x N test fix), the bench line with live counters, and the
# rocprofv3 kernel stats of the same bench command
cd "$(dirname "$0")/../.." || exit 1
: "${OUT:?set OUT to the directory that receives the outputs of this batch}"
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) && export OUT
python -m pytest tests -x -q -m gpu > $OUT/r05b_pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $OUT/r05b_pytest_gpu.log
tail -4 $OUT/r05b_pytest_gpu.log
python bench.py --full --steps 20 --warmup 5 > $OUT/r05b_bench.json 2> $OUT/r05b_bench.err; echo "bench rc=$?"
tail -c 1500 $OUT/r05b_bench.json; echo; wc -c $OUT/r05b_bench.json; tail -3 $OUT/r05b_bench.err
export TMPDIR=/tmp
R=$PWD
(cd /tmp && MM_BENCH_NO_PMC=1 rocprofv3 --kernel-trace --stats -d $OUT/r05b_prof -o bench --output-format csv -- python $R/bench.py --full --steps 20 --warmup 5 --no-cpu-baseline > $OUT/r05b_bench_under_rocprof.json 2> $OUT/r05b_rocprof.err)
find $OUT/r05b_prof -name "*kernel_stats.csv" | head -2
head -8 $(find $OUT/r05b_prof -name "*kernel_stats.csv" | head -1)
