: "${OUT:?set OUT to the directory that receives the outputs of this batch}"
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd) && export OUT
R=$PWD
timeout 300 python tools/pmc_mfma.py f32 --size 16384 --out $OUT/r04d_pmc_f32_16384.json > /dev/null 2> $OUT/r04d_pmc_err.txt
timeout 300 python tools/pmc_traffic.py --what f32 --size 16384 --out $OUT/r04d_traffic_f32_16384.json > /dev/null 2>> $OUT/r04d_pmc_err.txt
cp $OUT/r04d_pmc_f32_16384.json $OUT/r04d_traffic_f32_16384.json profiles/
tail -3 $OUT/r04d_pmc_err.txt
echo "HEAD $1" > $OUT/r04d_pytest_gpu.log
MM_PERF_FLOORS=1 timeout 1200 python -m pytest tests -m gpu -x -q -rs --timeout 600 2>&1 | tail -40 >> $OUT/r04d_pytest_gpu.log
tail -8 $OUT/r04d_pytest_gpu.log
timeout 600 python bench.py --full > $OUT/r04d_bench.json 2> $OUT/r04d_bench.err; tail -2 $OUT/r04d_bench.err
cd /tmp && export TMPDIR=/tmp && timeout 600 rocprofv3 --kernel-trace --stats -d $OUT/r04d_prof -o bench --output-format csv -- python $R/bench.py --no-extra --no-cpu-baseline > $OUT/r04d_bench_under_rocprof.json 2> $OUT/r04d_rocprof.err
cd "$R"; ls $OUT/r04d_prof | head; find $OUT/r04d_prof -name "*kernel_stats.csv" | head -2
python - <<'PY'
import json, os
d=json.loads(open(os.path.join(os.environ['OUT'], 'r04d_bench.json')).read().strip().splitlines()[-1])
print(d['value'], d['ms_per_step'], d['config']['kernel'], d['roofline']['frac'], d['roofline'].get('traffic'), d['roofline'].get('mfma_util_pct'))
for w in d['workloads']: print(w.get('workload','')[:60], w.get('value'), w.get('roofline',{}).get('frac'), w.get('kernel'), w.get('error'))
print(d.get('scale_base'))
PY
