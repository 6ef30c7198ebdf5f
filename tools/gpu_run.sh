# GPU-box script: tests, then bench, then an optional rocprofv3 kernel-trace pass.
# usage: bash tools/gpu_run.sh TAG [prof]
set -u
TAG=${1:-run}
R=$GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $R/$OUT  # where this script writes its results (under $R)
cd $R
timeout -k 10 700 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread -p no:cacheprovider > $OUT/$TAG.pytest.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -15 $OUT/$TAG.pytest.log
if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then exit $rc; fi
timeout -k 10 300 python bench.py --full --steps 10 --warmup 3 --verbose > $OUT/$TAG.bench.json 2> $OUT/$TAG.bench.err
rc=$?
echo "bench rc=$rc"; cat $OUT/$TAG.bench.json; grep -v amdgpu.ids $OUT/$TAG.bench.err | head -40
if [ $rc -ne 0 ]; then exit $rc; fi
if [ "${2:-}" = "prof" ] || [ "${3:-}" = "prof" ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $R/$OUT/$TAG.prof -o run --output-format csv -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline > $R/$OUT/$TAG.prof.log 2>&1
  echo "rocprof rc=$?"
  head -12 $R/$OUT/$TAG.prof/run_kernel_stats.csv | cut -c1-160
fi
if [ "${2:-}" = "pmc" ] || [ "${3:-}" = "pmc" ]; then
  cd /tmp && export TMPDIR=/tmp
  i=0
  for CN in "FETCH_SIZE" "WRITE_SIZE" "GRBM_GUI_ACTIVE SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_VALU_MFMA_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT"; do
    i=$((i+1))
    timeout -k 10 300 rocprofv3 --pmc $CN --output-format csv -d $R/$OUT/$TAG.pmc$i -o run -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline > $R/$OUT/$TAG.pmc$i.log 2>&1
    rc=$?
    echo "pmc pass $i rc=$rc"
    if [ $rc -ne 0 ]; then tail -5 $R/$OUT/$TAG.pmc$i.log; exit $rc; fi
  done
  cd $R && python3 tools/pmc_summary.py $OUT/$TAG.pmc_summary.json $OUT/$TAG.pmc1 $OUT/$TAG.pmc2 $OUT/$TAG.pmc3
fi
