# GPU-box script: the whole -m gpu suite WITHOUT -x (every failure listed), then the config-2
# bench line with CPU baseline.  usage: bash tools/gpu_suite.sh TAG
set -u
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT  # where this script writes its results
TAG=${1:-suite}
timeout -k 10 800 python -u -m pytest tests -m gpu -v --timeout 240 --timeout-method thread \
  -p no:cacheprovider --durations=12 -rP > $OUT/$TAG.pytest.log 2>&1
rc=$?
echo "pytest rc=$rc"; grep -E "passed|failed|error" $OUT/$TAG.pytest.log | tail -3
grep -E "^FAILED|^ERROR" $OUT/$TAG.pytest.log | head -20
[ $rc -ne 0 ] && [ $rc -ne 1 ] && exit $rc
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 --verbose > $OUT/$TAG.c2.json 2> $OUT/$TAG.c2.err
rc2=$?
echo "bench rc=$rc2"; cat $OUT/$TAG.c2.json | cut -c1-600
exit $rc
