# GPU-box script (r06): narrow-width GPU tests (-k, "-" = none), then the reference grid's
# ResUNet(base, 4) benches at 512^2 (bench.py --config res).
#   usage: bash tools/gpu_r06e.sh TAG "PYTEST_K" "BASES"
set -u
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT  # where this script writes its results
TAG=$1; K=$2; BASES=${3:-16 24 32 48}
if [ "$K" != "-" ]; then
  timeout -k 10 700 python -u -m pytest tests -m gpu -x -v --timeout 240 --timeout-method thread \
    -p no:cacheprovider -k "$K" > $OUT/$TAG.pytest.log 2>&1
  rc=$?
  echo "pytest rc=$rc"; grep -E "passed|failed|error" $OUT/$TAG.pytest.log | tail -2
  grep -E "^FAILED|^ERROR" $OUT/$TAG.pytest.log | head
  [ $rc -ne 0 ] && exit $rc
fi
for B in $BASES; do
  timeout -k 10 300 python bench.py --full --config res --base $B --depth 4 --no-cpu-baseline --verbose --steps 10 --warmup 3 \
    > $OUT/$TAG.res$B.json 2> $OUT/$TAG.res$B.err
  rc=$?
  echo "res base $B rc=$rc: $(python -c "import json;d=json.load(open('$OUT/$TAG.res$B.json'));print(d['value'],d['ms_per_step'],d['roofline'].get('step_conv_frac'))" 2>/dev/null)"
  [ $rc -ne 0 ] && { tail -n 20 $OUT/$TAG.res$B.err; exit $rc; }
done
exit 0
