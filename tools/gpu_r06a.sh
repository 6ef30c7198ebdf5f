# GPU-box script (r06): baseline per-layer tables of config 4 (bf16) and config 2 on one box.
#   usage: bash tools/gpu_r06a.sh TAG
set -u
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out}; mkdir -p $OUT  # where this script writes its results
TAG=${1:-r06a}
timeout -k 10 300 python bench.py --full --config 4 --mfma bf16 --verbose --steps 6 --warmup 2 --no-cpu-baseline > $OUT/$TAG.c4.json 2> $OUT/$TAG.c4.err
r=$?; echo "c4 rc=$r"; cut -c1-300 $OUT/$TAG.c4.json; [ $r -ne 0 ] && exit $r
timeout -k 10 300 python bench.py --full --verbose --steps 10 --warmup 3 --no-cpu-baseline > $OUT/$TAG.c2.json 2> $OUT/$TAG.c2.err
r=$?; echo "c2 rc=$r"; cut -c1-300 $OUT/$TAG.c2.json
exit $r
