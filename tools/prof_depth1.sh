# rocprofv3 kernel stats of bench.py --full with ONE commitment in flight (KZG_BENCH_PIPELINE=0): every k_msm_accumulate launch runs alone, so the
# average duration is directly comparable with roofline.avg_launch_ms of the bench line -> $PROF_OUT/<tag>_depth1_kernel_stats.csv
# usage: PROF_OUT=<directory> bash tools/prof_depth1.sh <tag>
TAG=${1:-r02}
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${PROF_OUT:?set PROF_OUT to the directory that receives the bench log and the kernel stats}
mkdir -p "$OUT" && OUT=$(cd "$OUT" && pwd)
TRACE=$(mktemp -d)
cd "$TRACE" && export TMPDIR=$TRACE
export KZG_BENCH_PIPELINE=0
rocprofv3 --kernel-trace --stats --output-format csv -d $TRACE/prof_d1 -o run -- python3 $ROOT/bench.py --full --steps 30 --warmup 4 --no-secondary --no-cpu-baseline > $OUT/${TAG}_depth1_bench.log 2>&1
cp "$(find $TRACE/prof_d1 -name '*kernel_stats.csv' | head -1)" $OUT/${TAG}_depth1_kernel_stats.csv
grep -o '"avg_launch_ms": [0-9.]*' $OUT/${TAG}_depth1_bench.log
head -4 $OUT/${TAG}_depth1_kernel_stats.csv | cut -c1-60,200-
rm -rf "$TRACE"
