# usage: bash tools/prof_bench.sh <tag> [bench args...]   -> $OUT_DIR/prof_<tag>/ kernel stats csv (OUT_DIR default: bench_out/)
tag=$1; shift
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT_DIR:-$R/bench_out}
mkdir -p $O && O=$(cd $O && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $O/prof_$tag -- python3 $R/bench.py --full --steps 6 --warmup 2 --no-cpu-baseline --no-class-replay --no-secondary --no-ddp-rehearsal "$@" > $O/prof_$tag.json 2> $O/prof_$tag.err
f=$(ls $O/prof_$tag/*/*kernel_stats.csv | head -1)
cp $f $O/prof_${tag}_kernel_stats.csv
head -40 $f | cut -c1-200
