# HBM-side traffic of the dominant conv kernel class: two SEPARATE counter passes (FETCH_SIZE, WRITE_SIZE), as
# MI355X_MICROARCH.md prescribes; --kernel-trace only.  Writes $OUT_DIR/pmc_{fetch,write}/ + a JSON summary (OUT_DIR default: bench_out/).
R=$(cd "$(dirname "$0")/.." && pwd)
O=${OUT_DIR:-$R/bench_out}
mkdir -p $O && O=$(cd $O && pwd)
cd /tmp && export TMPDIR=/tmp
rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d $O/pmc_fetch -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-graph > /dev/null 2> $O/pmc_fetch.err
rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d $O/pmc_write -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-graph > /dev/null 2> $O/pmc_write.err
python3 $R/tools/pmc_traffic.py $O/pmc_fetch $O/pmc_write > $O/pmc_traffic.json
cat $O/pmc_traffic.json
