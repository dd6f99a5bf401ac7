# every benchmarked configuration, full lines: bash tools/run_bench_configs.sh  -> $OUT_DIR/*.json (OUT_DIR default: bench_out/configs)
O=${OUT_DIR:-$PWD/bench_out/configs}
mkdir -p $O; rm -f $O/*
python bench.py --full --steps 30 --warmup 5 > $O/s4.json 2> $O/s4.err
python bench.py --full --steps 30 --warmup 5 --no-cpu-baseline --net newUNetTrans > $O/unet.json 2> $O/unet.err
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --fwd-only > $O/s4_fwd.json 2>/dev/null
python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --fwd-only --net newUNetTrans > $O/unet_fwd.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --dtype fp32 > $O/s4_fp32.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --net base_transformer_pos_s4_resnet50 > $O/r50_256.json 2>/dev/null
python bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --net base_transformer_pos_s4_resnet50 --img 1024 --batch 8 > $O/r50_1024.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --net xbd_unet_transformer --img 1024 --batch 1 > $O/xbd_b1.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --net xbd_unet_transformer --img 1024 --batch 4 > $O/xbd_b4.json 2>/dev/null
python bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --net base_transformer_pos_s4_dd8_o5 --img 512 --batch 8 > $O/o5_512.json 2>/dev/null
for f in $O/*.json; do echo $f; python -c "
import json,sys
d=json.load(open('$f')); print(d['value'], d['ms_per_step'], d['config'].get('step_tflops'), d['roofline'] and (d['roofline']['kernel'], d['roofline']['achieved'], d['roofline']['frac']), d.get('cpu_baseline',{}).get('value'))"; done
OUT_DIR=$O bash tools/prof_bench.sh s4f > /dev/null
OUT_DIR=$O bash tools/prof_bench.sh unetf --net newUNetTrans > /dev/null
