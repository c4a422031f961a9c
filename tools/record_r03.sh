#!/bin/bash
# records the round-3 numbers DESIGN.md quotes on an MI355X; usage: tools/record_r03.sh OUTDIR (the records go to OUTDIR, then
# into profiles/)
set -e
OUT=$(realpath -m "${1:?usage: tools/record_r03.sh OUTDIR}")
mkdir -p "$OUT"
export OUT
cd "$(dirname "$0")/.."
python bench.py --full --steps 10 --warmup 3 > $OUT/r03_g24_f32_bench.json 2> $OUT/r03_g24_f32_bench.err
echo "g24 f32 (+ other_configs) done"
ND_BENCH_REHEARSAL=1 python bench.py --full --gpus 2 --steps 12 --warmup 2 --no-roofline > $OUT/r03_rehearsal2_bench.json 2> $OUT/r03_rehearsal2_bench.err
echo "rehearsal N=2 (both ranks on one GPU, gloo) done"
python tools/bench_train.py --cs 184 --batch 30 > $OUT/r03_train_bench_cs184_b30.json 2>/dev/null || true
python tools/bench_train.py --cs 136 --batch 30 > $OUT/r03_train_bench_cs136_b30.json 2>/dev/null || true
echo "train done"
