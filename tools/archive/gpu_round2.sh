#!/bin/bash
# Run on an MI355X box: GPU test suite + the driver's bench command (with every leg), results under the directory given as $1.
OUT=${1:?usage: gpu_round2.sh OUTDIR}
mkdir -p "$OUT"
python -m pytest tests -x -q -m gpu 2>&1 | tail -15
python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/bench_driver_cmd.json" 2> "$OUT/bench_driver_cmd.err"
tail -c 2000 "$OUT/bench_driver_cmd.err"
python tools/archive/show_bench.py "$OUT/bench_driver_cmd.json"
