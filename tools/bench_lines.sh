#!/bin/bash
# On the GPU box: the bench line of every BASELINE-shaped workload (256 x 4 MiB), with its 1-thread CPU baseline, and with
# the committed PMC summaries and instruction counts of these sources in place -> $OUT/<model>_256x4MiB_bench.json
OUT=${OUT:-bench_out/lines}
mkdir -p "$OUT"
for m in "$@"; do
  t=$(echo $m | tr '+' '_')
  python3 bench.py --model $m --blocks 256 --block-bytes 4194304 --full --no-extras --cache-dir /tmp/zc > "$OUT/${t}_256x4MiB_bench.json" 2> "$OUT/$t.err" || tail -3 "$OUT/$t.err"
  python3 -c "
import json
d=json.load(open('$OUT/${t}_256x4MiB_bench.json')); r=d['roofline']
print('$m', round(d['value'],2), d['bit_exact'], 'kernel_ms', round(r['kernel_ms'],1), 'traffic', r['traffic'], 'instr', r.get('instr_per_byte'), 'cycles/byte', r.get('cycles_per_byte'))"
done
