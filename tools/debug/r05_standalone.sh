#!/bin/bash
# the other single-GPU BASELINE workloads as stand-alone bench lines (own live traffic passes): bash tools/debug/r05_standalone.sh <output directory>
set -u
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${1:?usage: bash tools/debug/r05_standalone.sh <output directory>}
mkdir -p "$OUT"
timeout -k 10 300 python bench.py --full --kfs 256 --cpu-kfs 4 --no-extra > $OUT/bench_480p_256kf_n20.json 2> $OUT/sa.err || echo "256kf failed"
timeout -k 10 300 python bench.py --full --res 720p --kfs 256 --nbrs 7 --cpu-kfs 3 --no-extra > $OUT/bench_720p_256kf_n7.json 2>> $OUT/sa.err || echo "720p failed"
timeout -k 10 300 python bench.py --full --res 1080p --kfs 64 --nbrs 7 --cpu-kfs 2 --no-extra > $OUT/bench_1080p_64kf_n7.json 2>> $OUT/sa.err || echo "1080p failed"
for f in 480p_256kf_n20 720p_256kf_n7 1080p_64kf_n7; do python3 -c "
import json; d=json.load(open('$OUT/bench_$f.json')); r=d['roofline']
print('$f', d['value'], d['ms_per_step'], 'K1', r['launch_ms'], 'frac', r['frac'], 'hbm_frac', r.get('hbm_frac'), (r.get('traffic_source') or r.get('traffic_note',''))[:30], 'streaming', d.get('value_streaming'), 'cpu', d['cpu_baseline']['value'])"; done
