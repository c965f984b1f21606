# round 5: bench lines + kernel stats of the final build (one GPU session): bash tools/r05_final.sh <output directory>
set -u
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${1:?usage: bash tools/r05_final.sh <output directory>}
mkdir -p "$OUT"
( time timeout -k 10 700 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err ) 2> $OUT/bench.time || echo "bench failed"
tail -c 300 $OUT/bench.json; cat $OUT/bench.time
timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -- python3 bench.py --full --steps 10 --warmup 2 --cpu-kfs 0 --no-extra --no-streaming --no-live-pmc > $OUT/kt.log 2>&1 || echo "kernel trace failed"
f=$(find $OUT/kt -name "*kernel_stats.csv" | head -1)
if [ -n "$f" ]; then (head -1 "$f"; grep "sdm::" "$f") > $OUT/kernel_stats.csv; fi
python3 tools/kstats.py $OUT/kt || true
rm -rf $OUT/kt
timeout -k 10 100 python tools/latency.py 7 > $OUT/latency.txt 2>&1 || echo "latency failed"
timeout -k 10 100 python tools/latency.py 20 >> $OUT/latency.txt 2>&1 || echo "latency failed"
grep -v amdgpu $OUT/latency.txt
for cfg in "disp10 --disparity 10" "spread03 --prior-spread 0.3" "disp10_spread03 --disparity 10 --prior-spread 0.3" "strip --scene strip --roll 5 --prior-spread 0.3"; do
  set -- $cfg; tag=$1; shift
  timeout -k 10 200 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt_$tag -- python3 bench.py --full --steps 10 --warmup 2 --cpu-kfs 0 --no-extra --no-stats --no-streaming --no-live-pmc "$@" > $OUT/kt_$tag.log 2>&1 || echo "kt $tag failed"
  f=$(find $OUT/kt_$tag -name "*kernel_stats.csv" | head -1)
  if [ -n "$f" ]; then (head -1 "$f"; grep "sdm::" "$f") > $OUT/kernel_stats_$tag.csv; fi
  rm -rf $OUT/kt_$tag
done
for n in 2 3; do
  SDM_BENCH_REHEARSE=1 timeout -k 10 300 python3 bench.py --full --gpus $n --kfs 16 --steps 5 --warmup 1 2> $OUT/rehearse$n.err | grep '^{"metric"' > $OUT/rehearsal_${n}ranks_one_gpu.json || echo "rehearsal $n failed"
done
echo done benches
