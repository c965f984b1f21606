set -u
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
OUT=${1:?usage: bash tools/run_rehearsals.sh <output directory>}
mkdir -p "$OUT"
for n in 2 3; do
  SDM_BENCH_REHEARSE=1 timeout -k 10 300 python3 bench.py --full --gpus $n --kfs 16 --steps 5 --warmup 1 2> $OUT/rehearse$n.err | grep '^{"metric"' > $OUT/rehearsal_${n}ranks_one_gpu.json || { echo "rehearsal $n failed"; tail -20 $OUT/rehearse$n.err; }
done
python3 - "$OUT" <<'PY'
import json, os, sys
for n in (2,3):
    d=json.load(open(os.path.join(sys.argv[1], "rehearsal_%dranks_one_gpu.json" % n)))
    print(n, d["value"], d.get("value_baseline_literal"), d.get("exchange_ms_per_step"), d["config"].get("exchange_wire"), d.get("staged_refused_maps"))
PY
timeout -k 10 300 python -m pytest tests/test_gpu_shard.py tests/test_gpu_comm.py -m gpu -x -q 2>&1 | tail -2
