set -u
OUT=${1:?usage: bash tools/run_gpu_suite.sh <output directory>}
mkdir -p "$OUT"
cd /tmp && export TMPDIR=/tmp && cd "$GRAFT_REPO_ROOT"
# the parity / fuzz files first, each under its own short timeout: a kernel fault must not cost minutes
for f in tests/test_gpu_parity.py tests/test_gpu_fuzz.py tests/test_gpu_statefuzz.py; do
  timeout -k 10 300 python -m pytest $f -m gpu -x -q > $OUT/$(basename $f).log 2>&1 || { echo "FAILED $f"; tail -15 $OUT/$(basename $f).log; exit 1; }
  tail -1 $OUT/$(basename $f).log
done
( timeout -k 10 900 python -m pytest tests -m gpu -x -q > $OUT/pytest.log 2>&1; echo "pytest rc=$?" >> $OUT/pytest.log )
tail -4 $OUT/pytest.log
grep -q "rc=0" $OUT/pytest.log || exit 1
for k in 0 1 2 4 0; do
  timeout -k 10 120 python tools/k1_time.py --outliers $k 2>&1 | grep -E "K1 median|Error|error" >> $OUT/k1.txt
done
cat $OUT/k1.txt
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kt -- python3 bench.py --full --steps 10 --warmup 2 --cpu-kfs 0 --no-extra > $OUT/kt.log 2>&1
python3 tools/kstats.py $OUT/kt | head -8; rm -rf $OUT/kt
