#!/bin/bash
# Round-5 GPU session: the -m gpu suite (parity log), smoke, the driver's
# bench command twice beside the 30 + 100 default, the strong-scaling shard
# (tools/strong_shard.py) and its rocprofv3 kernel trace.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$(pwd)
OUT=gpurun_out/${1:-r05}
mkdir -p "$OUT"
export TMPDIR=/tmp
rocm-smi --showproductname > "$OUT/smi.txt" 2>&1 || true
if [ -z "${SKIP_TESTS:-}" ]; then
  rm -f "$OUT/parity_checks.jsonl"
  SRCNN_PARITY_LOG=$ROOT/$OUT/parity_checks.jsonl timeout -k 10 900 python -u -m pytest tests -m gpu -q -x \
    --timeout 300 --timeout-method thread -p no:cacheprovider ${PYTEST_ARGS:-} > "$OUT/pytest_gpu.log" 2>&1
  rc=$?; echo "pytest rc=$rc"; tail -5 "$OUT/pytest_gpu.log"
  [ -s "$OUT/parity_checks.jsonl" ] && python3 tools/parity_summary.py "$OUT/parity_checks.jsonl" > "$OUT/parity_summary.json"
  [ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
  timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
  rc=$?; echo "smoke rc=$rc"; tail -2 "$OUT/smoke.log"; [ $rc -eq 0 ] || exit $rc
fi
summ() { python3 -c "import json; d=json.load(open('$1')); print('$2', d['value'], d['ms_per_step'], d['config'].get('settle_steps'), {k: v['ms_per_step'] for k, v in d['kernels'].items()})"; }
timeout -k 10 300 python bench.py --full --gpus 1 --steps 20 --warmup 5 > "$OUT/d20a.json" 2> "$OUT/d20a.err" || exit $?
summ "$OUT/d20a.json" d20a
timeout -k 10 300 python bench.py --full --no-cpu-baseline > "$OUT/d100.json" 2> "$OUT/d100.err" || exit $?
summ "$OUT/d100.json" d100
timeout -k 10 300 python bench.py --full --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline > "$OUT/d20b.json" 2> "$OUT/d20b.err" || exit $?
summ "$OUT/d20b.json" d20b
timeout -k 10 300 python tools/strong_shard.py > "$OUT/strong.jsonl" 2> "$OUT/strong.err" || exit $?
cat "$OUT/strong.jsonl"
cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$ROOT/$OUT/rocprof_strong" -o run --output-format csv -- \
  python3 "$ROOT/tools/strong_shard.py" --modes lazy,separate > "$ROOT/$OUT/rocprof_strong.log" 2>&1 || exit $?
echo "rocprof ok"
