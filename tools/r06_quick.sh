#!/bin/bash
# Round 6 quick GPU check: the tests named in $TESTS (default: the round-6
# additions), then one bench run.  Every GPU step has its own time limit and
# a fault / abort / timeout ends the script.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=gpurun_out/${1:-quick}
mkdir -p "$OUT"
export TMPDIR=/tmp
TESTS=${TESTS:-"tests/test_split_arith_gpu.py tests/test_parity_gpu.py::test_wide_tiles_past_the_wide_step tests/test_parity_gpu.py::test_train_activations_follow_the_step_arith"}
timeout -k 10 600 python -u -m pytest $TESTS -q -x --timeout 120 --timeout-method thread -p no:cacheprovider > "$OUT/pytest.log" 2>&1
rc=$?; echo "pytest rc=$rc"; tail -15 "$OUT/pytest.log"
[ $rc -eq 0 ] || [ $rc -eq 1 ] || exit $rc
if [ -z "${NO_BENCH:-}" ]; then
  timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---no-cpu-baseline} > "$OUT/bench.json" 2> "$OUT/bench.err"
  rc=$?; echo "bench rc=$rc"; tail -3 "$OUT/bench.err"
  python3 - "$OUT/bench.json" <<'PY'
import json,sys
d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print("value", d["value"], "ms", d["ms_per_step"])
for k,v in d["kernels"].items(): print("  %-24s %.4f" % (k, v["ms_per_step"]))
print("roof", json.dumps(d["roofline"])[:400])
print("step_roof", json.dumps(d["step_roofline"]))
for side in ("wide", "forward"):
    if side in d: print(side, d[side].get("ms_per_step", d[side].get("ms_per_frame")))
PY
fi
exit $rc
