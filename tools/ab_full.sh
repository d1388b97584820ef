#!/bin/bash
# Same-box A/B of library variants on the whole bench line (headline, wide
# net, 4K frame): tools/ab_full.sh <tag> <lib1.so> [lib2.so ...], two
# interleaved reps of bench.py --steps 20 --warmup 5 per library.
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT=gpurun_out/${1:-abf}; shift
mkdir -p "$OUT"
for rep in 1 2; do
  i=0
  for lib in "$@"; do
    i=$((i+1))
    SRCNN_HIP_LIB=$PWD/$lib timeout -k 10 240 python bench.py --full --no-cpu-baseline --steps 20 --warmup 5 \
      > "$OUT/bench_${i}_$rep.json" 2> "$OUT/bench_${i}_$rep.err" || exit $?
    python3 -c "import json; d=json.load(open('$OUT/bench_${i}_$rep.json')); w=d.get('wide',{}); f=d.get('forward',{}); print('variant $i rep $rep', round(d['value']), d['ms_per_step'], 'wide', w.get('ms_per_step'), 'fwd', f.get('ms_per_frame'), {k: round(v['ms_per_step'],4) for k,v in w.get('kernels',{}).items()})"
  done
done
