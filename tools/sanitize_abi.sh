#!/bin/bash
# Host-code sanitizer run of the C ABI's validation (CPU only, no device): the
# two ABI units (abi.cpp, abi_upscale.cpp) and tests/upscale_abi_sanitize.cpp,
# which feeds every image-level entry point invalid input, built with the
# host's AddressSanitizer + UndefinedBehaviorSanitizer (-Xarch_host: the device
# code is compiled as always) and linked with the library's other objects as
# `make` left them.  The program is run directly; what it prints must be what
# tests/golden/upscale_abi_errors.json holds under the same names.
#   make -C cnn-super-resolution_amd && tools/sanitize_abi.sh
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
K=$R/cnn-super-resolution_amd
O=${SANITIZE_OUT:-$K/build/sanitize}
ROCM=${ROCM:-/opt/rocm}
HIPCC=${HIPCC:-$ROCM/bin/hipcc}
SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=all -Xarch_host -fno-omit-frame-pointer"
mkdir -p "$O"
for u in abi abi_upscale; do
  $HIPCC -O1 -g -std=c++17 --offload-arch=gfx950 -fvisibility=hidden $SAN -I"$R/include" -I"$K/csrc/hip" \
    -x hip -c "$K/csrc/hip/$u.cpp" -o "$O/$u.san.o"
done
$HIPCC -O1 -g -std=c++17 $SAN -I"$R/include" -x c++ -c "$R/tests/upscale_abi_sanitize.cpp" -o "$O/upscale_abi_sanitize.o"
others=$(ls "$K"/build/obj/*.o | grep -v '/abi[_a-z]*\.cpp\.o$')
$HIPCC --offload-arch=gfx950 $SAN -o "$O/upscale_abi_sanitize" "$O/upscale_abi_sanitize.o" "$O/abi.san.o" \
  "$O/abi_upscale.san.o" $others -L"$ROCM/lib" -lrccl -Wl,-rpath,"$ROCM/lib"
# (the HIP runtime's own start-up allocations are not the code under test)
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 "$O/upscale_abi_sanitize" > "$O/upscale_abi.tsv"
python3 - "$O/upscale_abi.tsv" "$R/tests/golden/upscale_abi_errors.json" <<'EOF'
import json, sys
want = json.load(open(sys.argv[2]))
rows = [l.rstrip("\n").split("\t") for l in open(sys.argv[1])]
held = [(n, [int(r), m]) for n, r, m in rows if not n.startswith("extra/")]
wrong = [(n, got, want.get(n)) for n, got in held if want.get(n) != got]
for w in wrong:
    print("%s:\n  got  %r\n  want %r" % w)
print("sanitize_abi: %d calls ran clean, %d of them compared with the golden table, %d differ" % (len(rows), len(held), len(wrong)))
sys.exit(1 if wrong or not held else 0)
EOF
