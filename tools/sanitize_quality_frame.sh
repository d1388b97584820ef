#!/bin/bash
# Host-code sanitizer run of srcnn_quality_frame's argument checks (CPU only,
# no device): the two ABI units (abi.cpp, abi_upscale.cpp) and
# tests/quality_frame_sanitize.cpp, built with the host's AddressSanitizer +
# UndefinedBehaviorSanitizer (-Xarch_host: the device code is compiled as
# always) and linked with the library's other objects as `make` left them.
# The program is run directly and checks its own results.
#   make -C cnn-super-resolution_amd && tools/sanitize_quality_frame.sh
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
$HIPCC -O1 -g -std=c++17 $SAN -I"$R/include" -x c++ -c "$R/tests/quality_frame_sanitize.cpp" -o "$O/quality_frame_sanitize.o"
others=$(ls "$K"/build/obj/*.o | grep -v '/abi[_a-z]*\.cpp\.o$')
$HIPCC --offload-arch=gfx950 $SAN -o "$O/quality_frame_sanitize" "$O/quality_frame_sanitize.o" "$O/abi.san.o" \
  "$O/abi_upscale.san.o" $others -L"$ROCM/lib" -lrccl -Wl,-rpath,"$ROCM/lib"
# (the HIP runtime's own start-up allocations are not the code under test)
ASAN_OPTIONS=detect_leaks=0:abort_on_error=1 UBSAN_OPTIONS=print_stacktrace=1 "$O/quality_frame_sanitize"
