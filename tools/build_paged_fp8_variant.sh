#!/bin/bash
# Lab: libMFAFFI with fa_fwd_16_paged_fp8.hip recompiled under extra defines (the ablation of DESIGN.md section 3.1j):
#   tools/build_paged_fp8_variant.sh nocvt -DUMFA_FP8_ABLATE=1   ->  tools/lab_bin/libMFAFFI_nocvt.so   (run with UMFA_LIBRARY=that file)
# Needs the product's objects (make -C universal-metal-flash-attention_amd/csrc first).
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CS=$ROOT/universal-metal-flash-attention_amd/csrc
NAME=$1; shift
TMP=$(mktemp -d)
mkdir -p "$ROOT/tools/lab_bin"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -w -fno-slp-vectorize -mllvm -pragma-unroll-threshold=262144 \
    "$@" -I"$CS" -c "$CS/fa_fwd_16_paged_fp8.hip" -o "$TMP/fa_fwd_16_paged_fp8.o"
OBJS=$(ls "$CS"/build/*.o | grep -v fa_fwd_16_paged_fp8.o)
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -Wl,--version-script="$CS/exports.map" -o "$ROOT/tools/lab_bin/libMFAFFI_$NAME.so" $OBJS "$TMP/fa_fwd_16_paged_fp8.o"
rm -rf "$TMP"
echo "built tools/lab_bin/libMFAFFI_$NAME.so"
