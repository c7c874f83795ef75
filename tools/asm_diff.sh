#!/bin/bash
# Show that a source-only change left the device code alone: compile every csrc/*.hip of two checkouts device-only to
# assembly with build.sh's flags, replace the names that may differ (the zero block's, the per-compilation __hip_cuid)
# with one token each, and diff.  Needs no GPU.
#   tools/asm_diff.sh <tree A> <tree B> <output directory outside both trees>
# What remains for a pure move is the zero-block object's own declaration lines; any instruction, .amdhsa_ or metadata
# line in the output is a change of the kernels.
set -e
[ $# -eq 3 ] || { echo "usage: $0 <tree A> <tree B> <outdir>" >&2; exit 2; }
OUT="$3"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
JOBS="${JOBS:-6}"
ZERO='_ZN4gadkL12g_zero_blockE|_ZN12_GLOBAL__N_111g_attn_zeroE|_ZN4gadhL6g_zeroE|_ZN12_GLOBAL__N_16g_zeroE|_ZL12g_zero_block'
for side in A B; do
  [ $side = A ] && root="$1" || root="$2"
  pkg="$root/group-attribution-for-diffusion-models_amd"
  mkdir -p "$OUT/$side"
  # flags and per-file extras: those of build.sh
  flags="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$root/include -I$pkg/csrc -Wno-unused-result --cuda-device-only -S"
  for src in "$pkg"/csrc/*.hip; do
    f="$(basename "$src" .hip)"; extra=""
    [ "$f" = attention ] && extra="-mllvm -amdgpu-mfma-vgpr-form=1"
    [ "$f" = wino4_fused ] && extra="-fno-slp-vectorize"
    while [ "$(jobs -rp | wc -l)" -ge "$JOBS" ]; do wait -n; done
    ( $HIPCC $flags $extra "$src" -o "$OUT/$side/$f.s" 2>"$OUT/$side/$f.log" &&
      sed -E -i "s/$ZERO/ZERO_BLOCK/g; s/__hip_cuid_[0-9a-f]+/HIP_CUID/g; s/[ \t]+; @/ ; @/" "$OUT/$side/$f.s" ) &
  done
  wait
done
rc=0
for a in "$OUT"/A/*.s; do
  f="$(basename "$a")"
  n="$(diff "$a" "$OUT/B/$f" | grep -c '^[<>]' || true)"
  echo "$f: $(wc -l < "$a") / $(wc -l < "$OUT/B/$f") lines, $n differ"
  if [ "$n" != 0 ]; then diff "$a" "$OUT/B/$f" | head -40; rc=1; fi
done
exit $rc
