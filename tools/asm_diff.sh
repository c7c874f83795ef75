#!/bin/bash
# Show that a source-only change left the device code alone: compile every csrc/*.hip of two checkouts device-only to
# assembly with build.sh's flags, replace the names that may differ (the zero block's, the per-compilation __hip_cuid)
# with one token each, and diff.  Needs no GPU.
#   tools/asm_diff.sh [--by-kernel] <tree A> <tree B> <output directory outside both trees>
# What remains for a pure move is the zero-block object's own declaration lines; any instruction, .amdhsa_ or metadata
# line in the output is a change of the kernels.
# --by-kernel: for a change that moves kernels between files.  Each tree's .s files are cut into one file per kernel symbol
# (its code from the label to .Lfunc_end, which holds the .amdhsa_kernel block, then its metadata entry), the per-file
# function numbers of the local labels are dropped, and the trees are compared symbol by symbol, whatever file a kernel lives
# in: one line per kernel - identical, differs, or only on one side.
# REUSE=1 compares the .s files a previous run left in the output directory instead of compiling again.
set -e
BYK=0
[ "$1" = --by-kernel ] && { BYK=1; shift; }
[ $# -eq 3 ] || { echo "usage: $0 [--by-kernel] <tree A> <tree B> <outdir>" >&2; exit 2; }
OUT="$3"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
JOBS="${JOBS:-6}"
ZERO='_ZN4gadkL12g_zero_blockE|_ZN12_GLOBAL__N_111g_attn_zeroE|_ZN4gadhL6g_zeroE|_ZN12_GLOBAL__N_16g_zeroE|_ZL12g_zero_block'
for side in A B; do
  [ -n "$REUSE" ] && break
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
if [ $BYK = 1 ]; then
  for side in A B; do
    rm -rf "$OUT/$side.kernels"; mkdir -p "$OUT/$side.kernels"
    # kernels are the symbols with an .amdhsa_kernel block; a file is named by its number in the sorted list of both trees' symbols
    cat "$OUT/$side"/*.s | sed -n 's/^[ \t]*\.amdhsa_kernel[ \t]\+//p'
  done | sort -u > "$OUT/kernels.txt"
  for side in A B; do
    cat "$OUT/$side"/*.s | sed -E 's/\.L(func_end|func_begin|tmp)[0-9]+/.L\1/g; s/BB[0-9]+_/BB_/g; s/[ \t]+;/ ;/g' | awk -v dir="$OUT/$side.kernels" -v list="$OUT/kernels.txt" '
      BEGIN { while ((getline s < list) > 0) id[s] = ++n }
      cur == "" && /^[A-Za-z_$][A-Za-z0-9_$.]*:/ { s = $1; sub(/:.*/, "", s); if (s in id) cur = dir "/" id[s] ".s" }
      cur != "" { print > cur }
      cur != "" && /^\.Lfunc_end:/ { close(cur); cur = "" }
      /^amdhsa\.kernels:/ { meta = 1; next }
      meta && /^[^ ]/ { meta = 0; if (ent != "") close(ent); ent = "" }
      meta && /^  - / { if (ent != "") { close(ent); ent = "" } buf = $0 "\n"; next }                  # a new entry: held until its .name: line names it
      meta && ent == "" { buf = buf $0 "\n"; if ($1 == ".name:" && ($2 in id)) { ent = dir "/" id[$2] ".s"; printf "%s", buf >> ent } next }
      meta { print >> ent }'
  done
  rc=0; i=0
  while read -r sym; do
    i=$((i + 1)); a="$OUT/A.kernels/$i.s"; b="$OUT/B.kernels/$i.s"
    if [ ! -f "$a" ]; then echo "only in B   $sym"; rc=1
    elif [ ! -f "$b" ]; then echo "only in A   $sym"; rc=1
    elif cmp -s "$a" "$b"; then echo "identical   $sym"
    else echo "differs     $sym ($(diff "$a" "$b" | grep -c '^[<>]') lines; $a $b)"; rc=1; fi
  done < "$OUT/kernels.txt"
  exit $rc
fi
rc=0
for a in "$OUT"/A/*.s; do
  f="$(basename "$a")"
  n="$(diff "$a" "$OUT/B/$f" | grep -c '^[<>]' || true)"
  echo "$f: $(wc -l < "$a") / $(wc -l < "$OUT/B/$f") lines, $n differ"
  if [ "$n" != 0 ]; then diff "$a" "$OUT/B/$f" | head -40; rc=1; fi
done
exit $rc
