#!/bin/bash
# Build libgad_hip.so for gfx950 in-tree (the .so travels to the GPU box with the snapshot).
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/gad/libgad_hip.so"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="--offload-arch=gfx950 -O3 -std=c++17 -fPIC -I$HERE/../include -I$HERE/csrc -Wno-unused-result"
mkdir -p "$HERE/build"
# the translation units: the compile loop and the link line both read this list
UNITS="gemm_f32 winograd wino4_fused attention norm elementwise optim optim8 transformer half projector local scorenet influence manifold vit similarity vae text lora sampler latent"
pids=()
objs=()
for f in $UNITS; do
  src="$HERE/csrc/$f.hip"; obj="$HERE/build/$f.o"
  objs+=("$obj")
  stale=0
  [ -f "$obj" ] || stale=1
  for dep in "$src" "$HERE"/csrc/*.h "$HERE/../include/gad.h"; do   # every header: a new one cannot be forgotten
    if [ "$dep" -nt "$obj" ]; then stale=1; fi
  done
  if [ $stale = 1 ]; then
    extra=""
    # attention.hip: MFMA results feed the vector ALUs directly (softmax, dS), so keep them in VGPRs: with the default AGPR
    # form hipcc moved every score / gradient tile through v_accvgpr_read / _write (50-150 instructions per K/V tile)
    [ "$f" = attention ] && extra="-mllvm -amdgpu-mfma-vgpr-form=1"
    # wino4_fused.hip: its accumulator folds run beside MFMAs, where packed f32 VALU (what SLP makes of them) is slower than scalar
    [ "$f" = wino4_fused ] && extra="-fno-slp-vectorize"
    $HIPCC $FLAGS $extra -c "$src" -o "$obj" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT" "${objs[@]}"
echo "built $OUT"
