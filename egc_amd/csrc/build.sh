#!/bin/bash
# Build libegc_hip.so (gfx950 only) in-tree: egc_amd/lib/libegc_hip.so
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
OUT="$ROOT/egc_amd/lib"
OBJ="$HERE/obj"
[ -n "${EGC_EXTRA_FLAGS:-}" ] && OBJ="$OBJ/dbg_$(echo "$EGC_EXTRA_FLAGS" | tr -c "A-Za-z0-9\n" "_")"   # a diagnostic build never shares objects with the plain one
mkdir -p "$OUT" "$OBJ"
HIPCC="${HIPCC:-/opt/rocm/bin/hipcc}"
FLAGS="-O3 --offload-arch=gfx950 -fPIC -std=c++17 -ffp-contract=off -I$ROOT/include -I$HERE -Wall -Wno-unused-function -Wno-pass-failed ${EGC_EXTRA_FLAGS:-}"
SRCS="egc_graph egc_gather_plan egc_gemm egc_gemm_bf16x3 egc_gemm_f16x2 egc_gemm_f16x2k egc_gemm_xt egc_aggregate egc_aggregate_fast egc_aggregate_tile egc_fused_tile egc_fused_tile_wide1 egc_fused_tile_wide2 egc_fused_tile_wide3 egc_backward egc_tail egc_readout egc_encoder egc_softmax egc_token_head egc_head egc_typed_mean egc_mpnn egc_gatv2 egc_gat egc_pna egc_nbr_sum egc_collate egc_adam"
pids=()
objs=()
for src in $SRCS; do
  objs+=("$OBJ/$src.o")
  stale=0
  [ -f "$OBJ/$src.o" ] || stale=1
  for dep in "$HERE/$src.hip" "$HERE"/*.h "$HERE"/*.inc "$ROOT/include/egc_hip.h" "$ROOT/include/egc_optim.h"; do   # every header: an object does not say which it includes
    [ "$dep" -nt "$OBJ/$src.o" ] && stale=1
  done
  if [ $stale = 1 ]; then
    extra=""
    # packed-f32 VALU next to MFMAs costs more issue cycles than two scalar operations (egc_gemm_f16x2.hip header)
    { [ "$src" = egc_gemm_f16x2 ] || [ "$src" = egc_gemm_f16x2k ]; } && extra="-fno-slp-vectorize"
    $HIPCC $FLAGS $extra -c "$HERE/$src.hip" -o "$OBJ/$src.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]:-}"; do [ -n "$p" ] && wait "$p"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/libegc_hip.so" "${objs[@]}"
echo "built $OUT/libegc_hip.so"
