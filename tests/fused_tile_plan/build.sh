#!/bin/bash
# Build the host check of the one-launch batch kernel's plan (egc_amd/csrc/egc_fused_tile_host.h): plain C++, nothing linked from
# the project and no HIP header.  SANITIZE=1: with AddressSanitizer and UndefinedBehaviorSanitizer.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
mkdir -p "$HERE/_build"
SAN=""
[ "${SANITIZE:-0}" = 1 ] && SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -g"
"${CXX:-/opt/rocm/lib/llvm/bin/clang++}" -O1 -std=c++17 -Wall $SAN -I"$ROOT/include" -I"$ROOT/egc_amd/csrc" \
  -o "$HERE/_build/fused_tile_plan_check${SAN:+_san}" "$HERE/fused_tile_plan_check.cpp"
echo "built $HERE/_build/fused_tile_plan_check${SAN:+_san}"
