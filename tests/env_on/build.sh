#!/bin/bash
# Build the host check of egc::env_on (egc_amd/csrc/egc_plain.h): plain C++, nothing linked from the project and no HIP header.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
mkdir -p "$HERE/_build"
"${CXX:-/opt/rocm/lib/llvm/bin/clang++}" -O1 -std=c++17 -Wall -I"$ROOT/include" -I"$ROOT/egc_amd/csrc" \
  -o "$HERE/_build/env_on_check" "$HERE/env_on_check.cpp"
echo "built $HERE/_build/env_on_check"
