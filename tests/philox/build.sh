#!/bin/bash
# Build the host check of the Philox4x32-10 generator (egc_amd/csrc/egc_philox.h): host code only, nothing linked from the
# project.  SANITIZE=1: with AddressSanitizer and UndefinedBehaviorSanitizer on the host side.
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
ROOT="$(cd "$HERE/../.." && pwd)"
mkdir -p "$HERE/_build"
SAN=""
[ "${SANITIZE:-0}" = 1 ] && SAN="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined -g"
"${HIPCC:-/opt/rocm/bin/hipcc}" -O1 -std=c++17 --offload-arch=gfx950 $SAN -I"$ROOT/egc_amd/csrc" \
  -o "$HERE/_build/philox_check" "$HERE/philox_check.cpp"
echo "built $HERE/_build/philox_check"
