#!/bin/bash
# tools/isa_hash_all.sh <objdir> <source-stem>...: one line "<stem> <kernel symbol> <lines> <md5>" per gfx950 kernel of each object,
# symbols sorted, through tools/isa_hash.sh -- two builds left the device code alone when their lists are equal (md5sum the list)
set -euo pipefail
HERE="$(cd "$(dirname "${BASH_SOURCE[0]}")" && pwd)"
D=$1; shift
for f in "$@"; do
  T=$(mktemp -d); cp "$D/$f.o" $T/x.o; (cd $T && /opt/rocm/lib/llvm/bin/llvm-objdump --offloading x.o > /dev/null)
  syms=$(/opt/rocm/lib/llvm/bin/llvm-objdump -d $T/x.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 | sed -nE 's/^[0-9a-f]+ <(.*)>:$/\1/p' | sort -u)
  rm -rf $T
  for s in $syms; do echo "$f $s $(bash "$HERE/isa_hash.sh" "$D/$f.o" "<$s>" | tr '\n' ' ' | awk '{print $1, $2}')"; done
done
