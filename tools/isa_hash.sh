#!/bin/bash
# tools/isa_hash.sh <object.o> <kernel-name-substring>: md5 of the gfx950 instruction stream of the matching kernels, in the order
# the object emits them (addresses stripped) -- used to check that a refactoring leaves a tuned instance's code untouched
# tools/isa_hash.sh --each <object.o> <kernel-name-substring>: one "md5 symbol" line per matching kernel, sorted by symbol -- the
# comparison for a change that moves the kernels' emission order and nothing else
set -euo pipefail
EACH=0; [ "$1" = --each ] && { EACH=1; shift; }
O=$(realpath $1); K=$2; T=$(mktemp -d)
cp $O $T/x.o; (cd $T && /opt/rocm/lib/llvm/bin/llvm-objdump --offloading x.o > /dev/null)
/opt/rocm/lib/llvm/bin/llvm-objdump -d $T/x.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 | awk -v k="$K" '/^[0-9a-f]+ <.*>:/{p=index($0,k)>0} p' | sed -E 's/\/\/ [0-9A-F]+:.*$//; s/^[0-9a-f]+ //' > $T/k.s
if [ $EACH = 1 ]; then
  awk -v d="$T" '/^<.*>:$/{n++; print substr($0, 2, length($0) - 3) > (d "/syms")} {print > (d "/k" n ".s")}' $T/k.s
  n=0; while read -r sym; do n=$((n + 1)); echo "$(md5sum < $T/k$n.s | cut -d' ' -f1) $sym"; done < $T/syms | sort -k2
else
  wc -l < $T/k.s; md5sum < $T/k.s
fi
rm -rf $T
