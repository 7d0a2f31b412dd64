"""Record tests/golden/gemm_plan.json (tests/test_gemm_plan_cpu.py): which plane layout the basis GEMM's host code chose, and
what egc_basis_pack_bytes answered, for the test's grid of shapes and flags at COMMIT -- the commit before the choice moved
into egc_gemm_host.h, where it was spread over f16x2_shape (inline in that commit's egc_gemm_split.h), f16x2k_shape (a host
symbol of its library) and the EGC_GEMM_24BIT test in front of both.

    EGC_HIP_LIB=<libegc_hip.so built at COMMIT> python tests/golden/make_gemm_plan.py COMMIT

The program below is compiled against COMMIT's own headers (taken from git) and linked to COMMIT's library, so nothing of the
answer comes from the tree this script sits in.  The table is a record: it is not regenerated when the test fails."""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]

import test_gemm_plan_cpu as T  # noqa: E402

PROGRAM = r"""
#include <cstdio>
#include "egc_gemm_split.h"
int main() {
  int f_in, f_g, w, flags;
  while (std::scanf("%d %d %d %d", &f_in, &f_g, &w, &flags) == 4) {
    char layout = 'B';
    if (f_in > 0 && f_g > 0 && w >= 0 && (flags & EGC_GEMM_24BIT) == 0) {
      const int ldb = (f_g + 3) & ~3, NV = (ldb + w + 31) & ~31;
      if (egc::f16x2_shape(f_in, ldb, NV, w)) layout = 'H';
      else if (egc::f16x2k_shape(f_in, f_g, ldb, w)) layout = 'K';
    }
    std::printf("%c %zu\n", layout, egc_basis_pack_bytes(f_in, f_g, w));
  }
  return 0;
}
"""
HEADERS = ("egc_amd/csrc/egc_gemm_split.h", "egc_amd/csrc/egc_common.h", "include/egc_hip.h")


def main():
    commit, lib = sys.argv[1], os.path.abspath(os.environ["EGC_HIP_LIB"])
    assert len(commit) == 40, "the full hash of the commit the library was built at"
    shapes = [s[:4] for s in T.grid()]
    with tempfile.TemporaryDirectory() as d:
        for h in HEADERS:
            with open(os.path.join(d, os.path.basename(h)), "wb") as f:
                f.write(subprocess.run(["git", "-C", ROOT, "show", f"{commit}:{h}"], check=True, capture_output=True).stdout)
        with open(os.path.join(d, "record.cpp"), "w") as f:
            f.write(PROGRAM)
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O1", "-std=c++17", "--offload-arch=gfx950", "-I" + d,
                        "-o", os.path.join(d, "record"), os.path.join(d, "record.cpp"), "-L" + os.path.dirname(lib),
                        "-l:" + os.path.basename(lib), "-Wl,-rpath," + os.path.dirname(lib)], check=True)
        r = subprocess.run([os.path.join(d, "record")], input="".join("%d %d %d %d\n" % s for s in shapes), check=True,
                           capture_output=True, text=True)
    answers = dict(zip(shapes, (line.split() for line in r.stdout.split("\n") if line)))
    assert len(answers) == len(shapes)
    rows = []
    for f_in in T.F_IN:
        cells = [(f_in, f_g, w) for f_g in T.COLS for w in T.COLS]
        bytes_ = [{int(answers[c + (fl,)][1]) for fl in T.FLAGS} for c in cells]
        assert all(len(b) == 1 for b in bytes_)                     # egc_basis_pack_bytes takes no flag
        rows.append(dict(layout=["".join(answers[c + (fl,)][0] for c in cells) for fl in T.FLAGS], pack_bytes=[b.pop() for b in bytes_]))
    with open(T.GOLDEN, "w") as f:
        f.write("{\n")
        for k, v in (("commit", commit), ("f_in", T.F_IN), ("cols", list(T.COLS)), ("flags", list(T.FLAGS))):
            f.write(f" {json.dumps(k)}: {json.dumps(v)},\n")
        f.write(' "layout_codes": "B = three bf16 planes, H = fp16x2 (register-stationary), K = fp16x2 long k; one character per '
                '(f_g, w_cols) of cols x cols, f_g outer, one string per flag",\n')
        f.write(' "rows": [\n' + ",\n".join("  " + json.dumps(r) for r in rows) + "\n ]\n}\n")
    print(f"wrote {T.GOLDEN}: {len(shapes)} (shape, flag) pairs from {lib}")


if __name__ == "__main__":
    main()
