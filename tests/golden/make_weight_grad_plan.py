"""Record tests/golden/weight_grad_plan.json (tests/test_weight_grad_plan_cpu.py): egc_weight_grad_plan's plan8 and the two
workspace queries of the library for the test's grid of shapes and switches.  Host only: it runs without a GPU.

    EGC_HIP_LIB=<libegc_hip.so built at COMMIT> python tests/golden/make_weight_grad_plan.py COMMIT

The table is a record of what the library answered at COMMIT (the full hash is stored in it).  It exists to catch host code
that drifts from there: it is not regenerated when the test fails."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_weight_grad_plan_cpu as T  # noqa: E402
from egc_amd import _C  # noqa: E402


def main():
    commit = sys.argv[1]
    assert len(commit) == 40, "the full hash of the commit the library was built at"
    cases = T.grid()
    with pytest.MonkeyPatch.context() as mp:
        expect = T.answers(_C.load(), mp, cases)
    lines, start = [], 0                      # one line per (switches, shape): the rows of one case after the other
    for i in range(1, len(cases) + 1):
        if i == len(cases) or cases[i][:2] + cases[i][3:] != cases[start][:2] + cases[start][3:]:
            lines.append(expect[start:i])
            start = i
    axes = dict(commit=commit, rows=T.ROWS, shapes=T.SHAPES, e_cols=T.E_COLS, tiles=T.XT_TILES, forced_shapes=T.FORCED_SHAPES,
                forced_rows=T.FORCED_ROWS)
    with open(T.GOLDEN, "w") as f:
        f.write("{\n" + "".join(" %s: %s,\n" % (json.dumps(k), json.dumps(v)) for k, v in axes.items()))
        f.write(' "expect": [\n' + ",\n".join("  " + json.dumps(e, separators=(",", ":")) for e in lines) + "\n ]\n}\n")
    print(f"wrote {T.GOLDEN}: {len(cases)} cases from {_C.lib_path()}")


if __name__ == "__main__":
    main()
