"""Record tests/golden/weight_grad_forms.json (tests/test_weight_grad_forms_gpu.py) on the MI355X: the SHA-256 of what the
weight-gradient entry points wrote for every case of the test, from the library built at COMMIT.

    EGC_HIP_LIB=<libegc_hip.so built at COMMIT> python tests/golden/make_weight_grad_forms.py COMMIT

Every case is run twice and its digests must repeat (the reduction adds the row ranges in a fixed order): one that does not is
reported and nothing is written.  The table is a record: it is not regenerated when the test fails."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_weight_grad_forms_gpu as T  # noqa: E402
from egc_amd import _C  # noqa: E402


def main():
    commit = sys.argv[1]
    assert len(commit) == 40, "the full hash of the commit the library was built at"
    with pytest.MonkeyPatch.context() as mp:
        first = {c: T.digest(c, mp) for c in T.case_ids()}
        second = {c: T.digest(c, mp) for c in T.case_ids()}
    unstable = [c for c in first if first[c] != second[c]]
    assert not unstable, f"digests that did not repeat: {unstable}"
    with open(T.GOLDEN, "w") as f:
        f.write('{\n "commit": %s,\n "digests": {\n' % json.dumps(commit))
        f.write(",\n".join("  %s: %s" % (json.dumps(c), json.dumps(d)) for c, d in first.items()) + "\n }\n}\n")
    print(f"wrote {T.GOLDEN}: {len(first)} cases, each twice with equal digests, from {_C.lib_path()}")


if __name__ == "__main__":
    main()
