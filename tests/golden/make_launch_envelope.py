"""Record tests/golden/launch_envelope.json (tests/test_launch_envelope_cpu.py): the host-only size / capacity queries of the
library for the test's grid of layers.

    EGC_HIP_LIB=<libegc_hip.so built at COMMIT> python tests/golden/make_launch_envelope.py COMMIT

The table is a record of what the library answered at COMMIT (the full hash is stored in it).  It exists to catch host code
that drifts from there: it is not regenerated when the test fails."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import test_launch_envelope_cpu as T  # noqa: E402
from egc_amd import _C  # noqa: E402


def main():
    commit = sys.argv[1]
    assert len(commit) == 40, "the full hash of the commit the library was built at"
    lib = _C.load()
    cases = [dict(layer=spec, expect=T.envelope(lib, spec)) for spec in T.grid()]
    table = dict(commit=commit, edge_bounds=list(T.EDGE_BOUNDS), tile_node_bounds=list(T.TILE_NODE_BOUNDS),
                 graph_sizes=[list(s) for s in T.GRAPH_SIZES], cases=cases)
    with open(T.GOLDEN, "w") as f:
        f.write("{\n")
        for k in ("commit", "edge_bounds", "tile_node_bounds", "graph_sizes"):
            f.write(f" {json.dumps(k)}: {json.dumps(table[k])},\n")
        f.write(' "cases": [\n' + ",\n".join("  " + json.dumps(c) for c in cases) + "\n ]\n}\n")
    print(f"wrote {T.GOLDEN}: {len(cases)} layers from {_C.lib_path()}")


if __name__ == "__main__":
    main()
