"""The host envelope of the aggregate launchers, pinned against the library of the commit BEFORE their shared derivations
moved into egc_aggregate_host.h: the size / capacity queries of include/egc_hip.h (host only, no GPU touched) for every
layer shape a static table names and for the edges of the kernels' envelopes.  These numbers are what the callers size
workspaces, LDS images and tiles by, and they come out of the same functions the launchers use (agg_layer_fields,
agg_lds_strips, agg_lpr, ft_lds): a value that moves here is a launch that changed.

tests/golden/launch_envelope.json was recorded ONCE, by tests/golden/make_launch_envelope.py, from the library built at the
commit it names.  A mismatch is a behaviour change of the host code: find it and remove it, never re-record."""
import ctypes as C
import json
import os

import pytest

from egc_amd import _C
from egc_amd.functional import padded_basis_stride

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_envelope.json")

S, M, X, N, V, D, Y = (_C.AGGR_SUM, _C.AGGR_MEAN, _C.AGGR_MAX, _C.AGGR_MIN, _C.AGGR_VAR, _C.AGGR_STD, _C.AGGR_SYMNORM)
RAW, LOOPED = _C.SET_RAW, _C.SET_LOOPED

EDGE_BOUNDS = (0, 1, 4096, 65535, 65536)          # max_tile_edges: around the 16-bit cursors of the tiles' CSR builds
TILE_NODE_BOUNDS = (1, 160, 2048)                 # max_tile_nodes of egc_batch_tile_nodes
GRAPH_SIZES = ((0, 0), (1000, 5000), (169343, 1166243), (3000000, 100000000))   # (n_nodes, n_edges) of the workspace query


def _layer(f_out, heads, bases, aggrs, agg_set, sym_set, loops_all=True, f_in=None, layout=_C.LAYOUT_HBA, act=_C.ACT_NONE,
           stride=None):
    """The arguments of _C.make_layer as a dict (what the table stores next to the results)."""
    if stride is None:          # the stride the layer classes choose; 0 = contiguous bases
        stride = padded_basis_stride(f_out, heads, bases)
        stride = 0 if stride == f_out // heads else stride
    return dict(in_channels=f_out if f_in is None else f_in, out_channels=f_out, num_heads=heads, num_bases=bases,
                aggr_codes=list(aggrs), agg_set=agg_set, sym_set=sym_set, loops_all_nodes=int(loops_all), weight_layout=layout,
                weight_act=act, basis_stride=stride)


def grid():
    g = []
    # ---- (1) every shape a static table names ----
    g.append(_layer(128, 8, 4, (S, M, X, Y), LOOPED, LOOPED))       # EGConv EGC-M north star
    g.append(_layer(128, 8, 4, (S, X, Y), LOOPED, LOOPED))          # ... with the mean folded into the sum's weighting
    g.append(_layer(128, 8, 4, (S, D, X, Y), LOOPED, LOOPED))       # ... with std in place of mean
    g.append(_layer(128, 8, 4, (Y,), LOOPED, LOOPED))               # EGConv EGC-S
    g.append(_layer(128, 8, 4, (Y, X, M), RAW, LOOPED))             # EfficientGraphConv EGC-M at d = 128
    g.append(_layer(128, 8, 4, (Y,), RAW, LOOPED))                  # EfficientGraphConv EGC-S at d = 128
    g.append(_layer(184, 8, 4, (Y,), RAW, LOOPED))                  # arxiv EGC-S
    g.append(_layer(136, 4, 4, (Y, X, M), RAW, LOOPED))             # arxiv EGC-M
    g.append(_layer(168, 8, 4, (Y,), RAW, LOOPED))                  # zinc / cifar EGC-S
    g.append(_layer(124, 4, 4, (S, D, X), RAW, LOOPED))             # zinc EGC-M add,std,max
    g.append(_layer(128, 4, 4, (Y, D, X), RAW, LOOPED))             # cifar EGC-M symadd,std,max
    g.append(_layer(296, 8, 4, (Y,), RAW, LOOPED))                  # molhiv EGC-S
    g.append(_layer(224, 4, 4, (S, M, X), RAW, LOOPED))             # molhiv EGC-M add,mean,max
    g.append(_layer(352, 8, 4, (Y,), LOOPED, LOOPED))               # ogbn-mag EGConv, symnorm
    g.append(_layer(352, 8, 4, (M,), LOOPED, LOOPED))               # ogbn-mag EGConv, mean
    g.append(_layer(300, 4, 4, (Y, N, X), RAW, LOOPED))             # ogbg-code EGC-M symadd,min,max
    g.append(_layer(304, 8, 8, (Y,), RAW, LOOPED))                  # ogbg-code EGC-S
    for f_out, heads in ((128, 8), (64, 4)):                        # relational EGC: a relation's raw adjacency, and the root term
        g.append(_layer(f_out, heads, 4, (M, X), RAW, RAW))
        g.append(_layer(f_out, heads, 4, (S,), RAW, RAW))
    # ---- (2) the edges of the envelopes ----
    # slots per row = B * stride / 4: 16 / 17 / 32 / 33 / 64 / 65 / 128 / 129
    for f_out, heads, bases in ((128, 8, 4), (136, 2, 1), (128, 4, 4), (264, 2, 1), (256, 4, 4), (520, 2, 1), (256, 2, 4), (516, 1, 1)):
        g.append(_layer(f_out, heads, bases, (S, M, X), RAW, LOOPED))
        g.append(_layer(f_out, heads, bases, (Y, V, N), RAW, LOOPED, loops_all=False))
    g.append(_layer(184, 8, 4, (Y,), RAW, LOOPED, stride=0))        # L % 4 != 0, bases left contiguous
    g.append(_layer(124, 4, 4, (S, D, X), RAW, LOOPED, stride=0))
    g.append(_layer(296, 8, 4, (Y,), RAW, LOOPED, stride=40))       # ... and padded, the stride given explicitly
    g.append(_layer(96, 8, 3, (S, M, X), RAW, LOOPED))              # B not a power of two
    g.append(_layer(120, 6, 5, (Y,), LOOPED, LOOPED))
    g.append(_layer(128, 8, 4, (S, M, X, N, V, D, Y, S), LOOPED, LOOPED))   # A = 8
    g.append(_layer(64, 4, 2, (S, M, X, N, Y), RAW, LOOPED))                # A = 5: one past the register-resident combine
    g.append(_layer(128, 8, 4, (S, M, X, Y), LOOPED, LOOPED, layout=_C.LAYOUT_HAB))
    g.append(_layer(128, 8, 4, (S, M, X, Y), LOOPED, LOOPED, act=_C.ACT_SOFTMAX))
    g.append(_layer(128, 8, 4, (Y, X, M), RAW, LOOPED, act=_C.ACT_SIGMOID))
    g.append(_layer(168, 8, 4, (Y,), RAW, LOOPED, act=_C.ACT_HARDTANH))
    g.append(_layer(128, 16, 4, (S, M, X, Y), LOOPED, LOOPED))      # four heads per basis
    g.append(_layer(128, 32, 4, (S,), RAW, RAW))                    # eight: beyond the epilogue's head blocks
    g.append(_layer(64, 4, 4, (S, M, X, Y), LOOPED, LOOPED))        # the backward's H = 4 form
    g.append(_layer(128, 8, 4, (S, M, N, Y), LOOPED, LOOPED))       # min: outside the one-launch backward
    for f_in in (4, 128, 132, 320, 324):                            # F_in: the narrow and the wide one-launch forms, and past them
        g.append(_layer(128, 8, 4, (S, M, X, Y), LOOPED, LOOPED, f_in=f_in))
        g.append(_layer(168, 8, 4, (Y,), RAW, LOOPED, f_in=f_in))
        g.append(_layer(300, 4, 4, (Y, N, X), RAW, LOOPED, f_in=f_in))
    g.append(_layer(128, 8, 4, (S, M, X, Y), LOOPED, LOOPED, f_in=6))       # F_in % 4 != 0
    return g


def envelope(lib, spec):
    """Every host-only query of one layer -> a dict of plain ints / lists (JSON's types)."""
    lay = _C.make_layer(**spec)
    p = C.byref(lay)
    return dict(
        bases_ld=lib.egc_bases_ld(p),
        workspace_bytes=[lib.egc_aggregate_workspace_bytes(p, n, e) for n, e in GRAPH_SIZES],
        train_stats_floats=lib.egc_train_stats_floats(p),
        tile_nodes=[[[lib.egc_batch_tile_nodes(p, t, e, post) for e in EDGE_BOUNDS] for t in TILE_NODE_BOUNDS] for post in (0, 1)],
        fused_tile_nodes=[[lib.egc_batch_fused_tile_nodes(p, e, post) for e in EDGE_BOUNDS] for post in (0, 1)],
        fused_tile_quantum=lib.egc_batch_fused_tile_quantum(p),
        fused_pack_bytes=lib.egc_batch_fused_pack_bytes(p),
        fused_bwd_tile_nodes=[lib.egc_batch_fused_bwd_tile_nodes(p, e) for e in EDGE_BOUNDS],
        fused_bwd_pack_bytes=lib.egc_batch_fused_bwd_pack_bytes(p),
    )


@pytest.fixture(scope="module")
def table():
    with open(GOLDEN) as f:
        return json.load(f)


def test_table_covers_the_grid(table):
    assert len(table["commit"]) == 40
    assert [c["layer"] for c in table["cases"]] == grid()
    assert table["edge_bounds"] == list(EDGE_BOUNDS) and table["tile_node_bounds"] == list(TILE_NODE_BOUNDS)
    assert table["graph_sizes"] == [list(s) for s in GRAPH_SIZES]
    # the grid reaches every branch of the envelopes: shapes inside and outside each of the batch paths
    for key in ("fused_tile_quantum", "fused_pack_bytes", "fused_bwd_pack_bytes"):
        vals = {c["expect"][key] for c in table["cases"]}
        assert 0 in vals and len(vals) > 1, key
    assert {c["expect"]["fused_tile_quantum"] for c in table["cases"]} == {0, 16, 32}


def test_launch_envelope_matches_the_recorded_table(table, monkeypatch):
    monkeypatch.delenv("EGC_STDVAR_REFERENCE", raising=False)
    lib = _C.load()
    wrong = []
    for case in table["cases"]:
        got = envelope(lib, case["layer"])
        for key, want in case["expect"].items():
            if got[key] != want:
                wrong.append((case["layer"], key, want, got[key]))
    assert not wrong, wrong[:5]
