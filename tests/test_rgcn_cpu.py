"""The R-GCN baseline layer and the REGC net without a GPU: the CPU restatement (tests/rgcn_ref.py) against the fixtures of the
reference's own RGCNConv / REGC.forward, the edge cases those fixtures must hold, and the host side of egc_amd.RGCNConv /
egc_amd.REGC (construction, parameter names, the import shim, argument errors)."""
import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from rgcn_ref import (LAYER_FIXTURES, NET_FIXTURES, csr_by_destination, load_rgcn_golden, reference_distance, rel_out,
                      rgcn_forward)

CHUNK = 256


def test_chunk_constant_is_the_fixtures():
    assert _C.load().egc_typed_mean_chunk() == CHUNK
    for name in LAYER_FIXTURES + NET_FIXTURES:
        assert load_rgcn_golden(name)["meta"]["chunk"] == CHUNK


@pytest.mark.parametrize("name", LAYER_FIXTURES)
def test_restatement_matches_reference_rgcnconv(name):
    """Bound: max(1e-5, 5 x the reference's own float32-vs-float64 distance on the fixture), against the float64 output."""
    g = load_rgcn_golden(name)
    dist = reference_distance(g)
    bound = max(1e-5, 5.0 * dist)
    for dtype in (np.float32, np.float64):
        out = rgcn_forward(g["x"], g["ei"], g["params"], g["meta"]["edge_types"], CHUNK, dtype)
        for k in g["meta"]["node_types"]:
            err = rel_out(out[k], g["out64"][k])
            assert err <= bound, f"{name} {k} {dtype.__name__}: error {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("name", LAYER_FIXTURES + NET_FIXTURES)
def test_fixtures_cover_the_edge_cases(name):
    g = load_rgcn_golden(name)
    m = g["meta"]
    sizes = {k: v.shape[0] for k, v in g["out32"].items()}
    kinds = [tuple(k) for k in m["edge_types"]]
    assert len(g["ei"]) == len(kinds) - 1 and any(k not in g["ei"] for k in kinds)     # one relation is left out
    assert any(ei.shape[1] == 7 for ei in g["ei"].values())                            # one relation has 7 edges
    longest = 0
    for key, ei in g["ei"].items():
        deg = np.bincount(ei[1], minlength=sizes[key[2]])
        assert deg[-3:].sum() == 0, key                                                # the last three targets receive nothing
        assert ei[0].max() < sizes[key[0]] and ei[1].max() < sizes[key[2]]
        longest = max(longest, int(deg.max()))
    assert longest > 2 * CHUNK + 1                                                     # a row of more than two chunks and one entry
    if name == "rgcn_odd":
        assert m["fin"] % 4 != 0 and m["fout"] % 4 != 0
    if name == "rgcn_mag_shape":
        assert (m["fin"], m["fout"]) == (128, 349) and sizes == dict(author=150, field_of_study=40, institution=12, paper=120)


def test_csr_keeps_the_edge_list_order_inside_a_row():
    ei = np.array([[5, 1, 7, 2, 9], [1, 0, 1, 0, 1]])
    rowptr, col = csr_by_destination(ei, 3)
    assert rowptr.tolist() == [0, 2, 5, 5] and col.tolist() == [1, 2, 5, 7, 9]


@pytest.mark.parametrize("name", LAYER_FIXTURES)
def test_rgcnconv_constructs_with_the_reference_names(name):
    g = load_rgcn_golden(name)
    m = g["meta"]
    conv = egc_amd.RGCNConv(m["fin"], m["fout"])
    assert list(conv.state_dict()) == [k for k, _ in m["param_shapes"]]
    assert {k: list(v.shape) for k, v in conv.state_dict().items()} == dict((k, s) for k, s in m["param_shapes"])
    conv.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    for k, v in conv.state_dict().items():
        assert torch.equal(v, torch.from_numpy(g["params"][k]))
    assert all(lin.bias is None for lin in conv.rel_lins.values()) and all(lin.bias is not None for lin in conv.root_lins.values())
    assert repr(conv) == f"RGCNConv({m['fin']}, {m['fout']})"


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_regc_constructs_with_the_reference_names(name):
    g = load_rgcn_golden(name)
    m = g["meta"]
    net = egc_amd.REGC(m["hidden"], m["num_layers"], m["dropout"], use_egc=m["use_egc"], egc_heads=m["heads"], egc_bases=m["bases"],
                       num_nodes_dict=m["sizes"], in_features=m["in_features"], num_classes=m["num_classes"])
    assert set(net.state_dict()) == {k for k, _ in m["param_shapes"]}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    assert set(net.embs) == set(m["node_types"]) - {"paper"}
    kinds = [type(c).__name__ for c in net.convs]
    assert kinds == (["REGConv"] * 2 if m["use_egc"] else ["RGCNConv"] * 2) + ["RGCNConv"]
    assert net.convs[-1].out_channels == m["num_classes"]
    for emb in net.embs.values():         # xavier-uniform: inside its bound, not the zeros of an uninitialised table
        bound = (6.0 / (emb.size(0) + emb.size(1))) ** 0.5
        assert float(emb.abs().max()) <= bound and float(emb.abs().max()) > 0.5 * bound


def test_regc_defaults_are_the_reference_constants():
    from egc_amd import relational as rel
    assert rel.NUM_NODES_DICT == dict(author=1134649, field_of_study=59965, institution=8740, paper=736389)
    assert (rel.IN_FEATURES, rel.NUM_CLASSES, rel.X_TYPES) == (128, 349, ["paper"])
    small = dict(author=3, field_of_study=3, institution=3, paper=3)
    net = egc_amd.REGC(16, 2, 0.5, num_nodes_dict=small)
    assert net.convs[0].in_channels == 128 and net.convs[-1].out_channels == 349 and len(net.convs) == 2
    assert (net.convs[0].num_heads, net.convs[0].num_bases) == (8, 4)


def test_import_shim_resolves():
    from experiments.rmag.models import REGC, REGConv, RGCNConv
    assert RGCNConv is egc_amd.RGCNConv and REGC is egc_amd.REGC and REGConv is egc_amd.REGConv


def test_argument_errors():
    conv = egc_amd.RGCNConv(8, 4)
    x = {k: torch.randn(5, 8) for k in conv.node_types}
    with pytest.raises(RuntimeError, match="not one of the layer's edge types"):
        conv(x, {("paper", "reviews", "paper"): None})
    with pytest.raises(RuntimeError, match="not one of the layer's node types"):
        conv(dict(x, venue=torch.randn(2, 8)), {})
    with pytest.raises(RuntimeError, match="expected \\(rows, 8\\)"):
        conv(dict(x, paper=torch.randn(5, 7)), {})
    with pytest.raises(RuntimeError, match="unsupported adjacency type"):
        conv(x, {("paper", "cites", "paper"): torch.zeros(5, 5)})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        conv(x, {})
    crow = torch.tensor([0, 1, 1, 1, 1], dtype=torch.int64)       # a [4, 5] adjacency where the features say [5, 5]
    bad = torch.sparse_csr_tensor(crow, torch.tensor([0]), torch.ones(1), size=(4, 5))
    with pytest.raises(RuntimeError):
        conv(x, {("paper", "cites", "paper"): bad})
    lib = _C.load()
    table = (_C.EgcTypedRel * 1)()
    assert lib.egc_typed_mean_workspace_bytes(table, 1, 128) == 0                    # no relation longer than a chunk
    table[0].rowptr, table[0].n_edges = 16, 1000                                     # (never dereferenced by the size query)
    assert lib.egc_typed_mean_workspace_bytes(table, 1, 30) == 4 * 8 * 16            # ceil(1000 / 256) slots of 8 lanes
    assert lib.egc_typed_mean_f32(table, 1, 4, 0, 0, None, 0, None, 0, None) == 1    # EGC_ERR_INVALID: width
    assert lib.egc_typed_mean_f32(table, 9, 4, 8, 0, None, 8, None, 0, None) == 4    # EGC_ERR_UNSUPPORTED: relations
