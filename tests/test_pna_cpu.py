"""PNAConv without a GPU: the algebra (P / Q split, one-pass aggregators about the first entry, the two-record backward, scalers
behind the folded post o lin product) in float64 against the fixtures of the per-edge composition, the module's contract (state
dict, construction order, degree statistics, errors), and the properties the fixtures are named for."""
import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._pna import degree_statistics
from pna_ref import (ALL_AGGREGATORS, ALL_SCALERS, CASES, CHUNK, aggregate_forward, folded_from_params, layer_forward, load_pna_golden,
                     rel_grad, rel_out, scale_factors)


def _layer(g, **kw):
    m = g["meta"]
    return egc_amd.PNAConv(m["in_channels"], m["out_channels"], m["aggregators"], m["scalers"], torch.from_numpy(g["deg"]),
                           towers=m["towers"], divide_input=m["divide_input"], **kw)


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    g = load_pna_golden(name)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in g["params"].items()}
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    out = layer_forward(x, g["ei"], p, g["meta"])
    out.backward(torch.from_numpy(g["gout"]).double())
    errs = {"out": rel_out(out.detach().numpy(), g["out64"]), "x": rel_grad(x.grad.numpy(), g["grad_x64"])}
    errs.update({k: rel_grad(v.grad.numpy(), g["grad64"][k]) for k, v in p.items()})
    assert set(p) == set(g["grad64"])
    print(name, {k: f"{v:.1e}" for k, v in errs.items()})
    assert max(errs.values()) <= 1e-10, errs


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_and_strict_load(name):
    g = load_pna_golden(name)
    layer = _layer(g)
    t = g["meta"]["towers"]
    keys = [f"{nn}.{k}.0.{p}" for k in range(t) for nn in ("pre_nns", "post_nns") for p in ("weight", "bias")] + ["lin.weight", "lin.bias"]
    assert sorted(layer.state_dict().keys()) == sorted(keys) and not list(layer.buffers())
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    for k, v in layer.state_dict().items():
        assert v.shape == g["params"][k].shape and np.array_equal(v.numpy(), g["params"][k])


@pytest.mark.parametrize("name", ("messy", "nodivide", "all6"))
def test_construction_order_gives_the_seeded_initial_parameters(name):
    g = load_pna_golden(name)
    assert g["init"]
    torch.manual_seed(g["meta"]["seed"])
    layer = _layer(g)
    for k, v in layer.state_dict().items():
        assert np.array_equal(v.numpy(), g["init"][k]), k


def test_degree_statistics_from_a_histogram():
    hist = torch.tensor([3, 0, 5, 2])
    avg_lin, avg_log = degree_statistics(hist)
    assert avg_lin == pytest.approx((2 * 5 + 3 * 2) / 10, rel=1e-15)
    assert avg_log == pytest.approx((3 * np.log(1) + 5 * np.log(3) + 2 * np.log(4)) / 10, rel=1e-15)
    layer = egc_amd.PNAConv(4, 4, ["mean"], ["amplification"], hist)
    assert layer.avg_deg == {"lin": avg_lin, "log": avg_log}
    for name in CASES:
        g = load_pna_golden(name)
        lin, log = degree_statistics(g["deg"])
        assert lin == pytest.approx(g["meta"]["avg_lin"], rel=1e-14) and log == pytest.approx(g["meta"]["avg_log"], rel=1e-14)
    with pytest.raises(ValueError):
        degree_statistics(torch.zeros(3))
    with pytest.raises(ValueError):
        egc_amd.PNAConv(4, 4, ["mean"], ["amplification"], torch.tensor([7]))      # no node with an in-edge: avg_log = 0


def test_degree_histogram_on_the_three_graph_forms():
    g = load_pna_golden("messy")
    n, ei = g["meta"]["n"], torch.from_numpy(g["ei"])
    want = torch.from_numpy(g["deg"])
    assert want.dtype == torch.int64 and int(want.sum()) == n and int((torch.arange(len(want)) * want).sum()) == ei.size(1)
    got = egc_amd.degree_histogram(ei, n)
    assert got.dtype == torch.int64 and torch.equal(got, want)
    # without num_nodes the isolated tail is not counted: the nodes up to the largest index named
    assert int(egc_amd.degree_histogram(ei).sum()) == int(ei.max()) + 1
    order = torch.argsort(ei[1], stable=True)
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.bincount(ei[1], minlength=n), 0).int()
    csr = egc_amd.CSRGraph(n, ei.size(1), rowptr, ei[0][order].int(), order.int(), None, None, None, None)
    assert torch.equal(egc_amd.degree_histogram(csr), want)
    adj = object.__new__(egc_amd.SparseTensor)          # (the constructor builds its CSR on the GPU)
    adj._sizes, adj.graph = (n, n), csr
    assert torch.equal(egc_amd.degree_histogram(adj), want)
    with pytest.raises(RuntimeError):
        egc_amd.degree_histogram(ei.int())


def test_errors_of_the_contract():
    deg = torch.tensor([1, 2, 3])
    with pytest.raises(NotImplementedError, match="edge_dim"):
        egc_amd.PNAConv(8, 8, ["mean"], ["identity"], deg, edge_dim=4)
    with pytest.raises(NotImplementedError, match="pre_layers"):
        egc_amd.PNAConv(8, 8, ["mean"], ["identity"], deg, pre_layers=2)
    with pytest.raises(NotImplementedError, match="post_layers"):
        egc_amd.PNAConv(8, 8, ["mean"], ["identity"], deg, post_layers=3)
    with pytest.raises(ValueError, match="aggregator"):
        egc_amd.PNAConv(8, 8, ["mean", "median"], ["identity"], deg)
    with pytest.raises(ValueError, match="scaler"):
        egc_amd.PNAConv(8, 8, ["mean"], ["exponential"], deg)
    with pytest.raises(ValueError):
        egc_amd.PNAConv(8, 8, ["mean", "mean"], ["identity"], deg)
    with pytest.raises(AssertionError):
        egc_amd.PNAConv(10, 8, ["mean"], ["identity"], deg, towers=4, divide_input=True)
    with pytest.raises(AssertionError):
        egc_amd.PNAConv(8, 10, ["mean"], ["identity"], deg, towers=4)
    egc_amd.PNAConv(10, 8, ["mean"], ["identity"], deg, towers=4)                  # in_channels is free without divide_input
    layer = egc_amd.PNAConv(8, 8, ["mean"], ["identity"], deg, towers=2, divide_input=True)
    with pytest.raises(RuntimeError, match="expected"):
        layer(torch.zeros(5, 7), torch.zeros((2, 0), dtype=torch.int64))
    with pytest.raises(ValueError):
        egc_amd.pna_aggregate(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros((2, 0), dtype=torch.int64), ["mode"])
    with pytest.raises(ValueError):
        egc_amd.pna_scale_combine(torch.zeros(3, 4), torch.zeros(3, 4), torch.zeros((2, 0), dtype=torch.int64), ["cubic"], 1.0, 1.0)


def test_sizes_follow_towers_and_divide_input():
    deg = torch.tensor([1, 2, 3])
    a = egc_amd.PNAConv(12, 20, ["mean", "max"], ["identity", "linear", "attenuation"], deg, towers=2)
    assert (a.F_in, a.F_out) == (12, 10)
    assert a.pre_nns[1][0].weight.shape == (12, 24) and a.post_nns[0][0].weight.shape == (10, 7 * 12) and a.lin.weight.shape == (20, 20)
    b = egc_amd.PNAConv(12, 20, ["mean", "max"], ["identity"], deg, towers=2, divide_input=True)
    assert (b.F_in, b.F_out) == (6, 10) and b.post_nns[0][0].weight.shape == (10, 3 * 6)
    assert b._weights()[0].requires_grad                                 # with grad: folded inside autograd, every call
    with torch.no_grad():
        w_pq, b_pq, w_y, w_base, b_base = b._weights()
        assert w_pq.shape == (24, 12) and b_pq.shape == (24,) and w_y.shape == (20, 24) and w_base.shape == (20, 12) and b_base.shape == (20,)
        assert float(b_pq[:12].abs().max()) == 0.0
        assert b._weights()[0] is w_pq                               # kept between calls that need no gradient ...
        b.lin.bias.add_(1.0)
        assert b._weights()[0] is not w_pq                           # ... until a parameter changes
        w_pq, _, w_y, _, _ = a._weights()
    assert w_pq.shape == (48, 12) and w_y.shape == (60, 48)


def test_the_hub_has_its_long_row_in_both_directions():
    for name in ("hub", "ties"):
        g = load_pna_golden(name)
        n = g["meta"]["n"]
        assert np.bincount(g["ei"][1], minlength=n).max() > 2 * CHUNK + 1
        assert np.bincount(g["ei"][0], minlength=n).max() > 2 * CHUNK + 1


def test_the_ties_fixture_has_tied_maxima_within_and_across_chunks():
    g = load_pna_golden("ties")
    m = g["meta"]
    w_pq, _, _, _, _ = folded_from_params({k: torch.from_numpy(v) for k, v in g["params"].items()}, m)
    P = (torch.from_numpy(g["x"]) @ w_pq[:w_pq.shape[0] // 2].t()).numpy()
    assert np.array_equal(P, np.round(P))
    src, dst = g["ei"]
    row = int(np.bincount(dst).argmax())
    v = P[src[dst == row]]                                           # the long row's entries in edge-list order
    assert len(v) > 2 * CHUNK + 1
    for at in (v == v.max(axis=0), v == v.min(axis=0)):
        assert (at[:CHUNK].sum(axis=0) > 1).any()                                        # tied inside the first chunk
        assert (at[:CHUNK].any(axis=0) & at[CHUNK:].any(axis=0)).any()                   # and between chunks
    fwd = aggregate_forward(P, np.zeros_like(P), g["ei"], ("min", "max"), CHUNK, np.float32)
    e = np.nonzero(dst == row)[0]
    assert np.array_equal(fwd["arg_max"][row], e[(v == v.max(axis=0)).argmax(axis=0)])     # the first edge of the edge list
    assert np.array_equal(fwd["arg_min"][row], e[(v == v.min(axis=0)).argmax(axis=0)])


def test_an_empty_row_scales_like_degree_one_and_aggregates_to_zero():
    f = scale_factors(np.array([0, 1, 5]), ALL_SCALERS, 2.5, 1.2, np.float64)
    assert np.array_equal(f[0], f[1]) and not np.array_equal(f[1], f[2])
    assert f[1].tolist() == [1.0, np.log(2.0) / 1.2, 1.2 / np.log(2.0), 1 / 2.5, 2.5]
    ei = np.array([[0, 1, 1], [1, 1, 2]])                           # node 0 has no in-edge
    P = np.arange(12, dtype=np.float64).reshape(3, 4)
    fwd = aggregate_forward(P, np.full((3, 4), 100.0), ei, ALL_AGGREGATORS, CHUNK, np.float64)
    agg = fwd["agg"].reshape(3, 6, 4)
    assert np.array_equal(agg[0, :5], np.zeros((5, 4))) and np.array_equal(agg[0, 5], np.full(4, np.sqrt(1e-5)))   # Q is not added
    assert (fwd["arg_min"][0] == -1).all() and (fwd["arg_max"][0] == -1).all()
    assert np.array_equal(agg[1, 0], P[0] + P[1] + 200.0) and np.array_equal(agg[1, 4], np.full(4, 4.0))           # sum; var of {P0, P1}
    assert np.array_equal(agg[2, 4], np.zeros(4)) and np.array_equal(fwd["arg_max"][2], np.full(4, 2))
