"""egc_amd.GATv2Conv and the fused edge-softmax aggregate kernels (egc_gatv2_forward_f32 / _backward_f32) on the GPU against the
float64 fixtures of the per-edge torch composition (tests/golden/gat).

Bound (the project's rule, test_mpnn_gpu.py): the relative max error against the float64 fixture is at most
max(1e-5, 5 x the composition's own float32-vs-float64 distance recorded for that quantity)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._gat import gatv2_aggregate, gatv2_aggregate_backward, gatv2_aggregate_lse
from gat_ref import CASES, CHUNK, layer_kwargs, load_gat_golden, rel_grad, rel_out

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_gat_golden(name)


def _build(name):
    g = fixture(name)
    layer = egc_amd.GATv2Conv(**layer_kwargs(g))
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    return g, layer.to(DEV), torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["ei"]).to(DEV)


def _train_step(name, graph=None):
    g, layer, x, ei = _build(name)
    x.requires_grad_(True)
    out = layer(x, ei if graph is None else graph(ei, x.size(0)))
    out.backward(torch.from_numpy(g["gout"]).to(DEV))
    return g, layer, x, out.detach()


def _projections(name):
    """[xl | xr] of the fixture's layer (one [N, 2 H C] array), att [H, C], a cotangent, the layer's arguments."""
    g, layer, x, ei = _build(name)
    with torch.no_grad():
        lr = torch.cat([layer.lin_l(x), layer.lin_r(x)], dim=1).contiguous()
    gen = torch.Generator().manual_seed(g["meta"]["seed"] + 50)
    gout = torch.randn(lr.size(0), lr.size(1) // 2, generator=gen).to(DEV)
    return g, lr, layer.att.detach()[0].contiguous(), gout, ei, dict(negative_slope=layer.negative_slope,
                                                                    add_self_loops=layer.add_self_loops)


@pytest.mark.parametrize("name", CASES)
def test_forward_matches_float64_fixture(name):
    g, layer, x, ei = _build(name)
    dist = g["meta"]["f32_vs_f64_out"]
    bound = max(1e-5, 5.0 * dist)
    with torch.no_grad():
        out = layer(x, ei)
    out_grad = layer(x, ei)
    assert out_grad.requires_grad and not out.requires_grad
    for what, o in (("no_grad", out), ("grad", out_grad.detach())):
        err = rel_out(o.cpu().numpy(), g["out64"])
        print(f"{name} {what}: measured {err:.3e}, composition f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{name} {what}: error {err:.3e}, composition f32-vs-f64 {dist:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("name", CASES)
def test_gradients_match_float64_fixture(name):
    g, layer, x, _ = _train_step(name)
    m = g["meta"]
    checks = [("x", x.grad, g["grad_x64"], m["f32_vs_f64_grad_x"])]
    checks += [(k, p.grad, g["grad64"][k], m["f32_vs_f64_grad"][k]) for k, p in layer.named_parameters()]
    assert len(checks) == 1 + len(g["grad64"])
    for k, got, want, dist in checks:
        bound, err = max(1e-5, 5.0 * dist), rel_grad(got.cpu().numpy(), want)
        print(f"{name} d {k}: measured {err:.3e}, composition f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{name} d {k}: error {err:.3e}, composition f32-vs-f64 {dist:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("name", ("messy", "hub", "h8c13", "mean", "noloops"))
def test_column_blocks_and_separate_arrays_give_the_same_bits(name):
    """gatv2_aggregate and its backward on the halves of one [N, 2 H C] array (leading dimension 2 H C) and on contiguous copies."""
    g, lr, att, gout, ei, kw = _projections(name)
    w = lr.size(1) // 2
    blocks = [lr[:, :w].requires_grad_(True), lr[:, w:].requires_grad_(True)]
    copies = [lr[:, :w].contiguous().requires_grad_(True), lr[:, w:].contiguous().requires_grad_(True)]
    atts = [att.clone().requires_grad_(True), att.clone().requires_grad_(True)]
    assert blocks[0].stride(0) == 2 * w and copies[0].stride(0) == w
    outs = []
    for (xl, xr), a in zip((blocks, copies), atts):
        out = gatv2_aggregate(xl, xr, a, ei, **kw)
        out.backward(gout)
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1])
    for a, b in zip(blocks + atts[:1], copies + atts[1:]):
        assert a.grad is not None and torch.equal(a.grad, b.grad)
    # the kernels on their own: (out, lse), then the backward writing the halves of ONE array
    out, lse = gatv2_aggregate_lse(lr[:, :w], lr[:, w:], att, ei, **kw)
    assert torch.equal(out, outs[0]) and lse.shape == (lr.size(0), att.size(0))
    dxl, dxr, datt = gatv2_aggregate_backward(lr[:, :w].detach(), lr[:, w:].detach(), att, ei, out, lse, gout, **kw)
    assert dxl.stride(0) == 2 * w and dxl.data_ptr() + 4 * w == dxr.data_ptr()
    assert torch.equal(dxl, blocks[0].grad) and torch.equal(dxr, blocks[1].grad) and torch.equal(datt, atts[0].grad)
    if name == "hub":
        n = g["meta"]["n"]
        assert np.bincount(g["ei"][1], minlength=n).max() > 2 * CHUNK + 1 and np.bincount(g["ei"][0], minlength=n).max() > 2 * CHUNK + 1


@pytest.mark.parametrize("name", ("hub", "w112h8", "h8c13", "mean"))
def test_two_runs_are_bit_identical(name):
    runs = []
    for _ in range(2):
        _, layer, x, out = _train_step(name)
        runs.append([out, x.grad] + [p.grad for p in layer.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


FORMS = dict(
    SparseTensor=lambda ei, n: egc_amd.SparseTensor(row=ei[1], col=ei[0], sparse_sizes=(n, n)),
    CSRGraph=lambda ei, n: egc_amd.CSRGraph.from_edge_index(ei, n),
    fast=lambda ei, n: egc_amd.CSRGraph.from_edge_index(ei, n, build="fast"),
    sort=lambda ei, n: egc_amd.CSRGraph.from_edge_index(ei, n, build="sort"))


@pytest.mark.parametrize("form", sorted(FORMS))
def test_graph_forms_and_builds_give_the_same_bits(form):
    _, layer, x, out = _train_step("messy")
    _, layer2, x2, out2 = _train_step("messy", FORMS[form])
    assert torch.equal(out, out2) and torch.equal(x.grad, x2.grad)
    for a, b in zip(layer.parameters(), layer2.parameters()):
        assert torch.equal(a.grad, b.grad)


def test_a_row_with_only_its_self_loop_returns_its_own_row():
    """alpha = 1: out_i == xl_i exactly and lse_i == s_ii (the isolated tail of messy, and rows whose only in-edges are loops)."""
    g, lr, att, _, ei, kw = _projections("messy")
    assert kw["add_self_loops"]
    w, n = lr.size(1) // 2, lr.size(0)
    out, lse = gatv2_aggregate_lse(lr[:, :w], lr[:, w:], att, ei, **kw)
    src, dst = g["ei"]
    alone = np.bincount(dst[src != dst], minlength=n) == 0
    assert alone.sum() >= 3
    rows = torch.from_numpy(np.nonzero(alone)[0]).to(DEV)
    assert torch.equal(out[rows], lr[rows, :w])
    h, c = att.shape
    z = (lr[rows, :w] + lr[rows, w:]).view(-1, h, c).double()
    s = (att.double() * torch.where(z > 0, z, kw["negative_slope"] * z)).sum(-1)
    assert float((lse[rows].double() - s).abs().max()) <= 1e-5 * max(1.0, float(s.abs().max()))
    # without self loops the same rows are empty: 0 and -inf
    out0, lse0 = gatv2_aggregate_lse(lr[:, :w], lr[:, w:], att, ei, negative_slope=kw["negative_slope"], add_self_loops=False)
    empty = torch.from_numpy(np.nonzero(np.bincount(dst, minlength=n) == 0)[0]).to(DEV)
    assert len(empty) >= 3 and float(out0[empty].abs().max()) == 0.0 and bool(torch.isinf(lse0[empty]).all()) and bool((lse0[empty] < 0).all())


def test_empty_rows_without_self_loops_give_zero_and_a_zero_gradient():
    g, layer, x, out = _train_step("noloops")
    empty = torch.from_numpy(np.nonzero(np.bincount(g["ei"][1], minlength=g["meta"]["n"]) == 0)[0]).to(DEV)
    assert len(empty) >= 3 and torch.equal(out[empty], layer.bias.detach().expand(len(empty), -1))
    never_source = torch.from_numpy(np.nonzero(np.bincount(g["ei"].ravel(), minlength=g["meta"]["n"]) == 0)[0]).to(DEV)
    assert len(never_source) >= 3 and float(x.grad[never_source].abs().max()) == 0.0


def test_bigscore_is_finite_everywhere():
    g, layer, x, out = _train_step("bigscore")
    assert g["meta"]["score_span"] >= 80.0
    for name, t in [("out", out), ("x", x.grad)] + [(k, p.grad) for k, p in layer.named_parameters()]:
        assert bool(torch.isfinite(t).all()), name
    _, lr, att, _, ei, kw = _projections("bigscore")
    w = lr.size(1) // 2
    _, lse = gatv2_aggregate_lse(lr[:, :w], lr[:, w:], att, ei, **kw)
    assert bool(torch.isfinite(lse).all()) and float(lse.max()) >= 80.0


def test_dropout_is_ignored_in_eval_mode():
    g, layer, x, ei = _build("slope")
    layer.dropout = 0.6
    with pytest.raises(NotImplementedError, match="attention dropout"):
        layer(x, ei)
    with torch.no_grad():
        out = layer.eval()(x, ei)
    assert rel_out(out.cpu().numpy(), g["out64"]) <= max(1e-5, 5.0 * g["meta"]["f32_vs_f64_out"])


def test_a_graph_without_edges():
    layer = egc_amd.GATv2Conv(8, 4, heads=2).to(DEV)
    x = torch.randn(5, 8, device=DEV, requires_grad=True)
    out = layer(x, torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    assert torch.allclose(out.detach(), (layer.lin_l(x) + layer.bias).detach(), atol=1e-5)      # the self loop alone: alpha = 1
    out.sum().backward()
    assert float(layer.att.grad.abs().max()) == 0.0 and float(layer.lin_r.weight.grad.abs().max()) == 0.0


def test_training_step_needs_no_edge_sized_array():
    """Peak memory of a training step stays below ONE [E, H C] float32 array (PyG keeps several)."""
    n, e, h, c = 4096, 262144, 8, 8
    gen = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, e), generator=gen).to(DEV)
    layer = egc_amd.GATv2Conv(h * c, c, heads=h).to(DEV)
    x = torch.randn(n, h * c, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(n, h * c, generator=gen).to(DEV)
    graph = egc_amd.CSRGraph.from_edge_index(ei, n)
    graph.transposed()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    layer(x, graph).backward(gout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes = {rise / (n * h * c * 4):.1f} arrays of N H C floats; one [E, H C] array is {e * h * c * 4} bytes")
    assert x.grad is not None and bool(torch.isfinite(x.grad).all()) and rise < e * h * c * 4
