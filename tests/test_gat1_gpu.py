"""egc_amd.GATConv (GAT v1) and the additive-score edge-softmax aggregate kernels (egc_gat_forward_f32 / _backward_f32) on the GPU
against the float64 fixtures of the per-edge torch composition (tests/golden/gat1).

Bound (the project's rule, test_mpnn_gpu.py and test_gat_gpu.py): the relative max error against the float64 fixture is at most
max(1e-5, 5 x the composition's own float32-vs-float64 distance recorded for that quantity)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._gat import _GatFused, _ext_width, gat_aggregate, gat_aggregate_backward, gat_aggregate_lse
from gat1_ref import CASES, CHUNK, layer_kwargs, load, rel_grad, rel_out
from gat_ref import layer_kwargs as v2_layer_kwargs, load_gat_golden

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load(name)


def _build(name):
    g = fixture(name)
    layer = egc_amd.GATConv(**layer_kwargs(g))
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    return g, layer.to(DEV), torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["ei"]).to(DEV)


def _train_step(name, graph=None):
    g, layer, x, ei = _build(name)
    x.requires_grad_(True)
    out = layer(x, ei if graph is None else graph(ei, x.size(0)))
    out.backward(torch.from_numpy(g["gout"]).to(DEV))
    return g, layer, x, out.detach()


def _projections(name):
    """ext = [xl | a_src | a_dst | pad] of the fixture's layer (ONE array), (H, C), a cotangent, the layer's arguments."""
    g, layer, x, ei = _build(name)
    with torch.no_grad():
        ext = torch.nn.functional.linear(x, layer.extended_weight()).contiguous()
    h, c = layer.heads, layer.out_channels
    assert ext.size(1) == _ext_width(h, c) and ext.size(1) % 4 == 0
    gen = torch.Generator().manual_seed(g["meta"]["seed"] + 50)
    gout = torch.randn(ext.size(0), h * c, generator=gen).to(DEV)
    return g, ext, (h, c), gout, ei, dict(negative_slope=layer.negative_slope, add_self_loops=layer.add_self_loops)


def _blocks(ext, h, c):
    w = h * c
    return ext[:, :w], ext[:, w:w + h], ext[:, w + h:w + 2 * h]


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
    bad = []
    for k, got, want, dist in checks:
        bound, err = max(1e-5, 5.0 * dist), rel_grad(got.cpu().numpy(), want)
        print(f"{name} d {k}: measured {err:.3e}, composition f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        if not err <= bound:
            bad.append(f"d {k}: error {err:.3e}, composition f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("name", ("messy", "hub", "w152h8", "w152h1", "w304h1", "mean", "noloops"))
def test_fused_array_and_separate_arrays_give_the_same_bits(name):
    """The fused Function on [xl | a_src | a_dst | pad], gat_aggregate on its column blocks and on three contiguous copies."""
    g, ext, (h, c), gout, ei, kw = _projections(name)
    n, w = ext.size(0), h * c
    graph = egc_amd.CSRGraph.from_edge_index(ei, n)
    fused = ext.clone().requires_grad_(True)
    out_f = _GatFused.apply(fused, h, c, graph, kw["negative_slope"], kw["add_self_loops"])
    out_f.backward(gout)
    assert fused.grad.shape == ext.shape and (ext.size(1) == w + 2 * h or float(fused.grad[:, w + 2 * h:].abs().max()) == 0.0)
    blocks = [b.requires_grad_(True) for b in _blocks(ext, h, c)]
    copies = [b.detach().contiguous().requires_grad_(True) for b in _blocks(ext, h, c)]
    assert blocks[0].stride(0) == ext.size(1) and blocks[1].stride(0) == ext.size(1) and copies[1].stride(0) == h
    outs = []
    for leaves in (blocks, copies):
        out = gat_aggregate(*leaves, ei, **kw)
        out.backward(gout)
        outs.append(out.detach())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], out_f.detach())
    for a, b, f in zip(blocks, copies, _blocks(fused.grad, h, c)):
        assert a.grad is not None and torch.equal(a.grad, b.grad) and torch.equal(a.grad, f)
    # the kernels on their own: (out, lse), then the backward writing the blocks of ONE array
    xl, a_src, a_dst = (b.detach() for b in _blocks(ext, h, c))
    out, lse = gat_aggregate_lse(xl, a_src, a_dst, ei, **kw)
    assert torch.equal(out, outs[0]) and lse.shape == (n, h)
    dxl, das, dad = gat_aggregate_backward(xl, a_src, a_dst, ei, out, lse, gout, **kw)
    assert dxl.stride(0) == ext.size(1) and dxl.data_ptr() + 4 * w == das.data_ptr() and das.data_ptr() + 4 * h == dad.data_ptr()
    assert torch.equal(dxl, blocks[0].grad) and torch.equal(das, blocks[1].grad) and torch.equal(dad, blocks[2].grad)
    if name == "hub":
        assert np.bincount(g["ei"][1], minlength=n).max() > 2 * CHUNK + 1 and np.bincount(g["ei"][0], minlength=n).max() > 2 * CHUNK + 1


@pytest.mark.parametrize("name", ("hub", "w152h8", "w240h8", "w304h1", "mean"))
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
    g, ext, (h, c), _, ei, kw = _projections("messy")
    assert kw["add_self_loops"]
    n = ext.size(0)
    xl, a_src, a_dst = _blocks(ext, h, c)
    out, lse = gat_aggregate_lse(xl, a_src, a_dst, ei, **kw)
    src, dst = g["ei"]
    alone = np.bincount(dst[src != dst], minlength=n) == 0
    assert alone.sum() >= 3
    rows = torch.from_numpy(np.nonzero(alone)[0]).to(DEV)
    assert torch.equal(out[rows], xl[rows])
    z = a_src[rows] + a_dst[rows]                                  # one float32 addition and one product: the kernel's own
    assert torch.equal(lse[rows], torch.where(z > 0, z, torch.tensor(kw["negative_slope"], device=DEV) * z))
    # without self loops the same rows are empty: 0 and -inf
    out0, lse0 = gat_aggregate_lse(xl, a_src, a_dst, ei, negative_slope=kw["negative_slope"], add_self_loops=False)
    empty = torch.from_numpy(np.nonzero(np.bincount(dst, minlength=n) == 0)[0]).to(DEV)
    assert len(empty) >= 3 and float(out0[empty].abs().max()) == 0.0 and bool(torch.isinf(lse0[empty]).all()) and bool((lse0[empty] < 0).all())


def test_empty_rows_without_self_loops_give_zero_and_a_zero_gradient():
    g, layer, x, out = _train_step("noloops")
    n = g["meta"]["n"]
    empty = torch.from_numpy(np.nonzero(np.bincount(g["ei"][1], minlength=n) == 0)[0]).to(DEV)
    assert len(empty) >= 3 and torch.equal(out[empty], layer.bias.detach().expand(len(empty), -1))
    never_source = torch.from_numpy(np.nonzero(np.bincount(g["ei"].ravel(), minlength=n) == 0)[0]).to(DEV)
    assert len(never_source) >= 3 and float(x.grad[never_source].abs().max()) == 0.0
    # the kernels on their own: an empty row's d a_dst and a never-read row's d xl and d a_src are exactly zero
    _, ext, (h, c), gout, ei, kw = _projections("noloops")
    xl, a_src, a_dst = _blocks(ext, h, c)
    o, lse = gat_aggregate_lse(xl, a_src, a_dst, ei, **kw)
    dxl, das, dad = gat_aggregate_backward(xl, a_src, a_dst, ei, o, lse, gout, **kw)
    assert bool(torch.isinf(lse[empty]).all()) and float(o[empty].abs().max()) == 0.0 and float(dad[empty].abs().max()) == 0.0
    assert float(dxl[never_source].abs().max()) == 0.0 and float(das[never_source].abs().max()) == 0.0


def test_bigscore_is_finite_everywhere():
    g, layer, x, out = _train_step("bigscore")
    assert g["meta"]["score_span"] >= 80.0
    for name, t in [("out", out), ("x", x.grad)] + [(k, p.grad) for k, p in layer.named_parameters()]:
        assert bool(torch.isfinite(t).all()), name
    _, ext, (h, c), _, ei, kw = _projections("bigscore")
    _, lse = gat_aggregate_lse(*_blocks(ext, h, c), ei, **kw)
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
    layer = egc_amd.GATConv(8, 4, heads=2).to(DEV)
    x = torch.randn(5, 8, device=DEV, requires_grad=True)
    out = layer(x, torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    assert torch.allclose(out.detach(), (layer.lin_src(x) + layer.bias).detach(), atol=1e-5)      # the self loop alone: alpha = 1
    out.sum().backward()
    # alpha = 1 is a constant: both att gradients vanish.  The source pass forms g . xl - D per entry from the same products in
    # the same order: exactly 0.  The destination pass's factored g . (w xl) - D w rounds w into the products: 0 within a few
    # float32 roundings of |g . xl| = O(1) per row, five rows
    assert float(layer.att_src.grad.abs().max()) == 0.0 and float(layer.att_dst.grad.abs().max()) <= 1e-6
    assert float(x.grad.abs().max()) > 0.0
    loopless = egc_amd.GATConv(8, 4, heads=2, add_self_loops=False).to(DEV)
    out = loopless(x, torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    assert torch.equal(out.detach(), loopless.bias.detach().expand(5, -1))


def test_training_step_needs_no_edge_sized_array():
    """Peak memory of a training step stays below ONE [E, H C] float32 array (PyG keeps several)."""
    n, e, h, c = 4096, 262144, 8, 8
    gen = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, e), generator=gen).to(DEV)
    layer = egc_amd.GATConv(h * c, c, heads=h).to(DEV)
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


def test_gatv2_still_meets_its_own_recorded_bound():
    """GATv2Conv shares the lane mapping's header with this layer: fixture messy of tests/golden/gat, forward and gradients."""
    g = load_gat_golden("messy")
    layer = egc_amd.GATv2Conv(**v2_layer_kwargs(g))
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    layer, x, ei = layer.to(DEV), torch.from_numpy(g["x"]).to(DEV).requires_grad_(True), torch.from_numpy(g["ei"]).to(DEV)
    out = layer(x, ei)
    out.backward(torch.from_numpy(g["gout"]).to(DEV))
    m = g["meta"]
    assert rel_out(out.detach().cpu().numpy(), g["out64"]) <= max(1e-5, 5.0 * m["f32_vs_f64_out"])
    assert rel_grad(x.grad.cpu().numpy(), g["grad_x64"]) <= max(1e-5, 5.0 * m["f32_vs_f64_grad_x"])
    for k, p in layer.named_parameters():
        assert rel_grad(p.grad.cpu().numpy(), g["grad64"][k]) <= max(1e-5, 5.0 * m["f32_vs_f64_grad"][k]), k
