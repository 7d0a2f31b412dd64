"""egc_amd.Mpnn and the message-aggregate kernels (egc_mpnn_message_f32 / _backward_f32) on the GPU against the fixtures of the
reference's own Mpnn and against the sequential CPU restatement in the documented order (tests/mpnn_ref.py).

Bound of everything compared with a reference-derived fixture (the rule of test_rgcn_gpu.py): the relative max error against the
float64 fixture is at most max(1e-5, 5 x the reference's own float32-vs-float64 distance on that fixture) -- for the output the
distance between the two outputs stored, for a gradient the distance the generator recorded for that gradient.
tests/test_mpnn_shapes_gpu.py runs the two kernels at every row length and width they dispatch on."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._mpnn import mpnn_message, mpnn_message_arg, mpnn_message_backward
from mpnn_ref import (CASES, CHUNK, MAX_CASES, folded_weights, load_mpnn_golden, message_backward, message_forward,
                      reference_distance, rel_grad, rel_out)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_mpnn_golden(name)


@functools.lru_cache(maxsize=None)
def restated(name):
    """P, Q (float32, from the fixture's parameters), a fixed d m, and the float32 restatement of both kernels on them."""
    g = fixture(name)
    m = g["meta"]
    w_pq, b_pq, _, _ = folded_weights({k: torch.from_numpy(v) for k, v in g["params"].items()}, m["towers"])
    pq = (torch.from_numpy(g["x"]) @ w_pq.t() + b_pq).numpy()
    P, Q = np.ascontiguousarray(pq[:, :m["d"]]), np.ascontiguousarray(pq[:, m["d"]:])
    dm = np.random.default_rng(m["seed"] + 50).standard_normal(P.shape).astype(np.float32)
    want_m, want_arg = message_forward(P, Q, g["ei"], m["aggr"], CHUNK, np.float32)
    want_dP, want_dQ = message_backward(dm, g["ei"], m["aggr"], want_arg, CHUNK, np.float32)
    return dict(P=P, Q=Q, dm=dm, m=want_m, arg=want_arg, dP=want_dP, dQ=want_dQ)


def _build(name):
    g = fixture(name)
    m = g["meta"]
    layer = egc_amd.Mpnn(m["aggr"], m["d"], m["d"], towers=m["towers"])
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    return g, layer.to(DEV), torch.from_numpy(g["x"]).to(DEV), torch.from_numpy(g["ei"]).to(DEV)


def _train_step(name):
    g, layer, x, ei = _build(name)
    x.requires_grad_(True)
    out = layer(x, ei)
    out.backward(torch.from_numpy(g["gout"]).to(DEV))
    return g, layer, x, out.detach()


@pytest.mark.parametrize("name", CASES)
def test_forward_matches_reference_fixture(name):
    g, layer, x, ei = _build(name)
    dist = reference_distance(g)
    bound = max(1e-5, 5.0 * dist)
    with torch.no_grad():
        out = layer(x, ei)
    out_grad = layer(x, ei)
    assert out_grad.requires_grad and not out.requires_grad
    for what, o in (("no_grad", out), ("grad", out_grad.detach())):
        err = rel_out(o.cpu().numpy(), g["out64"])
        print(f"{name} {what}: measured {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{name} {what}: error {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("name", CASES)
def test_gradients_match_float64_fixture(name):
    g, layer, x, _ = _train_step(name)
    m = g["meta"]
    checks = [("x", x.grad, g["grad_x64"], m["f32_vs_f64_grad_x"])]
    checks += [(k, p.grad, g["grad64"][k], m["f32_vs_f64_grad"][k]) for k, p in layer.named_parameters()]
    assert len(checks) == 1 + len(g["grad64"])
    for k, got, want, dist in checks:
        bound, err = max(1e-5, 5.0 * dist), rel_grad(got.cpu().numpy(), want)
        print(f"{name} d {k}: measured {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{name} d {k}: error {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}"


@pytest.mark.parametrize("form", ("edge_index", "SparseTensor", "CSRGraph"))
def test_graph_forms_give_the_same_bits(form):
    g, layer, x, ei = _build("messy_max")
    n = x.size(0)
    graph = dict(edge_index=ei, SparseTensor=egc_amd.SparseTensor(row=ei[1], col=ei[0], sparse_sizes=(n, n)),
                 CSRGraph=egc_amd.CSRGraph.from_edge_index(ei, n))[form]
    with torch.no_grad():
        assert torch.equal(layer(x, graph), layer(x, ei))


@pytest.mark.parametrize("name", CASES)
def test_message_kernels_have_the_bits_of_the_documented_order(name):
    """m, arg, d P and d Q against the sequential float32 loops, the hub's long row and long transposed row included."""
    g, r = fixture(name), restated(name)
    aggr = g["meta"]["aggr"]
    ei = torch.from_numpy(g["ei"]).to(DEV)
    P, Q, dm = (torch.from_numpy(r[k]).to(DEV) for k in ("P", "Q", "dm"))
    if name.startswith("hub"):
        n = g["meta"]["n"]
        assert np.bincount(g["ei"][1], minlength=n).max() > 2 * CHUNK + 1 and np.bincount(g["ei"][0], minlength=n).max() > 2 * CHUNK + 1
    m = mpnn_message(P, Q, ei, aggr)
    assert torch.equal(m.cpu(), torch.from_numpy(r["m"]))
    arg = None
    if aggr == "max":
        m2, arg = mpnn_message_arg(P, Q, ei)
        assert torch.equal(m2, m) and torch.equal(arg.cpu(), torch.from_numpy(r["arg"]))
    # the inference form: a column block of a wider array, the other columns untouched
    d = Q.size(1)
    wide = torch.full((Q.size(0), 2 * d + 3), 7.0, device=DEV)
    block = mpnn_message(P, Q, ei, aggr, out=wide, out_col=d)
    assert torch.equal(block, m) and torch.equal(wide[:, d:2 * d], m)
    assert bool((wide[:, :d] == 7.0).all()) and bool((wide[:, 2 * d:] == 7.0).all())
    dP, dQ = mpnn_message_backward(dm, ei, aggr, arg)
    assert torch.equal(dP.cpu(), torch.from_numpy(r["dP"]))
    assert torch.equal(dQ.cpu(), torch.from_numpy(r["dQ"]))
    # the same through autograd
    P.requires_grad_(True), Q.requires_grad_(True)
    mpnn_message(P, Q, ei, aggr).backward(dm)
    assert torch.equal(P.grad, dP) and torch.equal(Q.grad, dQ)
    with pytest.raises(RuntimeError, match="inference form"):
        mpnn_message(P, Q, ei, aggr, out=wide)


def test_ties_go_to_the_first_edge():
    g, r = fixture("ties_max"), restated("ties_max")
    ei = torch.from_numpy(g["ei"]).to(DEV)
    _, arg = mpnn_message_arg(torch.from_numpy(r["P"]).to(DEV), torch.from_numpy(r["Q"]).to(DEV), ei)
    assert torch.equal(arg.cpu(), torch.from_numpy(g["arg"]))                # the reference's first-edge argument, exactly
    # the fixture does hold ties between different edges: some (row, column) maximum is attained more than once
    src, dst = g["ei"]
    tied = 0
    for row in range(g["meta"]["n"]):
        e = np.nonzero(dst == row)[0]
        if len(e):
            tied += int(((r["P"][src[e]] == r["P"][src[e]].max(axis=0)).sum(axis=0) > 1).sum())
    assert tied > 0
    g, layer, x, _ = _train_step("ties_max")
    dist = g["meta"]["f32_vs_f64_grad_x"]
    bound, err = max(1e-5, 5.0 * dist), rel_grad(x.grad.cpu().numpy(), g["grad_x64"])
    print(f"ties_max d x: measured {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
    assert err <= bound


@pytest.mark.parametrize("name", ("hub_add", "hub_max", "odd_max", "w116_max"))
def test_two_runs_are_bit_identical(name):
    runs = []
    for _ in range(2):
        _, layer, x, out = _train_step(name)
        runs.append([out, x.grad] + [p.grad for p in layer.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_a_graph_without_edges():
    layer = egc_amd.Mpnn("max", 8, 8, towers=2).to(DEV)
    x = torch.randn(5, 8, device=DEV, requires_grad=True)
    out = layer(x, torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    _, _, w_out, b_out = layer._weights()
    assert torch.allclose(out, x @ w_out[:, 8:].t() + b_out, atol=1e-5)      # m = 0 everywhere
    out.sum().backward()
    assert float(layer.message_layer[0].weight.grad.abs().max()) == 0.0


def test_training_step_needs_no_edge_sized_array():
    """The point of the layer: peak memory of a training step stays below the ONE [E, d] float32 message tensor the reference
    materialises (it keeps that and the [E, 2 d] concatenation)."""
    n, e, d = 4096, 262144, 64
    gen = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, e), generator=gen).to(DEV)
    layer = egc_amd.Mpnn("max", d, d, towers=4).to(DEV)
    x = torch.randn(n, d, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(n, d, generator=gen).to(DEV)
    graph = egc_amd.CSRGraph.from_edge_index(ei, n)
    graph.transposed()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    layer(x, graph).backward(gout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes = {rise / (n * d * 4):.1f} arrays of N d floats; one message tensor is {e * d * 4} bytes")
    assert x.grad is not None and rise < e * d * 4
