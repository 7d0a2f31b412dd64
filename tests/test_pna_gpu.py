"""egc_amd.PNAConv and the kernels of egc_pna.hip on the GPU against the fixtures of the per-edge composition of PyG's formulas
(tests/golden/make_golden_pna.py) and against the sequential CPU restatement in the documented order (tests/pna_ref.py).

Bound of everything compared with a fixture (the rule of test_mpnn_gpu.py): the relative max error against the float64 fixture is
at most max(1e-5, 5 x the generator's own float32-vs-float64 distance for that quantity).  Everything the kernels write -- agg,
both args, mu, v, d P, d Q, the combine and its backward -- is ``torch.equal`` to the float32 restatement: the std columns (sqrt) and
the scaler factors (double log and division, rounded once) are correctly rounded operations on both sides, so no column needs
the 2-ulp allowance.  tests/test_pna_shapes_gpu.py runs the kernels at every row length and width they dispatch on."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._pna import pna_aggregate_saved, pna_scale_combine_backward
from pna_ref import (ALL_AGGREGATORS, CASES, CHUNK, aggregate_backward, aggregate_forward, folded_from_params, load_pna_golden,
                     rel_grad, rel_out, scale_combine, scale_combine_backward)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_pna_golden(name)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def restated(name, aggregators=None):
    """P, Q (float32, from the fixture's parameters), fixed cotangents, and the float32 restatement of the kernels on them."""
    g = fixture(name)
    m = g["meta"]
    aggregators = tuple(m["aggregators"]) if aggregators is None else aggregators
    w_pq, b_pq, _, _, _ = folded_from_params({k: torch.from_numpy(v) for k, v in g["params"].items()}, m)
    pq = (torch.from_numpy(g["x"]) @ w_pq.t() + b_pq).numpy()
    w = pq.shape[1] // 2
    P, Q = np.ascontiguousarray(pq[:, :w]), np.ascontiguousarray(pq[:, w:])
    rng = np.random.default_rng(m["seed"] + 50)
    dagg = rng.standard_normal((P.shape[0], len(aggregators) * w)).astype(np.float32)
    fwd = aggregate_forward(P, Q, g["ei"], aggregators, CHUNK, np.float32)
    dP, dQ = aggregate_backward(dagg, g["ei"], aggregators, P, fwd, CHUNK, np.float32)
    return dict(P=P, Q=Q, dagg=dagg, fwd=fwd, dP=dP, dQ=dQ, aggregators=aggregators, w=w)


def _build(name):
    g = fixture(name)
    m = g["meta"]
    layer = egc_amd.PNAConv(m["in_channels"], m["out_channels"], m["aggregators"], m["scalers"], torch.from_numpy(g["deg"]),
                            towers=m["towers"], divide_input=m["divide_input"])
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    return g, layer.to(DEV), _dev(g["x"]), _dev(g["ei"])


def _train_step(name):
    g, layer, x, ei = _build(name)
    x.requires_grad_(True)
    out = layer(x, ei)
    out.backward(_dev(g["gout"]))
    return g, layer, x, out.detach()


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
        print(f"{name} {what}: measured {err:.3e}, generator f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        assert err <= bound, f"{name} {what}: error {err:.3e}, generator f32-vs-f64 {dist:.3e}, bound {bound:.3e}"


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
        print(f"{name} d {k}: measured {err:.3e}, generator f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        if not err <= bound:
            bad.append(f"d {k}: error {err:.3e}, generator f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("form", ("edge_index", "SparseTensor", "CSRGraph"))
def test_graph_forms_give_the_same_bits(form):
    g, layer, x, ei = _build("messy")
    n = x.size(0)
    graph = dict(edge_index=ei, SparseTensor=egc_amd.SparseTensor(row=ei[1], col=ei[0], sparse_sizes=(n, n)),
                 CSRGraph=egc_amd.CSRGraph.from_edge_index(ei, n))[form]
    with torch.no_grad():
        assert torch.equal(layer(x, graph), layer(x, ei))
    assert torch.equal(egc_amd.degree_histogram(graph, n).cpu(), torch.from_numpy(g["deg"]))


def _eq(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert torch.equal(got.cpu(), want), f"{what}: {int((got.cpu() != want).sum())} of {want.numel()} elements differ"


def _check_kernels(name, aggregators=None):
    g, r = fixture(name), restated(name, aggregators)
    aggregators, w, fwd = r["aggregators"], r["w"], r["fwd"]
    ei = _dev(g["ei"])
    P, Q, dagg = (_dev(r[k]) for k in ("P", "Q", "dagg"))
    agg = egc_amd.pna_aggregate(P, Q, ei, aggregators)
    _eq(agg, fwd["agg"], f"{name} agg")
    agg2, arg_min, arg_max, mu, var = pna_aggregate_saved(P, Q, ei, aggregators)
    assert torch.equal(agg2, agg)
    for k, t in (("arg_min", arg_min), ("arg_max", arg_max), ("mu", mu), ("var", var)):
        assert (t is None) == (fwd[k] is None), k
        if t is not None:
            _eq(t, fwd[k], f"{name} {k}")
    # the inference form: a column block of a wider array, the other columns untouched
    wide = torch.full((Q.size(0), agg.size(1) + w + 3), 7.0, device=DEV)
    block = egc_amd.pna_aggregate(P, Q, ei, aggregators, out=wide, out_col=w)
    assert torch.equal(block, agg) and torch.equal(wide[:, w:w + agg.size(1)], agg)
    assert bool((wide[:, :w] == 7.0).all()) and bool((wide[:, w + agg.size(1):] == 7.0).all())
    dP, dQ = egc_amd.pna_aggregate_backward(dagg, ei, aggregators, P=P, arg_min=arg_min, arg_max=arg_max, mu=mu, var=var)
    _eq(dP, r["dP"], f"{name} d P")
    _eq(dQ, r["dQ"], f"{name} d Q")
    # the same through autograd
    P.requires_grad_(True), Q.requires_grad_(True)
    egc_amd.pna_aggregate(P, Q, ei, aggregators).backward(dagg)
    assert torch.equal(P.grad, dP) and torch.equal(Q.grad, dQ)
    with pytest.raises(RuntimeError, match="inference form"):
        egc_amd.pna_aggregate(P, Q, ei, aggregators, out=wide)
    return agg, dP, dQ


@pytest.mark.parametrize("name", CASES)
def test_aggregate_kernels_have_the_bits_of_the_documented_order(name):
    """agg, both args, mu, d P and d Q against the sequential float32 loops, the hub's long row and long transposed row included."""
    g = fixture(name)
    if name in ("hub", "ties"):
        n = g["meta"]["n"]
        assert np.bincount(g["ei"][1], minlength=n).max() > 2 * CHUNK + 1 and np.bincount(g["ei"][0], minlength=n).max() > 2 * CHUNK + 1
    _check_kernels(name)


@pytest.mark.parametrize("name", ("messy", "hub", "w116"))
def test_sublists_give_the_bits_of_the_full_list(name):
    """A list without var / std (no shift, no second moment carried) and one without min / max (no positions carried) run other
    instantiations of the kernels; the blocks they share with the full six-aggregator list have the same bits."""
    r = restated(name, ALL_AGGREGATORS)
    w = r["w"]
    ei, P, Q = _dev(fixture(name)["ei"]), _dev(r["P"]), _dev(r["Q"])
    full = egc_amd.pna_aggregate(P, Q, ei, ALL_AGGREGATORS)
    _eq(full, r["fwd"]["agg"], f"{name} all six")
    for sub in (("sum", "mean", "min", "max"), ("sum", "mean", "var", "std"), ("min", "max"), ("var", "std"), ("max", "mean")):
        got = egc_amd.pna_aggregate(P, Q, ei, sub)
        for k, a in enumerate(sub):
            at = ALL_AGGREGATORS.index(a)
            assert torch.equal(got[:, k * w:(k + 1) * w], full[:, at * w:(at + 1) * w]), (sub, a)


@pytest.mark.parametrize("name", CASES)
def test_combine_kernels_have_the_bits_of_the_restatement(name):
    g = fixture(name)
    m = g["meta"]
    n, d, s = m["n"], m["out_channels"], len(m["scalers"])
    rng = np.random.default_rng(m["seed"] + 60)
    Y, base, gout = (rng.standard_normal(shape).astype(np.float32) for shape in ((n, s * d), (n, d), (n, d)))
    indeg = np.bincount(g["ei"][1], minlength=n)
    ei = _dev(g["ei"])
    Yd, bd = _dev(Y).requires_grad_(True), _dev(base).requires_grad_(True)
    out = egc_amd.pna_scale_combine(Yd, bd, ei, m["scalers"], m["avg_lin"], m["avg_log"])
    _eq(out.detach(), scale_combine(Y, base, indeg, m["scalers"], m["avg_lin"], m["avg_log"]), f"{name} combine")
    want = scale_combine_backward(gout, indeg, m["scalers"], m["avg_lin"], m["avg_log"])
    _eq(pna_scale_combine_backward(_dev(gout), ei, m["scalers"], m["avg_lin"], m["avg_log"]), want, f"{name} combine backward")
    out.backward(_dev(gout))
    _eq(Yd.grad, want, f"{name} d Y through autograd")
    _eq(bd.grad, gout, f"{name} d base")


def test_ties_go_to_the_first_edge():
    """Integer-valued P: the args are the first edge of the edge list attaining the extremum, found here by a plain search."""
    g, r = fixture("ties"), restated("ties")
    src, dst = g["ei"]
    _, arg_min, arg_max, _, _ = pna_aggregate_saved(_dev(r["P"]), _dev(r["Q"]), _dev(g["ei"]), r["aggregators"])
    arg_min, arg_max = arg_min.cpu().numpy(), arg_max.cpu().numpy()
    for row in range(g["meta"]["n"]):
        e = np.nonzero(dst == row)[0]
        if len(e) == 0:
            assert (arg_min[row] == -1).all() and (arg_max[row] == -1).all()
            continue
        v = r["P"][src[e]]
        assert np.array_equal(arg_max[row], e[(v == v.max(axis=0)).argmax(axis=0)])
        assert np.array_equal(arg_min[row], e[(v == v.min(axis=0)).argmax(axis=0)])


@pytest.mark.parametrize("name", ("hub", "all6", "w116"))
def test_two_training_steps_are_bit_identical(name):
    runs = []
    for _ in range(2):
        _, layer, x, out = _train_step(name)
        runs.append([out, x.grad] + [p.grad for p in layer.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_a_graph_without_edges():
    deg = torch.tensor([3, 2])
    layer = egc_amd.PNAConv(8, 8, ["mean", "max", "std"], ["identity", "amplification"], deg, towers=2, divide_input=True).to(DEV)
    x = torch.randn(5, 8, device=DEV, requires_grad=True)
    out = layer(x, torch.zeros((2, 0), dtype=torch.int64, device=DEV))
    assert out.shape == (5, 8) and bool(torch.isfinite(out).all())
    out.sum().backward()
    assert float(layer.pre_nns[0][0].weight.grad.abs().max()) == 0.0 and bool(torch.isfinite(x.grad).all())


def test_training_step_needs_no_edge_sized_array():
    """Peak memory of a training step stays below the ONE [E, W] float32 message tensor the stock layer materialises (it keeps
    that, its square's scatter and the [E, 2 F] concatenation)."""
    n, e, d = 4096, 524288, 64
    gen = torch.Generator().manual_seed(11)
    ei = torch.randint(0, n, (2, e), generator=gen).to(DEV)
    graph = egc_amd.CSRGraph.from_edge_index(ei, n)
    graph.transposed()
    layer = egc_amd.PNAConv(d, d, ["mean", "min", "max", "std"], ["identity", "amplification", "attenuation"],
                            egc_amd.degree_histogram(graph), towers=4, divide_input=True).to(DEV)
    x = torch.randn(n, d, generator=gen).to(DEV).requires_grad_(True)
    gout = torch.randn(n, d, generator=gen).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    layer(x, graph).backward(gout)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes = {rise / (n * d * 4):.1f} arrays of N W floats; one message tensor is {e * d * 4} bytes")
    assert x.grad is not None and rise < e * d * 4
