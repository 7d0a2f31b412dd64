"""egc_amd.RGCNConv / egc_amd.REGC on the gfx950 typed-mean kernel (egc_typed_mean_f32) against the fixtures of the reference's
own RGCNConv / REGC.forward and against the sequential CPU restatement in the documented summation order (tests/rgcn_ref.py).

Bound of everything compared with a reference-derived fixture: the relative max error against the float64 fixture is at most
max(1e-5, 5 x the reference's own float32-vs-float64 distance on that fixture) -- for outputs the distance between the two
outputs stored in the fixture, for a gradient the distance the generator recorded for that gradient.
tests/test_typed_mean_shapes_gpu.py runs the kernel, in both of its forms, at every row length and width it dispatches on."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._typed import TypedMeanPlan, TypedRel, typed_mean, typed_mean_cat, typed_mean_chunk
from rgcn_ref import (LAYER_FIXTURES, NET_FIXTURES, load_rgcn_golden, reference_distance, rel_grad, rel_out, typed_operands)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_rgcn_golden(name)


def _adj(g, sizes):
    return {key: egc_amd.SparseTensor(row=torch.from_numpy(ei[1]).to(DEV), col=torch.from_numpy(ei[0]).to(DEV),
                                      sparse_sizes=(sizes[key[2]], sizes[key[0]])) for key, ei in g["ei"].items()}


def _build(name):
    g = fixture(name)
    m = g["meta"]
    if name in NET_FIXTURES:
        mod = egc_amd.REGC(m["hidden"], m["num_layers"], m["dropout"], use_egc=m["use_egc"], egc_heads=m["heads"],
                           egc_bases=m["bases"], num_nodes_dict=m["sizes"], in_features=m["in_features"],
                           num_classes=m["num_classes"])
    else:
        mod = egc_amd.RGCNConv(m["fin"], m["fout"])
    mod.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    mod = mod.to(DEV).eval()
    sizes = {k: v.shape[0] for k, v in g["out32"].items()}
    x = {k: torch.from_numpy(v).to(DEV) for k, v in g["x"].items()}
    return g, mod, x, _adj(g, sizes)


@pytest.mark.parametrize("name", LAYER_FIXTURES + NET_FIXTURES)
def test_forward_matches_reference_fixture(name):
    g, mod, x, adj = _build(name)
    dist = reference_distance(g)
    bound = max(1e-5, 5.0 * dist)
    with torch.no_grad():
        out = mod(x, adj)
    out_grad = mod(x, adj)
    assert any(v.requires_grad for v in out_grad.values())
    for k in g["meta"]["node_types"]:
        for what, o in (("no_grad", out[k]), ("grad", out_grad[k].detach())):
            err = rel_out(o.cpu().numpy(), g["out64"][k])
            assert err <= bound, f"{name} {k} {what}: error {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}"
    worst = max(rel_out(out[k].cpu().numpy(), g["out64"][k]) for k in out)
    print(f"{name}: reference f32-vs-f64 {dist:.3e}, measured {worst:.3e}, bound {bound:.3e}")


@pytest.mark.parametrize("name", LAYER_FIXTURES + NET_FIXTURES)
def test_gradients_match_float64_fixture(name):
    g, mod, x, adj = _build(name)
    m = g["meta"]
    x = {k: v.clone().requires_grad_(True) for k, v in x.items()}
    out = mod(x, adj)
    sum((out[k] * torch.from_numpy(g["gout"][k]).to(DEV)).sum() for k in out).backward()
    for k, v in x.items():
        dist = m["f32_vs_f64_grad_x"][k]
        bound, err = max(1e-5, 5.0 * dist), rel_grad(v.grad.cpu().numpy(), g["grad_x64"][k])
        assert err <= bound, f"{name} d x[{k}]: error {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}"
    seen = 0
    for k, p in mod.named_parameters():
        if k not in g["grad64"]:          # the relation left out of adj_t_dict: no gradient in the reference either
            assert p.grad is None, k
            continue
        dist = m["f32_vs_f64_grad"][k]
        bound, err = max(1e-5, 5.0 * dist), rel_grad(p.grad.cpu().numpy(), g["grad64"][k])
        assert err <= bound, f"{name} d {k}: error {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}"
        seen += 1
    assert seen == len(g["grad64"])
    if name in NET_FIXTURES:
        assert all(f"embs.{k}" in g["grad64"] for k in mod.embs)


def _plan(g, x, adj):
    types = list(x)
    rels = {t: [] for t in types}
    for k in (tuple(k) for k in g["meta"]["edge_types"]):
        if k in adj:
            rels[k[2]].append((k[0], adj[k].graph))
    return TypedMeanPlan(types, rels)


@pytest.mark.parametrize("name", LAYER_FIXTURES)
def test_operand_has_the_bits_of_the_documented_order(name):
    """A_t = [x_t | mean_1 | ...] against the sequential float32 loop in chunked order, long row included."""
    g, _, x, adj = _build(name)
    chunk = typed_mean_chunk()
    assert chunk == g["meta"]["chunk"]
    want, blocks = typed_operands(g["x"], g["ei"], g["meta"]["edge_types"], chunk, np.float32)
    got = typed_mean_cat(_plan(g, x, adj), list(x.values()))
    deg = np.bincount(g["ei"][("paper", "cites", "paper")][1])
    assert deg.max() > 2 * chunk + 1
    for t, a in zip(x, got):
        assert a.shape == want[t].shape and len(blocks[t]) + 1 == a.size(1) // x[t].size(1)
        assert torch.equal(a.cpu(), torch.from_numpy(want[t])), t


@pytest.mark.parametrize("name", LAYER_FIXTURES)
def test_a_launch_over_all_relations_equals_one_launch_per_relation(name):
    g, _, x, adj = _build(name)
    plan = _plan(g, x, adj)
    got = typed_mean_cat(plan, list(x.values()))
    width = g["meta"]["fin"]
    for t, a in zip(plan.types, got):
        assert torch.equal(a[:, :width], x[t])
        for j, (src, graph) in enumerate(plan.rels[t]):
            one = torch.full((x[t].size(0), width), float("nan"), device=DEV)
            typed_mean([TypedRel(graph, x[src], post_mean=True)], x[t].size(0), width, one)
            assert torch.equal(one, a[:, (1 + j) * width:(2 + j) * width]), (t, j)


@pytest.mark.parametrize("name", ("rgcn_odd", "rgcn_mag_shape", "regc_rgcn"))
def test_two_runs_are_bit_identical(name):
    runs = []
    for _ in range(2):
        g, mod, x, adj = _build(name)
        x = {k: v.clone().requires_grad_(True) for k, v in x.items()}
        out = mod(x, adj)
        sum((out[k] * torch.from_numpy(g["gout"][k]).to(DEV)).sum() for k in out).backward()
        runs.append([out[k].detach() for k in out] + [v.grad for v in x.values()]
                    + [p.grad for p in mod.parameters() if p.grad is not None])
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_zero_row_type_and_zero_edge_relation():
    gen = torch.Generator().manual_seed(3)
    conv = egc_amd.RGCNConv(12, 6).to(DEV)
    sizes = dict(author=9, field_of_study=0, institution=4, paper=7)
    x = {k: torch.randn(n, 12, generator=gen).to(DEV).requires_grad_(True) for k, n in sizes.items()}
    ei = {("author", "writes", "paper"): torch.stack([torch.randint(0, 9, (20,), generator=gen), torch.randint(0, 7, (20,), generator=gen)]),
          ("author", "affiliated_with", "institution"): torch.zeros((2, 0), dtype=torch.int64),     # a relation without edges
          ("paper", "has_topic", "field_of_study"): torch.zeros((2, 0), dtype=torch.int64),         # into the type without rows
          ("field_of_study", "to", "paper"): torch.zeros((2, 0), dtype=torch.int64)}                # out of it
    adj = {k: egc_amd.SparseTensor(row=e[1].to(DEV), col=e[0].to(DEV), sparse_sizes=(sizes[k[2]], sizes[k[0]])) for k, e in ei.items()}
    out = conv(x, adj)
    assert out["field_of_study"].shape == (0, 6)
    lin = conv.root_lins["institution"]
    assert torch.allclose(out["institution"], x["institution"] @ lin.weight.t() + lin.bias, atol=1e-5)   # the means are zeros
    sum(o.sum() for o in out.values()).backward()
    assert x["field_of_study"].grad.shape == (0, 12)
    want = conv.root_lins["institution"].weight.sum(0).expand(4, 12)
    assert torch.allclose(x["institution"].grad, want, atol=1e-5)
    assert float(conv.rel_lins["author_affiliated_with_institution"].weight.grad.abs().max()) == 0.0
    # d x[author]: its own root term and the writes relation; against float64 on the host
    xa, xp = x["author"].detach().cpu().double(), x["paper"].detach().cpu().double()
    src, dst = ei[("author", "writes", "paper")]
    deg = torch.bincount(dst, minlength=7).clamp(min=1).double()
    w = conv.rel_lins["author_writes_paper"].weight.detach().cpu().double()
    d_mean = torch.ones(7, 6, dtype=torch.float64) @ w
    want = conv.root_lins["author"].weight.detach().cpu().double().sum(0).expand(9, 12).clone()
    want.index_add_(0, src, d_mean[dst] / deg[dst, None])
    assert float((x["author"].grad.cpu().double() - want).abs().max()) <= 1e-5


@pytest.mark.parametrize("name", ("rgcn_small", "regc_egc"))
def test_state_dict_round_trip_on_the_device(name):
    g, mod, _, _ = _build(name)
    state = mod.state_dict()
    assert set(state) == set(g["params"])
    for k, v in state.items():
        assert torch.equal(v.cpu(), torch.from_numpy(g["params"][k])), k
    other = _build(name)[1]
    with torch.no_grad():
        for p in other.parameters():
            p.zero_()
    other.load_state_dict(state, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, state[k]), k


@pytest.mark.parametrize("name", NET_FIXTURES)
def test_regc_training_dropout_is_seeded_and_eval_is_the_fixture(name):
    g, net, x, adj = _build(name)
    net.train()
    steps = []
    for _ in range(2):
        torch.manual_seed(17)
        net.zero_grad(set_to_none=True)
        out = net(x, adj)
        sum((out[k] * torch.from_numpy(g["gout"][k]).to(DEV)).sum() for k in out).backward()
        steps.append([out[k].detach() for k in out] + [p.grad.clone() for p in net.parameters() if p.grad is not None])
    for a, b in zip(*steps):
        assert torch.equal(a, b)
    net.eval()
    with torch.no_grad():
        out_eval = net(x, adj)
    dist = reference_distance(g)
    bound = max(1e-5, 5.0 * dist)
    differs = False
    for i, k in enumerate(out_eval):
        err = rel_out(out_eval[k].cpu().numpy(), g["out64"][k])
        assert err <= bound, f"{name} {k}: error {err:.3e}, reference f32-vs-f64 {dist:.3e}, bound {bound:.3e}"
        differs = differs or not torch.equal(out_eval[k], steps[0][i])
    assert differs            # dropout 0.5 was active in training mode
