"""egc_amd.GCNConv / SAGEConv / GINConv and the kernel of egc_nbr_sum.hip on the GPU against the fixtures of the per-edge composition
of the layers' published formulas (tests/golden/make_golden_gnn.py) and against the sequential CPU restatement in the documented
order (tests/nbr_ref.py).

Bound of everything compared with a fixture (the rule of test_mpnn_gpu.py): the relative max error against the float64 fixture is
at most max(1e-5, 5 x the generator's own float32-vs-float64 distance for that quantity).  What the kernel writes -- the
neighbour sum and its gradient with respect to x, in every configuration the layers launch -- is ``torch.equal`` to the float32
restatement.  tests/test_nbr_shapes_gpu.py runs the kernel at every row length and width it dispatches on."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from nbr_ref import CASES, CHUNK, build_layer, csr_by_destination, load_gnn_golden, nbr_sum, nbr_sum_transposed, rel_grad, rel_out

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_gnn_golden(name)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _build(name):
    g = fixture(name)
    layer = build_layer(g)
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
    assert len(checks) == 1 + len(g["grad64"]) and all(got is not None for _, got, _, _ in checks)
    bad = []
    for k, got, want, dist in checks:
        bound, err = max(1e-5, 5.0 * dist), rel_grad(got.cpu().numpy(), want)
        print(f"{name} d {k}: measured {err:.3e}, generator f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
        if not err <= bound:
            bad.append(f"d {k}: error {err:.3e}, generator f32-vs-f64 {dist:.3e}, bound {bound:.3e}")
    assert not bad, f"{name}: " + "; ".join(bad)


@pytest.mark.parametrize("form", ("edge_index", "SparseTensor", "CSRGraph"))
@pytest.mark.parametrize("name", ("gcn_messy_narrow_in", "sage_mean_messy", "gin_train_eps"))
def test_graph_forms_give_the_same_bits(name, form):
    g, layer, x, ei = _build(name)
    n = x.size(0)
    graph = dict(edge_index=ei, SparseTensor=egc_amd.SparseTensor(row=ei[1], col=ei[0], sparse_sizes=(n, n)),
                 CSRGraph=egc_amd.CSRGraph.from_edge_index(ei, n))[form]
    with torch.no_grad():
        assert torch.equal(layer(x, graph), layer(x, ei))


# --------------------------------------------------------------------------------- the kernel against the float32 restatement

def _eq(got, want, what):
    want = torch.from_numpy(np.ascontiguousarray(want))
    assert torch.equal(got.cpu(), want), f"{what}: {int((got.cpu() != want).sum())} of {want.numel()} elements differ"


# (tag, form, x_self is x, skip, self_scale, eps, table): every configuration the three layers launch
CONFIGS = (("sum", "sum", False, False, 1.0, None, None), ("sum+self", "sum", True, False, 1.3, None, None),
           ("sum+eps", "sum", True, False, 1.0, 0.3, None), ("sum+self+skip", "sum", True, True, 1.0, None, None),
           ("mean", "mean", False, False, 1.0, None, None), ("mean_t", "mean_t", False, False, 1.0, None, None),
           ("sym raw", "sym", False, False, 1.0, None, "raw"), ("sym looped+self+skip", "sym", True, True, 1.0, None, "looped"))


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: c[0].replace(" ", "_"))
@pytest.mark.parametrize("name,width", (("gcn_messy_narrow_in", 13), ("gcn_hub", 8), ("gcn_hub", 6)))
def test_neighbor_sum_and_its_gradient_have_the_bits_of_the_documented_order(name, width, cfg):
    tag, form, shared, skip, self_scale, eps, table = cfg
    g = fixture(name)
    n = g["meta"]["n"]
    rowptr, col, _ = csr_by_destination(g["ei"], n)
    rng = np.random.default_rng(g["meta"]["seed"] + 70)
    x, dout = (rng.standard_normal((n, width)).astype(np.float32) for _ in range(2))
    graph = egc_amd.CSRGraph.from_edge_index(_dev(g["ei"]), n)
    scale = dict(raw=graph.dis_raw, looped=graph.dis_looped).get(table)
    edge_scale = dict(raw=graph.edge_dis_raw, looped=graph.edge_dis_looped).get(table)
    scale_np = scale[:n].cpu().numpy() if scale is not None else None
    s = np.float32(1) + np.float32(eps) if eps is not None else np.float32(self_scale)
    kw = dict(deg_rowptr=np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n))])) if form == "mean_t" else {}
    want = nbr_sum(x, rowptr, col, form, x_self=x if shared else None, s=s, skip=skip, row_scale=scale_np, src_scale=scale_np, **kw)
    want_dx = nbr_sum_transposed(dout, rowptr, col, n, form, shared_self=shared, s=s, skip=skip, scale=scale_np)
    eps_t = torch.tensor([eps], device=DEV, requires_grad=True) if eps is not None else None
    for edge in ((None, edge_scale) if form == "sym" else (None,)):          # e_p gathered, and from the per-entry table
        assert form != "sym" or edge_scale is not None
        xd = _dev(x).requires_grad_(True)
        out = egc_amd.neighbor_sum(xd, graph, form, x_self=xd if shared else None, self_scale=self_scale, eps=eps_t, skip_self_entries=skip,
                                   scale=scale, edge_scale=edge)
        _eq(out.detach(), want, f"{name} {tag} out")
        out.backward(_dev(dout))
        _eq(xd.grad, want_dx, f"{name} {tag} d x")
    if eps is not None:         # a torch reduction: compared by value
        want_eps = float((dout.astype(np.float64) * x).sum())
        assert abs(float(eps_t.grad) - want_eps) <= 1e-5 * np.abs(dout.astype(np.float64) * x).sum()
    if shared and not skip:     # a separate x_self: the same output, the self path's gradient a product of its own
        xd, sd = _dev(x).requires_grad_(True), _dev(x).requires_grad_(True)
        out = egc_amd.neighbor_sum(xd, graph, form, x_self=sd, self_scale=self_scale, eps=eps_t.detach() if eps is not None else None)
        _eq(out.detach(), want, f"{name} {tag} out, x_self apart")
        out.backward(_dev(dout))
        _eq(xd.grad, nbr_sum_transposed(dout, rowptr, col, n, form), f"{name} {tag} d x, x_self apart")
        _eq(sd.grad, dout * s, f"{name} {tag} d x_self")


def test_the_hub_has_its_long_row_in_both_directions():
    g = fixture("gcn_hub")
    n = g["meta"]["n"]
    assert np.bincount(g["ei"][1], minlength=n).max() > 2 * CHUNK + 1 and np.bincount(g["ei"][0], minlength=n).max() > 2 * CHUNK + 1


def test_out_writes_only_its_column_block():
    g = fixture("gcn_hub")
    n, d = g["meta"]["n"], 6
    x = torch.randn(n, d, device=DEV)
    graph = egc_amd.CSRGraph.from_edge_index(_dev(g["ei"]), n)
    for form, kw in (("mean", {}), ("sum", dict(x_self=x, self_scale=0.5)),
                     ("sym", dict(x_self=x, skip_self_entries=True, scale=graph.dis_looped, edge_scale=graph.edge_dis_looped))):
        want = egc_amd.neighbor_sum(x, graph, form, **kw)
        wide = torch.full((n, d + 7), 7.0, device=DEV)
        block = egc_amd.neighbor_sum(x, graph, form, out=wide, out_col=3, **kw)
        assert block.data_ptr() == wide.data_ptr() + 12 and torch.equal(block, want) and torch.equal(wide[:, 3:3 + d], want)
        assert bool((wide[:, :3] == 7.0).all()) and bool((wide[:, 3 + d:] == 7.0).all())
    with pytest.raises(RuntimeError, match="inference form"):
        egc_amd.neighbor_sum(x.clone().requires_grad_(True), graph, "mean", out=wide)
    with pytest.raises(RuntimeError, match="out must be"):
        egc_amd.neighbor_sum(x, graph, "mean", out=wide, out_col=8)


def test_combinations_no_layer_launches_raise():
    g = fixture("gcn_messy_narrow_in")
    n = g["meta"]["n"]
    x = torch.randn(n, 4, device=DEV)
    graph = egc_amd.CSRGraph.from_edge_index(_dev(g["ei"]), n)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        egc_amd.neighbor_sum(x, graph, "mean", x_self=x)
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        egc_amd.neighbor_sum(x, graph, "sum", skip_self_entries=True)
    with pytest.raises(RuntimeError, match="scale"):
        egc_amd.neighbor_sum(x, graph, "sym")
    with pytest.raises(RuntimeError, match="x_self"):
        egc_amd.neighbor_sum(x, graph, "sum", eps=torch.zeros(1, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- the layers

@pytest.mark.parametrize("name", ("gcn_hub", "gcn_messy_narrow_in", "sage_mean_hub", "sage_no_root", "gin_hub", "gin_train_eps"))
def test_two_training_steps_are_bit_identical(name):
    runs = []
    for _ in range(2):
        _, layer, x, out = _train_step(name)
        runs.append([out, x.grad] + [p.grad for p in layer.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", ("gin_buffer_eps", "gin_train_eps"))
def test_filling_eps_in_place_changes_the_next_output(name):
    """The kernel reads eps on the device: nothing of it is kept on the host between calls."""
    g, layer, x, ei = _build(name)
    graph = egc_amd.CSRGraph.from_edge_index(ei, x.size(0))
    with torch.no_grad():
        first = layer(x, graph)
        want_first = layer.nn(egc_amd.neighbor_sum(x, graph, "sum", x_self=x, self_scale=float(np.float32(1) + g["params"]["eps"][0])))
        layer.eps.fill_(0.5)
        second = layer(x, graph)
        want_second = layer.nn(egc_amd.neighbor_sum(x, graph, "sum", x_self=x, self_scale=1.5))
    assert torch.equal(first, want_first) and torch.equal(second, want_second) and not torch.equal(first, second)


def test_a_captured_gin_forward_follows_eps():
    """GINConv(train_eps=True) inside a captured graph: the replay sees the value eps holds then."""
    g, layer, x, ei = _build("gin_train_eps")
    graph = egc_amd.CSRGraph.from_edge_index(ei, x.size(0))
    with torch.no_grad():
        layer(x, graph)                      # one eager call first
        torch.cuda.synchronize()
        cg = torch.cuda.CUDAGraph()
        with torch.cuda.graph(cg):
            out = layer(x, graph)
        for value in (0.3, -0.25):
            layer.eps.fill_(value)
            cg.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, layer.nn(egc_amd.neighbor_sum(x, graph, "sum", x_self=x, self_scale=float(np.float32(1) + np.float32(value)))))


def test_a_graph_without_edges():
    ei = torch.zeros((2, 0), dtype=torch.int64, device=DEV)
    x = torch.randn(5, 8, device=DEV, requires_grad=True)
    for layer in (egc_amd.GCNConv(8, 4), egc_amd.GCNConv(8, 12, normalize=False), egc_amd.SAGEConv(8, 4),
                  egc_amd.GINConv(torch.nn.Linear(8, 4), train_eps=True)):
        layer = layer.to(DEV)
        out = layer(x, ei)
        assert out.shape[0] == 5 and bool(torch.isfinite(out).all())
        out.sum().backward()
        assert bool(torch.isfinite(x.grad).all())
    gcn = egc_amd.GCNConv(8, 8).to(DEV)                    # every node keeps its self loop: out = x W^T + b
    assert torch.allclose(gcn(x, ei), gcn.lin(x) + gcn.bias, atol=1e-6)
