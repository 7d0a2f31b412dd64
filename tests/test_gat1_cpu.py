"""GATConv (GAT v1) without a GPU: the fixtures (tests/golden/gat1) and the properties their cases are named for, the float64
restatement of the kernel's formulation (tests/gat1_ref.py: chunked online softmax with the self entry last, the backward
sums with recomputed scores, the destination pass's factored) against them, and the host side of egc_amd.GATConv (parameter names and shapes, the
lin_dst is lin_src aliasing, the single-lin.weight layout, initial values, dropout, argument errors, the C table)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from egc_amd._gat import gat_aggregate
from gat1_ref import (CASES, CHUNK, SHAPES, aggregate_backward, aggregate_forward, layer_forward, layer_kwargs, load, per_edge_backward,
                      rel_grad, rel_out, workspace_bytes)


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load(name)


def test_every_case_of_the_table_is_there():
    assert _C.load().egc_typed_mean_chunk() == CHUNK
    assert set(CASES) == {"messy", "hub", "w152h8", "w152h1", "w240h8", "w304h1", "mean", "noloops", "bigscore", "slope", "nobias"}
    for name in CASES:
        g = fixture(name)
        m = g["meta"]
        assert m["name"] == name and m["chunk"] == CHUNK and (m["heads"], m["channels"]) == SHAPES[name] and m["in_channels"] <= 16
        width = m["channels"] if m["kwargs"].get("concat") is False else m["heads"] * m["channels"]
        assert g["x"].shape == (m["n"], m["in_channels"]) and g["out64"].shape == (m["n"], width) == g["gout"].shape == g["out32"].shape
        assert g["out64"].dtype == np.float64 and g["grad_x64"].dtype == np.float64 and g["out32"].dtype == np.float32
        want = {"lin_src.weight", "att_src", "att_dst"} | (set() if name == "nobias" else {"bias"})
        assert set(g["grad64"]) == want == set(m["f32_vs_f64_grad"])
        assert set(g["params"]) == want | {"lin_dst.weight"}
        assert np.array_equal(g["params"]["lin_src.weight"], g["params"]["lin_dst.weight"])


def test_cases_have_the_properties_they_are_named_for():
    for name in ("messy", "noloops"):
        g = fixture(name)
        ei, n = g["ei"], g["meta"]["n"]
        pairs = ei[0] * n + ei[1]
        assert n == 57 and int((ei[0] == ei[1]).sum()) >= 9 and len(pairs) - len(np.unique(pairs)) >= 20 and ei.max() < n - 3
        assert g["meta"]["channels"] % 4 != 0
    assert np.array_equal(fixture("messy")["ei"], fixture("noloops")["ei"])
    g = fixture("noloops")
    assert g["meta"]["kwargs"] == dict(add_self_loops=False)
    empty = np.bincount(g["ei"][1], minlength=57) == 0
    assert empty.sum() >= 3 and np.array_equal(g["out64"][empty], np.broadcast_to(g["params"]["bias"].astype(np.float64), (empty.sum(), 20)))
    g = fixture("hub")
    n = g["meta"]["n"]
    assert np.bincount(g["ei"][1], minlength=n).max() > 2 * CHUNK + 18 and np.bincount(g["ei"][0], minlength=n).max() > 2 * CHUNK + 18
    assert fixture("mean")["meta"]["kwargs"] == dict(concat=False) and fixture("mean")["out64"].shape[1] == 6 and (3 * 6) % 4 != 0
    assert fixture("slope")["meta"]["kwargs"] == dict(negative_slope=0.05)
    assert fixture("nobias")["meta"]["kwargs"] == dict(bias=False)
    g = fixture("w304h1")
    assert g["meta"]["n"] == 24 and g["meta"]["heads"] * g["meta"]["channels"] > 256


def test_bigscore_scores_span_80_within_a_row():
    g = fixture("bigscore")
    p = {k: v.astype(np.float64) for k, v in g["params"].items()}
    x, (src, dst) = g["x"].astype(np.float64), g["ei"]
    xl = (x @ p["lin_src.weight"].T).reshape(-1, 2, 8)
    a_src, a_dst = (xl * p["att_src"]).sum(-1), (xl * p["att_dst"]).sum(-1)
    keep = src != dst
    src, dst = np.concatenate([src[keep], np.arange(len(x))]), np.concatenate([dst[keep], np.arange(len(x))])
    z = a_src[src] + a_dst[dst]
    s = np.where(z > 0, z, 0.2 * z)
    assert max(min(s[dst == i, h].max(), -s[dst == i, h].min()) for i in range(len(x)) for h in range(2)) >= 80.0
    assert g["meta"]["score_span"] >= 80.0


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    """The kernel's formulation (the destination pass's factored sums included) differs from the per-edge composition by float64 rounding
    only: 1e-10 relative on the output and on every gradient."""
    g = fixture(name)
    m = g["meta"]
    params = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in g["params"].items() if k != "lin_dst.weight"}
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    out = layer_forward(x, g["ei"], params, m["heads"], m["channels"], **m["kwargs"])
    out.backward(torch.from_numpy(g["gout"]).double())
    assert rel_out(out.detach().numpy(), g["out64"]) <= 1e-10
    assert rel_grad(x.grad.numpy(), g["grad_x64"]) <= 1e-10
    assert set(params) == set(g["grad64"])
    for k, p in params.items():
        assert rel_grad(p.grad.numpy(), g["grad64"][k]) <= 1e-10, k


def test_restatement_does_not_depend_on_the_chunk_or_batch_size_beyond_rounding():
    g = fixture("hub")
    rng = np.random.default_rng(3)
    xl, a_src, a_dst, gout = rng.standard_normal((700, 8)), rng.standard_normal((700, 2)), rng.standard_normal((700, 2)), rng.standard_normal((700, 8))
    a, la = aggregate_forward(xl, a_src, a_dst, g["ei"], chunk=CHUNK, ahead=8)
    b, lb = aggregate_forward(xl, a_src, a_dst, g["ei"], chunk=10 ** 9, ahead=1)
    assert rel_out(a, b) <= 1e-12 and rel_out(la, lb) <= 1e-12
    ga = aggregate_backward(xl, a_src, a_dst, g["ei"], a, la, gout, chunk=CHUNK)
    gb = aggregate_backward(xl, a_src, a_dst, g["ei"], a, la, gout, chunk=10 ** 9)
    gc = per_edge_backward(xl, a_src, a_dst, g["ei"], a, la, gout)
    for p, q, r in zip(ga, gb, gc):
        assert rel_grad(p, q) <= 1e-12 and rel_grad(p, r) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_and_shapes(name):
    g = fixture(name)
    m = g["meta"]
    layer = egc_amd.GATConv(**layer_kwargs(g))
    h, c, fin = m["heads"], m["channels"], m["in_channels"]
    want = {"lin_src.weight": (h * c, fin), "lin_dst.weight": (h * c, fin), "att_src": (1, h, c), "att_dst": (1, h, c)}
    if name != "nobias":
        want["bias"] = (c,) if m["kwargs"].get("concat") is False else (h * c,)
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == want
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, torch.from_numpy(g["params"][k])), k
    assert name == "nobias" or float(layer.bias.detach().abs().max()) > 0


def test_lin_dst_is_lin_src_and_the_single_lin_layout_loads():
    layer = egc_amd.GATConv(6, 4, heads=2)
    assert layer.lin_dst is layer.lin_src and layer.lin_src.bias is None
    assert [k for k, _ in layer.named_parameters()] == ["att_src", "att_dst", "bias", "lin_src.weight"]
    state = {k: torch.randn_like(v) for k, v in layer.state_dict().items() if not k.startswith("lin_")}
    state["lin.weight"] = torch.randn(8, 6)
    layer.load_state_dict(state, strict=True)
    assert torch.equal(layer.lin_src.weight, state["lin.weight"]) and torch.equal(layer.att_dst, state["att_dst"])
    assert set(state) == {"att_src", "att_dst", "bias", "lin.weight"}                 # the caller's dict is left as it was
    # inside a parent module, under a prefix
    net = torch.nn.Sequential(torch.nn.Identity(), egc_amd.GATConv(6, 4, heads=2))
    net.load_state_dict({"1." + k: v for k, v in state.items()}, strict=True)
    assert torch.equal(net[1].lin_dst.weight, state["lin.weight"])
    with pytest.raises(RuntimeError, match="lin_src.weight"):                          # neither layout: still an error
        layer.load_state_dict({k: v for k, v in state.items() if k != "lin.weight"}, strict=True)
    with pytest.raises(RuntimeError, match="Unexpected"):
        layer.load_state_dict(dict(layer.state_dict(), **{"lin.weight": state["lin.weight"]}), strict=True)


def test_extended_weight_folds_the_att_vectors():
    torch.manual_seed(1)
    for h, c, ext in ((8, 19, 168), (1, 152, 156), (3, 6, 24), (2, 5, 16)):
        layer = egc_amd.GATConv(7, c, heads=h).double()
        x = torch.randn(9, 7, dtype=torch.float64)
        with torch.no_grad():
            e = x @ layer.extended_weight().t()
            xl = layer.lin_src(x)
        assert e.shape == (9, ext) and ext % 4 == 0 and torch.equal(e[:, :h * c], xl)
        for att, lo in ((layer.att_src, h * c), (layer.att_dst, h * c + h)):
            assert torch.allclose(e[:, lo:lo + h], (xl.view(9, h, c) * att).sum(-1), rtol=1e-12, atol=1e-12)
        assert float(e[:, h * c + 2 * h:].detach().abs().sum()) == 0.0


def test_initial_values_and_options():
    torch.manual_seed(0)
    layer = egc_amd.GATConv(16, 19, heads=8)
    assert float(layer.bias.abs().max()) == 0.0
    assert float(layer.lin_src.weight.abs().max()) <= (6.0 / (152 + 16)) ** 0.5
    for att in (layer.att_src, layer.att_dst):
        assert float(att.abs().max()) <= (6.0 / (8 + 19)) ** 0.5 and float(att.std()) > 0
    assert not torch.equal(layer.att_src, layer.att_dst)
    assert egc_amd.GATConv(4, 4, bias=False).bias is None and "bias" not in egc_amd.GATConv(4, 4, bias=False).state_dict()
    assert egc_amd.GATConv(4, 4, heads=3, concat=False).bias.shape == (4,)
    with pytest.raises(ValueError, match="1..512"):
        egc_amd.GATConv(4, 65, heads=8)
    with pytest.raises(ValueError, match="bipartite"):
        egc_amd.GATConv((4, 4), 8)
    with pytest.raises(TypeError):
        egc_amd.GATConv(4, 8, edge_dim=3)


def test_dropout_raises_in_training_and_is_ignored_in_eval():
    layer = egc_amd.GATConv(6, 4, heads=2, dropout=0.5)
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        layer(torch.randn(5, 6), ei)
    layer.eval()
    with pytest.raises(RuntimeError) as info:                              # past the dropout check: a CPU tensor, no CPU fallback
        layer(torch.randn(5, 6), ei)
    assert not isinstance(info.value, NotImplementedError)


def test_bad_shapes_raise():
    layer = egc_amd.GATConv(6, 4, heads=2)
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="expected \\(rows, 6\\)"):
        layer(torch.randn(5, 7), ei)
    with pytest.raises(RuntimeError, match="expected \\(rows, 6\\)"):
        layer(torch.randn(6), ei)
    with pytest.raises(RuntimeError):
        layer(torch.randn(5, 6).double(), ei)
    with pytest.raises(RuntimeError, match="two-dimensional"):
        gat_aggregate(torch.randn(5, 8), torch.randn(10), torch.randn(5, 2), ei)


def test_c_entries_are_in_the_table_and_reject_bad_arguments_without_device_work():
    lib = _C.load()
    for sym in ("egc_gat_forward_f32", "egc_gat_forward_workspace_bytes", "egc_gat_backward_f32", "egc_gat_backward_workspace_bytes"):
        assert sym in _C.SYMBOLS and getattr(lib, sym) is not None
    INVALID = 1
    assert lib.egc_gat_forward_workspace_bytes(CHUNK, 8, 19) == 0              # no row can be longer than a chunk
    assert lib.egc_gat_forward_workspace_bytes(1000, 8, 19) == 4 * 64 * 3 * 16     # 4 slots, 38 lanes padded to 64, (m, l, acc)
    assert lib.egc_gat_forward_workspace_bytes(1000, 1, 304) == 4 * 128 * 3 * 16   # two 64-lane slots per row
    assert lib.egc_gat_backward_workspace_bytes(10, 0, 2, 4) == 4 * 20             # D alone
    assert lib.egc_gat_backward_workspace_bytes(10, 1000, 8, 19) == workspace_bytes(8, 19, 10, 1000)[1] == 4 * 80 + 4 * 64 * 64
    for h, c in ((0, 4), (2, 0), (8, 65)):
        assert lib.egc_gat_forward_workspace_bytes(1000, h, c) == 0 == lib.egc_gat_backward_workspace_bytes(10, 1000, h, c)

    def fwd(n_rows=4, n_edges=0, n_src=4, ld_xl=8, ld_as=2, ld_ad=2, h=2, c=4, loops=1, ld_out=8):
        return lib.egc_gat_forward_f32(None, None, n_rows, n_edges, n_src, None, ld_xl, None, ld_as, None, ld_ad, h, c, 0.2, loops, None,
                                       ld_out, None, None, 0, None)

    def bwd(n_rows=4, n_edges=0, ld_xl=8, ld_as=2, ld_ad=2, h=2, c=4, ld_out=8, ld_g=8, ld_dxl=8, ld_das=2, ld_dad=2):
        return lib.egc_gat_backward_f32(None, None, None, None, n_rows, n_edges, None, ld_xl, None, ld_as, None, ld_ad, h, c, 0.2, 1,
                                        None, ld_out, None, None, ld_g, None, ld_dxl, None, ld_das, None, ld_dad, None, 0, None)

    assert fwd() == INVALID                                                   # rows to do and no pointers
    assert fwd(n_rows=0, n_src=0) == 0                                        # nothing to do
    for h, c in ((0, 4), (2, 0), (8, 65)):                                    # H < 1, C < 1, H C > 512
        assert fwd(n_rows=0, n_src=0, h=h, c=c, ld_xl=600, ld_out=600, ld_as=600, ld_ad=600) == INVALID
        assert bwd(n_rows=0, h=h, c=c, ld_xl=600, ld_out=600, ld_g=600, ld_as=600, ld_ad=600) == INVALID
    for kw in (dict(n_rows=-1), dict(n_edges=-1), dict(n_src=-1), dict(ld_xl=7), dict(ld_out=7), dict(ld_as=1), dict(ld_ad=1)):
        assert fwd(**dict(dict(n_rows=0, n_src=0), **kw)) == INVALID, kw      # a negative count, a stride below its width
    assert fwd(n_rows=0, n_src=5) == INVALID                                  # self loops on a non-square graph
    assert fwd(n_rows=0, n_src=5, loops=0) == 0
    assert bwd() == 0                                                         # no gradient wanted: nothing to do
    for kw in (dict(n_rows=-1), dict(n_edges=-1), dict(ld_xl=7), dict(ld_out=7), dict(ld_g=7), dict(ld_as=1), dict(ld_ad=1)):
        assert bwd(**kw) == INVALID, kw
    # a gradient wanted (a pointer that is never followed: the inputs are missing)
    one = torch.zeros(64)
    assert lib.egc_gat_backward_f32(None, None, None, None, 4, 0, None, 8, None, 2, None, 2, 2, 4, 0.2, 1, None, 8, None, None, 8,
                                    one.data_ptr(), 8, None, 0, None, 0, None, 0, None) == INVALID
    assert lib.egc_gat_backward_f32(None, None, None, None, 4, 0, None, 8, None, 2, None, 2, 2, 4, 0.2, 1, None, 8, None, None, 8,
                                    one.data_ptr(), 7, None, 0, None, 0, None, 0, None) == INVALID     # d xl's stride below H C
    assert lib.egc_gat_backward_f32(None, None, None, None, 4, 0, None, 8, None, 2, None, 2, 2, 4, 0.2, 1, None, 8, None, None, 8,
                                    None, 0, one.data_ptr(), 1, None, 0, None, 0, None) == INVALID     # d a_src's stride below H
