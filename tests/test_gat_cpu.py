"""GATv2Conv without a GPU: the fixtures (tests/golden/gat) and the properties their cases are named for, the float64 restatement
of the kernel's formulation (tests/gat_ref.py: chunked online softmax with the self entry last, the D = g . out backward with
recomputed scores) against them, and the host side of egc_amd.GATv2Conv (parameter names and shapes, weight sharing, dropout,
argument errors, the C table)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from gat_ref import CASES, CHUNK, SHAPES, aggregate_forward, layer_forward, layer_kwargs, load_gat_golden, rel_grad, rel_out


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_gat_golden(name)


def test_every_case_of_the_table_is_there():
    assert _C.load().egc_typed_mean_chunk() == CHUNK
    for name in CASES:
        g = fixture(name)
        m = g["meta"]
        assert m["name"] == name and m["chunk"] == CHUNK and (m["heads"], m["channels"]) == SHAPES[name]
        width = m["channels"] if m["kwargs"].get("concat") is False else m["heads"] * m["channels"]
        assert g["x"].shape == (m["n"], m["in_channels"]) and g["out64"].shape == (m["n"], width) == g["gout"].shape
        assert g["out64"].dtype == np.float64 and g["grad_x64"].dtype == np.float64
        want = {"lin_l.weight", "lin_l.bias", "att", "bias"} | (set() if name == "shared" else {"lin_r.weight", "lin_r.bias"})
        assert set(g["grad64"]) == want == set(m["f32_vs_f64_grad"])
        assert set(g["params"]) == {"lin_l.weight", "lin_l.bias", "lin_r.weight", "lin_r.bias", "att", "bias"}


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
    assert fixture("mean")["meta"]["kwargs"] == dict(concat=False) and fixture("mean")["out64"].shape[1] == 6
    g = fixture("shared")
    assert g["meta"]["kwargs"] == dict(share_weights=True) and np.array_equal(g["params"]["lin_l.weight"], g["params"]["lin_r.weight"])
    assert fixture("slope")["meta"]["kwargs"] == dict(negative_slope=0.05)
    assert np.array_equal(fixture("w112h8")["ei"], fixture("h8c13")["ei"])


def test_bigscore_scores_span_80_within_a_row():
    g = fixture("bigscore")
    p = {k: v.astype(np.float64) for k, v in g["params"].items()}
    x, (src, dst) = g["x"].astype(np.float64), g["ei"]
    xl, xr = x @ p["lin_l.weight"].T + p["lin_l.bias"], x @ p["lin_r.weight"].T + p["lin_r.bias"]
    keep = src != dst
    src, dst = np.concatenate([src[keep], np.arange(len(x))]), np.concatenate([dst[keep], np.arange(len(x))])
    z = (xl[src] + xr[dst]).reshape(-1, 2, 8)
    s = (p["att"] * np.where(z > 0, z, 0.2 * z)).sum(axis=-1)
    assert max(min(s[dst == i, h].max(), -s[dst == i, h].min()) for i in range(len(x)) for h in range(2)) >= 80.0
    assert g["meta"]["score_span"] >= 80.0


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_fixture(name):
    """The kernel's formulation differs from the per-edge composition by float64 rounding only: 1e-10 relative on the output and
    on every gradient."""
    g = fixture(name)
    m = g["meta"]
    keys = [k for k in g["params"] if not (name == "shared" and k.startswith("lin_r"))]
    params = {k: torch.from_numpy(g["params"][k]).double().requires_grad_(True) for k in keys}
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
    xl, xr, att = rng.standard_normal((700, 8)), rng.standard_normal((700, 8)), rng.standard_normal((2, 4))
    a, la = aggregate_forward(xl, xr, att, g["ei"], chunk=CHUNK, ahead=8)
    b, lb = aggregate_forward(xl, xr, att, g["ei"], chunk=10 ** 9, ahead=1)
    assert rel_out(a, b) <= 1e-12 and rel_out(la, lb) <= 1e-12


@pytest.mark.parametrize("name", CASES)
def test_state_dict_keys_and_shapes(name):
    g = fixture(name)
    m = g["meta"]
    layer = egc_amd.GATv2Conv(**layer_kwargs(g))
    h, c, fin = m["heads"], m["channels"], m["in_channels"]
    want = {"lin_l.weight": (h * c, fin), "lin_l.bias": (h * c,), "lin_r.weight": (h * c, fin), "lin_r.bias": (h * c,),
            "att": (1, h, c), "bias": (c,) if m["kwargs"].get("concat") is False else (h * c,)}
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == want
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, torch.from_numpy(g["params"][k])), k
    assert float(layer.bias.detach().abs().max()) > 0


def test_initial_values_and_options():
    torch.manual_seed(0)
    layer = egc_amd.GATv2Conv(16, 13, heads=8)
    assert float(layer.bias.abs().max()) == 0.0 and float(layer.lin_l.bias.abs().max()) == 0.0 == float(layer.lin_r.bias.abs().max())
    assert float(layer.lin_l.weight.abs().max()) <= (6.0 / (104 + 16)) ** 0.5 and float(layer.att.abs().max()) <= (6.0 / (8 + 13)) ** 0.5
    assert float(layer.att.std()) > 0 and not torch.equal(layer.lin_l.weight, layer.lin_r.weight)
    assert egc_amd.GATv2Conv(4, 4, bias=False).bias is None
    assert "bias" not in egc_amd.GATv2Conv(4, 4, bias=False).state_dict()
    with pytest.raises(ValueError, match="1..512"):
        egc_amd.GATv2Conv(4, 65, heads=8)


def test_share_weights_ties_the_two_linears():
    layer = egc_amd.GATv2Conv(6, 4, heads=2, share_weights=True)
    assert layer.lin_r is layer.lin_l
    assert [k for k, _ in layer.named_parameters()] == ["att", "bias", "lin_l.weight", "lin_l.bias"]
    assert egc_amd.GATv2Conv(6, 4, heads=2).lin_r is not egc_amd.GATv2Conv(6, 4, heads=2).lin_l


def test_dropout_raises_in_training_and_is_ignored_in_eval():
    layer = egc_amd.GATv2Conv(6, 4, heads=2, dropout=0.5)
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(NotImplementedError, match="attention dropout"):
        layer(torch.randn(5, 6), ei)
    layer.eval()
    with pytest.raises(RuntimeError) as info:                              # past the dropout check: a CPU tensor, no CPU fallback
        layer(torch.randn(5, 6), ei)
    assert not isinstance(info.value, NotImplementedError)


def test_bad_shapes_raise():
    layer = egc_amd.GATv2Conv(6, 4, heads=2)
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="expected \\(rows, 6\\)"):
        layer(torch.randn(5, 7), ei)
    with pytest.raises(RuntimeError, match="expected \\(rows, 6\\)"):
        layer(torch.randn(6), ei)
    with pytest.raises(RuntimeError):
        layer(torch.randn(5, 6).double(), ei)
    from egc_amd._gat import gatv2_aggregate
    with pytest.raises(RuntimeError, match="att must be"):
        gatv2_aggregate(torch.randn(5, 8), torch.randn(5, 8), torch.randn(8), ei)
    with pytest.raises(RuntimeError, match="xr must be"):
        gatv2_aggregate(torch.randn(5, 8), torch.randn(40), torch.randn(2, 4), ei)


def test_c_entries_are_in_the_table_and_reject_bad_arguments_without_device_work():
    lib = _C.load()
    for sym in ("egc_gatv2_forward_f32", "egc_gatv2_forward_workspace_bytes", "egc_gatv2_backward_f32",
                "egc_gatv2_backward_workspace_bytes"):
        assert sym in _C.SYMBOLS and getattr(lib, sym) is not None
    INVALID = 1
    assert lib.egc_gatv2_forward_workspace_bytes(CHUNK, 8, 14) == 0            # no row can be longer than a chunk
    assert lib.egc_gatv2_forward_workspace_bytes(1000, 8, 14) == 4 * 32 * 3 * 16   # 4 slots, 28 lanes padded to 32, (m, l, acc)
    assert lib.egc_gatv2_forward_workspace_bytes(1000, 1, 300) == 4 * 128 * 3 * 16  # two 64-lane slots per row
    assert lib.egc_gatv2_backward_workspace_bytes(10, 0, 2, 4) > 0
    for h, c in ((0, 4), (2, 0), (8, 65)):
        assert lib.egc_gatv2_forward_f32(None, None, 4, 0, 4, None, 600, None, 600, None, h, c, 0.2, 1, None, 600, None, None, 0,
                                         None) == INVALID
    # rows to do and no pointers; a stride smaller than the width; self loops on a non-square graph
    assert lib.egc_gatv2_forward_f32(None, None, 4, 0, 4, None, 8, None, 8, None, 2, 4, 0.2, 1, None, 8, None, None, 0, None) == INVALID
    assert lib.egc_gatv2_forward_f32(None, None, 4, 0, 4, None, 4, None, 8, None, 2, 4, 0.2, 1, None, 8, None, None, 0, None) == INVALID
    assert lib.egc_gatv2_forward_f32(None, None, 4, 0, 5, None, 8, None, 8, None, 2, 4, 0.2, 1, None, 8, None, None, 0, None) == INVALID
    assert lib.egc_gatv2_backward_f32(None, None, None, None, 4, 0, None, 8, None, 8, None, 2, 4, 0.2, 1, None, 8, None, None, 8,
                                      16, 8, None, 0, None, None, 0, None) == INVALID
