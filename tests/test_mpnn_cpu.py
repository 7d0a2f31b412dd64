"""The baseline MPNN layer without a GPU: the fixtures of the reference's own Mpnn (tests/golden/mpnn) and the properties their
graphs must have, the float64 restatement through the P / Q split and the folded update (tests/mpnn_ref.py) against them, and
the host side of egc_amd.Mpnn (construction under a seed, parameter names, the import shim, argument errors)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd import _C
from mpnn_ref import CASES, CHUNK, MAX_CASES, csr_by_destination, layer_forward, load_mpnn_golden, rel_grad, rel_out


@functools.lru_cache(maxsize=None)
def fixture(name):
    return load_mpnn_golden(name)


def test_every_case_of_the_table_is_there():
    assert _C.load().egc_typed_mean_chunk() == CHUNK
    want = dict(messy=(16, 4), hub=(8, 2), ties=(8, 2), odd=(6, 2), w116=(116, 4), t1=(12, 1))
    for name in CASES:
        g = fixture(name)
        m = g["meta"]
        assert m["chunk"] == CHUNK and f"{m['name']}_{m['aggr']}" == name and (m["d"], m["towers"]) == want[m["name"]]
        assert g["x"].shape == (m["n"], m["d"]) == g["out64"].shape == g["gout"].shape and g["out64"].dtype == np.float64
        assert (g["arg"] is not None) == (name in MAX_CASES)
        assert set(g["grad64"]) == set(g["params"]) == set(g["init"])


@pytest.mark.parametrize("name", [c for c in CASES if c.startswith(("messy", "hub", "ties"))])
def test_graphs_have_the_properties_the_cases_are_for(name):
    g = fixture(name)
    ei, n = g["ei"], g["meta"]["n"]
    pairs = ei[0] * n + ei[1]
    dups = len(pairs) - len(np.unique(pairs))
    if name.startswith("messy"):
        assert n == 57 and int((ei[0] == ei[1]).sum()) >= 9 and dups >= 20
        assert ei.max() < n - 3                                           # three isolated tail rows
        assert (np.bincount(ei[1], minlength=n) == 0).any()
    elif name.startswith("hub"):
        assert np.bincount(ei[1], minlength=n).max() > 2 * CHUNK + 1      # a row of more than two chunks and one entry
        assert np.bincount(ei[0], minlength=n).max() > 2 * CHUNK + 1      # and a source with as many out-edges
        assert 600 <= n <= 800
    else:
        assert n == 20 and dups >= 25
        assert np.array_equal(g["x"], np.round(g["x"])) and all(np.array_equal(8 * v, np.round(8 * v)) for v in g["params"].values())
        # arg names an in-edge of its own row (that the maxima really tie between different edges: tests/test_mpnn_gpu.py)
        rowptr, col, eid = csr_by_destination(ei, n)
        assert g["arg"].min() >= -1 and g["arg"].max() < ei.shape[1]
        live = g["arg"] >= 0
        assert np.array_equal(ei[1][g["arg"][live]], np.nonzero(live)[0])


@pytest.mark.parametrize("name", CASES)
def test_float64_restatement_reproduces_the_reference(name):
    """The P / Q split and the folded update differ from the reference's formulation by float64 rounding only: 1e-10 relative
    on the output and on every gradient."""
    g = fixture(name)
    m = g["meta"]
    params = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in g["params"].items()}
    x = torch.from_numpy(g["x"]).double().requires_grad_(True)
    out = layer_forward(x, g["ei"], params, m["towers"], m["aggr"])
    out.backward(torch.from_numpy(g["gout"]).double())
    assert rel_out(out.detach().numpy(), g["out64"]) <= 1e-10
    assert rel_grad(x.grad.numpy(), g["grad_x64"]) <= 1e-10
    for k, p in params.items():
        assert rel_grad(p.grad.numpy(), g["grad64"][k]) <= 1e-10, k


@pytest.mark.parametrize("name", CASES)
def test_seed_gives_the_reference_initial_parameters_and_names(name):
    g = fixture(name)
    m = g["meta"]
    torch.manual_seed(m["seed"])
    layer = egc_amd.Mpnn(m["aggr"], m["d"], m["d"], towers=m["towers"])
    state = layer.state_dict()
    assert list(state) == list(g["init"])
    for k, v in state.items():
        assert v.shape == g["init"][k].shape and torch.equal(v, torch.from_numpy(g["init"][k])), k
    layer.load_state_dict({k: torch.from_numpy(v) for k, v in g["params"].items()}, strict=True)
    for k, v in layer.state_dict().items():
        assert torch.equal(v, torch.from_numpy(g["params"][k])), k
    assert (layer.towers, layer.in_dim, layer.out_dim, layer.aggr) == (m["towers"], m["d"], m["d"], m["aggr"])


def test_import_shim_resolves():
    from experiments.layers import EfficientGraphConv, Mpnn
    assert Mpnn is egc_amd.Mpnn and EfficientGraphConv is egc_amd.EfficientGraphConv


def test_construction_and_forward_errors():
    for bad in ("min", "sum", None):
        with pytest.raises(ValueError, match="aggr must be one of"):
            egc_amd.Mpnn(bad, 8, 8)
    with pytest.raises(AssertionError):
        egc_amd.Mpnn("add", 10, 8, towers=4)
    layer = egc_amd.Mpnn("add", 8, 16, towers=4)                         # the reference constructs this pair too
    assert layer.message_layer[0].weight.shape == (4, 4) and layer.update_layer[0].weight.shape == (4, 8)
    ei = torch.zeros((2, 3), dtype=torch.int64)
    with pytest.raises(RuntimeError, match="in_dim .8. != out_dim .16."):
        layer(torch.randn(5, 8), ei)
    layer = egc_amd.Mpnn("max", 8, 8, towers=2)
    with pytest.raises(RuntimeError, match="expected \\(rows, 8\\)"):
        layer(torch.randn(5, 7), ei)
    with pytest.raises(RuntimeError):                                    # a CPU tensor: there is no CPU fallback
        layer(torch.randn(5, 8), ei)


def test_c_entries_reject_bad_arguments_without_device_work():
    lib = _C.load()
    INVALID = 1
    assert lib.egc_mpnn_message_workspace_bytes(CHUNK, 30, _C.MPNN_ADD) == 0          # no row can be longer than a chunk
    assert lib.egc_mpnn_message_workspace_bytes(1000, 30, _C.MPNN_ADD) == 4 * 8 * 16  # ceil(1000 / 256) slots of 8 lanes
    assert lib.egc_mpnn_message_workspace_bytes(1000, 30, _C.MPNN_MAX) == 2 * 4 * 8 * 16     # values and positions
    assert lib.egc_mpnn_message_backward_workspace_bytes(1000, 30) == 4 * 8 * 16
    for width in (0, -4):
        assert lib.egc_mpnn_message_f32(None, None, None, 4, 0, 4, None, 8, None, 8, width, 0, None, 8, None, None, 0, None) == INVALID
        assert lib.egc_mpnn_message_backward_f32(None, None, 4, None, None, None, 4, 0, None, 8, None, width, 0, None, 8, None, 8,
                                                 None, 0, None) == INVALID
    # width 8, rows to do, and no pointers at all
    assert lib.egc_mpnn_message_f32(None, None, None, 4, 0, 4, None, 8, None, 8, 8, 0, None, 8, None, None, 0, None) == INVALID
    assert lib.egc_mpnn_message_f32(None, None, None, 4, 0, 4, None, 8, None, 8, 8, 3, None, 8, None, None, 0, None) == INVALID  # op
    assert lib.egc_mpnn_message_f32(None, None, None, 4, 0, 4, None, 4, None, 8, 8, 0, None, 8, None, None, 0, None) == INVALID  # ld_p
    # the backward with an output asked for (a non-null d Q) and nothing to read
    assert lib.egc_mpnn_message_backward_f32(None, None, 4, None, None, None, 4, 0, None, 8, None, 8, 0, None, 8, 16, 8,
                                             None, 0, None) == INVALID
