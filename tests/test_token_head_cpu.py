"""The token head without a GPU: on CPU tensors TokenHead and the functional forms ARE the reference's expression (bit for
bit), the module is state-dict compatible with the reference's ``token_predictors``, arguments are checked, the header, the
binding and the host-only workspace query agree, and the float64 reference of token_head_ref.py is torch's float64."""
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import egc_amd
from egc_amd import _C
import token_head_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _reference_head(k, v, t, seed=0):
    torch.manual_seed(seed)
    return nn.ModuleList(nn.Linear(k, v) for _ in range(t))


@pytest.mark.parametrize("g,k,v,t", [(6, 12, 37, 5), (1, 4, 1, 1), (5, 302, 70, 3), (4, 8, 9, 9), (0, 8, 5, 2)])
def test_cpu_tensors_take_the_reference_expression_bit_for_bit(g, k, v, t):
    theirs = _reference_head(k, v, t)
    ours = egc_amd.TokenHead(k, v, t)
    ours.load_state_dict(theirs.state_dict())
    x = torch.randn(g, k)
    y = torch.randint(0, v, (g, t))
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    preds = [p(xa) for p in theirs]
    want = sum(F.cross_entropy(preds[i], y[:, i]) for i in range(t)) / t
    got = ours.loss(xb, y)
    assert torch.equal(got, want) or (g == 0 and bool(torch.isnan(got)) and bool(torch.isnan(want)))
    for a, b in zip(ours(xb), preds):
        assert torch.equal(a, b)
    assert torch.equal(ours.predict(x), torch.stack([torch.argmax(p, dim=1) for p in preds], dim=1))
    assert ours.predict(x).dtype == torch.int64 and ours.predict(x).shape == (g, t)
    if g:
        want.backward()
        got.backward()
        assert torch.equal(xa.grad, xb.grad)
        for a, b in zip(ours.parameters(), theirs.parameters()):
            assert torch.equal(a.grad, b.grad)
    ws, bs = [p.weight for p in theirs], [p.bias for p in theirs]
    assert torch.equal(egc_amd.token_head_loss(x, ws, bs, y), want.detach()) or g == 0
    assert torch.equal(egc_amd.token_head_argmax(x, ws, bs), ours.predict(x))


def test_state_dict_of_the_reference_module_list_loads_strictly():
    class Theirs(nn.Module):
        def __init__(self):
            super().__init__()
            self.token_predictors = nn.ModuleList(nn.Linear(12, 37) for _ in range(5))

    class Ours(nn.Module):
        def __init__(self):
            super().__init__()
            self.token_predictors = egc_amd.TokenHead(12, 37, 5)

    theirs, ours = Theirs(), Ours()
    assert list(ours.state_dict()) == list(theirs.state_dict())
    ours.load_state_dict(theirs.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    assert [tuple(p.shape) for p in ours.parameters()] == [tuple(p.shape) for p in theirs.parameters()]
    for a, b in zip(ours.parameters(), theirs.parameters()):
        assert torch.equal(a, b)
    assert len(torch.optim.SGD(ours.parameters(), lr=0.1).param_groups[0]["params"]) == 10


def test_argument_errors():
    head = egc_amd.TokenHead(8, 11, 3)
    x = torch.randn(4, 8)
    with pytest.raises(ValueError, match="y_arr"):
        head.loss(x, torch.zeros(4, dtype=torch.int64))                  # one column short of [G, T]
    with pytest.raises(ValueError, match="y_arr"):
        head.loss(x, torch.zeros(4, 2, dtype=torch.int64))
    with pytest.raises(ValueError, match="y_arr"):
        head.loss(x, torch.zeros(3, 3, dtype=torch.int64))
    with pytest.raises(ValueError, match="y_arr"):
        head.loss(x, torch.zeros(4, 3, dtype=torch.int32))
    ws, bs = [p.weight for p in head], [p.bias for p in head]
    y = torch.zeros(4, 3, dtype=torch.int64)
    with pytest.raises(ValueError, match="weight"):
        egc_amd.token_head_loss(x, ws[:2] + [torch.randn(12, 8)], bs, y)  # another vocabulary
    with pytest.raises(ValueError, match="weight"):
        egc_amd.token_head_loss(torch.randn(4, 6), ws, bs, y)             # another width
    with pytest.raises(ValueError, match="per position"):
        egc_amd.token_head_loss(x, ws, bs[:2], y)
    with pytest.raises(ValueError, match="weight"):
        egc_amd.token_head_argmax(x, ws, [b[:5] for b in bs])
    with pytest.raises(ValueError, match="in_features"):
        egc_amd.token_head_loss(torch.randn(8), ws, bs, y)
    with pytest.raises(ValueError, match="positive"):
        egc_amd.TokenHead(8, 11, 0)
    # more positions than the kernels take is no error: nine positions are the reference's expression (the GPU test holds
    # the same call on the device to torch), and the C side answers EGC_ERR_UNSUPPORTED / a zero workspace
    assert _C.load().egc_token_head_workspace_bytes(4, 8, 11, _C.TOKEN_HEAD_MAX_SEQ + 1) == 0


def test_header_constants_match_the_binding():
    hdr = open(os.path.join(ROOT, "include", "egc_hip.h")).read()
    header = _C.ABI.constants
    assert header["EGC_TOKEN_HEAD_MAX_SEQ"] == _C.TOKEN_HEAD_MAX_SEQ == 8
    assert header["EGC_TOKEN_HEAD_SLAB"] == _C.TOKEN_HEAD_SLAB == 64
    assert header["EGC_TOKEN_HEAD_MAX_IN"] == _C.TOKEN_HEAD_MAX_IN == 384
    for name in ("egc_token_head_workspace_bytes", "egc_token_head_forward_f32", "egc_token_head_backward_f32"):
        assert name in _C.SYMBOLS
    assert "stay with the caller" not in hdr


def test_workspace_query_is_zero_outside_the_envelope_and_positive_inside():
    q = _C.load().egc_token_head_workspace_bytes
    assert q(128, 304, 5002, 5) > 0 and q(128, 300, 5002, 5) > 0
    assert q(128, 384, 1, 8) > 0 and q(1, 4, 1, 1) > 0 and q(0, 304, 5002, 5) > 0
    for bad in [(128, 302, 5002, 5), (128, 388, 5002, 5), (128, 304, 5002, 9), (128, 304, 0, 5), (128, 0, 5002, 5),
                (-1, 304, 5002, 5), (128, 304, 5002, 0)]:
        assert q(*bad) == 0, bad
    # the dx partials dominate at the reference's shape: one [G, K] array per workgroup, never one per slab
    slabs = 5 * -(-5002 // _C.TOKEN_HEAD_SLAB)
    assert q(128, 304, 5002, 5) <= min(slabs, 256) * 128 * 304 * 4 + 16


@pytest.mark.parametrize("g,k,v,t", [(9, 12, 37, 5), (3, 4, 1, 2)])
def test_float64_reference_is_torch_float64(g, k, v, t):
    x, ws, bs, y = ref.make_inputs(g, k, v, t, "mixed", seed=g)
    y[0, 0] = v - 1
    r = ref.reference(x, ws, bs, y, grad_loss=3.0)
    xd = x.double().requires_grad_(True)
    wd = [w.double().requires_grad_(True) for w in ws]
    bd = [b.double().requires_grad_(True) for b in bs]
    loss = ref.torch_composition(xd, wd, bd, y)
    (3.0 * loss).backward()
    loss = loss.detach()
    assert abs(r["loss"] - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert float((r["dx"] - xd.grad).abs().max()) <= 1e-12
    for i in range(t):
        assert float((r["dw"][i] - wd[i].grad).abs().max()) <= 1e-12
        assert float((r["db"][i] - bd[i].grad).abs().max()) <= 1e-12
    logits = torch.stack([F.linear(xd, w, b) for w, b in zip(wd, bd)]).detach()
    assert float((r["lse"] - torch.logsumexp(logits, dim=2).t()).abs().max()) <= 1e-12
    assert torch.equal(ref.first_argmax(logits), logits.argmax(dim=2).t())
    assert bool((r["logit_bound"] > 0).all()) and bool((r["lse_bound"] > 0).all()) and r["loss_bound"] > 0
