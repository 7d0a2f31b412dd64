"""The output head and loss on CPU tensors (no GPU): egc_amd.log_softmax / nll_log_softmax / cross_entropy take torch's
operators there and must equal F.log_softmax / F.nll_loss / F.cross_entropy; argument errors; RowSelection's counts; the
float64 reference of the GPU tests against torch's own float64."""
import os

import pytest
import torch
import torch.nn.functional as F

import egc_amd
import softmax_ref as ref
from egc_amd import _C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("c,ld", [(349, 352), (40, 40), (7, 9), (1, 1), (1025, 1030)])
def test_log_softmax_on_cpu_is_torchs(c, ld):
    torch.manual_seed(c)
    x = torch.randn(50, ld, requires_grad=True)
    out, arg = egc_amd.log_softmax(x, num_classes=c, return_argmax=True)
    want = F.log_softmax(x[:, :c], dim=-1)
    assert torch.equal(out, want) and torch.equal(arg, want.argmax(-1)) and arg.dtype == torch.int64
    g = torch.randn(50, c)
    out.backward(g)
    got, x.grad = x.grad, None
    want.backward(g)
    assert got.shape == x.shape and torch.equal(got, x.grad)
    assert torch.equal(egc_amd.log_softmax(x.detach()), F.log_softmax(x.detach(), dim=-1))     # num_classes defaults to ld


@pytest.mark.parametrize("reduction", ["mean", "sum"])
@pytest.mark.parametrize("mode", ["none", "tensor", "selection"])
def test_nll_log_softmax_on_cpu_is_torchs(mode, reduction):
    torch.manual_seed(3)
    n, c, ld = 200, 349, 352
    x = torch.randn(n, ld, requires_grad=True)
    y = torch.randint(0, c, (n,))
    idx = torch.randperm(n)[:120]
    index = {"none": None, "tensor": idx, "selection": egc_amd.RowSelection(idx, n)}[mode]
    loss = egc_amd.nll_log_softmax(x, y, index, num_classes=c, reduction=reduction)
    logp = x[:, :c].log_softmax(-1)
    want = F.nll_loss(logp, y, reduction=reduction) if mode == "none" else F.nll_loss(logp[idx], y[idx], reduction=reduction)
    assert torch.equal(loss, want)
    loss.backward()
    got, x.grad = x.grad, None
    want.backward()
    assert got.shape == (n, ld) and torch.equal(got, x.grad)
    assert not got[:, c:].any()


def test_cross_entropy_on_cpu_is_torchs():
    torch.manual_seed(1)
    x, y = torch.randn(128, 10), torch.randint(0, 10, (128,))
    assert torch.equal(egc_amd.cross_entropy(x, y), F.cross_entropy(x, y))


def test_row_selection_counts_duplicates():
    sel = egc_amd.RowSelection(torch.tensor([4, 1, 4, 4, 0]), 6)
    assert sel.cnt.tolist() == [1, 1, 0, 0, 3, 0] and sel.cnt.dtype == torch.int32
    assert sel.M.tolist() == [5] and sel.M.dtype == torch.int64 and sel.n_rows == 6
    empty = egc_amd.RowSelection(torch.zeros(0, dtype=torch.int64), 3)
    assert empty.cnt.tolist() == [0, 0, 0] and empty.M.tolist() == [0]
    # duplicates weigh as often as they occur: the loss of [4, 1, 4, 4, 0] is the mean over five picks
    torch.manual_seed(0)
    x, y = torch.randn(6, 5), torch.randint(0, 5, (6,))
    idx = torch.tensor([4, 1, 4, 4, 0])
    assert torch.equal(egc_amd.nll_log_softmax(x, y, sel), F.nll_loss(x.log_softmax(-1)[idx], y[idx]))


def test_argument_errors():
    x, y = torch.randn(6, 5), torch.randint(0, 5, (6,))
    with pytest.raises(ValueError, match="num_classes"):
        egc_amd.log_softmax(x, num_classes=6)
    with pytest.raises(ValueError, match="num_classes"):
        egc_amd.nll_log_softmax(x, y, num_classes=0)
    with pytest.raises(ValueError, match="rows, width"):
        egc_amd.log_softmax(torch.randn(5))
    with pytest.raises(ValueError, match="reduction"):
        egc_amd.nll_log_softmax(x, y, reduction="none")
    with pytest.raises(ValueError, match="one int64 label per row"):
        egc_amd.nll_log_softmax(x, y[:5])
    with pytest.raises(ValueError, match="one int64 label per row"):
        egc_amd.nll_log_softmax(x, y.to(torch.int32))
    with pytest.raises(ValueError, match="index must be"):
        egc_amd.nll_log_softmax(x, y, index=torch.tensor([0, 1], dtype=torch.int32))
    with pytest.raises(ValueError, match="built for 7 rows"):
        egc_amd.nll_log_softmax(x, y, index=egc_amd.RowSelection(torch.tensor([0]), 7))
    with pytest.raises(ValueError, match="1-D int64"):
        egc_amd.RowSelection(torch.tensor([[0]]), 3)
    with pytest.raises(IndexError):
        egc_amd.RowSelection(torch.tensor([3]), 3)


def test_header_limit_matches_the_binding_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "egc_hip.h")).read()
    assert _C.ABI.constants["EGC_SOFTMAX_MAX_CLASSES"] == _C.SOFTMAX_MAX_CLASSES == 1024
    lib = _C.load()     # host-side size query: one float per chunk of 128 rows, 0 outside the limits
    assert lib.egc_nll_log_softmax_workspace_bytes(1000, 349) == 4 * 8
    assert lib.egc_nll_log_softmax_workspace_bytes(1000, 1025) == 0
    assert "ignore_index" in hdr


def test_float64_reference_against_torch_float64():
    torch.manual_seed(5)
    n, c, ld = 64, 7, 9
    x = (torch.randn(n, ld) * 10).double().requires_grad_(True)
    y = torch.randint(0, c, (n,))
    idx = torch.tensor([0, 5, 5, 9, 63])
    cnt = ref.counts(idx, n)
    logp, lse = ref.log_softmax(x.detach(), c)
    want = x[:, :c].log_softmax(-1)
    assert torch.allclose(logp, want.detach(), rtol=0, atol=1e-12)
    loss = F.nll_loss(want[idx], y[idx])
    got, _ = ref.nll_forward(x.detach(), y, cnt, c, True)
    assert abs(float(got) - float(loss.detach())) <= 1e-12
    (loss * 3.0).backward()
    assert torch.allclose(ref.nll_backward(3.0, x.detach(), y, cnt, c, True), x.grad, rtol=0, atol=1e-12)
    g = torch.randn(n, c).double()
    x.grad = None
    x[:, :c].log_softmax(-1).backward(g)
    assert torch.allclose(ref.log_softmax_backward(g, logp, ld), x.grad, rtol=0, atol=1e-12)
    ties = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 2.0, 9.0]])
    assert ref.first_argmax(ties, 3).tolist() == [1, 0]
