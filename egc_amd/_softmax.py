"""Output head and loss of the reference's classification nets (egc_softmax.hip through the C ABI): the row log-softmax
with its arg-max, and the selected-row NLL loss fused with it.

The reference writes ``conv(x)[:, :349].log_softmax(-1)``, ``out[train_idx]``, ``F.nll_loss(out, y[train_idx])``
(mag/models.py:68-69 with mag/configs.py:34-35; arxiv/norm_models.py:42-43 with arxiv/configs.py:53-54;
rmag/configs.py:35-36) or ``F.cross_entropy`` (cifar/configs.py:57).  ``nll_log_softmax`` takes the FULL-WIDTH logits, so its
gradient has their shape and padding: the forward reads the selected rows once, the backward reads them once more and
writes every element of the gradient once.  CPU tensors, dtypes other than float32 and more than 1,024 classes take
torch's operators.  Nothing reads back from the device: all of it records inside ``GraphedStep``; an index or a label out
of range contributes nothing and raises at the deferred check (graph._IndexFlag), as the encoders' indices do.
``ignore_index`` and class weights are not supported (the reference uses neither).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _C
from ._args import _check_f32, _ptr
from .graph import _IndexFlag, _device_guard, _stream_ptr


def _rows(x: torch.Tensor, num_classes) -> int:
    """The validated class count of x [N, ld]."""
    if x.dim() != 2:
        raise ValueError(f"egc_amd: logits must be [rows, width] (got {tuple(x.shape)})")
    c = x.size(1) if num_classes is None else int(num_classes)
    if not 1 <= c <= max(x.size(1), 1):
        raise ValueError(f"egc_amd: num_classes must be in [1, {x.size(1)}] (got {c})")
    return c


def softmax_supported(x: torch.Tensor, n_classes: int) -> bool:
    """Whether the kernels take x: a float32 tensor on a ROCm device with at most EGC_SOFTMAX_MAX_CLASSES classes."""
    return x.is_cuda and x.dtype == torch.float32 and n_classes <= _C.SOFTMAX_MAX_CLASSES


def log_softmax_forward(x: torch.Tensor, n_classes: int, want_lse: bool = False, want_argmax: bool = False):
    """(out [N, n_classes], lse [N] or None, argmax int32 [N] or None) of the rows of x [N, ld]
    (egc_log_softmax_forward_f32): one launch, one read of x; the first maximal column wins the arg-max."""
    lib = _C.load()
    _check_f32(x, "x")
    x = x.contiguous()
    n, dev = x.size(0), x.device
    with _device_guard(dev):
        out = torch.empty((n, n_classes), dtype=torch.float32, device=dev)
        lse = torch.empty(n, dtype=torch.float32, device=dev) if want_lse else None
        arg = torch.empty(n, dtype=torch.int32, device=dev) if want_argmax else None
        _C.check(lib.egc_log_softmax_forward_f32(x.data_ptr(), n, n_classes, x.size(1), out.data_ptr(), _ptr(lse), _ptr(arg),
                                                 _stream_ptr(dev)), "egc_log_softmax_forward_f32")
    return out, lse, arg


def log_softmax_backward(grad_out: torch.Tensor, out: torch.Tensor, ld: int) -> torch.Tensor:
    """d x [N, ld] of log_softmax_forward (egc_log_softmax_backward_f32): g - exp(out) * sum(g) per row, zeros in the
    padding columns; every element written once."""
    lib = _C.load()
    _check_f32(grad_out, "grad_out")
    _check_f32(out, "out", grad_out.shape)
    grad_out, out = grad_out.contiguous(), out.contiguous()
    n, c, dev = out.size(0), out.size(1), out.device
    with _device_guard(dev):
        dx = torch.empty((n, int(ld)), dtype=torch.float32, device=dev)
        _C.check(lib.egc_log_softmax_backward_f32(grad_out.data_ptr(), out.data_ptr(), n, c, int(ld), dx.data_ptr(),
                                                  _stream_ptr(dev)), "egc_log_softmax_backward_f32")
    return dx


class RowSelection:
    """The rows a loss is taken over, as counts: ``cnt`` (int32 [n_rows], how often each row occurs in ``index``) and ``M``
    (int64 [1], the number of selected rows, duplicates counted), both on ``index``'s device.  Build it once for a fixed
    ``train_idx`` and pass it wherever ``index=`` is accepted; a plain index tensor builds one per call.  An index outside
    [0, n_rows) is never used as an address on the device: it is not counted and the deferred check raises."""

    def __init__(self, index: torch.Tensor, n_rows: int):
        if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.dtype != torch.int64:
            raise ValueError("egc_amd: a row selection is built from a 1-D int64 index tensor")
        if int(n_rows) < 0:
            raise ValueError(f"egc_amd: n_rows must be >= 0 (got {n_rows})")
        self.index, self.n_rows, dev = index, int(n_rows), index.device
        if not index.is_cuda:
            if index.numel() and (int(index.min()) < 0 or int(index.max()) >= self.n_rows):
                raise IndexError(f"egc_amd: index out of range for {self.n_rows} rows")
            self.cnt = torch.bincount(index, minlength=self.n_rows).to(torch.int32)
            self.M = torch.tensor([index.numel()], dtype=torch.int64)
            return
        lib = _C.load()
        _IndexFlag.poll()
        index = index.contiguous()
        with _device_guard(dev):
            self.cnt = torch.empty(self.n_rows, dtype=torch.int32, device=dev)
            self.M = torch.empty(1, dtype=torch.int64, device=dev)
            _C.check(lib.egc_row_selection_count(index.data_ptr(), index.numel(), self.n_rows, self.cnt.data_ptr(),
                                                 self.M.data_ptr(), _IndexFlag.ptr(), _stream_ptr(dev)),
                     "egc_row_selection_count")


def nll_forward(x: torch.Tensor, y: torch.Tensor, sel, n_classes: int, mean: bool):
    """(loss 0-dim, lse [N]) of the selected rows of x [N, ld] (egc_nll_log_softmax_forward_f32); ``sel`` a RowSelection
    or None for every row once.  Two launches, a fixed summation order, no float atomics."""
    lib = _C.load()
    _IndexFlag.poll()
    n, dev = x.size(0), x.device
    with _device_guard(dev):
        loss = torch.empty((), dtype=torch.float32, device=dev)
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        nbytes = int(lib.egc_nll_log_softmax_workspace_bytes(n, n_classes))
        ws = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=dev)
        _C.check(lib.egc_nll_log_softmax_forward_f32(x.data_ptr(), y.data_ptr(), _ptr(sel.cnt if sel else None),
                                                     _ptr(sel.M if sel else None), n, n_classes, x.size(1), int(mean),
                                                     loss.data_ptr(), lse.data_ptr(), ws.data_ptr(), nbytes,
                                                     _IndexFlag.ptr(), _stream_ptr(dev)), "egc_nll_log_softmax_forward_f32")
    return loss, lse


def nll_backward(grad_loss: torch.Tensor, x: torch.Tensor, y: torch.Tensor, cnt, total, lse: torch.Tensor, n_classes: int,
                 mean: bool) -> torch.Tensor:
    """d x [N, ld] of nll_forward (egc_nll_log_softmax_backward_f32): one launch that writes every element once -- zeros in
    the padding columns and on the rows outside the selection."""
    lib = _C.load()
    n, dev = x.size(0), x.device
    grad_loss = grad_loss.to(torch.float32).contiguous()
    with _device_guard(dev):
        dx = torch.empty_like(x)
        _C.check(lib.egc_nll_log_softmax_backward_f32(x.data_ptr(), y.data_ptr(), _ptr(cnt), _ptr(total), lse.data_ptr(),
                                                      grad_loss.data_ptr(), n, n_classes, x.size(1), int(mean),
                                                      dx.data_ptr(), _stream_ptr(dev)), "egc_nll_log_softmax_backward_f32")
    return dx


class _LogSoftmaxFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_classes, want_argmax):
        out, _, arg = log_softmax_forward(x, n_classes, want_argmax=want_argmax)
        ctx.ld = x.size(1)
        ctx.save_for_backward(out)
        if want_argmax:
            ctx.mark_non_differentiable(arg)
            return out, arg
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_out, *_):
        (out,) = ctx.saved_tensors
        return log_softmax_backward(d_out, out, ctx.ld), None, None


class _NllFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, sel, n_classes, mean):
        loss, lse = nll_forward(x, y, sel, n_classes, mean)
        ctx.n_classes, ctx.mean, ctx.selected = n_classes, mean, sel is not None
        ctx.save_for_backward(x, y, lse, *((sel.cnt, sel.M) if sel is not None else ()))
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        x, y, lse, *sel = ctx.saved_tensors
        cnt, total = sel if ctx.selected else (None, None)
        return nll_backward(d_loss, x, y, cnt, total, lse, ctx.n_classes, ctx.mean), None, None, None, None


def log_softmax(x: torch.Tensor, num_classes: int | None = None, return_argmax: bool = False):
    """``x[:, :num_classes].log_softmax(-1)`` of the full-width logits x [N, ld] (``num_classes`` defaults to ld) as a
    dense [N, num_classes] tensor, differentiable; the gradient has x's shape, zeros in the padding columns.  With
    ``return_argmax`` also the int64 [N] arg-max of each row, the first maximal column -- the ``out.argmax(-1)`` of the
    reference's ``test()`` -- from the same read of x."""
    c = _rows(x, num_classes)
    if not softmax_supported(x, c):
        out = x[:, :c].log_softmax(-1)
        return (out, out.argmax(-1)) if return_argmax else out
    x = x.contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        res = _LogSoftmaxFunction.apply(x, c, return_argmax)
    else:
        out, _, arg = log_softmax_forward(x, c, want_argmax=return_argmax)
        res = (out, arg) if return_argmax else out
    return (res[0], res[1].to(torch.int64)) if return_argmax else res


def nll_log_softmax(x: torch.Tensor, y: torch.Tensor, index=None, num_classes: int | None = None,
                    reduction: str = "mean") -> torch.Tensor:
    """``F.nll_loss(x[:, :num_classes].log_softmax(-1)[index], y[index], reduction=reduction)`` of the full-width logits
    x [N, ld] and the labels y [N] of ALL rows (int64).  ``index``: None (every row), a 1-D int64 tensor of row numbers
    (duplicates count as often as they occur) or a ``RowSelection`` built once from it.  ``reduction``: "mean" | "sum".
    The gradient with respect to x has x's own shape: zeros in the padding columns and on rows outside the selection,
    every element written once.  The sum runs in a fixed order (include/egc_hip.h): two calls give the same bits."""
    c = _rows(x, num_classes)
    if reduction not in ("mean", "sum"):
        raise ValueError(f"egc_amd: reduction must be 'mean' or 'sum' (got {reduction!r})")
    if y.dim() != 1 or y.size(0) != x.size(0) or y.dtype != torch.int64 or y.device != x.device:
        raise ValueError(f"egc_amd: y must hold one int64 label per row of x, on its device (got {y.dtype} "
                         f"{tuple(y.shape)} for {x.size(0)} rows)")
    sel = index
    if isinstance(index, RowSelection):
        if index.n_rows != x.size(0) or index.cnt.device != x.device:
            raise ValueError(f"egc_amd: the row selection was built for {index.n_rows} rows on {index.cnt.device}, "
                             f"x has {x.size(0)} on {x.device}")
    elif index is not None:
        if not isinstance(index, torch.Tensor) or index.dim() != 1 or index.dtype != torch.int64 or index.device != x.device:
            raise ValueError("egc_amd: index must be None, a RowSelection or a 1-D int64 tensor on x's device")
    if not softmax_supported(x, c):
        idx = sel.index if isinstance(sel, RowSelection) else sel
        logp = x[:, :c].log_softmax(-1)
        return F.nll_loss(logp, y, reduction=reduction) if idx is None else F.nll_loss(logp[idx], y[idx], reduction=reduction)
    if sel is not None and not isinstance(sel, RowSelection):
        sel = RowSelection(sel, x.size(0))
    x, y = x.contiguous(), y.contiguous()
    if torch.is_grad_enabled() and x.requires_grad:
        return _NllFunction.apply(x, y, sel, c, reduction == "mean")
    return nll_forward(x, y, sel, c, reduction == "mean")[0]


def cross_entropy(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """``F.cross_entropy(logits, target)`` for class-index targets (cifar/configs.py:57): ``nll_log_softmax`` over every
    row and column."""
    return nll_log_softmax(logits, target)
