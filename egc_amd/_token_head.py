"""The token head of the reference's ogbg-code net (egc_token_head.hip through the C ABI): ``seq_len`` Linear maps of the
pooled graph rows onto the vocabulary, fused with the mean cross-entropy over the positions and with the arg-max.

The reference writes (code/models.py:95-98, 121-125 with code/configs.py:63-66, 94)

    self.token_predictors = nn.ModuleList(nn.Linear(hidden, 5002) for _ in range(5))
    preds = [p(x) for p in self.token_predictors]
    loss  = sum(F.cross_entropy(preds[i], y_arr[:, i]) for i in range(5)) / 5
    pred  = torch.argmax(preds[i], dim=1)

``token_head_loss`` and ``token_head_argmax`` compute the last two lines without the logits: x, the weights, y, one lse per
(row, position) and the gradients are all that crosses memory.  CPU tensors, dtypes other than float32 and shapes outside
the kernels' envelope (in_features % 4 != 0 or > 384, more than 8 positions) take torch's composition, exactly the
reference's expression.  Nothing reads back from the device: all of it records inside ``GraphedStep``; a label outside
[0, num_classes) contributes nothing and raises at the deferred check (graph._IndexFlag), as the NLL head's labels do.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C
from ._args import _ptr, _workspace
from .graph import _IndexFlag, _device_guard, _stream_ptr


def _head_args(x, weights, biases):
    """The validated (weights, biases, in_features, num_classes) of a head call."""
    weights, biases = list(weights), list(biases)
    if x.dim() != 2:
        raise ValueError(f"egc_amd: x must be [graphs, in_features] (got {tuple(x.shape)})")
    if not weights or len(weights) != len(biases):
        raise ValueError(f"egc_amd: the token head needs one weight and one bias per position (got {len(weights)} and "
                         f"{len(biases)})")
    v, k = weights[0].size(0) if weights[0].dim() else 0, x.size(1)
    for w, b in zip(weights, biases):
        if tuple(w.shape) != (v, k) or v < 1 or tuple(b.shape) != (v,):
            raise ValueError(f"egc_amd: every position needs a weight [num_classes, {x.size(1)}] and a bias [num_classes] of "
                             f"one num_classes (got {tuple(w.shape)} and {tuple(b.shape)})")
        if w.device != x.device or b.device != x.device or w.dtype != x.dtype or b.dtype != x.dtype:
            raise ValueError("egc_amd: x and the token head's parameters must share one device and dtype")
    return weights, biases, k, v


def _check_labels(x, y_arr, seq_len):
    if (not isinstance(y_arr, torch.Tensor) or y_arr.dim() != 2 or tuple(y_arr.shape) != (x.size(0), seq_len)
            or y_arr.dtype != torch.int64 or y_arr.device != x.device):
        got = f"{y_arr.dtype} {tuple(y_arr.shape)}" if isinstance(y_arr, torch.Tensor) else type(y_arr).__name__
        raise ValueError(f"egc_amd: y_arr must hold one int64 label per row and position, [{x.size(0)}, {seq_len}] on x's "
                         f"device (got {got})")


def token_head_supported(x: torch.Tensor, weights, biases) -> bool:
    """Whether the kernels take the call: float32 on a ROCm device, in_features % 4 == 0 and <= 384, at most
    EGC_TOKEN_HEAD_MAX_SEQ positions, 16-byte aligned dense operands."""
    k = x.size(1)
    if not (x.is_cuda and x.dtype == torch.float32 and k % 4 == 0 and 0 < k <= _C.TOKEN_HEAD_MAX_IN
            and len(weights) <= _C.TOKEN_HEAD_MAX_SEQ):
        return False
    return all(w.is_contiguous() and b.is_contiguous() and w.data_ptr() % 16 == 0 for w, b in zip(weights, biases))


def _pointers(tensors):
    return (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _head_workspace(lib, g, k, v, t, dev):
    return _workspace(lib.egc_token_head_workspace_bytes(g, k, v, t), dev,
                      f"egc_amd: the token head's kernels do not take [{g}, {k}] x {t} x [{v}, {k}]")


def head_forward(x, weights, biases, y, want_argmax: bool):
    """(loss 0-dim or None, lse [G, T] or None, argmax int32 [G, T] or None) (egc_token_head_forward_f32); ``y`` None is the
    evaluation form.  No [G, V] array: the slabs' records and the workspace are all that is allocated."""
    lib = _C.load()
    _IndexFlag.poll()
    g, k, v, t, dev = x.size(0), x.size(1), weights[0].size(0), len(weights), x.device
    with _device_guard(dev):
        loss = torch.empty((), dtype=torch.float32, device=dev) if y is not None else None
        lse = torch.empty((g, t), dtype=torch.float32, device=dev) if y is not None else None
        arg = torch.empty((g, t), dtype=torch.int32, device=dev) if want_argmax else None
        ws, nbytes = _head_workspace(lib, g, k, v, t, dev)
        _C.check(lib.egc_token_head_forward_f32(x.data_ptr(), _pointers(weights), _pointers(biases), _ptr(y), g, k, v, t,
                                                _ptr(loss), _ptr(lse), _ptr(arg), ws.data_ptr(), nbytes, _IndexFlag.ptr(),
                                                _stream_ptr(dev)), "egc_token_head_forward_f32")
    return loss, lse, arg


def head_backward(grad_loss, x, weights, biases, y, lse, want_dx: bool, want_dw: bool, want_db: bool):
    """(d_x or None, [d_W_t] or None, [d_b_t] or None) (egc_token_head_backward_f32): the logit tiles are formed again from
    the forward's lse; every gradient element is written by the kernels, no zero fill."""
    lib = _C.load()
    g, k, v, t, dev = x.size(0), x.size(1), weights[0].size(0), len(weights), x.device
    grad_loss = grad_loss.to(torch.float32).contiguous()
    with _device_guard(dev):
        dx = torch.empty_like(x) if want_dx else None
        dw = [torch.empty_like(w) for w in weights] if want_dw else None
        db = [torch.empty_like(b) for b in biases] if want_db else None
        ws, nbytes = _head_workspace(lib, g, k, v, t, dev)
        _C.check(lib.egc_token_head_backward_f32(x.data_ptr(), _pointers(weights), _pointers(biases), y.data_ptr(),
                                                 lse.data_ptr(), grad_loss.data_ptr(), g, k, v, t, _ptr(dx),
                                                 _pointers(dw) if want_dw else None, _pointers(db) if want_db else None,
                                                 ws.data_ptr(), nbytes, _stream_ptr(dev)), "egc_token_head_backward_f32")
    return dx, dw, db


class _TokenHeadLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, seq_len, *params):
        weights, biases = params[:seq_len], params[seq_len:]
        loss, lse, _ = head_forward(x, weights, biases, y, want_argmax=False)
        ctx.seq_len = seq_len
        ctx.save_for_backward(x, y, lse, *params)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        x, y, lse, *params = ctx.saved_tensors
        t = ctx.seq_len
        weights, biases = params[:t], params[t:]
        need = ctx.needs_input_grad
        dx, dw, db = head_backward(d_loss, x, weights, biases, y, lse, need[0], any(need[3:3 + t]), any(need[3 + t:]))
        grads = [dw[i] if need[3 + i] else None for i in range(t)] + [db[i] if need[3 + t + i] else None for i in range(t)]
        return (dx, None, None, *grads)


def _reference_loss(x, weights, biases, y_arr):
    return sum(F.cross_entropy(F.linear(x, w, b), y_arr[:, i]) for i, (w, b) in enumerate(zip(weights, biases))) / len(weights)


def token_head_loss(x: torch.Tensor, weights, biases, y_arr: torch.Tensor) -> torch.Tensor:
    """``sum(F.cross_entropy(F.linear(x, weights[i], biases[i]), y_arr[:, i]) for i in range(T)) / T`` of the pooled rows
    x [G, in_features], T weights [num_classes, in_features] with their biases, and the labels y_arr [G, T] (int64),
    differentiable with respect to x and every weight and bias.  On the device no logits array exists forward or backward;
    the sums run in a fixed order (include/egc_hip.h): two calls give the same bits."""
    weights, biases, _, _ = _head_args(x, weights, biases)
    _check_labels(x, y_arr, len(weights))
    if not token_head_supported(x, weights, biases):
        return _reference_loss(x, weights, biases, y_arr)
    x, y_arr = x.contiguous(), y_arr.contiguous()
    if x.data_ptr() % 16:
        return _reference_loss(x, weights, biases, y_arr)
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in weights + biases)):
        return _TokenHeadLoss.apply(x, y_arr, len(weights), *weights, *biases)
    return head_forward(x.detach(), [w.detach() for w in weights], [b.detach() for b in biases], y_arr, want_argmax=False)[0]


@torch.no_grad()
def token_head_argmax(x: torch.Tensor, weights, biases) -> torch.Tensor:
    """int64 [G, T]: ``torch.argmax(F.linear(x, weights[i], biases[i]), dim=1)`` of every position, the first maximal column,
    without the logits."""
    weights, biases, _, _ = _head_args(x, weights, biases)
    if not token_head_supported(x, weights, biases) or x.contiguous().data_ptr() % 16:
        return torch.stack([torch.argmax(F.linear(x, w, b), dim=1) for w, b in zip(weights, biases)], dim=1)
    return head_forward(x.contiguous(), weights, biases, None, want_argmax=True)[2].to(torch.int64)


class TokenHead(nn.ModuleList):
    """``nn.ModuleList(nn.Linear(in_features, num_classes) for _ in range(seq_len))`` -- assigned to
    ``self.token_predictors`` it loads the reference's checkpoints with ``strict=True`` and hands an optimizer the same
    parameters -- with the fused training loss and prediction of the module docstring:

        forward(x)        the reference's list of seq_len logits tensors, through torch's Linear (compatibility)
        loss(x, y_arr)    the mean cross-entropy over rows and positions, under autograd
        predict(x)        int64 [G, seq_len] arg-max, no graph
    """

    def __init__(self, in_features: int, num_classes: int, seq_len: int):
        if int(in_features) < 1 or int(num_classes) < 1 or int(seq_len) < 1:
            raise ValueError(f"egc_amd: in_features, num_classes and seq_len must be positive (got {in_features}, {num_classes}, "
                             f"{seq_len})")
        super().__init__(nn.Linear(int(in_features), int(num_classes)) for _ in range(int(seq_len)))
        self.in_features, self.num_classes, self.seq_len = int(in_features), int(num_classes), int(seq_len)

    def _params(self):
        return [p.weight for p in self], [p.bias for p in self]

    def forward(self, x: torch.Tensor):
        return [p(x) for p in self]

    def loss(self, x: torch.Tensor, y_arr: torch.Tensor) -> torch.Tensor:
        return token_head_loss(x, *self._params(), y_arr)

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        return token_head_argmax(x, *self._params())
