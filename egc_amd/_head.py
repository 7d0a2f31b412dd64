"""The graph-level MLP head of the reference's batched nets (egc_head.hip through the C ABI), fused with its loss.

Every batched net of the reference ends ``pool -> mlp([h, h // 2, h // 4, out]) -> loss`` with ``experiments.utils.mlp``
(utils.py:30-40: Linear -> BatchNorm1d -> act -> Dropout per hidden layer, then a Linear) and ``F.l1_loss``
(zinc/configs.py:48-50), ``F.binary_cross_entropy_with_logits`` over the labelled entries (mol/configs.py:64-68) or
``F.cross_entropy`` (cifar/configs.py:57).  ``GraphHead`` is that ``nn.Sequential`` -- the same children, state-dict keys,
parameter order and ``repr`` -- whose ``forward`` / ``l1_loss`` / ``bce_with_logits_loss`` / ``predict`` run on the kernels:
one launch per Linear forward in training (one in all in evaluation), one row pass per Linear and one parameter-gradient
launch backward (include/egc_hip.h).  CPU tensors, dtypes other than float32, an activation other than ReLU, dropout > 0 in
training and shapes outside the envelope (a width > 384, more than 64 outputs, more than 3 hidden layers, more than 65,536
rows) take torch's operators, as ``_softmax.py`` does.  Nothing reads back from the device: every call records inside
``GraphedStep``.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C
from ._args import _ptr, _workspace
from .graph import _device_guard, _stream_ptr

LOSS_NONE, LOSS_L1, LOSS_BCE = _C.HEAD_LOSS_NONE, _C.HEAD_LOSS_L1, _C.HEAD_LOSS_BCE_MASKED


def _masked_bce_reference(out, y):
    y = y.view_as(out)
    labelled = y == y
    return F.binary_cross_entropy_with_logits(out[labelled], y[labelled])


def _l1_reference(out, y):
    return F.l1_loss(out, y.view_as(out))


_REFERENCE_LOSS = {LOSS_L1: _l1_reference, LOSS_BCE: _masked_bce_reference}


def _loss_supported(out, y):
    return (out.is_cuda and out.dtype == torch.float32 and y.dtype == torch.float32 and y.device == out.device
            and out.numel() <= _C.HEAD_MAX_ROWS * _C.HEAD_MAX_OUT)


class _LossFunction(torch.autograd.Function):
    """One of the two losses alone on out [G, OUT]: one launch forward, one backward."""

    @staticmethod
    def forward(ctx, out, y, kind):
        lib = _C.load()
        fwd = lib.egc_l1_loss_forward_f32 if kind == LOSS_L1 else lib.egc_bce_masked_forward_f32
        with _device_guard(out.device):
            loss2 = torch.empty(2, dtype=torch.float32, device=out.device)
            _C.check(fwd(out.data_ptr(), y.data_ptr(), out.numel(), loss2.data_ptr(), _stream_ptr(out.device)), "the loss forward")
        ctx.kind = kind
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(out, y, loss2)
        return loss2[0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, d_loss):
        if d_loss is None or not ctx.needs_input_grad[0]:
            return None, None, None
        out, y, loss2 = ctx.saved_tensors
        lib = _C.load()
        bwd = lib.egc_l1_loss_backward_f32 if ctx.kind == LOSS_L1 else lib.egc_bce_masked_backward_f32
        d_loss = d_loss.to(torch.float32).contiguous()
        with _device_guard(out.device):
            d_out = torch.empty_like(out)
            _C.check(bwd(out.data_ptr(), y.data_ptr(), d_loss.data_ptr(), loss2.data_ptr(), out.numel(), d_out.data_ptr(),
                         _stream_ptr(out.device)), "the loss backward")
        return d_out, None, None


def _loss(out, y, kind):
    if not isinstance(out, torch.Tensor) or not isinstance(y, torch.Tensor) or y.numel() != out.numel():
        raise ValueError("egc_amd: the loss takes an output tensor and as many targets")
    if not _loss_supported(out, y):
        return _REFERENCE_LOSS[kind](out, y)
    return _LossFunction.apply(out.contiguous(), y.contiguous().view_as(out), kind)


def l1_loss(out: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``F.l1_loss(out, y.view_as(out))`` (zinc/configs.py:48-50), differentiable with respect to out: the terms are added in
    float64 in a fixed order and the mean rounded once; d out = sign(out - y) / numel, sign(0) = 0."""
    return _loss(out, y, LOSS_L1)


def masked_bce_with_logits(out: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """``F.binary_cross_entropy_with_logits(out[y == y], y[y == y])`` (mol/configs.py:64-68) without the selection: a NaN
    target adds nothing and has a zero gradient, the divisor is the labelled count taken on the device, no labelled entry
    gives NaN.  Differentiable with respect to out."""
    return _loss(out, y, LOSS_BCE)


class _HeadFunction(torch.autograd.Function):
    """The whole head in training mode, with or without a fused loss: (out) or (loss)."""

    @staticmethod
    def forward(ctx, head, x, y, kind, *params):
        st = head._launch_train(x, y, kind)
        ctx.head, ctx.kind, ctx.n_hidden = head, kind, len(st["z"])
        ctx.set_materialize_grads(False)
        # (every tensor through save_for_backward: ``out`` is this node's own output, and a node that holds its output in an
        # attribute is a reference cycle that keeps the whole autograd graph of the step alive)
        ctx.save_for_backward(x, y, st["out"], st["loss2"], *st["z"], *st["stats"], *st["affine"])
        return st["out"] if kind == LOSS_NONE else st["loss2"][0]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        n_params = len(ctx.needs_input_grad) - 4
        if grad is None:
            return (None,) * (4 + n_params)
        x, y, out, loss2, *rest = ctx.saved_tensors
        h = ctx.n_hidden
        st = {"out": out, "loss2": loss2, "z": rest[:h], "stats": rest[h:2 * h], "affine": rest[2 * h:3 * h]}
        need = ctx.needs_input_grad
        dx, grads = ctx.head._launch_backward(st, x, y, ctx.kind, grad, need[1], any(need[4:]))
        return (None, dx, None, None, *[g if n else None for g, n in zip(grads, need[4:])])


def _head_workspace(lib, d, g, dev):
    return _workspace(lib.egc_head_workspace_bytes(C.byref(d), g), dev, "egc_amd: the head's kernels do not take this shape")


class GraphHead(nn.Sequential):
    """``experiments.utils.mlp(sizes, act, dropout)``: the same children (``mlp.*`` state dicts of the reference load with
    ``strict=True``; parameter order and ``repr`` match), on the head kernels:

        forward(x)                    out [G, sizes[-1]]
        l1_loss(x, y)                 F.l1_loss(forward(x), y.view_as(out)), the loss fused into the last launch
        bce_with_logits_loss(x, y)    the BCE-with-logits mean over the entries whose target is not NaN, fused alike
        predict(x)                    the evaluation-mode forward under no_grad, whatever the module's mode: one launch
    """

    def __init__(self, sizes, act=nn.ReLU, dropout: float = 0.0):
        sizes = [int(s) for s in sizes]
        if len(sizes) < 2 or min(sizes) < 1:
            raise ValueError(f"egc_amd: GraphHead needs at least [in, out] positive widths (got {sizes})")
        modules = []
        for a, b in zip(sizes[:-2], sizes[1:-1]):
            modules += [nn.Linear(a, b), nn.BatchNorm1d(b), act(), nn.Dropout(dropout)]
        modules.append(nn.Linear(sizes[-2], sizes[-1]))
        super().__init__(*modules)
        # (plain attributes: nothing here may show in the state dict or the repr)
        self.__dict__["sizes"] = sizes
        self.__dict__["_relu"] = act is nn.ReLU
        self.__dict__["_dropout"] = float(dropout)
        self.__dict__["_sync"] = {}

    def _get_name(self):
        return "Sequential"   # the reference's repr: the head IS its nn.Sequential

    # ---- which path ----------------------------------------------------------------------------------------------------
    def _linears(self):
        return [m for m in self if isinstance(m, nn.Linear)]

    def _norms(self):
        return [m for m in self if isinstance(m, nn.BatchNorm1d)]

    def _params(self):
        ps = []
        for m in self._linears():
            ps += [m.weight, m.bias]
        for m in self._norms():
            ps += [p for p in (m.weight, m.bias) if p is not None]
        return ps

    def _supported(self, x, training: bool) -> bool:
        s = self.sizes
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.size(1) == s[0]):
            return False
        if not self._relu or (training and self._dropout > 0.0):
            return False
        if (len(s) - 1 > _C.HEAD_MAX_LINEARS or max(s[:-1]) > _C.HEAD_MAX_WIDTH or s[-1] > _C.HEAD_MAX_OUT
                or x.size(0) > _C.HEAD_MAX_ROWS):
            return False
        for m in self._linears():
            if m.bias is None or any(p.device != x.device or p.dtype != torch.float32 or not p.is_contiguous()
                                     for p in (m.weight, m.bias)):
                return False
        for m in self._norms():
            for t in (m.weight, m.bias, m.running_mean, m.running_var):
                if t is not None and (t.device != x.device or t.dtype != torch.float32 or not t.is_contiguous()):
                    return False
            if (m.weight is None) != (m.bias is None):
                return False
        return True

    def _batch_statistics(self) -> bool:
        """nn.BatchNorm1d uses the batch's statistics in training mode and wherever it keeps no running ones."""
        return self.training or any(m.running_mean is None for m in self._norms())

    # ---- marshalling ----------------------------------------------------------------------------------------------------
    def _descriptor(self, update_running: bool):
        s = self.sizes
        d = _C.EgcHead()
        d.n_linears = len(s) - 1
        for i, v in enumerate(s):
            d.sizes[i] = v
        for i, m in enumerate(self._linears()):
            d.weight[i], d.bias[i] = m.weight.data_ptr(), m.bias.data_ptr()
        for i, m in enumerate(self._norms()):
            d.gamma[i], d.beta[i] = _ptr(m.weight), _ptr(m.bias)
            d.eps[i] = float(m.eps)
            d.momentum[i] = -1.0 if m.momentum is None else float(m.momentum)
            if update_running and m.running_mean is not None:
                d.running_mean[i], d.running_var[i] = m.running_mean.data_ptr(), m.running_var.data_ptr()
                d.num_batches_tracked[i] = _ptr(m.num_batches_tracked)
        return d

    def _sync_word(self, dev):
        """The arrival counter of the launches: zero between them; the module's for its lifetime.  One made while a stream
        capture is under way belongs to that capture's memory pool, so it is not kept."""
        w = self._sync.get(dev)
        if w is None:
            w = torch.zeros(1, dtype=torch.int32, device=dev)
            if not torch.cuda.is_current_stream_capturing():
                self._sync[dev] = w
        return w

    def _launch_train(self, x, y, kind):
        """The training forward: L launches.  Returns what the backward needs."""
        lib = _C.load()
        s, g, dev = self.sizes, x.size(0), x.device
        d = self._descriptor(update_running=self.training)
        with _device_guard(dev):
            st = {"z": [torch.empty((g, w), dtype=torch.float32, device=dev) for w in s[1:-1]],
                  "stats": [torch.empty((3, w), dtype=torch.float64, device=dev) for w in s[1:-1]],
                  "affine": [torch.empty((2, w), dtype=torch.float32, device=dev) for w in s[1:-1]],
                  "out": torch.empty((g, s[-1]), dtype=torch.float32, device=dev),
                  "loss2": torch.empty(2, dtype=torch.float32, device=dev) if kind != LOSS_NONE else None}
            for i in range(len(s) - 2):
                d.z[i], d.stats[i], d.affine[i] = st["z"][i].data_ptr(), st["stats"][i].data_ptr(), st["affine"][i].data_ptr()
            ws, nbytes = _head_workspace(lib, d, g, dev)
            _C.check(lib.egc_head_forward_train_f32(C.byref(d), x.data_ptr(), g, kind, _ptr(y), st["out"].data_ptr(),
                                                    _ptr(st["loss2"]), ws.data_ptr(), nbytes, self._sync_word(dev).data_ptr(),
                                                    _stream_ptr(dev)), "egc_head_forward_train_f32")
        return st

    def _launch_backward(self, st, x, y, kind, grad, want_dx, want_params):
        """(d x or None, the gradients in _params() order): L row passes and one parameter-gradient launch."""
        lib = _C.load()
        s, g, dev = self.sizes, x.size(0), x.device
        n_lin = len(s) - 1
        d = self._descriptor(update_running=False)
        grad = grad.to(torch.float32).contiguous()
        with _device_guard(dev):
            dz = [torch.empty((g, w), dtype=torch.float32, device=dev) for w in s[1:-1]]
            dz.append(torch.empty((g, s[-1]), dtype=torch.float32, device=dev) if kind != LOSS_NONE else None)
            gs = [torch.empty((g, w), dtype=torch.float32, device=dev) for w in s[1:-1]]
            coef = [torch.empty((5, w), dtype=torch.float32, device=dev) for w in s[1:-1]]
            dx = torch.empty_like(x) if want_dx else None
            dw = [torch.empty_like(m.weight) for m in self._linears()] if want_params else []
            db = [torch.empty_like(m.bias) for m in self._linears()] if want_params else []
            for i in range(n_lin - 1):
                d.z[i], d.stats[i], d.affine[i] = st["z"][i].data_ptr(), st["stats"][i].data_ptr(), st["affine"][i].data_ptr()
                d.coef[i], d.g[i] = coef[i].data_ptr(), gs[i].data_ptr()
            for i in range(n_lin):
                d.dz[i] = _ptr(dz[i])
                if want_params:
                    d.d_weight[i], d.d_bias[i] = dw[i].data_ptr(), db[i].data_ptr()
            ws, nbytes = _head_workspace(lib, d, g, dev)
            _C.check(lib.egc_head_backward_f32(C.byref(d), x.data_ptr(), g, kind, _ptr(y), st["out"].data_ptr(), _ptr(st["loss2"]),
                                               grad.data_ptr(), _ptr(dx), int(want_params), ws.data_ptr(), nbytes,
                                               self._sync_word(dev).data_ptr(), _stream_ptr(dev)), "egc_head_backward_f32")
        st["dz"], st["coef"], st["g"] = dz, coef, gs           # (kept for the tests' stage-by-stage comparison)
        grads = []
        if want_params:
            for w, b in zip(dw, db):
                grads += [w, b]
            for i, m in enumerate(self._norms()):
                if m.weight is not None:
                    grads += [coef[i][0], coef[i][1]]
        else:
            grads = [None] * len(self._params())
        return dx, grads

    def _launch_eval(self, x):
        lib = _C.load()
        g, dev = x.size(0), x.device
        d = self._descriptor(update_running=True)
        with _device_guard(dev):
            out = torch.empty((g, self.sizes[-1]), dtype=torch.float32, device=dev)
            _C.check(lib.egc_head_forward_eval_f32(C.byref(d), x.data_ptr(), g, out.data_ptr(), _stream_ptr(dev)),
                     "egc_head_forward_eval_f32")
        return out

    # ---- the public calls ------------------------------------------------------------------------------------------------
    def _check_rows(self, x):
        if len(self.sizes) > 2 and x.size(0) < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        if x.size(0) < 1:
            raise ValueError("egc_amd: the head's training forward needs at least one row")

    def _run(self, x, y, kind):
        """out (LOSS_NONE) or the scalar loss of the module's current mode."""
        if y is not None and (not isinstance(y, torch.Tensor) or y.numel() != x.size(0) * self.sizes[-1]):
            raise ValueError(f"egc_amd: y must hold one target per output, {x.size(0)} x {self.sizes[-1]} "
                             f"(got {tuple(y.shape) if isinstance(y, torch.Tensor) else type(y).__name__})")
        ok = self._supported(x, self.training) and (y is None or (y.dtype == torch.float32 and y.device == x.device))
        if not ok:
            out = nn.Sequential.forward(self, x)
            return out if kind == LOSS_NONE else _REFERENCE_LOSS[kind](out, y)
        x = x.contiguous()
        y = y.contiguous().view(x.size(0), self.sizes[-1]) if y is not None else None
        if not self._batch_statistics():
            out = self._launch_eval(x.detach()) if not (torch.is_grad_enabled() and self._any_grad(x)) else None
            if out is None:   # gradients through running statistics: torch's operators (no reference net does this)
                out = nn.Sequential.forward(self, x)
            return out if kind == LOSS_NONE else _loss(out, y, kind)
        self._check_rows(x)
        params = self._params()
        if torch.is_grad_enabled() and self._any_grad(x):
            return _HeadFunction.apply(self, x, y, kind, *params)
        st = self._launch_train(x.detach(), y, kind)
        return st["out"] if kind == LOSS_NONE else st["loss2"][0]

    def _any_grad(self, x):
        return x.requires_grad or any(p.requires_grad for p in self._params())

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self._run(x, None, LOSS_NONE)

    def l1_loss(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return self._run(x, y, LOSS_L1)

    def bce_with_logits_loss(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        return self._run(x, y, LOSS_BCE)

    @torch.no_grad()
    def predict(self, x: torch.Tensor) -> torch.Tensor:
        if self._supported(x, False) and all(m.running_mean is not None for m in self._norms()):
            return self._launch_eval(x.contiguous())
        was = self.training
        self.eval()
        try:
            return nn.Sequential.forward(self, x)
        finally:
            self.train(was)
