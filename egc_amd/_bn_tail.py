"""The training-mode BatchNorm tail of a block, out = act(batch_norm(h)) + residual, under autograd (egc_tail.hip
through the C ABI), and the BatchNorm operands the compiled block nodes take."""
from __future__ import annotations

import torch

from . import _C
from ._args import _check_keep, _ptr, _row_parts
from ._dense import _column_sums
from .graph import _device_guard, _stream_ptr


def _f32_vec(t, c):
    """A [C] parameter / buffer the finalize kernels may read in place (float32, dense), else None."""
    return t is not None and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == c


class _BatchNormActResidualFunction(torch.autograd.Function):
    """out = act(batch_norm(h; batch statistics) * gamma + beta) + residual -- the training-mode tail of the
    reference's blocks (zinc/models.py:66-72) in two streaming passes each way plus ONE per-channel launch between them
    (egc_tail.hip), which also updates the module's running statistics when they are passed.  ``keep`` ([N, C] uint8,
    0 = dropped) with ``keep_scale`` = 1 / (1 - p) puts a dropout between the activation and the residual add, as the
    ogbn-arxiv net has it (arxiv/norm_models.py:34-40).  Returns (out, batch mean, biased batch variance), both float64."""

    @staticmethod
    def forward(ctx, h, residual, gamma, beta, eps, relu, running_mean, running_var, momentum, n_tracked, keep, keep_scale,
                n_valid, sync=None, res_link=None):
        lib = _C.load()
        n, c = h.shape
        dev = h.device
        ctx.res_link = res_link
        h = h.contiguous()
        gamma_c = gamma.detach().contiguous().float() if gamma is not None else None
        beta_c = beta.detach().contiguous().float() if beta is not None else None
        res = residual.contiguous() if residual is not None else None
        ctx.sync = sync
        with _device_guard(dev):
            n_parts = _row_parts(n)
            parts = torch.empty((n_parts, 2, c), dtype=torch.float64, device=dev)
            stats = torch.empty((3, c), dtype=torch.float64, device=dev)     # mean | biased variance | 1 / std
            affine = torch.empty((2, c), dtype=torch.float32, device=dev)    # scale | shift
            out = torch.empty_like(h)
            stream, nv_p, nt_p = _stream_ptr(dev), _ptr(n_valid), _ptr(n_tracked)
            # statistics pass (which also bumps num_batches_tracked) + the per-channel step: one call, and with a sync word
            # and few partial blocks one launch (egc_bn_forward_stats_f32)
            _C.check(lib.egc_bn_forward_stats_f32(
                h.data_ptr(), n, c, parts.data_ptr(), n_parts, nt_p if running_mean is not None else None, nv_p,
                _ptr(gamma_c), _ptr(beta_c), float(eps), stats.data_ptr(), affine.data_ptr(), _ptr(running_mean),
                _ptr(running_var), -1.0 if momentum is None else float(momentum), nt_p, _ptr(sync), stream),
                "egc_bn_forward_stats_f32")
            _C.check(lib.egc_affine_act_residual_f32(h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), _ptr(res),
                                                     int(relu), _ptr(keep), float(keep_scale), n, c, out.data_ptr(), nv_p,
                                                     stream), "egc_affine_act_residual_f32")
        ctx.save_for_backward(h, affine, stats, gamma_c, keep, n_valid)
        ctx.keep_scale = float(keep_scale)
        ctx.set_materialize_grads(False)     # (mean / var carry no gradient: no zero-filled stand-ins per backward)
        ctx.relu, ctx.has_res, ctx.has_gamma, ctx.has_beta = bool(relu), residual is not None, gamma is not None, beta is not None
        mean, var = stats[0], stats[1]
        ctx.mark_non_differentiable(mean, var)
        return out, mean, var

    @staticmethod
    def backward(ctx, dout, _dmean, _dvar):
        lib = _C.load()
        h, affine, stats, gamma_c, keep, n_valid = ctx.saved_tensors
        n, c = h.shape
        dev = h.device
        if dout is None:
            return (None,) * 15
        dout = dout.contiguous()
        dh = dgamma = dbeta = None
        if ctx.needs_input_grad[0] or (ctx.has_gamma and ctx.needs_input_grad[2]) or (ctx.has_beta and ctx.needs_input_grad[3]):
            masked = ctx.relu or keep is not None or n_valid is not None
            if not masked:
                s1 = _column_sums(dout).double()
                sgh = (dout.double() * h.double()).sum(0) if n else torch.zeros(c, dtype=torch.float64, device=dev)
                parts = torch.stack([s1, sgh]).unsqueeze(0).contiguous()
            with _device_guard(dev):
                out5 = torch.empty((5, c), dtype=torch.float32, device=dev)   # d gamma | d beta | coef_g | coef_h | coef_1
                stream, keep_p, nv_p = _stream_ptr(dev), _ptr(keep), _ptr(n_valid)
                if masked:      # sum g, sum g h (g = dout * dropout mask * relu mask) + the per-channel step: one call
                    n_parts = _row_parts(n)
                    parts = torch.empty((n_parts, 2, c), dtype=torch.float64, device=dev)
                    _C.check(lib.egc_bn_backward_stats_f32(
                        dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(), affine[1].data_ptr(), int(ctx.relu), keep_p,
                        ctx.keep_scale, n, c, parts.data_ptr(), n_parts, nv_p, stats.data_ptr(), _ptr(gamma_c), out5.data_ptr(),
                        _ptr(ctx.sync), stream), "egc_bn_backward_stats_f32")
                else:
                    _C.check(lib.egc_bn_backward_finalize(parts.data_ptr(), parts.size(0), c, n, stats.data_ptr(), _ptr(gamma_c),
                                                          out5.data_ptr(), nv_p, stream), "egc_bn_backward_finalize")
                dgamma = out5[0] if ctx.has_gamma and ctx.needs_input_grad[2] else None
                dbeta = out5[1] if ctx.has_beta and ctx.needs_input_grad[3] else None
                if ctx.needs_input_grad[0]:
                    dh = torch.empty_like(h)
                    _C.check(lib.egc_affine_act_backward_f32(dout.data_ptr(), h.data_ptr(), affine[0].data_ptr(),
                                                             affine[1].data_ptr(), int(ctx.relu), keep_p, ctx.keep_scale,
                                                             out5[2].data_ptr(), out5[3].data_ptr(), out5[4].data_ptr(), n, c,
                                                             dh.data_ptr(), nv_p, stream), "egc_affine_act_backward_f32")
        dres = dout if ctx.has_res and ctx.needs_input_grad[1] else None
        if dres is not None and ctx.res_link is not None:
            ctx.res_link.grad, dres = dres, None      # (joins d x inside the conv's backward launch: ResidualLink)
        return dh, dres, dgamma, dbeta, None, None, None, None, None, None, None, None, None, None, None


def batch_norm_act_residual_supported(h: torch.Tensor) -> bool:
    return (h.is_cuda and h.dtype == torch.float32 and h.dim() == 2 and h.size(0) > 1 and h.size(1) % 4 == 0
            and h.size(1) <= 1024)


def batch_norm_act_residual(h, residual, gamma, beta, eps: float, relu: bool, running_mean=None, running_var=None,
                            momentum=None, num_batches_tracked=None, keep=None, keep_scale: float = 1.0, n_valid=None,
                            sync=None, res_link=None):
    """Training-mode BatchNorm1d (batch statistics) -> optional ReLU -> optional residual add, fused
    (_BatchNormActResidualFunction): returns (out, batch mean [C] float64, biased batch variance [C] float64).
    With ``running_mean`` / ``running_var`` (float32 [C], dense) the running statistics are updated in the same launch
    that finishes the batch statistics, as nn.BatchNorm1d does: unbiased variance, ``momentum``, or -- momentum None --
    the cumulative average over ``num_batches_tracked`` (a device int64 scalar, INCREMENTED here when given).
    ``keep`` / ``keep_scale``: dropout between the activation and the residual add (see the Function).
    ``n_valid`` (device int64 scalar): only the first n_valid rows are real -- the rest is the padding of a batch brought
    to a recording's static shape; statistics and gradients are those of nn.BatchNorm1d on the real rows.
    ``sync`` (device int32 scalar, zero; the caller's for the lifetime of its module): lets the statistics pass and the
    per-channel step of small inputs be ONE launch each way (egc_bn_forward_stats_f32)."""
    c = h.size(1)
    if running_mean is not None and not (_f32_vec(running_mean, c) and _f32_vec(running_var, c)
                                         and (momentum is not None or num_batches_tracked is not None)):
        raise RuntimeError("egc_amd: running statistics must be dense float32 [C] tensors")
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or num_batches_tracked.numel() != 1
                                            or num_batches_tracked.device != h.device):
        raise RuntimeError("egc_amd: num_batches_tracked must be an int64 scalar on the device of h")
    _check_keep(keep, h.size(0), c, h.device, "h")
    if n_valid is not None and (n_valid.dtype != torch.int64 or n_valid.numel() != 1 or n_valid.device != h.device):
        raise RuntimeError("egc_amd: n_valid must be an int64 scalar on the device of h")
    return _BatchNormActResidualFunction.apply(h, residual, gamma, beta, float(eps), bool(relu), running_mean, running_var,
                                               momentum, num_batches_tracked, keep, float(keep_scale), n_valid, sync, res_link)


def _bn_tail_operands(spec, bn, residual):
    """The BatchNorm operands of a block node's tail -- (gamma, beta, running_mean, running_var, num_batches_tracked, eps,
    momentum) -- or None when the BatchNorm is outside the node's envelope.  The tail reads bn.weight / bn.bias as [f_out] and
    adds x as an [N, f_out] residual: a module of other widths is declined (the Python route then raises torch's own shape
    error, as the unfused composition does)."""
    if not (bn.training and bn.affine and spec.f_out % 4 == 0 and spec.f_out <= 1024) or (residual and spec.f_in != spec.f_out):
        return None
    gamma, beta = bn.weight, bn.bias
    if any(t is None or t.numel() != spec.f_out or not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous())
           for t in (gamma, beta)):
        return None
    rm = rv = nt = None
    if bn.track_running_stats:
        rm, rv, nt = bn.running_mean, bn.running_var, bn.num_batches_tracked
        if not (_f32_vec(rm, spec.f_out) and _f32_vec(rv, spec.f_out) and rm.is_cuda and nt is not None and nt.dtype == torch.int64
                and nt.is_cuda):
            return None
    return gamma, beta, rm, rv, nt, float(bn.eps), -1.0 if bn.momentum is None else float(bn.momentum)
