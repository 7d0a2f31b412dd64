"""The dense side of a layer's training step: the parameter pack / unpack (egc_weights_pack_f32) and the gradient GEMMs
and column sums of the backward (x^T d_cat, d_cat W^T, bias sums)."""
from __future__ import annotations

import ctypes as C

import torch

from . import _C
from ._args import _ptr, _row_parts
from .graph import _device_guard, _stream_ptr


def gemm_exact() -> bool:
    """EGC_GEMM_EXACT=1 selects the plain fp32-MFMA GEMM instead of the split-precision matrix-core form."""
    return _C.env_flag("EGC_GEMM_EXACT")


def _dims(f_in, H, A, B, L, Ls):
    """The (f_in, H, A, B, L, Ls) tuple the pack's entry points and the parameter Functions carry, as plain ints."""
    return (int(f_in), int(H), int(A), int(B), int(L), int(Ls))


def _pack_params(dims, permute, comb_w, comb_b, bases):
    """(wcat [f_in, B Ls + H B A], bcat [H B A] or None) from the parameters: one launch (egc_weights_pack_f32)."""
    lib = _C.load()
    f_in, H, A, B, L, Ls = dims
    dev = comb_w.device
    parts = [b.contiguous() for b in bases]
    cw = comb_w.contiguous()
    cb = comb_b.contiguous() if comb_b is not None else None
    ptrs = (C.c_void_p * len(parts))(*[p.data_ptr() for p in parts])
    with _device_guard(dev):
        wcat = torch.empty((f_in, B * Ls + H * B * A), dtype=torch.float32, device=dev)
        bcat = torch.empty(H * B * A, dtype=torch.float32, device=dev) if cb is not None else None
        _C.check(lib.egc_weights_pack_f32(ptrs, len(parts), cw.data_ptr(), _ptr(cb), f_in, H, A, B, L, Ls, int(permute),
                                          wcat.data_ptr(), _ptr(bcat), 0, _stream_ptr(dev)), "egc_weights_pack_f32")
    return wcat, bcat


def _unpack_param_grads(dims, permute, shapes, has_b, dwcat, dbcat):
    """The parameters' gradients (d comb_w, d comb_b or None, [d basis matrices]) from (d wcat, d bcat): the same index
    map read the other way, one launch."""
    lib = _C.load()
    f_in, H, A, B, L, Ls = dims
    dev = dwcat.device if dwcat is not None else dbcat.device
    with _device_guard(dev):
        if dwcat is None:
            dwcat = torch.zeros((f_in, B * Ls + H * B * A), dtype=torch.float32, device=dev)
        dwcat = dwcat.contiguous()
        dcw = torch.empty(shapes[0], dtype=torch.float32, device=dev)
        dcb = dbc = None
        if has_b:
            dbc = (dbcat if dbcat is not None else torch.zeros(H * B * A, dtype=torch.float32, device=dev)).contiguous()
            dcb = torch.empty(shapes[1], dtype=torch.float32, device=dev)
        dparts = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes[2]]
        ptrs = (C.c_void_p * len(dparts))(*[p.data_ptr() for p in dparts])
        _C.check(lib.egc_weights_pack_f32(ptrs, len(dparts), dcw.data_ptr(), _ptr(dcb), f_in, H, A, B, L, Ls, int(permute),
                                          dwcat.data_ptr(), _ptr(dbc), 1, _stream_ptr(dev)), "egc_weights_pack_f32")
    return dcw, dcb, dparts


class _PackWeightsFunction(torch.autograd.Function):
    """(wcat, bcat) = the GEMM operand of a layer from its parameters, and the parameters' gradients from (d wcat,
    d bcat): one launch each way (egc_weights_pack_f32) instead of the cat / pad / permute / transpose chain and its
    autograd mirror -- seven or more launches of 5 us per training step.  Inputs: dims, permute flag, comb weight,
    comb bias (or None), then the basis matrices (one [F_in, B L] or B of [F_in, L])."""

    @staticmethod
    def forward(ctx, dims, permute, comb_w, comb_b, *bases):
        wcat, bcat = _pack_params(dims, permute, comb_w, comb_b, bases)
        ctx.dims, ctx.permute, ctx.has_b = dims, permute, comb_b is not None
        ctx.shapes = (comb_w.shape, comb_b.shape if comb_b is not None else None, [b.shape for b in bases])
        if bcat is None:
            bcat = wcat.new_empty(0)
            ctx.mark_non_differentiable(bcat)
        return wcat, bcat

    @staticmethod
    def backward(ctx, dwcat, dbcat):
        dcw, dcb, dparts = _unpack_param_grads(ctx.dims, ctx.permute, ctx.shapes, ctx.has_b, dwcat, dbcat)
        return (None, None, dcw, dcb, *dparts)


def pack_layer_weights(bases, comb_w, comb_b, f_in, H, A, B, L, Ls, permute_hab: bool):
    """Differentiable (wcat [f_in, B Ls + H B A], bcat [H B A] or None) on the device kernel; ``bases`` is a list of one
    [f_in, B L] matrix or of B [f_in, L] matrices (float32 CUDA parameters)."""
    wcat, bcat = _PackWeightsFunction.apply(_dims(f_in, H, A, B, L, Ls), bool(permute_hab), comb_w, comb_b, *bases)
    return wcat, (bcat if comb_b is not None else None)


def third_stream_rides(f_in: int, k: int, e_cols: int) -> bool:
    """Whether an [N, e_cols] array's column sums ride along with the [f_in, k] weight gradient: in the one-tile kernel only
    (include/egc_hip.h; the fp32-MFMA form of EGC_GEMM_EXACT has no third stream either: the caller asks gemm_exact())."""
    return f_in <= _C.WEIGHT_GRAD_TILE_ROWS and k <= _C.WEIGHT_GRAD_TILE_COLS and e_cols <= _C.WEIGHT_GRAD_MAX_SUM_COLS


def _xt_operands(n, *operands) -> bool:
    """Whether every operand is an [n, multiple of 4] matrix as the weight-gradient entry points take it: float32 on the device,
    n > 0, unit column stride, row stride a multiple of 4, 16-byte aligned."""
    return n > 0 and all(t.dim() == 2 and t.size(0) == n and t.size(1) % 4 == 0 and t.is_cuda and t.dtype == torch.float32
                         and t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in operands)


def _xt_workspace(lib, n, f_in, k, e_cols, dev):
    return torch.empty(max(int(lib.egc_weight_grad_ex_workspace_bytes(n, f_in, k, e_cols)), 16), dtype=torch.uint8, device=dev)


def _weight_grads(x: torch.Tensor, d: torch.Tensor, col_sums: bool = False, extra: torch.Tensor | None = None):
    """(x^T @ d, d.sum(0) or None[, extra.sum(0)]) for tall x [N, F], d [N, K]: the gradient of [bases_weight |
    comb_weights.weight], of comb_weights.bias and -- with ``extra`` = grad_out -- of the layer's bias (autograd's
    products behind optimized_layers.py:177-178,207-208) in one pass over the operands through egc_weight_grad_ex_f32:
    split-bf16 matrix-core products with fp32-level accuracy over row ranges (outputs of one accumulator tile) or exact fp32
    products on a grid of output tiles (wider ones), added in a fixed order.  Shapes outside that entry point's envelope
    (a dimension not a multiple of 4) take torch's GEMM on the device.  (Rounds 2 - 5 also sent wide outputs on long
    reductions there; with the tall tiles and the per-XCD row split of round 6 the entry point is level with the library's
    split GEMM at the ogbn-mag widths -- 1.26 against 1.32 ms at 736 k x 352 x 208 -- and ahead below them, so one
    deterministic path serves every width.)  Returns a pair without ``extra``, a triple with it."""
    n, f = x.shape
    k = d.size(1)

    def done(w, s, e):
        return (w, s) if extra is None else (w, s, e)
    if not _xt_operands(n, x, d):
        return done(_xt_library(x, d), _column_sums(d) if col_sums else None, _column_sums(extra) if extra is not None else None)
    lib = _C.load()
    dev = x.device
    ride = extra is not None and col_sums and _xt_operands(n, extra) and third_stream_rides(f, k, extra.size(1)) and not gemm_exact()
    with _device_guard(dev):
        out = torch.empty((f, k), dtype=torch.float32, device=dev)
        cs = torch.empty(k, dtype=torch.float32, device=dev) if col_sums else None
        e_cols = extra.size(1) if ride else 0
        es = torch.empty(e_cols, dtype=torch.float32, device=dev) if ride else None
        ws = _xt_workspace(lib, n, f, k, e_cols, dev)
        _C.check(lib.egc_weight_grad_ex_f32(x.data_ptr(), x.stride(0), d.data_ptr(), d.stride(0), n, f, k, out.data_ptr(), _ptr(cs),
                                            extra.data_ptr() if ride else None, extra.stride(0) if ride else 0, e_cols, _ptr(es),
                                            ws.data_ptr(), ws.numel(), _stream_ptr(dev)), "egc_weight_grad_ex_f32")
    if extra is not None and not ride:
        es = _column_sums(extra)
    return done(out, cs, es)


def _weight_grads_into_params(x, d, extra, dims, permute, shapes, packed_b):
    """x^T @ d, the column sums of d's weightings part and of ``extra`` (= grad_out) written STRAIGHT into gradients of the
    module's own parameters through the pack's index map (egc_weight_grad_params_f32: no d wcat array, no unpack launch), or None
    when the call is outside that entry point's envelope.  Returns (d comb_w, d comb_b or None, d bcat or None, [d basis parts],
    d bias)."""
    f_in, H, A, B, L, Ls = dims
    n, k = x.size(0), d.size(1)
    if (not _xt_operands(n, x, d, extra) or not third_stream_rides(f_in, k, extra.size(1)) or gemm_exact()
            or x.size(1) != f_in or k != B * Ls + H * B * A):
        return None
    lib = _C.load()
    dev = x.device
    with _device_guard(dev):
        dcw = torch.empty(shapes[0], dtype=torch.float32, device=dev)
        dcb = torch.empty(shapes[1], dtype=torch.float32, device=dev) if packed_b else None
        dbc = None if packed_b else torch.empty(H * B * A, dtype=torch.float32, device=dev)
        dparts = [torch.empty(sh, dtype=torch.float32, device=dev) for sh in shapes[2]]
        ptrs = (C.c_void_p * len(dparts))(*[p.data_ptr() for p in dparts])
        e_cols = extra.size(1)
        es = torch.empty(e_cols, dtype=torch.float32, device=dev)
        ws = _xt_workspace(lib, n, f_in, k, e_cols, dev)
        _C.check(lib.egc_weight_grad_params_f32(x.data_ptr(), x.stride(0), d.data_ptr(), d.stride(0), n, f_in, H, A, B, L, Ls,
                                                int(permute), ptrs, len(dparts), dcw.data_ptr(), _ptr(dcb), _ptr(dbc), extra.data_ptr(),
                                                extra.stride(0), e_cols, es.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr(dev)),
                 "egc_weight_grad_params_f32")
    return dcw, dcb, dbc, dparts, es


def _xt_library(x: torch.Tensor, d: torch.Tensor) -> torch.Tensor:
    """x^T @ d on the library GEMM: as one product rocBLAS runs a single tile grid over the tiny output (397 us at
    N = 169k); split into 64 row ranges + a sum it takes 96 us."""
    n = x.size(0)
    splits = 64
    if n < 64 * splits:
        return x.t() @ d
    m = (n // splits) * splits
    out = torch.bmm(x[:m].view(splits, m // splits, -1).transpose(1, 2), d[:m].view(splits, m // splits, -1)).sum(0)
    if m < n:
        out = out + x[m:].t() @ d[m:]
    return out


def _column_sums(t: torch.Tensor) -> torch.Tensor:
    """t.sum(0) for a float32 matrix (or a column block of one) through egc_column_sums_f32: one pass at the
    memory rate instead of torch's generic reduction (26 us per 87 MB operand at config 2)."""
    n, c = t.shape
    if (not t.is_cuda or t.dtype != torch.float32 or t.stride(1) != 1 or c % 4 or c > 1024 or n == 0
            or (n > 1 and t.stride(0) % 4) or t.data_ptr() % 16):
        return t.sum(0)
    lib = _C.load()
    dev = t.device
    with _device_guard(dev):
        parts = _row_parts(n)     # partial rows: one workgroup each, then a small torch sum
        out = torch.empty((parts, c), dtype=torch.float32, device=dev)
        _C.check(lib.egc_column_sums_f32(t.data_ptr(), n, int(t.stride(0)) if n > 1 else c, c, out.data_ptr(), parts,
                                         _stream_ptr(dev)), "egc_column_sums_f32")
        if parts == 1:
            return out[0]
        total = torch.empty(c, dtype=torch.float32, device=dev)
        _C.check(lib.egc_sum_partials_f32(out.data_ptr(), parts, c, total.data_ptr(), _stream_ptr(dev)), "egc_sum_partials_f32")
    return total


def _dx_matmul(d_cat: torch.Tensor, wcat: torch.Tensor) -> torch.Tensor:
    """d_cat [N, F_g + W] @ wcat^T [F_g + W, F_in] (the gradient w.r.t. x) on the split-precision matrix-core GEMM
    of the forward (egc_basis_pack / egc_basis_transform_packed with no weightings block): 95 us instead of the
    128 us of the fp32 library GEMM at config 2, 44 instead of 79 for an EGC-S layer; same fp32-level accuracy."""
    f_in, k = wcat.size(0), wcat.size(1)
    n = d_cat.size(0)
    if (gemm_exact() or f_in % 4 != 0 or k % 4 != 0 or n == 0 or not d_cat.is_cuda or not d_cat.is_contiguous()
            or d_cat.data_ptr() % 16):      # (rows of d_cat must be 16-byte aligned for the split-precision kernels)
        return d_cat @ wcat.t()
    lib = _C.load()
    dev = d_cat.device
    with _device_guard(dev):
        w = wcat.detach().contiguous()          # [f_in, k]: the transpose of this GEMM's operand, packed where it lies
        nbytes = lib.egc_basis_pack_bytes(k, f_in, 0)
        packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        dx = torch.empty((n, f_in), dtype=torch.float32, device=dev)
        stream = _stream_ptr(dev)
        _C.check(lib.egc_basis_pack_transposed(w.data_ptr(), k, k, f_in, 0, packed.data_ptr(), nbytes, stream),
                 "egc_basis_pack_transposed")
        _C.check(lib.egc_basis_transform_packed(d_cat.data_ptr(), packed.data_ptr(), None, n, k, f_in, 0, dx.data_ptr(),
                                                f_in, None, stream), "egc_basis_transform_packed")
    return dx


def _dense_param_grads(x, d_cat, d_w, grad_out, spec, need_w, need_b, need_bias):
    """(d wcat, d bcat, d bias) from x, the joint gradient d_cat [N, ldb + W] and grad_out; what is not needed is None.  Both
    bias sums ride along with x^T d_cat where they can.  ``d_w``: d_cat's weightings part as the caller holds it, summed when
    the comb bias alone takes a gradient; None (the one-launch backward): a dense copy of that column block."""
    dwcat = dbcat = dbias = None
    if need_w:
        if need_bias and need_b:
            dwcat, sums, dbias = _weight_grads(x, d_cat, col_sums=True, extra=grad_out)
        else:
            dwcat, sums = _weight_grads(x, d_cat, col_sums=need_b)
        dbcat = sums[d_cat.size(1) - spec.w_cols:] if need_b else None
    elif need_b:
        dbcat = _column_sums(d_w if d_w is not None else d_cat[:, spec.ldb:].contiguous())
    if need_bias and dbias is None:
        dbias = _column_sums(grad_out)
    return dwcat, dbcat, dbias
