"""Typed mean aggregation on the device: the sparse part of the relational baseline layer (egc_typed_mean.hip through
the C ABI) -- one launch per node type over all its relations, forward and backward -- and its autograd form, the
"concatenated typed mean" that ``relational.RGCNConv`` multiplies with its concatenated weights."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import torch

from . import _C
from ._args import _check_f32, _ptr, _workspace
from .graph import CSRGraph, _device_guard, _stream_ptr


class TypedRel(NamedTuple):
    """One relation of a typed-mean launch (``egc_typed_rel``).  ``graph``: the CSR whose rows are the launch's rows, or
    None for the identity relation (row i has the one entry i).  ``inp`` [rows the entries name, >= in_col + width]
    float32 with unit column stride; the relation reads its columns in_col .. in_col + width.  ``pre_rowptr``: None, or
    the int32 rowptr whose row lengths scale the entries (1 / length of row col[p]).  ``post_mean``: divide the row's
    sum by its entry count.  ``out_col``: first column of the relation's block of the output (non-accumulating form)."""
    graph: CSRGraph | None
    inp: torch.Tensor
    in_col: int = 0
    pre_rowptr: torch.Tensor | None = None
    post_mean: bool = False
    out_col: int = 0


def typed_mean_chunk() -> int:
    """Entries per chunk of the documented summation order (EGC_TYPED_MEAN_CHUNK, asked of the library)."""
    return int(_C.load().egc_typed_mean_chunk())


def typed_mean(rels, n_rows: int, width: int, out: torch.Tensor, accumulate: bool = False) -> torch.Tensor:
    """egc_typed_mean_f32: out[row, block(r)] (+)= post * sum over the row's entries of pre * inp[col, in_col : in_col +
    width] for every relation of ``rels`` in ONE call (two launches when a relation has more entries than one chunk).
    ``accumulate`` False: every relation writes out[:, out_col : out_col + width]; True: the relations' terms are added in
    list order into out[:, :width].  Every element named is written exactly once; nothing is read back.  A row's float32
    sum follows the chunked order of include/egc_hip.h (tests/rgcn_ref.py restates it)."""
    lib = _C.load()
    rels = list(rels)
    if len(rels) > _C.TYPED_MAX_RELATIONS:
        raise RuntimeError(f"egc_amd: a typed-mean launch takes at most {_C.TYPED_MAX_RELATIONS} relations (got {len(rels)})")
    _check_f32(out, "out")
    n_rows, width = int(n_rows), int(width)
    if out.dim() != 2 or out.size(0) != n_rows or out.stride(1) != 1 and out.numel() > 0:
        raise RuntimeError(f"egc_amd: out must be [{n_rows}, columns] with unit column stride (got {tuple(out.shape)})")
    dev = out.device
    table = (_C.EgcTypedRel * max(len(rels), 1))()
    for d, r in zip(table, rels):
        _check_f32(r.inp, "a relation's input")
        if r.inp.dim() != 2 or r.inp.device != dev or (r.inp.numel() > 0 and r.inp.stride(1) != 1) \
                or r.in_col < 0 or r.in_col + width > r.inp.size(1):
            raise RuntimeError(f"egc_amd: a relation's input must be a [rows, >= {r.in_col + width}] tensor with unit column "
                               f"stride on {dev} (got {tuple(r.inp.shape)})")
        g = r.graph
        if g is not None:
            if g.n_nodes != n_rows or g.n_src_rows != r.inp.size(0) or g.device != dev:
                raise RuntimeError(f"egc_amd: a relation's adjacency is [{g.n_nodes}, {g.n_src_rows}] on {g.device}, the launch "
                                   f"has {n_rows} rows and the input {r.inp.size(0)} on {dev}")
            d.rowptr, d.col, d.n_edges = g.rowptr.data_ptr(), g.col.data_ptr(), g.n_edges
        elif r.inp.size(0) < n_rows:
            raise RuntimeError("egc_amd: the identity relation needs one input row per output row")
        if r.pre_rowptr is not None:
            p = r.pre_rowptr
            if p.dtype != torch.int32 or p.device != dev or p.numel() != r.inp.size(0) + 1 or not p.is_contiguous():
                raise RuntimeError("egc_amd: pre_rowptr must be the dense int32 [input rows + 1] rowptr of the forward graph")
            d.pre_rowptr = p.data_ptr()
        d.in_ = r.inp.data_ptr() + 4 * r.in_col if r.inp.numel() > 0 else None
        d.n_in_rows = r.inp.size(0)
        d.ld_in = r.inp.stride(0) if r.inp.size(0) > 1 else max(r.inp.size(1), width)
        d.out_col, d.post_mean = int(r.out_col), int(bool(r.post_mean))
    ld_out = out.stride(0) if n_rows > 1 else max(out.size(1), 1)
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_typed_mean_workspace_bytes(table, len(rels), width), dev)
        _C.check(lib.egc_typed_mean_f32(table, len(rels), n_rows, width, int(bool(accumulate)),
                                        out.data_ptr() if out.numel() else None, ld_out,
                                        _ptr(ws), nbytes, _stream_ptr(dev)),
                 "egc_typed_mean_f32")
    return out


class TypedMeanPlan:
    """What one call of the concatenated typed mean runs over: the node types in the order of their features and, per
    target type, the relations that reach it as (source type, CSRGraph [N_target, N_source]) in the order of their
    column blocks."""

    def __init__(self, types, rels):
        self.types = list(types)
        self.rels = {t: list(rels.get(t, ())) for t in self.types}
        for t, lst in self.rels.items():
            if len(lst) + 1 > _C.TYPED_MAX_RELATIONS:
                raise RuntimeError(f"egc_amd: at most {_C.TYPED_MAX_RELATIONS - 1} relations may reach one node type "
                                   f"({t}: {len(lst)})")
        for s in self.types:
            n_out = sum(1 for lst in self.rels.values() for src, _ in lst if src == s)
            if n_out + 1 > _C.TYPED_MAX_RELATIONS:
                raise RuntimeError(f"egc_amd: at most {_C.TYPED_MAX_RELATIONS - 1} relations may leave one node type "
                                   f"({s}: {n_out})")


class _TypedMeanCat(torch.autograd.Function):
    """A_t = [x_t | mean over relation 1's in-neighbours | mean over relation 2's ...] for every node type t: one launch
    per target type forward, one per source type backward (egc_typed_mean_f32 over the transposed CSRs, the relations
    of a source added in plan order, every d x element written once)."""

    @staticmethod
    def forward(ctx, plan: TypedMeanPlan, *xs):
        xs = [x.detach().contiguous() for x in xs]
        x_of = dict(zip(plan.types, xs))
        width = xs[0].size(1)
        outs = []
        for t, x in zip(plan.types, xs):
            rels = [TypedRel(None, x)]
            for j, (src, g) in enumerate(plan.rels[t]):
                rels.append(TypedRel(g, x_of[src], post_mean=True, out_col=(1 + j) * width))
            a = torch.empty((x.size(0), len(rels) * width), dtype=torch.float32, device=x.device)
            outs.append(typed_mean(rels, x.size(0), width, a))
        ctx.plan, ctx.width, ctx.rows = plan, width, [x.size(0) for x in xs]
        return tuple(outs)

    @staticmethod
    def backward(ctx, *d_as):
        plan, width = ctx.plan, ctx.width
        d_of = {t: d.contiguous() for t, d in zip(plan.types, d_as)}
        grads = []
        for i, s in enumerate(plan.types):
            if not ctx.needs_input_grad[1 + i]:
                grads.append(None)
                continue
            rels = [TypedRel(None, d_of[s])]
            for t in plan.types:
                for j, (src, g) in enumerate(plan.rels[t]):
                    if src == s and g.n_edges > 0:
                        rels.append(TypedRel(g.transposed(), d_of[t], in_col=(1 + j) * width, pre_rowptr=g.rowptr))
            d_x = torch.empty((ctx.rows[i], width), dtype=torch.float32, device=d_of[s].device)
            grads.append(typed_mean(rels, ctx.rows[i], width, d_x, accumulate=True))
        return (None, *grads)


def typed_mean_cat(plan: TypedMeanPlan, xs) -> tuple:
    """The operands A_t [N_t, (1 + relations into t) * width] of ``plan``'s node types from their features ``xs`` (float32
    [N_t, width] device tensors in the order of plan.types), differentiable with respect to every x."""
    xs = list(xs)
    if len(xs) != len(plan.types) or not xs:
        raise RuntimeError("egc_amd: one feature tensor per node type of the plan")
    width = xs[0].size(1) if xs[0].dim() == 2 else -1
    for t, x in zip(plan.types, xs):
        _check_f32(x, f"x[{t}]")
        if x.dim() != 2 or x.size(1) != width or x.device != xs[0].device:
            raise RuntimeError(f"egc_amd: x[{t}] must be [rows, {width}] on {xs[0].device} (got {tuple(x.shape)} on {x.device})")
    return _TypedMeanCat.apply(plan, *xs)
