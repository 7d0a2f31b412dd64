"""GCNConv, SAGEConv and GINConv (PyG 2.x; the three cheapest baselines of the reference's experiments/code/models.py) on the
neighbour-sum kernel of egc_nbr_sum.hip.

All three are one sparse operation with a dense product on one side: with agg_i the sum over row i's in-edges, in edge-list
order, of a per-entry term,

    sum      agg_i = sum_j x_j                      out_i = agg_i + s x_self_i              GIN (s = 1 + eps), GCN unnormalised, SAGE sum
    mean     agg_i = sum_j x_j                      out_i = agg_i / deg_i + s x_self_i      SAGE mean
    mean_t   agg_i = sum_j x_j / max(deg_j, 1)      out_i = agg_i + s x_self_i              the transpose of mean
    sym      agg_i = sum_j scale_j x_j              out_i = scale_i (agg_i + scale_i x_self_i)      GCN (scale = deg^-1/2)

0 for a row without edges (never divided); without x_self the self term is left out.  ``skip_self_entries`` leaves the entries
with j == i out -- the LOOPED edge set of include/egc_hip.h: every self loop of the input removed, the self term standing for
the one that ``add_remaining_self_loops`` adds.  The transpose of every form is a form again (sum -> sum, mean -> mean_t,
sym -> sym), so the backward is the same kernel on the transposed CSR, the self path fused into the same launch when x_self is x.
O(N d) memory, one gather pass over an [N, d] array each way, no [E, .] array, atomic-free and bit-reproducible in the
summation order of include/egc_hip.h (tests/nbr_ref.py restates it bit for bit).  The dense products are torch's (rocBLAS)."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C
from ._args import _as_csr, _check_f32, _layer_graph, _out_block, _ptr, _rows2d, _unit_columns, _workspace
from .graph import CSRGraph, _device_guard, _stream_ptr

_FORM = {"sum": _C.NBR_SUM, "add": _C.NBR_SUM, "mean": _C.NBR_MEAN, "mean_t": _C.NBR_MEAN_T, "sym": _C.NBR_SYM}
_TRANSPOSE = {_C.NBR_SUM: _C.NBR_SUM, _C.NBR_MEAN: _C.NBR_MEAN_T, _C.NBR_MEAN_T: _C.NBR_MEAN, _C.NBR_SYM: _C.NBR_SYM}


def _form_code(form) -> int:
    if form not in _FORM:
        raise ValueError(f"egc_amd.neighbor_sum: form must be one of {sorted(_FORM)}, got {form!r}")
    return _FORM[form]


def _table(t, name, n, dev):
    """A float32 device table of at least n entries, dense."""
    _check_f32(t, name)
    if t.dim() != 1 or t.numel() < n or t.device != dev or not t.is_contiguous():
        raise RuntimeError(f"egc_amd: {name} must be a dense float32 [>= {n}] tensor on {dev} (got {tuple(t.shape)} on {t.device})")
    return t


def _launch(g: CSRGraph, transposed: bool, x, x_self, form: int, skip: bool, self_scale: float, eps, scale, edge_scale, out):
    """egc_nbr_sum_f32 over ``g`` (``transposed``: over its transposed CSR, rows = the sources): ``out`` (a column block of
    the caller's operand is fine) from x and the optional x_self."""
    lib = _C.load()
    width, dev = x.size(1), x.device
    if g.device != dev:
        raise RuntimeError(f"egc_amd: the graph is on {g.device}, x on {dev}")
    walk = g.transposed() if transposed else g
    n_rows, n_in = (g.n_src_rows, g.n_nodes) if transposed else (g.n_nodes, g.n_src_rows)
    ld_x, ld_out = _rows2d(x, "x", n_in, width, dev), _rows2d(out, "out", n_rows, width, dev)
    ld_self = _rows2d(x_self, "x_self", n_rows, width, dev) if x_self is not None else 0
    deg_rowptr = None
    if form == _C.NBR_MEAN_T:        # the degrees of the rows the entries name: the rowptr of the walked CSR's transpose
        deg_rowptr = g.rowptr if transposed else g.transposed().rowptr
    if form == _C.NBR_SYM:
        if scale is None:
            raise RuntimeError("egc_amd.neighbor_sum: sym needs scale")
        _table(scale, "scale", max(n_rows, n_in), dev)
        if edge_scale is not None:
            _table(edge_scale, "edge_scale", g.n_edges, dev)
    if eps is not None and (eps.dtype != torch.float32 or eps.numel() != 1 or eps.device != dev):
        raise RuntimeError(f"egc_amd.neighbor_sum: eps must be one float32 on {dev}")
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_nbr_sum_workspace_bytes(g.n_edges, width), dev)
        _C.check(lib.egc_nbr_sum_f32(walk.rowptr.data_ptr(), walk.col.data_ptr(), n_rows, g.n_edges, n_in, x.data_ptr(), ld_x,
                                     _ptr(x_self), ld_self, width, form, int(skip), float(self_scale), _ptr(eps), _ptr(deg_rowptr),
                                     _ptr(scale), _ptr(scale), _ptr(edge_scale), out.data_ptr(), ld_out, _ptr(ws), nbytes,
                                     _stream_ptr(dev)), "egc_nbr_sum_f32")


class _NeighborSum(torch.autograd.Function):
    """out [N, d] from x (and x_self, eps).  ``shared``: x is the self operand too, and its gradient's self path is the backward
    launch's self term."""

    @staticmethod
    def forward(ctx, x, x_self, eps, g, form, skip, self_scale, scale, edge_scale, shared):
        xd = _unit_columns(x.detach())
        sd = xd if shared else (_unit_columns(x_self.detach()) if x_self is not None else None)
        ed = eps.detach() if eps is not None else None
        out = torch.empty((g.n_nodes, xd.size(1)), dtype=torch.float32, device=xd.device)
        _launch(g, False, xd, sd, form, skip, self_scale, ed, scale, edge_scale, out)
        ctx.cfg = (g, form, skip, self_scale, scale, shared, sd is not None)
        ctx.save_for_backward(ed, sd if (ed is not None and ctx.needs_input_grad[2]) else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        g, form, skip, self_scale, scale, shared, has_self = ctx.cfg
        eps, x_self = ctx.saved_tensors
        dout = _unit_columns(dout)
        dx = dself = deps = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty((g.n_src_rows, dout.size(1)), dtype=torch.float32, device=dout.device)
            _launch(g, True, dout, dout if shared else None, _TRANSPOSE[form], skip, self_scale, eps, scale, None, dx)
        if has_self and not shared and ctx.needs_input_grad[1]:
            if form == _C.NBR_SYM:
                s = scale[:g.n_nodes].unsqueeze(1)
                dself = (dout * s) * s
            else:
                dself = dout * (1.0 + eps) if eps is not None else dout * self_scale
        if eps is not None and ctx.needs_input_grad[2]:
            deps = (dout * x_self).sum().reshape(1)
        return dx, dself, deps, None, None, None, None, None, None, None


def _check_operands(x, x_self, g, form, skip, eps, who):
    _check_f32(x, "x")
    if x.dim() != 2 or x.size(0) != g.n_src_rows:
        raise RuntimeError(f"egc_amd.{who}: x has shape {tuple(x.shape)}, the graph's entries name {g.n_src_rows} rows")
    if x_self is not None:
        _check_f32(x_self, "x_self")
        if tuple(x_self.shape) != (g.n_nodes, x.size(1)):
            raise RuntimeError(f"egc_amd.{who}: x_self has shape {tuple(x_self.shape)}, expected {(g.n_nodes, x.size(1))}")
    elif eps is not None:
        raise RuntimeError(f"egc_amd.{who}: eps weights the self term; it needs x_self")
    if (form == _C.NBR_SYM or skip) and g.n_src_rows != g.n_nodes:
        raise RuntimeError(f"egc_amd.{who}: sym and skip_self_entries need a square graph (got [{g.n_nodes}, {g.n_src_rows}])")
    if form == _C.NBR_SYM and eps is not None:
        raise RuntimeError(f"egc_amd.{who}: sym weights its self term by scale^2, not by eps")


def neighbor_sum(x, graph, form, x_self=None, self_scale=1.0, eps=None, skip_self_entries=False, scale=None, edge_scale=None,
                 out=None, out_col=0):
    """The neighbour sum out [N, d] (module docstring) of x [rows the edges' sources name, d] over ``graph`` (a CSRGraph, an
    ``egc_amd.SparseTensor`` or a [2, E] int64 edge_index); ``form`` is "sum" (or "add"), "mean", "mean_t" or "sym".

    ``x_self`` [N, d] (may be x itself): the self term, weighted by ``self_scale``, or by 1 + eps when ``eps`` is given -- a
    one-element float32 DEVICE tensor that only the kernel reads, so a call never synchronises and stays capturable however
    eps changes.  ``scale`` [N] (sym): the row and source factor; ``edge_scale`` [E]: scale[col[p]] per CSR entry if the
    caller has it (``CSRGraph.edge_dis_*``), else the kernel gathers it.  ``skip_self_entries``: leave out the entries whose
    source is their row.  The library compiles the combinations the three layers launch (include/egc_hip.h lists them); any
    other raises.

    Differentiable in x, in x_self and in eps.  d x is the transposed form on ``graph.transposed()``; when x_self is x its
    self path is that launch's self term, otherwise d x_self = s * d out is a torch product.  d eps = (d out * x_self).sum() is
    a torch reduction.  ``out`` [N, >= out_col + d]: the inference form -- the result is written into its columns
    out_col .. out_col + d (the other columns are not touched) and that block is returned; it cannot carry a gradient."""
    code = _form_code(form)
    if x.dim() != 2:
        raise RuntimeError(f"egc_amd.neighbor_sum: x must be [rows, d] (got {tuple(x.shape)})")
    g = _as_csr(graph, x_self.size(0) if x_self is not None else x.size(0))
    skip = bool(skip_self_entries)
    _check_operands(x, x_self, g, code, skip, eps, "neighbor_sum")
    shared = x_self is x
    if out is None:
        return _NeighborSum.apply(x, None if shared else x_self, eps, g, code, skip, float(self_scale), scale, edge_scale, shared)
    block = _out_block(out, out_col, x.size(1), "neighbor_sum", (x, x_self, eps))
    xd = _unit_columns(x.detach())
    sd = xd if shared else (_unit_columns(x_self.detach()) if x_self is not None else None)
    _launch(g, False, xd, sd, code, skip, float(self_scale), eps.detach() if eps is not None else None, scale, edge_scale, block)
    return block


class _NbrOperand(torch.autograd.Function):
    """A = [agg | x] from x: the kernel writes the left half of A, x is copied into the right one (the _MpnnOperand pattern).
    Backward: d x = (the transposed form of d A's left half) + d A's right half, the addition being the launch's self term."""

    @staticmethod
    def forward(ctx, x, g, form):
        x = _unit_columns(x.detach())
        n, d = x.shape
        a = torch.empty((n, 2 * d), dtype=torch.float32, device=x.device)
        _launch(g, False, x, None, form, False, 1.0, None, None, None, a[:, :d])
        a[:, d:].copy_(x)
        ctx.g, ctx.form, ctx.d = g, form, d
        return a

    @staticmethod
    def backward(ctx, da):
        g, d = ctx.g, ctx.d
        da = _unit_columns(da)
        dx = torch.empty((g.n_src_rows, d), dtype=torch.float32, device=da.device)
        _launch(g, True, da[:, :d], da[:, d:], _TRANSPOSE[ctx.form], False, 1.0, None, None, None, dx)
        return dx, None, None


class GCNConv(nn.Module):
    """PyG 2.x ``GCNConv(in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True,
    bias=True)`` without edge weights: ``forward(x, edge_index)`` with edge_index a [2, E] int64 tensor, an
    ``egc_amd.SparseTensor`` or a ``CSRGraph``.  Parameters ``lin.weight`` [out, in] and ``bias`` [out] (state dicts interchange
    with strict=True; glorot / zeros as in PyG).  ``cached`` is accepted and ignored: the graph cache keeps the CSR and its
    degree tables whatever the flag says.  ``improved=True`` is not implemented.

    normalize and add_self_loops: out_i = dis_i (sum over the non-self in-edges of dis_j h_j + dis_i h_i), dis the LOOPED
    deg^-1/2 of the CSRGraph -- gcn_norm after add_remaining_self_loops.  normalize alone: the same over the edges as given with
    the RAW table and no self term.  add_self_loops alone: the plain sum over the non-self in-edges plus h_i.  Neither: the plain
    sum.  The sparse step runs on the narrower side: x W^T first when out <= in (PyG's order), the aggregate first otherwise;
    the bias is added last."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True):
        super().__init__()
        if improved:
            raise NotImplementedError("egc_amd.GCNConv: improved=True is not implemented")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.improved, self.cached, self.add_self_loops, self.normalize = False, bool(cached), bool(add_self_loops), bool(normalize)
        self.lin = nn.Linear(self.in_channels, self.out_channels, bias=False)
        self.register_parameter("bias", nn.Parameter(torch.empty(self.out_channels)) if bias else None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.xavier_uniform_(self.lin.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def propagate(self, h, g: CSRGraph):
        loops = self.add_self_loops
        if self.normalize:
            scale, edge_scale = (g.dis_looped, g.edge_dis_looped) if loops else (g.dis_raw, g.edge_dis_raw)
            return neighbor_sum(h, g, "sym", x_self=h if loops else None, skip_self_entries=loops, scale=scale, edge_scale=edge_scale)
        return neighbor_sum(h, g, "sum", x_self=h if loops else None, skip_self_entries=loops)

    def forward(self, x, edge_index):
        g = _layer_graph(x, edge_index, self.in_channels, "GCNConv")
        if self.out_channels <= self.in_channels:
            out = self.propagate(self.lin(x), g)
            return out + self.bias if self.bias is not None else out
        return F.linear(self.propagate(x, g), self.lin.weight, self.bias)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, add_self_loops={self.add_self_loops}, normalize={self.normalize}"


class SAGEConv(nn.Module):
    """PyG 2.x ``SAGEConv(in_channels, out_channels, aggr="mean", normalize=False, root_weight=True, project=False, bias=True)``:
    out = lin_l(aggr_j x_j) + lin_r(x_i), aggr "mean" or "sum" / "add".  Parameters ``lin_l.weight``, ``lin_l.bias``,
    ``lin_r.weight`` (state dicts interchange with strict=True).  The kernel writes the aggregate into the left half of
    [agg | x] and one product with [W_l | W_r] follows; without root_weight it is the aggregate and lin_l alone.
    ``normalize``: F.normalize(out, p=2, dim=-1).  ``project=True`` and the other aggregators are not implemented."""

    def __init__(self, in_channels, out_channels, aggr="mean", normalize=False, root_weight=True, project=False, bias=True):
        super().__init__()
        if aggr not in ("mean", "sum", "add"):
            raise ValueError(f"egc_amd.SAGEConv: aggr must be 'mean', 'sum' or 'add', got {aggr!r}")
        if project:
            raise NotImplementedError("egc_amd.SAGEConv: project=True is not implemented")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.aggr, self.normalize, self.root_weight, self.project = aggr, bool(normalize), bool(root_weight), False
        self.lin_l = nn.Linear(self.in_channels, self.out_channels, bias=bias)
        if self.root_weight:
            self.lin_r = nn.Linear(self.in_channels, self.out_channels, bias=False)

    def forward(self, x, edge_index):
        g = _layer_graph(x, edge_index, self.in_channels, "SAGEConv")
        if self.root_weight:
            a = _NbrOperand.apply(x, g, _FORM[self.aggr])
            out = F.linear(a, torch.cat([self.lin_l.weight, self.lin_r.weight], dim=1), self.lin_l.bias)
        else:
            out = self.lin_l(neighbor_sum(x, g, self.aggr))
        return F.normalize(out, p=2.0, dim=-1) if self.normalize else out

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, aggr={self.aggr}, root_weight={self.root_weight}, normalize={self.normalize}"


class GINConv(nn.Module):
    """PyG 2.x ``GINConv(nn, eps=0., train_eps=False)``: out = nn((1 + eps) x_i + sum_j x_j).  ``eps`` is a [1] Parameter with
    train_eps and a [1] buffer otherwise, in the state dict either way.  The kernel reads it on the device, so training it or
    filling it in place never synchronises."""

    def __init__(self, nn, eps=0.0, train_eps=False):
        super().__init__()
        self.nn = nn
        self.initial_eps = float(eps)
        if train_eps:
            self.eps = torch.nn.Parameter(torch.empty(1))
        else:
            self.register_buffer("eps", torch.empty(1))
        self.reset_parameters()

    def reset_parameters(self):
        for m in self.nn.modules():
            if callable(getattr(m, "reset_parameters", None)):
                m.reset_parameters()
        with torch.no_grad():
            self.eps.fill_(self.initial_eps)

    def forward(self, x, edge_index):
        if x.dim() != 2:
            raise RuntimeError(f"egc_amd.GINConv: x has shape {tuple(x.shape)}, expected (rows, channels)")
        g = _layer_graph(x, edge_index, x.size(1), "GINConv")
        return self.nn(neighbor_sum(x, g, "sum", x_self=x, eps=self.eps))

    def extra_repr(self):
        return f"train_eps={isinstance(self.eps, torch.nn.Parameter)}"
