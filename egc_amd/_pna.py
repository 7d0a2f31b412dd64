"""PNAConv (PyG 2.x, ``edge_dim=None``, ``pre_layers=1``, ``post_layers=1``) on the multi-aggregator kernels of egc_pna.hip.

The stock layer builds [E, 2 F] endpoint features and [E, T F] messages, makes one scatter pass per aggregator over them (one of
them over their squares) and forms a [N, T, A S F] scaled concatenation.  None of that is needed:

  * a tower's pre-transform acts on [x_i | x_j] and its weight is [Wd_t | Ws_t] (target half first), so with P = x Ms^T and
    Q = x Md^T + b_pre (both [N, W], W = towers * F_in; Ms / Md the block diagonals of the tower blocks with ``divide_input``,
    their vertical stacks otherwise) the message of edge j -> i is P_j + Q_i;
  * every aggregator of the list comes out of ONE gather pass over P (``pna_aggregate``: agg [N, A W], block a = aggregator a);
  * a scaler is a per-row scalar and commutes with the linear post-transform, and post and lin have nothing between them, so
    Y = agg G^T [N, S out] (G: lin folded over the post blocks of each scaler) and base = x (lin post_x)^T + folded bias, and
    out_i = base_i + sum_k f_k(d_i) Y_i[k] (``pna_scale_combine``).

``PNAConv.forward`` is: one dense product x -> [P | Q], the aggregate kernel, one dense product agg -> Y, one dense product
x -> base, the combine kernel.  No [E, .] and no [N, S A W] array exists forward or backward.  The dense products are torch's;
the folds are torch on the small weight matrices inside autograd, so the parameter gradients fall out of them."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _C
from ._args import _as_csr, _check_f32, _layer_graph, _out_block, _ptr, _rows2d, _unit_columns, _workspace
from .graph import CSRGraph, GraphBatch, SparseTensor, _device_guard, _stream_ptr

AGGREGATORS = {"sum": _C.PNA_SUM, "mean": _C.PNA_MEAN, "min": _C.PNA_MIN, "max": _C.PNA_MAX, "var": _C.PNA_VAR, "std": _C.PNA_STD}
SCALERS = {"identity": _C.PNA_IDENTITY, "amplification": _C.PNA_AMPLIFICATION, "attenuation": _C.PNA_ATTENUATION,
           "linear": _C.PNA_LINEAR, "inverse_linear": _C.PNA_INVERSE_LINEAR}


def _codes(names, table, what):
    names = [names] if isinstance(names, str) else list(names)
    for a in names:
        if a not in table:
            raise ValueError(f"egc_amd.PNAConv: unknown {what} {a!r}; expected one of {sorted(table)}")
    if len(names) == 0 or len(set(names)) != len(names):
        raise ValueError(f"egc_amd.PNAConv: the {what} list must hold at least one name and none twice (got {names})")
    return tuple(table[a] for a in names)


def _int_array(codes):
    return (C.c_int32 * len(codes))(*codes)


def degree_statistics(deg):
    """(avg_lin, avg_log) of an in-degree histogram ``deg`` (deg[k] = the number of nodes with in-degree k), in float64 on the
    host: sum k deg[k] / sum deg[k] and sum log(k + 1) deg[k] / sum deg[k]."""
    d = torch.as_tensor(deg).detach().to("cpu", torch.float64)
    if d.dim() != 1 or d.numel() == 0 or float(d.sum()) <= 0:
        raise ValueError("egc_amd.PNAConv: deg must be a non-empty 1-D in-degree histogram with a positive total")
    k = torch.arange(d.numel(), dtype=torch.float64)
    total = float(d.sum())
    return float((k * d).sum()) / total, float(((k + 1).log() * d).sum()) / total


def degree_histogram(graph, num_nodes=None):
    """The in-degree histogram PNAConv's ``deg`` wants: int64 [max in-degree + 1], entry k = the number of nodes with k in-edges
    (``torch.bincount(degree(edge_index[1], num_nodes))``, what the reference's PNA configs compute by hand).  ``graph``: a
    [2, E] int64 edge_index (``num_nodes``: the node count, default max index + 1), an ``egc_amd.SparseTensor`` or a CSRGraph."""
    if isinstance(graph, SparseTensor):
        graph = graph.graph
    if isinstance(graph, GraphBatch):
        graph = graph.csr()
    if isinstance(graph, CSRGraph):
        indeg = graph.rowptr[1:graph.n_nodes + 1].long() - graph.rowptr[:graph.n_nodes].long()
    elif isinstance(graph, torch.Tensor) and graph.dim() == 2 and graph.size(0) == 2 and graph.dtype == torch.int64:
        n = int(num_nodes) if num_nodes is not None else (int(graph.max()) + 1 if graph.numel() else 0)
        indeg = torch.bincount(graph[1], minlength=n)
    else:
        raise RuntimeError(f"egc_amd.degree_histogram: expected a [2, E] int64 edge_index, a SparseTensor or a CSRGraph, got {type(graph)}")
    return torch.bincount(indeg) if indeg.numel() else torch.zeros(1, dtype=torch.int64, device=indeg.device)


# ------------------------------------------------------------------------------------------------------------ the launches

def _launch_aggregate(P, Q, g: CSRGraph, codes, out, arg_min=None, arg_max=None, mu=None, var=None):
    """egc_pna_aggregate_f32: ``out`` [n_nodes, A * width] (a column block of the caller's array) = the A aggregate blocks."""
    lib = _C.load()
    width, dev, a = Q.size(1), Q.device, len(codes)
    ld_q, ld_p = _rows2d(Q, "Q", g.n_nodes, width, dev), _rows2d(P, "P", g.n_src_rows, width, dev)
    ld_out = _rows2d(out, "out", g.n_nodes, a * width, dev)
    if g.device != dev:
        raise RuntimeError(f"egc_amd: the graph is on {g.device}, P and Q on {dev}")
    ops = _int_array(codes)
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_pna_aggregate_workspace_bytes(g.n_edges, width, C.addressof(ops), a), dev)
        _C.check(lib.egc_pna_aggregate_f32(g.rowptr.data_ptr(), g.col.data_ptr(), g.edge_id.data_ptr(), g.n_nodes, g.n_edges,
                                           g.n_src_rows, P.data_ptr(), ld_p, Q.data_ptr(), ld_q, width, C.addressof(ops), a,
                                           out.data_ptr(), ld_out, _ptr(arg_min), _ptr(arg_max), _ptr(mu), _ptr(var), _ptr(ws), nbytes,
                                           _stream_ptr(dev)), "egc_pna_aggregate_f32")


def _launch_aggregate_backward(dagg, g: CSRGraph, codes, P, arg_min, arg_max, mu, var, dP, dQ):
    """egc_pna_aggregate_backward_f32: dP [n_src_rows, width] and dQ [n_nodes, width] (either may be None) from d agg."""
    lib = _C.load()
    a, dev = len(codes), dagg.device
    width = dagg.size(1) // a
    ld_g = _rows2d(dagg, "d agg", g.n_nodes, a * width, dev)
    ld_dp = _rows2d(dP, "d P", g.n_src_rows, width, dev) if dP is not None else 0
    ld_dq = _rows2d(dQ, "d Q", g.n_nodes, width, dev) if dQ is not None else 0
    ld_p = _rows2d(P, "P", g.n_src_rows, width, dev) if P is not None else 0
    t = g.transposed() if dP is not None else None
    ops = _int_array(codes)
    with _device_guard(dev):
        ws, nbytes = _workspace(lib.egc_pna_aggregate_backward_workspace_bytes(g.n_nodes, g.n_edges, width) if dP is not None else 0,
                                dev)
        _C.check(lib.egc_pna_aggregate_backward_f32(
            g.rowptr.data_ptr(), g.edge_id.data_ptr(), g.n_nodes, _ptr(t.rowptr if t else None), _ptr(t.col if t else None),
            _ptr(t.edge_id if t else None), g.n_src_rows, g.n_edges, dagg.data_ptr(), ld_g, C.addressof(ops), a, width, _ptr(P), ld_p,
            _ptr(arg_min), _ptr(arg_max), _ptr(mu), _ptr(var), _ptr(dP), ld_dp, _ptr(dQ), ld_dq, _ptr(ws), nbytes,
            _stream_ptr(dev)), "egc_pna_aggregate_backward_f32")


def _launch_combine(Y, base, g: CSRGraph, scodes, avg_lin, avg_log, out):
    lib = _C.load()
    dim, dev, s = base.size(1), base.device, len(scodes)
    ld_y, ld_b = _rows2d(Y, "Y", g.n_nodes, s * dim, dev), _rows2d(base, "base", g.n_nodes, dim, dev)
    ld_o = _rows2d(out, "out", g.n_nodes, dim, dev)
    sc = _int_array(scodes)
    with _device_guard(dev):
        _C.check(lib.egc_pna_scale_combine_f32(g.rowptr.data_ptr(), g.n_nodes, C.addressof(sc), s, float(avg_lin), float(avg_log), dim,
                                               Y.data_ptr(), ld_y, base.data_ptr(), ld_b, out.data_ptr(), ld_o, _stream_ptr(dev)),
                 "egc_pna_scale_combine_f32")


def _launch_combine_backward(gout, g: CSRGraph, scodes, avg_lin, avg_log, dY):
    lib = _C.load()
    dim, dev, s = gout.size(1), gout.device, len(scodes)
    ld_g, ld_dy = _rows2d(gout, "d out", g.n_nodes, dim, dev), _rows2d(dY, "d Y", g.n_nodes, s * dim, dev)
    sc = _int_array(scodes)
    with _device_guard(dev):
        _C.check(lib.egc_pna_scale_combine_backward_f32(g.rowptr.data_ptr(), g.n_nodes, C.addressof(sc), s, float(avg_lin),
                                                        float(avg_log), dim, gout.data_ptr(), ld_g, dY.data_ptr(), ld_dy,
                                                        _stream_ptr(dev)), "egc_pna_scale_combine_backward_f32")


# -------------------------------------------------------------------------------------------------------------- autograd

def _saved_arrays(codes, n, width, dev, training):
    """(arg_min, arg_max, mu, var) the backward needs for this list -- allocated only when a gradient is wanted."""
    def new(dtype, wanted):
        return torch.empty((n, width), dtype=dtype, device=dev) if (training and wanted) else None
    mom2 = _C.PNA_VAR in codes or _C.PNA_STD in codes
    return (new(torch.int32, _C.PNA_MIN in codes), new(torch.int32, _C.PNA_MAX in codes), new(torch.float32, mom2),
            new(torch.float32, mom2))


class _PnaAggregate(torch.autograd.Function):
    """agg [N, A W] from P and Q: the aggregate kernel forward, the two backward passes over the rows and the transposed CSR."""

    @staticmethod
    def forward(ctx, P, Q, g, codes):
        P, Q = P.detach(), Q.detach()
        width = Q.size(1)
        ctx.saved = _saved_arrays(codes, g.n_nodes, width, Q.device, any(ctx.needs_input_grad[:2]))
        agg = torch.empty((g.n_nodes, len(codes) * width), dtype=torch.float32, device=Q.device)
        _launch_aggregate(P, Q, g, codes, agg, *ctx.saved)
        ctx.g, ctx.codes, ctx.width = g, codes, width
        ctx.save_for_backward(P)
        return agg

    @staticmethod
    def backward(ctx, dagg):
        g, width, codes = ctx.g, ctx.width, ctx.codes
        P, = ctx.saved_tensors
        dagg = _unit_columns(dagg)
        dP = torch.empty((g.n_src_rows, width), dtype=torch.float32, device=dagg.device) if ctx.needs_input_grad[0] else None
        dQ = torch.empty((g.n_nodes, width), dtype=torch.float32, device=dagg.device) if ctx.needs_input_grad[1] else None
        _launch_aggregate_backward(dagg, g, codes, P, *ctx.saved, dP, dQ)
        return dP, dQ, None, None


class _PnaAggregatePQ(torch.autograd.Function):
    """The same from pq = [P | Q] (a square graph): the backward writes d P and d Q into the two halves of ONE d pq."""

    @staticmethod
    def forward(ctx, pq, g, codes):
        pq = pq.detach()
        width = pq.size(1) // 2
        ctx.saved = _saved_arrays(codes, g.n_nodes, width, pq.device, ctx.needs_input_grad[0])
        agg = torch.empty((g.n_nodes, len(codes) * width), dtype=torch.float32, device=pq.device)
        _launch_aggregate(pq[:, :width], pq[:, width:], g, codes, agg, *ctx.saved)
        ctx.g, ctx.codes, ctx.width = g, codes, width
        ctx.save_for_backward(pq)
        return agg

    @staticmethod
    def backward(ctx, dagg):
        g, width, codes = ctx.g, ctx.width, ctx.codes
        pq, = ctx.saved_tensors
        dagg = _unit_columns(dagg)
        dpq = torch.empty((g.n_nodes, 2 * width), dtype=torch.float32, device=dagg.device)
        _launch_aggregate_backward(dagg, g, codes, pq[:, :width], *ctx.saved, dpq[:, :width], dpq[:, width:])
        return dpq, None, None


class _PnaCombine(torch.autograd.Function):
    """out = base + sum_k f_k(d) Y[k]: the combine kernel; backward d Y[k] = f_k(d) g by its twin, d base = g."""

    @staticmethod
    def forward(ctx, Y, base, g, scodes, avg_lin, avg_log):
        Y, base = Y.detach(), base.detach()
        out = torch.empty((g.n_nodes, base.size(1)), dtype=torch.float32, device=base.device)
        _launch_combine(Y, base, g, scodes, avg_lin, avg_log, out)
        ctx.g, ctx.scodes, ctx.avg = g, scodes, (avg_lin, avg_log)
        return out

    @staticmethod
    def backward(ctx, gout):
        g, scodes = ctx.g, ctx.scodes
        gout = _unit_columns(gout)
        dY = None
        if ctx.needs_input_grad[0]:
            dY = torch.empty((g.n_nodes, len(scodes) * gout.size(1)), dtype=torch.float32, device=gout.device)
            _launch_combine_backward(gout, g, scodes, *ctx.avg, dY)
        return dY, (gout if ctx.needs_input_grad[1] else None), None, None, None, None


# ---------------------------------------------------------------------------------------------------- kernel-level functions

def _q_and_graph(Q, graph):
    _check_f32(Q, "Q")
    if Q.dim() != 2:
        raise RuntimeError(f"egc_amd: Q must be [N, W] (got {tuple(Q.shape)})")
    return _as_csr(graph, Q.size(0))


def pna_aggregate(P, Q, graph, aggregators, out=None, out_col=0):
    """agg [N, A W]: block a (columns a W .. (a + 1) W) is aggregator a of ``aggregators`` (names of sum / mean / min / max / var /
    std, in this order) of the messages P_j + Q_i over every row's in-edges in edge-list order (module docstring), in the order
    of operations of include/egc_hip.h (tests/pna_ref.py restates it bit for bit).  P [rows the edges' sources name, W], Q [N, W];
    ``graph`` a CSRGraph, SparseTensor or [2, E] int64 edge_index.  Differentiable with respect to P and Q.  ``out``
    [N, >= out_col + A W]: the inference form -- the blocks are written into its columns out_col .. out_col + A W (the other
    columns are not touched) and that block is returned; with ``out`` neither P nor Q may require a gradient."""
    codes = _codes(aggregators, AGGREGATORS, "aggregator")
    g = _q_and_graph(Q, graph)
    if out is None:
        return _PnaAggregate.apply(P, Q, g, codes)
    block = _out_block(out, out_col, len(codes) * Q.size(1), "pna_aggregate", (P, Q))
    _launch_aggregate(P.detach(), Q.detach(), g, codes, block)
    return block


def pna_aggregate_saved(P, Q, graph, aggregators):
    """(agg, arg_min, arg_max, mu, var) of the training form: the int32 [N, W] positions in the edge list of the first in-edge
    attaining each column's minimum / maximum (-1 for a row without edges; None when not listed) and the row means and clamped
    variances of P (None without var / std) -- what the backward reads."""
    codes = _codes(aggregators, AGGREGATORS, "aggregator")
    g = _q_and_graph(Q, graph)
    saved = _saved_arrays(codes, g.n_nodes, Q.size(1), Q.device, True)
    agg = torch.empty((g.n_nodes, len(codes) * Q.size(1)), dtype=torch.float32, device=Q.device)
    _launch_aggregate(P.detach(), Q.detach(), g, codes, agg, *saved)
    return (agg,) + saved


def pna_aggregate_backward(dagg, graph, aggregators, P=None, arg_min=None, arg_max=None, mu=None, var=None, want=(True, True)):
    """(d P, d Q) of ``pna_aggregate`` from d agg [N, A W] and what ``pna_aggregate_saved`` returned (``P``, ``mu``, ``var``: read
    when var / std is listed): the backward kernels on their own.  ``want``: which of the two
    to compute (the other is None)."""
    codes = _codes(aggregators, AGGREGATORS, "aggregator")
    _check_f32(dagg, "d agg")
    g = _as_csr(graph, dagg.size(0))
    if dagg.dim() != 2 or dagg.size(1) % len(codes):
        raise RuntimeError(f"egc_amd: d agg must be [N, {len(codes)} W] (got {tuple(dagg.shape)})")
    width = dagg.size(1) // len(codes)
    if want[0]:
        if (_C.PNA_MIN in codes and arg_min is None) or (_C.PNA_MAX in codes and arg_max is None):
            raise RuntimeError("egc_amd.pna_aggregate_backward: min / max need the forward's arg_min / arg_max")
        if (_C.PNA_VAR in codes or _C.PNA_STD in codes) and (mu is None or var is None or P is None):
            raise RuntimeError("egc_amd.pna_aggregate_backward: var / std need P and the forward's mu and var")
    dP = torch.empty((g.n_src_rows, width), dtype=torch.float32, device=dagg.device) if want[0] else None
    dQ = torch.empty((g.n_nodes, width), dtype=torch.float32, device=dagg.device) if want[1] else None
    _launch_aggregate_backward(dagg, g, codes, P, arg_min, arg_max, mu, var, dP, dQ)
    return dP, dQ


def pna_scale_combine(Y, base, graph, scalers, avg_lin, avg_log):
    """out [N, D] = base + sum_k f_k(d_i) Y[:, k D : (k + 1) D] with the degree scalers ``scalers`` (names of identity /
    amplification / attenuation / linear / inverse_linear), d_i = max(in-degree, 1), the factors computed in the kernel from the
    graph's offsets.  Differentiable with respect to Y and base."""
    scodes = _codes(scalers, SCALERS, "scaler")
    _check_f32(base, "base")
    if base.dim() != 2:
        raise RuntimeError(f"egc_amd: base must be [N, D] (got {tuple(base.shape)})")
    return _PnaCombine.apply(Y, base, _as_csr(graph, base.size(0)), scodes, float(avg_lin), float(avg_log))


def pna_scale_combine_backward(gout, graph, scalers, avg_lin, avg_log):
    """d Y [N, S D] of ``pna_scale_combine`` from d out [N, D] (d base is d out itself)."""
    scodes = _codes(scalers, SCALERS, "scaler")
    _check_f32(gout, "d out")
    g = _as_csr(graph, gout.size(0))
    dY = torch.empty((g.n_nodes, len(scodes) * gout.size(1)), dtype=torch.float32, device=gout.device)
    _launch_combine_backward(gout, g, scodes, float(avg_lin), float(avg_log), dY)
    return dY


# ------------------------------------------------------------------------------------------------------------------ layer

def fold_weights(pre_w, pre_b, post_w, post_b, lin_w, lin_b, n_aggr, n_scalers, divide_input):
    """(w_pq [2 W, in], b_pq [2 W]; w_y [S out, A W]; w_base [out, in], b_base [out]) from the per-tower weights (lists over the
    towers).  torch, differentiable, any dtype.  Columns of post_w[t]: [x^t : F_in | scaler 0 : (aggregator 0 : F_in | ...) | ...]."""
    fi = pre_w[0].size(0)
    place = (lambda blocks: torch.block_diag(*blocks)) if divide_input else (lambda blocks: torch.cat(list(blocks), dim=0))
    w_pq = torch.cat([place([w[:, fi:] for w in pre_w]), place([w[:, :fi] for w in pre_w])], dim=0)     # P: source, Q: target
    b_pre = torch.cat(list(pre_b))
    b_pq = torch.cat([torch.zeros_like(b_pre), b_pre])
    per_scaler = []
    for s in range(n_scalers):
        blocks = [torch.block_diag(*[w[:, fi * (1 + s * n_aggr + a):fi * (2 + s * n_aggr + a)] for w in post_w]) for a in range(n_aggr)]
        per_scaler.append(lin_w @ torch.cat(blocks, dim=1))
    w_y = torch.cat(per_scaler, dim=0)
    w_base = lin_w @ place([w[:, :fi] for w in post_w])
    b_base = lin_w @ torch.cat(list(post_b)) + lin_b
    return w_pq, b_pq, w_y, w_base, b_base


class PNAConv(nn.Module):
    """PyG 2.x ``PNAConv(in_channels, out_channels, aggregators, scalers, deg, edge_dim=None, towers=1, pre_layers=1, post_layers=1,
    divide_input=False)`` with ``edge_dim=None`` and one pre and one post layer (anything else raises NotImplementedError).
    Submodules ``pre_nns.{t}.0``, ``post_nns.{t}.0`` and ``lin`` are built in PyG's order, so state dicts interchange with
    strict=True and a seed gives PyG's initial parameters.  ``forward(x, edge_index)`` with edge_index a [2, E] int64 tensor, an
    ``egc_amd.SparseTensor``, a ``CSRGraph`` or a ``GraphBatch``.  ``deg``: the in-degree histogram (``egc_amd.degree_histogram``)."""

    def __init__(self, in_channels, out_channels, aggregators, scalers, deg, edge_dim=None, towers=1, pre_layers=1, post_layers=1,
                 divide_input=False):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("egc_amd.PNAConv: edge_dim is not implemented (edge features are out of scope)")
        if pre_layers != 1 or post_layers != 1:
            raise NotImplementedError("egc_amd.PNAConv: only pre_layers=1 and post_layers=1 are implemented "
                                      f"(got pre_layers={pre_layers}, post_layers={post_layers})")
        if divide_input:
            assert in_channels % towers == 0
        assert out_channels % towers == 0
        self.aggregators = [aggregators] if isinstance(aggregators, str) else list(aggregators)
        self.scalers = [scalers] if isinstance(scalers, str) else list(scalers)
        self._codes = _codes(self.aggregators, AGGREGATORS, "aggregator")
        self._scodes = _codes(self.scalers, SCALERS, "scaler")
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.towers, self.divide_input = int(towers), bool(divide_input)
        self.F_in = self.in_channels // self.towers if divide_input else self.in_channels
        self.F_out = self.out_channels // self.towers
        self.avg_deg = dict(zip(("lin", "log"), degree_statistics(deg)))
        if ({"amplification", "attenuation"} & set(self.scalers) and not self.avg_deg["log"] > 0) or \
                ({"linear", "inverse_linear"} & set(self.scalers) and not self.avg_deg["lin"] > 0):
            raise ValueError("egc_amd.PNAConv: the degree histogram has no node with an in-edge; its scalers are undefined")
        self.pre_nns, self.post_nns = nn.ModuleList(), nn.ModuleList()
        width_post = (len(self._codes) * len(self._scodes) + 1) * self.F_in
        for _ in range(self.towers):
            self.pre_nns.append(nn.Sequential(nn.Linear(2 * self.F_in, self.F_in)))
            self.post_nns.append(nn.Sequential(nn.Linear(width_post, self.F_out)))
        self.lin = nn.Linear(self.out_channels, self.out_channels)
        self._fold_key, self._fold = None, None

    def _folded(self):
        pre, post = [s[0] for s in self.pre_nns], [s[0] for s in self.post_nns]
        return fold_weights([l.weight for l in pre], [l.bias for l in pre], [l.weight for l in post], [l.bias for l in post],
                            self.lin.weight, self.lin.bias, len(self._codes), len(self._scodes), self.divide_input)

    def _weights(self):
        params = list(self.parameters())
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return self._folded()
        key = tuple((p.data_ptr(), p._version) for p in params)
        if key != self._fold_key:
            with torch.no_grad():
                self._fold = tuple(t.contiguous() for t in self._folded())
            self._fold_key = key
        return self._fold

    def forward(self, x, edge_index):
        g = _layer_graph(x, edge_index, self.in_channels, "PNAConv")
        w_pq, b_pq, w_y, w_base, b_base = self._weights()
        pq = F.linear(x, w_pq, b_pq)                                          # both halves of every tower's pre-transform
        agg = _PnaAggregatePQ.apply(pq, g, self._codes)                       # every aggregator, one gather pass
        y = F.linear(agg, w_y)                                                # lin o post, one block of columns per scaler
        base = F.linear(x, w_base, b_base)                                    # lin o post on the x^t columns, folded biases
        return _PnaCombine.apply(y, base, g, self._scodes, self.avg_deg["lin"], self.avg_deg["log"])

    def extra_repr(self):
        return (f"{self.in_channels}, {self.out_channels}, aggregators={self.aggregators}, scalers={self.scalers}, "
                f"towers={self.towers}, divide_input={self.divide_input}")
