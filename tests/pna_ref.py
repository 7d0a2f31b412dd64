"""Fixtures and CPU restatement of PNAConv (tests/golden/pna/*.npz, written by tests/golden/make_golden_pna.py from a per-edge torch
composition of PyG 2.x's formulas) and of the three kernels of egc_amd/csrc/egc_pna.hip.

The algebra.  T towers, F_in per tower, W = T F_in.  pre_nns[t].0.weight is [F_in, 2 F_in] = [Wd_t | Ws_t] (target half first); with
P = x Ms^T and Q = x Md^T + b_pre (Ms / Md: block diagonals of the tower blocks with divide_input, their vertical stacks otherwise)
the message of edge j -> i is P_j + Q_i.  Over a row's n in-edges in edge-list order, per column:

    sum  S0 + n Q_i    mean  S0 / n + Q_i    min / max  (min / max P_j) + Q_i    var  v = max(S2 / n - (S1 / n)^2, 0)    std  sqrt(v + 1e-5)

with S0 = sum P_j, s = P of the row's first entry, S1 = sum (P_j - s), S2 = sum (P_j - s)^2, mu = s + S1 / n; 0 (std: sqrt(1e-5);
arg -1) for a row without edges.  Backward: a column whose v is exactly 0 takes no var / std gradient (PyG's relu'(0) = 0).
Scalers act per row on d = max(n, 1); out = lin(post(.)) folds into Y = agg G^T, base = x (lin post_x)^T + bias and
out_i = base_i + sum_k f_k(d_i) Y_i[k] (egc_amd/_pna.py:fold_weights).

``aggregate_forward`` / ``aggregate_backward`` / ``scale_combine`` / ``scale_combine_backward`` are sequential numpy in one dtype in the
documented order of egc_pna.hip: a row's entries are cut into consecutive chunks of ``chunk`` entries counted from its first entry,
every accumulator takes a chunk's entries in order (``np.add.accumulate`` is that left-to-right sum), the chunks are merged in
ascending order (addition; a strict compare for min / max, so the first entry and the first chunk keep a tie), then the finishing
steps one correctly rounded operation each -- so in float32 these ARE the kernels' bits, in float64 the truth of the shape sweep.
The scaler factors are formed in float64 and rounded once to the dtype, as the kernel does."""
import json
import os

import numpy as np
import torch

from egc_amd._pna import fold_weights
from mpnn_ref import CHUNK, WIDTHS, csr_by_destination, ladder_graph, ladder_inputs, rel_grad, rel_out  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pna")
CASES = ("messy", "hub", "ties", "nodivide", "all6", "meanonly", "w116")
ALL_AGGREGATORS = ("sum", "mean", "min", "max", "var", "std")
ALL_SCALERS = ("identity", "amplification", "attenuation", "linear", "inverse_linear")
REF_AGGREGATORS = ("mean", "min", "max", "std")


def load_pna_golden(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        z = {k: z[k] for k in z.files}
    meta = json.loads(bytes(z["meta"]).decode())
    g = dict(meta=meta, name=name, x=z["x"], ei=z["edge_index"], deg=z["deg"], gout=z["gout"], out32=z["out32"], out64=z["out64"],
             grad_x64=z["grad_x64"])
    g["params"] = {k[len("param:"):]: v for k, v in z.items() if k.startswith("param:")}
    g["init"] = {k[len("init:"):]: v for k, v in z.items() if k.startswith("init:")}
    g["grad64"] = {k[len("grad64:"):]: v for k, v in z.items() if k.startswith("grad64:")}
    return g


def _seq_sum(v):
    """((v0 + v1) + v2) + ... along axis 0 in v's dtype"""
    return np.add.accumulate(v, axis=0)[-1]


def aggregate_forward(P, Q, ei, aggregators, chunk=CHUNK, dtype=np.float32):
    """dict(agg [N, A W], arg_min, arg_max [N, W] int32 edge-list positions or None, mu, var [N, W] or None) in the documented order.
    P may have any number of rows (the rows the edges' sources name); N is Q's."""
    P, Q = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    n, w = Q.shape
    aggregators = list(aggregators)
    rowptr, col, eid = csr_by_destination(ei, n)
    need_sum = bool({"sum", "mean"} & set(aggregators))
    need_mom = bool({"var", "std"} & set(aggregators))
    need_ext = bool({"min", "max"} & set(aggregators))
    eps = dtype(1e-5)
    blocks = {a: np.zeros((n, w), dtype=dtype) for a in aggregators}
    if "std" in blocks:
        blocks["std"][:] = np.sqrt(eps)
    arg_min = np.full((n, w), -1, dtype=np.int32) if "min" in aggregators else None
    arg_max = np.full((n, w), -1, dtype=np.int32) if "max" in aggregators else None
    mu = np.zeros((n, w), dtype=dtype) if need_mom else None
    var = np.zeros((n, w), dtype=dtype) if need_mom else None
    for row in range(n):
        p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
        if p1 == p0:
            continue
        nf, q = dtype(p1 - p0), Q[row]
        shift = P[col[p0]]
        s0 = s1 = s2 = mn = mx = pmn = pmx = None
        for s in range(p0, p1, chunk):
            v = P[col[s:min(s + chunk, p1)]]
            first = s == p0
            if need_sum:
                c = _seq_sum(v)
                s0 = c if first else s0 + c
            if need_mom:
                d = v - shift
                c1, c2 = _seq_sum(d), _seq_sum(d * d)
                s1, s2 = (c1, c2) if first else (s1 + c1, s2 + c2)
            if need_ext:      # argmin / argmax name the first occurrence: the strict compare inside a chunk
                c_mn, c_pmn, c_mx, c_pmx = v.min(axis=0), s + v.argmin(axis=0), v.max(axis=0), s + v.argmax(axis=0)
                if first:
                    mn, pmn, mx, pmx = c_mn, c_pmn, c_mx, c_pmx
                else:         # ... and between chunks: the first chunk keeps a tie
                    lt, gt = c_mn < mn, c_mx > mx
                    mn, pmn = np.where(lt, c_mn, mn), np.where(lt, c_pmn, pmn)
                    mx, pmx = np.where(gt, c_mx, mx), np.where(gt, c_pmx, pmx)
        if "sum" in blocks:
            blocks["sum"][row] = s0 + nf * q
        if "mean" in blocks:
            blocks["mean"][row] = s0 / nf + q
        if "min" in blocks:
            blocks["min"][row], arg_min[row] = mn + q, eid[pmn]
        if "max" in blocks:
            blocks["max"][row], arg_max[row] = mx + q, eid[pmx]
        if need_mom:
            m1 = s1 / nf
            t = s2 / nf - m1 * m1
            v = np.where(t > 0, t, dtype(0))
            if "var" in blocks:
                blocks["var"][row] = v
            if "std" in blocks:
                blocks["std"][row] = np.sqrt(v + eps)
            mu[row], var[row] = shift + m1, v
    return dict(agg=np.concatenate([blocks[a] for a in aggregators], axis=1), arg_min=arg_min, arg_max=arg_max, mu=mu, var=var)


def aggregate_backward(dagg, ei, aggregators, P=None, fwd=None, chunk=CHUNK, dtype=np.float32, n_src=None):
    """(d P [n_src, W], d Q [N, W]) from d agg [N, A W] and the forward's dict, in the documented order: the destination pass
    (d Q and the records a, b), then per source the four plain sums over the transposed CSR and d P = ((A + P B) + Mn) + Mx."""
    aggregators = list(aggregators)
    dagg = np.asarray(dagg, dtype=dtype)
    n, w = dagg.shape[0], dagg.shape[1] // len(aggregators)
    n_src = n if n_src is None else int(n_src)
    g = {a: dagg[:, k * w:(k + 1) * w] for k, a in enumerate(aggregators)}
    rowptr, col, eid = csr_by_destination(ei, n)
    deg = np.diff(rowptr)
    live = (deg > 0)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        nf = deg.astype(dtype)[:, None]
        zero = np.zeros((n, w), dtype=dtype)
        dq, a = zero.copy(), zero.copy()
        if "sum" in g:
            dq, a = dq + nf * g["sum"], a + g["sum"]
        if "mean" in g:
            dq, a = dq + g["mean"], a + g["mean"] / nf
        if "min" in g:
            dq = dq + g["min"]
        if "max" in g:
            dq = dq + g["max"]
        b = None
        if "var" in g or "std" in g:
            c, v = zero.copy(), np.asarray(fwd["var"], dtype=dtype)
            if "var" in g:
                c = c + g["var"]
            if "std" in g:
                c = c + g["std"] / (dtype(2) * np.sqrt(v + dtype(1e-5)))
            c = np.where(v > 0, c, dtype(0))          # a variance of exactly 0 takes no gradient (relu'(0) = 0)
            b = (dtype(2) * c) / nf
            a = a - b * np.asarray(fwd["mu"], dtype=dtype)
            b = np.where(live, b, dtype(0))
        dq, a = np.where(live, dq, dtype(0)), np.where(live, a, dtype(0))
    has_lin = bool({"sum", "mean", "var", "std"} & set(aggregators))
    row_of = np.repeat(np.arange(n), deg)                               # destination of every forward CSR position
    t_order = np.argsort(col, kind="stable")                            # forward positions grouped by source, ascending inside
    t_rowptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n_src), out=t_rowptr[1:])
    dP = np.zeros((n_src, w), dtype=dtype)
    P = None if P is None else np.asarray(P, dtype=dtype)
    for j in range(n_src):
        q0, q1 = int(t_rowptr[j]), int(t_rowptr[j + 1])
        if q1 == q0:
            continue
        acc = {}
        for s in range(q0, q1, chunk):
            p = t_order[s:min(s + chunk, q1)]
            i = row_of[p]
            part = {}
            if has_lin:
                part["a"] = _seq_sum(a[i])
            if b is not None:
                part["b"] = _seq_sum(b[i])
            for side in ("min", "max"):
                if side in g:
                    arg = fwd["arg_" + side]
                    part[side] = _seq_sum(np.where(arg[i] == eid[p][:, None], g[side][i], dtype(0)))
            acc = part if s == q0 else {k: acc[k] + part[k] for k in part}
        d = acc["a"] if has_lin else np.zeros(w, dtype=dtype)
        if b is not None:
            d = d + P[j] * acc["b"]
        for side in ("min", "max"):
            if side in g:
                d = d + acc[side]
        dP[j] = d
    return dP, dq


def scale_factors(indeg, scalers, avg_lin, avg_log, dtype=np.float32):
    """[N, S] factors of rows with ``indeg`` in-edges: formed in float64 on d = max(n, 1), rounded once to ``dtype``."""
    d = np.maximum(np.asarray(indeg), 1).astype(np.float64)
    table = dict(identity=lambda: np.ones_like(d), amplification=lambda: np.log(d + 1.0) / avg_log,
                 attenuation=lambda: avg_log / np.log(d + 1.0), linear=lambda: d / avg_lin, inverse_linear=lambda: avg_lin / d)
    return np.stack([table[s]() for s in scalers], axis=1).astype(dtype)


def scale_combine(Y, base, indeg, scalers, avg_lin, avg_log, dtype=np.float32):
    """out = base, then out = out + f_k * Y[:, k D : (k + 1) D] in list order."""
    Y, out = np.asarray(Y, dtype=dtype), np.asarray(base, dtype=dtype).copy()
    f, dim = scale_factors(indeg, scalers, avg_lin, avg_log, dtype), out.shape[1]
    for k in range(len(scalers)):
        out = out + f[:, k:k + 1] * Y[:, k * dim:(k + 1) * dim]
    return out


def scale_combine_backward(gout, indeg, scalers, avg_lin, avg_log, dtype=np.float32):
    gout = np.asarray(gout, dtype=dtype)
    f = scale_factors(indeg, scalers, avg_lin, avg_log, dtype)
    return np.concatenate([f[:, k:k + 1] * gout for k in range(len(scalers))], axis=1)


def folded_from_params(params, meta):
    """fold_weights (egc_amd/_pna.py) on a dict of PyG-named parameters (torch tensors of any dtype)."""
    t = meta["towers"]
    return fold_weights([params[f"pre_nns.{k}.0.weight"] for k in range(t)], [params[f"pre_nns.{k}.0.bias"] for k in range(t)],
                        [params[f"post_nns.{k}.0.weight"] for k in range(t)], [params[f"post_nns.{k}.0.bias"] for k in range(t)],
                        params["lin.weight"], params["lin.bias"], len(meta["aggregators"]), len(meta["scalers"]), meta["divide_input"])


class _RefAggregate(torch.autograd.Function):
    """aggregate_forward / aggregate_backward (numpy, the tensors' dtype) as an autograd node on the CPU."""

    @staticmethod
    def forward(ctx, P, Q, ei, aggregators, chunk):
        Pn = P.detach().numpy()
        dtype = Pn.dtype.type
        fwd = aggregate_forward(Pn, Q.detach().numpy(), ei, aggregators, chunk, dtype)
        ctx.saved = (ei, aggregators, chunk, fwd, dtype, Pn)
        return torch.from_numpy(fwd["agg"])

    @staticmethod
    def backward(ctx, dagg):
        ei, aggregators, chunk, fwd, dtype, Pn = ctx.saved
        dP, dQ = aggregate_backward(dagg.numpy(), ei, aggregators, Pn, fwd, chunk, dtype)
        return torch.from_numpy(dP), torch.from_numpy(dQ), None, None, None


class _RefCombine(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, base, indeg, scalers, avg_lin, avg_log):
        dtype = Y.detach().numpy().dtype.type
        ctx.saved = (indeg, scalers, avg_lin, avg_log, dtype)
        return torch.from_numpy(scale_combine(Y.detach().numpy(), base.detach().numpy(), indeg, scalers, avg_lin, avg_log, dtype))

    @staticmethod
    def backward(ctx, gout):
        indeg, scalers, avg_lin, avg_log, dtype = ctx.saved
        return torch.from_numpy(scale_combine_backward(gout.numpy(), indeg, scalers, avg_lin, avg_log, dtype)), gout, None, None, None, None


def layer_forward(x, ei, params, meta, chunk=CHUNK):
    """The layer through the P / Q split, the restated kernels and the folded post-transform, on the CPU in the dtype of ``x``
    (torch tensors; differentiable with respect to x and every parameter)."""
    w_pq, b_pq, w_y, w_base, b_base = folded_from_params(params, meta)
    w = w_pq.shape[0] // 2
    pq = x @ w_pq.t() + b_pq
    agg = _RefAggregate.apply(pq[:, :w].contiguous(), pq[:, w:].contiguous(), ei, tuple(meta["aggregators"]), chunk)
    indeg = np.bincount(np.asarray(ei[1]), minlength=x.shape[0])
    return _RefCombine.apply(agg @ w_y.t(), x @ w_base.t() + b_base, indeg, tuple(meta["scalers"]), meta["avg_lin"], meta["avg_log"])
