"""Fixtures and CPU restatement of the neighbour sum under GCNConv, SAGEConv and GINConv (tests/golden/gnn/*.npz, written by
tests/golden/make_golden_gnn.py from a per-edge torch composition of the layers' published formulas).

``nbr_sum`` is sequential numpy in one dtype in the documented order of egc_amd/csrc/egc_nbr_sum.hip over a CSR (rowptr, col):
a row's entries are cut into consecutive chunks of ``chunk`` entries counted from its first entry, a chunk's sum is
((0 + t0) + t1) + ..., the row's sum is chunk 0's with the sums of chunks 1, 2, ... added in ascending order; a term's product or
division and every step of the finish are one correctly rounded IEEE operation -- so in float32 these ARE the kernel's bits.

    sum      t_p = x[col[p]]                          out_i = agg_i + s x_self_i
    mean     t_p = x[col[p]]                          out_i = agg_i / deg_i + s x_self_i     (an empty row: agg = 0, no division)
    mean_t   t_p = x[col[p]] / max(deg_of(col[p]), 1)     out_i = agg_i + s x_self_i
    sym      t_p = e_p x[col[p]]                      out_i = r_i (agg_i + r_i x_self_i)      e_p = edge_scale[p] or src_scale[col[p]]

(without x_self: agg, agg / deg, agg, r agg).  ``skip``: an entry with col[p] == i keeps its place in the chunk layout and
contributes nothing.  ``nbr_sum_plain`` is the same mathematics through a dense [rows, sources] count matrix, no chunks, float64.
The transposed CSR (``transposed_csr``) keeps a row's entries in ascending forward position, as CSRGraph.transposed() does."""
import json
import os

import numpy as np

from mpnn_ref import CHUNK, csr_by_destination, ladder_graph, rel_grad, rel_out  # noqa: F401  (the tests import them from here)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gnn")
CASES = ("gcn_messy_narrow_in", "gcn_messy_wide_in", "gcn_hub", "gcn_norm_only", "gcn_loops_only", "gcn_plain_sum",
         "sage_mean_messy", "sage_mean_hub", "sage_sum", "sage_no_root", "sage_normalize", "gin_train_eps", "gin_hub", "gin_buffer_eps")
FORMS = ("sum", "mean", "mean_t", "sym")
TRANSPOSE = {"sum": "sum", "mean": "mean_t", "mean_t": "mean", "sym": "sym"}


def load_gnn_golden(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        z = {k: z[k] for k in z.files}
    meta = json.loads(bytes(z["meta"]).decode())
    g = dict(meta=meta, name=name, x=z["x"], ei=z["edge_index"], gout=z["gout"], out32=z["out32"], out64=z["out64"],
             grad_x64=z["grad_x64"])
    g["params"] = {k[len("param:"):]: v for k, v in z.items() if k.startswith("param:")}
    g["grad64"] = {k[len("grad64:"):]: v for k, v in z.items() if k.startswith("grad64:")}
    return g


def build_layer(g):
    """The egc_amd module of a fixture, with fresh parameters."""
    import torch

    import egc_amd
    m = g["meta"]
    opt, fin, fout = m["options"], m["in_channels"], m["out_channels"]
    if m["layer"] == "gcn":
        return egc_amd.GCNConv(fin, fout, **opt)
    if m["layer"] == "sage":
        return egc_amd.SAGEConv(fin, fout, **opt)
    dims = [fin] + list(opt["hidden"]) + [fout]
    mods = []
    for k in range(len(dims) - 1):      # Sequential(Linear, ReLU, Linear, ...)
        mods += [torch.nn.Linear(dims[k], dims[k + 1])] + ([torch.nn.ReLU()] if k + 2 < len(dims) else [])
    return egc_amd.GINConv(torch.nn.Sequential(*mods), eps=opt["eps"], train_eps=opt["train_eps"])


def transposed_csr(rowptr, col, n_src):
    """(t_rowptr [n_src + 1], t_col = the row of every entry) of the transposed CSR, a row's entries in ascending forward position"""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    row_of = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))
    order = np.argsort(col, kind="stable")
    t_rowptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n_src), out=t_rowptr[1:])
    return t_rowptr, row_of[order]


def dis_tables(rowptr, col):
    """(dis_raw, dis_looped) of a square CSR: indeg^-1/2 over the entries as given (0 where indeg = 0) and
    (non-self indeg + 1)^-1/2, in float64 (CSRGraph's tables are these rounded to float32)"""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    deg = np.diff(rowptr).astype(np.float64)
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    non_self = np.bincount(row_of[col != row_of], minlength=n).astype(np.float64)
    with np.errstate(divide="ignore"):
        raw = np.where(deg > 0, deg ** -0.5, 0.0)
    return raw, (non_self + 1.0) ** -0.5


def nbr_sum(x, rowptr, col, form, x_self=None, s=1.0, skip=False, deg_rowptr=None, row_scale=None, src_scale=None,
            edge_scale=None, chunk=CHUNK, dtype=np.float32):
    """out [rows, d] in the documented order; every operand is rounded to ``dtype`` first (s too: pass 1 + eps formed in dtype)."""
    assert form in FORMS
    x = np.asarray(x, dtype=dtype)
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n, d = len(rowptr) - 1, x.shape[1]
    s = dtype(s)
    if x_self is not None:
        x_self = np.asarray(x_self, dtype=dtype)
    if form == "mean_t":
        inv = np.maximum(np.diff(np.asarray(deg_rowptr, dtype=np.int64)), 1).astype(dtype)
    if form == "sym":
        r = np.asarray(row_scale, dtype=dtype)
        e = np.asarray(edge_scale, dtype=dtype) if edge_scale is not None else np.asarray(src_scale, dtype=dtype)[col]
    out = np.zeros((n, d), dtype=dtype)
    for row in range(n):
        p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
        total = np.zeros(d, dtype=dtype)
        for k, c0 in enumerate(range(p0, p1, chunk)):
            acc = np.zeros(d, dtype=dtype)
            for p in range(c0, min(c0 + chunk, p1)):
                j = col[p]
                if skip and j == row:
                    continue
                if form == "mean_t":
                    t = x[j] / inv[j]
                elif form == "sym":
                    t = e[p] * x[j]
                else:
                    t = x[j]
                acc = acc + t
            total = acc if k == 0 else total + acc
        if form == "mean" and p1 > p0:
            total = total / dtype(p1 - p0)
        if form == "sym":
            if x_self is not None:
                total = total + r[row] * x_self[row]
            total = r[row] * total
        elif x_self is not None:
            total = total + s * x_self[row]
        out[row] = total
    return out


def nbr_sum_plain(x, rowptr, col, form, x_self=None, s=1.0, skip=False, deg_rowptr=None, row_scale=None, src_scale=None,
                  edge_scale=None):
    """The same mathematics without the order: a dense [rows, sources] matrix of the entries' weights times x, float64."""
    x = np.asarray(x, dtype=np.float64)
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    row_of = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    w = np.ones(len(col), dtype=np.float64)
    if form == "mean_t":
        w = w / np.maximum(np.diff(np.asarray(deg_rowptr, dtype=np.int64)), 1)[col]
    if form == "sym":
        w = np.asarray(edge_scale, dtype=np.float64) if edge_scale is not None else np.asarray(src_scale, dtype=np.float64)[col]
    if skip:
        w = np.where(col == row_of, 0.0, w)
    A = np.zeros((n, x.shape[0]), dtype=np.float64)
    np.add.at(A, (row_of, col), w)
    out = A @ x
    if form == "mean":
        out = out / np.maximum(np.diff(rowptr), 1)[:, None]
    xs = np.asarray(x_self, dtype=np.float64) if x_self is not None else None
    if form == "sym":
        r = np.asarray(row_scale, dtype=np.float64)[:n, None]
        return r * (out + r * xs) if xs is not None else r * out
    return out + float(s) * xs if xs is not None else out


def nbr_sum_transposed(dout, rowptr, col, n_src, form, shared_self=False, s=1.0, skip=False, scale=None, chunk=CHUNK,
                       dtype=np.float32):
    """d x [n_src, d] of ``nbr_sum(x, rowptr, col, form, ...)`` from d out, as the package computes it: the transposed form on the
    transposed CSR (mean -> mean_t with the forward rowptr, mean_t -> mean, sym -> sym with the same table gathered per entry),
    and with ``shared_self`` (x_self was x) the self term of the same pass."""
    t_rowptr, t_col = transposed_csr(rowptr, col, n_src)
    return nbr_sum(dout, t_rowptr, t_col, TRANSPOSE[form], x_self=dout if shared_self else None, s=s, skip=skip,
                   deg_rowptr=rowptr if form == "mean" else None, row_scale=scale, src_scale=scale, chunk=chunk, dtype=dtype)
