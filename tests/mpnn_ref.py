"""Fixtures and CPU restatement of the baseline MPNN layer (tests/golden/mpnn/*.npz, written by tests/golden/make_golden_mpnn.py
from the reference's own Mpnn, experiments/layers.py:231-267).

The algebra.  T towers, d = in_dim = out_dim, c = d / T.  message_layer[t].weight is [c, 2 c] = [Wd_t | Ws_t]: the first half
multiplies the target slice x_i^t, the second the source slice x_j^t.  With BD the block diagonal of the tower blocks,

    P = x BD(Ws)^T  [N, d]        Q = x BD(Wd)^T + b_msg  [N, d]

and for a row i with deg_i in-edges, in edge-list order, no self loops added:

    add   m_i = (sum_j P_j) + deg_i Q_i      mean   m_i = (sum_j P_j) / deg_i + Q_i      max   m_i = max_j P_j + Q_i

0 for deg_i = 0; for max the argument is the first edge in edge-list order attaining the maximum (duplicates are separate
entries), -1 for an empty row.  out_i = lin(BD(Wu) [m_i^t | x_i^t]_t + b_upd), and update and lin fold into one [d, 2 d] product.

``message_forward`` / ``message_backward`` are sequential numpy in one dtype in the documented order of egc_amd/csrc/egc_mpnn.hip:
a row's entries are cut into consecutive chunks of ``chunk`` entries counted from its first entry, a chunk's sum is
((0 + v0) + v1) + ..., the row's sum is chunk 0's with the sums of chunks 1, 2, ... added in ascending order, then the division
(mean), then the self term agg + s * Q -- every step one correctly rounded IEEE operation, so in float32 these ARE the kernels'
bits.  The backward sums d P_j over j's out-edges in the order of the transposed CSR: ascending position in the forward CSR
(by destination, then edge-list order).  Both take rectangular graphs (P and d P have the rows the sources name).

The end of the file holds the generated sweep graph (``ladder_graph``, ``ladder_inputs``, ``WIDTHS``) that
tests/test_mpnn_shapes_*.py and tests/test_typed_mean_shapes_*.py run the kernels on; tests/rgcn_ref.py imports it from here."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mpnn")
CHUNK = 256
CASES = ("messy_add", "messy_mean", "messy_max", "hub_add", "hub_max", "ties_max", "odd_add", "odd_max", "w116_max", "t1_mean")
MAX_CASES = tuple(c for c in CASES if c.endswith("_max"))


def load_mpnn_golden(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        z = {k: z[k] for k in z.files}
    meta = json.loads(bytes(z["meta"]).decode())
    g = dict(meta=meta, name=name, x=z["x"], ei=z["edge_index"], gout=z["gout"], out32=z["out32"], out64=z["out64"],
             grad_x64=z["grad_x64"], arg=z.get("arg"))
    g["params"] = {k[len("param:"):]: v for k, v in z.items() if k.startswith("param:")}
    g["init"] = {k[len("init:"):]: v for k, v in z.items() if k.startswith("init:")}
    g["grad64"] = {k[len("grad64:"):]: v for k, v in z.items() if k.startswith("grad64:")}
    return g


def rel_out(a, b):
    """max |a - b| relative to max(1, max |b|): the distance of outputs (tests/rgcn_ref.py)."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(1.0, float(np.abs(b).max())))


def rel_grad(a, b):
    """max |a - b| relative to max |b|: the distance of gradients."""
    b = np.asarray(b, dtype=np.float64)
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(1e-30, float(np.abs(b).max())))


def reference_distance(g):
    """The reference's own float32 against its float64 output on this fixture."""
    return rel_out(g["out32"], g["out64"])


def csr_by_destination(ei, n):
    """(rowptr, source of every entry, edge-list position of every entry), stable inside a row."""
    src, dst = np.asarray(ei[0]), np.asarray(ei[1])
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n), out=rowptr[1:])
    return rowptr, src[order], order


def message_forward(P, Q, ei, aggr, chunk=CHUNK, dtype=np.float32):
    """(m [N, d], arg [N, d] int32 -- edge-list positions, max only, else None) in the documented order.  P may have any number of
    rows (the rows the edges' sources name); N is Q's."""
    P, Q = np.asarray(P, dtype=dtype), np.asarray(Q, dtype=dtype)
    n, d = Q.shape
    rowptr, col, eid = csr_by_destination(ei, n)
    m = np.zeros((n, d), dtype=dtype)
    arg = np.full((n, d), -1, dtype=np.int32) if aggr == "max" else None
    for row in range(n):
        p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
        if p1 == p0:
            continue
        deg = dtype(p1 - p0)
        if aggr == "max":
            best = pos = None
            for s in range(p0, p1, chunk):               # strict > twice: the first entry keeps a tie inside a chunk ...
                c_best, c_pos = np.full(d, -np.inf, dtype=dtype), np.full(d, s, dtype=np.int64)
                for p in range(s, min(s + chunk, p1)):
                    v = P[col[p]]
                    better = v > c_best
                    c_best, c_pos = np.where(better, v, c_best), np.where(better, p, c_pos)
                if best is None:
                    best, pos = c_best, c_pos
                else:                                    # ... and the first chunk keeps one between chunks
                    better = c_best > best
                    best, pos = np.where(better, c_best, best), np.where(better, c_pos, pos)
            m[row], arg[row] = best + Q[row], eid[pos]
            continue
        total = None
        for s in range(p0, p1, chunk):
            acc = np.zeros(d, dtype=dtype)
            for p in range(s, min(s + chunk, p1)):
                acc = acc + P[col[p]]
            total = acc if total is None else total + acc
        m[row] = total + deg * Q[row] if aggr == "add" else total / deg + Q[row]
    return m, arg


def message_backward(dm, ei, aggr, arg=None, chunk=CHUNK, dtype=np.float32, n_src=None):
    """(d P [n_src, d], d Q [N, d]) from d m [N, d] in the documented order over the transposed CSR.  ``n_src``: the rows of P
    (None: a square graph, N)."""
    dm = np.asarray(dm, dtype=dtype)
    n, d = dm.shape
    n_src = n if n_src is None else int(n_src)
    rowptr, col, eid = csr_by_destination(ei, n)
    deg = np.diff(rowptr)
    row_of = np.repeat(np.arange(n), deg)                               # destination of every forward CSR position
    t_order = np.argsort(col, kind="stable")                            # forward positions grouped by source, ascending inside
    t_rowptr = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n_src), out=t_rowptr[1:])
    dP = np.zeros((n_src, d), dtype=dtype)
    for j in range(n_src):
        total = None
        for s in range(int(t_rowptr[j]), int(t_rowptr[j + 1]), chunk):
            acc = np.zeros(d, dtype=dtype)
            for q in range(s, min(s + chunk, int(t_rowptr[j + 1]))):
                p = t_order[q]
                i = row_of[p]
                if aggr == "add":
                    v = dm[i]
                elif aggr == "mean":
                    v = dm[i] / dtype(deg[i])
                else:
                    v = np.where(arg[i] == eid[p], dm[i], dtype(0))
                acc = acc + v
            total = acc if total is None else total + acc
        if total is not None:
            dP[j] = total
    s = deg.astype(dtype) if aggr == "add" else (deg > 0).astype(dtype)
    return dP, s[:, None] * dm


def folded_weights(params, towers):
    """torch, differentiable: ([2 d, d], [2 d]) of x -> [P | Q] and ([d, 2 d], [d]) of [m | x] -> out from a dict of the
    reference's parameters."""
    msg_w = [params[f"message_layer.{t}.weight"] for t in range(towers)]
    upd_w = [params[f"update_layer.{t}.weight"] for t in range(towers)]
    c = msg_w[0].shape[1] // 2
    w_pq = torch.cat([torch.block_diag(*[w[:, c:] for w in msg_w]), torch.block_diag(*[w[:, :c] for w in msg_w])], dim=0)
    b_msg = torch.cat([params[f"message_layer.{t}.bias"] for t in range(towers)])
    b_pq = torch.cat([torch.zeros_like(b_msg), b_msg])
    w_upd = torch.cat([torch.block_diag(*[w[:, :c] for w in upd_w]), torch.block_diag(*[w[:, c:] for w in upd_w])], dim=1)
    lin_w = params["lin.weight"]
    b_out = lin_w @ torch.cat([params[f"update_layer.{t}.bias"] for t in range(towers)]) + params["lin.bias"]
    return w_pq, b_pq, lin_w @ w_upd, b_out


class _RefMessage(torch.autograd.Function):
    """message_forward / message_backward (numpy, the tensors' dtype) as an autograd node on the CPU."""

    @staticmethod
    def forward(ctx, P, Q, ei, aggr, chunk):
        dtype = P.detach().numpy().dtype.type
        m, arg = message_forward(P.detach().numpy(), Q.detach().numpy(), ei, aggr, chunk, dtype)
        ctx.saved = (ei, aggr, chunk, arg, dtype)
        return torch.from_numpy(m)

    @staticmethod
    def backward(ctx, dm):
        ei, aggr, chunk, arg, dtype = ctx.saved
        dP, dQ = message_backward(dm.numpy(), ei, aggr, arg, chunk, dtype)
        return torch.from_numpy(dP), torch.from_numpy(dQ), None, None, None


def layer_forward(x, ei, params, towers, aggr, chunk=CHUNK):
    """The layer through the P / Q split and the folded update, on the CPU in the dtype of ``x`` (torch tensors; differentiable
    with respect to x and every parameter)."""
    w_pq, b_pq, w_out, b_out = folded_weights(params, towers)
    d = x.shape[1]
    pq = x @ w_pq.t() + b_pq
    m = _RefMessage.apply(pq[:, :d].contiguous(), pq[:, d:].contiguous(), ei, aggr, chunk)
    return torch.cat([m, x], dim=1) @ w_out.t() + b_out


# ------------------------------------------------------------------------------------------------------------------------------
# The sweep graph of tests/test_mpnn_shapes_*.py and tests/test_typed_mean_shapes_*.py: a LADDER of row lengths, one row of each,
# laid out so that the long rows (more than CHUNK entries) start where the chunk kernels' slot arithmetic has its edges.

LADDER = (0, 1, 7, 8, 9, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK, 2 * CHUNK + 18)
PAD, FILL = 32, 5            # the padding rows' length; the one extra row of ``pad_to_chunk`` (neither is a ladder length)
# rows in CSR order: a ladder length, or ("pad", k) = k rows of PAD entries.  Start of every long row (position, mod CHUNK):
_LAYOUT = (CHUNK + 1,                                   # row 0: 0
           2 * CHUNK + 1,                               # 257 = 1: one past a slot boundary, adjacent to a long row
           CHUNK - 1, 15, 8, 7, ("pad", 7),
           2 * CHUNK - 1,                               # 1279 = CHUNK - 1: one before a slot boundary
           1, 16, 17, ("pad", 7),
           2 * CHUNK,                                   # 2048 = 0: on a slot boundary, and its every chunk too
           3 * CHUNK,                                   # 2560 = 0: adjacent again
           9, 0, CHUNK, ("pad", 56),
           2 * CHUNK + 18)                              # the last row
WIDTHS = (1, 2, 3, 4, 5, 12, 64, 100, 116, 128, 256, 260, 1028, 1030)     # the width sweep (8 and 6: the degree sweep)


def ladder_lengths(tail_empty=False, pad_to_chunk=False, max_len=None, prepend=0):
    """The row lengths of the sweep graph in CSR order (ladder_graph's arguments)."""
    rows = [1] * int(prepend)
    for item in _LAYOUT:
        rows += [PAD] * item[1] if isinstance(item, tuple) else [item]
    if max_len is not None:
        rows = [r for r in rows if r <= max_len]
    if pad_to_chunk:
        need = -sum(rows) % CHUNK
        extra = [PAD] * (need // PAD) + ([need % PAD] if need % PAD else [])
        assert not set(extra) & set(LADDER)
        rows[-1:-1] = extra
    return rows + [0] * (3 if tail_empty else 0)


def ladder_graph(seed, flip=False, tail_empty=False, pad_to_chunk=False, square=False, max_len=None, prepend=0):
    """(edge_index [2, E] int64, n_dst, n_src): destinations carry one row of every LADDER length between padding rows of PAD
    entries (_LAYOUT: row 0 and the last row long, long rows starting at positions = 0, 1 and CHUNK - 1 mod CHUNK, two pairs of
    adjacent long rows, an empty row between non-empty ones), sources uniform over n_src = 3 n_dst / 2 (``square``: n_dst), the
    edge list permuted -- so duplicates, self loops, and a CSR that only a stable sort gets right.  ``tail_empty``: three empty
    rows after the last one.  ``pad_to_chunk``: FILL- and PAD-entry rows before the last row until the entry count is a multiple
    of CHUNK (it is not otherwise).  ``max_len``: without the rows longer than that.  ``prepend``: that many one-entry rows first.
    ``flip``: the two rows of edge_index, and n_dst and n_src, swapped -- the ladder is in the out-degrees then."""
    rng = np.random.default_rng(seed)
    lengths = np.array(ladder_lengths(tail_empty, pad_to_chunk, max_len, prepend), dtype=np.int64)
    n_dst = len(lengths)
    n_src = n_dst if square else (3 * n_dst) // 2
    dst = np.repeat(np.arange(n_dst, dtype=np.int64), lengths)
    src = rng.integers(0, n_src, len(dst)).astype(np.int64)
    ei = np.ascontiguousarray(np.stack([src, dst])[:, rng.permutation(len(dst))])
    return (np.ascontiguousarray(ei[::-1]), n_src, n_dst) if flip else (ei, n_dst, n_src)


def ladder_inputs(n_dst, n_src, width, seed, ties=False):
    """(P [n_src, width], Q [n_dst, width], d m [n_dst, width]) float32 standard normals.  ``ties``: P holds the integers
    -2 .. 2 instead, so nearly every (row, column) maximum is attained by several edges, in several chunks of a long row."""
    rng = np.random.default_rng(seed)
    P, Q, dm = (rng.standard_normal((n, width)).astype(np.float32) for n in (n_src, n_dst, n_dst))
    if ties:
        P = rng.integers(-2, 3, (n_src, width)).astype(np.float32)
    return P, Q, dm


def tie_counts(P, ei, n_dst, chunk=CHUNK):
    """(the (row, column) pairs whose maximum of P over the row's entries is attained by more than one edge, those where it is
    attained in more than one chunk of the row)"""
    rowptr, col, _ = csr_by_destination(ei, n_dst)
    edges = chunks = 0
    for row in range(n_dst):
        p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
        if p1 == p0:
            continue
        v = np.asarray(P)[col[p0:p1]]
        at = v == v.max(axis=0)                                                   # [entries, width]
        edges += int((at.sum(axis=0) > 1).sum())
        per_chunk = np.add.reduceat(at, np.arange(0, p1 - p0, chunk), axis=0) > 0     # [chunks, width]
        chunks += int((per_chunk.sum(axis=0) > 1).sum())
    return edges, chunks
