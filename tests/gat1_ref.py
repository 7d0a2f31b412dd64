"""Fixtures and CPU restatement of GATConv, GAT v1 (tests/golden/gat1/*.npz, written by tests/golden/make_golden_gat1.py from a
plain per-edge torch composition of the PyG formulas).

``aggregate_forward`` / ``aggregate_backward`` are sequential numpy in one dtype in the KERNEL's formulation
(egc_amd/csrc/egc_gat.hip).  Forward: a row's entries in CSR order (by destination, edge-list order inside a row), the entries
whose source equals the row skipped when self loops are added, cut into chunks of ``chunk`` entries counted from the row's
first entry (skipped entries keep their place); inside a chunk an online softmax in batches of ``ahead`` entries over the scores
s = leaky_relu(a_src[j] + a_dst[i]); the chunk states merged in ascending order; the self entry LAST; out = acc / l,
lse = m + log l (0 and -inf for a row without entries).  Backward, nothing per-edge kept: alpha = exp(s - lse_i),
w = alpha leaky_relu'(a_src[j] + a_dst[i]), D_i = g_i . out_i per head, and
    destination pass (CSR), FACTORED    v_i = sum_j w_ij xl_j,  t_i = sum_j w_ij,           d a_dst[i] = g_i . v_i - D_i t_i
    source pass (transposed CSR)        d xl_j = sum_i alpha_ij g_i,  d a_src[j] = sum_i w_ij (g_i . xl_j - D_i)  (d s per entry)
each sum per chunk from zero in entry order, the chunks added in ascending order, the self entry last.

``SWEEP_SHAPES`` / ``geometry`` / ``sweep_reference``: the (H, C) table of the geometry sweep (tests/test_gat1_shapes_cpu.py
guards the table, tests/test_gat1_shapes_gpu.py runs the kernels over it) on gat_ref's sweep graph, which needs no fixture: the
restatement above is its float64 truth and, in float32, its yardstick."""
import functools
import json
import os

import numpy as np
import torch

from gat_ref import sweep_graph  # noqa: F401  (re-exported: the graph of the sweep)
from mpnn_ref import csr_by_destination, rel_grad, rel_out  # noqa: F401  (re-exported: the distances of the bound)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gat1")
CHUNK = 256
AHEAD = 8
CASES = ("messy", "hub", "w152h8", "w152h1", "w240h8", "w304h1", "mean", "noloops", "bigscore", "slope", "nobias")
SHAPES = dict(messy=(4, 5), hub=(2, 4), w152h8=(8, 19), w152h1=(1, 152), w240h8=(8, 30), w304h1=(1, 304), mean=(3, 6), noloops=(4, 5),
              bigscore=(2, 8), slope=(2, 8), nobias=(2, 8))
REFERENCE_SHAPES = ((8, 19), (1, 152), (8, 30), (1, 240), (8, 38), (1, 304))      # the arxiv, mol and code nets' blocks

# (H, C) of the geometry sweep: every template instance (S, VEC, SMALL) and every group size G of egc_gat.hip, the places where
# a head's sum (D and g . v at the row's end, g . xl per entry) straddles lanes or crosses column 256 (slot 0 / slot 1), and the reference's shapes.
# Columns 4 v .. 4 v + 3 belong to virtual lane v.  C >= 4: a lane reads the per-head scalars of its first and its last column
# (two heads at the most); C < 4: of all four.
SWEEP_SHAPES = (
    # ---- S = 1 (H C <= 256)
    (1, 1),      # G 1, SMALL, scalar: one live column of the lane's four
    (4, 1),      # G 1, SMALL, 16-byte rows: four heads in one lane
    (1, 4),      # G 1, 16-byte rows: a head is exactly one lane
    (2, 3),      # G 2, SMALL, scalar: head 1 = columns 3..5 straddles lanes 0 and 1
    (4, 2),      # G 2, SMALL, 16-byte rows: two heads per lane
    (3, 3),      # G 4 with one idle lane, SMALL, scalar
    (16, 2),     # G 8, SMALL, 16-byte rows
    (12, 5),     # G 16 with one idle lane, 16-byte rows: C mod 4 = 1, a head starts at every phase of a quad
    (9, 7),      # G 16, scalar: 63 columns, the last lane has three live columns
    (4, 25),     # G 32, 16-byte rows: heads straddle, C mod 4 = 1
    (5, 21),     # G 32, scalar: 105 columns
    (3, 43),     # G 64, scalar: 129 columns on 33 lanes, 31 idle lanes
    (85, 3),     # G 64, SMALL, scalar: 255 columns
    (64, 4),     # G 64: every lane is a head of its own
    (1, 256),    # G 64: one head over the whole wavefront, the widest S = 1
    # ---- S = 2 (257 <= H C <= 512)
    (1, 257),    # scalar: one live column in slot 1, the head crosses 256 into it
    (1, 260),    # 16-byte rows: one live lane in slot 1
    (3, 100),    # head 2 = columns 200..299 crosses 256
    (8, 33),     # 16-byte rows: head 7 = columns 231..263 crosses 256, C mod 4 = 1
    (37, 13),    # scalar: head 19 = columns 247..259 crosses 256
    (2, 256),    # a head boundary exactly at column 256: head 1 is all of slot 1
    (128, 3),    # SMALL, 16-byte rows: head 85 = columns 255..257 crosses 256
    (170, 3),    # SMALL, scalar: 510 columns, the last virtual lane has two live columns
    (512, 1),    # SMALL, 16-byte rows: 512 heads of one column
) + REFERENCE_SHAPES


def geometry(h, c):
    """The kernels' launch geometry for (H, C), restated from gat_geom / gat_fill_walk (egc_gat_dev.h) and the host dispatch of
    egc_gat.hip: S slots per lane, G lanes per row (group), V = S G virtual lanes, seg = the head sum's scan limit, small = the
    C < 4 forms, vec_by_width = the width allows 16-byte accesses (pointers and strides permitting); spans_256 = some head has
    columns on both sides of column 256, boundary_256 = a head starts exactly at column 256; straddles = some head starts
    inside a lane's quad; ext_width = the columns of [xl | a_src | a_dst | pad]."""
    width = h * c
    lanes = (width + 3) // 4
    g = 1
    while g < lanes and g < 64:
        g *= 2
    s = 2 if lanes > 64 else 1
    return dict(S=s, G=g, V=s * g, seg=(c + 3) // 4 + 1, small=c < 4, vec_by_width=width % 4 == 0,
                spans_256=width > 256 and 256 % c != 0, boundary_256=width > 256 and 256 % c == 0,
                straddles=any((k * c) % 4 for k in range(h)), ext_width=(width + 2 * h + 3) // 4 * 4)


def workspace_bytes(h, c, n, e):
    """(forward, backward) workspace of the library for n rows and e entries, restated: per chunk slot and virtual lane three
    16-byte values forward (m, l, acc) and two + two backward ((v, t), (d xl, d a_src)), and D [n, H] rounded up to 16 bytes."""
    q = geometry(h, c)
    slots = -(-e // CHUNK) if e > CHUNK else 0
    return slots * q["V"] * 48, 4 * ((n * h + 3) // 4 * 4) + slots * q["V"] * 64


def sweep_inputs(h, c, n, seed):
    """xl, gout ~ N(0, 1) float32 [n, H C] and a_src, a_dst ~ N(0, 1) float32 [n, H]."""
    rng = np.random.default_rng(seed)
    xl, gout = (rng.standard_normal((n, h * c)).astype(np.float32) for _ in range(2))
    a_src, a_dst = (rng.standard_normal((n, h)).astype(np.float32) for _ in range(2))
    return xl, a_src, a_dst, gout


def load(name):
    with np.load(os.path.join(GOLDEN, f"{name}.npz")) as z:
        z = {k: z[k] for k in z.files}
    meta = json.loads(bytes(z["meta"]).decode())
    g = dict(meta=meta, name=name, x=z["x"], ei=z["edge_index"], gout=z["gout"], out32=z["out32"], out64=z["out64"],
             grad_x64=z["grad_x64"])
    g["params"] = {k[len("param:"):]: v for k, v in z.items() if k.startswith("param:")}
    g["grad64"] = {k[len("grad64:"):]: v for k, v in z.items() if k.startswith("grad64:")}
    return g


def layer_kwargs(g):
    m = g["meta"]
    return dict(in_channels=m["in_channels"], out_channels=m["channels"], heads=m["heads"], **m["kwargs"])


def _lrelu(z, slope):
    return np.where(z > 0, z, slope * z)


def _chunk_state(sources, row, xl, a_src, ad_i, slope, loops, ahead, dtype):
    h = ad_i.shape[0]
    m, l, acc = np.full(h, -np.inf, dtype=dtype), np.zeros(h, dtype=dtype), np.zeros(xl.shape[1:], dtype=dtype)
    for b in range(0, len(sources), ahead):
        live = [j for j in sources[b:b + ahead] if not (loops and j == row)]
        if not live:
            continue
        s = [_lrelu(a_src[j] + ad_i, dtype(slope)) for j in live]
        bm = np.maximum(m, np.max(s, axis=0))
        with np.errstate(invalid="ignore"):
            r = np.where(m == bm, dtype(1), np.exp(m - bm))
        l, acc = l * r, acc * r[:, None]
        for j, sj in zip(live, s):
            w = np.exp(sj - bm)
            l, acc = l + w, acc + w[:, None] * xl[j]
        m = bm
    return m, l, acc


def _merge(a, b):
    (m1, l1, a1), (m2, l2, a2) = a, b
    bm = np.maximum(m1, m2)
    with np.errstate(invalid="ignore"):
        r1, r2 = np.where(m1 == bm, 1.0, np.exp(m1 - bm)).astype(l1.dtype), np.where(m2 == bm, 1.0, np.exp(m2 - bm)).astype(l1.dtype)
    return bm, l1 * r1 + l2 * r2, a1 * r1[:, None] + a2 * r2[:, None]


def aggregate_forward(xl, a_src, a_dst, ei, slope=0.2, loops=True, chunk=CHUNK, ahead=AHEAD, dtype=np.float64):
    """(out [N, H C], lse [N, H]) in the kernel's formulation.  a_src: [rows of xl, H]; a_dst: [N, H]."""
    a_src, a_dst = np.asarray(a_src, dtype=dtype), np.asarray(a_dst, dtype=dtype)
    n, h = a_dst.shape
    xl = np.asarray(xl, dtype=dtype)
    c = xl.shape[1] // h
    xl = xl.reshape(-1, h, c)
    rowptr, col, _ = csr_by_destination(ei, n)
    out, lse = np.zeros((n, h, c), dtype=dtype), np.full((n, h), -np.inf, dtype=dtype)
    for row in range(n):
        p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
        state = _chunk_state([], row, xl, a_src, a_dst[row], slope, loops, ahead, dtype)
        for k, s0 in enumerate(range(p0, p1, chunk)):
            part = _chunk_state(list(col[s0:min(s0 + chunk, p1)]), row, xl, a_src, a_dst[row], slope, loops, ahead, dtype)
            state = part if k == 0 else _merge(state, part)
        if loops:
            state = _self_entry(state, xl[row], _lrelu(a_src[row] + a_dst[row], dtype(slope)), dtype)
        m, l, acc = state
        any_ = l > 0
        out[row] = np.where(any_[:, None], acc / np.where(any_, l, 1)[:, None], 0)
        lse[row] = np.where(any_, m + np.log(np.where(any_, l, 1)), -np.inf)
    return out.reshape(n, h * c), lse


def _self_entry(state, xl_i, s, dtype):
    """The self entry as a batch of one."""
    m, l, acc = state
    bm = np.maximum(m, s)
    r, w = np.where(m == bm, dtype(1), np.exp(m - bm)), np.exp(s - bm)
    return bm, l * r + w, acc * r[:, None] + w[:, None] * xl_i


def _chunked_sums(entries, row, loops, chunk, zero, term):
    """sum of term(k) over the row's entries k != row (when loops), each chunk summed from zero in entry order, the chunk sums
    added in ascending order, then term(row) when loops: the order of the kernel's backward sums."""
    total = None
    for s0 in range(0, max(len(entries), 1), chunk):
        part = [z.copy() for z in zero]
        for k in entries[s0:s0 + chunk]:
            if not (loops and k == row):
                part = [a + b for a, b in zip(part, term(int(k)))]
        total = part if total is None else [a + b for a, b in zip(total, part)]
    if loops:
        total = [a + b for a, b in zip(total, term(row))]
    return total


def aggregate_backward(xl, a_src, a_dst, ei, out, lse, gout, slope=0.2, loops=True, chunk=CHUNK, dtype=np.float64):
    """(d xl [N, H C], d a_src, d a_dst [N, H]) from d out, with the scores recomputed: the destination pass's sums factored, the
    source pass's d s per entry."""
    a_src, a_dst, lse = (np.asarray(a, dtype=dtype) for a in (a_src, a_dst, lse))
    n, h = a_dst.shape
    c = np.asarray(xl).shape[1] // h
    xl, out, g = (np.asarray(a, dtype=dtype).reshape(n, h, c) for a in (xl, out, gout))
    slope = dtype(slope)
    rowptr, col, _ = csr_by_destination(ei, n)
    D = (g * out).sum(axis=-1)

    def weights(j, i):
        z = a_src[j] + a_dst[i]
        alpha = np.exp(_lrelu(z, slope) - lse[i])
        return alpha, alpha * np.where(z > 0, dtype(1), slope)

    def dst_term(i):
        def term(j):
            w = weights(j, i)[1]
            return w[:, None] * xl[j], w
        return term

    def src_term(j):
        def term(i):
            alpha, w = weights(j, i)
            return alpha[:, None] * g[i], w * ((g[i] * xl[j]).sum(axis=-1) - D[i])
        return term

    dxl, das, dad = np.zeros((n, h, c), dtype=dtype), np.zeros((n, h), dtype=dtype), np.zeros((n, h), dtype=dtype)
    zc, zh = np.zeros((h, c), dtype=dtype), np.zeros(h, dtype=dtype)
    for i in range(n):                                   # destination pass: the forward CSR, the self entry last
        v, t = _chunked_sums(col[rowptr[i]:rowptr[i + 1]], i, loops, chunk, (zc, zh), dst_term(i))
        dad[i] = (g[i] * v).sum(axis=-1) - D[i] * t
    row_of = np.repeat(np.arange(n), np.diff(rowptr))
    order = np.argsort(col, kind="stable")               # source pass: the transposed CSR (ascending forward position)
    t_rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=t_rowptr[1:])
    for j in range(n):
        dests = row_of[order[t_rowptr[j]:t_rowptr[j + 1]]]
        dxl[j], das[j] = _chunked_sums(dests, j, loops, chunk, (zc, zh), src_term(j))
    return dxl.reshape(n, h * c), das, dad


def per_edge_backward(xl, a_src, a_dst, ei, out, lse, gout, slope=0.2, loops=True):
    """float64, the UNfactored form: d s_ij = alpha_ij (g_i . xl_j - D_i) per entry, scattered.  What the factored sums must equal."""
    a_src, a_dst, lse = (np.asarray(a, dtype=np.float64) for a in (a_src, a_dst, lse))
    n, h = a_dst.shape
    c = np.asarray(xl).shape[1] // h
    xl, out, g = (np.asarray(a, dtype=np.float64).reshape(n, h, c) for a in (xl, out, gout))
    src, dst = np.asarray(ei[0]), np.asarray(ei[1])
    if loops:
        keep = src != dst
        src, dst = np.concatenate([src[keep], np.arange(n)]), np.concatenate([dst[keep], np.arange(n)])
    z = a_src[src] + a_dst[dst]
    alpha = np.exp(_lrelu(z, slope) - lse[dst])
    ds = alpha * ((g[dst] * xl[src]).sum(axis=-1) - (g * out).sum(axis=-1)[dst]) * np.where(z > 0, 1.0, slope)
    dxl, das, dad = np.zeros_like(xl), np.zeros((n, h)), np.zeros((n, h))
    np.add.at(dxl, src, alpha[:, :, None] * g[dst])
    np.add.at(das, src, ds)
    np.add.at(dad, dst, ds)
    return dxl.reshape(n, h * c), das, dad


@functools.lru_cache(maxsize=None)
def sweep_reference(h, c, loops, n=40, graph_seed=5, input_seed=7):
    """{dtype: (out, lse, d xl, d a_src, d a_dst)} of the restatement on the sweep graph in float64 (the truth) and float32 (the
    yardstick), each backward fed its own forward's out and lse.  Computed once per shape; the arrays are read-only."""
    ei = sweep_graph(graph_seed, n)[0]
    xl, a_src, a_dst, gout = sweep_inputs(h, c, n, input_seed)
    ref = {}
    for dtype in (np.float64, np.float32):
        out, lse = aggregate_forward(xl, a_src, a_dst, ei, loops=loops, dtype=dtype)
        ref[dtype] = (out, lse) + aggregate_backward(xl, a_src, a_dst, ei, out, lse, gout, loops=loops, dtype=dtype)
        for a in ref[dtype]:
            a.setflags(write=False)
    return ref


def lse_distance(a, b):
    """(the -inf positions agree, max |a - b| over the finite entries relative to max(1, max |b|))"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fa, fb = np.isfinite(a), np.isfinite(b)
    same = np.array_equal(fa, fb) and np.array_equal(a[~fa], b[~fb])
    both = fa & fb
    return same, (rel_out(a[both], b[both]) if both.any() else 0.0)


QUANTITIES = ("out", "lse", "dxl", "das", "dad")
DISTANCE = dict(out=rel_out, lse=lambda a, b: lse_distance(a, b)[1], dxl=rel_grad, das=rel_grad, dad=rel_grad)


class _RefAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xl, a_src, a_dst, ei, slope, loops):
        a = [t.detach().numpy() for t in (xl, a_src, a_dst)]
        dtype = a[0].dtype.type
        out, lse = aggregate_forward(*a, ei, slope, loops, dtype=dtype)
        ctx.saved = (a, ei, slope, loops, out, lse, dtype)
        return torch.from_numpy(out)

    @staticmethod
    def backward(ctx, gout):
        a, ei, slope, loops, out, lse, dtype = ctx.saved
        dxl, das, dad = aggregate_backward(*a, ei, out, lse, gout.numpy(), slope, loops, dtype=dtype)
        return torch.from_numpy(dxl), torch.from_numpy(das), torch.from_numpy(dad), None, None, None


def layer_forward(x, ei, params, heads, channels, concat=True, negative_slope=0.2, add_self_loops=True, bias=True):
    """GATConv through the restatement, on the CPU in the dtype of x (torch; differentiable in x and every parameter)."""
    xl = x @ params["lin_src.weight"].t()
    xh = xl.view(-1, heads, channels)
    a_src, a_dst = (xh * params["att_src"]).sum(dim=-1), (xh * params["att_dst"]).sum(dim=-1)
    out = _RefAggregate.apply(xl, a_src, a_dst, ei, negative_slope, add_self_loops)
    if not concat:
        out = out.view(-1, heads, channels).mean(dim=1)
    return out + params["bias"] if bias else out
