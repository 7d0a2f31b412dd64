"""Fixtures and CPU restatement of GATv2Conv (tests/golden/gat/*.npz, written by tests/golden/make_golden_gat.py from a plain
per-edge torch composition of the PyG 2.x formulas).

``aggregate_forward`` / ``aggregate_backward`` are sequential numpy in one dtype in the KERNEL's formulation
(egc_amd/csrc/egc_gatv2.hip): a row's entries in CSR order (by destination, edge-list order inside a row), the entries whose
source equals the row skipped when self loops are added, cut into chunks of ``chunk`` entries counted from the row's first entry
(skipped entries keep their place); inside a chunk an online softmax in batches of ``ahead`` entries -- bm = max(m, the batch's
live scores), l = l exp(m - bm) + sum exp(s_k - bm), the accumulator likewise, m = bm; the chunk states merged in ascending
order; the self entry LAST; out = acc / l, lse = m + log l (0 and -inf for a row without entries).  Nothing per-edge is kept:
the backward recomputes z and s from xl, xr and att and uses alpha = exp(s - lse), D_i = g_i . out_i per head,
d s = alpha (g_i . xl_j - D_i), d z = d s att leaky_relu'(z): a destination pass (d xr, d att) over the CSR and a source pass
(d xl) over the transposed CSR, the self entry last in both.

``SWEEP_SHAPES`` / ``geometry`` / ``sweep_graph`` / ``sweep_inputs``: the (H, C) table of the geometry sweep
(tests/test_gat_shapes_cpu.py guards the table, tests/test_gat_shapes_gpu.py runs the kernels over it), which needs no fixture:
the restatement above is its float64 truth and, in float32, its yardstick."""
import json
import os

import numpy as np
import torch

from mpnn_ref import csr_by_destination, rel_grad, rel_out  # noqa: F401  (re-exported: the distances of the bound)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gat")
CHUNK = 256
AHEAD = 8
CASES = ("messy", "hub", "w104h1", "w112h8", "h8c13", "mean", "shared", "noloops", "bigscore", "slope")
SHAPES = dict(messy=(4, 5), hub=(2, 4), w104h1=(1, 104), w112h8=(8, 14), h8c13=(8, 13), mean=(3, 6), shared=(2, 8), noloops=(4, 5),
              bigscore=(2, 8), slope=(2, 8))


# (H, C) of the geometry sweep (tests/test_gat_shapes_*.py): every template instance (S, VEC, SMALL) and every group size G of
# egc_gatv2.hip, and the places where the per-head scan's lane bookkeeping changes.  Columns 4 v .. 4 v + 3 belong to virtual
# lane v; slot 1 (S = 2) starts at column 256.
SWEEP_SHAPES = (
    # ---- S = 1 (H C <= 256)
    (1, 1),      # G 1, SMALL: one live column of the lane's four
    (4, 1),      # G 1, SMALL, 16-byte rows: four heads in one lane
    (1, 3),      # G 1, SMALL, scalar: a head of three columns inside one lane
    (1, 4),      # G 1: the smallest scanned head, a segment of one lane (seg = 2)
    (1, 5),      # G 2, scalar: the head runs into a second lane with one live column
    (2, 3),      # G 2, SMALL, scalar: head 1 = columns 3..5 straddles lanes 0 and 1
    (4, 2),      # G 2, SMALL, 16-byte rows: two heads per lane, none straddles
    (3, 3),      # G 4 with one idle lane, SMALL, scalar: 9 columns on 3 lanes
    (16, 2),     # G 8, SMALL, 16-byte rows
    (7, 3),      # G 8 with two idle lanes, SMALL, scalar: heads straddle at every phase
    (12, 5),     # G 16 with one idle lane, 16-byte rows: C mod 4 = 1, every head start phase
    (9, 7),      # G 16, scalar: 63 columns, the last lane has three live columns, C mod 4 = 3
    (1, 64),     # G 16: one head over the whole group (scan distances 1 .. 16)
    (3, 43),     # G 64, scalar: 129 columns on 33 lanes, 31 idle lanes
    (5, 50),     # G 64, scalar: 250 columns, C mod 4 = 2, one idle lane
    (85, 3),     # G 64, SMALL, scalar: 255 columns, the last lane has three live columns
    (64, 4),     # G 64: every lane is a head of its own
    (4, 64),     # G 64: four aligned heads of 16 lanes
    (1, 256),    # G 64: one head scanning the whole wavefront, the widest S = 1
    # ---- S = 2 (257 <= H C <= 512)
    (1, 257),    # scalar: one live column in slot 1, the head crosses 256 into it
    (1, 260),    # 16-byte rows: one live lane in slot 1, the head crosses 256
    (3, 100),    # head 2 = columns 200..299 crosses 256 (virtual lane 63 -> 64)
    (8, 33),     # head 7 = columns 231..263 crosses 256, C mod 4 = 1
    (37, 13),    # scalar: head 19 = columns 247..259 crosses 256
    (2, 256),    # a head boundary exactly at column 256: head 1 is all of slot 1
    (1, 512),    # seg = 129: scan distances up to 128, across both slots
    (128, 4),    # every virtual lane is a head of its own, both slots full
    (128, 3),    # SMALL, 16-byte rows: head 85 = columns 255..257 crosses 256
    (170, 3),    # SMALL, scalar: 510 columns, the last virtual lane has two live columns
    (256, 2),    # SMALL, 16-byte rows, both slots full
    (512, 1),    # SMALL, 16-byte rows: 512 heads of one column
)


def geometry(h, c):
    """The kernel's launch geometry for (H, C), restated from gat_geom / gat_fill_walk and the host dispatch of egc_gatv2.hip:
    S slots per lane, G lanes per row (group), V = S G virtual lanes, seg = the scan's distance limit, small = the C < 4
    window sum, vec_by_width = the width allows 16-byte accesses (pointers and strides permitting); spans_256 = some head has
    columns on both sides of column 256 (slot 0 / slot 1), boundary_256 = a head starts exactly at column 256."""
    width = h * c
    lanes = (width + 3) // 4
    g = 1
    while g < lanes and g < 64:
        g *= 2
    s = 2 if lanes > 64 else 1
    return dict(S=s, G=g, V=s * g, seg=(c + 3) // 4 + 1, small=c < 4, vec_by_width=width % 4 == 0,
                spans_256=width > 256 and 256 % c != 0, boundary_256=width > 256 and 256 % c == 0)


def datt_partials(h, c, n, e):
    """How many workgroup partials of d att the backward sums for n rows and e entries: 256 / G rows (or chunk slots) per
    workgroup, the row workgroups and, when some row can be longer than a chunk, the chunk workgroups."""
    per = 256 // geometry(h, c)["G"]
    slots = -(-e // CHUNK) if e > CHUNK else 0
    return -(-n // per) + -(-slots // per)


def sweep_graph(seed, n=40):
    """(edge_index int64 [2, E], n), shuffled: 160 random edges among nodes 0 .. n - 4 (the last three nodes are isolated),
    12 self loops, 20 duplicates of random edges, one destination (node 1) with exactly 2 CHUNK + 9 in-edges and one source
    (node 2) with exactly 2 CHUNK + 9 out-edges -- three chunks each: two full ones and a tail of 9 (one full forward batch
    and one entry; two backward batches and one entry).  The hubs' own entries may name the hub itself (skipped entries
    inside a chunked row when self loops are added).  E = 1,234."""
    assert n >= 20
    rng = np.random.default_rng(seed)
    live, hub_dst, hub_src, long_row = n - 3, 1, 2, 2 * CHUNK + 9
    not_hub_src = np.array([i for i in range(live) if i != hub_src])
    not_hub_dst = np.array([i for i in range(live) if i != hub_dst])
    plain = np.array([i for i in range(live) if i not in (hub_dst, hub_src)])
    rand = np.stack([rng.choice(not_hub_src, 160), rng.choice(not_hub_dst, 160)])
    loops = np.tile(rng.choice(plain, 12, replace=False), (2, 1))
    dups = rand[:, rng.choice(160, 20, replace=False)]
    into = np.stack([rng.choice(not_hub_src, long_row), np.full(long_row, hub_dst)])
    out_of = np.stack([np.full(long_row, hub_src), rng.choice(not_hub_dst, long_row)])
    ei = np.concatenate([rand, loops, dups, into, out_of], axis=1).astype(np.int64)
    return np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])]), n


def sweep_inputs(h, c, n, seed):
    """xl, xr, gout ~ N(0, 1) float32 [n, H C] and att ~ N(0, 1) / sqrt(C) float32 [H, C]."""
    rng = np.random.default_rng(seed)
    xl, xr, gout = (rng.standard_normal((n, h * c)).astype(np.float32) for _ in range(3))
    return xl, xr, gout, (rng.standard_normal((h, c)) / np.sqrt(c)).astype(np.float32)


def load_gat_golden(name):
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


def _score(xl_j, xr_i, att, slope):
    """[H] from [H, C] rows."""
    return (att * _lrelu(xl_j + xr_i, slope)).sum(axis=-1)


def _chunk_state(sources, row, xl, xr_i, att, slope, loops, ahead, dtype):
    h = att.shape[0]
    m, l, acc = np.full(h, -np.inf, dtype=dtype), np.zeros(h, dtype=dtype), np.zeros_like(att)
    for b in range(0, len(sources), ahead):
        live = [j for j in sources[b:b + ahead] if not (loops and j == row)]
        if not live:
            continue
        s = [_score(xl[j], xr_i, att, slope) for j in live]
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


def aggregate_forward(xl, xr, att, ei, slope=0.2, loops=True, chunk=CHUNK, ahead=AHEAD, dtype=np.float64):
    """(out [N, H C], lse [N, H]) in the kernel's formulation.  att: [H, C]."""
    att = np.asarray(att, dtype=dtype)
    h, c = att.shape
    n = xr.shape[0]
    xl, xr = np.asarray(xl, dtype=dtype).reshape(-1, h, c), np.asarray(xr, dtype=dtype).reshape(n, h, c)
    rowptr, col, _ = csr_by_destination(ei, n)
    out, lse = np.zeros((n, h, c), dtype=dtype), np.full((n, h), -np.inf, dtype=dtype)
    for row in range(n):
        p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
        state = _chunk_state([], row, xl, xr[row], att, slope, loops, ahead, dtype)
        for k, s0 in enumerate(range(p0, p1, chunk)):
            part = _chunk_state(list(col[s0:min(s0 + chunk, p1)]), row, xl, xr[row], att, slope, loops, ahead, dtype)
            state = part if k == 0 else _merge(state, part)
        if loops:
            m, l, acc = state
            s = _score(xl[row], xr[row], att, slope)
            bm = np.maximum(m, s)
            r, w = np.where(m == bm, dtype(1), np.exp(m - bm)), np.exp(s - bm)
            state = bm, l * r + w, acc * r[:, None] + w[:, None] * xl[row]
        m, l, acc = state
        any_ = l > 0
        out[row] = np.where(any_[:, None], acc / np.where(any_, l, 1)[:, None], 0)
        lse[row] = np.where(any_, m + np.log(np.where(any_, l, 1)), -np.inf)
    return out.reshape(n, h * c), lse


def aggregate_backward(xl, xr, att, ei, out, lse, gout, slope=0.2, loops=True, dtype=np.float64):
    """(d xl, d xr [N, H C], d att [H, C]) from d out, with the scores recomputed and D_i = g_i . out_i."""
    att = np.asarray(att, dtype=dtype)
    h, c = att.shape
    n = xr.shape[0]
    xl, xr, out, g = (np.asarray(a, dtype=dtype).reshape(n, h, c) for a in (xl, xr, out, gout))
    rowptr, col, _ = csr_by_destination(ei, n)
    D = (g * out).sum(axis=-1)
    dxl, dxr, datt = np.zeros_like(xl), np.zeros_like(xr), np.zeros_like(att)

    def edge(j, i):
        z = xl[j] + xr[i]
        alpha = np.exp((att * _lrelu(z, slope)).sum(axis=-1) - lse[i])
        ds = alpha * ((g[i] * xl[j]).sum(axis=-1) - D[i])
        return alpha, ds, z

    row_of = np.repeat(np.arange(n), np.diff(rowptr))
    for i in range(n):                                   # destination pass: the forward CSR, the self entry last
        for j in [j for j in col[rowptr[i]:rowptr[i + 1]] if not (loops and j == i)] + ([i] if loops else []):
            _, ds, z = edge(j, i)
            dxr[i] += ds[:, None] * att * np.where(z > 0, 1.0, slope)
            datt += ds[:, None] * _lrelu(z, slope)
    order = np.argsort(col, kind="stable")               # source pass: the transposed CSR (ascending forward position)
    t_rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(col, minlength=n), out=t_rowptr[1:])
    for j in range(n):
        dests = [int(row_of[p]) for p in order[t_rowptr[j]:t_rowptr[j + 1]]]
        for i in [i for i in dests if not (loops and i == j)] + ([j] if loops else []):
            alpha, ds, z = edge(j, i)
            dxl[j] += alpha[:, None] * g[i] + ds[:, None] * att * np.where(z > 0, 1.0, slope)
    return dxl.reshape(n, h * c), dxr.reshape(n, h * c), datt


class _RefAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xl, xr, att, ei, slope, loops):
        a = [t.detach().numpy() for t in (xl, xr, att)]
        dtype = a[0].dtype.type
        out, lse = aggregate_forward(*a, ei, slope, loops, dtype=dtype)
        ctx.saved = (a, ei, slope, loops, out, lse, dtype)
        return torch.from_numpy(out)

    @staticmethod
    def backward(ctx, gout):
        a, ei, slope, loops, out, lse, dtype = ctx.saved
        dxl, dxr, datt = aggregate_backward(*a, ei, out, lse, gout.numpy(), slope, loops, dtype=dtype)
        return torch.from_numpy(dxl), torch.from_numpy(dxr), torch.from_numpy(datt), None, None, None


def layer_forward(x, ei, params, heads, channels, concat=True, negative_slope=0.2, add_self_loops=True, share_weights=False):
    """GATv2Conv through the restatement, on the CPU in the dtype of x (torch; differentiable in x and every parameter)."""
    xl = x @ params["lin_l.weight"].t() + params["lin_l.bias"]
    xr = xl if share_weights else x @ params["lin_r.weight"].t() + params["lin_r.bias"]
    out = _RefAggregate.apply(xl, xr, params["att"].view(heads, channels), ei, negative_slope, add_self_loops)
    if not concat:
        out = out.view(-1, heads, channels).mean(dim=1)
    return out + params["bias"]
