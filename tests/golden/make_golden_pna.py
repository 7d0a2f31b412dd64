#!/usr/bin/env python3
"""Generate tests/golden/pna/*.npz: PNAConv (PyG 2.x, edge_dim=None, pre_layers=1, post_layers=1) by a plain per-edge torch
composition of its published formulas -- index_select both ends, concatenate, the per-tower pre Linears on [x_i | x_j], one
scatter per aggregator (index_add_ / scatter_reduce), the degree scalers, concatenate with x, the per-tower post Linears, lin --
forward and backward of a seeded cotangent, on the CPU in float32 and in float64.  PyG is not installed here; nothing of the
reference tree is used.

var / std are PyG's: relu(E[h^2] - E[h]^2) and sqrt(var + 1e-5).  min / max go through an explicit first-edge argument (the first
edge, in edge-list order, whose message equals the row's extremum), so tied extrema have a defined gradient: the first edge takes
it.  A row without in-edges aggregates to 0 (std: sqrt(1e-5)); its degree in the scalers is 1.

Per case: the inputs, the in-degree histogram ``deg``, the state dict (PyG's names and shapes), the cotangent; out32 / out64; the
float64 gradients of x and of every parameter; the composition's own float32-vs-float64 distance of the output and of every
gradient (``meta``); for the cases whose parameters are the seeded initial ones, those again under ``init:`` (what
``torch.manual_seed(seed)`` followed by PyG's construction order gives).  While generating, every case is checked for the
property it is named for.
Usage:  python tests/golden/make_golden_pna.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import rand_graph  # noqa: E402

CHUNK = 256          # EGC_TYPED_MEAN_CHUNK: the hub rows are sized by it
LONG = 2 * CHUNK + 18
OUT = os.path.join(HERE, "pna")

REF_AGGR = ["mean", "min", "max", "std"]
REF_SCAL = ["identity", "amplification", "attenuation"]
G_PLAIN = dict(n=48, e=200)
G_MESSY = dict(n=57, e=150, self_loops=9, dups=25, isolated_tail=3)
CASES = [   # name, graph, in, out, towers, divide_input, aggregators, scalers, seed
    ("messy", G_MESSY, 32, 32, 4, True, REF_AGGR, REF_SCAL, 9100),
    ("hub", dict(hub=True, n=700, e=1500), 8, 8, 2, True, REF_AGGR, REF_SCAL, 9200),
    ("ties", dict(hub=True, n=300, e=900), 8, 8, 2, True, REF_AGGR, ["identity", "amplification"], 9300),
    ("nodivide", G_PLAIN, 12, 20, 2, False, REF_AGGR, REF_SCAL, 9400),
    ("all6", G_MESSY, 16, 16, 1, False, ["sum", "mean", "min", "max", "var", "std"],
     ["identity", "amplification", "attenuation", "linear", "inverse_linear"], 9500),
    ("meanonly", G_PLAIN, 8, 8, 2, True, ["mean"], ["identity"], 9600),
    ("w116", G_PLAIN, 116, 36, 4, True, REF_AGGR, REF_SCAL, 9700),
]
WITH_INIT = ("messy", "nodivide", "all6")


def make_graph(rng, g):
    g = dict(g)
    if not g.pop("hub", False):
        return rand_graph(rng, **g), g["n"]
    n, e = g["n"], g["e"]       # one in-row (3) and one out-row (5) of LONG extra entries
    src = np.concatenate([rng.integers(0, n, size=e), rng.integers(0, n, size=LONG), np.full(LONG, 5)])
    dst = np.concatenate([rng.integers(0, n - 3, size=e), np.full(LONG, 3), rng.integers(0, n - 3, size=LONG)])
    perm = rng.permutation(len(src))
    return np.stack([src[perm], dst[perm]]).astype(np.int64), n


def degree_stats(hist):
    h = hist.astype(np.float64)
    k = np.arange(len(h), dtype=np.float64)
    return float((k * h).sum() / h.sum()), float((np.log(k + 1) * h).sum() / h.sum())


def sizes(fin, fout, towers, divide):
    return (fin // towers if divide else fin), fout // towers


def init_params(seed, fin, fout, towers, divide, n_aggr, n_scal):
    """PyG's construction order: per tower the pre Linear, then the post Linear; lin last."""
    f_in, f_out = sizes(fin, fout, towers, divide)
    torch.manual_seed(seed)
    p = {}
    for t in range(towers):
        for name, lin in ((f"pre_nns.{t}.0", torch.nn.Linear(2 * f_in, f_in)),
                          (f"post_nns.{t}.0", torch.nn.Linear((n_aggr * n_scal + 1) * f_in, f_out))):
            p[f"{name}.weight"], p[f"{name}.bias"] = lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()
    lin = torch.nn.Linear(fout, fout)
    p["lin.weight"], p["lin.bias"] = lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()
    return p


def first_edge_extremum(msg, dst, idx, n, cnt, largest):
    """[N, W] extremum of the messages per destination, taken from the FIRST edge attaining it (0 for an empty row)."""
    e = msg.size(0)
    start = torch.full((n, msg.size(1)), -float("inf") if largest else float("inf"), dtype=msg.dtype)
    ext = start.scatter_reduce(0, idx, msg.detach(), "amax" if largest else "amin", include_self=True)
    hit = msg.detach() == ext.index_select(0, dst)
    pos = torch.arange(e).view(-1, 1).expand_as(msg)
    arg = torch.full((n, msg.size(1)), e, dtype=torch.int64).scatter_reduce(0, idx, torch.where(hit, pos, e), "amin", include_self=True)
    val = msg.gather(0, arg.clamp(max=e - 1))
    return torch.where((cnt > 0).view(-1, 1), val, torch.zeros_like(val)), arg


def messages(x, ei, p, towers, divide):
    """[E, towers * F_in] messages pre_t([x_i^t | x_j^t]), j -> i."""
    src, dst = ei[0], ei[1]
    xi, xj = x.index_select(0, dst), x.index_select(0, src)
    if divide:
        xi, xj = xi.view(xi.size(0), towers, -1), xj.view(xj.size(0), towers, -1)
    else:
        xi, xj = xi.unsqueeze(1).expand(-1, towers, -1), xj.unsqueeze(1).expand(-1, towers, -1)
    h = torch.cat([xi, xj], dim=-1)
    return torch.cat([h[:, t] @ p[f"pre_nns.{t}.0.weight"].t() + p[f"pre_nns.{t}.0.bias"] for t in range(towers)], dim=-1)


def compose(x, ei, p, towers, divide, aggregators, scalers, avg_lin, avg_log):
    """PNAConv.forward, edge by edge, in the dtype of x."""
    n, dst = x.size(0), ei[1]
    msg = messages(x, ei, p, towers, divide)
    w = msg.size(1)
    f_in = w // towers
    cnt = torch.bincount(dst, minlength=n)
    deg = cnt.clamp(min=1).to(x.dtype).view(-1, 1)
    idx = dst.view(-1, 1).expand_as(msg)
    total = torch.zeros((n, w), dtype=x.dtype).index_add_(0, dst, msg)
    mean = total / deg
    var = torch.relu(torch.zeros((n, w), dtype=x.dtype).index_add_(0, dst, msg * msg) / deg - mean * mean)
    blocks = []
    for a in aggregators:
        if a == "sum":
            blocks.append(total)
        elif a == "mean":
            blocks.append(mean)
        elif a in ("min", "max"):
            blocks.append(first_edge_extremum(msg, dst, idx, n, cnt, a == "max")[0])
        elif a == "var":
            blocks.append(var)
        elif a == "std":
            blocks.append(torch.sqrt(var + 1e-5))
        else:
            raise ValueError(a)
    out = torch.cat([b.view(n, towers, f_in) for b in blocks], dim=-1)                      # [N, T, A F_in]
    d = deg.view(-1, 1, 1)
    factor = dict(identity=lambda: torch.ones_like(d), amplification=lambda: torch.log(d + 1) / avg_log,
                  attenuation=lambda: avg_log / torch.log(d + 1), linear=lambda: d / avg_lin, inverse_linear=lambda: avg_lin / d)
    out = torch.cat([out * factor[s]() for s in scalers], dim=-1)                           # [N, T, S A F_in]
    xt = x.view(n, towers, -1) if divide else x.unsqueeze(1).expand(-1, towers, -1)
    out = torch.cat([xt, out], dim=-1)
    out = torch.cat([out[:, t] @ p[f"post_nns.{t}.0.weight"].t() + p[f"post_nns.{t}.0.bias"] for t in range(towers)], dim=-1)
    return out @ p["lin.weight"].t() + p["lin.bias"]


def run(x, ei, params, gout, dtype, *cfg):
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = compose(xx, ei, p, *cfg)
    out.backward(torch.from_numpy(gout).to(dtype))
    return out.detach().numpy(), xx.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1e-30, float(np.abs(b).max())))


def rel_out(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1.0, float(np.abs(b).max())))


def source_projection(x, params, towers, divide):
    """P [N, W] in float64: the source half of every tower's pre-transform."""
    f_in = params["pre_nns.0.0.weight"].shape[0]
    xx = x.astype(np.float64)
    cols = []
    for t in range(towers):
        ws = params[f"pre_nns.{t}.0.weight"][:, f_in:].astype(np.float64)
        cols.append((xx[:, t * f_in:(t + 1) * f_in] if divide else xx) @ ws.T)
    return np.concatenate(cols, axis=1)


def check_property(name, ei, n, x, params, towers, divide, fin, fout):
    src, dst = ei
    indeg, outdeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    pairs = src * n + dst
    if name in ("messy", "all6"):
        assert int((src == dst).sum()) >= 9 and len(pairs) - len(np.unique(pairs)) >= 20
        assert (indeg == 0).sum() >= 3 and (indeg == 1).sum() >= 1
    if name == "messy":
        assert towers == 4 and divide
    if name in ("hub", "ties"):
        assert indeg.max() > 2 * CHUNK + 1 and outdeg.max() > 2 * CHUNK + 1
    if name == "ties":
        P = source_projection(x, params, towers, divide)
        assert np.array_equal(P, np.round(P)) and np.abs(P).max() < 2 ** 20          # exact in float32 too
        row = int(indeg.argmax())
        v = P[src[dst == row]]                                                     # the long row's entries, edge-list order
        at = v == v.max(axis=0)
        assert (at[:CHUNK].sum(axis=0) > 1).any() and ((at[:CHUNK].any(axis=0)) & (at[CHUNK:].any(axis=0))).any()
    if name == "nodivide":
        assert not divide and fin != fout
    if name == "all6":
        assert towers == 1
    if name == "w116":
        f_in = fin // towers
        assert towers * f_in == 116 and (4 * f_in) % 16 != 0


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, graph, fin, fout, towers, divide, aggregators, scalers, seed in CASES:
        rng = np.random.default_rng(seed)
        ei, n = make_graph(rng, graph)
        hist = np.bincount(np.bincount(ei[1], minlength=n)).astype(np.int64)
        avg_lin, avg_log = degree_stats(hist)
        params = init_params(seed, fin, fout, towers, divide, len(aggregators), len(scalers))
        init = {k: v.copy() for k, v in params.items()} if name in WITH_INIT else {}
        x = rng.standard_normal((n, fin)).astype(np.float32)
        if name == "ties":      # integer inputs and integer pre weights: P is integer-valued, maxima tie between edges
            x = rng.integers(-2, 3, (n, fin)).astype(np.float32)
            for t in range(towers):
                params[f"pre_nns.{t}.0.weight"] = rng.integers(-1, 2, params[f"pre_nns.{t}.0.weight"].shape).astype(np.float32)
        gout = rng.standard_normal((n, fout)).astype(np.float32)
        check_property(name, ei, n, x, params, towers, divide, fin, fout)
        cfg = (towers, divide, aggregators, scalers, avg_lin, avg_log)
        ei_t = torch.from_numpy(ei)
        out32, gx32, gp32 = run(x, ei_t, params, gout, torch.float32, *cfg)
        out64, gx64, gp64 = run(x, ei_t, params, gout, torch.float64, *cfg)
        meta = dict(name=name, n=n, in_channels=fin, out_channels=fout, towers=towers, divide_input=divide, aggregators=aggregators,
                    scalers=scalers, seed=seed, chunk=CHUNK, avg_lin=avg_lin, avg_log=avg_log,
                    f32_vs_f64_out=rel_out(out32, out64), f32_vs_f64_grad_x=rel(gx32, gx64),
                    f32_vs_f64_grad={k: rel(gp32[k], v) for k, v in gp64.items()})
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(
            path, x=x, edge_index=ei, deg=hist, gout=gout, out32=out32, out64=out64, grad_x64=gx64,
            meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **{f"param:{k}": v for k, v in params.items()},
            **{f"init:{k}": v for k, v in init.items()}, **{f"grad64:{k}": v for k, v in gp64.items()})
        print(f"{name:9s} N={n:4d} E={ei.shape[1]:5d} W={towers * sizes(fin, fout, towers, divide)[0]:3d} {os.path.getsize(path):7d} bytes  "
              f"out f32-vs-f64 {meta['f32_vs_f64_out']:.2e}  grad_x {meta['f32_vs_f64_grad_x']:.2e}  worst parameter "
              f"{max(meta['f32_vs_f64_grad'].values()):.2e}")


if __name__ == "__main__":
    main()
