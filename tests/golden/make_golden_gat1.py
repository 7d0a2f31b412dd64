#!/usr/bin/env python3
"""Generate tests/golden/gat1/*.npz: GATConv (GAT v1) by a plain per-edge torch composition of the published PyG formulas
(xl = x W^T, a_src = per-head dot of xl with att_src, a_dst likewise, index_select both ends, leaky_relu of the sum, scatter
softmax over the destinations, index_add), forward and backward of a seeded cotangent, on the CPU in float32 and in float64.
PyG is not installed here; nothing of the reference tree is used.

Edge set, file layout and ``meta``: as tests/golden/make_golden_gat.py (the given edges without their j == i entries plus one
(i, i) per node with add_self_loops, otherwise the edges as given; duplicates count each time; per case the inputs, the state
dict in the PyG 2.0 - 2.2 names -- lin_src.weight and lin_dst.weight hold the same array --, the cotangent, out32 / out64, the
float64 gradients of x and of every parameter, and the composition's own float32-vs-float64 distances).  While generating,
every case is checked for the property it is named for.
Usage:  python tests/golden/make_golden_gat1.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_gat import CHUNK, G_MESSY, G_PLAIN, edge_set, glorot, make_graph, rel, rel_out  # noqa: E402

OUT = os.path.join(HERE, "gat1")
G_SMALL = dict(n=24, e=100)
CASES = [   # name, graph, in_channels, H, C, layer arguments, seed
    ("messy", G_MESSY, 12, 4, 5, {}, 9100),
    ("hub", dict(hub=True, n=700, e=1500), 6, 2, 4, {}, 9200),
    ("w152h8", G_PLAIN, 16, 8, 19, {}, 9300),
    ("w152h1", G_PLAIN, 16, 1, 152, {}, 9400),
    ("w240h8", G_PLAIN, 16, 8, 30, {}, 9500),
    ("w304h1", G_SMALL, 16, 1, 304, {}, 9600),
    ("mean", G_PLAIN, 10, 3, 6, dict(concat=False), 9700),
    ("noloops", G_MESSY, 12, 4, 5, dict(add_self_loops=False), 9100),
    ("bigscore", G_PLAIN, 10, 2, 8, {}, 9800),
    ("slope", G_PLAIN, 10, 2, 8, dict(negative_slope=0.05), 9900),
    ("nobias", G_PLAIN, 10, 2, 8, dict(bias=False), 9950),
]


def scores(x, p, src, dst, heads, channels, slope):
    """[E, H] attention scores and xl [N, H, C]."""
    xl = (x @ p["lin_src.weight"].t()).view(-1, heads, channels)
    a_src, a_dst = (xl * p["att_src"]).sum(dim=-1), (xl * p["att_dst"]).sum(dim=-1)
    return torch.nn.functional.leaky_relu(a_src.index_select(0, src) + a_dst.index_select(0, dst), slope), xl


def compose(x, ei, p, heads, channels, concat=True, negative_slope=0.2, add_self_loops=True, bias=True):
    """GATConv.forward, edge by edge, in the dtype of x.  ``p``: lin_src.weight, att_src and att_dst [1, H, C], (bias)."""
    n = x.size(0)
    src, dst = edge_set(ei, n, add_self_loops)
    s, xl = scores(x, p, src, dst, heads, channels, negative_slope)
    idx = dst.view(-1, 1).expand_as(s)
    top = torch.full((n, heads), -float("inf"), dtype=x.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    ex = torch.exp(s - top.index_select(0, dst))
    den = torch.zeros((n, heads), dtype=x.dtype).index_add(0, dst, ex)
    alpha = ex / den.index_select(0, dst)
    out = torch.zeros((n, heads, channels), dtype=x.dtype).index_add(0, dst, alpha.unsqueeze(-1) * xl.index_select(0, src))
    out = out.reshape(n, heads * channels) if concat else out.mean(dim=1)
    return out + p["bias"] if bias else out


def make_params(rng, fin, heads, channels, concat, bias):
    p = {"lin_src.weight": glorot(rng, heads * channels, fin), "att_src": glorot(rng, 1, heads, channels),
         "att_dst": glorot(rng, 1, heads, channels)}
    if bias:
        p["bias"] = 0.1 * rng.standard_normal(heads * channels if concat else channels).astype(np.float32)
    return p


def run(x, ei, params, gout, dtype, heads, channels, kw):
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = compose(xx, ei, p, heads, channels, **kw)
    out.backward(torch.from_numpy(gout).to(dtype))
    return out.detach().numpy(), xx.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}


def score_span(x, ei, params, heads, channels, kw):
    """float64: the largest over (row, head) of min(max score, -min score) among the row's entries."""
    p = {k: torch.from_numpy(v).double() for k, v in params.items()}
    xx = torch.from_numpy(x).double()
    src, dst = edge_set(ei, xx.size(0), kw.get("add_self_loops", True))
    s, _ = scores(xx, p, src, dst, heads, channels, kw.get("negative_slope", 0.2))
    best = 0.0
    for row in range(xx.size(0)):
        e = dst == row
        if bool(e.any()):
            best = max(best, float(torch.minimum(s[e].max(dim=0).values, -s[e].min(dim=0).values).max()))
    return best


def check_property(name, ei, n, heads, channels, kw, span):
    src, dst = ei
    indeg = np.bincount(dst, minlength=n)
    pairs = src * n + dst
    if name in ("messy", "noloops"):
        assert n == 57 and 240 <= ei.shape[1] <= 300 and int((src == dst).sum()) >= 9
        assert len(pairs) - len(np.unique(pairs)) >= 20 and ei.max() < n - 3
        assert (heads * channels) % 4 == 0 and channels % 4 != 0           # heads straddle the four-column lanes
    if name == "noloops":
        assert not kw["add_self_loops"] and (indeg == 0).any()
    if name == "hub":
        assert indeg.max() > 2 * CHUNK + 18 and np.bincount(src, minlength=n).max() > 2 * CHUNK + 18
    shapes = dict(w152h8=(8, 19), w152h1=(1, 152), w240h8=(8, 30), w304h1=(1, 304))
    if name in shapes:
        assert (heads, channels) == shapes[name] and (heads * channels + 2 * heads) % 4 == (0 if heads == 8 else 2)
    if name == "w304h1":
        assert n == 24 and heads * channels > 256                          # two slots per lane
    if name == "mean":
        assert kw["concat"] is False and (heads * channels) % 4 != 0      # and the 4-byte access path
    if name == "bigscore":
        assert span >= 80.0, span
    if name == "slope":
        assert kw["negative_slope"] == 0.05
    if name == "nobias":
        assert kw["bias"] is False


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, graph, fin, heads, channels, kw, seed in CASES:
        rng = np.random.default_rng(seed)
        ei, n = make_graph(rng, graph)
        x = rng.standard_normal((n, fin)).astype(np.float32)
        concat = kw.get("concat", True)
        gout = rng.standard_normal((n, heads * channels if concat else channels)).astype(np.float32)
        params = make_params(rng, fin, heads, channels, concat, kw.get("bias", True))
        ei_t = torch.from_numpy(ei)
        if name == "bigscore":      # scale head 0's att (and with it every score of that head) until some row spans +-80; head
            scale = np.array([2.0, 1.0], dtype=np.float32).reshape(1, 2, 1)   # 1 keeps an unsaturated softmax next to it, so
            while score_span(x, ei_t, params, heads, channels, kw) < 90.0:    # that d att does not vanish as a whole
                params["att_src"], params["att_dst"] = params["att_src"] * scale, params["att_dst"] * scale
        span = score_span(x, ei_t, params, heads, channels, kw)
        check_property(name, ei, n, heads, channels, kw, span)
        out32, gx32, gp32 = run(x, ei_t, params, gout, torch.float32, heads, channels, kw)
        out64, gx64, gp64 = run(x, ei_t, params, gout, torch.float64, heads, channels, kw)
        if name == "noloops":
            empty = np.bincount(ei[1], minlength=n) == 0
            assert np.array_equal(out64[empty], np.broadcast_to(params["bias"].astype(np.float64), out64[empty].shape))
        state = dict(params)
        state["lin_dst.weight"] = params["lin_src.weight"]
        meta = dict(name=name, n=n, in_channels=fin, heads=heads, channels=channels, seed=seed, chunk=CHUNK, kwargs=kw,
                    score_span=span, f32_vs_f64_out=rel_out(out32, out64), f32_vs_f64_grad_x=rel(gx32, gx64),
                    f32_vs_f64_grad={k: rel(gp32[k], v) for k, v in gp64.items()})
        np.savez_compressed(
            os.path.join(OUT, f"{name}.npz"), x=x, edge_index=ei, gout=gout, out32=out32, out64=out64, grad_x64=gx64,
            meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **{f"param:{k}": v for k, v in state.items()},
            **{f"grad64:{k}": v for k, v in gp64.items()})
        print(f"{name:9s} N={n:4d} E={ei.shape[1]:5d} H={heads} C={channels:3d} span {span:6.1f}  out f32-vs-f64 "
              f"{meta['f32_vs_f64_out']:.2e}  grad_x {meta['f32_vs_f64_grad_x']:.2e}  worst parameter "
              f"{max(meta['f32_vs_f64_grad'].values()):.2e}")


if __name__ == "__main__":
    main()
