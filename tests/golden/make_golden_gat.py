#!/usr/bin/env python3
"""Generate tests/golden/gat/*.npz: GATv2Conv by a plain per-edge torch composition of the published PyG 2.x formulas
(index_select both ends, leaky_relu, per-head dot with att, scatter softmax over the destinations, index_add), forward and
backward of a seeded cotangent, on the CPU in float32 and in float64.  PyG is not installed here; nothing of the reference tree
is used.

Edge set: with add_self_loops the given edges without their j == i entries, then one (i, i) per node appended; otherwise the
edges as given.  Duplicates count each time.

Per case: the inputs, the state dict (PyG's names and shapes), the cotangent; out32 / out64; the float64 gradients of x and of
every parameter; the composition's own float32-vs-float64 distance of the output and of every gradient (``meta``).  While
generating, every case is checked for the property it is named for.
Usage:  python tests/golden/make_golden_gat.py
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
OUT = os.path.join(HERE, "gat")

G_PLAIN = dict(n=48, e=200)
G_MESSY = dict(n=57, e=260, self_loops=9, dups=25, isolated_tail=3)
CASES = [   # name, graph, in_channels, H, C, layer arguments, seed
    ("messy", G_MESSY, 12, 4, 5, {}, 8100),
    ("hub", dict(hub=True, n=700, e=1500), 6, 2, 4, {}, 8200),
    ("w104h1", G_PLAIN, 16, 1, 104, {}, 8300),
    ("w112h8", G_PLAIN, 16, 8, 14, {}, 8400),
    ("h8c13", G_PLAIN, 16, 8, 13, {}, 8400),
    ("mean", G_PLAIN, 10, 3, 6, dict(concat=False), 8500),
    ("shared", G_PLAIN, 10, 2, 8, dict(share_weights=True), 8600),
    ("noloops", G_MESSY, 12, 4, 5, dict(add_self_loops=False), 8100),
    ("bigscore", G_PLAIN, 10, 2, 8, {}, 8700),
    ("slope", G_PLAIN, 10, 2, 8, dict(negative_slope=0.05), 8800),
]


def make_graph(rng, g):
    g = dict(g)
    if not g.pop("hub", False):
        return rand_graph(rng, **g), g["n"]
    n, e = g["n"], g["e"]       # one in-row (3) and one out-row (5) of LONG extra entries
    src = np.concatenate([rng.integers(0, n, size=e), rng.integers(0, n, size=LONG), np.full(LONG, 5)])
    dst = np.concatenate([rng.integers(0, n - 3, size=e), np.full(LONG, 3), rng.integers(0, n - 3, size=LONG)])
    perm = rng.permutation(len(src))
    return np.stack([src[perm], dst[perm]]).astype(np.int64), n


def edge_set(ei, n, add_self_loops):
    src, dst = ei[0], ei[1]
    if add_self_loops:
        keep = src != dst
        loops = torch.arange(n, dtype=src.dtype)
        src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
    return src, dst


def scores(xl, xr, att, src, dst, slope):
    """[E, H] attention scores and the [E, H, C] source rows."""
    h, c = att.shape[-2:]
    xj = xl.index_select(0, src).view(-1, h, c)
    z = xj + xr.index_select(0, dst).view(-1, h, c)
    return (torch.nn.functional.leaky_relu(z, slope) * att.view(1, h, c)).sum(dim=-1), xj


def compose(x, ei, p, heads, channels, concat=True, negative_slope=0.2, add_self_loops=True, share_weights=False):
    """GATv2Conv.forward, edge by edge, in the dtype of x.  ``p``: lin_l.weight, lin_l.bias, (lin_r.*), att [1, H, C], bias."""
    n = x.size(0)
    xl = x @ p["lin_l.weight"].t() + p["lin_l.bias"]
    xr = xl if share_weights else x @ p["lin_r.weight"].t() + p["lin_r.bias"]
    src, dst = edge_set(ei, n, add_self_loops)
    s, xj = scores(xl, xr, p["att"], src, dst, negative_slope)
    idx = dst.view(-1, 1).expand_as(s)
    top = torch.full((n, heads), -float("inf"), dtype=x.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    ex = torch.exp(s - top.index_select(0, dst))
    den = torch.zeros((n, heads), dtype=x.dtype).index_add(0, dst, ex)
    alpha = ex / den.index_select(0, dst)
    out = torch.zeros((n, heads, channels), dtype=x.dtype).index_add(0, dst, alpha.unsqueeze(-1) * xj)
    out = out.reshape(n, heads * channels) if concat else out.mean(dim=1)
    return out + p["bias"]


def glorot(rng, *shape):
    bound = np.sqrt(6.0 / (shape[-2] + shape[-1]))
    return rng.uniform(-bound, bound, size=shape).astype(np.float32)


def make_params(rng, fin, heads, channels, concat, share_weights):
    p = {"lin_l.weight": glorot(rng, heads * channels, fin), "lin_l.bias": 0.1 * rng.standard_normal(heads * channels).astype(np.float32)}
    if not share_weights:
        p["lin_r.weight"] = glorot(rng, heads * channels, fin)
        p["lin_r.bias"] = 0.1 * rng.standard_normal(heads * channels).astype(np.float32)
    p["att"] = glorot(rng, 1, heads, channels)
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
    xl = xx @ p["lin_l.weight"].t() + p["lin_l.bias"]
    xr = xl if kw.get("share_weights") else xx @ p["lin_r.weight"].t() + p["lin_r.bias"]
    src, dst = edge_set(ei, xx.size(0), kw.get("add_self_loops", True))
    s, _ = scores(xl, xr, p["att"], src, dst, kw.get("negative_slope", 0.2))
    best = 0.0
    for row in range(xx.size(0)):
        e = dst == row
        if bool(e.any()):
            best = max(best, float(torch.minimum(s[e].max(dim=0).values, -s[e].min(dim=0).values).max()))
    return best


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1e-30, float(np.abs(b).max())))


def rel_out(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1.0, float(np.abs(b).max())))


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
    if name == "w104h1":
        assert (heads, channels) == (1, 104)
    if name == "w112h8":
        assert (heads, channels) == (8, 14)
    if name == "h8c13":
        assert (heads, channels) == (8, 13) and channels % 2 == 1             # heads start at odd columns
    if name == "mean":
        assert kw["concat"] is False and (heads * channels) % 4 != 0      # and the 4-byte access path
    if name == "shared":
        assert kw["share_weights"]
    if name == "bigscore":
        assert span >= 80.0, span
    if name == "slope":
        assert kw["negative_slope"] == 0.05


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, graph, fin, heads, channels, kw, seed in CASES:
        rng = np.random.default_rng(seed)
        ei, n = make_graph(rng, graph)
        x = rng.standard_normal((n, fin)).astype(np.float32)
        concat = kw.get("concat", True)
        gout = rng.standard_normal((n, heads * channels if concat else channels)).astype(np.float32)
        params = make_params(rng, fin, heads, channels, concat, kw.get("share_weights", False))
        ei_t = torch.from_numpy(ei)
        if name == "bigscore":      # scale att (and with it every score) until some row spans +-80
            while score_span(x, ei_t, params, heads, channels, kw) < 90.0:
                params["att"] = params["att"] * np.float32(2.0)
        span = score_span(x, ei_t, params, heads, channels, kw)
        check_property(name, ei, n, heads, channels, kw, span)
        out32, gx32, gp32 = run(x, ei_t, params, gout, torch.float32, heads, channels, kw)
        out64, gx64, gp64 = run(x, ei_t, params, gout, torch.float64, heads, channels, kw)
        if name == "noloops":
            empty = np.bincount(ei[1], minlength=n) == 0
            assert np.array_equal(out64[empty], np.broadcast_to(params["bias"].astype(np.float64), out64[empty].shape))
        state = dict(params)
        if kw.get("share_weights", False):
            state["lin_r.weight"], state["lin_r.bias"] = params["lin_l.weight"], params["lin_l.bias"]
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
