#!/usr/bin/env python3
"""Generate tests/golden/gnn/*.npz: GCNConv, SAGEConv and GINConv (PyG 2.x, no edge weights) by a plain per-edge torch composition
of their published formulas -- forward and backward of a seeded cotangent, on the CPU in float32 and in float64.  PyG is not
installed here; nothing of the reference tree is used.

  GCN   add_remaining_self_loops (every self loop of the input removed, one per node appended), gcn_norm (deg = the in-degree
        over that edge set, w_e = deg^-1/2[src] deg^-1/2[dst], 0 where deg = 0), h = x W^T, index_add_ of w_e h[src], + bias --
        PyG's order, whatever the widths; each of the two flags may be off
  SAGE  index_add_ of x[src], divided by max(in-degree, 1) for mean; lin_l(agg) + lin_r(x); optionally F.normalize
  GIN   nn((1 + eps) x + index_add_ of x[src]), nn a Linear / ReLU stack

Per case: the inputs, the state dict (PyG's names and shapes), the cotangent; out32 / out64; the float64 gradients of x and of
every parameter (eps included where it is trained); the composition's own float32-vs-float64 distance of the output and of every
gradient (``meta``).  While generating, every case is checked for the property it is named for.
Usage:  python tests/golden/make_golden_gnn.py
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
OUT = os.path.join(HERE, "gnn")

G_PLAIN = dict(n=48, e=200)
G_MESSY = dict(n=57, e=150, self_loops=9, dups=25, isolated_tail=3)
G_HUB = dict(hub=True, n=700, e=1500)
CASES = [   # name, layer, graph, in, out, options, seed
    ("gcn_messy_narrow_in", "gcn", G_MESSY, 13, 22, dict(normalize=True, add_self_loops=True), 9800),
    ("gcn_messy_wide_in", "gcn", G_MESSY, 22, 13, dict(normalize=True, add_self_loops=True), 9810),
    ("gcn_hub", "gcn", G_HUB, 8, 8, dict(normalize=True, add_self_loops=True), 9820),
    ("gcn_norm_only", "gcn", G_MESSY, 12, 7, dict(normalize=True, add_self_loops=False), 9830),
    ("gcn_loops_only", "gcn", G_MESSY, 7, 12, dict(normalize=False, add_self_loops=True), 9840),
    ("gcn_plain_sum", "gcn", G_MESSY, 6, 6, dict(normalize=False, add_self_loops=False), 9850),
    ("sage_mean_messy", "sage", G_MESSY, 13, 9, dict(aggr="mean", root_weight=True, normalize=False), 9860),
    ("sage_mean_hub", "sage", G_HUB, 8, 8, dict(aggr="mean", root_weight=True, normalize=False), 9870),
    ("sage_sum", "sage", G_MESSY, 10, 14, dict(aggr="sum", root_weight=True, normalize=False), 9880),
    ("sage_no_root", "sage", G_MESSY, 12, 5, dict(aggr="mean", root_weight=False, normalize=False), 9890),
    ("sage_normalize", "sage", G_PLAIN, 8, 8, dict(aggr="mean", root_weight=True, normalize=True), 9900),
    ("gin_train_eps", "gin", G_MESSY, 13, 7, dict(eps=0.3, train_eps=True, hidden=[16]), 9910),
    ("gin_hub", "gin", G_HUB, 8, 8, dict(eps=0.0, train_eps=True, hidden=[]), 9920),
    ("gin_buffer_eps", "gin", G_PLAIN, 10, 6, dict(eps=-0.5, train_eps=False, hidden=[12]), 9930),
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


def linear(rng, fout, fin, bias=True):
    k = 1.0 / np.sqrt(fin)
    w = rng.uniform(-k, k, (fout, fin)).astype(np.float32)
    return (w, rng.uniform(-k, k, fout).astype(np.float32)) if bias else (w, None)


def init_params(rng, layer, fin, fout, opt):
    """The state dict under PyG's names (random values: a zero bias would hide a bias that is not added)."""
    p = {}
    if layer == "gcn":
        p["lin.weight"], p["bias"] = linear(rng, fout, fin)
    elif layer == "sage":
        p["lin_l.weight"], p["lin_l.bias"] = linear(rng, fout, fin)
        if opt["root_weight"]:
            p["lin_r.weight"], _ = linear(rng, fout, fin, bias=False)
    else:
        p["eps"] = np.array([opt["eps"]], dtype=np.float32)
        dims = [fin] + list(opt["hidden"]) + [fout]
        for k in range(len(dims) - 1):      # Sequential(Linear, ReLU, Linear, ...): the Linears sit at the even positions
            p[f"nn.{2 * k}.weight"], p[f"nn.{2 * k}.bias"] = linear(rng, dims[k + 1], dims[k])
    return p


def scatter_rows(v, dst, n):
    return torch.zeros((n, v.size(1)), dtype=v.dtype).index_add_(0, dst, v)


def compose(x, ei, p, layer, opt):
    """The layer's forward, edge by edge, in the dtype of x."""
    n, src, dst = x.size(0), ei[0], ei[1]
    if layer == "gcn":
        if opt["add_self_loops"]:           # add_remaining_self_loops without weights
            keep = src != dst
            loops = torch.arange(n)
            src, dst = torch.cat([src[keep], loops]), torch.cat([dst[keep], loops])
        w = torch.ones(src.numel(), dtype=x.dtype)
        if opt["normalize"]:                # gcn_norm
            deg = torch.zeros(n, dtype=x.dtype).index_add_(0, dst, w)
            dis = deg.pow(-0.5)
            dis = torch.where(torch.isinf(dis), torch.zeros_like(dis), dis)
            w = dis[src] * w * dis[dst]
        h = x @ p["lin.weight"].t()
        return scatter_rows(w.view(-1, 1) * h.index_select(0, src), dst, n) + p["bias"]
    agg = scatter_rows(x.index_select(0, src), dst, n)
    if layer == "sage":
        if opt["aggr"] == "mean":
            agg = agg / torch.bincount(dst, minlength=n).clamp(min=1).to(x.dtype).view(-1, 1)
        out = agg @ p["lin_l.weight"].t() + p["lin_l.bias"]
        if opt["root_weight"]:
            out = out + x @ p["lin_r.weight"].t()
        return torch.nn.functional.normalize(out, p=2.0, dim=-1) if opt["normalize"] else out
    h = (1 + p["eps"]) * x + agg
    n_lin = len(opt["hidden"]) + 1
    for k in range(n_lin):
        h = h @ p[f"nn.{2 * k}.weight"].t() + p[f"nn.{2 * k}.bias"]
        if k + 1 < n_lin:
            h = torch.relu(h)
    return h


def run(x, ei, params, gout, dtype, layer, opt):
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
    xx = torch.from_numpy(x).to(dtype).requires_grad_(True)
    out = compose(xx, ei, p, layer, opt)
    out.backward(torch.from_numpy(gout).to(dtype))
    return out.detach().numpy(), xx.grad.numpy(), {k: v.grad.numpy() for k, v in p.items()}


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1e-30, float(np.abs(b).max())))


def rel_out(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1.0, float(np.abs(b).max())))


def check_property(name, layer, graph, ei, n, fin, fout, opt):
    src, dst = ei
    indeg, outdeg = np.bincount(dst, minlength=n), np.bincount(src, minlength=n)
    pairs = src * n + dst
    if graph is G_MESSY:
        assert int((src == dst).sum()) >= 9 and len(pairs) - len(np.unique(pairs)) >= 20
        assert (indeg[-3:] == 0).all() and (outdeg[-3:] == 0).all() and (indeg == 1).sum() >= 1
    if graph is G_HUB:
        assert indeg.max() > 2 * CHUNK + 1 and outdeg.max() > 2 * CHUNK + 1
    if name == "gcn_messy_narrow_in":
        assert fin < fout and fin % 4 and fout % 4
    if name == "gcn_messy_wide_in":
        assert fin > fout and fin % 4 and fout % 4
    if name in ("gcn_norm_only", "gcn_loops_only", "gcn_plain_sum"):
        assert (opt["normalize"], opt["add_self_loops"]) == dict(gcn_norm_only=(True, False), gcn_loops_only=(False, True),
                                                                 gcn_plain_sum=(False, False))[name]
    if name == "sage_mean_messy":
        assert fin % 4 and opt["aggr"] == "mean" and opt["root_weight"]
    if name == "sage_sum":
        assert opt["aggr"] == "sum" and fin % 4
    if name == "sage_no_root":
        assert not opt["root_weight"]
    if name == "sage_normalize":
        assert opt["normalize"]
    if name == "gin_train_eps":
        assert opt["train_eps"] and opt["eps"] != 0.0 and fin % 4
    if name == "gin_buffer_eps":
        assert not opt["train_eps"] and opt["eps"] != 0.0


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, layer, graph, fin, fout, opt, seed in CASES:
        rng = np.random.default_rng(seed)
        ei, n = make_graph(rng, graph)
        params = init_params(rng, layer, fin, fout, opt)
        x = rng.standard_normal((n, fin)).astype(np.float32)
        gout = rng.standard_normal((n, fout)).astype(np.float32)
        check_property(name, layer, graph, ei, n, fin, fout, opt)
        ei_t = torch.from_numpy(ei)
        out32, gx32, gp32 = run(x, ei_t, params, gout, torch.float32, layer, opt)
        out64, gx64, gp64 = run(x, ei_t, params, gout, torch.float64, layer, opt)
        if layer == "gin" and not opt["train_eps"]:         # a buffer has no gradient
            gp32.pop("eps"), gp64.pop("eps")
        meta = dict(name=name, layer=layer, n=n, in_channels=fin, out_channels=fout, options=opt, seed=seed, chunk=CHUNK,
                    f32_vs_f64_out=rel_out(out32, out64), f32_vs_f64_grad_x=rel(gx32, gx64),
                    f32_vs_f64_grad={k: rel(gp32[k], v) for k, v in gp64.items()})
        path = os.path.join(OUT, f"{name}.npz")
        np.savez_compressed(
            path, x=x, edge_index=ei, gout=gout, out32=out32, out64=out64, grad_x64=gx64,
            meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **{f"param:{k}": v for k, v in params.items()},
            **{f"grad64:{k}": v for k, v in gp64.items()})
        print(f"{name:20s} N={n:4d} E={ei.shape[1]:5d} {fin:3d} -> {fout:3d} {os.path.getsize(path):7d} bytes  "
              f"out f32-vs-f64 {meta['f32_vs_f64_out']:.2e}  grad_x {meta['f32_vs_f64_grad_x']:.2e}  worst parameter "
              f"{max(meta['f32_vs_f64_grad'].values()):.2e}")


if __name__ == "__main__":
    main()
