#!/usr/bin/env python3
"""Generate tests/golden/mpnn/*.npz by running the REFERENCE's own Mpnn (experiments/layers.py:231-267), forward and backward
of a seeded cotangent, in float32 (the reference's own precision) and in float64.

Same arrangement as make_golden_grad.py (build container only; the absent third-party packages are its differentiable shims).
Those shims' ``propagate`` stops after ``aggregate``; PyG's ends with ``self.update(out, **kwargs picked by signature)``, and
Mpnn's ``update()`` is half of the layer, so this generator installs a MessagePassing subclass of its own that does the same.

Per case: the inputs, the state dict, the cotangent; out32 / out64; the float64 gradients of x and of every parameter; the
reference's own float32-vs-float64 distance of every gradient (``meta``; that of the output follows from the two outputs
stored); the parameters right after ``torch.manual_seed(seed)`` construction; for max the float32 argument (edge-list position
of the first edge attaining the maximum).  Only vectors are committed.

For every max case but ``ties`` the generator asserts, in float64, that in every (row, channel) the largest message and the
largest message of any OTHER source differ by more than 1e-4 of their magnitude (duplicates of one edge carry the same
message bit for bit in either formulation, and both take the first), so the float32 argument cannot differ between the
reference's formulation and the P / Q split.  In ``ties`` x is small integers and every parameter a multiple of 1/8: all
products and sums are exact in float32, so a tie among messages is exactly a tie among the P_j.
Usage:  python tests/golden/make_golden_mpnn.py
"""
import functools
import inspect
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402
import make_golden_grad as mgg  # noqa: E402

CHUNK = 256          # EGC_TYPED_MEAN_CHUNK: the hub rows are sized by it
LONG = 2 * CHUNK + 18
OUT = os.path.join(HERE, "mpnn")

G_PLAIN = dict(n=48, e=200)
CASES = [   # name, graph, d, towers, aggregators, seed
    ("messy", dict(n=57, e=260, self_loops=9, dups=25, isolated_tail=3), 16, 4, ("add", "mean", "max"), 7100),
    ("hub", dict(hub=True, n=700, e=1500), 8, 2, ("add", "max"), 7200),
    ("ties", dict(n=20, e=120, dups=30), 8, 2, ("max",), 7300),
    ("odd", G_PLAIN, 6, 2, ("add", "max"), 7400),
    ("w116", G_PLAIN, 116, 4, ("max",), 7510),
    ("t1", G_PLAIN, 12, 1, ("mean",), 7600),
]


class UpdatingMessagePassing(mgg.DiffMessagePassing):
    """propagate = message + aggregate (the differentiable shim) + update, as torch_geometric's."""

    def propagate(self, edge_index, size=None, **kwargs):
        out = super().propagate(edge_index, size=size, **kwargs)
        picked = list(inspect.signature(self.update).parameters)[1:]
        return self.update(out, **{k: kwargs[k] for k in picked})

    def update(self, inputs):
        return inputs


def install():
    mgg.install()
    sys.modules["torch_geometric.nn"].MessagePassing = UpdatingMessagePassing
    sys.modules["torch_geometric.nn.conv"].MessagePassing = UpdatingMessagePassing


def make_graph(rng, g):
    g = dict(g)
    if not g.pop("hub", False):
        return mg.make_graph(rng, g)
    n, e = g["n"], g["e"]
    src = np.concatenate([rng.integers(0, n, size=e), rng.integers(0, n, size=LONG), np.full(LONG, 5)])
    dst = np.concatenate([rng.integers(0, n - 3, size=e), np.full(LONG, 3), rng.integers(0, n - 3, size=LONG)])
    perm = rng.permutation(len(src))
    return np.stack([src[perm], dst[perm]]).astype(np.int64), n


def run(layer, x, ei_t, gout, dtype):
    layer = layer.to(dtype)
    for p in layer.parameters():
        p.grad = None
    xx = x.to(dtype).clone().requires_grad_(True)
    mgg.ARGS.clear()
    messages = []
    message = layer.message

    @functools.wraps(message)       # (the shim's propagate picks the arguments by signature)
    def recording(*args, **kwargs):
        messages.append(message(*args, **kwargs))
        return messages[-1]

    layer.message = recording
    try:
        out = layer(xx, ei_t)
    finally:
        del layer.message
    out.backward(gout.to(dtype))
    grads = {k: v.grad.detach().numpy().copy() for k, v in layer.named_parameters()}
    args = [a for _, a in mgg.ARGS.get("args", [])]
    return out.detach().numpy(), xx.grad.detach().numpy(), grads, args, messages[0].detach().numpy()


def assert_max_is_separated(msg, ei, n):
    """float64 messages [E, d]: per (row, channel) the largest message against the largest of any other source."""
    src, dst = ei
    for row in range(n):
        e = np.nonzero(dst == row)[0]
        if len(set(src[e].tolist())) < 2:
            continue
        top = msg[e].max(axis=0)
        winner = src[e][msg[e].argmax(axis=0)]
        for c in range(msg.shape[1]):
            others = msg[e[src[e] != winner[c]], c]
            gap = top[c] - others.max()
            assert gap > 1e-4 * max(abs(top[c]), abs(others.max())), (row, c, gap)


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / max(1e-30, float(np.abs(b).max())))


def main():
    os.makedirs(OUT, exist_ok=True)
    install()
    lay = mg.load_ref("layers")
    for name, graph, d, towers, aggrs, seed0 in CASES:
        for k, aggr in enumerate(aggrs):
            seed = seed0 + k
            rng = np.random.default_rng(seed)
            ei, n = make_graph(rng, graph)
            integer = name == "ties"
            if integer:
                x = torch.from_numpy(rng.integers(-2, 3, size=(n, d)).astype(np.float32))
            else:
                x = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
            gout = torch.from_numpy(rng.standard_normal((n, d)).astype(np.float32))
            torch.manual_seed(seed)
            layer = lay.Mpnn(aggr, d, d, towers=towers)
            init = {f"init:{k}": v.detach().numpy().copy() for k, v in layer.state_dict().items()}
            if integer:
                with torch.no_grad():
                    for p in layer.parameters():
                        p.copy_(torch.from_numpy(rng.integers(-8, 9, size=tuple(p.shape)).astype(np.float32) / 8))
            state = {f"param:{k}": v.detach().numpy().copy() for k, v in layer.state_dict().items()}
            ei_t = torch.from_numpy(ei)
            out32, gx32, gp32, args32, _ = run(layer, x, ei_t, gout, torch.float32)
            out64, gx64, gp64, _, msg64 = run(layer, x, ei_t, gout, torch.float64)
            layer.float()
            extra = {}
            if aggr == "max":
                assert len(args32) == 1
                extra["arg"] = np.where(args32[0].numpy() >= ei.shape[1], -1, args32[0].numpy()).astype(np.int32)
                if not integer:
                    assert_max_is_separated(msg64, ei, n)
            meta = dict(name=name, aggr=aggr, d=d, towers=towers, n=n, seed=seed, chunk=CHUNK, integer=integer,
                        f32_vs_f64_grad_x=rel(gx32, gx64), f32_vs_f64_grad={k: rel(gp32[k], v) for k, v in gp64.items()})
            np.savez_compressed(
                os.path.join(OUT, f"{name}_{aggr}.npz"), x=x.numpy(), edge_index=ei, gout=gout.numpy(), out32=out32, out64=out64,
                grad_x64=gx64, meta=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **state, **init, **extra,
                **{f"grad64:{k}": v for k, v in gp64.items()})
            print(f"{name}_{aggr:5s} N={n:4d} E={ei.shape[1]:5d}  out f32-vs-f64 {rel(out32, out64):.2e}  "
                  f"grad_x {meta['f32_vs_f64_grad_x']:.2e}  worst parameter {max(meta['f32_vs_f64_grad'].values()):.2e}")


if __name__ == "__main__":
    main()
