#!/usr/bin/env python3
"""Generate tests/golden/rgcn/rgcn_*.npz and regc_*.npz (a directory of their own: golden_util.golden_names() takes every
*.npz directly under tests/golden for a single-layer fixture) by running the REFERENCE's own RGCNConv and REGC.forward
(experiments/rmag/models.py:32-72, 151-212).

Same arrangement as make_golden_nets.py (build container only; the absent third-party packages are its differentiable
shims).  The reference's REGC cannot be constructed (``super(self)``, rmag/models.py:161): the object is allocated with
``REGC.__new__``, initialised as a plain nn.Module and given the three attributes its forward reads -- ``embs``, ``convs``,
``dropout`` -- built from the reference's own layer classes at the fixture's small sizes.  The forward that runs is the
reference's.  Every case runs in float32 (the reference's own precision) and in float64, forward and backward of a seeded
cotangent.  Only vectors are committed; a case too large for one file is spread over several (tests/rgcn_ref.py merges
them), the parameters of the widest case are drawn from a seed on both sides instead of being stored, and its float64
parameter gradients are stored rounded to float32 (6e-8 relative, far inside the bound they are used with).
Usage:  python tests/golden/make_golden_rgcn.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402
import make_golden_nets as mgn  # noqa: E402
from rgcn_ref import seeded_arrays  # noqa: E402

CHUNK = 256          # egc_typed_mean_chunk(): fixed before the long row was sized
LONG_ROW = 2 * CHUNK + 18
PART_BYTES = 700 << 10
OUT = os.path.join(HERE, "rgcn")

LAYER_CASES = [
    dict(name="rgcn_small", fin=24, fout=32, sizes=dict(author=37, field_of_study=11, institution=5, paper=29), edges=60, seed=11),
    dict(name="rgcn_odd", fin=30, fout=13, sizes=dict(author=37, field_of_study=11, institution=5, paper=29), edges=60, seed=12),
    dict(name="rgcn_mag_shape", fin=128, fout=349, sizes=dict(author=150, field_of_study=40, institution=12, paper=120),
         edges=900, seed=13, params_from_seed=True, grads_as_f32=True),
]
NET_CASES = [
    dict(name="regc_egc", use_egc=True, seed=21),
    dict(name="regc_rgcn", use_egc=False, seed=22),
]
NET = dict(num_layers=3, hidden=32, in_features=24, num_classes=13, heads=8, bases=4,
           sizes=dict(author=41, field_of_study=23, institution=17, paper=37), edges=90)
LEFT_OUT = 6         # ("field_of_study", "to", "paper") is not in adj_t_dict


def make_edges(rng, ref, sizes, edges):
    adj, save = {}, {}
    for i, key in enumerate(ref.EDGE_TYPES):
        if i == LEFT_OUT:
            continue
        n_src, n_dst = sizes[key[0]], sizes[key[2]]
        e = 7 if i == 1 else edges + (LONG_ROW if i == 4 else 0)   # one very sparse relation
        src = rng.integers(0, n_src, size=e)
        dst = rng.integers(0, max(1, n_dst - 3), size=e)           # the last three targets never receive anything
        if i == 4:
            dst[:LONG_ROW] = 0                                     # a row of more than two chunks and one entry
        adj[key] = mg.SparseTensor(row=torch.from_numpy(dst), col=torch.from_numpy(src), sparse_sizes=(n_dst, n_src))
        save[f"ei_{i}"] = np.stack([src, dst]).astype(np.int64)
    return adj, save


def run_both(module, state, x_np, adj, gout_np):
    """forward + backward in float32 and float64 from the same state: {tag: (out, grad_x, grad_params)}."""
    res = {}
    for tag, dtype in (("32", torch.float32), ("64", torch.float64)):
        module.load_state_dict(state)
        module = module.to(dtype)
        for p in module.parameters():
            p.grad = None
        xs = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in x_np.items()}
        out = module(xs, adj)
        sum((out[k] * torch.from_numpy(gout_np[k]).to(dtype)).sum() for k in out).backward()
        res[tag] = ({k: v.detach().numpy() for k, v in out.items()},
                    {k: v.grad.detach().numpy() for k, v in xs.items()},
                    {k: v.grad.detach().numpy() for k, v in module.named_parameters() if v.grad is not None})
    return res


def save_case(name, meta, arrays, res, grads_as_f32=False):
    d_grad = {}
    for k, v in res["64"][2].items():
        d_grad[k] = float(np.abs(res["32"][2][k].astype(np.float64) - v).max() / max(1e-30, float(np.abs(v).max())))
    d_gx = {}
    for k, v in res["64"][1].items():
        d_gx[k] = float(np.abs(res["32"][1][k].astype(np.float64) - v).max() / max(1e-30, float(np.abs(v).max())))
    for k in res["64"][0]:
        arrays[f"out32_{k}"] = res["32"][0][k]
        arrays[f"out64_{k}"] = res["64"][0][k]
    for k, v in res["64"][1].items():
        arrays[f"grad_x64_{k}"] = v
    for k, v in res["64"][2].items():
        arrays[f"grad64:{k}"] = v.astype(np.float32) if grads_as_f32 else v
    meta = dict(meta, f32_vs_f64_grad=d_grad, f32_vs_f64_grad_x=d_gx)
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    parts, size = [{}], 0
    for k in sorted(arrays, key=lambda k: (k != "meta", k)):
        if size and size + arrays[k].nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = arrays[k]
        size += arrays[k].nbytes
    for i, part in enumerate(parts):
        np.savez_compressed(os.path.join(OUT, f"{name}.npz" if i == 0 else f"{name}.part{i}.npz"), **part)
    print(f"{name:16s} {len(parts)} file(s)   worst gradient f32-vs-f64 {max(list(d_grad.values()) + list(d_gx.values())):.2e}")


def main():
    os.makedirs(OUT, exist_ok=True)
    mgn.install()
    ref = mgn._load("experiments.rmag.models", os.path.join(mgn.REF, "rmag", "models.py"))
    common = dict(node_types=list(ref.NODE_TYPES), edge_types=[list(k) for k in ref.EDGE_TYPES],
                  present=[i for i in range(len(ref.EDGE_TYPES)) if i != LEFT_OUT], chunk=CHUNK)
    for c in LAYER_CASES:
        rng = np.random.default_rng(c["seed"])
        torch.manual_seed(c["seed"])
        conv = ref.RGCNConv(c["fin"], c["fout"])
        shapes = [(k, list(v.shape)) for k, v in conv.state_dict().items()]
        meta = dict(common, fin=c["fin"], fout=c["fout"], param_shapes=shapes, gout_seed=c["seed"] + 100)
        if c.get("params_from_seed"):
            meta.update(params_from_seed=True, param_seed=c["seed"] + 200, param_scale=1.0 / np.sqrt(c["fin"]))
            state = {k: torch.from_numpy(v) for k, v in seeded_arrays(shapes, meta["param_seed"], meta["param_scale"]).items()}
        else:
            state = {k: v.clone() for k, v in conv.state_dict().items()}
        x_np = {k: rng.standard_normal((n, c["fin"])).astype(np.float32) for k, n in c["sizes"].items()}
        adj, arrays = make_edges(rng, ref, c["sizes"], c["edges"])
        gout = seeded_arrays([(k, (c["sizes"][k], c["fout"])) for k in ref.NODE_TYPES], meta["gout_seed"])
        res = run_both(conv, state, x_np, adj, gout)
        arrays.update({f"x_{k}": v for k, v in x_np.items()})
        if not c.get("params_from_seed"):
            arrays.update({f"p_{k}": v.numpy() for k, v in state.items()})
        save_case(c["name"], meta, arrays, res, c.get("grads_as_f32", False))
    for c in NET_CASES:
        rng = np.random.default_rng(c["seed"])
        torch.manual_seed(c["seed"])
        n = NET
        net = ref.REGC.__new__(ref.REGC)
        torch.nn.Module.__init__(net)
        net.embs = torch.nn.ParameterDict({k: torch.nn.Parameter(torch.empty(n["sizes"][k], n["in_features"]))
                                           for k in ref.NODE_TYPES if k not in ref.X_TYPES})
        widths = [n["in_features"]] + [n["hidden"]] * (n["num_layers"] - 2)
        net.convs = torch.nn.ModuleList(
            [ref.REGConv(w, n["hidden"], n["heads"], n["bases"]) if c["use_egc"] else ref.RGCNConv(w, n["hidden"]) for w in widths]
            + [ref.RGCNConv(n["hidden"], n["num_classes"])])
        net.dropout = 0.5
        net.reset_parameters()
        net.eval()
        state = {k: v.clone() for k, v in net.state_dict().items()}
        shapes = [(k, list(v.shape)) for k, v in state.items()]
        meta = dict(common, use_egc=c["use_egc"], num_layers=n["num_layers"], hidden=n["hidden"], in_features=n["in_features"],
                    num_classes=n["num_classes"], heads=n["heads"], bases=n["bases"], sizes=n["sizes"], dropout=0.5,
                    param_shapes=shapes, gout_seed=c["seed"] + 100)
        x_np = {"paper": rng.standard_normal((n["sizes"]["paper"], n["in_features"])).astype(np.float32)}
        adj, arrays = make_edges(rng, ref, n["sizes"], n["edges"])
        gout = seeded_arrays([(k, (n["sizes"][k], n["num_classes"])) for k in ref.NODE_TYPES], meta["gout_seed"])
        res = run_both(net, state, x_np, adj, gout)
        arrays.update({f"x_{k}": v for k, v in x_np.items()})
        arrays.update({f"p_{k}": v.numpy() for k, v in state.items()})
        save_case(c["name"], meta, arrays, res)


if __name__ == "__main__":
    main()
