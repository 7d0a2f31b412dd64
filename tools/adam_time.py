#!/usr/bin/env python3
"""Time of the optimizer step of the reference's nets -- Adam(lr, weight_decay) followed by zeroing the gradients -- on the
parameter sets of

    zinc    ZincNetLike, EGC-S 168 / H8 / B4, 4 layers      (tests/callers.py)
    molhiv  HIVNetLike, EGC-S 296 / H8 / B4, 4 layers
    arxiv   ArxivNetLike, EGC-S 184 / H8 / B4, 3 layers

with random gradients, three contenders in one process:

    A = egc_amd.Adam.step(zero_grad=True)                                       (egc_adam.hip, one launch per 120 tensors)
    B = torch.optim.Adam(capturable=True, foreach=True) + zero_grad(set_to_none=False)
    C = torch.optim.Adam(fused=True, capturable=True)   + zero_grad(set_to_none=False)

eager (host-bound: what a loop without hipGraph sees) and as ONE captured graph each (what GraphedStep replays).  Every
repetition times B1 / A / B2 and C1 / A / C2 in turn: |B1 - B2| is the spread this run shows between two runs of the same
code, and A is not slower than B where it lies at or below the larger of the two.  HIP events, `iters` calls per window, the
median of `reps` windows, three warm-up calls first.  The launch counts are egc_adam_launch_count's for A and the device
activities torch's profiler sees in one eager call for B and C.

--step: the ZINC b128 iteration of DESIGN.md section 3.31 (tools/collate_time.py: Embedding -> 4 x FusedEGCBlock -> mean pool
-> Linear -> loss -> optimizer, next() inside) as ONE recording with A, with B and with SGD as it stands there; wall clock
over 200 replays, every contender twice, alternating.  Raw records go to --out (profiles/adam_time.json)."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import egc_amd  # noqa: E402
from egc_amd import _optim  # noqa: E402
import callers  # noqa: E402
from head_time import graphed, series  # noqa: E402


def _egc_s(d):
    return egc_amd.EGConv(d, d, aggrs=["symnorm"], num_heads=8, num_bases=4)


NETS = (("zinc", lambda: callers.ZincNetLike(168, 4, _egc_s)), ("molhiv", lambda: callers.HIVNetLike(296, 4, _egc_s)),
        ("arxiv", lambda: callers.ArxivNetLike(184, 3, _egc_s)))
LR, WD = 1e-3, 5e-4          # zinc/configs.py's defaults


def contenders(net, dev):
    """Three copies of the net's parameters with the same random gradients, and the three steps."""
    sets = []
    for _ in range(3):
        params = [nn.Parameter(p.detach().clone().to(dev)) for p in net.parameters()]
        gen = torch.Generator(device=dev).manual_seed(1)
        for p in params:
            p.grad = torch.randn(p.shape, device=dev, generator=gen)
        sets.append(params)
    a = egc_amd.Adam(sets[0], lr=LR, weight_decay=WD)
    b = torch.optim.Adam(sets[1], lr=LR, weight_decay=WD, capturable=True, foreach=True)
    c = torch.optim.Adam(sets[2], lr=LR, weight_decay=WD, capturable=True, fused=True)

    def a_step():
        a.step(zero_grad=True)

    def b_step():
        b.step()
        b.zero_grad(set_to_none=False)

    def c_step():
        c.step()
        c.zero_grad(set_to_none=False)
    return sets, a_step, b_step, c_step


def device_activities(fn):
    """Kernels, copies and memsets of one eager call as torch's profiler sees them (None where it is not available)."""
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == DeviceType.CUDA)
    except Exception as exc:  # noqa: BLE001
        print("launch count of a torch contender not available:", str(exc).splitlines()[0][:120], flush=True)
        return None


def pair(name, base, a_fn, iters, reps):
    """B1 / A / B2 around A for one baseline."""
    windows, med = series([base, a_fn, base], iters, reps)
    spread = abs(med[0] - med[2])
    return {f"{name}1_us": round(med[0], 2), "A_us": round(med[1], 2), f"{name}2_us": round(med[2], 2),
            "spread_us": round(spread, 2), "A_not_slower": bool(med[1] <= max(med[0], med[2])),
            "A_beats_both": bool(med[1] < min(med[0], med[2])), "speedup": round(min(med[0], med[2]) / med[1], 2),
            "windows_us": {k: [round(u, 2) for u in w] for k, w in zip((name + "1", "A", name + "2"), windows)}}


def optimizer_shapes(args, dev):
    lib = _optim.load()
    records, later = [], []
    for name, make in NETS:
        if name not in args.nets.split(","):
            continue
        torch.manual_seed(0)
        net = make()
        sets, a_step, b_step, c_step = contenders(net, dev)
        for fn in (b_step, c_step, a_step):
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        n0 = lib.egc_adam_launch_count()
        a_step()
        rec = dict(net=name, tensors=len(sets[0]), elements=sum(p.numel() for p in sets[0]), iters=args.iters, reps=args.reps,
                   launches=dict(A=lib.egc_adam_launch_count() - n0))
        rec["eager"] = dict(vs_B=pair("B", b_step, a_step, args.iters, args.reps), vs_C=pair("C", c_step, a_step, args.iters, args.reps))
        ga, gb, gc = graphed(a_step), graphed(b_step), graphed(c_step)
        rec["graph"] = dict(vs_B=pair("B", gb.replay, ga.replay, args.iters, args.reps),
                            vs_C=pair("C", gc.replay, ga.replay, args.iters, args.reps))
        records.append(rec)
        later.append((rec, b_step, c_step))
        print(json.dumps({k: ({m: {kk: vv for kk, vv in v[m].items() if kk != "windows_us"} for m in v} if k in ("eager", "graph") else v)
                          for k, v in rec.items()}), flush=True)
    return records, later


def training_step(dev):
    """The ZINC b128 iteration of tools/collate_time.py as one recording, the optimizer swapped."""
    from collate_time import build_store
    g, m, hidden = 128, 1024, 128
    store, _ = build_store("zinc", m, 0, dev)
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(1)).to(dev)

    def recording(kind):
        col = egc_amd.BatchCollator(store, g)
        col.set_epoch(perm)
        torch.manual_seed(0)
        blocks = nn.ModuleList([egc_amd.FusedEGCBlock(egc_amd.EGConv(hidden, hidden, aggrs=["sum", "mean", "max", "symnorm"],
                                                                     num_heads=8, num_bases=4), nn.BatchNorm1d(hidden))
                                for _ in range(4)])
        net = nn.ModuleList([egc_amd.Embedding(28, hidden), blocks, nn.Linear(hidden, 1)]).to(dev).train()
        params = list(net.parameters())
        if kind == "A":
            opt = egc_amd.Adam(params, lr=LR, weight_decay=WD)
        elif kind == "B":
            opt = torch.optim.Adam(params, lr=LR, weight_decay=WD, capturable=True, foreach=True)
        else:
            opt = torch.optim.SGD(params, lr=0.01, foreach=True)

        def step():
            col.next()
            h = net[0](col.fields["atom"])
            for blk in net[1]:
                h = blk(h, col.edge_index, n_valid=col.n_valid)
            out = net[2](egc_amd.global_mean_pool(h, col.batch, size=g + 1))
            (((out - col.fields["y"]) ** 2 * col.graph_mask).sum() * col.inv_g).backward()
            if kind == "A":
                opt.step(zero_grad=True)
            else:
                opt.step()
                opt.zero_grad(set_to_none=False)
        return egc_amd.GraphedStep(step, params=params), col

    def wall(fn, it=200):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(it):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / it * 1e6

    recs = {kind: recording(kind) for kind in ("A", "B", "SGD")}
    order = ("B", "A", "SGD") * 2
    times = {kind: [] for kind in recs}
    for kind in order:
        times[kind].append(round(wall(recs[kind][0]), 1))
    for _, col in recs.values():
        col.check()
    rec = dict(workload="zinc b128 4-block training iteration, one recording, next() inside", width=hidden,
               tensors=len(list(recs["A"][0]._params)), A_us=times["A"], B_us=times["B"], SGD_us=times["SGD"])
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--nets", default="zinc,molhiv,arxiv", help="which of the nets' parameter sets to time")
    ap.add_argument("--step", action="store_true", help="also the ZINC b128 training iteration as one recording with A, B and SGD")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adam_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    records, later = optimizer_shapes(args, dev)
    out = dict(device=torch.cuda.get_device_name(0), lr=LR, weight_decay=WD, records=records)
    if args.step:
        out["training_step"] = training_step(dev)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    write()
    for rec, b_step, c_step in later:       # last: the profiler stays out of every timed window
        rec["launches"].update(B=device_activities(b_step), C=device_activities(c_step))
        print(json.dumps(dict(net=rec["net"], launches=rec["launches"])), flush=True)
    write()


if __name__ == "__main__":
    main()
