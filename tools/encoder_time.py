#!/usr/bin/env python3
"""Time of the node encoders (egc_encoder_forward_f32 / egc_encoder_backward_f32 under egc_amd.AtomEncoder, ASTNodeEncoder
and Embedding) against what they replace: nn.Embedding modules composed as the reference composes them (nine lookups and
adds for AtomEncoder, three and a clamp for ASTNodeEncoder, one for the ZINC nets), forward and backward separately.

HIP events, warmed up, median of the repetitions; the contenders alternate repetition by repetition in ONE process, in
the order B1, A, B2: B is timed as two series and |B1 - B2| is the spread this run shows for identical work.  A passes a
shape when it is not slower than the mean of B1 and B2 by more than that spread.  The backward is torch.autograd.grad on
retained forward graphs (no accumulation into .grad for either side); the gradient rows d_out rotate over more than
256 MiB so that they do not live in the Infinity Cache.  Algorithmic bytes: N T 8 + N F 4 forward,
N F 4 + N T 8 + sum R_t F 4 backward; their share of 8 TB/s is given for A.
"""
import argparse
import json
import os
import sys

import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402
from egc_amd import workloads as wl  # noqa: E402
from egc_amd.encoders import ATOM_FEATURE_DIMS  # noqa: E402

PEAK = 8e12
AST_ROWS, MAX_DEPTH = (98, 10030, 21), 20


class TorchAtom(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList([nn.Embedding(r, width) for r in ATOM_FEATURE_DIMS])

    def forward(self, x):
        out = 0
        for i in range(x.shape[1]):
            out = out + self.atom_embedding_list[i](x[:, i])
        return out


class TorchAST(nn.Module):
    def __init__(self, width):
        super().__init__()
        self.type_encoder, self.attribute_encoder = nn.Embedding(AST_ROWS[0], width), nn.Embedding(AST_ROWS[1], width)
        self.depth_encoder = nn.Embedding(MAX_DEPTH + 1, width)

    def forward(self, x, depth):
        depth[depth > MAX_DEPTH] = MAX_DEPTH
        return self.type_encoder(x[:, 0]) + self.attribute_encoder(x[:, 1]) + self.depth_encoder(depth)


def series(fns, reps, min_window_us=2000.0):
    """Interleaved timing: per repetition every fn in turn, a fixed number of calls between two events -- per fn as many
    as make the window at least `min_window_us` long (from a first window of 20 calls).  Median microseconds per call."""
    def window(fn, iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(iters):
            fn(i)
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / iters * 1e3
    iters = [max(20, int(min_window_us / max(window(fn, 20), 1e-3)) + 1) for fn in fns]
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ts[k].append(window(fn, iters[k]))
    return [sorted(t)[len(t) // 2] for t in ts]


def indices(n, rows, seed, hi=None):
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, (hi or {}).get(t, r), (n,), generator=g) for t, r in enumerate(rows)], dim=1)


def encoder_shapes(args, dev):
    shapes = (("molhiv b2048", "atom", lambda: wl.molecule_batch(2048, seed=0)[1], (224, 296)),
              ("zinc b128", "zinc", lambda: wl.zinc_like_batch(128, seed=0)[2], (168,)),
              ("zinc b2048", "zinc", lambda: wl.zinc_like_batch(2048, seed=0)[2], (168,)),
              ("code b128", "ast", lambda: wl.code_like_batch(128, seed=0)[1], (304,)))
    records = []
    for name, kind, n_of, widths in shapes:
        if not name.startswith(args.only):
            continue
        n = n_of()
        for width in widths:
            if args.width and width != args.width:
                continue
            torch.manual_seed(0)
            if kind == "atom":
                rows, a, b = ATOM_FEATURE_DIMS, egc_amd.AtomEncoder(width), TorchAtom(width)
                inputs = (indices(n, rows, 1).to(dev),)
            elif kind == "zinc":
                rows, a, b = (28,), egc_amd.Embedding(28, width), nn.Embedding(28, width)
                inputs = (indices(n, rows, 1)[:, 0].contiguous().to(dev),)
            else:
                rows, a, b = AST_ROWS, egc_amd.ASTNodeEncoder(width, AST_ROWS[0], AST_ROWS[1], MAX_DEPTH), TorchAST(width)
                idx = indices(n, rows, 1, {2: 40})
                inputs = (idx[:, :2].contiguous().to(dev), idx[:, 2].contiguous().to(dev))
            a, b = a.to(dev), b.to(dev)
            b.load_state_dict(a.state_dict(), strict=True)
            pa, pb = list(a.parameters()), list(b.parameters())
            copies = max(2, min(256, -(-300 * 2 ** 20 // (n * width * 4))))
            gos = [torch.randn(n, width, device=dev) for _ in range(copies)]
            b_inputs = tuple(t.clone() for t in inputs)      # (the reference's AST encoder clamps its depth in place)
            out_a, out_b = a(*inputs), b(*(t.clone() for t in inputs))     # (graphs kept for the backward: own inputs)
            assert torch.equal(out_a, out_b), "forward bits differ from the torch composition"

            def fwd_a(i):
                a(*inputs)

            def fwd_b(i):
                b(*b_inputs)

            def bwd_a(i):
                torch.autograd.grad(out_a, pa, gos[i % copies], retain_graph=True)

            def bwd_b(i):
                torch.autograd.grad(out_b, pb, gos[i % copies], retain_graph=True)

            def nograd(fn):
                def call(i):
                    with torch.no_grad():
                        fn(i)
                return call

            if args.profile:
                torch.cuda.synchronize()
                for i in range(10 if args.profile != "none" else 0):
                    if args.profile == "a":
                        torch.autograd.grad(a(*inputs), pa, gos[i % copies])
                    elif args.profile == "b-fwd":
                        b(*b_inputs)
                    else:
                        torch.autograd.grad(b(*b_inputs), pb, gos[i % copies])
                torch.cuda.synchronize()
                print(json.dumps(dict(workload=name, width=width, profile=args.profile, calls=10)), flush=True)
                return records
            for fn in (fwd_a, fwd_b, bwd_a, bwd_b):
                for i in range(3):
                    fn(i)
            torch.cuda.synchronize()
            t, total = len(rows), sum(rows)
            for direction, fa, fb, by in (("forward", fwd_a, fwd_b, n * t * 8 + n * width * 4),
                                          ("forward (no grad)", nograd(fwd_a), nograd(fwd_b), n * t * 8 + n * width * 4),
                                          ("backward", bwd_a, bwd_b, n * width * 4 + n * t * 8 + total * width * 4)):
                b1, us_a, b2 = series([fb, fa, fb], args.reps)
                spread = abs(b1 - b2)
                rec = dict(workload=name, rows=n, tables=t, table_rows=total, width=width, direction=direction,
                           a_us=round(us_a, 2), b_us=[round(b1, 2), round(b2, 2)], spread_us=round(spread, 2),
                           bytes=by,
                           a_share_of_8TBps=round(by / (us_a * 1e-6) / PEAK, 4),
                           not_slower=bool(us_a <= (b1 + b2) / 2 + spread))
                records.append(rec)
                print(json.dumps(rec), flush=True)
            del gos, out_a, out_b
    return records


def training_step(args, dev):
    """tools/batch_train_step_time.py's net at its default shape -- 4 x FusedEGCBlock(EGConv 128 / H8 / B4, sum + mean + max +
    symnorm) on the molhiv batch of 2,048 graphs, COO edge list, backward from a fixed gradient -- behind an encoder with
    an input dropout of 0.2.  Microseconds per step (wall clock over synchronised loops)."""
    import time
    width = 128
    ei, n, _ = wl.molecule_batch(2048, seed=0)
    ei = ei.to(dev)
    x = indices(n, ATOM_FEATURE_DIMS, 1).to(dev)
    gout = torch.randn(n, width, device=dev)

    def net(head):
        torch.manual_seed(0)
        blocks = nn.ModuleList([egc_amd.FusedEGCBlock(egc_amd.EGConv(width, width, aggrs=["sum", "mean", "max", "symnorm"],
                                                                     num_heads=8, num_bases=4), nn.BatchNorm1d(width))
                                for _ in range(4)])
        m = nn.ModuleList([head, blocks]).to(dev).train()
        params = list(m.parameters())

        def step():
            h = m[0](x)
            for blk in m[1]:
                h = blk(h, ei)
            h.backward(gout)

        def eager():
            for p in params:
                p.grad = None
            step()
        return step, eager, params

    def wall(fn, it=30):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(it):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / it * 1e6

    step_a, eager_a, params_a = net(egc_amd.AtomEncoder(width, dropout=0.2))
    _, eager_b, _ = net(nn.Sequential(TorchAtom(width), nn.Dropout(0.2)))
    b1, a, b2 = wall(eager_b), wall(eager_a), wall(eager_b)
    graphed = egc_amd.GraphedStep(step_a, params=params_a)
    rec = dict(workload="molhiv b2048 4-block training step, encoder + dropout 0.2 at the head", width=width,
               eager_a_us=round(a, 1), eager_b_us=[round(b1, 1), round(b2, 1)], recorded_a_us=round(wall(graphed), 1))
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="", help="workload name prefix")
    ap.add_argument("--width", type=int, default=0, help="only this width")
    ap.add_argument("--profile", default="", choices=("", "a", "b-fwd", "b", "none"), help="no timing: ten calls for rocprofv3")
    ap.add_argument("--step", action="store_true", help="also the 4-block molhiv training step behind the encoder")
    ap.add_argument("--json", default=None, help="write every record to this file")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("encoder_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    records = encoder_shapes(args, dev)
    if args.profile:
        return
    step = training_step(args, dev) if args.step else None
    print(f"\n{'workload':<14}{'width':>6} {'direction':<18}{'A us':>9}{'B1 us':>9}{'B2 us':>9}{'spread':>8}{'MB':>8}{'A of 8 TB/s':>13}  verdict")
    for r in records:
        print(f"{r['workload']:<14}{r['width']:>6} {r['direction']:<18}{r['a_us']:>9.2f}{r['b_us'][0]:>9.2f}{r['b_us'][1]:>9.2f}"
              f"{r['spread_us']:>8.2f}{r['bytes'] / 1e6:>8.1f}{100 * r['a_share_of_8TBps']:>12.1f}%  {'ok' if r['not_slower'] else 'SLOWER'}")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(encoders=records, training_step=step), f, indent=1)


if __name__ == "__main__":
    main()
