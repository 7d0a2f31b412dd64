#!/usr/bin/env python3
"""Time of the graph-level readouts (egc_segment_reduce_f32 / egc_segment_reduce_backward_f32) on the batch workloads:
ZINC-like and molhiv-like batches of 2,048 graphs and a CIFAR-superpixel-like batch of 128, at width 128 and at the width
of the reference's net for that data set (168 / 296 / 168).  Per record: microseconds (HIP events, median of the
repetitions), algorithmic bytes (x read once + out (+ arg) written; the mirror for the backward) and their share of 8 TB/s.

The inputs rotate over enough copies of x to exceed the 256 MiB Infinity Cache: a readout reads its input once per step,
behind a layer that wrote other things since.

--parent-lib PATH: a libegc_hip.so built from the parent commit.  Its egc_segment_mean_f32 is then timed twice
(series P1 and P2) interleaved with the mean forward of this tree's library in the same process, repetition by repetition:
|P1 - P2| is the spread this run shows between two runs of the same kernel, and the new kernel passes a shape when it is not
slower than the parent's mean by more than that.  The mean backward is timed against the three torch operators it replaced
(clamp, divide, index_select) the same way; reported only."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import egc_amd  # noqa: E402,F401
from egc_amd import _C, workloads as wl  # noqa: E402
from egc_amd import functional as F  # noqa: E402

PEAK = 8e12
OPS = ("sum", "mean", "max")


def series(fns, iters, reps):
    """Interleaved timing: per repetition every fn in turn, `iters` calls between two events.  Median microseconds per call."""
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, fn in enumerate(fns):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                fn(i)
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) / iters * 1e3)
    return [sorted(t)[len(t) // 2] for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="", help="workload name prefix")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("readout_time.py needs the GPU: a timing taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib = _C.load()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.egc_segment_mean_f32.restype = C.c_int
        parent.egc_segment_mean_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p]
    stream = torch.cuda.current_stream().cuda_stream
    shapes = (("zinc b2048", lambda: wl.zinc_like_batch(2048, seed=0)[3], (128, 168)),
              ("molhiv b2048", lambda: wl.molecule_batch(2048, seed=0)[2], (128, 296)),
              ("cifar b128", lambda: wl.knn_superpixel_batch(128, seed=0)[2], (128, 168)))
    records, verdicts = [], []
    for name, gen, widths in shapes:
        if not name.startswith(args.only):
            continue
        batch = gen().to(dev)
        n, G = batch.numel(), int(batch.max()) + 1
        seg = torch.searchsorted(batch, torch.arange(G + 1, device=dev))
        for width in widths:
            x_bytes = n * width * 4
            copies = max(2, min(64, -(-600 * 2 ** 20 // x_bytes)))
            xs = [torch.randn(n, width, device=dev) for _ in range(copies)]
            dxs = [torch.empty(n, width, device=dev) for _ in range(copies)]
            out = torch.empty(G, width, device=dev)
            arg = torch.empty(G, width, dtype=torch.int32, device=dev)
            go = torch.randn(G, width, device=dev)

            def fwd(code, want_arg=False):
                def call(i):
                    st = lib.egc_segment_reduce_f32(xs[i % copies].data_ptr(), seg.data_ptr(), G, n, width, code, out.data_ptr(),
                                                    arg.data_ptr() if want_arg else None, stream)
                    assert st == 0, st
                return call

            def bwd(code):
                def call(i):
                    st = lib.egc_segment_reduce_backward_f32(go.data_ptr(), seg.data_ptr(), arg.data_ptr(), G, n, width, code,
                                                             dxs[i % copies].data_ptr(), stream)
                    assert st == 0, st
                return call

            def parent_mean(i):
                st = parent.egc_segment_mean_f32(xs[i % copies].data_ptr(), seg.data_ptr(), G, width, out.data_ptr(), stream)
                assert st == 0, st

            def torch_mean_bwd(i):
                counts = (seg[1:] - seg[:-1]).clamp_(min=1).to(go.dtype)
                torch.index_select(go / counts[:, None], 0, batch, out=dxs[i % copies])

            fwd(_C.READOUT_MAX, True)(0)      # a valid arg for the max backward; also the first launch of the code object
            fns = {"sum fwd": fwd(_C.READOUT_SUM), "mean fwd": fwd(_C.READOUT_MEAN), "max fwd": fwd(_C.READOUT_MAX),
                   "max+arg fwd": fwd(_C.READOUT_MAX, True), "sum bwd": bwd(_C.READOUT_SUM), "mean bwd": bwd(_C.READOUT_MEAN),
                   "max bwd": bwd(_C.READOUT_MAX), "torch mean bwd (3 ops)": torch_mean_bwd}
            if parent is not None:
                fns["parent mean fwd P1"] = parent_mean
                fns["parent mean fwd P2"] = parent_mean
                # the order inside a repetition: P1, new, P2
                order = ["parent mean fwd P1", "mean fwd", "parent mean fwd P2"] + [k for k in fns if k not in
                                                                                  ("parent mean fwd P1", "mean fwd", "parent mean fwd P2")]
            else:
                order = list(fns)
            for k in order:                   # warm-up of every shape and kernel the timed window uses
                for i in range(3):
                    fns[k](i)
            torch.cuda.synchronize()
            med = dict(zip(order, series([fns[k] for k in order], args.iters, args.reps)))
            small = G * width * 4
            for k in order:
                by = x_bytes + small + (small if "arg" in k or k == "max bwd" else 0)
                rec = dict(workload=name, rows=n, graphs=G, width=width, kernel=k, us=round(med[k], 2), bytes=by,
                           share_of_8TBps=round(by / (med[k] * 1e-6) / PEAK, 4))
                records.append(rec)
                print(json.dumps(rec), flush=True)
            if parent is not None:
                p1, p2, new = med["parent mean fwd P1"], med["parent mean fwd P2"], med["mean fwd"]
                spread = abs(p1 - p2)
                ok = new <= (p1 + p2) / 2 + spread
                verdicts.append(dict(workload=name, width=width, parent_us=[round(p1, 2), round(p2, 2)], new_us=round(new, 2),
                                     spread_us=round(spread, 2), not_slower=bool(ok)))
                print(json.dumps(verdicts[-1]), flush=True)
                # the two libraries agree bit for bit on this input
                ref = torch.empty_like(out)
                parent.egc_segment_mean_f32(xs[0].data_ptr(), seg.data_ptr(), G, width, ref.data_ptr(), stream)
                assert torch.equal(ref, F.segment_reduce(xs[0], seg, "mean")), "mean bits changed"
            del xs, dxs
    print(f"\n{'workload':<14}{'width':>6}  {'kernel':<24}{'us':>9}{'MB':>9}{'of 8 TB/s':>11}")
    for r in records:
        print(f"{r['workload']:<14}{r['width']:>6}  {r['kernel']:<24}{r['us']:>9.2f}{r['bytes'] / 1e6:>9.1f}{100 * r['share_of_8TBps']:>10.1f}%")
    if verdicts:
        print("\nmean forward against the parent's egc_segment_mean_f32:", "PASS" if all(v["not_slower"] for v in verdicts) else "FAIL")


if __name__ == "__main__":
    main()
