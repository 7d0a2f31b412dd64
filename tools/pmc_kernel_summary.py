#!/usr/bin/env python3
"""Condense rocprofv3 counter passes into one row per (pass, counter, kernel): the counter summed over its dimension
entries per dispatch, then the median over dispatches.  Only the benchmark's two kernels (the fp16x2 GEMM and the
register-resident aggregate) are kept.

    python tools/pmc_kernel_summary.py OUT.csv NAME=DIR [NAME=DIR ...]

Each DIR is a `rocprofv3 --pmc <counter> -d DIR -o pmc --output-format csv` output directory (pmc_counter_collection.csv
inside, possibly one level down).  Counter units are rocprofv3's (FETCH_SIZE / WRITE_SIZE in KiB; FETCH_SIZE is doubled by
the readers of this table, MI355X_MICROARCH.md)."""
import collections
import csv
import glob
import os
import sys

KEEP = ("basis_gemm_f16x2", "agg_fast_kernel")


def collection(d):
    hits = sorted(glob.glob(os.path.join(d, "pmc_counter_collection.csv")) + glob.glob(os.path.join(d, "*", "*counter_collection.csv")))
    if not hits:
        raise SystemExit(f"no counter collection under {d}")
    return hits[0]


def main():
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    rows_out = []
    for arg in sys.argv[2:]:
        name, d = arg.split("=", 1)
        per = collections.defaultdict(lambda: collections.defaultdict(float))
        for r in csv.DictReader(open(collection(d))):
            if any(k in r["Kernel_Name"] for k in KEEP):
                per[(r["Counter_Name"], r["Kernel_Name"])][r["Dispatch_Id"]] += float(r["Counter_Value"])
        for (counter, kernel), d_ in sorted(per.items()):
            v = sorted(d_.values())
            rows_out.append((name, counter, kernel, len(v), v[len(v) // 2]))
    with open(sys.argv[1], "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["build", "counter", "kernel", "dispatches", "median_per_dispatch"])
        for r in rows_out:
            w.writerow(r[:4] + (f"{r[4]:.6g}",))


if __name__ == "__main__":
    main()
