"""Fixtures and CPU restatement of the R-GCN baseline layer and the REGC net (tests/golden/rgcn/rgcn_*.npz, regc_*.npz, written by
tests/golden/make_golden_rgcn.py from the reference's own RGCNConv / REGC.forward).

The restatement is sequential numpy in one dtype.  ``chunked_row_mean`` is the documented summation order of
egc_amd/csrc/egc_typed_mean.hip: a row's entries, in the order of the edge list, are cut into consecutive chunks of
``chunk`` entries; a chunk's sum is ((0 + v0) + v1) + ..., the row's sum is chunk 0's with the sums of chunks 1, 2, ...
added in ascending order, and the mean divides that sum by the entry count -- every step one correctly rounded IEEE
operation of the dtype, so in float32 these ARE the kernel's bits.

A fixture too large for one file is spread over ``<name>.npz`` and ``<name>.part<k>.npz`` (the loader merges them).  Where
``meta["params_from_seed"]`` is set the parameters are not stored: generator and loader both draw them from
``seeded_arrays`` -- and the cotangents of every fixture come from there too."""
import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rgcn")
LAYER_FIXTURES = ("rgcn_small", "rgcn_odd", "rgcn_mag_shape")
NET_FIXTURES = ("regc_egc", "regc_rgcn")


def seeded_arrays(names_shapes, seed, scale=1.0):
    """{name: float32 array of the shape}: standard normals times ``scale``, drawn in the order given from one
    numpy Generator (PCG64: the same stream on every machine)."""
    rng = np.random.default_rng(seed)
    return {k: (scale * rng.standard_normal(tuple(shape))).astype(np.float32) for k, shape in names_shapes}


def load_rgcn_golden(name):
    files = [os.path.join(GOLDEN, f"{name}.npz")] + sorted(glob.glob(os.path.join(GOLDEN, f"{name}.part*.npz")))
    z = {}
    for f in files:
        with np.load(f) as part:
            z.update({k: part[k] for k in part.files})
    meta = json.loads(bytes(z["meta"]).decode())
    types = meta["node_types"]
    g = dict(meta=meta, name=name)
    g["ei"] = {tuple(meta["edge_types"][i]): z[f"ei_{i}"] for i in meta["present"]}
    if meta.get("params_from_seed"):
        g["params"] = seeded_arrays(meta["param_shapes"], meta["param_seed"], meta["param_scale"])
    else:
        g["params"] = {k: z[f"p_{k}"] for k, _ in meta["param_shapes"]}
    g["x"] = {k: z[f"x_{k}"] for k in types if f"x_{k}" in z}
    g["out32"] = {k: z[f"out32_{k}"] for k in types}
    g["out64"] = {k: z[f"out64_{k}"] for k in types}
    g["gout"] = seeded_arrays([(k, g["out32"][k].shape) for k in types], meta["gout_seed"])
    g["grad_x64"] = {k: z[f"grad_x64_{k}"].astype(np.float64) for k in types if f"grad_x64_{k}" in z}
    g["grad64"] = {k[len("grad64:"):]: z[k].astype(np.float64) for k in z if k.startswith("grad64:")}
    return g


def rel_out(a, b):
    """max |a - b| relative to max(1, max |b|): the distance of outputs (tests/test_nets_golden.py)."""
    b = np.asarray(b, dtype=np.float64)
    if b.size == 0:
        return 0.0
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(1.0, float(np.abs(b).max())))


def rel_grad(a, b):
    """max |a - b| relative to max |b|: the distance of gradients (relgrad_* fixtures)."""
    b = np.asarray(b, dtype=np.float64)
    if b.size == 0:
        return 0.0
    return float(np.abs(np.asarray(a, dtype=np.float64) - b).max() / max(1e-30, float(np.abs(b).max())))


def reference_distance(g):
    """The reference's own float32 against its float64 output on this fixture, from the two outputs stored in it."""
    return max(rel_out(g["out32"][k], g["out64"][k]) for k in g["meta"]["node_types"])


def csr_by_destination(ei, n_dst):
    """(rowptr, source ids in row order) of an edge list [2, E] (row 0 = sources, row 1 = destinations), stable inside
    a row: a row's entries keep the order of the edge list."""
    src, dst = np.asarray(ei[0]), np.asarray(ei[1])
    order = np.argsort(dst, kind="stable")
    rowptr = np.zeros(n_dst + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n_dst), out=rowptr[1:])
    return rowptr, src[order]


def chunked_row_mean(x_src, ei, n_dst, chunk, dtype=np.float32):
    """mean over every destination's in-neighbours of x_src in the documented order (module docstring); 0 for a row
    without entries."""
    x_src = np.asarray(x_src, dtype=dtype)
    rowptr, col = csr_by_destination(ei, n_dst)
    out = np.zeros((n_dst, x_src.shape[1]), dtype=dtype)
    for row in range(n_dst):
        p0, p1 = int(rowptr[row]), int(rowptr[row + 1])
        if p1 == p0:
            continue
        total = None
        for s in range(p0, p1, chunk):
            acc = np.zeros(x_src.shape[1], dtype=dtype)
            for p in range(s, min(s + chunk, p1)):
                acc = acc + x_src[col[p]]
            total = acc if total is None else total + acc
        out[row] = total / dtype(p1 - p0)
    return out


def typed_operands(x, ei, edge_types, chunk, dtype=np.float32):
    """{type: [x_t | mean of relation 1 | mean of relation 2 ...]} with a type's relations in the order of
    ``edge_types`` (those present in ``ei``), and {type: the relations of its blocks}."""
    ops, blocks = {}, {}
    for t, xt in x.items():
        rels = [tuple(k) for k in edge_types if tuple(k) in ei and k[2] == t]
        parts = [np.asarray(xt, dtype=dtype)] + [chunked_row_mean(x[k[0]], ei[k], xt.shape[0], chunk, dtype) for k in rels]
        ops[t], blocks[t] = np.concatenate(parts, axis=1), rels
    return ops, blocks


def rgcn_forward(x, ei, params, edge_types, chunk, dtype=np.float32, prefix=""):
    """out[t] = root_lins[t](x[t]) + sum over the relations into t of rel_lins[s_r_t](mean) (rmag/models.py:61-72)."""
    ops, blocks = typed_operands(x, ei, edge_types, chunk, dtype)
    out = {}
    for t, a in ops.items():
        names = [f"{prefix}root_lins.{t}.weight"] + [f"{prefix}rel_lins.{k[0]}_{k[1]}_{k[2]}.weight" for k in blocks[t]]
        wcat = np.concatenate([np.asarray(params[n], dtype=dtype) for n in names], axis=1)
        out[t] = a @ wcat.T + np.asarray(params[f"{prefix}root_lins.{t}.bias"], dtype=dtype)
    return out
