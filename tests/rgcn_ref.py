"""Fixtures and CPU restatement of the R-GCN baseline layer and the REGC net (tests/golden/rgcn/rgcn_*.npz, regc_*.npz, written by
tests/golden/make_golden_rgcn.py from the reference's own RGCNConv / REGC.forward).

The restatement is sequential numpy in one dtype.  ``chunked_row_mean`` is the documented summation order of
egc_amd/csrc/egc_typed_mean.hip: a row's entries, in the order of the edge list, are cut into consecutive chunks of
``chunk`` entries; a chunk's sum is ((0 + v0) + v1) + ..., the row's sum is chunk 0's with the sums of chunks 1, 2, ...
added in ascending order, and the mean divides that sum by the entry count -- every step one correctly rounded IEEE
operation of the dtype, so in float32 these ARE the kernel's bits.  ``typed_mean_restated`` is the same for a whole launch
in either of the kernel's forms (several relations, ``pre_rowptr``, ``post_mean``, column blocks or accumulation in list order).

A fixture too large for one file is spread over ``<name>.npz`` and ``<name>.part<k>.npz`` (the loader merges them).  Where
``meta["params_from_seed"]`` is set the parameters are not stored: generator and loader both draw them from
``seeded_arrays`` -- and the cotangents of every fixture come from there too."""
import glob
import json
import os
from typing import NamedTuple

import numpy as np

from mpnn_ref import CHUNK, LADDER, WIDTHS, ladder_graph, ladder_inputs, ladder_lengths  # noqa: F401  (the shared sweep graph)

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


class RelSpec(NamedTuple):
    """One relation of a typed-mean launch as numpy, field for field egc_amd._typed.TypedRel: ``csr`` = (rowptr, col) of the rows
    of the launch, or None for the identity relation; ``inp`` [rows the entries name, >= in_col + width]; ``pre_rowptr``: None or
    the rowptr whose row lengths scale the entries; ``post_mean``; ``out_col``."""
    csr: tuple | None
    inp: np.ndarray
    in_col: int = 0
    pre_rowptr: np.ndarray | None = None
    post_mean: bool = False
    out_col: int = 0


def typed_mean_restated(rels, n_rows, width, accumulate=False, chunk=CHUNK, dtype=np.float32, n_cols=None, fill=0.0):
    """egc_typed_mean_f32 over the RelSpecs ``rels``, sequentially in ``dtype``, operation for operation in the kernel's order:
    an entry's value is inp[col] times dtype(1) / dtype(max(length of pre_rowptr's row col, 1)) -- a reciprocal, then one
    multiply -- where there is a pre_rowptr; a chunk's sum is ((0 + v0) + v1) + ... in entry order, the row's sum chunk 0's
    with those of chunks 1, 2, ... added in ascending order; ``post_mean`` is one division by the entry count (0 for an empty
    row).  ``accumulate``: out [n_rows, width] = ((0 + r0) + r1) + ... in list order; otherwise every relation writes columns
    out_col .. out_col + width of out [n_rows, n_cols] (default: as many as the blocks need), the others keep ``fill``."""
    if not accumulate and n_cols is None:
        n_cols = max([r.out_col + width for r in rels], default=0)
    out = np.zeros((n_rows, width), dtype=dtype) if accumulate else np.full((n_rows, n_cols), fill, dtype=dtype)
    for r in rels:
        x = np.asarray(r.inp, dtype=dtype)[:, r.in_col:r.in_col + width]
        if r.pre_rowptr is not None:
            x = x * (dtype(1) / np.maximum(np.diff(np.asarray(r.pre_rowptr)), 1).astype(dtype))[:, None]
        for row in range(n_rows):
            if r.csr is None:
                entries = (row,) if row < x.shape[0] else ()
            else:
                entries = r.csr[1][int(r.csr[0][row]):int(r.csr[0][row + 1])]
            total = np.zeros(width, dtype=dtype)
            for s in range(0, len(entries), chunk):
                acc = np.zeros(width, dtype=dtype)
                for j in entries[s:s + chunk]:
                    acc = acc + x[j]
                total = acc if s == 0 else total + acc
            if r.post_mean and len(entries):
                total = total / dtype(len(entries))
            if accumulate:
                out[row] = out[row] + total
            else:
                out[row, r.out_col:r.out_col + width] = total
    return out


def transposed_csr(csr, n_in_rows):
    """(rowptr, col) of the transposed of ``csr`` = (rowptr, col) over ``n_in_rows`` rows, a row's entries in ascending position
    of the CSR they come from: CSRGraph.transposed()."""
    rowptr, col = csr
    row_of = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return csr_by_destination(np.stack([row_of, np.asarray(col)]), n_in_rows)


EIGHT_ROWS = len(ladder_lengths(tail_empty=True))


def eight_relations(seed, width):
    """The relations of the one launch of EGC_TYPED_MAX_RELATIONS = 8 of tests/test_typed_mean_shapes_*.py, all over EIGHT_ROWS
    rows: [(edge_index [2, E] or None for the identity, input rows, input [input rows, width] float32)] -- identity; the ladder
    graph (its rows and three empty ones); 300 entries and no long row (workspace slots nobody writes or reads); 200 entries
    (no slots, between two relations that have some); the flip of the square ladder graph; identity again; no entries at all;
    the ladder graph with ``tail_empty`` from another seed."""
    rng = np.random.default_rng(seed)
    n = EIGHT_ROWS
    lad, n_lad, lad_src = ladder_graph(seed)
    flip, flip_dst, flip_src = ladder_graph(seed + 1, flip=True, tail_empty=True, square=True)
    tail, tail_dst, tail_src = ladder_graph(seed + 2, tail_empty=True)
    assert n_lad + 3 == flip_dst == flip_src == tail_dst == n

    def scattered(e, n_in):
        return np.stack([rng.integers(0, n_in, e), rng.integers(0, n, e)]).astype(np.int64), n_in

    shapes = [(None, n + 2), (lad, lad_src), scattered(300, 40), scattered(200, 57), (flip, flip_src), (None, n),
              (np.zeros((2, 0), dtype=np.int64), 10), (tail, tail_src)]
    return [(ei, n_in, rng.standard_normal((n_in, width)).astype(np.float32)) for ei, n_in in shapes]
