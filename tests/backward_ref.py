"""The sweep of the layer backward (egc_amd/csrc/egc_backward.hip) at every form it dispatches on: what
tests/test_backward_shapes_cpu.py checks without a device and tests/test_backward_shapes_gpu.py runs on one.

Four parts.

``aggregate_combine`` restates aggregate + combine at the OPERAND level: from ``bases`` [n_src, ldb] (each basis padded from L to
Ls columns; the padding takes no part), pre-activation ``weightings`` [N, H B A] in the HBA layout, the edge list, the aggregator
list, the two edge sets and the weight nonlinearity to ``out`` [N, H L], in torch on the CPU and differentiable.  The aggregators
are those of oracle/egc_torch_ref.py (``_aggregate`` / ``_scatter``), so the first-maximal-entry rule and its float32-rounded tie
decision are the ones every other gradient test uses.  Autograd through it in float64 is the truth for ``d_bases`` and
``d_weightings`` themselves -- no GEMM and no parameter gradient in between; the same function in float32 is the yardstick of what
one float32 evaluation of the same mathematics is worth.  ``arg_positions`` gives the edge every (row, column) extremum goes to.

``ladder`` is the sweep graph: SQUARE, one row of every length of LENGTHS on the destination side AND (in another order) on the
source side, the flip being the same graph transposed.  LENGTHS are the ladder of tests/mpnn_ref.py around the chunk size (256),
3 / 4 / 5 around the four-deep load pipeline of the source kernel, 63 / 64 / 65 around the long-row threshold, rows of one and two
entries (an entry that receives more columns than a record holds), 8 / 9 (the ballot ranking limit of the record builder, also as
the tail of a second chunk: 264 / 265).  ``rect`` (more or fewer source rows than there are destinations, short ones among them), ``sparse``
(many short rows: no records are built) and ``boundary`` (a graph exactly on, or one entry beyond, the rule that turns records
on) are its variants.

``dispatch`` restates, as data, which kernels ``egc_aggregate_combine_backward_f32`` launches for a layer on a graph, and
``arg_extrema_instance`` the instance of the separate arg pass of the training forward.  ``source_instances`` reads the rows of the
instance lists of egc_backward_host.h, which the launches expand from, so that an instance added there without a case here is
noticed; tests/test_backward_plan_cpu.py holds the C++ plan itself against ``dispatch``.

``CASES`` is the table: every cell of the rule at the smallest shape that reaches it, the trained nets' shapes among them."""
import functools
import os
import re
from typing import NamedTuple

import numpy as np
import torch

from egc_amd import _C
from egc_amd.functional import padded_basis_stride
from mpnn_ref import CHUNK, LADDER, rel_grad, rel_out  # noqa: F401  (the distances of every sweep)
from oracle import egc_oracle as orc
from oracle import egc_torch_ref as tref

THRESHOLD = _C.LONG_ROW_THRESHOLD
assert CHUNK == _C.LONG_ROW_CHUNK
CODES = {"sum": _C.AGGR_SUM, "mean": _C.AGGR_MEAN, "max": _C.AGGR_MAX, "min": _C.AGGR_MIN, "var": _C.AGGR_VAR, "std": _C.AGGR_STD,
         "symnorm": _C.AGGR_SYMNORM}
ACTS = {"none": _C.ACT_NONE, "softmax": _C.ACT_SOFTMAX, "sigmoid": _C.ACT_SIGMOID, "hardtanh": _C.ACT_HARDTANH}
# (set of every aggregator but symnorm, set of symnorm): EGConv without / with self loops, EfficientGraphConv with them
SETS = {"raw": (_C.SET_RAW, _C.SET_RAW), "looped": (_C.SET_LOOPED, _C.SET_LOOPED), "lay": (_C.SET_RAW, _C.SET_LOOPED)}
# ... and the pair neither layer class produces but the C ABI accepts (tests/forward_ref.py): what the restatement looks a name up in
ALL_SETS = dict(SETS, xl=(_C.SET_LOOPED, _C.SET_RAW))


class Case(NamedTuple):
    """One layer of the table.  ``dst``: the destination kernel the rule must choose for it (checked without a device)."""
    out: int
    H: int
    B: int
    aggrs: tuple
    sets: str
    dst: str
    act: str = "none"
    graph: str = "ladder"        # "reduced" (longest row 513) for rows of more than 256 columns

    @property
    def name(self):
        return (f"{self.out}-H{self.H}-B{self.B}-{'+'.join(self.aggrs)}-{self.sets}" + (f"-{self.act}" if self.act != "none" else ""))


def geometry(case):
    """(L, Ls, ldb, slots, A, W) of a case, with the basis stride the layers choose -- or the case's own ``stride``, where it
    has one (tests/forward_ref.py: an unpadded basis whose length is no multiple of 4)."""
    L = case.out // case.H
    Ls = getattr(case, "stride", 0) or padded_basis_stride(case.out, case.H, case.B)
    ldb = (case.B * Ls + 3) & ~3
    return L, Ls, ldb, ldb // 4, len(case.aggrs), case.H * case.B * len(case.aggrs)


def extrema(case):
    return ("max" in case.aggrs) + ("min" in case.aggrs)


def stdvar(case):
    return bool({"std", "var"} & set(case.aggrs))


# ------------------------------------------------------------------------------------------------------------------------------
# the operand-level restatement

def edge_sets(ei, n, sets, n_loop=None):
    """{set code: (edge list [2, E'], the raw edge every entry is -- E for an appended self loop)} for the two sets of ``sets``.
    ``n_loop``: a LOOPED set appends self loops to rows < n_loop only (a layer without ``loops_all_nodes``: 1 + the largest index
    of the edge list, as add_remaining_self_loops infers the node count); every row by default."""
    ei = np.asarray(ei, dtype=np.int64)
    e = ei.shape[1]
    n_loop = n if n_loop is None else n_loop
    got = {}
    for code in set(ALL_SETS[sets]):
        if code == _C.SET_RAW:
            got[code] = (ei, np.arange(e, dtype=np.int64))
        else:            # add_remaining_self_loops: existing loops dropped, one per node appended behind the remaining edges
            looped, _ = orc.add_remaining_self_loops(ei, None, 1.0, n_loop)
            got[code] = (looped, np.concatenate([np.nonzero(ei[0] != ei[1])[0], np.full(n_loop, e, dtype=np.int64)]))
    return got


def symnorm_weights(edges, n, dtype):
    """deg^-1/2 [source] deg^-1/2 [destination] per edge, deg = the in-degree over ``edges`` (gcn_norm), in ``dtype``."""
    deg = np.bincount(edges[1], minlength=n).astype(np.float64)
    with np.errstate(divide="ignore"):
        dis = np.where(deg > 0, deg ** -0.5, 0.0)
    return torch.from_numpy(dis[edges[0]] * dis[edges[1]]).to(dtype)


def real_columns(bases, B, L, Ls):
    """[rows, ldb] -> [rows, B L]: the columns that are not padding."""
    return bases[:, :B * Ls].reshape(bases.shape[0], B, Ls)[:, :, :L].reshape(bases.shape[0], B * L)


def activate(w, H, act):
    n = w.shape[0]
    if act == "softmax":
        return w.view(n, H, -1).softmax(dim=-1).reshape(n, -1)
    if act == "sigmoid":
        return torch.sigmoid(w)
    if act == "hardtanh":
        return torch.nn.functional.hardtanh(w)
    return w


def aggregate_combine(bases, weightings, ei, n, case, n_loop=None):
    """out [n, H L]; torch tensors of one dtype on the CPU, differentiable with respect to ``bases`` and ``weightings``.
    ``n_loop``: see ``edge_sets``."""
    L, Ls, ldb, _, A, W = geometry(case)
    assert bases.shape[1] == ldb and weightings.shape == (n, W)
    H, B = case.H, case.B
    xb = real_columns(bases, B, L, Ls)
    sets = edge_sets(ei, n, case.sets, n_loop)
    agg_code, sym_code = ALL_SETS[case.sets]
    aggs = []
    for a in case.aggrs:
        edges = sets[sym_code if a == "symnorm" else agg_code][0]
        idx = torch.from_numpy(edges)
        sw = symnorm_weights(edges, n, bases.dtype) if a == "symnorm" else None
        aggs.append(tref._aggregate(a, xb[idx[0]], idx[1], n, sw).view(n, B, L))
    agg = torch.stack(aggs, dim=1)                                        # [n, A, B, L]
    w = activate(weightings, H, case.act).view(n, H, B, A)
    return torch.einsum("nhba,nabl->nhl", w, agg).reshape(n, H * L)


def gradients(bases, weightings, gout, ei, n, case, dtype, n_loop=None):
    """(out, d_bases [n_src, ldb], d_weightings [n, W]) as numpy, evaluated in ``dtype`` from float32 inputs."""
    b = torch.from_numpy(bases).to(dtype).requires_grad_(True)
    w = torch.from_numpy(weightings).to(dtype).requires_grad_(True)
    out = aggregate_combine(b, w, ei, n, case, n_loop)
    out.backward(torch.from_numpy(gout).to(dtype))
    return out.detach().numpy(), b.grad.numpy(), w.grad.numpy()


def arg_positions(bases, ei, n, case, which, n_loop=None):
    """[n, B L] int64: the raw edge (position in ``ei``) the maximum (``which`` = "max") or minimum of every (row, real column)
    goes to -- the first entry of the aggregators' edge set attaining it, in edge order, the appended self loop last; E for that
    self loop, -1 for a row without entries."""
    L, Ls, _, _, _, _ = geometry(case)
    xb = real_columns(np.asarray(bases, dtype=np.float32), case.B, L, Ls)
    edges, raw = edge_sets(ei, n, case.sets, n_loop)[ALL_SETS[case.sets][0]]
    _, arg = orc.scatter(xb[edges[0]], edges[1], n, which)
    return np.where(arg >= edges.shape[1], -1, raw[np.minimum(arg, edges.shape[1] - 1)])


# ------------------------------------------------------------------------------------------------------------------------------
# the sweep graphs

EXTRA = (3, 4, 5, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1)                 # the load pipeline, the long-row threshold
RECORD_ROWS = (1, 2, 8, 9, CHUNK + 8, CHUNK + 9)                            # record overflow; the ballot limit, in a row and a chunk tail
LENGTHS = tuple(sorted(set(LADDER) | set(EXTRA) | set(RECORD_ROWS)))
# rows in CSR order: long rows first, last and adjacent; an empty row between non-empty ones
_LAYOUT = (3 * CHUNK, 2 * CHUNK + 1, CHUNK + 1, 3, 4, 5, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1, 0, 1, 2, 7, 8, 9, 15, 16, 17,
           CHUNK - 1, CHUNK, 2, 1, 0, CHUNK + 8, CHUNK + 9, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 18)
REDUCED_MAX = 2 * CHUNK + 1
assert sorted(set(_LAYOUT)) == list(LENGTHS)


def ladder_lengths(reduced=False):
    return [r for r in _LAYOUT if not reduced or r <= REDUCED_MAX]


@functools.lru_cache(maxsize=None)
def ladder(seed, flip=False, reduced=False):
    """(edge_index [2, E] int64, n, n): in-degrees = ladder_lengths in row order, out-degrees = the same lengths in reverse row
    order (long rows first, last and adjacent on either side; hub sources feed hub destinations: duplicate edges, self loops
    inside long rows), edge list shuffled.  ``flip``: transposed."""
    rng = np.random.default_rng(seed)
    lengths = np.array(ladder_lengths(reduced), dtype=np.int64)
    n = len(lengths)
    dst = np.repeat(np.arange(n, dtype=np.int64), lengths)
    src = np.repeat(np.arange(n, dtype=np.int64)[::-1], lengths)[rng.permutation(len(dst))]   # out-degree of row n - 1 - k = lengths[k]
    ei = np.ascontiguousarray(np.stack([src, dst])[:, rng.permutation(len(dst))])
    return (np.ascontiguousarray(ei[::-1]) if flip else ei), n, n


@functools.lru_cache(maxsize=None)
def rect(seed, more, flip=False):
    """The ladder on the destinations, sources drawn from n_src = 3 n / 2 (``more``) or n / 2 rows, every third of them fifty
    times less often than the others (short source rows next to hubs); ``flip`` swaps the sides.
    Raw edge sets only: a rectangular adjacency has no self loops and no symmetric normalisation."""
    rng = np.random.default_rng(seed)
    lengths = np.array(ladder_lengths(), dtype=np.int64)
    n = len(lengths)
    n_src = (3 * n) // 2 if more else n // 2
    dst = np.repeat(np.arange(n, dtype=np.int64), lengths)
    weight = np.where(np.arange(n_src) % 3 == 1, 0.02, 1.0)                    # every third source row stays short
    src = rng.choice(n_src, len(dst), p=weight / weight.sum()).astype(np.int64)
    ei = np.ascontiguousarray(np.stack([src, dst])[:, rng.permutation(len(dst))])
    return (np.ascontiguousarray(ei[::-1]), n_src, n) if flip else (ei, n, n_src)


SPARSE_LENGTHS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17) + (1, 0, 1) * 50


@functools.lru_cache(maxsize=None)
def sparse(seed, flip=False):
    """Square, many rows of at most 17 entries, 1.2 entries per row: 16 basis columns already are more than ten per entry."""
    rng = np.random.default_rng(seed)
    lengths = np.array(SPARSE_LENGTHS, dtype=np.int64)
    n = len(lengths)
    dst = np.repeat(np.arange(n, dtype=np.int64), lengths)
    src = rng.integers(0, n, len(dst)).astype(np.int64)
    src[::23] = dst[::23]                                                       # explicit self loops
    ei = np.ascontiguousarray(np.stack([src, dst])[:, rng.permutation(len(dst))])
    return (np.ascontiguousarray(ei[::-1]) if flip else ei), n, n


BOUNDARY_ROWS = 50


@functools.lru_cache(maxsize=None)
def boundary(seed, ldb, on):
    """Square, 50 rows, ldb * 50 / 10 entries (``on``: the last graph with records) or one fewer (the first without)."""
    assert (ldb * BOUNDARY_ROWS) % REC_FIT_COLUMNS == 0
    rng = np.random.default_rng(seed)
    n, e = BOUNDARY_ROWS, ldb * BOUNDARY_ROWS // REC_FIT_COLUMNS - (0 if on else 1)
    lengths = np.full(n, e // n, dtype=np.int64)
    lengths[:e % n] += 1
    dst = np.repeat(np.arange(n, dtype=np.int64), lengths)
    src = rng.integers(0, n, e).astype(np.int64)
    return np.ascontiguousarray(np.stack([src, dst])[:, rng.permutation(e)]), n, n


def degrees(ei, n, n_src):
    return np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n_src)


def make_inputs(case, n, n_src, seed, ties=False):
    """(bases [n_src, ldb], weightings [n, W], grad_out [n, H L]) float32; the padding columns of ``bases`` are zero, as the GEMM
    that produces them leaves them.  ``ties``: the real columns hold the integers -2 .. 2, so that nearly every extremum is
    attained by several entries, in several chunks of a long row, and by the row's own features.  With std / var the normals
    are rounded to eighths: a row's variance is then exactly zero or at least 2^-8, where 1 / (2 std) amplifies the rounding of
    the variance itself by no more than 8 -- a variance of 1e-4 between two nearly equal normals (one in a few thousand columns)
    put the float32 restatement itself 3e-4 from float64, beyond what any float32 evaluation can be held to."""
    L, Ls, ldb, _, _, W = geometry(case)
    rng = np.random.default_rng(seed)
    real = rng.integers(-2, 3, (n_src, case.B, L)).astype(np.float32) if ties else \
        rng.standard_normal((n_src, case.B, L)).astype(np.float32)
    if stdvar(case) and not ties:
        real = np.round(real * 8) / 8
    bases = np.zeros((n_src, ldb), dtype=np.float32)
    bases[:, :case.B * Ls].reshape(n_src, case.B, Ls)[:, :, :L] = real
    return bases, rng.standard_normal((n, W)).astype(np.float32), rng.standard_normal((n, case.out)).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch rule of egc_aggregate_combine_backward_f32, as data

REC_ITEMS, REC_FIT_COLUMNS, REC_BALLOT_MAX, BWD_HMAX, BWD_FU = 12, 10, 8, 16, 4
OOB = 0x80000000
# the aggregator lists compiled into bwd_dst_fast_kernel, by (LPR_LOG2, HT, AT)
COMPILED_DST = {
    (6, 4, 3): (("sum", "mean", "max"), ("symnorm", "max", "mean")),
    (6, 8, 1): (("symnorm",),),
    (5, 8, 1): (("symnorm",),),
    (5, 4, 3): (("sum", "std", "max"), ("symnorm", "std", "max")),
    (4, 8, 4): (("sum", "mean", "max", "symnorm"),),
    (4, 8, 3): (("symnorm", "max", "mean"),),
    (4, 8, 1): (("symnorm",),),
}
# the flag words compiled into bwd_src_kernel<1, ...>: tables T S V X N, LOOPED sets of the aggregators (XL) and of symnorm (YL), records
COMPILED_SRC = frozenset(frozenset(f.split()) for f in (
    "T X YL", "T S X YL", "T V X YL", "T S V X YL", "T S X XL YL",
    "T S X XL YL REC", "T S X YL REC", "S YL", "S XL YL", "T X REC", "T V X YL REC", "T S V X YL REC", "T X YL REC"))


class Cell(NamedTuple):
    dst: str            # "fast<LPR_LOG2,HT,AT>" / "fast<LPR_LOG2,HT,AT,list>" / "lds/wavefronts per block"
    basis: str          # fast: how the d w' shares of a basis meet -- "p2:H%P" / "p2:H<P" (butterfly) / "np2" (through LDS); else ""
    src: str            # "src<ns>" (run-time flags) / "src<1,flags>"
    lpr_log2: int       # lane group of the source kernel
    rec: str            # "off" / "fused" / "sep<NS>"


def records_apply(case, n, e, env=()):
    _, _, ldb, _, _, _ = geometry(case)
    return (extrema(case) > 0 and e > 0 and ldb <= 256 and e * 64 < OOB and "EGC_BWD_NO_REC" not in env
            and ldb * max(n, 1) <= REC_FIT_COLUMNS * e)


def dispatch(case, n, e, env=()):
    """The kernels one backward call launches on a graph of ``n`` destination rows and ``e`` entries with the record-sized
    workspace, under the environment switches ``env`` (EGC_BWD_NO_REC, EGC_BWD_REC_SEPARATE, EGC_BWD_GENERIC)."""
    L, Ls, ldb, slots, A, W = geometry(case)
    H, B, aggrs = case.H, case.B, tuple(case.aggrs)
    generic = "EGC_BWD_GENERIC" in env
    rec = records_apply(case, n, e, env)
    lds_floats = A * ldb + ((case.out + 3) & ~3) + 2 * ((W + 3) & ~3)
    wpb = 4 if 4 * lds_floats * 4 <= 48 * 1024 else 1
    assert wpb * lds_floats * 4 <= 64 * 1024, "unsupported"
    P = Ls // 4
    p2 = P & (P - 1) == 0
    by_shape = ((slots <= 16 and H == 8 and A in (1, 3, 4)) or
                (slots > 16 and ((H == 4 and A == 3) or (H == 8 and A == 1))))
    fast = (not generic and Ls % 4 == 0 and ldb == B * Ls and 1 <= P <= 16 and B & (B - 1) == 0 and slots <= 64 and A <= 4
            and H <= BWD_HMAX and (not p2 or H % P == 0 or H < P) and case.act != "softmax" and by_shape)
    if fast:
        lg = 4 if slots <= 16 else 5 if slots <= 32 else 6
        key = (lg, 8, A) if lg == 4 else (lg, H, A)
        compiled = case.act == "none" and aggrs in COMPILED_DST.get(key, ())
        dst = f"fast<{key[0]},{key[1]},{key[2]}" + (f",{'+'.join(aggrs)}>" if compiled else ">")
        basis = "np2" if not p2 else "p2:H%P" if H % P == 0 else "p2:H<P"
    else:
        dst, basis = f"lds/{wpb}", ""
    rec_mode = "off" if not rec else "fused" if fast and "EGC_BWD_REC_SEPARATE" not in env else f"sep<{min((slots + 15) // 16, 4)}>"
    lg = 4
    while (1 << lg) < slots and lg < 6:
        lg += 1
    ns = (slots + (1 << lg) - 1) >> lg
    assert ns <= 4, "unsupported"
    agg_looped, sym_looped = (s == _C.SET_LOOPED for s in SETS[case.sets])
    flags = {f for f, on in (("T", bool({"sum", "mean", "var", "std"} & set(aggrs))), ("S", "symnorm" in aggrs), ("V", stdvar(case)),
                             ("X", "max" in aggrs), ("N", "min" in aggrs), ("XL", agg_looped), ("YL", sym_looped), ("REC", rec)) if on}
    if not generic and ns == 1 and frozenset(flags) in COMPILED_SRC:
        src = "src<1," + "|".join(f for f in ("T", "S", "V", "X", "N", "XL", "YL", "REC") if f in flags) + ">"
    else:
        src = f"src<{ns}>"
    return Cell(dst, basis, src, lg, rec_mode)


def arg_extrema_instance(case):
    """NS of arg_extrema_kernel<NS>, the separate arg pass of the training forward (generic kernels), or None without max / min."""
    if not extrema(case):
        return None
    slots = geometry(case)[3]
    lg = 4
    while (1 << lg) < slots and lg < 6:
        lg += 1
    return (slots + (1 << lg) - 1) >> lg


_NAMES = {"EGC_AGGR_" + k.upper(): k for k in CODES}
_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "egc_amd", "csrc")
KERNELS = ("bwd_dst_fast_kernel", "bwd_src_kernel", "bwd_records_kernel", "arg_extrema_kernel")


def source_text(name="egc_backward.hip"):
    with open(os.path.join(_CSRC, name)) as f:
        return f.read()


def list_rows(lists, macro):
    """The argument text of every ROW(...) of the list ``macro`` of egc_backward_host.h (a #define continued by backslashes)."""
    body = re.search(r"#define %s\(ROW\)((?:.*\\\n)*.*)" % macro, lists).group(1)
    return [m.group(1) for m in re.finditer(r"ROW\(([^()]*)\)", body)]


def source_instances(lists=None, source=None):
    """The template instances egc_backward.hip launches, in the notation of ``Cell`` -- read from the rows of the lists of
    egc_backward_host.h, which the launches (one per kernel template in egc_backward.hip: asserted here) expand from."""
    lists = source_text("egc_backward_host.h") if lists is None else lists
    source = source_text() if source is None else source
    for k in KERNELS:
        assert len(re.findall(k + r"<[^;{}]*?><<<", source)) == 1, k
    got = dict(dst=set(), src=set(), rec=set(), arg=set())
    for row in list_rows(lists, "EGC_BWD_DST_LISTS"):
        parts = [p.strip() for p in row.split(",")]
        got["dst"].add(f"fast<{parts[0]},{parts[1]},{parts[2]}," + "+".join(_NAMES[a] for a in parts[3:]) + ">")
    for row in list_rows(lists, "EGC_BWD_DST_TRIPLES"):
        got["dst"].add("fast<" + ",".join(p.strip() for p in row.split(",")) + ">")
    for row in list_rows(lists, "EGC_BWD_SRC_FLAGS"):
        fl = [f.strip()[len("SRC_"):] for f in row.split("|")]
        got["src"].add("src<1," + "|".join(f for f in ("T", "S", "V", "X", "N", "XL", "YL", "REC") if f in fl) + ">")
    for ns in list_rows(lists, "EGC_BWD_NS"):
        got["src"].add(f"src<{ns}>")
        got["rec"].add(f"sep<{ns}>")
        got["arg"].add(int(ns))
    return got


# ------------------------------------------------------------------------------------------------------------------------------
# the table

NORTH, EGCM, EGCS = ("sum", "mean", "max", "symnorm"), ("symnorm", "max", "mean"), ("symnorm",)
ALL7 = ("sum", "mean", "max", "min", "var", "std", "symnorm")
CASES = (
    # ---- register form, 16 lanes a row: the aggregator list compiled in
    Case(64, 8, 4, NORTH, "looped", "fast<4,8,4,sum+mean+max+symnorm>"),
    Case(64, 8, 4, EGCM, "lay", "fast<4,8,3,symnorm+max+mean>"),
    Case(64, 8, 4, EGCS, "lay", "fast<4,8,1,symnorm>"),
    Case(64, 8, 4, EGCS, "looped", "fast<4,8,1,symnorm>"),
    # ---- 16 lanes, run-time list
    Case(64, 8, 4, ("min", "std", "var"), "looped", "fast<4,8,3>"),
    Case(64, 8, 4, ("sum", "mean", "max", "min"), "raw", "fast<4,8,4>"),
    Case(64, 8, 4, ("mean",), "lay", "fast<4,8,1>"),
    Case(64, 8, 4, ("sum", "mean", "max"), "raw", "fast<4,8,3>"),                    # the relational layer's flag word
    # ---- 16 lanes, the other geometries
    Case(96, 8, 4, ("sum", "max", "min"), "looped", "fast<4,8,3>"),                  # P = 3: not a power of two, 12 of 16 lanes
    Case(32, 8, 4, ("symnorm", "max", "mean"), "lay", "fast<4,8,3,symnorm+max+mean>"),   # P = 1, 4 of 16 lanes
    Case(128, 8, 1, NORTH, "looped", "fast<4,8,4,sum+mean+max+symnorm>"),            # B = 1, 4 of 16 lanes
    Case(512, 8, 1, ("max", "var", "mean"), "raw", "fast<4,8,3>"),                   # P = 16 > H
    # ---- 32 lanes
    Case(124, 4, 4, ("sum", "std", "max"), "lay", "fast<5,4,3,sum+std+max>"),        # zinc EGC-M, L = 31 padded to 32
    Case(128, 4, 4, ("symnorm", "std", "max"), "lay", "fast<5,4,3,symnorm+std+max>"),    # CIFAR EGC-M
    Case(128, 4, 4, ("mean", "max", "min"), "raw", "fast<5,4,3>"),
    Case(168, 8, 4, EGCS, "lay", "fast<5,8,1,symnorm>"),                             # zinc / CIFAR EGC-S, P = 6, 24 of 32 lanes
    Case(168, 8, 4, ("max",), "lay", "fast<5,8,1>"),
    Case(256, 8, 4, ("min",), "raw", "fast<5,8,1>"),
    Case(64, 8, 16, ("mean",), "looped", "fast<5,8,1>"),                             # B = 16
    # ---- 64 lanes
    Case(136, 4, 4, EGCM, "lay", "fast<6,4,3,symnorm+max+mean>"),                    # arxiv EGC-M, P = 9, 36 of 64 lanes
    Case(224, 4, 4, ("sum", "mean", "max"), "lay", "fast<6,4,3,sum+mean+max>"),      # molhiv EGC-M, P = 14
    Case(224, 4, 4, ("max", "min", "var"), "raw", "fast<6,4,3>"),
    Case(296, 8, 4, EGCS, "lay", "fast<6,8,1,symnorm>"),                             # molhiv EGC-S, P = 10
    Case(296, 8, 4, ("mean",), "lay", "fast<6,8,1>"),
    Case(512, 8, 4, EGCS, "lay", "fast<6,8,1,symnorm>"),                             # P = 16 > H, every lane
    Case(256, 4, 4, ("sum", "max", "mean"), "looped", "fast<6,4,3>"),
    Case(64, 4, 16, ("sum", "min", "mean"), "lay", "fast<6,4,3>"),                    # P = 4 divides H, B = 16, every lane
    # ---- weight nonlinearities on the register form (run-time list) ...
    Case(64, 8, 4, NORTH, "looped", "fast<4,8,4>", act="sigmoid"),
    Case(64, 8, 4, EGCM, "lay", "fast<4,8,3>", act="hardtanh"),
    Case(96, 8, 4, ("sum", "max", "min"), "looped", "fast<4,8,3>", act="sigmoid"),   # ... behind the transposed shares
    Case(224, 4, 4, ("sum", "mean", "max"), "lay", "fast<6,4,3>", act="hardtanh"),
    # ---- LDS form, four wavefronts a block
    Case(42, 6, 3, ("max", "min", "mean"), "looped", "lds/4"),                       # L = 7 padded to 8
    Case(42, 6, 3, ("symnorm", "min", "var"), "lay", "lds/4", act="softmax"),
    Case(42, 6, 3, ("sum", "std", "max"), "raw", "lds/4", act="sigmoid"),
    Case(42, 6, 3, ("mean",), "lay", "lds/4", act="hardtanh"),
    Case(88, 2, 2, ("symnorm", "max"), "lay", "lds/4"),                              # 22 slots
    Case(256, 4, 4, ("max",), "raw", "lds/4"),                                       # 64 slots, H = 4 with one aggregator
    Case(64, 8, 4, ("sum", "mean", "max", "min", "symnorm"), "looped", "lds/4"),     # five aggregators
    Case(64, 8, 4, NORTH, "looped", "lds/4", act="softmax"),                         # a register shape under softmax
    Case(224, 4, 4, ("sum", "mean", "max"), "lay", "lds/4", act="softmax"),
    # ---- LDS form, two to four slots a lane in the source kernel and the arg pass
    Case(320, 4, 4, ("sum", "max", "min"), "looped", "lds/4", graph="reduced"),      # 80 slots
    Case(384, 4, 8, ("symnorm", "max", "std"), "lay", "lds/4", graph="reduced"),     # 192 slots
    Case(512, 4, 8, ("mean", "min"), "raw", "lds/4", graph="reduced"),               # 256 slots
    # ---- LDS form, one wavefront a block
    Case(1024, 8, 8, ALL7, "looped", "lds/1", graph="reduced"),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RECORD_CASES = tuple(c for c in CASES if extrema(c) and geometry(c)[2] <= 256)      # cells that can build records
RECT_CASES = tuple(c for c in CASES if c.sets == "raw" and "symnorm" not in c.aggrs and c.graph == "ladder")
BOUNDARY_CASES = (BY_NAME["64-H8-B4-sum+mean+max+symnorm-looped"], BY_NAME["42-H6-B3-max+min+mean-looped"])
GRAPH_SEED, INPUT_SEED = 31, 32


def case_graph(case, flip=False):
    return ladder(GRAPH_SEED, flip, case.graph == "reduced")
