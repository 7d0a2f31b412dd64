"""The sweep of the full-graph inference aggregate + combine (egc_amd/csrc/egc_aggregate.hip, egc_aggregate_fast.hip,
egc_aggregate_fast_dev.h) at every form it dispatches on: what tests/test_forward_shapes_cpu.py checks without a device and
tests/test_forward_shapes_gpu.py runs on one.  The pattern is that of tests/backward_ref.py, whose restatement, graphs and inputs
are used here, not copied.

Four parts.

``forward`` restates one inference call at the OPERAND level -- bases, pre-activation weightings (either column layout), bias and
the fused post-op ``out = relu((z + bias) * scale + shift) + residual`` of egc_post -- on ``backward_ref.aggregate_combine``, in
torch on the CPU; in float64 it is the truth, in float32 the yardstick of what one float32 evaluation is worth.  ``n_loop`` is the
rule of a layer without ``loops_all_nodes`` (EGConv with self loops, no symnorm: add_remaining_self_loops infers the node count
from the edge list): a LOOPED set appends self loops to rows <= the largest index only.

The graphs are the ladder of backward_ref and its variants, plus ``tail`` (the ladder and five rows that appear in no edge: without
``loops_all`` they get no self loop, their output is the epilogue of an empty row), ``edgeless`` and ``big`` (exactly 32768 rows, the
ladder first, one or two entries in every other row: the four-row-groups-per-wavefront form of launch_fast).

``dispatch`` restates, as data, which kernel family and instance one call launches: fast_path_supported / try_static /
agg_dispatch<NeedFine> of the register kernel, wide_path_supported / try_wide_static / agg_dispatch_rows<NeedCoarse> of the
two-slots-per-lane kernel, launch_all<1..4> with the wavefronts-per-block rule and the lane group of the LDS kernels, rows_per_wave,
under the switches EGC_FORCE_GENERIC, EGC_NO_STATIC_CFG and EGC_NO_WIDE.  ``static_rows`` reads the compiled-in configurations out
of egc_aggregate_fast.hip, so that a row added there without a case here is noticed.

``CASES`` is the table: every cell of the rule at the smallest shape that reaches it.

``plan_form`` / ``plan_instances`` add the gather plan of a static graph to the rule: which calls take agg_fast_kernel's PLAN form
on a trimmed graph, and which PLAN kernels the library compiles (tests/test_forward_plan_cpu.py, tests/test_forward_plan_gpu.py)."""
import functools
import re
from typing import NamedTuple

import numpy as np
import torch

import backward_ref
from backward_ref import (ACTS, ALL7, ALL_SETS, CODES, GRAPH_SEED, INPUT_SEED, THRESHOLD, aggregate_combine,  # noqa: F401
                          extrema, geometry, ladder, make_inputs, rect, source_text, sparse, stdvar)
from egc_amd import _C

SETS = ALL_SETS                       # raw / looped / lay, and xl = (LOOPED, RAW): refused by the register kernels, legal in the C ABI
LAYOUTS = {"HBA": _C.LAYOUT_HBA, "HAB": _C.LAYOUT_HAB}
AMAX, HPB_MAX = 4, 4                  # egc_plain.h, egc_aggregate_fast_dev.h
RPW_ROWS = 32768                      # launch_fast: one-row groups on at least this many rows take four row groups per wavefront


class Case(NamedTuple):
    """One layer of the table.  ``cell``: the kernel instance a plain call on the case's graph must launch without switches."""
    out: int
    H: int
    B: int
    aggrs: tuple
    sets: str
    cell: str
    act: str = "none"
    graph: str = "ladder"        # "reduced" (longest row 513) where the CPU reference would take seconds on the full ladder
    loops_all: bool = True       # False: LOOPED sets loop rows <= the largest index only; such a case runs on the ``tail`` graph
    layout: str = "HBA"
    bias: bool = True
    ldw: int = 0                 # > 0: the weightings are a column block of an array of that width
    stride: int = 0              # > 0: the basis stride itself (an unpadded basis); 0: the stride the layers choose

    @property
    def name(self):
        return (f"{self.out}-H{self.H}-B{self.B}-{'+'.join(self.aggrs)}-{self.sets}"
                + (f"-{self.act}" if self.act != "none" else "") + ("" if self.loops_all else "-noloopsall")
                + ("-HAB" if self.layout == "HAB" else "") + ("" if self.bias else "-nobias") + (f"-ldw{self.ldw}" if self.ldw else "")
                + (f"-stride{self.stride}" if self.stride else ""))


def need_of(case):
    return "|".join(f for f, on in (("SQ", stdvar(case)), ("MN", "min" in case.aggrs)) if on) or "0"


# ------------------------------------------------------------------------------------------------------------------------------
# the operand-level restatement

class Post(NamedTuple):
    """egc_post: every part optional."""
    scale: object = None
    shift: object = None
    residual: object = None
    relu: bool = False


def post_op(z, bias, post):
    """relu((z + bias) * scale + shift) + residual in the dtype of ``z`` (torch); ``bias`` and ``post`` may be None."""
    if bias is not None:
        z = z + bias
    if post is None:
        return z
    if post.scale is not None:
        z = z * post.scale + post.shift
    if post.relu:
        z = torch.relu(z)
    if post.residual is not None:
        z = z + post.residual
    return z


def hba_columns(weightings, case):
    """The weightings in the column order [h][b][a] the restatement reads (HAB: column (h A + a) B + b)."""
    if case.layout == "HBA":
        return weightings
    n, A = weightings.shape[0], len(case.aggrs)
    return weightings.view(n, case.H, A, case.B).transpose(2, 3).reshape(n, -1)


def forward(bases, weightings, ei, n, case, bias=None, post=None, n_loop=None):
    """out [n, H L] of one inference call; torch tensors of one dtype on the CPU."""
    return post_op(aggregate_combine(bases, hba_columns(weightings, case), ei, n, case, n_loop), bias, post)


def n_loop_of(case, ei, n):
    ei = np.asarray(ei)
    return n if case.loops_all else (int(ei.max()) + 1 if ei.size else 0)


VARIANTS = {"plain": (), "full": ("affine", "relu", "residual"), "affine": ("affine",), "relu": ("relu",), "residual": ("residual",)}


def make_post(case, n, seed):
    """dict(bias [F], scale [F], shift [F], residual [n, F]) float32: the scale from +-[0.5, 2] with both signs, so that relu
    cuts on either side of the affine map; the others standard normals."""
    rng = np.random.default_rng(seed)
    f = case.out
    sign = np.where(np.arange(f) % 2 == 0, 1.0, -1.0)[rng.permutation(f)] if f > 1 else np.ones(1)
    return dict(bias=rng.standard_normal(f).astype(np.float32), scale=(sign * rng.uniform(0.5, 2.0, f)).astype(np.float32),
                shift=rng.standard_normal(f).astype(np.float32), residual=rng.standard_normal((n, f)).astype(np.float32))


def post_of(operands, variant, dtype):
    """(bias, Post) as torch tensors of ``dtype`` for a variant of VARIANTS; ``operands`` from make_post, its bias None without one."""
    t = lambda a: None if a is None else torch.from_numpy(a).to(dtype)       # noqa: E731
    parts = VARIANTS[variant]
    post = None
    if parts:
        post = Post(t(operands["scale"]) if "affine" in parts else None, t(operands["shift"]) if "affine" in parts else None,
                    t(operands["residual"]) if "residual" in parts else None, "relu" in parts)
    return t(operands["bias"]), post


# ------------------------------------------------------------------------------------------------------------------------------
# the graphs

TAIL_ROWS = 5


@functools.lru_cache(maxsize=None)
def tail(seed, flip=False, reduced=False):
    """The ladder and TAIL_ROWS further rows that appear in no edge."""
    ei, n, _ = ladder(seed, flip, reduced)
    return ei, n + TAIL_ROWS, n + TAIL_ROWS


def edgeless(n=9):
    return np.zeros((2, 0), dtype=np.int64), n, n


@functools.lru_cache(maxsize=None)
def big(seed):
    """Exactly RPW_ROWS rows: the ladder first, every other row one or two entries from anywhere in the graph."""
    rng = np.random.default_rng(seed)
    ei, n0, _ = ladder(seed)
    n = RPW_ROWS
    lengths = rng.integers(1, 3, n - n0)
    dst = np.repeat(np.arange(n0, n, dtype=np.int64), lengths)
    src = rng.integers(0, n, len(dst)).astype(np.int64)
    more = np.stack([src, dst])
    both = np.concatenate([ei, more], axis=1)
    return np.ascontiguousarray(both[:, rng.permutation(both.shape[1])]), n, n


def edges(kind, flip=False, reduced=False):
    """(edge_index, n, n_src) of a graph key: ("ladder",) / ("tail",) / ("rect", more) / ("sparse",) / ("edgeless",) / ("big",)."""
    if kind[0] == "ladder":
        return ladder(GRAPH_SEED, flip, reduced)
    if kind[0] == "tail":
        return tail(GRAPH_SEED, flip, reduced)
    if kind[0] == "rect":
        return rect(GRAPH_SEED, kind[1], flip)
    if kind[0] == "sparse":
        return sparse(GRAPH_SEED, flip)
    if kind[0] == "edgeless":
        return edgeless()
    assert kind[0] == "big" and not flip
    return big(GRAPH_SEED)


def home(case):
    """The graph key of a case's own sweep: the ladder, with the isolated tail where ``loops_all`` is off."""
    return ("ladder",) if case.loops_all else ("tail",)


def graph_key(case, kind, flip):
    return kind, flip, kind[0] in ("ladder", "tail") and case.graph == "reduced"


# ------------------------------------------------------------------------------------------------------------------------------
# the compiled-in configurations of egc_aggregate_fast.hip

class StaticRow(NamedTuple):
    kind: str           # "reg" (EGC_STATIC_CFG of launch_fast) / "wide" (try_wide_static of launch_wide_rows)
    H: int
    B: int
    L: int
    Ls: int
    aggrs: tuple
    act: str
    xl: bool
    yl: bool
    loops_all: bool
    need: str

    @property
    def name(self):
        sets = {(False, False): "raw", (True, True): "looped", (False, True): "lay", (True, False): "xl"}[(self.xl, self.yl)]
        return (f"{'wide:' if self.kind == 'wide' else ''}st<{self.H},{self.B},{self.L},{'+'.join(self.aggrs)},{self.act},{sets}"
                + ("" if self.loops_all else ",noloopsall") + ">")


_ROW = r"(\d+), (\d+), (\d+), (\d+), agg_pack\(([^()]*)\), EGC_ACT_(\w+), (true|false), (true|false), (true|false), "
_NEEDS = {"0": "0", "NEED_SQ": "SQ", "NEED_MN": "MN", "NEED_SQ | NEED_MN": "SQ|MN"}


def static_rows(source=None):
    """Every EGC_STATIC_CFG(...) row of launch_fast and every try_wide_static<StCfg<...>> row of launch_wide_rows, in order."""
    source = source_text("egc_aggregate_fast.hip") if source is None else source
    letters = {m.group(1): m.group(2).lower() for m in re.finditer(r"\b([A-Z]) = EGC_AGGR_([A-Z]+)", source)}

    def aggrs(text):
        names = tuple(letters[t] if t in letters else t[len("EGC_AGGR_"):].lower() for t in (s.strip() for s in text.split(",")))
        assert all(a in CODES for a in names), text
        return names
    rows = []
    for m in re.finditer(r"^\s*EGC_STATIC_CFG\(" + _ROW + r"([^()]*)\)", source, re.M):
        H, B, L, A = (int(m.group(k)) for k in (1, 2, 3, 4))
        rows.append(StaticRow("reg", H, B, L, (L + 3) // 4 * 4, aggrs(m.group(5)), m.group(6).lower(), m.group(7) == "true",
                              m.group(8) == "true", m.group(9) == "true", _NEEDS[m.group(10).strip()]))
        assert len(rows[-1].aggrs) == A, m.group(0)
    n_reg = len(rows)
    assert n_reg == len(re.findall(r"EGC_STATIC_CFG\(", source)) - 1          # every use but the #define itself was understood
    for m in re.finditer(r"try_wide_static<StCfg<" + _ROW + r"(\d+)>, (\d+), ([^,]*), (\d+), (\d+)>\(", source):
        H, B, L, A = (int(m.group(k)) for k in (1, 2, 3, 4))
        rows.append(StaticRow("wide", H, B, L, int(m.group(10)), aggrs(m.group(5)), m.group(6).lower(), m.group(7) == "true",
                              m.group(8) == "true", m.group(9) == "true", _NEEDS[m.group(12).strip()]))
        assert len(rows[-1].aggrs) == A and int(m.group(13)) + int(m.group(14)) == rows[-1].Ls // 4, m.group(0)
    assert len(rows) - n_reg == len(re.findall(r"try_wide_static<", source))   # (the template's definition names no arguments)
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def _rows_of_the_source():
    return static_rows()


# ------------------------------------------------------------------------------------------------------------------------------
# the dispatch rule of an inference call, as data

class Cell(NamedTuple):
    family: str         # "reg" (agg_fast_kernel) / "wide" (agg_wide_kernel) / "lds" (agg_chunks / agg_rows / agg_merge kernels)
    instance: str       # reg: "st<...>" / "rt<LPR_LOG2,HPB,NEED>"; wide: "wide:st<...>" / "wide<HPB,NEED>"; lds: "lds<CHUNKS>/wavefronts per block"
    reason: str         # lds: why the register kernels do not run ("" for the others)
    rows_per_wave: int  # row groups per wavefront (reg: 1 / 4, wide: 8, lds: 0 -- one row per wavefront)
    store: str          # reg / wide: "contig" (L a multiple of 4) / "padded" (ragged head tails); lds: ""
    basis: str          # reg: how the sum over bases runs -- "dpp" (16 slots, four lanes per basis) / "p2" / "np2"; wide: "odd" / "even" (P); lds: ""
    lpr_log2: int       # lane group of a row: reg 4 .. 6, wide 6, lds 0 .. 6


def agg_lpr(slots):
    return 16 if slots <= 16 else 32 if slots <= 32 else 64


def _hpb(case):
    hpb = -(-case.H // case.B)
    return hpb, (1 if hpb <= 1 else 2 if hpb <= 2 else 4)


def fast_refusal(case):
    """The first condition of fast_path_supported a layer fails ("" if none)."""
    L, Ls, ldb, slots, A, W = geometry(case)
    xl, yl = (s == _C.SET_LOOPED for s in SETS[case.sets])
    for reason, hit in (("slots>64", slots > 64), ("HAB", case.layout != "HBA"), ("softmax", case.act == "softmax"),
                        ("xl", xl and not yl), ("unpadded", Ls % 4 != 0 or ldb != case.B * Ls), ("B", case.B & (case.B - 1) != 0),
                        ("A>4", A > AMAX), ("hpb>4", _hpb(case)[0] > HPB_MAX), ("W", W > 8 * agg_lpr(slots))):
        if hit:
            return reason
    return ""


def wide_refusal(case, post):
    """The first condition of wide_path_supported an inference call fails ("" if none)."""
    L, Ls, ldb, slots, A, W = geometry(case)
    xl, yl = (s == _C.SET_LOOPED for s in SETS[case.sets])
    strips = (2 if post else 1) * ((case.H * Ls + 3) & ~3) + ((W + 3) & ~3)
    for reason, hit in (("HAB", case.layout != "HBA"), ("softmax", case.act == "softmax"), ("xl", xl and not yl),
                        ("slots>128", slots <= 64 or slots > 128), ("unpadded", Ls % 4 != 0 or ldb != case.B * Ls),
                        ("B", case.B & (case.B - 1) != 0), ("A>4", A > AMAX), ("hpb>4", _hpb(case)[0] > HPB_MAX), ("W", W > 512),
                        ("B*P0>64", case.B * ((Ls // 4 + 1) // 2) > 64), ("lds", 4 * strips * 4 > 64 * 1024)):
        if hit:
            return reason
    return ""


def static_match(case, kind):
    """The compiled-in configuration of ``kind`` a layer equals (cfg_matches, and try_static's lane-group condition), or None."""
    L, Ls, ldb, slots, A, W = geometry(case)
    xl, yl = (s == _C.SET_LOOPED for s in SETS[case.sets])
    for r in _rows_of_the_source():
        if r.kind == kind and (case.H, case.B, L, Ls, tuple(case.aggrs), case.act, xl, yl, case.loops_all) == \
                (r.H, r.B, r.L, r.Ls, r.aggrs, r.act, r.xl, r.yl, r.loops_all):
            lpr = agg_lpr(r.B * r.Ls // 4)
            if kind == "wide" or lpr // 2 < slots <= lpr:
                assert need_of(case) == r.need or kind == "wide", (case.name, r)
                return r
    return None


def dispatch(case, n, post=False, env=()):
    """The kernels one inference call over ``n`` rows (the row range) launches, with or without a fused post-op, under the
    environment switches ``env`` (EGC_FORCE_GENERIC, EGC_NO_STATIC_CFG, EGC_NO_WIDE)."""
    L, Ls, ldb, slots, A, W = geometry(case)
    generic = "EGC_FORCE_GENERIC" in env
    static = "EGC_NO_STATIC_CFG" not in env
    chunks = 1 if slots <= 64 else (slots + 63) // 64
    P = Ls // 4
    store = "contig" if L % 4 == 0 else "padded"
    why = fast_refusal(case)
    if not generic and not why:
        lpr = agg_lpr(slots)
        lg = {16: 4, 32: 5, 64: 6}[lpr]
        rpw = 4 if lpr == 64 and n >= RPW_ROWS else 1
        basis = "dpp" if (P == 4 and slots == 16) else "p2" if P & (P - 1) == 0 else "np2"
        row = static_match(case, "reg") if static else None
        inst = row.name if row is not None else f"rt<{lg},{_hpb(case)[1]},{need_of(case)}>"
        return Cell("reg", inst, "", rpw, store, basis, lg)
    assert 1 <= chunks <= 4, "unsupported"
    if chunks == 2 and not generic and "EGC_NO_WIDE" not in env and not wide_refusal(case, post):
        row = static_match(case, "wide") if static else None
        inst = row.name if row is not None else f"wide<{_hpb(case)[1]},{'0' if need_of(case) == '0' else 'SQ|MN'}>"
        return Cell("wide", inst, "", 8, store, "odd" if P % 2 else "even", 6)
    lds_floats = A * ldb + ((W + 3) & ~3)
    wpb = 4 if 4 * lds_floats * 4 <= 40 * 1024 else 1
    assert wpb * lds_floats * 4 <= 64 * 1024, "unsupported"
    lg = 6
    if slots <= 64:
        lg = 0
        while (1 << lg) < slots:
            lg += 1
    if generic:
        why = "forced"
    elif chunks == 2:
        why = "no_wide" if "EGC_NO_WIDE" in env and not wide_refusal(case, post) else wide_refusal(case, post)
    elif chunks > 2:
        why = "slots>128"
    return Cell("lds", f"lds<{chunks}>/{wpb}", why, 0, "", "", lg)


SWITCHES = ((), ("EGC_NO_STATIC_CFG",), ("EGC_NO_WIDE",), ("EGC_FORCE_GENERIC",))


def forms(case, n):
    """The switch sets under which a case launches something else than without switches, the empty set first."""
    got, seen = [], set()
    for env in SWITCHES:
        cell = dispatch(case, n, False, env)
        if cell not in seen:
            got.append(env)
            seen.add(cell)
    return tuple(got)


# ------------------------------------------------------------------------------------------------------------------------------
# the table

NORTH, EGCM, EGCS = backward_ref.NORTH, backward_ref.EGCM, backward_ref.EGCS


def _st(H, B, L, aggrs, sets, **kw):
    """A compiled-in configuration of launch_fast at its own shape."""
    return Case(H * L, H, B, aggrs, sets, f"st<{H},{B},{L},{'+'.join(aggrs)},none,{sets}>", **kw)


# the RtCfg ladder of agg_fast_kernel: one shape per (lane group, heads per lane), one aggregator list per need mask
_RT_SHAPES = {
    (4, 1): (64, 4, 4),      # L = 16, P = 4: 16 slots, four lanes per basis (DPP)
    (4, 2): (96, 8, 4),      # L = 12, P = 3: rotation butterfly, magic division, 12 of 16 lanes
    (4, 4): (88, 8, 2),      # L = 11 padded to 12: ragged head tails, 6 of 16 lanes
    (5, 1): (124, 4, 4),     # L = 31 padded to 32, P = 8, every lane
    (5, 2): (192, 8, 4),     # L = 24, P = 6, 24 of 32 lanes
    (5, 4): (296, 8, 2),     # L = 37 padded to 40, P = 10, 20 of 32 lanes
    (6, 1): (144, 4, 4),     # L = 36, P = 9, 36 of 64 lanes
    (6, 2): (512, 8, 4),     # L = 64, P = 16, every lane
    (6, 4): (600, 8, 2),     # L = 75 padded to 76, P = 19, 38 of 64 lanes
}
_RT_LISTS = {"0": ("max", "symnorm", "sum"), "SQ": ("mean", "std"), "MN": ("min",), "SQ|MN": ("var", "min", "sum", "max")}


def _rt_ladder():
    cases = []
    for k, ((lg, hpb), (out, H, B)) in enumerate(_RT_SHAPES.items()):
        for j, (need, aggrs) in enumerate(_RT_LISTS.items()):
            i = 4 * k + j
            cases.append(Case(out, H, B, aggrs, ("raw", "looped", "lay")[i % 3], f"rt<{lg},{hpb},{need}>",
                              act=("none", "none", "sigmoid", "none", "hardtanh")[i % 5], bias=i % 4 != 3,
                              graph="reduced" if out > 256 else "ladder"))
    return tuple(cases)


CASES = (
    # ---- register kernel: every compiled-in configuration of launch_fast, in the order of the source
    _st(8, 4, 16, NORTH, "looped"),                                     # W = 128 = 8 * 16 exactly
    _st(8, 4, 16, ("sum", "max", "symnorm"), "looped"),
    _st(8, 4, 16, ("sum", "std", "max", "symnorm"), "looped"),
    _st(8, 4, 16, EGCS, "looped"),
    _st(8, 4, 16, EGCM, "lay"),
    _st(8, 4, 16, EGCS, "lay", bias=False),
    _st(8, 4, 23, EGCS, "lay"),                                         # L = 23 padded to 24
    _st(4, 4, 34, EGCM, "lay"),                                         # L = 34 padded to 36, 36 of 64 lanes
    _st(8, 4, 21, EGCS, "lay"),
    _st(4, 4, 31, ("sum", "std", "max"), "lay"),
    _st(4, 4, 32, ("symnorm", "std", "max"), "lay"),
    _st(8, 4, 37, EGCS, "lay", graph="reduced"),
    _st(4, 4, 56, ("sum", "mean", "max"), "lay"),
    _st(8, 4, 44, EGCS, "looped", graph="reduced"),
    _st(8, 4, 44, ("mean",), "looped", graph="reduced", bias=False),
    _st(8, 4, 16, ("mean", "max"), "raw"),
    _st(8, 4, 16, ("sum",), "raw"),
    _st(4, 4, 16, ("mean", "max"), "raw"),
    _st(4, 4, 16, ("sum",), "raw", bias=False),
    # ---- register kernel: the run-time ladder, lane group x heads per lane x need mask
    *_rt_ladder(),
    # ---- register kernel: the edges of its rule
    Case(128, 8, 4, ("min", "std", "sum", "max"), "lay", "rt<4,2,SQ|MN>"),             # W = 128 = 8 * 16 exactly, A = 4, DPP
    Case(128, 8, 4, NORTH, "looped", "rt<4,2,0>", loops_all=False),                    # the north star without loops_all
    Case(184, 8, 4, ("symnorm", "max"), "lay", "rt<5,2,0>", loops_all=False),          # ... a padded basis
    Case(144, 4, 4, ("mean", "min"), "looped", "rt<6,1,MN>", loops_all=False, act="sigmoid"),
    Case(128, 8, 4, EGCM, "lay", "st<8,4,16,symnorm+max+mean,none,lay>", ldw=112),     # a strided weightings block
    Case(124, 4, 4, ("max", "mean"), "looped", "rt<5,1,0>", ldw=48),                   # ... a padded basis
    Case(4, 1, 1, ("sum", "max"), "looped", "rt<4,1,0>"),                              # one slot: 1 of 16 lanes
    Case(40, 2, 1, ("min", "var"), "raw", "rt<4,2,SQ|MN>"),                            # five slots
    # ---- two-slots-per-lane kernel: both compiled-in configurations
    Case(300, 4, 4, ("symnorm", "min", "max"), "lay", "wide:st<4,4,75,symnorm+min+max,none,lay>", graph="reduced"),
    Case(304, 8, 8, EGCS, "lay", "wide:st<8,8,38,symnorm,none,lay>", graph="reduced"),
    # ---- ... heads per lane x need mask; P odd and even
    Case(320, 4, 4, ("sum", "max"), "looped", "wide<1,0>", graph="reduced"),                       # P = 20
    Case(324, 4, 4, ("min", "std"), "lay", "wide<1,SQ|MN>", graph="reduced", act="hardtanh"),      # L = 81 padded to 84, P = 21
    Case(600, 8, 4, ("symnorm", "mean"), "lay", "wide<2,0>", graph="reduced", bias=False),         # L = 75 padded to 76, P = 19
    Case(576, 8, 4, ("var",), "raw", "wide<2,SQ|MN>", graph="reduced"),                            # P = 18, squares alone
    Case(792, 6, 2, ("max", "sum", "symnorm"), "looped", "wide<4,0>", graph="reduced", act="sigmoid"),   # P = 33
    Case(816, 6, 2, ("min", "mean"), "raw", "wide<4,SQ|MN>", graph="reduced"),                     # P = 34, min alone
    Case(320, 4, 4, ("sum", "max", "symnorm"), "looped", "wide<1,0>", graph="reduced", loops_all=False),
    Case(324, 4, 4, ("mean", "symnorm"), "lay", "wide<1,0>", graph="reduced", ldw=64),             # a strided weightings block
    # ---- ... and its refusal at B * P0 > 64: launch_all<2>
    Case(16, 4, 128, ("mean",), "lay", "lds<2>/4"),
    # ---- LDS kernels: every refusal of the register kernel at 64 slots or fewer
    Case(128, 8, 4, NORTH, "looped", "lds<1>/4", act="softmax"),
    Case(128, 8, 4, EGCM, "lay", "lds<1>/4", layout="HAB"),
    Case(42, 6, 3, ("max", "min", "mean"), "looped", "lds<1>/4"),                                  # B = 3; L = 7 padded to 8
    Case(28, 4, 2, ("sum", "std", "max"), "raw", "lds<1>/4", stride=7),                            # unpadded: ldb = 16 != B Ls = 14
    Case(64, 8, 4, ("sum", "mean", "max", "min", "symnorm"), "looped", "lds<1>/4", act="sigmoid"),  # five aggregators
    Case(64, 8, 1, ("mean", "max"), "raw", "lds<1>/4"),                                            # ceil(H / B) = 8; two slots
    Case(128, 8, 4, ("sum", "symnorm", "max"), "xl", "lds<1>/4"),                                  # x_looped && !y_looped
    Case(256, 16, 4, ("sum", "mean", "max"), "lay", "lds<1>/4"),                                   # W = 192: the next layer beyond 8 * 16
    Case(12, 3, 3, ("mean", "symnorm"), "lay", "lds<1>/4", bias=False),                            # three slots
    Case(42, 6, 3, ("symnorm", "var"), "looped", "lds<1>/4", loops_all=False, act="hardtanh"),
    Case(42, 6, 3, ("sum", "max"), "lay", "lds<1>/4", ldw=40),                                     # a strided weightings block
    # ---- LDS kernels: three and four chunks, one wavefront per block
    Case(384, 4, 8, ("symnorm", "max", "std"), "lay", "lds<3>/4", graph="reduced"),                # 192 slots
    Case(384, 4, 8, ("symnorm", "min"), "looped", "lds<3>/4", graph="reduced", loops_all=False),
    Case(512, 4, 8, ("mean", "min"), "raw", "lds<4>/4", graph="reduced"),                          # 256 slots
    Case(1024, 8, 8, ALL7, "looped", "lds<4>/1", graph="reduced"),
)
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
RECT_CASES = tuple(c for c in CASES if c.sets == "raw" and "symnorm" not in c.aggrs and c.graph == "ladder" and c.loops_all)
TIE_CASES = tuple(c for c in CASES if extrema(c))
NOLOOP_CASES = tuple(c for c in CASES if not c.loops_all)
STRIDED_CASES = tuple(c for c in CASES if c.ldw)
BIG_CASE = next(c for c in CASES if c.cell == "rt<6,1,0>")                                          # 36 slots: one-row groups
POST_SEED = 33


def runs(case):
    """Every (graph key, flip, ties, post variants) the GPU file runs a case on: what the CPU file holds the yardstick to."""
    got = [(home(case), False, False, tuple(VARIANTS)), (home(case), True, False, ("plain", "full")),
           (("sparse",), False, False, ("plain", "full")), (("edgeless",), False, False, ("plain", "full"))]
    if case in TIE_CASES:
        got.append((home(case), False, True, ("full",)))
    if case in RECT_CASES:
        got += [(("rect", more), flip, False, ("plain", "full")) for more in (True, False) for flip in (False, True)]
    return got


def family(case, n=32, env=()):
    """"reg contig" / "reg padded" / "wide" / "lds one chunk" / "lds chunks": the five epilogues of the post-op."""
    cell = dispatch(case, n, False, env)
    if cell.family == "reg":
        return "reg " + cell.store
    if cell.family == "wide":
        return "wide"
    return "lds one chunk" if cell.instance.startswith("lds<1>") else "lds chunks"


FAMILIES = ("reg contig", "reg padded", "wide", "lds one chunk", "lds chunks")


# ------------------------------------------------------------------------------------------------------------------------------
# the gather plan of a static graph as part of the rule

PLAN_SWITCH = "EGC_NO_GATHER_PLAN"
PLAN_FORMS = ((), ("EGC_NO_STATIC_CFG",))      # a compiled-in configuration and its rt<...,0> fallback are two compiled PLAN kernels


def plan_form(case, kind, rows=None, env=()):
    """True exactly when the call ``dispatch(case, n, ...)`` describes -- ``n`` the rows of the graph key ``kind``, ``rows`` a row
    range or None -- takes the PLAN form of agg_fast_kernel on a TRIMMED graph (CSRGraph.trim_launches(), whose plan the small
    graphs here always keep).  launch_one gives the form to every register instance without optional aggregates; aggregate_combine_impl
    offers a plan to a whole-graph inference launch on a square graph unless EGC_NO_GATHER_PLAN is set."""
    ei, n, n_src = edges(*graph_key(case, kind, False))
    whole = rows is None or tuple(rows) == (0, n)
    return (dispatch(case, n if rows is None else rows[1] - rows[0], False, env).family == "reg" and need_of(case) == "0"
            and n_src == n and whole and PLAN_SWITCH not in env)


def plan_instances(source=None):
    """The PLAN instances the library compiles, by name: every EGC_STATIC_CFG row of need 0 and the need-0 column of the RtCfg ladder."""
    return ({r.name for r in static_rows(source) if r.kind == "reg" and r.need == "0"}
            | {f"rt<{lg},{hpb},0>" for lg in (4, 5, 6) for hpb in (1, 2, 4)})


PLAN_CASES = tuple(c for c in CASES if plan_form(c, home(c)))
