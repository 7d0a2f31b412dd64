"""The table of the inference-aggregate sweep without a GPU (tests/forward_ref.py).  This guards the TABLE and the restatement, not
the kernels: that every compiled-in configuration of egc_aggregate_fast.hip has a case the rule sends to it (a row added there
without a case fails here), that the cells the cases reach under the four switch sets are the full enumerated set -- asserted on
the set itself, so a dropped case fails --, that the restatement means what it says about ``n_loop``, empty rows and the post-op
and is backward_ref's with default arguments, and that the bound of the GPU file is usable: on every (case, graph, post variant)
it runs, the restatement in float32 stays within HALF of the 1e-5 element-wise bound of its own float64 evaluation."""
import numpy as np
import pytest
import torch

import backward_ref
import forward_ref
from forward_ref import (BIG_CASE, CASES, FAMILIES, GRAPH_SEED, INPUT_SEED, NOLOOP_CASES, POST_SEED, RECT_CASES, RPW_ROWS, STRIDED_CASES,
                         SWITCHES, TAIL_ROWS, THRESHOLD, TIE_CASES, VARIANTS, Case, Post, aggregate_combine, agg_lpr, big, dispatch,
                         edges, family, forms, forward, geometry, graph_key, hba_columns, home, make_inputs, make_post,
                         n_loop_of, post_of, post_op, runs, static_rows)
from golden_util import elementwise_excess

NEEDS = ("0", "SQ", "MN", "SQ|MN")


def _rows(case):
    return edges(*graph_key(case, home(case), False))[1]


def _cells(cases=CASES):
    """{(case name, switch set): Cell} on every case's own graph, and the register kernel's two row schedules on the big one."""
    cells = {(c.name, env): dispatch(c, _rows(c), False, env) for c in cases for env in SWITCHES}
    if BIG_CASE in cases:
        cells[(BIG_CASE.name, "big")] = dispatch(BIG_CASE, RPW_ROWS)
        cells[(BIG_CASE.name, "big less one row")] = dispatch(BIG_CASE, RPW_ROWS - 1)
    return cells


def _enumerated(rows):
    """The full cell set of the rule: (family, instance)."""
    want = {("wide" if r.kind == "wide" else "reg", r.name) for r in rows}
    want |= {("reg", f"rt<{lg},{hpb},{need}>") for lg in (4, 5, 6) for hpb in (1, 2, 4) for need in NEEDS}
    want |= {("wide", f"wide<{hpb},{need}>") for hpb in (1, 2, 4) for need in ("0", "SQ|MN")}
    want |= {("lds", f"lds<{ch}>/4") for ch in (1, 2, 3, 4)} | {("lds", "lds<4>/1")}
    return want


REASONS = {"HAB", "softmax", "xl", "unpadded", "B", "A>4", "hpb>4", "W", "B*P0>64", "slots>128", "forced", "no_wide"}


def test_every_case_takes_the_cell_the_table_names():
    for c in CASES:
        assert dispatch(c, _rows(c)).instance == c.cell, c.name
        assert dispatch(c, _rows(c), True).instance == c.cell, c.name            # ... with a post-op too
        assert dispatch(c, _rows(c), False, ("EGC_FORCE_GENERIC",)).family == "lds", c.name
        assert forms(c, _rows(c))[0] == ()


def test_every_compiled_in_configuration_has_a_case():
    rows = static_rows()
    assert len([r for r in rows if r.kind == "reg"]) == 19 and len([r for r in rows if r.kind == "wide"]) == 2   # what the file holds today
    assert len({r.name for r in rows}) == len(rows)
    named = {c.cell for c in CASES if "st<" in c.cell}
    assert named == {r.name for r in rows}              # none without a case, no case naming a row that is not in the source
    reached = {cell.instance for cell in _cells().values() if "st<" in cell.instance}
    assert reached == named
    # a row added to the source is noticed; so is a use of the macro the parser does not understand
    source = backward_ref.source_text("egc_aggregate_fast.hip")
    line = "    EGC_STATIC_CFG(8, 4, 16, 2, agg_pack(S, X), EGC_ACT_NONE, false, false, true, 0)\n"
    anchor = "    // EGConv / EGC-S default"
    more = source.replace(anchor, line + anchor)
    assert more != source and {r.name for r in static_rows(more)} - named == {"st<8,4,16,sum+max,none,raw>"}
    with pytest.raises(AssertionError):
        static_rows(source.replace(anchor, "    EGC_STATIC_CFG(8, 4, 16, 2, some_other_pack(S, X), EGC_ACT_NONE, false, false, true, 0)\n" + anchor))


def test_the_cells_the_cases_reach_are_the_full_enumerated_set():
    cells = _cells()
    assert {(c.family, c.instance) for c in cells.values()} == _enumerated(static_rows())
    assert {c.reason for c in cells.values() if c.family == "lds"} == REASONS
    default = {k[0]: c for k, c in cells.items() if k[1] == ()}
    assert {c.reason for c in default.values() if c.family == "lds"} == REASONS - {"forced", "no_wide"}
    # every refusal of the register kernel at 64 slots or fewer
    small = {default[c.name].reason for c in CASES if geometry(c)[3] <= 64 and default[c.name].family == "lds"}
    assert small == {"HAB", "softmax", "xl", "unpadded", "B", "A>4", "hpb>4", "W"}
    assert {c.rows_per_wave for c in cells.values() if c.family == "reg"} == {1, 4}
    assert cells[(BIG_CASE.name, "big")].rows_per_wave == 4 and cells[(BIG_CASE.name, "big less one row")].rows_per_wave == 1
    assert big(GRAPH_SEED)[1] == RPW_ROWS and 32 < geometry(BIG_CASE)[3] <= 64
    assert {c.lpr_log2 for c in cells.values() if c.family == "lds"} == {0, 1, 2, 3, 4, 5, 6}
    assert {1, 2, 3, 5} <= {geometry(c)[3] for c in CASES}                                 # slot counts of the LDS kernels' small lane groups
    # the run-time ladder is reached WITHOUT a switch, by layers that match no compiled-in configuration
    assert {c.instance for c in default.values() if c.instance.startswith("rt<")} == \
        {f"rt<{lg},{hpb},{need}>" for lg in (4, 5, 6) for hpb in (1, 2, 4) for need in NEEDS}
    assert {c.instance for c in default.values() if c.instance.startswith("wide<")} == \
        {f"wide<{hpb},{need}>" for hpb in (1, 2, 4) for need in ("0", "SQ|MN")}


def test_the_cases_reach_every_variant_of_the_epilogues():
    cells = _cells()
    default = {k[0]: c for k, c in cells.items() if k[1] == ()}
    by = {c.name: c for c in CASES}
    reg = [by[k] for k, c in default.items() if c.family == "reg"]
    wide = [by[k] for k, c in default.items() if c.family == "wide"]
    lds = [by[k] for k, c in default.items() if c.family == "lds"]
    for lg in (4, 5, 6):
        assert {default[c.name].store for c in reg if default[c.name].lpr_log2 == lg} == {"contig", "padded"}, lg
    assert {default[c.name].basis for c in reg} == {"dpp", "p2", "np2"}
    for tag in ("rt<", "st<"):                                                             # the DPP form at run-time and compiled-in constants
        assert any(default[c.name].basis == "dpp" and default[c.name].instance.startswith(tag) for c in reg)
    idle = {(geometry(c)[3], agg_lpr(geometry(c)[3])) for c in reg}
    assert {(12, 16), (36, 64), (1, 16), (16, 16), (32, 32), (64, 64)} <= idle
    assert {len(c.aggrs) for c in reg} == {1, 2, 3, 4} and {len(c.aggrs) for c in wide} >= {1, 2, 3}
    assert {c.act for c in reg} == {c.act for c in wide} == {"none", "sigmoid", "hardtanh"} and {c.act for c in lds} == set(backward_ref.ACTS)
    assert any(geometry(c)[5] == 8 * agg_lpr(geometry(c)[3]) for c in reg)                 # W on the edge of the register kernel ...
    assert any(default[c.name].reason == "W" and geometry(c)[5] > 8 * agg_lpr(geometry(c)[3]) for c in lds)   # ... and beyond it
    assert {default[c.name].basis for c in wide} == {"odd", "even"} and {default[c.name].store for c in wide} == {"contig", "padded"}
    assert {c.sets for c in reg} == {c.sets for c in wide} == {"raw", "looped", "lay"} and {c.sets for c in lds} == set(forward_ref.SETS)
    for group in (reg, wide, lds):
        assert {c.bias for c in group} == {True, False} and {c.loops_all for c in group} == {True, False}
        assert any(c.ldw for c in group)
    assert all(c.ldw % 4 == 0 and c.ldw >= geometry(c)[5] + 4 for c in STRIDED_CASES)
    assert all(c.sets != "raw" for c in NOLOOP_CASES)
    assert {family(c) for c in CASES} == set(FAMILIES)
    assert {family(c) for c in NOLOOP_CASES} == set(FAMILIES) and {family(c) for c in TIE_CASES} == set(FAMILIES)
    assert {dispatch(c, 32).family for c in RECT_CASES} == {"reg", "lds"}
    assert set(backward_ref.ALL7) == {a for c in CASES for a in c.aggrs} and {"HBA", "HAB"} == {c.layout for c in CASES}
    assert any(c.stride == c.out // c.H and geometry(c)[2] != c.B * geometry(c)[1] for c in lds)
    # several chunks and one wavefront per block
    assert {default[c.name].instance for c in lds} == {"lds<1>/4", "lds<2>/4", "lds<3>/4", "lds<4>/4", "lds<4>/1"}


def test_dropping_a_case_is_noticed():
    rows = static_rows()
    for lone in ("rt<5,4,MN>", "wide<2,SQ|MN>", "lds<4>/1", "st<8,4,16,sum,none,raw>"):
        fewer = tuple(c for c in CASES if c.cell != lone)
        assert 0 < len(CASES) - len(fewer) <= 2
        got = {(c.family, c.instance) for c in _cells(fewer).values()}
        assert _enumerated(rows) - got == {(("wide" if lone.startswith("wide") else "lds" if lone.startswith("lds") else "reg"), lone)}


# ------------------------------------------------------------------------------------------------------------------------------
# the restatement

def _inputs(case, kind, flip, ties=False):
    ei, n, n_src = edges(*graph_key(case, kind, flip))
    bases, wt, _ = make_inputs(case, n, n_src, INPUT_SEED, ties)
    ops = make_post(case, n, POST_SEED)
    if not case.bias:
        ops["bias"] = None
    return ei, n, n_src, bases, wt, ops


def test_with_default_arguments_the_restatement_is_the_backward_sweeps():
    for case in backward_ref.CASES[:6] + backward_ref.CASES[31:34]:
        ei, n, n_src = backward_ref.case_graph(case)
        bases, wt, _ = make_inputs(case, n, n_src, INPUT_SEED)
        b, w = torch.from_numpy(bases), torch.from_numpy(wt)
        fcase = Case(case.out, case.H, case.B, case.aggrs, case.sets, "", act=case.act, graph=case.graph)
        assert geometry(fcase) == geometry(case)
        assert torch.equal(forward(b, w, ei, n, fcase), backward_ref.aggregate_combine(b, w, ei, n, case))
        assert torch.equal(forward(b, w, ei, n, fcase, n_loop=n), backward_ref.aggregate_combine(b, w, ei, n, case))


def test_the_post_op_is_its_definition_line_by_line():
    rng = np.random.default_rng(3)
    z, bias, scale, shift, res = (rng.standard_normal(s) for s in ((7, 5), 5, 5, 5, (7, 5)))
    scale[::2] *= -1
    t = torch.from_numpy
    full = post_op(t(z), t(bias), Post(t(scale), t(shift), t(res), True)).numpy()
    want = np.empty_like(z)
    for i in range(7):
        for j in range(5):
            v = (z[i, j] + bias[j]) * scale[j] + shift[j]
            want[i, j] = (v if v > 0 else 0.0) + res[i, j]
    assert np.array_equal(full, want) and (want == res).any() and (want != res).any()       # relu cuts some, not all
    assert np.array_equal(post_op(t(z), None, None).numpy(), z)
    assert np.array_equal(post_op(t(z), t(bias), None).numpy(), z + bias)
    assert np.array_equal(post_op(t(z), None, Post(relu=True)).numpy(), np.maximum(z, 0))
    assert np.array_equal(post_op(t(z), None, Post(residual=t(res))).numpy(), z + res)
    assert np.array_equal(post_op(t(z), t(bias), Post(t(scale), t(shift))).numpy(), (z + bias) * scale + shift)
    assert post_op(t(z).float(), t(bias).float(), Post(t(scale).float(), t(shift).float(), t(res).float(), True)).dtype == torch.float32
    ops = make_post(CASES[0], 9, POST_SEED)
    assert (ops["scale"] > 0).any() and (ops["scale"] < 0).any() and np.abs(ops["scale"]).min() >= 0.5 and np.abs(ops["scale"]).max() <= 2
    assert set(VARIANTS) == {"plain", "full", "affine", "relu", "residual"}
    for v, parts in VARIANTS.items():
        bias, post = post_of(ops, v, torch.float64)
        assert (post is None) == (v == "plain")
        if post is not None:
            assert ((post.scale is not None) == (post.shift is not None) == ("affine" in parts)
                    and (post.residual is not None) == ("residual" in parts) and post.relu == ("relu" in parts))


def test_the_weight_layouts_name_the_same_weight():
    case = next(c for c in CASES if c.layout == "HAB")
    n, A = 3, len(case.aggrs)
    w = torch.arange(n * case.H * case.B * A, dtype=torch.float64).view(n, -1)
    hba = hba_columns(w, case)
    for h in range(case.H):
        for b in range(case.B):
            for a in range(A):
                assert hba[1, (h * case.B + b) * A + a] == w[1, (h * A + a) * case.B + b]


@pytest.mark.parametrize("case", NOLOOP_CASES, ids=lambda c: c.name)
def test_without_loops_all_only_rows_up_to_the_largest_index_get_a_self_loop(case):
    """The tail rows (in no edge, beyond the largest index) equal the epilogue of an empty row; with a self loop on every row
    they do not; rows up to the largest index are those of the looped ladder."""
    ei, n, n_src, bases, wt, ops = _inputs(case, ("tail",), False)
    n_loop = n_loop_of(case, ei, n)
    assert n_loop == n - TAIL_ROWS == int(ei.max()) + 1 and n_loop_of(case._replace(loops_all=True), ei, n) == n
    assert n_loop_of(case, np.zeros((2, 0), dtype=np.int64), 9) == 0
    looped = backward_ref.edge_sets(ei, n, "looped", n_loop)[backward_ref._C.SET_LOOPED]
    assert looped[0].shape[1] == int((ei[0] != ei[1]).sum()) + n_loop and looped[0][:, -1].tolist() == [n_loop - 1, n_loop - 1]
    assert (looped[1][-n_loop:] == ei.shape[1]).all()
    b, w = torch.from_numpy(bases).double(), torch.from_numpy(wt).double()
    some = aggregate_combine(b, w, ei, n, case, n_loop)
    every = aggregate_combine(b, w, ei, n, case)
    empty = aggregate_combine(b, w, np.zeros((2, 0), dtype=np.int64), n, case, 0)
    assert torch.equal(some[n_loop:], empty[n_loop:]) and not torch.equal(every[n_loop:], empty[n_loop:])
    ladder_only = aggregate_combine(b[:n_loop], w[:n_loop], ei, n_loop, case)
    assert torch.allclose(some[:n_loop], ladder_only, rtol=0, atol=0)
    # the empty row's aggregates: zero but for std, sqrt(eps) -- the epilogue applies bias, post-op and residual once
    act = backward_ref.activate(w, case.H, case.act).view(n, case.H, case.B, len(case.aggrs))
    L = case.out // case.H
    want = torch.zeros(n, case.H, L, dtype=torch.float64)
    for a, name in enumerate(case.aggrs):
        if name == "std":
            want += act[:, :, :, a].sum(dim=2, keepdim=True) * 1e-5 ** 0.5
    assert torch.allclose(empty.view(n, case.H, L), want, rtol=1e-12, atol=1e-12)


def test_rows_without_entries():
    """Every aggregate of an empty row is zero (std: sqrt(1e-5)); a LOOPED set leaves the row its own features."""
    case = Case(64, 8, 4, ("sum", "mean", "max", "min", "var", "symnorm"), "looped", "")
    ei, n, n_src = forward_ref.edgeless()
    bases, wt, _ = make_inputs(case, n, n_src, INPUT_SEED)
    b, w = torch.from_numpy(bases).double(), torch.from_numpy(wt).double()
    assert float(aggregate_combine(b, w, ei, n, case, 0).abs().max()) == 0.0
    own = aggregate_combine(b, w, ei, n, case)                                  # sum = mean = max = min = symnorm = x, var = 0
    L, Ls, ldb, _, A, W = geometry(case)
    x = backward_ref.real_columns(b, case.B, L, Ls).view(n, case.B, L)
    wsum = w.view(n, case.H, case.B, A)[:, :, :, [0, 1, 2, 3, 5]].sum(dim=3)
    assert torch.allclose(own.view(n, case.H, L), torch.einsum("nhb,nbl->nhl", wsum, x), rtol=1e-12, atol=1e-12)


def test_the_graphs_are_what_they_are_built_for():
    ei, n, _ = big(GRAPH_SEED)
    lad, n0, _ = backward_ref.ladder(GRAPH_SEED)
    deg = np.bincount(ei[1], minlength=n)
    assert n == RPW_ROWS and np.array_equal(deg[:n0], np.bincount(lad[1], minlength=n0)) and set(deg[n0:]) == {1, 2}
    assert ei.min() >= 0 and ei.max() < n
    for reduced in (False, True):
        t, nt, _ = forward_ref.tail(GRAPH_SEED, False, reduced)
        assert nt == backward_ref.ladder(GRAPH_SEED, False, reduced)[1] + TAIL_ROWS and int(t.max()) == nt - TAIL_ROWS - 1
        deg = np.bincount(t[1], minlength=nt)
        long = deg > THRESHOLD
        assert (long[:-1] & long[1:]).any() and any(long[r] and not long[r - 1] and not long[r + 1] for r in range(1, nt - 1))
    assert forward_ref.edgeless()[0].shape == (2, 0)
    # an unpadded basis keeps its padding columns at the end of the row, and they are zero
    case = next(c for c in CASES if c.stride)
    bases = make_inputs(case, 8, 8, INPUT_SEED)[0]
    L, Ls, ldb, _, _, _ = geometry(case)
    assert Ls == L and ldb > case.B * L and (bases[:, :case.B * L] != 0).mean() > 0.8 and (bases[:, case.B * L:] == 0).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_bound_is_usable(case):
    """The float32 restatement against itself in float64, on everything the GPU file runs the case on: at most HALF the 1e-5
    element-wise bound on the scale of the element's own row, so that a correct float32 kernel has the other half."""
    worst = 0.0
    for kind, flip, ties, variants in runs(case):
        ei, n, n_src, bases, wt, ops = _inputs(case, kind, flip, ties)
        n_loop = n_loop_of(case, ei, n)
        z = {dt: aggregate_combine(torch.from_numpy(bases).to(dt), hba_columns(torch.from_numpy(wt).to(dt), case), ei, n, case, n_loop)
             for dt in (torch.float32, torch.float64)}
        for v in variants:
            out = {dt: post_op(z[dt], *post_of(ops, v, dt)).numpy() for dt in z}
            excess = elementwise_excess(out[torch.float32], out[torch.float64], tol=1e-5)
            worst = max(worst, excess)
            assert excess <= 0.5, (kind, flip, ties, v, excess)
    print(f"{case.name}: float32 restatement, worst excess {worst:.3f}")
