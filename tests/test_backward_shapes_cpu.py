"""The table of the layer-backward sweep without a GPU (tests/backward_ref.py).  This guards the TABLE and the restatement, not
the kernels: that the cases reach every kernel instance egc_backward.hip launches and every branch of its dispatch rule (the
instances are the rows of the lists of egc_backward_host.h, which the launches expand from, so one added there without a case fails here), that the rule agrees with the library
where the library can be asked without a device, that the sweep graphs have the rows they are built for on both sides and sit on
the intended side of the rule that turns the extremum records on, and that the operand-level restatement is the mathematics of the
module-level one."""
import ctypes as C

import numpy as np
import pytest
import torch

import backward_ref
from backward_ref import (ALL7, BOUNDARY_CASES, BOUNDARY_ROWS, BWD_FU, CASES, CHUNK, GRAPH_SEED, INPUT_SEED, LENGTHS, RECORD_CASES,
                          RECT_CASES, REC_BALLOT_MAX, REC_ITEMS, THRESHOLD, Case, arg_extrema_instance, boundary, case_graph,
                          degrees, dispatch, extrema, geometry, gradients, ladder, make_inputs, records_apply, rect, rel_grad,
                          source_instances, sparse, stdvar, CODES, ACTS, SETS)
from egc_amd import _C
from egc_amd.functional import make_spec
from oracle import egc_torch_ref as tref

MODES = ((), ("EGC_BWD_NO_REC",), ("EGC_BWD_REC_SEPARATE",), ("EGC_BWD_GENERIC",))


def _spec(case):
    agg_set, sym_set = SETS[case.sets]
    return make_spec(16, case.out, case.H, case.B, [CODES[a] for a in case.aggrs], agg_set, sym_set, True, _C.LAYOUT_HBA,
                     ACTS[case.act], basis_stride=geometry(case)[1])


def _cells():
    """{(case name, graph, mode): Cell} over everything the GPU file runs."""
    cells = {}
    for c in CASES:
        ei, n, _ = case_graph(c)
        for mode in MODES:
            cells[(c.name, c.graph, mode)] = dispatch(c, n, ei.shape[1], mode)
        if c in RECORD_CASES:
            ei, n, _ = sparse(GRAPH_SEED)
            cells[(c.name, "sparse", ())] = dispatch(c, n, ei.shape[1])
    return cells


def test_every_case_takes_the_destination_kernel_the_table_names():
    for c in CASES:
        ei, n, _ = case_graph(c)
        assert dispatch(c, n, ei.shape[1]).dst == c.dst, c.name
        assert dispatch(c, n, ei.shape[1], ("EGC_BWD_GENERIC",)).dst.startswith("lds/"), c.name
        assert geometry(c)[2] == _C.load().egc_bases_ld(C.byref(_spec(c).c)), c.name


def test_the_table_reaches_every_instance_the_source_launches():
    """Every launch of egc_backward.hip against the cells of the table; no compiled instance is out of a legal layer's reach."""
    src = source_instances()
    cells = _cells()
    assert len(src["dst"]) == 16 and len(src["src"]) == 13 + 4                  # what the file launches today
    assert {c.dst for c in cells.values() if c.dst.startswith("fast")} == src["dst"]
    assert {c.dst for c in cells.values() if c.dst.startswith("lds")} == {"lds/4", "lds/1"}
    assert {c.src for c in cells.values()} == src["src"]
    assert {c.rec for c in cells.values()} == {"off", "fused"} | src["rec"] and len(src["rec"]) == 4
    assert {arg_extrema_instance(c) for c in CASES} - {None} == src["arg"] == {1, 2, 3, 4}
    # the compiled flag words run with AND without records (low-degree batches), the run-time form at every slot count
    default = {k: c for k, c in cells.items() if k[2] == ()}
    assert {c.src for c in default.values()} == src["src"]
    unreachable = set()                                                         # (none: named here if one appears)
    assert src["dst"] - {c.dst for c in default.values()} == unreachable


def test_the_table_reaches_every_branch_of_the_rule():
    cells = _cells()
    default = {k[0]: c for k, c in cells.items() if k[1] != "sparse" and k[2] == ()}
    for lg in (4, 5, 6):       # per lane-group size: a power-of-two basis by butterfly (H a multiple of P, H < P) and another through LDS
        assert {c.basis for c in default.values() if c.dst.startswith(f"fast<{lg}")} == {"p2:H%P", "p2:H<P", "np2"}, lg
    assert {c.lpr_log2 for c in default.values()} == {4, 5, 6}
    by = {c.name: c for c in CASES}
    fast = [by[k] for k, c in default.items() if c.dst.startswith("fast")]
    lds = [by[k] for k, c in default.items() if c.dst.startswith("lds")]
    assert {c.act for c in fast} == {"none", "sigmoid", "hardtanh"} and {c.act for c in lds} == set(ACTS)
    assert any(c.act != "none" and default[c.name].basis == "np2" for c in fast)           # the nonlinearity behind the transposed shares
    assert {c.sets for c in fast} == {c.sets for c in lds} == set(SETS)
    assert {geometry(c)[0] != geometry(c)[1] for c in fast} == {geometry(c)[0] != geometry(c)[1] for c in lds} == {True, False}
    assert any(geometry(c)[3] < (1 << default[c.name].lpr_log2) for c in fast)           # idle lanes of a lane group
    assert {1, 16} <= {c.B for c in fast} and set(ALL7) == {a for c in CASES for a in c.aggrs}
    assert {len(c.aggrs) for c in fast} == {1, 3, 4} and max(len(c.aggrs) for c in lds) == 7
    # every record mode at a fused-capable and at an LDS cell; one and two record arrays
    assert {extrema(c) for c in RECORD_CASES} == {1, 2}
    for name, kind in (("64-H8-B4-sum+mean+max+symnorm-looped", "fused"), ("42-H6-B3-max+min+mean-looped", "sep<1>")):
        assert [cells[(name, "ladder", m)].rec for m in MODES[:3]] == [kind, "off", "sep<1>"]
        assert cells[(name, "sparse", ())].rec == "off"
    # the trained nets' shapes
    trained = {(124, 4, 4), (128, 4, 4), (136, 4, 4), (168, 8, 4), (224, 4, 4), (296, 8, 4), (64, 8, 4)}
    assert trained <= {(c.out, c.H, c.B) for c in CASES}


def test_removing_a_case_or_adding_an_instance_is_noticed():
    """The two checks above do fail: without the only case of a cell, and with a row or a launch the table does not know."""
    src = source_instances()
    lone = "fast<5,4,3,symnorm+std+max>"
    fewer = tuple(c for c in CASES if c.dst != lone)
    assert len(fewer) == len(CASES) - 1
    reached = set()
    for c in fewer:
        ei, n, _ = case_graph(c)
        reached |= {dispatch(c, n, ei.shape[1], m).dst for m in MODES}
    assert src["dst"] - reached == {lone}
    lists = backward_ref.source_text("egc_backward_host.h")
    head = "#define EGC_BWD_SRC_FLAGS(ROW)"
    more = lists.replace(head, head + " ROW(SRC_T | SRC_N)")                    # one more row of the list
    assert more != lists and source_instances(more)["src"] - src["src"] == {"src<1,T|N>"}
    with pytest.raises(AssertionError):                                         # a literal launch beside the list
        source_instances(source=backward_ref.source_text() + "\n  bwd_src_kernel<1, SRC_STATIC | SRC_T | SRC_N><<<grid, 256, 0, stream>>>(a);\n")


def test_the_rule_agrees_with_the_library_on_records():
    """egc_backward_workspace_bytes_for reserves 64 bytes per entry and extremum exactly where the rule says records are built --
    asked of the library itself, which reads nothing of the graph but its two counts."""
    lib = _C.load()
    graphs = [case_graph(CASES[0]), sparse(GRAPH_SEED)] + [boundary(GRAPH_SEED, ldb, on) for ldb in (24, 64) for on in (True, False)]
    seen = set()
    for c in CASES:
        spec = _spec(c)
        for ei, n, _ in graphs + [case_graph(c)]:
            e = ei.shape[1]
            g = _C.EgcGraph(n, e, None, None, None, None, None, None, None, -1, n, None, None)
            small = lib.egc_backward_workspace_bytes(C.byref(spec.c), n)
            big = lib.egc_backward_workspace_bytes_for(C.byref(spec.c), C.byref(g))
            want = records_apply(c, n, e)
            assert big - small == (extrema(c) * e * 64 if want else 0), (c.name, n, e)
            seen.add(want)
    assert seen == {True, False}


def test_the_graphs_are_on_the_intended_side_of_the_record_rule():
    for c in RECORD_CASES:
        ldb = geometry(c)[2]
        for flip in (False, True):
            ei, n, _ = case_graph(c, flip)
            assert ldb * n <= 10 * ei.shape[1]                                   # near side: records at every ldb <= 256
            ei, n, _ = sparse(GRAPH_SEED, flip)
            assert ldb * n > 10 * ei.shape[1]                                    # far side: none, already at 16 columns
    assert min(geometry(c)[2] for c in RECORD_CASES) == 16 and max(geometry(c)[2] for c in RECORD_CASES) == 256
    for c in BOUNDARY_CASES:
        ldb = geometry(c)[2]
        on, off = boundary(GRAPH_SEED, ldb, True), boundary(GRAPH_SEED, ldb, False)
        assert ldb * BOUNDARY_ROWS == 10 * on[0].shape[1] == 10 * (off[0].shape[1] + 1)
        assert dispatch(c, on[1], on[0].shape[1]).rec != "off" and dispatch(c, off[1], off[0].shape[1]).rec == "off"


@pytest.mark.parametrize("flip", (False, True), ids=("ladder", "flip"))
def test_the_ladder_has_its_rows_on_both_sides(flip):
    for reduced in (False, True):
        ei, n, n_src = ladder(GRAPH_SEED, flip, reduced)
        assert n == n_src and ei.dtype == np.int64 and ei.min() >= 0 and ei.max() < n
        want = backward_ref.ladder_lengths(reduced)
        assert set(want) == {r for r in LENGTHS if not reduced or r <= 2 * CHUNK + 1}
        indeg, outdeg = degrees(ei, n, n_src)
        assert sorted(indeg) == sorted(outdeg) == sorted(want) and not np.array_equal(indeg, outdeg)
        both = set(indeg)
        assert {BWD_FU - 1, BWD_FU, BWD_FU + 1, THRESHOLD - 1, THRESHOLD, THRESHOLD + 1, CHUNK - 1, CHUNK, CHUNK + 1} <= both
        assert {1, 2, REC_BALLOT_MAX, REC_BALLOT_MAX + 1, CHUNK + REC_BALLOT_MAX, CHUNK + REC_BALLOT_MAX + 1} <= both
        assert min(geometry(c)[2] for c in RECORD_CASES) > REC_ITEMS             # a one-entry row overflows its record at every width
        for deg in (indeg, outdeg):                                              # long rows first, last and adjacent on either side
            long = deg > THRESHOLD
            assert long[0] and long[-1] and (long[:-1] & long[1:]).any() and (deg[1:-1] == 0).any()
        assert int((ei[0] == ei[1]).sum()) >= 5
        pairs = ei[0] * n + ei[1]
        assert len(pairs) - len(np.unique(pairs)) >= 20
        hub = int(indeg.argmax())
        assert int((ei[0][ei[1] == hub] == hub).sum()) >= 1                      # a self loop inside a chunked row (skipped when LOOPED)
        at = np.nonzero(ei[1] == hub)[0]
        assert at.max() - at.min() > len(at)                                     # shuffled: only a stable sort gets the CSR right
        assert 3500 <= ladder(GRAPH_SEED, flip)[0].shape[1] <= 4500 and n <= 32
    a, b = ladder(GRAPH_SEED, flip), ladder(GRAPH_SEED, not flip)
    assert np.array_equal(a[0], b[0][::-1])


def test_the_variants_have_the_rows_they_are_built_for():
    for more in (True, False):
        ei, n, n_src = rect(GRAPH_SEED, more)
        assert (n_src > n) == more and n_src != n and sorted(degrees(ei, n, n_src)[0]) == sorted(degrees(*ladder(GRAPH_SEED))[0])
        outdeg = degrees(ei, n, n_src)[1]
        assert int(((outdeg > 0) & (outdeg <= THRESHOLD)).sum()) >= 3 and int((outdeg > THRESHOLD).sum()) >= 3
        fe, fn, fs = rect(GRAPH_SEED, more, flip=True)
        assert (fn, fs) == (n_src, n) and np.array_equal(fe, ei[::-1])
    ei, n, n_src = sparse(GRAPH_SEED)
    indeg, outdeg = degrees(ei, n, n_src)
    assert indeg.max() == 17 and {1, 2, 3, 4, 5, 8, 9, 16, 17} <= set(indeg) and outdeg.max() <= THRESHOLD and n > 100
    assert int((ei[0] == ei[1]).sum()) >= 5
    assert RECT_CASES and all(c.sets == "raw" for c in RECT_CASES)
    ei, n, _ = rect(GRAPH_SEED, True)
    assert {dispatch(c, n, ei.shape[1]).dst.split("<")[0] for c in RECT_CASES} == {"fast", "lds/4"}


def test_the_operand_level_restatement_is_the_module_level_one():
    """Gradients of d_bases / d_weightings pushed through the dense part by hand equal float32 autograd through
    oracle/egc_torch_ref.py on one small layer of either kind (padded bases, self loops, softmax)."""
    rng = np.random.default_rng(5)
    n, fin = 40, 12
    ei = rng.integers(0, n, size=(2, 300)).astype(np.int64)
    ei[1, :90] = 3
    ei[:, 290:] = ei[0, 290:]
    torch.manual_seed(0)
    for case, kind in ((Case(24, 4, 2, ("sum", "mean", "max", "symnorm", "std"), "looped", ""), "opt"),
                       (Case(28, 4, 2, ("symnorm", "min", "var"), "lay", "", act="softmax"), "lay"),
                       (Case(28, 4, 2, ("mean", "max"), "lay", "", act="hardtanh"), "lay")):
        L, Ls, ldb, _, A, W = geometry(case)
        H, B = case.H, case.B
        x = torch.randn(n, fin, requires_grad=True)
        wb = torch.randn(fin, B * L, requires_grad=True)
        cw, cb = torch.randn(W, fin, requires_grad=True), torch.randn(W, requires_grad=True)
        gout = torch.randn(n, case.out)
        bases_real = x @ wb                                                    # [n, B L]
        wt = x @ cw.t() + cb                                                   # HBA columns
        if kind == "opt":                                                      # the reference's column order is h A B + a B + b
            hab = torch.tensor([(h * B + b) * A + a for h in range(H) for a in range(A) for b in range(B)])
            ref = tref.egconv_forward(x, ei, wb, cw[hab], cb[hab], None, H, B, list(case.aggrs))
        else:
            names = ["symadd" if a == "symnorm" else "add" if a == "sum" else a for a in case.aggrs]
            ref = tref.efficient_graph_conv_forward(x, ei, [wb[:, b * L:(b + 1) * L] for b in range(B)], cw, cb, None, H, names,
                                                    softmax=case.act == "softmax", hardtanh=case.act == "hardtanh")
        want = torch.autograd.grad(ref, (x, wb, cw, cb), gout)
        bases = torch.zeros(n, ldb)
        bases[:, :B * Ls].view(n, B, Ls)[:, :, :L] = bases_real.detach().view(n, B, L)
        out, d_b, d_w = gradients(bases.numpy(), wt.detach().numpy(), gout.numpy(), ei, n, case, torch.float32)
        assert rel_grad(out, ref.detach().numpy()) <= 1e-5
        d_real = torch.from_numpy(d_b)[:, :B * Ls].view(n, B, Ls)
        assert float(d_real[:, :, L:].abs().max()) == 0.0 if Ls > L else True   # the padding takes no part
        got = torch.autograd.grad((bases_real, wt), (x, wb, cw, cb), (d_real[:, :, :L].reshape(n, B * L), torch.from_numpy(d_w)))
        for g, w in zip(got, want):
            assert rel_grad(g.numpy(), w.numpy()) <= 1e-5


@pytest.mark.parametrize("case", [c for c in CASES if stdvar(c)], ids=lambda c: c.name)
def test_the_yardstick_of_std_and_var_stays_below_the_ceiling(case):
    """With std / var the bound of the GPU file is twice the float32 restatement's own distance from float64, never more than the
    2e-4 of tests/test_backward_gpu.py: the yardstick itself stays below that on every such case and input set."""
    for flip in (False, True):
        ei, n, n_src = case_graph(case, flip)
        for ties in ((False, True) if extrema(case) else (False,)):
            ins = make_inputs(case, n, n_src, INPUT_SEED, ties)
            f32, f64 = (gradients(*ins, ei, n, case, dt) for dt in (torch.float32, torch.float64))
            for a, b in zip(f32[1:], f64[1:]):
                assert rel_grad(a, b) <= 2e-4, (flip, ties, rel_grad(a, b))
