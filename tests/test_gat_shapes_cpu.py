"""The (H, C) table of the GATv2 geometry sweep without a GPU (tests/gat_ref.py: SWEEP_SHAPES, geometry, sweep_graph).  This guards
the TABLE, not the kernel: that its shapes reach every template instance and group size of egc_gatv2.hip and the slot boundary at
column 256, that ``geometry`` restates the library's own (where the library can be asked without a device), that the sweep graph
has the rows it is built for, and that the float64 restatement does not share the kernel's chunk logic as a blind spot."""
import itertools

import numpy as np
import pytest

from egc_amd import _C
from gat_ref import CHUNK, SHAPES, SWEEP_SHAPES, aggregate_forward, datt_partials, geometry, rel_out, sweep_graph, sweep_inputs


def test_the_table_holds_the_shapes_it_was_set_up_with():
    assert len(set(SWEEP_SHAPES)) == len(SWEEP_SHAPES) and all(1 <= h * c <= 512 for h, c in SWEEP_SHAPES)
    one = {(1, 1), (4, 1), (1, 3), (1, 4), (1, 5), (2, 3), (4, 2), (3, 3), (16, 2), (7, 3), (12, 5), (9, 7), (1, 64), (3, 43), (5, 50),
           (85, 3), (64, 4), (4, 64), (1, 256)}
    two = {(1, 257), (1, 260), (3, 100), (8, 33), (37, 13), (2, 256), (1, 512), (128, 4), (128, 3), (170, 3), (256, 2), (512, 1)}
    assert one | two <= set(SWEEP_SHAPES)
    assert all(geometry(*s)["S"] == 1 for s in one) and all(geometry(*s)["S"] == 2 for s in two)


def test_the_table_covers_every_instance_group_size_and_the_slot_boundary():
    geoms = {s: geometry(*s) for s in SWEEP_SHAPES}
    triples = {(g["S"], g["vec_by_width"], g["small"]) for g in geoms.values()}
    assert triples == set(itertools.product((1, 2), (True, False), (True, False)))
    groups = {g["G"] for g in geoms.values()}
    assert groups == {1, 2, 4, 8, 16, 64}                                        # no sweep shape has 17 .. 32 lanes ...
    assert groups | {geometry(*s)["G"] for s in SHAPES.values()} == {1, 2, 4, 8, 16, 32, 64}   # ... the fixtures' 104 and 112 do
    assert all(g["V"] == g["S"] * g["G"] and (g["S"] == 1 or g["G"] == 64) for g in geoms.values())
    assert max(g["seg"] for g in geoms.values()) > 64 and geometry(1, 512)["seg"] == 129
    assert sum(g["spans_256"] for g in geoms.values()) >= 3 and sum(g["boundary_256"] for g in geoms.values()) >= 1
    assert not any(g["spans_256"] and g["boundary_256"] for g in geoms.values())
    assert not any(g["spans_256"] or g["boundary_256"] for g in geoms.values() if g["S"] == 1)
    for s in (1, 2):
        assert {c for (h, c), g in geoms.items() if g["small"] and g["S"] == s} == {1, 2, 3}
    # the heads the table's comments name
    for (h, c), head in (((3, 100), 2), ((8, 33), 7), ((37, 13), 19), ((128, 3), 85)):
        assert head < h and head * c < 256 < (head + 1) * c and geoms[(h, c)]["spans_256"]
    assert geoms[(2, 256)]["boundary_256"] and geoms[(37, 13)]["vec_by_width"] is False and geoms[(128, 3)]["vec_by_width"] is True
    # padding lanes: 129 columns on 64 lanes, 9 columns on 4
    assert geoms[(3, 43)]["G"] == 64 and -(-129 // 4) == 33 and geoms[(3, 3)]["G"] == 4


@pytest.mark.parametrize("shape", SWEEP_SHAPES + tuple(sorted(set(SHAPES.values()))), ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry_agrees_with_the_library(shape):
    """1,000 entries are 4 chunk slots of V virtual lanes with three 16-byte values (m, l, acc) each."""
    h, c = shape
    assert _C.load().egc_gatv2_forward_workspace_bytes(1000, h, c) == 4 * geometry(h, c)["V"] * 48


def test_the_sweep_graph_has_the_rows_it_is_built_for():
    for n in (40, 300):
        ei, n_ = sweep_graph(5, n)
        assert n_ == n and ei.dtype == np.int64 and ei.shape == (2, 1234) and ei.min() >= 0 and ei.max() < n - 3
        indeg, outdeg = np.bincount(ei[1], minlength=n), np.bincount(ei[0], minlength=n)
        assert indeg.max() == 2 * CHUNK + 9 == outdeg.max()                      # two full chunks and a tail of 9, both ways
        assert int((indeg == 0).sum()) >= 3 and int((indeg[n - 3:] + outdeg[n - 3:]).sum()) == 0
        assert int((ei[0] == ei[1]).sum()) >= 9
        pairs = ei[0] * n + ei[1]
        assert len(pairs) - len(np.unique(pairs)) >= 20
        # shuffled: the long row's entries are not one run of the edge list
        at = np.nonzero(ei[1] == indeg.argmax())[0]
        assert at.max() - at.min() > len(at)
        # a skipped entry (source == row) inside a chunked row when self loops are added
        if n == 40:
            assert int((ei[0][ei[1] == indeg.argmax()] == indeg.argmax()).sum()) >= 1
    a, b = sweep_graph(5), sweep_graph(5)
    assert np.array_equal(a[0], b[0]) and not np.array_equal(a[0], sweep_graph(6)[0])


def test_the_two_level_sum_case_has_more_than_64_partials():
    ei, n = sweep_graph(5, 300)
    assert datt_partials(3, 43, n, ei.shape[1]) == 75 + 2 > 64                   # G 64: 4 rows a workgroup, 5 slots in 2
    assert datt_partials(1, 3, n, ei.shape[1]) == 2 + 1                           # G 1: 256 rows a workgroup
    assert datt_partials(2, 4, 700, CHUNK) == -(-700 // 128)                      # no row can be longer than a chunk


def test_sweep_inputs():
    xl, xr, gout, att = sweep_inputs(3, 43, 40, 7)
    assert xl.shape == xr.shape == gout.shape == (40, 129) and att.shape == (3, 43)
    assert all(a.dtype == np.float32 for a in (xl, xr, gout, att))
    assert not np.array_equal(xl, xr) and np.array_equal(xl, sweep_inputs(3, 43, 40, 7)[0])


@pytest.mark.parametrize("shape", ((12, 5), (7, 3), (3, 100), (128, 3)), ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("loops", (True, False))
def test_restatement_without_chunks_or_batches_is_the_same_beyond_rounding(shape, loops):
    """One shape per (S, small) pair: the float64 truth of the sweep does not hinge on the chunk and batch cuts it shares with
    the kernel."""
    h, c = shape
    g = geometry(h, c)
    assert (g["S"], g["small"]) == {(12, 5): (1, False), (7, 3): (1, True), (3, 100): (2, False), (128, 3): (2, True)}[shape]
    ei, n = sweep_graph(5)
    xl, xr, _, att = sweep_inputs(h, c, n, 7)
    a, la = aggregate_forward(xl, xr, att, ei, loops=loops)
    b, lb = aggregate_forward(xl, xr, att, ei, loops=loops, chunk=10 ** 9, ahead=1)
    fin = np.isfinite(la)
    assert np.array_equal(fin, np.isfinite(lb)) and (loops or int((~fin).sum()) >= 3 * h)
    assert rel_out(a, b) <= 1e-12 and rel_out(la[fin], lb[fin]) <= 1e-12
