"""The sweep graph, the width table and the restatements behind tests/test_mpnn_shapes_gpu.py and tests/test_typed_mean_shapes_gpu.py,
without a GPU (tests/mpnn_ref.py: ladder_graph, ladder_inputs, WIDTHS, message_forward, message_backward).  This guards the INPUTS,
not the kernels: that the graph has one row of every ladder length, that its long rows start where the chunk kernels' slot
arithmetic has its edges, that the widths reach every lane-group size the launchers distinguish, that the ``ties`` inputs do tie,
and that the chunked order of the restatement is a reordering of the plain one and nothing else."""
import functools

import numpy as np
import pytest

from egc_amd import _C
from mpnn_ref import (CASES, CHUNK, FILL, LADDER, PAD, WIDTHS, csr_by_destination, ladder_graph, ladder_inputs, ladder_lengths,
                      load_mpnn_golden, message_backward, message_forward, rel_grad, rel_out, tie_counts)

SEED = 11
VARIANTS = (dict(), dict(tail_empty=True), dict(pad_to_chunk=True), dict(square=True), dict(tail_empty=True, square=True))


def test_the_ladder_is_the_list_the_kernels_are_read_against():
    assert _C.load().egc_typed_mean_chunk() == CHUNK
    assert LADDER == (0, 1, 7, 8, 9, 15, 16, 17, 255, 256, 257, 511, 512, 513, 768, 530)
    assert PAD not in LADDER and FILL not in LADDER and PAD != FILL and PAD < CHUNK


def _rows(ei, n_dst, n_src, flip):
    """(rowptr of the side that carries the ladder, its row count, the other side's)"""
    if flip:
        ei, n_dst, n_src = ei[::-1], n_src, n_dst
    return csr_by_destination(ei, n_dst)[0], n_dst, n_src


@pytest.mark.parametrize("flip", (False, True))
@pytest.mark.parametrize("kw", VARIANTS, ids=lambda kw: "-".join(kw) or "default")
def test_every_length_once_and_every_placement(kw, flip):
    ei, n_dst, n_src = ladder_graph(SEED, flip=flip, **kw)
    assert ei.dtype == np.int64 and ei.shape[0] == 2 and ei.flags["C_CONTIGUOUS"]
    assert 0 <= ei[0].min() and ei[0].max() < n_src and 0 <= ei[1].min() and ei[1].max() < n_dst
    rowptr, n_lad, n_other = _rows(ei, n_dst, n_src, flip)
    length, start = np.diff(rowptr), rowptr[:-1]
    tail = 3 if kw.get("tail_empty") else 0
    assert n_lad < 100 and 5500 <= ei.shape[1] <= 6500
    assert n_other == (n_lad if kw.get("square") else (3 * n_lad) // 2)
    # one row of every ladder length (the three appended rows aside); everything else is padding of one fixed length
    body = length[:n_lad - tail]
    assert int(length[n_lad - tail:].sum()) == 0
    for want in LADDER:
        assert int((body == want).sum()) == 1, want
    other = sorted(set(body.tolist()) - set(LADDER))
    assert other == ([FILL, PAD] if kw.get("pad_to_chunk") else [PAD])
    assert int((body == FILL).sum()) == (1 if kw.get("pad_to_chunk") else 0)
    # the placement conditions
    long_rows = np.nonzero(length > CHUNK)[0]
    assert sorted(length[long_rows].tolist()) == sorted(x for x in LADDER if x > CHUNK) and len(long_rows) == 6
    assert long_rows[0] == 0                                                     # row 0 is long
    assert long_rows[-1] == n_lad - 1 - tail                                     # the last row (before the empty tail) is long
    if tail:
        assert rowptr[-1] == rowptr[-4] == ei.shape[1]                           # the bisection must still pick the long row
    residue = {int(start[r] % CHUNK) for r in long_rows if start[r] > 0}
    assert {0, 1, CHUNK - 1} <= residue                                          # on a slot boundary, one past, one before
    assert sum(int(b - a == 1) for a, b in zip(long_rows, long_rows[1:])) >= 2   # adjacent long rows, twice
    assert any(length[r] == 0 and length[r - 1] > 0 and length[r + 1] > 0 for r in range(1, n_lad - 1))
    assert (ei.shape[1] % CHUNK == 0) == bool(kw.get("pad_to_chunk"))
    # a row of exactly 2 CHUNK entries whose every chunk starts on a slot boundary, followed by a long row on one
    r = int(np.nonzero(length == 2 * CHUNK)[0][0])
    assert start[r] % CHUNK == 0 and start[r] > 0 and length[r + 1] > CHUNK
    # permuted (the ladder side is not sorted in the edge list), with self loops and duplicates
    side = ei[0] if flip else ei[1]
    assert int((np.diff(side) < 0).sum()) > ei.shape[1] // 4
    assert int((ei[0] == ei[1]).sum()) >= 5
    pairs = ei[0] * max(n_dst, n_src) + ei[1]
    assert len(pairs) - len(np.unique(pairs)) >= 100
    # the other side has more than a chunk of entries and no long row: chunk groups that all return early
    assert np.bincount(ei[1] if flip else ei[0], minlength=n_other).max() <= CHUNK


def test_flip_is_the_same_edge_list_with_its_rows_swapped():
    a, b = ladder_graph(SEED), ladder_graph(SEED, flip=True)
    assert np.array_equal(a[0][::-1], b[0]) and a[1:] == b[1:][::-1]
    assert np.array_equal(ladder_graph(SEED)[0], a[0]) and not np.array_equal(ladder_graph(SEED + 1)[0], a[0])


def test_the_reduced_and_the_shifted_graph():
    cut = ladder_lengths(max_len=2 * CHUNK + 1)
    assert max(cut) == 2 * CHUNK + 1 and sorted(set(LADDER) - set(cut)) == [2 * CHUNK + 18, 3 * CHUNK] and cut[0] > CHUNK
    assert sum(1 for x in cut if x > CHUNK) == 4
    shifted = ladder_lengths(prepend=300)
    assert shifted[:300] == [1] * 300 and shifted[300:] == ladder_lengths()
    # the long rows' first partial slot moves and their groups leave the first workgroup at every width of the test
    assert 300 % CHUNK != 0 and 300 * 2 > 256
    ei, n_dst, n_src = ladder_graph(SEED, prepend=300)
    assert (n_dst, n_src) == (386, 579) and ei.shape[1] == sum(shifted)


def test_the_width_table_reaches_every_lane_group_size():
    lanes = {w: (w + 3) // 4 for w in WIDTHS + (8, 6)}
    assert len(set(WIDTHS)) == len(WIDTHS) == 14
    assert 1 in lanes.values()
    assert any(2 <= n <= 63 and 256 % n != 0 for n in lanes.values())
    assert {64, 65, 257} <= set(lanes.values())
    for side in (lambda n: n < 64, lambda n: n > 64):
        assert {w % 4 == 0 for w, n in lanes.items() if side(n)} == {True, False}
    assert {w for w in WIDTHS if lanes[w] == 1} == {1, 2, 3, 4}                    # one lane, three to no dead columns
    assert lanes[1030] > 257 and 1030 % 4 != 0                                    # wider than a workgroup on the 4-byte path
    assert lanes[8] == lanes[6] == 2 and 6 % 4 != 0


@functools.lru_cache(maxsize=None)
def _restated(flip, aggr, chunk, ties=False):
    ei, n_dst, n_src = ladder_graph(SEED, flip=flip)
    P, Q, dm = ladder_inputs(n_dst, n_src, 5, SEED + 1, ties=ties)
    m, arg = message_forward(P, Q, ei, aggr, chunk, np.float64)
    return (m, arg) + message_backward(dm, ei, aggr, arg, chunk, np.float64, n_src=n_src)


@pytest.mark.parametrize("flip", (False, True))
@pytest.mark.parametrize("aggr", ("add", "mean", "max"))
def test_the_chunked_order_is_a_reordering_and_nothing_else(aggr, flip):
    """float64, chunk = CHUNK against no chunking at all: 1e-12 relative, the max argument identical."""
    a, b = _restated(flip, aggr, CHUNK), _restated(flip, aggr, 10 ** 9)
    assert rel_out(a[0], b[0]) <= 1e-12 and rel_grad(a[2], b[2]) <= 1e-12 and rel_grad(a[3], b[3]) <= 1e-12
    if aggr == "max":
        assert np.array_equal(a[1], b[1]) and a[1].dtype == np.int32
        assert np.array_equal(_restated(flip, aggr, CHUNK, True)[1], _restated(flip, aggr, 10 ** 9, True)[1])
    else:
        assert a[1] is None
        if flip and aggr == "add":                                               # ... and in float32 it IS another order
            ei, n_dst, n_src = ladder_graph(SEED, flip=True)
            dm = ladder_inputs(n_dst, n_src, 5, SEED + 1)[2]
            assert not np.array_equal(message_backward(dm, ei, aggr, n_src=n_src)[0], message_backward(dm, ei, aggr, chunk=10 ** 9, n_src=n_src)[0])
    ei, n_dst, n_src = ladder_graph(SEED, flip=flip)
    assert a[0].shape == (n_dst, 5) == a[3].shape and a[2].shape == (n_src, 5)


@pytest.mark.parametrize("flip", (False, True))
def test_ties_inputs_tie_between_edges_and_between_chunks(flip):
    ei, n_dst, n_src = ladder_graph(SEED, flip=flip)
    P = ladder_inputs(n_dst, n_src, 8, SEED + 1, ties=True)[0]
    assert np.array_equal(P, np.round(P)) and P.dtype == np.float32
    edges, chunks = tie_counts(P, ei, n_dst)
    print(f"flip {int(flip)}: {edges} maxima tied between edges, {chunks} between chunks of one row")
    assert edges > 0 and (chunks > 0) == (not flip)                              # only the ladder side has chunked rows
    # and the winner is the first: the argument's edge precedes, in the edge list, every other edge of its row that ties
    m, arg = message_forward(P, np.zeros((n_dst, 8), np.float32), ei, "max")
    for row, c in ((0, 0), (n_dst - 1, 7), (n_dst // 2, 3)):
        if arg[row, c] < 0:
            continue
        tied = np.nonzero((ei[1] == row) & (P[ei[0], c] == m[row, c]))[0]
        assert arg[row, c] == tied.min() and ei[1][arg[row, c]] == row
    plain = ladder_inputs(n_dst, n_src, 8, SEED + 1)[0]
    assert tie_counts(plain, ei, n_dst)[0] < edges                               # (normals tie through duplicate edges only)


@pytest.mark.parametrize("name", CASES)
def test_the_rectangular_extension_keeps_the_square_bits(name):
    """On the fixtures' square graphs: n_src given equals n_src left out; unused extra rows of P change nothing and get a zero
    d P; the chunked max walk gives the bits and the argument of the plain first-entry walk."""
    g = load_mpnn_golden(name)
    ei, n, aggr = g["ei"], g["meta"]["n"], g["meta"]["aggr"]
    rng = np.random.default_rng(5)
    P, Q, dm = (rng.standard_normal((n, 4)).astype(np.float32) for _ in range(3))
    m, arg = message_forward(P, Q, ei, aggr)
    dP, dQ = message_backward(dm, ei, aggr, arg)
    assert m.dtype == dP.dtype == dQ.dtype == np.float32 and dP.shape == dQ.shape == (n, 4)
    dP2, dQ2 = message_backward(dm, ei, aggr, arg, n_src=n)
    assert np.array_equal(dP, dP2) and np.array_equal(dQ, dQ2)
    m3, arg3 = message_forward(np.concatenate([P, P[:7] + 1]), Q, ei, aggr)
    dP3, dQ3 = message_backward(dm, ei, aggr, arg, n_src=n + 7)
    assert np.array_equal(m, m3) and np.array_equal(dQ, dQ3) and np.array_equal(dP, dP3[:n]) and not dP3[n:].any()
    if aggr == "max":
        m1, arg1 = message_forward(P, Q, ei, aggr, chunk=10 ** 9)
        assert np.array_equal(arg, arg3) and np.array_equal(arg, arg1) and np.array_equal(m, m1)
        src, dst = ei
        for row in (0, n // 2, int(np.bincount(dst, minlength=n).argmax())):     # the plain definition, straight from the edge list
            e = np.nonzero(dst == row)[0]
            if len(e):
                assert np.array_equal(arg[row], e[np.argmax(P[src[e]], axis=0)])
