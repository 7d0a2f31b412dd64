"""The geometry table, the row ladders and the ties inputs behind tests/test_softmax_shapes_gpu.py, without a GPU
(tests/softmax_ref.py: CELLS, GEOMETRIES, WIDE_PADDING, LADDER_*, FINALIZE_*, ties_logits).  This guards the INPUTS, not the
kernels: the lane rule of include/egc_hip.h is restated here and the table is held against it -- every (lanes, pieces)
cell of the launcher in all three forms, the zero-fill loop of both store forms with several trips, row counts on, before
and after a chunk edge, one to three trips of the finalize loop, inputs that do tie."""
import re
from pathlib import Path

import pytest

import softmax_ref as ref

HEADER = (Path(__file__).resolve().parent.parent / "include" / "egc_hip.h").read_text()


def lane_shape(n_classes):
    """(gl, K) of include/egc_hip.h: G = 2^gl the power of two >= ceil(n_classes / 4), 64 at the most; K = ceil(n_classes / (4 G))."""
    q = -(-n_classes // 4)
    gl = 0
    while (1 << gl) < q and gl < 6:
        gl += 1
    return gl, -(-q // (1 << gl))


def forms(c, ld):
    """Which form (True: 16-byte accesses) each kernel takes for aligned pointers: log-softmax forward / backward need
    n_classes % 4 == 0 as well (their [N, n_classes] operand), the NLL pair the row stride alone."""
    return {"log_softmax": ld % 4 == 0 and c % 4 == 0, "nll": ld % 4 == 0}


def zero_fill_trips(c, ld, vec):
    """Trips of lane 0 through the loop that zero-fills columns [4 K G, ld) of a gradient row."""
    gl, k = lane_shape(c)
    g = 1 << gl
    first, step = 4 * k * g, (4 * g if vec else g)
    return len(range(first, ld, step))


def test_the_header_states_the_rule_restated_here():
    assert "#define EGC_SOFTMAX_MAX_CLASSES 1024" in HEADER
    text = re.sub(r"[\s*]+", " ", HEADER)
    assert "rows are cut into chunks of 128" in text and "chunk sums t, t + 256, ... ascending" in text
    assert "128 G / 256 + 9 + ceil(chunks / 256) + 9" in text
    assert ref.SM_CHUNK == 128 and ref.SM_BLOCK == 256
    # the cells tile 1 .. 1024 and every class count inside a cell has the cell's (gl, K)
    want = [(gl, 1) for gl in range(6)] + [(6, k) for k in (1, 2, 3, 4)]
    assert len(ref.CELLS) == 10 and ref.CELLS[0][0] == 1 and ref.CELLS[-1][1] == 1024
    for (lo, hi), (lo2, _), cell in zip(ref.CELLS, ref.CELLS[1:] + [(1025, None)], want):
        assert lo2 == hi + 1
        assert {lane_shape(c) for c in range(lo, hi + 1)} == {cell}, (lo, hi)
    assert [lo for lo, _ in ref.CELLS] == [1, 5, 9, 17, 33, 65, 129, 257, 513, 769]
    assert [hi for _, hi in ref.CELLS] == [4, 8, 16, 32, 64, 128, 256, 512, 768, 1024]


def test_every_cell_is_reached_in_all_three_forms():
    assert all(lo % 4 == 1 and hi % 4 == 0 for lo, hi in ref.CELLS)
    seen = {}
    for c, ld in ref.GEOMETRIES:
        assert 1 <= c <= ld <= 1024
        f = forms(c, ld)
        seen.setdefault(lane_shape(c), set()).add((f["log_softmax"], f["nll"]))
    assert len(seen) == 10
    for cell, got in seen.items():
        assert {(True, True), (False, True), (False, False)} <= got, cell
    for lo, hi in ref.CELLS:
        a, b, c = ref.cell_geometries(lo, hi)
        assert forms(*a) == {"log_softmax": True, "nll": True}
        assert forms(*b) == {"log_softmax": False, "nll": True} and b[1] - b[0] == 3     # the last piece straddles n_classes
        assert forms(*c) == {"log_softmax": False, "nll": False} and c[0] == c[1]
        assert all(g in ref.GEOMETRIES for g in (a, b, c))
    assert all(lane_shape(c)[1] == 3 for c, _ in ref.cell_geometries(513, 768))         # the K = 3 kernels


def test_the_zero_fill_loop_runs_several_trips_in_both_forms():
    trips = {(c, ld): zero_fill_trips(c, ld, ld % 4 == 0) for c, ld in ref.WIDE_PADDING}
    assert trips[(10, 64)] == 3 and trips[(10, 63)] == 12
    assert {ld % 4 == 0 for _, ld in ref.WIDE_PADDING} == {True, False}
    for vec in (True, False):
        assert sum(1 for (c, ld), t in trips.items() if (ld % 4 == 0) == vec and t >= 2) >= 1
    assert trips[(40, 128)] == 1 and trips[(349, 1024)] == 2                          # (one trip in each of (40, 128)'s 16 lanes)
    # nothing in the cells' own geometries does: that is what the wide rows are for
    assert all(zero_fill_trips(c, ld, ld % 4 == 0) == 0 for lo, hi in ref.CELLS for c, ld in ref.cell_geometries(lo, hi))
    assert all(g in ref.GEOMETRIES for g in ref.WIDE_PADDING)


def test_the_row_ladders_sit_on_the_chunk_and_finalize_edges():
    chunk = ref.SM_CHUNK
    assert ref.SWEEP_ROWS // chunk == 2 and ref.SWEEP_ROWS % chunk not in (0, 1, chunk - 1)
    for edge in (chunk, 2 * chunk):
        assert {edge - 1, edge, edge + 1} <= set(ref.LADDER_ROWS)
    assert 1 in ref.LADDER_ROWS
    assert [1 << lane_shape(c)[0] for c, _ in ref.LADDER_GEOMETRIES] == [1, 16, 64]
    assert ref.SM_BLOCK >> lane_shape(ref.LADDER_GEOMETRIES[0][0])[0] > chunk        # G = 1: more groups than rows of a chunk
    trips = [-(-(-(-n // chunk)) // ref.SM_BLOCK) for n in ref.FINALIZE_ROWS]
    assert trips == [1, 2, 3]
    c, ld = ref.FINALIZE_GEOMETRY
    assert max(ref.FINALIZE_ROWS) * ld * 4 <= 1.01 * 2 ** 20


@pytest.mark.parametrize("lo, hi", ref.CELLS)
def test_the_ties_inputs_tie(lo, hi):
    for c, ld in ref.cell_geometries(lo, hi):
        x = ref.ties_logits(ref.SWEEP_ROWS, c, ld, seed=c)
        assert bool((x[:, :c] == x[:, :c].round()).all()) and bool(x[:, c:].isnan().all())
        share = ref.tied_share(x, c)
        print(f"C={c} ld={ld}: {share:.3f} of the rows have their maximum twice or more")
        if c >= 4:
            assert share >= 0.5, (c, share)
        # the reference alone: the arg-max is a maximal column and no column before it is maximal
        arg = ref.first_argmax(x, c)
        v = x[:, :c]
        m = v.max(dim=1).values
        assert bool((v[range(v.size(0)), arg] == m).all())
        before = (v == m[:, None]) & (ref.torch.arange(c)[None, :] < arg[:, None])
        assert not before.any()
        if c == 1:
            assert not arg.any()


def test_loss_chain_agrees_with_the_restated_lane_rule():
    for c in (1, 4, 5, 10, 40, 61, 128, 129, 349, 513, 768, 1024):
        g = 1 << lane_shape(c)[0]
        for n in ref.LADDER_ROWS + ref.FINALIZE_ROWS + [ref.SWEEP_ROWS]:
            chunks = -(-n // ref.SM_CHUNK)
            assert ref.loss_chain(n, c) == max(ref.SM_CHUNK * g // ref.SM_BLOCK, 1) + 9 + -(-chunks // ref.SM_BLOCK) + 9


def test_the_unaligned_geometries_are_vector_eligible():
    assert all(forms(c, ld)["nll"] for c, ld in ref.UNALIGNED_GEOMETRIES)
    assert sum(forms(c, ld)["log_softmax"] for c, ld in ref.UNALIGNED_GEOMETRIES) >= 2
    assert {lane_shape(c) for c, _ in ref.UNALIGNED_GEOMETRIES} == {(4, 1), (6, 2), (6, 3)}
