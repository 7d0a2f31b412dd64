"""The restated summation order, the width and table lists and the crafted chunks behind tests/test_encoder_shapes_gpu.py,
without a GPU (tests/encoder_ref.py: chunked_backward, SWEEP_*, sweep_tables, ladder_indices, *_LADDER).  This guards the
INPUTS and the REFERENCE, not the kernels: that the chunked order is a reordering of the float64 sum and nothing else, that
without chunks it is the plain loop to the bit and with chunks it is not, that the widths reach every lane count the
launchers distinguish in both forms, that the table counts sit on the forward's batch of four and on the limit, and that
the crafted chunks hold the list lengths they claim."""
import re
from pathlib import Path

import torch

import encoder_ref as ref
from egc_amd import _C

ROOT = Path(__file__).resolve().parent.parent
HEADER = re.sub(r"[\s*]+", " ", (ROOT / "include" / "egc_hip.h").read_text())


def test_the_header_states_the_order_restated_here():
    assert "nodes are cut into chunks of 256; inside a chunk the rows of one destination are added in ascending n" in HEADER
    assert "chunk sums are added in ascending chunk order" in HEADER
    assert _C.ENCODER_MAX_TABLES == 16 and _C.ENCODER_MAX_WIDTH == 1024
    assert ref.ENC_CHUNK == 256 and max(ref.SWEEP_TABLE_COUNTS) == 16 and max(ref.SWEEP_WIDTHS) == 1024


def _case(n, rows, seed, width=5):
    g = torch.Generator().manual_seed(seed)
    idx = torch.stack([torch.randint(0, r, (n,), generator=g) for r in rows], dim=1)
    return idx, torch.randn(n, width, generator=g)


def test_float64_chunked_order_is_a_reordering_of_the_float64_sum():
    """Only the order differs: per element |chunked64 - index_add64| <= k 2^-53 sum |g|, k the list's length and 2^-53 the
    unit roundoff of float64 (each side is a float64 sum of the same k terms in its own order)."""
    rows, clamp = [2, 7, 300, 40], [None, None, None, 30]
    idx, g = _case(3000, rows, 1)
    idx[:, 3] = torch.randint(0, 80, (3000,), generator=torch.Generator().manual_seed(2))      # beyond the clamp
    idx[5, 0], idx[9, 1] = -1, 7                                                               # outside their tables
    got = ref.chunked_backward(g, idx, rows, clamp, chunk=256, dtype=torch.float64)
    for d, (s, a, k) in zip(got, ref.backward(g, idx, rows, clamp)):
        assert d.dtype == torch.float64 and d.shape == s.shape
        bound = k.double()[:, None] * 2.0 ** -53 * a
        assert bool(((d - s).abs() <= bound).all())
        assert bool((d[k == 0] == 0).all()) and torch.equal(d[k == 1], s[k == 1])


def test_without_chunks_it_is_the_plain_loop_and_with_chunks_it_is_not():
    rows, clamp = [2, 7, 300], [None, 5, None]
    idx, g = _case(1500, rows, 3)
    idx[11, 2] = 300
    plain = ref.sequential_backward(g, idx, rows, clamp)
    whole = ref.chunked_backward(g, idx, rows, clamp, chunk=10 ** 9)
    chunked = ref.chunked_backward(g, idx, rows, clamp, chunk=256)
    assert all(torch.equal(a, b) and a.dtype == torch.float32 for a, b in zip(whole, plain))
    assert not torch.equal(chunked[0], plain[0]) and not torch.equal(chunked[1], plain[1])      # lists across chunks: another order
    # ... the same sums nevertheless, each within the any-order bound of the float64 reference
    for d, (s, a, k) in zip(chunked, ref.backward(g, idx, rows, clamp)):
        assert bool(((d.double() - s).abs() <= ref.gamma((k - 1).clamp(min=0))[:, None] * a).all())
    # one chunk's worth of nodes: nothing to reorder
    for a, b in zip(ref.chunked_backward(g[:256], idx[:256], rows, clamp), ref.sequential_backward(g[:256], idx[:256], rows, clamp)):
        assert torch.equal(a, b)
    # a chunk of another size is another order again: the chunk size is part of what is restated
    assert not torch.equal(ref.chunked_backward(g, idx, rows, clamp, chunk=128)[0], chunked[0])


def test_a_lost_doubled_or_misfiled_row_is_seen():
    """What the any-order bound lets through in a long list, bit equality does not."""
    rows = [2, 4]
    idx, g = _case(ref.SWEEP_NODES, rows, 4)
    want = ref.chunked_backward(g, idx, rows)
    lost = g.clone(); lost[300] = 0
    moved = idx.clone(); moved[300, 0] ^= 1
    for other in (ref.chunked_backward(lost, idx, rows), ref.chunked_backward(torch.cat([g, g[300:301]]), torch.cat([idx, idx[300:301]]), rows),
                  ref.chunked_backward(g, moved, rows)):
        assert not torch.equal(other[0], want[0])


def test_the_widths_reach_every_lane_count_in_both_forms():
    lanes = {w: (w + 3) // 4 for w in ref.SWEEP_WIDTHS}
    assert {1, 2, 64, 65, 128, 129, 256} <= set(lanes.values()) and max(lanes.values()) == 256
    for side in (lambda n: n < 64, lambda n: n > 64):
        assert {w % 4 == 0 for w, n in lanes.items() if side(n)} == {True, False}
    for n in (1, 2, 64, 128, 256):                     # both forms at the lane counts that have a multiple-of-4 width
        assert {w % 4 == 0 for w, m in lanes.items() if m == n} == {True, False}, n
    assert {w for w, n in lanes.items() if n == 1} == {1, 2, 3, 4}
    # nodes per workgroup of the forward (256 / lanes): many, two, one
    assert {256 // lanes[w] for w in (509, 512)} == {2} and {256 // lanes[w] for w in (513, 1021, 1024)} == {1}
    assert all(w % 4 for w in (77, 255, 257, 509, 513, 1021)) and set(ref.T_SWEEP_WIDTHS) == {256, 77}


def test_the_table_counts_and_rows():
    counts = ref.SWEEP_TABLE_COUNTS
    assert {t % ref.ENC_FWD_BATCH for t in counts} >= {0, 1} and {1, 4, 5, 8, 9, 16} <= set(counts)
    cases = ref.sweep_cases()
    assert len(cases) == len(set(cases))
    for w in ref.SWEEP_WIDTHS:
        assert {(w, 9, "uniform"), (w, 9, "skewed")} <= set(cases)
    for t in counts:
        assert {w % 4 == 0 for w, tt, _ in cases if tt == t} == {True, False}
    seen = set()
    for t in counts:
        rows, clamp, beyond = ref.sweep_tables(t)
        assert len(rows) == t and set(rows) <= set(ref.ROW_EDGES)
        seen |= set(rows)
        assert (sum(c is not None for c in clamp) == 1) == (t >= 3)
        if t >= 3:
            assert clamp[-1] == rows[-1] - 1 and beyond[-1] > rows[-1]
            idx = ref.sweep_indices(ref.SWEEP_NODES, rows, "uniform", 1, beyond)
            assert int(idx[:, -1].max()) > clamp[-1]                                   # indices beyond the clamp are in the input
            assert bool(ref.keys(idx, rows, clamp)[1].all())                           # and none is outside after it
    assert seen == set(ref.ROW_EDGES) and set(ref.sweep_tables(9)[0]) == set(ref.ROW_EDGES)
    assert ref.SWEEP_NODES == 2 * ref.ENC_CHUNK + 88
    skew = ref.sweep_indices(ref.SWEEP_NODES, [600, 1], "skewed", 1)
    assert skew[:, 0].unique().numel() == 1 and skew[:, 1].unique().tolist() == [0]


def _list_lengths(col, lo, hi):
    return sorted(torch.bincount(col[lo:hi]).tolist())


def test_the_crafted_chunks_hold_the_stated_lists():
    idx = ref.ladder_indices()
    assert idx.shape == (ref.SWEEP_NODES, 2) and idx.dtype == torch.int64
    rest = ref.ENC_CHUNK - sum(ref.LADDER_LENGTHS)
    assert rest == 183 and _list_lengths(idx[:, 0], 0, 256) == sorted(ref.LADDER_LENGTHS + (rest,))
    assert {n - ref.ENC_RD_AHEAD for n in (7, 8, 9)} == {-1, 0, 1} and {n - 2 * ref.ENC_RD_AHEAD for n in (15, 16, 17)} == {-1, 0, 1}
    # no list of more than one node is a contiguous run: the lists are found by key, not by position
    for v in range(8):
        pos = torch.nonzero(idx[:256, 0] == v).view(-1)
        assert pos.numel() == 1 or int(pos[-1] - pos[0]) >= pos.numel()
    assert idx[256:512, 0].unique().tolist() == [4]                                     # all 256 nodes share a key
    assert int(idx[:, 0].max()) < ref.LADDER_ROWS[0] - 1                                # the last row is indexed by nobody
    assert int(idx[:, 1].max()) < ref.LADDER_ROWS[1]
    assert torch.equal(idx, ref.ladder_indices())


def test_the_node_and_chunk_ladders():
    c, a = ref.ENC_CHUNK, ref.ENC_RD_AHEAD
    for edge in (c, 2 * c):
        assert {edge - 1, edge, edge + 1} <= set(ref.NODE_LADDER)
    assert 1 in ref.NODE_LADDER
    chunks = [-(-n // c) for n in ref.CHUNK_LADDER]
    assert {a - 1, a, a + 1, 2 * a, 2 * a + 1} <= set(chunks)
    assert sum(n % c != 0 for n in ref.CHUNK_LADDER) == 1                               # one ragged last chunk
    assert ref.LADDER_WIDTH % 4 == 0 and (ref.LADDER_WIDTH + 3) // 4 == 2
    # the two-row table meets every chunk; the 600-row table's rows miss most of them
    n = max(ref.CHUNK_LADDER)
    idx = ref.sweep_indices(n, ref.NODE_LADDER_ROWS, "uniform", 1)
    per_chunk = [set(idx[i:i + c, 0].tolist()) for i in range(0, n, c)]
    assert all(s == {0, 1} for s in per_chunk)
    met = torch.zeros(600, len(per_chunk), dtype=torch.bool)
    met[idx[:, 2], torch.arange(n) // c] = True
    assert 0.2 < float(met.float().mean()) < 0.5
