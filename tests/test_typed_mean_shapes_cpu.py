"""The general typed-mean restatement (tests/rgcn_ref.py: typed_mean_restated) and the inputs of tests/test_typed_mean_shapes_gpu.py
without a GPU: the restatement reproduces ``chunked_row_mean`` on the layer fixtures, its chunked order is a reordering of the
plain one and nothing else, its scale is a reciprocal and a multiply, its accumulation runs in list order, and the launch of eight
relations holds the mix of relations it is built for."""
import numpy as np
import pytest

from egc_amd import _C
from rgcn_ref import (CHUNK, EIGHT_ROWS, LAYER_FIXTURES, RelSpec, chunked_row_mean, csr_by_destination, eight_relations, ladder_graph,
                      ladder_inputs, load_rgcn_golden, rel_grad, rel_out, transposed_csr, typed_mean_restated, typed_operands)

SEED = 11


def test_constants():
    assert _C.load().egc_typed_mean_chunk() == CHUNK and _C.TYPED_MAX_RELATIONS == 8 == len(eight_relations(SEED, 4))


@pytest.mark.parametrize("name", LAYER_FIXTURES)
def test_restatement_reproduces_chunked_row_mean_on_the_layer_fixtures(name):
    """[x_t | mean_1 | ...] of every node type as ONE restated launch (identity + the relations, own column blocks) against the
    operands assembled from chunked_row_mean, bit for bit in float32, long row included."""
    g = load_rgcn_golden(name)
    want, blocks = typed_operands(g["x"], g["ei"], g["meta"]["edge_types"], CHUNK, np.float32)
    width = g["meta"]["fin"]
    longest = 0
    for t, xt in g["x"].items():
        rels = [RelSpec(None, xt)]
        for j, k in enumerate(blocks[t]):
            csr = csr_by_destination(g["ei"][k], xt.shape[0])
            longest = max(longest, int(np.diff(csr[0]).max()))
            rels.append(RelSpec(csr, g["x"][k[0]], post_mean=True, out_col=(1 + j) * width))
            one = typed_mean_restated([rels[-1]._replace(out_col=0)], xt.shape[0], width)
            assert np.array_equal(one, chunked_row_mean(g["x"][k[0]], g["ei"][k], xt.shape[0], CHUNK))
        got = typed_mean_restated(rels, xt.shape[0], width)
        assert got.dtype == np.float32 and got.shape == want[t].shape and np.array_equal(got, want[t]), t
    assert longest > 2 * CHUNK + 1


def _backward_form(flip, width, dtype, chunk):
    """d x of the ladder graph's sources from a d A [n_dst, 2 width]: identity on block 0 of an own array, then the transposed
    CSR reading block 1, scaled by the forward graph's row lengths."""
    ei, n_dst, n_src = ladder_graph(SEED, flip=flip)
    csr = csr_by_destination(ei, n_dst)
    d_own, _, d_a = ladder_inputs(n_dst, n_src, 2 * width, SEED + 1)
    rels = [RelSpec(None, d_own), RelSpec(transposed_csr(csr, n_src), d_a, in_col=width, pre_rowptr=csr[0])]
    return typed_mean_restated(rels, n_src, width, accumulate=True, chunk=chunk, dtype=dtype), rels


@pytest.mark.parametrize("flip", (False, True))
def test_the_chunked_order_is_a_reordering_and_nothing_else(flip):
    ei, n_dst, n_src = ladder_graph(SEED, flip=flip)
    x = ladder_inputs(n_dst, n_src, 5, SEED + 1)[0]
    fwd = [RelSpec(csr_by_destination(ei, n_dst), x, post_mean=True)]
    a, b = (typed_mean_restated(fwd, n_dst, 5, chunk=c, dtype=np.float64) for c in (CHUNK, 10 ** 9))
    assert rel_out(a, b) <= 1e-12
    a, b = (_backward_form(flip, 5, np.float64, c)[0] for c in (CHUNK, 10 ** 9))
    assert rel_grad(a, b) <= 1e-12 and a.shape == (n_src, 5)
    if flip:    # in float32 it IS another order
        assert not np.array_equal(_backward_form(flip, 5, np.float32, CHUNK)[0], _backward_form(flip, 5, np.float32, 10 ** 9)[0])


def test_the_scale_is_a_reciprocal_then_a_multiply_and_the_sum_runs_in_list_order():
    got, rels = _backward_form(False, 6, np.float32, CHUNK)
    ei, n_dst, n_src = ladder_graph(SEED)
    deg = np.bincount(ei[1], minlength=n_dst)
    (t_rowptr, t_col), d_a = rels[1].csr, rels[1].inp[:, 6:12]
    j = int(np.nonzero(np.diff(t_rowptr) >= 3)[0][0])
    rows = t_col[t_rowptr[j]:t_rowptr[j + 1]]
    assert len(rows) < CHUNK and len(set(deg[rows].tolist()) - {1, 2, 4, 8, 16, 32, 256, 512}) > 0     # a length whose reciprocal rounds
    acc = np.zeros(6, dtype=np.float32)
    for i in rows:
        acc = acc + d_a[i] * (np.float32(1) / np.float32(deg[i]))
    assert np.array_equal(got[j], (np.float32(0) + rels[0].inp[j, :6]) + acc)
    divided = rels[0].inp[:, :6] + np.stack([sum((d_a[i] / np.float32(deg[i]) for i in t_col[t_rowptr[k]:t_rowptr[k + 1]]),
                                                 np.zeros(6, np.float32)) for k in range(n_src)])
    assert not np.array_equal(got, divided) and rel_grad(got, divided) <= 1e-5                           # a division is other bits
    # list order: three relations of magnitudes that do not associate
    big = np.full((4, 1), 1e8, dtype=np.float32)
    three = [RelSpec(None, big), RelSpec(None, np.ones((4, 1), np.float32)), RelSpec(None, -big)]
    assert typed_mean_restated(three, 4, 1, accumulate=True).tolist() == [[0.0]] * 4
    assert typed_mean_restated([three[0], three[2], three[1]], 4, 1, accumulate=True).tolist() == [[1.0]] * 4
    # post_mean: 0 for an empty row; the identity beyond its input's rows has no entry; untouched columns keep the fill
    empty = RelSpec((np.zeros(5, np.int64), np.zeros(0, np.int64)), big, post_mean=True, out_col=2)
    out = typed_mean_restated([empty, RelSpec(None, big[:2] * 0 + 3, out_col=0)], 4, 1, n_cols=4, fill=-77.0)
    assert out.tolist() == [[3.0, -77.0, 0.0, -77.0]] * 2 + [[0.0, -77.0, 0.0, -77.0]] * 2


def test_the_launch_of_eight_holds_the_mix_it_is_built_for():
    rels = eight_relations(SEED, 8)
    assert [ei is None for ei, _, _ in rels] == [True, False, False, False, False, True, False, False]
    slots, longest = [], []
    for ei, n_in, x in rels:
        assert x.shape == (n_in, 8) and x.dtype == np.float32
        if ei is None:
            assert n_in >= EIGHT_ROWS
            slots.append(0), longest.append(1)
            continue
        assert ei.shape[1] == 0 or (ei[0].max() < n_in and ei[1].max() < EIGHT_ROWS)
        e = ei.shape[1]
        slots.append(-(-e // CHUNK) if e > CHUNK else 0)
        longest.append(int(np.bincount(ei[1], minlength=EIGHT_ROWS).max()) if e else 0)
    assert [s > 0 for s in slots] == [False, True, True, False, True, False, False, True]
    assert [n > CHUNK for n in longest] == [False, True, False, False, False, False, False, True]
    assert rels[2][0].shape[1] == 300 and rels[3][0].shape[1] == 200 and rels[6][0].shape[1] == 0
    assert longest[1] == longest[7] == 3 * CHUNK and not np.array_equal(rels[1][0], rels[7][0][:, :rels[1][0].shape[1]])
    # the second ladder's first slot is not a multiple of anything convenient: slots of 1, 2, 4 come before it
    assert sum(slots[:7]) == 24 + 2 + 24 and slots[7] == 24
    deg = np.bincount(rels[7][0][1], minlength=EIGHT_ROWS)
    assert deg[-3:].sum() == 0 and deg[-4] > CHUNK and np.bincount(rels[1][0][1], minlength=EIGHT_ROWS)[-3:].sum() == 0
