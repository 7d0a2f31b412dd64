"""The typed-mean kernel (egc_typed_mean.hip) on the GPU, called directly with TypedRel lists, at every row length and width it
dispatches on and in both of its forms: the forward form (``post_mean``, own column blocks) and the backward form
(``accumulate``, ``pre_rowptr``, transposed CSRs, a relation's block as ``in_col``) over the ladder graph of tests/mpnn_ref.py and
its flip, the backward through ``typed_mean_cat`` and autograd, one launch of all EGC_TYPED_MAX_RELATIONS = 8 relations mixing
relations with and without workspace slots and the identity in other places than 0, and the 4-byte path taken for an address or
a stride at a 16-byte width.  tests/test_typed_mean_shapes_cpu.py checks the restatement and the inputs.

Two checks per case, those of tests/test_mpnn_shapes_gpu.py.  Bits: ``torch.equal`` to ``typed_mean_restated`` in float32 -- the
kernel documents its order.  Values: the truth is the same restatement in float64 on the same float32 inputs, the yardstick the
float32 restatement's own distance from it, and  error <= max(1e-5, 5 x yardstick)  (rel_out in the forward form, rel_grad in the
accumulating one)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from egc_amd._typed import TypedMeanPlan, TypedRel, typed_mean, typed_mean_cat
from rgcn_ref import (CHUNK, EIGHT_ROWS, RelSpec, csr_by_destination, eight_relations, ladder_graph, ladder_inputs, rel_grad, rel_out,
                      seeded_arrays, transposed_csr, typed_mean_restated)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAPH_SEED, INPUT_SEED = 11, 12
BOTH = (False, True)
SENTINEL = -77.0


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def graph(flip=False):
    ei, n_dst, n_src = ladder_graph(GRAPH_SEED, flip=flip)
    ei.setflags(write=False)
    return ei, n_dst, n_src


def device_graph(ei, n_rows, n_in):
    g = egc_amd.CSRGraph.from_edge_index(_dev(ei), n_rows, n_in)
    assert (g.n_nodes, g.n_src_rows, g.n_edges) == (n_rows, n_in, ei.shape[1])
    return g


@functools.lru_cache(maxsize=None)
def ladder_device_graph(flip=False):
    return device_graph(*graph(flip))


def pair(ei, n_rows, n_in, inp, inp_dev=None, graph_dev=None, transposed=False, pre=False, **kw):
    """(RelSpec, TypedRel) of one relation over the graph ``ei`` [n_rows, n_in] (None: the identity).  ``transposed``: the
    relation walks the graph's transposed CSR (the launch has n_in rows, ``inp`` n_rows) scaled by the graph's own row lengths
    -- the backward form.  ``pre``: the graph's own CSR scaled by the row lengths of its transposed."""
    inp_dev = _dev(inp) if inp_dev is None else inp_dev
    if ei is None:
        return RelSpec(None, inp, **kw), TypedRel(None, inp_dev, **kw)
    g = device_graph(ei, n_rows, n_in) if graph_dev is None else graph_dev
    csr = csr_by_destination(ei, n_rows)
    if transposed:
        return (RelSpec(transposed_csr(csr, n_in), inp, pre_rowptr=csr[0], **kw),
                TypedRel(g.transposed(), inp_dev, pre_rowptr=g.rowptr, **kw))
    if pre and ei.shape[1] > 0:
        t_rowptr = np.concatenate([[0], np.cumsum(np.bincount(csr[1], minlength=n_in))])
        return RelSpec(csr, inp, pre_rowptr=t_rowptr, **kw), TypedRel(g, inp_dev, pre_rowptr=g.transposed().rowptr, **kw)
    return RelSpec(csr, inp, **kw), TypedRel(g, inp_dev, **kw)


def check(tag, got, specs, n_rows, width, accumulate, n_cols=None):
    """Bits against the float32 restatement, then measured / yardstick / bound against the float64 one."""
    want, truth = (typed_mean_restated(specs, n_rows, width, accumulate, CHUNK, dtype, n_cols=n_cols, fill=SENTINEL)
                   for dtype in (np.float32, np.float64))
    written = np.zeros(want.shape[1], dtype=bool)            # the distances are taken over the columns the launch writes
    for s in specs:
        written[0 if accumulate else s.out_col:(0 if accumulate else s.out_col) + width] = True
    dist = rel_grad if accumulate else rel_out
    measured, yard = dist(got.cpu().numpy()[:, written], truth[:, written]), dist(want[:, written], truth[:, written])
    bound = max(1e-5, 5.0 * yard)
    print(f"{tag}: measured {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
    assert got.shape == want.shape
    differ = int((got.cpu() != torch.from_numpy(want)).sum())
    assert torch.equal(got.cpu(), torch.from_numpy(want)), f"{tag}: not the bits of the documented order ({differ} elements differ)"
    assert measured <= bound, f"{tag}: error {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}"
    return want


# ---------------------------------------------------------------------------------------------------------- a. forward form

@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("width", (8, 6, 1, 100, 260, 1028))
def test_forward_form_over_the_ladder(width, flip):
    """[x | mean over the row's entries] as the layer launches it: the identity into block 0, the relation into block 1."""
    ei, n_dst, n_src = graph(flip)
    x_src, x_dst, _ = ladder_inputs(n_dst, n_src, width, INPUT_SEED)
    rels = [pair(None, n_dst, n_dst, x_dst), pair(ei, n_dst, n_src, x_src, graph_dev=ladder_device_graph(flip), post_mean=True, out_col=width)]
    out = torch.full((n_dst, 2 * width + 4), SENTINEL, device=DEV)
    typed_mean([t for _, t in rels], n_dst, width, out)
    want = check(f"forward form width {width} {'flip' if flip else 'ladder'}", out, [s for s, _ in rels], n_dst, width, False, 2 * width + 4)
    assert (want[:, 2 * width:] == SENTINEL).all() and np.array_equal(want[:, :width], x_dst)
    assert not want[np.diff(csr_by_destination(ei, n_dst)[0]) == 0, width:2 * width].any()          # 0 for a row without entries


# --------------------------------------------------------------------------------------------------------- b. backward form

@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("width", (8, 6))
def test_backward_form_over_the_transposed_ladder(width, flip):
    """d x of the sources as the layer's backward launches it: the identity on block 0 of the sources' own d A, then the
    transposed CSR reading block 1 of the destinations' d A scaled by 1 / the forward row length, added in that order.  With
    ``flip`` the transposed rows are the ladder."""
    ei, n_dst, n_src = graph(flip)
    d_own, _, d_a = ladder_inputs(n_dst, n_src, 2 * width, INPUT_SEED)
    rels = [pair(None, n_src, n_src, d_own), pair(ei, n_dst, n_src, d_a, graph_dev=ladder_device_graph(flip), transposed=True, in_col=width)]
    assert (int(np.diff(rels[1][0].csr[0]).max()) > 2 * CHUNK + 1) == flip
    out = torch.full((n_src, width), SENTINEL, device=DEV)
    typed_mean([t for _, t in rels], n_src, width, out, accumulate=True)
    check(f"backward form width {width} {'flip' if flip else 'ladder'}", out, [s for s, _ in rels], n_src, width, True)


# --------------------------------------------------------------------------------- c. through typed_mean_cat and autograd

@pytest.mark.parametrize("width", (8, 6))
def test_gradients_of_typed_mean_cat_have_the_bits_of_the_restated_backward(width):
    """Two node types, a (the ladder graph's destinations) and b (its sources); the ladder graph b -> a and its flip a -> b.
    A_a, A_b against the restated forward, d x_a and d x_b against the restated backward launches."""
    (lad, n_a, n_b), (flp, _, _) = graph(False), graph(True)
    g_lad, g_flp = ladder_device_graph(False), ladder_device_graph(True)
    plan = TypedMeanPlan(["a", "b"], dict(a=[("b", g_lad)], b=[("a", g_flp)]))
    arr = seeded_arrays([("x_a", (n_a, width)), ("x_b", (n_b, width)), ("d_a", (n_a, 2 * width)), ("d_b", (n_b, 2 * width))], INPUT_SEED)
    x_a, x_b = (_dev(arr[k]).requires_grad_(True) for k in ("x_a", "x_b"))
    a_a, a_b = typed_mean_cat(plan, [x_a, x_b])
    torch.autograd.backward([a_a, a_b], [_dev(arr["d_a"]), _dev(arr["d_b"])])
    fwd_a = [RelSpec(None, arr["x_a"]), RelSpec(csr_by_destination(lad, n_a), arr["x_b"], post_mean=True, out_col=width)]
    fwd_b = [RelSpec(None, arr["x_b"]), RelSpec(csr_by_destination(flp, n_b), arr["x_a"], post_mean=True, out_col=width)]
    check(f"cat width {width} A_a", a_a.detach(), fwd_a, n_a, width, False)
    check(f"cat width {width} A_b", a_b.detach(), fwd_b, n_b, width, False)
    bwd_a = [RelSpec(None, arr["d_a"]), pair(flp, n_b, n_a, arr["d_b"], graph_dev=g_flp, transposed=True, in_col=width)[0]]
    bwd_b = [RelSpec(None, arr["d_b"]), pair(lad, n_a, n_b, arr["d_a"], graph_dev=g_lad, transposed=True, in_col=width)[0]]
    assert int(np.diff(bwd_a[1].csr[0]).max()) == 3 * CHUNK and int(np.diff(bwd_b[1].csr[0]).max()) <= CHUNK
    check(f"cat width {width} d x_a", x_a.grad, bwd_a, n_a, width, True)
    check(f"cat width {width} d x_b", x_b.grad, bwd_b, n_b, width, True)


# ----------------------------------------------------------------------------------------- d. one launch of eight relations

@functools.lru_cache(maxsize=None)
def eight(width, accumulate):
    """[(RelSpec, TypedRel)] of eight_relations: own column blocks and post_mean, or accumulating with the entries scaled
    (every relation with entries but the 200-entry one, which stays unscaled between two scaled ones)."""
    rels = []
    for r, (ei, n_in, x) in enumerate(eight_relations(GRAPH_SEED, width)):
        kw = dict(pre=(r != 3)) if accumulate else dict(post_mean=ei is not None, out_col=r * width)
        rels.append(pair(ei, EIGHT_ROWS, n_in, x, **kw))
    return rels


@pytest.mark.parametrize("width", (8, 6))
def test_one_launch_of_eight_relations_forward_form(width):
    rels = eight(width, False)
    out = torch.full((EIGHT_ROWS, 8 * width + 1), SENTINEL, device=DEV)
    typed_mean([t for _, t in rels], EIGHT_ROWS, width, out)
    check(f"eight relations, forward form, width {width}", out, [s for s, _ in rels], EIGHT_ROWS, width, False, 8 * width + 1)
    assert bool((out[:, 8 * width:] == SENTINEL).all())
    for r, (_, t) in enumerate(rels):           # ... and eight launches of one relation each
        one = torch.full((EIGHT_ROWS, width), SENTINEL, device=DEV)
        typed_mean([t._replace(out_col=0)], EIGHT_ROWS, width, one)
        assert torch.equal(one, out[:, r * width:(r + 1) * width]), r


@pytest.mark.parametrize("width", (8, 6))
def test_one_launch_of_eight_relations_accumulating(width):
    rels = eight(width, True)
    assert [s.pre_rowptr is not None for s, _ in rels] == [False, True, True, False, True, False, False, True]
    out = torch.full((EIGHT_ROWS, width), SENTINEL, device=DEV)
    typed_mean([t for _, t in rels], EIGHT_ROWS, width, out, accumulate=True)
    check(f"eight relations, accumulating, width {width}", out, [s for s, _ in rels], EIGHT_ROWS, width, True)


def test_nine_relations_raise_without_device_work():
    rels = [t for _, t in eight(8, False)]
    out = torch.full((EIGHT_ROWS, 9 * 8), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="at most 8 relations"):
        typed_mean(rels + [rels[0]._replace(out_col=64)], EIGHT_ROWS, 8, out)
    assert bool((out == SENTINEL).all())


# ----------------------------------------------------------------------------------- e. the 4-byte path taken for an address

@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("how", ("in_col", "out_col", "stride"))
def test_misaligned_operands_at_width_8_give_the_bits_of_aligned_ones(how, flip):
    """``in_col`` = 1 of a [n, 12] input (the pointer 4 bytes off, the stride a multiple of 16); an ``out_col`` of 5; an input
    of row stride 11 read from column 0.  Both forms; each equals the aligned launch, and the restatement, bit for bit."""
    width = 8
    ei, n_dst, n_src = graph(flip)
    g = ladder_device_graph(flip)
    x_src, x_dst, d_a = ladder_inputs(n_dst, n_src, width, INPUT_SEED)

    def launches(in_cols, in_col, out_cols, out_col):
        def wide(a):
            big = np.full((a.shape[0], in_cols), SENTINEL, dtype=np.float32)
            big[:, in_col:in_col + width] = a
            return big
        fwd = [pair(None, n_dst, n_dst, wide(x_dst), in_col=in_col, out_col=out_col),
               pair(ei, n_dst, n_src, wide(x_src), graph_dev=g, post_mean=True, in_col=in_col, out_col=out_col + width)]
        out_f = torch.full((n_dst, out_cols + width), SENTINEL, device=DEV)
        typed_mean([t for _, t in fwd], n_dst, width, out_f)
        bwd = [pair(None, n_src, n_src, wide(x_src), in_col=in_col), pair(ei, n_dst, n_src, wide(d_a), graph_dev=g, transposed=True, in_col=in_col)]
        out_b = torch.full((n_src, out_cols), SENTINEL, device=DEV)
        typed_mean([t for _, t in bwd], n_src, width, out_b[:, out_col:out_col + width], accumulate=True)
        for t in [t for _, t in fwd + bwd]:
            ptr = t.inp.data_ptr() + 4 * t.in_col
            assert (ptr % 16 == 0) == (in_col % 4 == 0) and (t.inp.stride(0) % 4 == 0) == (in_cols % 4 == 0)
        return out_f, out_b, fwd, bwd

    aligned_f, aligned_b, fwd, bwd = launches(8, 0, 8, 0)
    check(f"aligned forward {'flip' if flip else 'ladder'}", aligned_f, [s for s, _ in fwd], n_dst, width, False, 16)
    check(f"aligned backward {'flip' if flip else 'ladder'}", aligned_b, [s for s, _ in bwd], n_src, width, True)
    in_cols, in_col, out_cols, out_col = dict(in_col=(12, 1, 8, 0), out_col=(8, 0, 16, 5), stride=(11, 0, 8, 0))[how]
    out_f, out_b, _, _ = launches(in_cols, in_col, out_cols, out_col)
    assert torch.equal(out_f[:, out_col:out_col + 2 * width], aligned_f[:, :2 * width])
    assert torch.equal(out_b[:, out_col:out_col + width], aligned_b[:, :width])
    for out, n in ((out_f, 2 * width), (out_b, width)):
        assert bool((out[:, :out_col] == SENTINEL).all()) and bool((out[:, out_col + n:] == SENTINEL).all())
