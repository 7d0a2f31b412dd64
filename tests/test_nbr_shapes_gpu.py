"""The neighbour-sum kernel (egc_nbr_sum.hip) on the GPU at every row length and width it dispatches on: the ladder graph of
tests/mpnn_ref.py (one row of each of 0, 1, 7, 8, 9, 15, 16, 17, CHUNK - 1 .. CHUNK + 1, 2 CHUNK - 1 .. 2 CHUNK + 1, 3 CHUNK and
2 CHUNK + 18 entries; long rows first, last, adjacent, on / one past / one before a slot boundary; about 6,000 edges) and its flip
(the ladder in the transposed CSR the backward walks), square and -- where the form has a meaning there -- rectangular, with
``tail_empty`` and ``pad_to_chunk``, in every configuration GCNConv, SAGEConv and GINConv launch, over the 16-byte and the 4-byte
path, one lane to more lanes than a workgroup, plus the 4-byte path taken for an address or a stride.

Two checks per case, of the output and of the gradient with respect to x (the transposed form on the transposed CSR).  Bits:
``torch.equal`` to the sequential float32 restatement (tests/nbr_ref.py) -- the kernel documents its summation order.  Values, the
project's rule with the fixture constant replaced by a measurement made here: the truth is the same restatement in float64 on the
same float32 inputs, the yardstick the float32 restatement's own distance from it, and per quantity
error <= max(1e-5, 5 x yardstick)  (rel_out for the output, rel_grad for the gradient)."""
import functools

import numpy as np
import pytest
import torch

import egc_amd
from mpnn_ref import WIDTHS
from nbr_ref import CHUNK, csr_by_destination, ladder_graph, nbr_sum, nbr_sum_transposed, rel_grad, rel_out

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GRAPH_SEED, INPUT_SEED = 21, 22
BOTH = (False, True)                                     # the ladder in the forward CSR, in the transposed one
REDUCED = (("max_len", 2 * CHUNK + 1),)                  # the graph of the two widths above 1024

# tag: (form, self operand -- None, "x" (x_self is x: square graphs) or "apart" --, skip, s = self_scale or 1 + eps, table, e_p)
CONFIGS = {
    "sum": ("sum", None, False, None, None, None),                        # GCN neither flag, SAGE sum
    "sum+self": ("sum", "x", False, ("scale", 1.0), None, None),          # the backward of SAGE's [agg | x] operand
    "sum+eps": ("sum", "x", False, ("eps", 0.3), None, None),             # GIN
    "sum+apart": ("sum", "apart", False, ("scale", 0.7), None, None),     # the self operand another array (rectangular too)
    "sum+self+skip": ("sum", "x", True, ("scale", 1.0), None, None),      # GCN add_self_loops alone
    "mean": ("mean", None, False, None, None, None),                      # SAGE mean (its backward: mean_t)
    "mean_t": ("mean_t", None, False, None, None, None),                  # (its backward: mean)
    "sym": ("sym", None, False, None, "raw", "table"),                    # GCN normalize alone
    "sym gather": ("sym", None, False, None, "raw", "gather"),
    "sym+self+skip": ("sym", "x", True, None, "looped", "table"),         # GCN
    "sym+self+skip gather": ("sym", "x", True, None, "looped", "gather"),
}
RECTANGULAR = ("sum", "sum+apart", "mean", "mean_t")
SQUARE = tuple(CONFIGS)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def graph(flip, square, variant=()):
    """(edge_index, n_dst, n_src, rowptr, col) of ladder_graph(GRAPH_SEED, flip, square, **dict(variant))"""
    ei, n_dst, n_src = ladder_graph(GRAPH_SEED, flip=flip, square=square, **dict(variant))
    rowptr, col, _ = csr_by_destination(ei, n_dst)
    return (*_frozen(ei), n_dst, n_src, *_frozen(rowptr, col))


@functools.lru_cache(maxsize=None)
def device_graph(flip, square, variant=()):
    ei, n_dst, n_src, _, _ = graph(flip, square, variant)
    g = egc_amd.CSRGraph.from_edge_index(_dev(ei), n_dst, n_src)
    assert (g.n_nodes, g.n_src_rows, g.n_edges) == (n_dst, n_src, ei.shape[1])
    tables = {k: t[:n_dst].cpu().numpy() for k, t in (("raw", g.dis_raw), ("looped", g.dis_looped))} if square else {}
    return g, tables


@functools.lru_cache(maxsize=None)
def inputs(flip, square, variant, width):
    """(x [n_src, width], x_self [n_dst, width], d out [n_dst, width]) float32 standard normals"""
    _, n_dst, n_src, _, _ = graph(flip, square, variant)
    rng = np.random.default_rng(INPUT_SEED)
    return _frozen(*(rng.standard_normal((n, width)).astype(np.float32) for n in (n_src, n_dst, n_dst)))


def _s(weight, dtype):
    if weight is None:
        return dtype(1)
    v = dtype(np.float32(weight[1]))          # what the kernel is handed: a float32
    return v if weight[0] == "scale" else dtype(1) + v


@functools.lru_cache(maxsize=None)
def reference(flip, square, variant, width, tag):
    """{dtype: (out, d x)} of the restatement in float64 (the truth) and float32 (the bits, and the yardstick)."""
    form, self_op, skip, weight, table, _ = CONFIGS[tag]
    _, n_dst, n_src, rowptr, col = graph(flip, square, variant)
    x, xs, dout = inputs(flip, square, variant, width)
    scale = device_graph(flip, square, variant)[1].get(table)
    kw = dict(deg_rowptr=np.concatenate([[0], np.cumsum(np.bincount(col, minlength=n_src))])) if form == "mean_t" else {}
    ref = {}
    for dtype in (np.float64, np.float32):
        s = _s(weight, dtype)          # (1 + eps is formed in the working precision from the float32 eps)
        x_self = dict(x=x, apart=xs).get(self_op)
        out = nbr_sum(x, rowptr, col, form, x_self=x_self, s=s, skip=skip, row_scale=scale, src_scale=scale, dtype=dtype, **kw)
        dx = nbr_sum_transposed(dout, rowptr, col, n_src, form, shared_self=self_op == "x", s=s, skip=skip, scale=scale, dtype=dtype)
        ref[dtype] = _frozen(out, dx)
    return ref


def device_run(flip, square, variant, width, tag, arrays=None):
    """(out, d x) of the forward launch and, through autograd, the backward one"""
    form, self_op, skip, weight, table, e_p = CONFIGS[tag]
    g, _ = device_graph(flip, square, variant)
    x, xs, dout = (_dev(a) for a in inputs(flip, square, variant, width)) if arrays is None else arrays
    x = x.detach().requires_grad_(True)
    kw = {}
    if weight is not None:
        kw = dict(self_scale=weight[1]) if weight[0] == "scale" else dict(eps=torch.tensor([weight[1]], device=DEV))
    if table is not None:
        kw["scale"] = dict(raw=g.dis_raw, looped=g.dis_looped)[table]
        kw["edge_scale"] = dict(raw=g.edge_dis_raw, looped=g.edge_dis_looped)[table] if e_p == "table" else None
        assert e_p != "table" or kw["edge_scale"] is not None
    out = egc_amd.neighbor_sum(x, g, form, x_self=dict(x=x, apart=xs).get(self_op), skip_self_entries=skip, **kw)
    out.backward(dout)
    assert out.shape == (g.n_nodes, width) and x.grad.shape == (g.n_src_rows, width)
    return out.detach(), x.grad


def check(tag, got, ref):
    """Bits against the float32 restatement, then measured / yardstick / bound against the float64 one."""
    want, truth = ref[np.float32], ref[np.float64]
    bad = []
    for k, i, dist in (("out", 0, rel_out), ("d x", 1, rel_grad)):
        t = got[i].cpu()
        measured, yard = dist(t.numpy(), truth[i]), dist(want[i], truth[i])
        bound = max(1e-5, 5.0 * yard)
        print(f"{tag} {k}: measured {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
        if not torch.equal(t, torch.from_numpy(want[i])):
            bad.append(f"{k}: not the bits of the documented order ({int((t != torch.from_numpy(want[i])).sum())} elements differ)")
        if not measured <= bound:
            bad.append(f"{k}: error {measured:.3e}, restatement f32-vs-f64 {yard:.3e}, bound {bound:.3e}")
    assert not bad, f"{tag}: " + "; ".join(bad)


def _tag(flip, square, variant, width, tag):
    lanes = (width + 3) // 4
    return (f"{tag} width {width} ({lanes} lane{'s' if lanes > 1 else ''}, {'vec' if width % 4 == 0 else 'scalar'}) "
            f"{'flip' if flip else 'ladder'} {'square' if square else 'rectangular'}{''.join(' ' + k for k, _ in variant)}")


def _run_and_check(flip, square, variant, width, tag):
    check(_tag(flip, square, variant, width, tag), device_run(flip, square, variant, width, tag), reference(flip, square, variant, width, tag))


def test_the_graphs_are_what_the_sweep_claims():
    for square in BOTH:
        ei, n_dst, n_src, rowptr, col = graph(False, square)
        lengths = set(np.diff(rowptr).tolist())
        assert {0, 1, 7, 8, 9, 15, 16, 17, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK - 1, 2 * CHUNK, 2 * CHUNK + 1, 3 * CHUNK, 2 * CHUNK + 18} <= lengths
        assert 5500 <= ei.shape[1] <= 6500 and (n_dst == n_src) == square and ei.shape[1] % CHUNK != 0
        assert graph(False, square, (("pad_to_chunk", True),))[0].shape[1] % CHUNK == 0
        assert (np.diff(graph(False, square, (("tail_empty", True),))[3])[-3:] == 0).all()
        fe, fn_dst, fn_src, f_rowptr, f_col = graph(True, square)
        assert (fn_dst, fn_src) == (n_src, n_dst) and set(np.bincount(fe[0], minlength=fn_src).tolist()) == lengths
    _, n, _, rowptr, col = graph(False, True)
    assert (col == np.repeat(np.arange(n), np.diff(rowptr))).sum() > 10          # self entries for the skip flag, some in long rows
    assert max(WIDTHS) > 1024 and {1, 2, 3, 4, 5} <= set(WIDTHS)


# ------------------------------------------------------------------------------------------------------ a. the degree sweep

VARIANTS = ((), (("tail_empty", True),), (("pad_to_chunk", True),))
DEGREE_CASES = [(True, v, w, t) for v in VARIANTS for w in ((8, 6) if v == () else (8,)) for t in SQUARE] + \
               [(False, v, w, t) for v in VARIANTS for w in ((8, 6) if v == () else (8,)) for t in RECTANGULAR]


def _case_id(c):
    square, variant, width, tag = c
    return f"{'square' if square else 'rect'}-{'-'.join(k for k, _ in variant) or 'default'}-{width}-{tag.replace(' ', '_')}"


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("case", DEGREE_CASES, ids=_case_id)
def test_degree_sweep(case, flip):
    square, variant, width, tag = case
    _run_and_check(flip, square, variant, width, tag)


# ------------------------------------------------------------------------------------------------------- b. the width sweep

@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("square,tag", ((False, "mean"), (True, "sum+eps"), (True, "sym+self+skip")), ids=("mean", "sum+eps", "sym+self+skip"))
@pytest.mark.parametrize("width", WIDTHS)
def test_width_sweep(width, square, tag, flip):
    _run_and_check(flip, square, REDUCED if width > 1024 else (), width, tag)


# ----------------------------------------------------------------------------------- c. the 4-byte path taken for an address

def _block(t, cols, col):
    """t as columns col .. col + width of a fresh [rows, cols] array of sentinels"""
    big = torch.full((t.size(0), cols), -77.0, device=DEV)
    big[:, col:col + t.size(1)] = t
    return big, big[:, col:col + t.size(1)]


def _sentinels_kept(big, col, width):
    return bool((big[:, :col] == -77.0).all()) and bool((big[:, col + width:] == -77.0).all())


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("tag", ("mean", "sum+eps", "sym+self+skip", "sym+self+skip gather"), ids=lambda t: t.replace(" ", "_"))
@pytest.mark.parametrize("how", ("pointer", "stride", "out"))
def test_misaligned_operands_at_width_8_give_the_bits_of_aligned_ones(how, tag, flip):
    """``pointer``: x, x_self and d out are wide[:, 1:9] of a [n, 12] array (4 bytes off a 16-byte boundary, the stride a multiple
    of 16); ``stride``: they are wide[:, 0:8] of a [n, 11] array (aligned at row 0, a stride of 44 bytes); ``out``: the result is
    written at column 1 of a [n, 12] array and at column 0 of a [n, 11] one.  Each takes the 4-byte path at a width the 16-byte path
    takes otherwise, and has the bits the aligned call has (which test_degree_sweep holds to the restatement)."""
    width, square = 8, True
    want = device_run(flip, square, (), width, tag)
    check(_tag(flip, square, (), width, tag), want, reference(flip, square, (), width, tag))
    x, xs, dout = (_dev(a) for a in inputs(flip, square, (), width))
    if how in ("pointer", "stride"):
        cols, col = (11, 0) if how == "stride" else (12, 1)
        ops = []
        for t in (x, xs, dout):
            big, view = _block(t, cols, col)
            assert torch.equal(view, t) and view.stride(1) == 1
            assert (view.data_ptr() % 16 == 4 and view.stride(0) % 4 == 0) if how == "pointer" else (view.data_ptr() % 16 == 0 and view.stride(0) % 4 != 0)
            ops.append(view)
        got = device_run(flip, square, (), width, tag, arrays=ops)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        return
    form, self_op, skip, weight, table, e_p = CONFIGS[tag]
    g, _ = device_graph(flip, square, ())
    kw = dict(skip_self_entries=skip, x_self=x if self_op == "x" else None)
    if weight is not None:
        kw["eps"] = torch.tensor([weight[1]], device=DEV)
    if table is not None:
        kw.update(scale=g.dis_looped, edge_scale=g.edge_dis_looped if e_p == "table" else None)
    for cols, col in ((12, 1), (11, 0)):
        big = torch.full((g.n_nodes, cols), -77.0, device=DEV)
        block = egc_amd.neighbor_sum(x, g, form, out=big, out_col=col, **kw)
        assert block.data_ptr() == big.data_ptr() + 4 * col and (block.data_ptr() % 16 != 0 or block.stride(0) % 4 != 0)
        assert torch.equal(block, want[0]) and _sentinels_kept(big, col, width)


# ------------------------------------------------------------------------------ d. the same rows elsewhere in the grid

SHIFTED = (("prepend", 300),)


@pytest.mark.parametrize("flip", BOTH, ids=("ladder", "flip"))
@pytest.mark.parametrize("square,tag", ((False, "mean"), (True, "sum+self+skip"), (True, "sym+self+skip")), ids=("mean", "sum+self+skip", "sym+self+skip"))
@pytest.mark.parametrize("width", (6, 260))
def test_rows_landing_elsewhere_in_the_grid(width, square, tag, flip):
    """300 one-entry rows first: every long row's groups fall into later workgroups and its slots 300 / CHUNK further on, no
    longer aligned as in the sweep."""
    _run_and_check(flip, square, SHIFTED, width, tag)
