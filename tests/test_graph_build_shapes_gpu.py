"""The graph build kernels (egc_amd/csrc/egc_graph.hip) on the GPU at every row length and size they dispatch on.  Every case
runs BOTH builds -- egc_graph_build (EGC_GRAPH_BUILD=fast) and the radix-sort pipeline egc_coo_to_csr_checked + egc_csr_prepare +
egc_csr_edge_dis (=sort) -- and each is compared WITH THE ORACLE of tests/graph_ref.py (numpy; itself checked in
tests/test_graph_build_shapes_cpu.py), not with the other build:

    rowptr, col[:kept], edge_id[:kept], max_index     torch.equal
    dis_raw, dis_looped, their per-entry copies       the float64 oracle at rtol = 2e-7 (the bound of test_parity_gpu.py)
    rint(1 / (d * d)) in float32                      = the entry count (non-self count + 1 for dis_looped), on the DEVICE's values:
                                                      what the forward GEMM's folded weightings rely on (egc_gemm_f16x2.hip)
    the long-row plan                                 graph_ref.check_plan: the whole layout of egc_plain.h
    check_indices()                                   passes where nothing was dropped, raises where something was

``CSRGraph.transposed()`` (csr_transposed_coo_kernel + a build) against ``transposed_csr`` of the forward CSR, and
``egc_gather_rows_f32`` against ``index_select``, close the file.

Which case lands on which constant (value - 1, value, value + 1 unless stated); the constants are read from the sources
(graph_ref.constants()), the cases below are built from them:

    constant (egc_graph.hip / egc_hip.h)        case
    ------------------------------------------  -------------------------------------------------------------------------------
    16 lanes of a short row (a literal)         ladder-*: rows of 15, 16, 17
    EGC_LONG_ROW_THRESHOLD = 64                 ladder-*: rows of 63, 64, 65;  cap-all-65: every row one past it
    BUILD_WAVE_ROW = 256 (= EGC_LONG_ROW_CHUNK) ladder-*: rows of 255, 256, 257 (one chunk, one chunk, two)
    BUILD_RANK_ROW = 1024                       ladder-*: rows of 1023, 1024, 1025
    PREP_HUGE = 2048                            ladder-*: rows of 2047, 2048, 2049;  hubs-2048 / hubs-2049: 64 such rows filling
                                                one block of prepare_kernel (all of s_huge_* / none of it)
    BUILD_LDS_SORT = 4096                       ladder-*: rows of 4095, 4096, 4097 (4097: merge_sort_big, last chunk of ONE entry),
                                                8193 (two full chunks + one entry), 12288 (three full chunks, no remainder)
    BUILD_MERGE_ROW = 65536                     ladder-*: rows of 65535, 65536 (merge_sort_big at its cap: 16 chunks);
                                                top-*: rows of 65535, 65536, 65537 -- 65537 is the first row bitonic_big sorts
                                                in any test;  cap-one-row: a row of 70,000
    BUILD_SCAN_ITEMS = 4096 (rows per scan      nodes-4095 / -4096 / -4097 and nodes-8191 / -8192 / -8193 (the writer of
      block; rowptr[n] by base <= n < base + 4)   rowptr[n] is the last thread of a block, the first of the next one, ...);
                                                nodes-1 .. -5 (the four elements of thread 0);  nodes-4096-tail / -4097-tail
    ROWS_PER_BLOCK x ROWS_PER_GROUP = 128 rows  nodes-127 / -128 / -129
      per workgroup of build_rows_kernel
    PREP_ROWS = 64                              nodes-63 / -64 / -65;  hubs-*: the hub rows are one whole block (row id 128 .. 191)
    BUILD_TILE = 2048                           edges-2047 / -2048 / -2049, edges-4096 / -4097 (and 1, 255, 256: one partial tile)
    BUILD_WIN = 2048                            window: a tile whose destinations span exactly 2048 rows (LDS path) next to one
                                                that spans 2049 (per-edge atomics);  window-below: a tile spanning 2047;
                                                ladder-shuffled: every tile beyond the window;
                                                ladder-by_dst / -reversed: every tile inside it
    plan_caps (egc_plain.h)                     cap-all-65: n_long = cap_long - 1, one chunk each;  cap-one-row: cap_long clamped
                                                to n + 1
    the range check                             dropped-all, dropped-tile (one whole tile out of range between two good ones),
                                                dropped-narrowing (2^32 + 5, -(2^40): valid after a careless narrowing)
    the non-self rule off the square            rect-wide (n_src > n), rect-narrow (n_src < n), with source id = destination id
    csr_transposed_coo_kernel's row search      ends-square / -wide / -narrow: first and last rows AND source columns empty
"""
import functools

import numpy as np
import pytest
import torch

import egc_amd
import graph_ref as gr
from egc_amd import _C
from egc_amd.graph import _IndexFlag, _stream_ptr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BUILDS = ("fast", "sort")
C = gr.constants()
TILE, WIN, MERGE, HUGE, PREP_ROWS, THR = (C[k] for k in ("BUILD_TILE", "BUILD_WIN", "BUILD_MERGE_ROW", "PREP_HUGE", "PREP_ROWS",
                                                         "EGC_LONG_ROW_THRESHOLD"))
SCAN = C["BUILD_SCAN_ITEMS"]
ROWS_BLOCK = C["ROWS_PER_BLOCK"] * C["ROWS_PER_GROUP"]
NODE_COUNTS = (1, 2, 3, 4, 5, PREP_ROWS - 1, PREP_ROWS, PREP_ROWS + 1, ROWS_BLOCK - 1, ROWS_BLOCK, ROWS_BLOCK + 1,
               SCAN - 1, SCAN, SCAN + 1, 2 * SCAN - 1, 2 * SCAN, 2 * SCAN + 1)
EDGE_COUNTS = (1, 255, 256, TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1)


# ---- the cases: name -> (edge_index int64 [2, E], n, n_src or None) ----------------------------------------------------------
def _random(seed, n, e, n_src=None, dst_range=None, src_range=None, last_row=True):
    rng = np.random.default_rng(seed)
    ns = n if n_src is None else n_src
    d0, d1 = dst_range or (0, n)
    s0, s1 = src_range or (0, ns)
    ei = np.stack([rng.integers(s0, s1, size=e), rng.integers(d0, d1, size=e)]).astype(np.int64)
    if last_row and e:
        ei[1, e // 2] = d1 - 1
    return ei


def _nodes(n, tail=0):
    # three edges per row on average, self loops among them (n = 1: nothing else); `tail` last rows empty
    return _random(100 + n + tail, n, 3 * n, dst_range=(0, n - tail)), n, None


def _window():
    n = 2 * WIN + 1
    rng = np.random.default_rng(7)
    dst = np.concatenate([rng.integers(0, WIN, size=TILE), rng.integers(WIN, n, size=TILE)])
    dst[[0, 1]] = 0, WIN - 1                   # tile 0: span WIN exactly
    dst[[TILE, TILE + 1]] = n - 1, WIN         # tile 1: span WIN + 1
    assert [int(np.ptp(dst[a:a + TILE])) + 1 for a in (0, TILE)] == [WIN, WIN + 1]
    return np.stack([rng.integers(0, n, size=2 * TILE), dst]).astype(np.int64), n, None


def _window_below():
    n = WIN
    ei = _random(8, n, TILE, dst_range=(0, WIN - 1))     # one tile, span WIN - 1: the last row stays empty
    ei[1, 0] = 0
    assert int(np.ptp(ei[1])) + 1 == WIN - 1
    return ei, n, None


def _hubs(length):
    n, first = 200 + PREP_ROWS, 2 * PREP_ROWS
    rng = np.random.default_rng(length)
    row_len = rng.integers(0, 9, size=n)
    row_len[first:first + PREP_ROWS] = length
    return gr.rows_to_edge_index(n, row_len, 31, "shuffled"), n, None


def _dropped_all():
    n, e = 100, 3000
    ei = _random(41, n, e)
    k = np.arange(e)
    ei[0, k % 4 == 0] = n + k[k % 4 == 0]
    ei[1, k % 4 == 1] = n
    ei[0, k % 4 == 2] = -1
    ei[1, k % 4 == 3] = -1 - k[k % 4 == 3]
    return ei, n, None


def _dropped_tile():
    n = 300
    ei = _random(42, n, 3 * TILE)
    ei[0, TILE:2 * TILE:2] += n                # the whole middle tile, by its source or by its destination
    ei[1, TILE + 1:2 * TILE:2] -= n
    return ei, n, None


def _dropped_narrowing():
    n = 50
    ei = _random(43, n, 400)
    ei[0, 10], ei[1, 20], ei[0, 30], ei[1, 40] = 2 ** 32 + 5, 2 ** 32 + 5, -(2 ** 40), -(2 ** 40)     # int32: 5, 5, 0, 0
    ei[1, 50], ei[0, 60], ei[1, 399] = 2 ** 32, 2 ** 33 + n - 1, 2 ** 31 + 7
    return ei, n, None


def _rect(n, ns, seed):
    rng = np.random.default_rng(seed)
    row_len = rng.integers(0, 9, size=n)
    row_len[[3, n - 2]] = 3 * THR, THR + 1
    ei = gr.rows_to_edge_index(n, row_len, seed, "shuffled", n_src=ns)
    onto = np.flatnonzero(ei[1] < ns)          # a source id equal to the destination id, wherever there is such a source
    pick = onto[rng.choice(onto.size, size=onto.size // 5, replace=False)]
    ei[0, pick] = ei[1, pick]
    return ei, n, ns


def _ends(n, ns, seed):
    # first 5 / last 7 rows without an entry, first 4 / last 9 source columns never named; one long row, one long column
    ei = _random(seed, n, 2500, n_src=ns, dst_range=(5, n - 7), src_range=(4, ns - 9))
    ei[1, :300] = 5
    ei[0, 300:500] = ns - 10
    return ei, n, (None if ns == n else ns)


CASES = {}
for _order in gr.ORDERS:
    CASES[f"ladder-{_order}"] = functools.partial(lambda o: gr.tier_ladder(5, o, max_len=MERGE)[:2] + (None,), _order)
    CASES[f"top-{_order}"] = functools.partial(lambda o: gr.tier_ladder(6, o, lengths=(MERGE - 1, MERGE, MERGE + 1), n=300)[:2] + (None,),
                                               _order)
for _n in NODE_COUNTS:
    CASES[f"nodes-{_n}"] = functools.partial(_nodes, _n)
for _n in (SCAN, SCAN + 1):
    CASES[f"nodes-{_n}-tail"] = functools.partial(_nodes, _n, 9)
for _e in EDGE_COUNTS:
    CASES[f"edges-{_e}"] = functools.partial(lambda e: (_random(200 + e, 300, e), 300, None), _e)
CASES["window"] = _window
CASES["window-below"] = _window_below
CASES[f"hubs-{HUGE + 1}"] = functools.partial(_hubs, HUGE + 1)
CASES[f"hubs-{HUGE}"] = functools.partial(_hubs, HUGE)
CASES["cap-all-65"] = lambda: (gr.rows_to_edge_index(200, np.full(200, THR + 1), 51, "shuffled"), 200, None)
CASES["cap-one-row"] = lambda: (gr.rows_to_edge_index(3, np.array([0, 70000, 1]), 52, "shuffled"), 3, None)
CASES["rect-wide"] = functools.partial(_rect, 200, 500, 61)
CASES["rect-narrow"] = functools.partial(_rect, 500, 120, 62)
CASES["ends-square"] = functools.partial(_ends, 300, 300, 71)
CASES["ends-wide"] = functools.partial(_ends, 200, 450, 72)
CASES["ends-narrow"] = functools.partial(_ends, 450, 200, 73)
DROPPED = {"dropped-all": _dropped_all, "dropped-tile": _dropped_tile, "dropped-narrowing": _dropped_narrowing}
CASES.update(DROPPED)


@functools.lru_cache(maxsize=None)
def case(name):
    """(edge_index, n, n_src or None, Csr oracle, Tables oracle), computed once and shared by the tests that need it"""
    ei, n, ns = CASES[name]()
    o = gr.csr_oracle(ei, n, ns)
    t = gr.oracle_tables(o)
    for a in (ei, *o[:3], *(x for x in t if x is not None)):
        a.setflags(write=False)
    return ei, n, ns, o, t


def _i32(a):
    return torch.from_numpy(np.asarray(a).astype(np.int32))


def _same(got, want, what, rowptr=None):
    """torch.equal, and on a mismatch where it is: the row's length names the tier of build_rows_kernel that sorted it"""
    got, want = got.cpu(), _i32(want)
    if torch.equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)}, oracle {tuple(want.shape)}"
    bad = torch.nonzero(got != want).flatten()
    p, where = int(bad[0]), ""
    if rowptr is not None:
        row = int(np.searchsorted(rowptr, p, side="right")) - 1
        where = f" (entry {p - int(rowptr[row])} of row {row}, a row of {int(rowptr[row + 1] - rowptr[row])} entries)"
    raise AssertionError(f"{what}: {bad.numel()} of {want.numel()} values differ, the first at {p}{where}: {int(got[p])}, "
                         f"oracle {int(want[p])}")


def _built(ei, n, ns, build, monkeypatch):
    monkeypatch.setenv("EGC_GRAPH_BUILD", build)
    g = egc_amd.CSRGraph.from_edge_index(torch.from_numpy(ei.copy()).to(DEV), n, ns)      # (the shared array is read-only)
    torch.cuda.synchronize()
    return g


def _check_tables(g, n, o, t, per_entry):
    k = o.kept
    raw, looped = g.dis_raw[:n].cpu().numpy(), g.dis_looped[:n].cpu().numpy()
    np.testing.assert_allclose(raw, t.dis_raw, rtol=2e-7, atol=0)
    np.testing.assert_allclose(looped, t.dis_looped, rtol=2e-7, atol=0)
    assert np.array_equal(gr.recovered_count(raw), t.deg), "rint(1 / dis_raw^2) is not the entry count"
    assert np.array_equal(gr.recovered_count(looped), t.non_self + 1), "rint(1 / dis_looped^2) is not the non-self count + 1"
    if per_entry:
        assert g.edge_dis_raw is not None and g.edge_dis_looped is not None
        np.testing.assert_allclose(g.edge_dis_raw[:k].cpu().numpy(), t.edge_dis_raw, rtol=2e-7, atol=0)
        np.testing.assert_allclose(g.edge_dis_looped[:k].cpu().numpy(), t.edge_dis_looped, rtol=2e-7, atol=0)
    else:
        assert g.edge_dis_raw is None and g.edge_dis_looped is None       # per-entry copies belong to square graphs


def _check_graph(g, ei, n, ns, o, t):
    e, k = ei.shape[1], o.kept
    assert (g.n_nodes, g.n_edges, g.n_src_rows) == (n, e, n if ns is None else ns)
    _same(g.rowptr, o.rowptr, "rowptr")
    _same(g.edge_id[:k], o.edge_id, "edge_id", o.rowptr)
    _same(g.col[:k], o.col, "col", o.rowptr)
    _same(g.max_index, [o.max_index], "max_index")
    _check_tables(g, n, o, t, ns is None or ns == n)
    gr.check_plan(g.plan.cpu().numpy(), o.rowptr, n_edges=e)


CLEAN = [name for name in CASES if name not in DROPPED]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", CLEAN)
def test_build_equals_the_oracle(name, build, monkeypatch):
    ei, n, ns, o, t = case(name)
    assert o.kept == ei.shape[1]
    g = _built(ei, n, ns, build, monkeypatch)
    _check_graph(g, ei, n, ns, o, t)
    assert g.check_indices() is g


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", list(DROPPED))
def test_build_with_dropped_edges_equals_the_oracle_of_the_filtered_list(name, build, monkeypatch):
    ei, n, ns, o, t = case(name)
    assert o.kept < ei.shape[1] and (name != "dropped-all" or o.kept == 0)
    try:
        g = _built(ei, n, ns, build, monkeypatch)
        assert _IndexFlag._view.value == 1                 # the device has raised the sticky host-visible word
        _check_graph(g, ei, n, ns, o, t)                   # (edge_id: positions in the list as given)
        with pytest.raises(RuntimeError, match="out of range"):
            g.check_indices()
        assert _IndexFlag._view.value == 0                 # reported there
    finally:
        torch.cuda.synchronize()
        _IndexFlag._view.value = 0                         # later tests are unaffected whatever happened here


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ["ladder-shuffled", "ends-square", "ends-wide", "ends-narrow", "rect-wide", "rect-narrow", "nodes-1"])
def test_transposed_equals_the_transposed_oracle(name, build, monkeypatch):
    ei, n, ns, o, _ = case(name)
    e, n_src = ei.shape[1], n if ns is None else ns
    g = _built(ei, n, ns, build, monkeypatch)
    t = g.transposed()
    torch.cuda.synchronize()
    t_rowptr, t_col = gr.transposed_csr(o.rowptr, o.col, n_src)
    forward_pos = np.argsort(o.col, kind="stable")         # a row's entries in ascending forward position
    assert (t.n_nodes, t.n_edges, t.n_src_rows) == (n_src, e, n)
    _same(t.rowptr, t_rowptr, "transposed rowptr")
    _same(t.col[:e], t_col, "transposed col", t_rowptr)
    _same(t.edge_id[:e], forward_pos, "transposed edge_id", t_rowptr)
    _same(t.max_index, [o.max_index], "transposed max_index")
    to = gr.Csr(t_rowptr, t_col, forward_pos, e, o.max_index)
    _check_tables(t, n_src, to, gr.oracle_tables(to), n_src == n)
    gr.check_plan(t.plan.cpu().numpy(), t_rowptr, n_edges=e)
    assert t.check_indices() is t and g.transposed() is t


# ---- egc_gather_rows_f32 -------------------------------------------------------------------------------------------------
def _gather(table_ptr, ld, idx, width, out):
    return _C.load().egc_gather_rows_f32(table_ptr, ld, idx.data_ptr(), int(idx.numel()), width, out.data_ptr(), _stream_ptr(DEV))


@pytest.mark.parametrize("pad", [0, 4])
@pytest.mark.parametrize("width,rows,table_rows", [(4, 0, 37), (4, 1, 37), (4, 1000, 37), (8, 0, 37), (8, 1, 37), (8, 1000, 37),
                                                   (132, 0, 37), (132, 1, 37), (132, 1000, 37), (512, 8200, 64)])
def test_gather_rows_equals_index_select(width, rows, table_rows, pad):
    """ld = width, and ld = width + 4 through a view into a wider table; no row, one row, and (8,200 rows of 512 floats)
    more 16-byte pieces than the capped grid of 256 * 16 blocks of 256 threads has lanes; repeated indices, the last index."""
    gen = torch.Generator().manual_seed(width + rows + pad)
    full = torch.randn(table_rows, width + pad, generator=gen).to(DEV)
    idx = torch.randint(0, table_rows, (rows,), generator=gen)
    if rows:
        idx[rows // 2] = table_rows - 1
    if rows > 2:
        idx[-1] = idx[0] = idx[1]
    idx = idx.to(DEV)
    if rows == 8200:
        assert rows * (width // 4) > 256 * 16 * 256
    out = torch.full((rows + 1, width), float("nan"), device=DEV)          # one guard row behind the rows asked for
    assert _gather(full.data_ptr(), width + pad, idx, width, out) == 0
    torch.cuda.synchronize()
    assert torch.equal(out[:rows], full[:, :width].index_select(0, idx))
    assert bool(torch.isnan(out[rows]).all())


def test_gather_rows_refuses_what_it_cannot_do_in_16_byte_pieces():
    INVALID = _C.ERR_INVALID
    assert INVALID == 1
    assert _C._STATUS[INVALID] == "EGC_ERR_INVALID"
    full = torch.randn(16, 16, device=DEV)
    idx = torch.arange(4, device=DEV)
    out = torch.zeros(4 * 8 + 16, device=DEV)                               # four rows of eight floats, then a guard
    assert full.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert _gather(full.data_ptr(), 16, idx, 8, out) == 0
    assert _gather(full.data_ptr(), 16, idx, 6, out) == INVALID            # a width that is no multiple of 4
    assert _gather(full.data_ptr(), 16, idx, 0, out) == INVALID
    assert _gather(full.data_ptr(), 4, idx, 8, out) == INVALID             # ld < width
    assert _gather(full.data_ptr(), 10, idx, 8, out) == INVALID            # ld no multiple of 4
    assert _gather(full.data_ptr() + 4, 16, idx, 8, out) == INVALID        # a table that is not 16-byte aligned
    assert _gather(full.data_ptr(), 16, idx, 8, out[1:]) == INVALID        # an output that is not
    torch.cuda.synchronize()
    assert torch.equal(out[:32].view(4, 8), full[:4, :8]) and not bool(out[32:].any())      # only the valid call wrote
