"""The oracle of the graph-build tests (tests/graph_ref.py) checked on the CPU, no GPU: ``csr_oracle`` against a deliberately naive
second formulation; ``tier_ladder`` really holds one row of every length it names, in every order, and stays small; ``check_plan``
accepts a plan built in Python and REFUSES each single corruption it exists to catch; the forward GEMM's count recovery
``rint(1 / (d * d))`` holds in float32 on the float32-rounded oracle tables at every degree the GPU tests use."""
import numpy as np
import pytest

import graph_ref as gr

C = gr.constants()
THR, CHUNK = C["EGC_LONG_ROW_THRESHOLD"], C["EGC_LONG_ROW_CHUNK"]


def test_the_constants_come_from_the_sources_and_the_ladder_follows_them():
    from egc_amd import _C
    assert (THR, CHUNK) == (_C.LONG_ROW_THRESHOLD, _C.LONG_ROW_CHUNK)
    assert set(gr.KERNEL_NAMES + gr.HEADER_NAMES) <= set(C)
    assert C["BUILD_WAVE_ROW"] == C["BUILD_LDS_SORT"] // 16          # an expression over an earlier constant is evaluated
    assert gr.LANE_ROW < THR < C["BUILD_WAVE_ROW"] < C["BUILD_RANK_ROW"] < C["BUILD_LDS_SORT"] < C["BUILD_MERGE_ROW"]
    with open(gr.GRAPH_HIP) as f:                                    # the one tier edge without a name is still that literal
        assert "if (deg[r] <= %d)" % gr.LANE_ROW in f.read()
    assert gr.ladder_lengths() == (0, 1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096,
                                   4097, 8193, 12288, 65535, 65536, 65537)


def _naive(ei, n, n_src):
    """Per-row Python lists, appended to in input order."""
    rows = [[] for _ in range(n)]
    top = -1
    for p in range(ei.shape[1]):
        s, d = int(ei[0, p]), int(ei[1, p])
        if 0 <= s < n_src and 0 <= d < n:
            rows[d].append((s, p))
            top = max(top, s, d)
    rowptr, col, eid = [0], [], []
    for r in rows:
        col += [s for s, _ in r]
        eid += [p for _, p in r]
        rowptr.append(len(col))
    return rowptr, col, eid, top


@pytest.mark.parametrize("n,n_src,e,bad", [(1, None, 0, 0), (1, None, 5, 0), (1, None, 6, 3), (7, None, 0, 0), (7, None, 40, 0),
                                           (30, None, 300, 25), (30, 90, 300, 25), (90, 30, 300, 25), (12, 5, 100, 100)])
def test_csr_oracle_equals_the_naive_formulation(n, n_src, e, bad):
    rng = np.random.default_rng(1000 * n + e + bad)
    ns = n if n_src is None else n_src
    ei = np.stack([rng.integers(0, ns, size=e), rng.integers(0, n, size=e)]).astype(np.int64)
    far = np.array([-1, -7, n, ns, max(n, ns), max(n, ns) + 3, 2 ** 32, 2 ** 32 + 1, -(2 ** 40), 2 ** 31], dtype=np.int64)
    for p in rng.choice(e, size=bad, replace=False) if bad else []:
        ei[rng.integers(0, 2), p] = far[rng.integers(0, far.size)]       # (n in the source row of a wide source space stays valid)
    o = gr.csr_oracle(ei, n, n_src)
    rowptr, col, eid, top = _naive(ei, n, ns)
    assert o.rowptr.tolist() == rowptr and o.col.tolist() == col and o.edge_id.tolist() == eid
    assert o.kept == len(col) and o.max_index == top
    if bad == e and e:
        assert o.kept < e
    # ... and it is the oracle of the filtered list, through the kept edges' own numbering
    keep = np.array(sorted(eid), dtype=np.int64)
    f = gr.csr_oracle(ei[:, keep], n, n_src)
    assert np.array_equal(f.rowptr, o.rowptr) and np.array_equal(f.col, o.col) and np.array_equal(keep[f.edge_id], o.edge_id)


def test_oracle_tables_on_a_hand_made_graph():
    # row 0: sources 0, 0, 2 (two self loops); row 1: empty; row 2: source 1
    o = gr.csr_oracle(np.array([[0, 1, 0, 2], [0, 2, 0, 0]], dtype=np.int64), 3)
    t = gr.oracle_tables(o)
    assert t.deg.tolist() == [3, 0, 1] and t.non_self.tolist() == [1, 0, 1]
    assert np.allclose(t.dis_raw, [3 ** -0.5, 0.0, 1.0]) and np.allclose(t.dis_looped, [2 ** -0.5, 1.0, 2 ** -0.5])
    assert np.array_equal(t.edge_dis_raw, t.dis_raw[o.col]) and np.array_equal(t.edge_dis_looped, t.dis_looped[o.col])


@pytest.mark.parametrize("order", gr.ORDERS)
def test_tier_ladder_holds_one_row_of_every_length(order):
    ei, n, where = gr.tier_ladder(5, order)
    assert 4500 <= n <= 5500 and ei.dtype == np.int64 and ei.shape[0] == 2
    assert 230_000 <= ei.shape[1] < 300_000
    deg = np.bincount(ei[1], minlength=n)
    assert sorted(where) == list(gr.ladder_lengths())
    for m, r in where.items():
        assert deg[r] == m
        assert m == 0 or int((deg == m).sum()) == 1, f"{int((deg == m).sum())} rows of {m} entries"
    rows = sorted(where.values())
    assert rows[0] == 0 and rows[-1] == n - 1 and deg[0] > THR and deg[n - 1] > THR      # long rows first and last
    assert int((np.diff(rows) == 1).sum()) == 1                                            # two adjacent, no other neighbours
    assert int((deg == 0).sum()) > 1000 and int(((deg >= 2) & (deg <= 8)).sum()) > 2000
    # self loops and duplicates inside the long rows
    o = gr.csr_oracle(ei, n)
    for m in (65, 4097, 65537):
        a = int(o.rowptr[where[m]])
        cols = o.col[a:a + m]
        assert int((cols == where[m]).sum()) >= 2 and np.unique(cols).size < m - 5
    # what the order is for
    tile, win = C["BUILD_TILE"], C["BUILD_WIN"]
    spans = [int(ei[1, a:a + tile].max() - ei[1, a:a + tile].min()) + 1 for a in range(0, ei.shape[1], tile)]
    if order == "shuffled":
        assert min(spans[:-1]) > win                   # every full tile takes the per-edge-atomic path
    else:
        assert max(spans) <= win                       # every tile fits the LDS window; the hub rows span many tiles
        step = np.diff(ei[1])
        assert (step >= 0).all() if order == "by_dst" else (step <= 0).all()
    # the same rows and the same entries in every order; the reversed list is by_dst read backwards
    base, _, where0 = gr.tier_ladder(5, "by_dst")
    assert where0 == where
    if order == "reversed":
        assert np.array_equal(ei, base[:, ::-1])
    assert np.array_equal(np.sort(ei[0] * n + ei[1]), np.sort(base[0] * n + base[1]))


def test_tier_ladder_variants_of_the_gpu_tests():
    m = C["BUILD_MERGE_ROW"]
    ei, n, where = gr.tier_ladder(5, "shuffled", max_len=m)
    assert sorted(where) == [v for v in gr.ladder_lengths() if v <= m] and ei.shape[1] < 300_000
    ei, n, where = gr.tier_ladder(6, "by_dst", lengths=(m - 1, m, m + 1), n=300)
    deg = np.bincount(ei[1], minlength=n)
    assert n == 300 and sorted(deg[deg > 8].tolist()) == [m - 1, m, m + 1] and ei.shape[1] < 300_000


# ---- check_plan ----------------------------------------------------------------------------------------------------------
def _plan_case(seed=3):
    """rowptr with long rows of 65, 256, 257, 700 and 5000 entries among short ones, and its plan in two random orders"""
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, THR + 1, size=60)
    deg[[0, 7, 8, 30, 59]] = [THR + 1, CHUNK, CHUNK + 1, 700, 5000]
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    return rowptr, gr.python_plan(rowptr, seed=seed)


def _views(plan):
    cl, cc = int(plan[2]), int(plan[3])
    return plan[4:4 + cl], plan[4 + cl:4 + 2 * cl], plan[4 + 2 * cl:4 + 2 * cl + cc], plan[4 + 2 * cl + cc:4 + 2 * cl + 2 * cc]


def test_check_plan_accepts_a_plan_built_from_the_oracle():
    rowptr, plan = _plan_case()
    assert plan[0] == 5 and plan[1] == 1 + 1 + 2 + 3 + 20
    gr.check_plan(plan, rowptr)
    gr.check_plan(gr.python_plan(rowptr), rowptr)                                   # slots in row order
    gr.check_plan(gr.python_plan(rowptr, n_edges=rowptr[-1] + 900), rowptr, n_edges=rowptr[-1] + 900)   # a build that dropped 900 edges
    ei, n, _ = gr.tier_ladder(5, "shuffled")
    o = gr.csr_oracle(ei, n)
    gr.check_plan(gr.python_plan(o.rowptr, seed=1), o.rowptr)
    # no long row at all, no row at all
    short = np.arange(0, 10 * THR + 1, THR, dtype=np.int64)
    gr.check_plan(gr.python_plan(short), short)
    gr.check_plan(gr.python_plan(np.zeros(1, dtype=np.int64)), np.zeros(1, dtype=np.int64))
    # the capacities of the two plan-capacity cases of the GPU file
    assert gr.plan_caps(200, 200 * (THR + 1)) == (201, 200 * (THR + 1) // CHUNK + 201)
    assert gr.plan_caps(3, 70001) == (4, 70001 // CHUNK + 4)


def _corrupt(kind, plan):
    long_row, long_chunk0, chunk_slot, chunk_begin = _views(plan)
    n_long, n_chunks = int(plan[0]), int(plan[1])
    big = int(np.argmax(np.bincount(chunk_slot[:n_chunks])))          # the slot of the 5000-entry row: 20 chunks
    if kind == "chunk_begin off by one chunk":
        chunk_begin[long_chunk0[big] + 3] += CHUNK
    elif kind == "two slots share a chunk range":
        long_chunk0[(big + 1) % n_long] = long_chunk0[big]
    elif kind == "a long row is missing":
        long_row[(big + 1) % n_long] = long_row[big]                  # ... its slot names another long row twice
    elif kind == "a short row is registered":
        long_row[(big + 1) % n_long] = 1
    elif kind == "n_chunks one too many":
        plan[1] += 1
    elif kind == "n_chunks one too few":
        plan[1] -= 1
    elif kind == "n_long one too few":
        plan[0] -= 1
    elif kind == "chunk_slot names another slot":
        chunk_slot[long_chunk0[big] + 19] = (big + 1) % n_long
    elif kind == "cap_chunks off by one":
        plan[3] += 1
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("kind", ["chunk_begin off by one chunk", "two slots share a chunk range", "a long row is missing",
                                  "a short row is registered", "n_chunks one too many", "n_chunks one too few", "n_long one too few",
                                  "chunk_slot names another slot", "cap_chunks off by one"])
def test_check_plan_rejects_every_single_corruption(kind):
    rowptr, plan = _plan_case()
    gr.check_plan(plan, rowptr)
    before = plan.copy()
    _corrupt(kind, plan)
    assert int((plan != before).sum()) == 1                           # ONE word is wrong
    with pytest.raises(AssertionError, match="plan"):
        gr.check_plan(plan, rowptr)


# ---- the count-recovery contract -------------------------------------------------------------------------------------------
def test_the_entry_count_is_recovered_from_the_float32_tables_at_every_degree_in_use():
    degs = np.unique(np.concatenate([np.arange(1, 4097), np.array(gr.ladder_lengths()[1:]), [70000]])).astype(np.int64)
    d32 = (degs.astype(np.float64) ** -0.5).astype(np.float32)       # the oracle's table, rounded to the device's format
    assert np.array_equal(gr.recovered_count(d32), degs)
    # ... and one float32 step either side of it (the device table may differ from the rounded oracle by the test's rtol of 2e-7)
    assert np.array_equal(gr.recovered_count(np.nextafter(d32, np.float32(0))), degs)
    assert np.array_equal(gr.recovered_count(np.nextafter(d32, np.float32(2))), degs)
    # through the oracle: dis_raw recovers the entry count, dis_looped the non-self count + 1
    ei, n, _ = gr.tier_ladder(5, "by_dst")
    t = gr.oracle_tables(gr.csr_oracle(ei, n))
    live = t.deg > 0
    assert np.array_equal(gr.recovered_count(t.dis_raw.astype(np.float32))[live], t.deg[live])
    assert (t.dis_raw[~live] == 0).all()
    assert np.array_equal(gr.recovered_count(t.dis_looped.astype(np.float32)), t.non_self + 1)
