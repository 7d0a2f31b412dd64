"""The oracle of the graph build (egc_amd/csrc/egc_graph.hip), in numpy on the CPU, and the graphs its tests are run on.

``csr_oracle`` is what both device builds (egc_graph_build; egc_coo_to_csr_checked + egc_csr_prepare + egc_csr_edge_dis) must
produce from a COO list: edges with an id out of range dropped -- decided on the int64 values --, the rest ordered by a STABLE sort
on the destination, ``edge_id`` = the position in the list as given.  ``oracle_tables`` adds the float64 deg^-1/2 tables
(``nbr_ref.dis_tables``: they live there) and their per-entry copies.  ``check_plan`` asserts the whole long-row plan layout
documented in egc_plain.h; ``python_plan`` builds a valid one from a rowptr (what ``check_plan`` must accept; corrupt it and it must
refuse).  ``recovered_count`` is the forward GEMM's ``rint(1 / (d * d))`` (egc_gemm_f16x2.hip, cnt_inverse) in float32.

``tier_ladder`` is an edge list with one destination row of every length at which build_rows_kernel changes its sort -- one below,
on and one above each tier constant.  The constants are READ FROM THE SOURCES (``constants()``: the ``constexpr int NAME = ...;``
lines of egc_graph.hip and the two long-row ``#define``s of include/egc_hip.h as the binding reads them), so the ladder follows the code when one moves;
the one tier edge that has no name there (a row of up to 16 entries is ranked through the lanes) is ``LANE_ROW`` below."""
import functools
import os
import re
from collections import namedtuple

import numpy as np

from egc_amd import _C
from nbr_ref import dis_tables, transposed_csr  # noqa: F401  (the graph tests import them from here)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAPH_HIP = os.path.join(ROOT, "egc_amd", "csrc", "egc_graph.hip")
KERNEL_NAMES = ("BUILD_SCAN_ITEMS", "BUILD_LDS_SORT", "BUILD_WAVE_ROW", "BUILD_RANK_ROW", "BUILD_TILE", "BUILD_WIN",
                "BUILD_MERGE_ROW", "PREP_ROWS", "PREP_HUGE", "ROWS_PER_BLOCK", "ROWS_PER_GROUP")
HEADER_NAMES = ("EGC_LONG_ROW_THRESHOLD", "EGC_LONG_ROW_CHUNK")
LANE_ROW = 16      # build_rows_kernel: `if (deg[r] <= 16)` -- one entry per lane of a 16-lane group, a literal in the source

Csr = namedtuple("Csr", "rowptr col edge_id kept max_index")
Tables = namedtuple("Tables", "dis_raw dis_looped edge_dis_raw edge_dis_looped deg non_self")


@functools.lru_cache(maxsize=None)
def constants():
    """{name: value} of the tier and size constants, parsed from the sources (an expression may name earlier constants)."""
    with open(GRAPH_HIP) as f:
        hip = f.read()
    out = {}
    for name in HEADER_NAMES:
        if name not in _C.ABI.constants:
            raise AssertionError(f"include/egc_hip.h no longer has '#define {name} <int>': tests/graph_ref.py takes the tiers from it")
        out[name] = _C.ABI.constants[name]
    found = {m.group(1): m.group(2) for m in re.finditer(r"^constexpr int (\w+) = ([^;]+);", hip, re.M)}
    for name in KERNEL_NAMES:
        if name not in found:
            raise AssertionError(f"egc_graph.hip no longer has 'constexpr int {name} = ...;': tests/graph_ref.py takes the tiers from it")
    for name, text in found.items():      # in source order: an expression names only what stands above it
        if not re.fullmatch(r"[\w\s+\-*/()]+", text):
            raise AssertionError(f"egc_graph.hip: cannot evaluate 'constexpr int {name} = {text};'")
        out[name] = int(eval(text.replace("/", "//"), {"__builtins__": {}}, dict(out)))
    return out


def ladder_lengths():
    """Row lengths of the ladder: 0, 1, then value - 1, value, value + 1 of every tier constant of build_rows_kernel (and of
    prepare_kernel's PREP_HUGE), a merge-sorted row whose last chunk holds ONE entry and one that is an exact multiple of the chunk."""
    c = constants()
    tiers = (LANE_ROW, c["EGC_LONG_ROW_THRESHOLD"], c["BUILD_WAVE_ROW"], c["BUILD_RANK_ROW"], c["PREP_HUGE"], c["BUILD_LDS_SORT"],
             c["BUILD_MERGE_ROW"])
    lens = [0, 1] + [t + d for t in tiers for d in (-1, 0, 1)] + [2 * c["BUILD_LDS_SORT"] + 1, 3 * c["BUILD_LDS_SORT"]]
    assert len(set(lens)) == len(lens), "two tier constants have moved next to each other: the ladder needs distinct lengths"
    return tuple(sorted(lens))


# ---------------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------------
def csr_oracle(edge_index, n, n_src=None):
    """Csr(rowptr [n + 1], col [kept], edge_id [kept], kept, max_index) of an int64 [2, E] list (row 0 sources, row 1 destinations)"""
    ei = np.asarray(edge_index)
    assert ei.dtype == np.int64 and ei.ndim == 2 and ei.shape[0] == 2
    n, ns = int(n), int(n if n_src is None else n_src)
    src, dst = ei[0], ei[1]
    pos = np.flatnonzero((src >= 0) & (src < ns) & (dst >= 0) & (dst < n))     # on the int64 values: nothing is narrowed first
    order = pos[np.argsort(dst[pos], kind="stable")]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst[pos], minlength=n), out=rowptr[1:])
    max_index = int(max(src[pos].max(), dst[pos].max())) if pos.size else -1
    return Csr(rowptr, src[order], order, int(pos.size), max_index)


def oracle_tables(csr):
    """Tables(dis_raw [n], dis_looped [n], their per-entry copies dis_*[col[p]] (None where a source id has no row: n_src > n),
    deg, non-self deg) in float64 / int64"""
    raw, looped = dis_tables(csr.rowptr, csr.col)
    n = len(csr.rowptr) - 1
    deg = np.diff(csr.rowptr)
    row_of = np.repeat(np.arange(n, dtype=np.int64), deg)
    non_self = np.bincount(row_of[csr.col != row_of], minlength=n)
    per_entry = csr.col.size == 0 or int(csr.col.max()) < n
    return Tables(raw, looped, raw[csr.col] if per_entry else None, looped[csr.col] if per_entry else None, deg, non_self)


def recovered_count(dis):
    """rint(1 / (d * d)) in float32 on float32 values: the entry count the forward GEMM's folded weightings recover (0 for d = 0:
    a row without entries)"""
    d = np.asarray(dis, dtype=np.float32)
    live = d != 0
    return np.rint(np.float32(1.0) / np.where(live, d * d, np.float32(1.0))).astype(np.int64) * live


def plan_caps(n, e):
    """(cap_long, cap_chunks): egc_plain.h's plan_caps restated"""
    c = constants()
    cap_long = min(int(e) // (c["EGC_LONG_ROW_THRESHOLD"] + 1) + 1, int(n) + 1)
    return cap_long, int(e) // c["EGC_LONG_ROW_CHUNK"] + cap_long


def plan_ints(n, e):
    cap_long, cap_chunks = plan_caps(n, e)
    return 4 + 2 * cap_long + 2 * cap_chunks


def python_plan(rowptr, n_edges=None, seed=None):
    """A valid long-row plan (int32 words, egc_plain.h layout) of a CSR; with a seed, slots and chunk ranges are handed out in two
    unrelated random orders (the device hands them out by atomics).  Unused capacity holds -1."""
    c = constants()
    rowptr = np.asarray(rowptr, dtype=np.int64)
    n = len(rowptr) - 1
    e = int(rowptr[-1]) if n_edges is None else int(n_edges)
    cap_long, cap_chunks = plan_caps(n, e)
    deg = np.diff(rowptr)
    rows = np.flatnonzero(deg > c["EGC_LONG_ROW_THRESHOLD"])
    chunk_order = np.arange(len(rows))
    if seed is not None:
        rng = np.random.default_rng(seed)
        rows = rng.permutation(rows)
        chunk_order = rng.permutation(len(rows))
    nch = -(-deg[rows] // c["EGC_LONG_ROW_CHUNK"])
    plan = np.full(4 + 2 * cap_long + 2 * cap_chunks, -1, dtype=np.int32)
    plan[:4] = len(rows), int(nch.sum()), cap_long, cap_chunks
    long_row, long_chunk0 = plan[4:4 + cap_long], plan[4 + cap_long:4 + 2 * cap_long]
    chunk_slot = plan[4 + 2 * cap_long:4 + 2 * cap_long + cap_chunks]
    chunk_begin = plan[4 + 2 * cap_long + cap_chunks:]
    at = 0
    for s in chunk_order:
        long_row[s], long_chunk0[s] = rows[s], at
        for k in range(int(nch[s])):
            chunk_slot[at + k], chunk_begin[at + k] = s, rowptr[rows[s]] + k * c["EGC_LONG_ROW_CHUNK"]
        at += int(nch[s])
    return plan


def check_plan(plan, rowptr, n_edges=None):
    """Assert the long-row plan layout of egc_plain.h on host arrays: header caps = plan_caps(rows, edges handed to the build --
    ``n_edges``, the entries of ``rowptr`` if not given); n_long / n_chunks = the rows longer than the threshold / their chunks;
    long_row a permutation of exactly those rows; the slots' chunk ranges pairwise disjoint and tiling [0, n_chunks); every chunk
    names its slot and starts at rowptr[row] + k * EGC_LONG_ROW_CHUNK."""
    c = constants()
    thr, chunk = c["EGC_LONG_ROW_THRESHOLD"], c["EGC_LONG_ROW_CHUNK"]
    plan = np.asarray(plan).astype(np.int64)
    rowptr = np.asarray(rowptr).astype(np.int64)
    n = len(rowptr) - 1
    e = int(rowptr[-1]) if n_edges is None else int(n_edges)
    cap_long, cap_chunks = plan_caps(n, e)
    assert plan.size >= 4, "plan: no header"
    n_long, n_chunks = int(plan[0]), int(plan[1])
    assert (int(plan[2]), int(plan[3])) == (cap_long, cap_chunks), f"plan caps {tuple(plan[2:4])} != plan_caps {(cap_long, cap_chunks)}"
    assert plan.size >= 4 + 2 * cap_long + 2 * cap_chunks, "plan: shorter than its capacities"
    deg = np.diff(rowptr)
    want_rows = np.flatnonzero(deg > thr)
    assert n_long == want_rows.size, f"plan: n_long {n_long}, rows longer than {thr}: {want_rows.size}"
    want_chunks = int((-(-deg[want_rows] // chunk)).sum())
    assert n_chunks == want_chunks, f"plan: n_chunks {n_chunks}, sum of ceil(deg / {chunk}) over the long rows: {want_chunks}"
    assert n_long <= cap_long and n_chunks <= cap_chunks, "plan: more entries than capacity"
    long_row = plan[4:4 + n_long]
    long_chunk0 = plan[4 + cap_long:4 + cap_long + n_long]
    chunk_slot = plan[4 + 2 * cap_long:4 + 2 * cap_long + n_chunks]
    chunk_begin = plan[4 + 2 * cap_long + cap_chunks:4 + 2 * cap_long + cap_chunks + n_chunks]
    assert np.array_equal(np.sort(long_row), want_rows), "plan: long_row[:n_long] is not a permutation of the long rows"
    nch = -(-deg[long_row] // chunk)
    by_c0 = np.argsort(long_chunk0, kind="stable")
    starts, ends = long_chunk0[by_c0], long_chunk0[by_c0] + nch[by_c0]
    if n_long:
        assert starts[0] == 0 and ends[-1] == n_chunks and np.array_equal(ends[:-1], starts[1:]), \
            "plan: the slots' chunk ranges [long_chunk0, long_chunk0 + nch) do not tile [0, n_chunks) disjointly"
    want_slot = np.repeat(by_c0, nch[by_c0])
    k = np.arange(n_chunks, dtype=np.int64) - np.repeat(starts, nch[by_c0])
    want_begin = np.repeat(rowptr[long_row[by_c0]], nch[by_c0]) + chunk * k
    bad = np.flatnonzero(chunk_slot != want_slot)
    assert bad.size == 0, f"plan: chunk_slot[{bad[:4]}] = {chunk_slot[bad[:4]]}, owner slots {want_slot[bad[:4]]}"
    bad = np.flatnonzero(chunk_begin != want_begin)
    assert bad.size == 0, f"plan: chunk_begin[{bad[:4]}] = {chunk_begin[bad[:4]]}, rowptr[row] + {chunk} k = {want_begin[bad[:4]]}"


# ---------------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------------
ORDERS = ("shuffled", "by_dst", "reversed")


def rows_to_edge_index(n, row_len, seed, order, n_src=None):
    """int64 [2, E]: row i gets row_len[i] entries with random sources; rows longer than EGC_LONG_ROW_THRESHOLD also get self loops
    (where the row id is a source id) and duplicate entries.  ``order``: "by_dst" -- ascending destination, so a tile of consecutive
    edges points into a narrow window of rows and a long row spans many tiles; "reversed" -- that list read backwards (destinations
    descend, a row's entries come in the opposite order: the slot an entry draws in the scatter is the hardware's business, the
    list is what a test can set); "shuffled" -- a random permutation, so every tile spans the whole id range."""
    assert order in ORDERS
    rng = np.random.default_rng(seed)
    ns = n if n_src is None else n_src
    row_len = np.asarray(row_len, dtype=np.int64)
    dst = np.repeat(np.arange(n, dtype=np.int64), row_len)
    src = rng.integers(0, ns, size=dst.size).astype(np.int64)
    at = np.concatenate([[0], np.cumsum(row_len)])
    for row in np.flatnonzero(row_len > constants()["EGC_LONG_ROW_THRESHOLD"]):
        a, m = int(at[row]), int(row_len[row])
        if row < ns:
            src[a + rng.choice(m, size=5, replace=False)] = row              # self loops, scattered over the row
        src[a + m // 2:a + m // 2 + 7] = src[a + 3]                           # seven more copies of one entry
    if order == "reversed":
        src, dst = src[::-1], dst[::-1]
    elif order == "shuffled":
        p = rng.permutation(dst.size)
        src, dst = src[p], dst[p]
    return np.ascontiguousarray(np.stack([src, dst]))


def tier_ladder(seed, order, max_len=None, lengths=None, n=5000):
    """(edge_index int64 [2, E], n, {length: row id}): a square graph of ``n`` rows in which exactly one row has each length of
    ``lengths`` (default: ``ladder_lengths()``, without those above ``max_len``) -- one is the first row, one the last, two are
    adjacent, the rest scattered -- and every other row is empty or has 2 .. 8 entries (so none of them has a ladder length but 0)."""
    lengths = [m for m in (ladder_lengths() if lengths is None else lengths) if max_len is None or m <= max_len]
    rng = np.random.default_rng(seed)
    assert n >= 4 * len(lengths) + 8
    filler = np.where(rng.random(n) < 0.35, 0, rng.integers(2, 9, size=n))
    assert not (set(filler.tolist()) & set(lengths)) - {0}
    perm = [lengths[i] for i in rng.permutation(len(lengths))]
    perm.sort(key=lambda m: m <= constants()["EGC_LONG_ROW_THRESHOLD"])        # (stable) long rows take the four named places
    pair = int(rng.integers(n // 4, 3 * n // 4))
    taken = {0, n - 1, pair, pair + 1}
    places = [0, n - 1, pair, pair + 1]
    while len(places) < len(perm):
        r = int(rng.integers(1, n - 1))
        if not ({r - 1, r, r + 1} & taken):          # scattered: no third neighbour
            taken.add(r)
            places.append(r)
    row_len = filler.copy()
    where = {}
    for m, r in zip(perm, places):
        row_len[r] = m
        where[m] = r
    return rows_to_edge_index(n, row_len, seed + 1, order), n, where
