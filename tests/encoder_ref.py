"""The sequential CPU reference of the node encoders (egc_amd.Embedding / AtomEncoder / ASTNodeEncoder / NodeEncoder):
the float32 forward in table order, and for the backward the float64 gradient sums with, next to them, sum |g| and the
count k per destination row -- what the error bound of tests/test_encoder_gpu.py is made of.  torch's CPU float32 add and
multiply are single correctly rounded IEEE operations, so the forward IS the order rule of egc_amd/csrc/egc_encoder.hip
restated; nothing here calls the code under test."""
import torch

U = 2.0 ** -24     # unit roundoff of float32


def gamma(m: torch.Tensor) -> torch.Tensor:
    """Higham, Accuracy and Stability of Numerical Algorithms, section 4.2 eq. 4.4: gamma_m = m u / (1 - m u) (float64)."""
    m = m.to(torch.float64)
    return m * U / (1.0 - m * U)


def keys(idx: torch.Tensor, table_rows, clamp=None):
    """(row of table t that node n uses [N, T] int64, valid [N, T] bool): min(idx, clamp[t]) where a clamp is given; an
    index outside [0, R_t) after the clamp is not valid (the table contributes nothing for that node)."""
    idx = idx[:, None] if idx.dim() == 1 else idx
    k = idx.clone()
    for t in range(idx.size(1)):
        if clamp is not None and clamp[t] is not None and clamp[t] >= 0:
            k[:, t] = k[:, t].clamp(max=clamp[t])
    rows = torch.tensor(list(table_rows), dtype=torch.int64)
    valid = (k >= 0) & (k < rows[None, :])
    return torch.where(valid, k, torch.zeros_like(k)), valid


def forward(tables, idx: torch.Tensor, clamp=None) -> torch.Tensor:
    """out = ((W_0[k_0] + W_1[k_1]) + W_2[k_2]) + ..., one float32 add per table, tables ascending."""
    assert all(w.dtype == torch.float32 and w.device.type == "cpu" for w in tables)
    k, valid = keys(idx, [w.size(0) for w in tables], clamp)
    out = None
    for t, w in enumerate(tables):
        row = torch.where(valid[:, t, None], w[k[:, t]], torch.zeros((), dtype=torch.float32))
        out = row if out is None else out + row
    return out


def masked_rows(d_out: torch.Tensor, keep=None, scale: float = 1.0) -> torch.Tensor:
    """The contribution rows g: d_out, or where(keep, d_out * float32(scale), 0) -- one float32 rounding."""
    assert d_out.dtype == torch.float32 and d_out.device.type == "cpu"
    if keep is None:
        return d_out
    return torch.where(keep.bool(), d_out * torch.tensor(scale, dtype=torch.float32), torch.zeros((), dtype=torch.float32))


def backward(g: torch.Tensor, idx: torch.Tensor, table_rows, clamp=None):
    """Per table: (sum of g rows in float64 [R, F], sum of |g| in float64 [R, F], count k int64 [R])."""
    k, valid = keys(idx, table_rows, clamp)
    g64 = g.to(torch.float64)
    res = []
    for t, r in enumerate(table_rows):
        sel = torch.nonzero(valid[:, t]).view(-1)
        s = torch.zeros(r, g.size(1), dtype=torch.float64).index_add_(0, k[sel, t], g64[sel])
        a = torch.zeros(r, g.size(1), dtype=torch.float64).index_add_(0, k[sel, t], g64[sel].abs())
        res.append((s, a, torch.bincount(k[sel, t], minlength=r)))
    return res


# ---------------------------------------------------------------------------------------------------------------------
# The backward's own summation order (include/egc_hip.h, header of egc_amd/csrc/egc_encoder.hip), restated.
# ---------------------------------------------------------------------------------------------------------------------
def _ordered_list_sums(rows: torch.Tensor, group: torch.Tensor, n_groups: int) -> torch.Tensor:
    """sums [n_groups, F]: for every group the rows whose ``group`` entry names it, taken in the order they stand in
    ``rows``: the first is ASSIGNED, every later one added with one add of rows.dtype.  Groups nobody names stay 0.
    Vectorised over the groups by rank inside the list: step k handles the k-th member of every list at once, so a list's
    chain of adds is the sequential one."""
    out = torch.zeros(n_groups, rows.size(1), dtype=rows.dtype)
    if rows.size(0) == 0:
        return out
    order = torch.argsort(group, stable=True)              # lists back to back, the given order kept inside each
    gs = group[order]
    pos = torch.arange(gs.numel())
    rank = pos - torch.searchsorted(gs, gs, right=False)   # position inside its list
    by_rank = torch.argsort(rank, stable=True)
    steps = torch.bincount(rank).tolist()
    at = 0
    for k, m in enumerate(steps):
        sel = by_rank[at:at + m]
        at += m
        dst, src = gs[sel], rows[order[sel]]
        if k == 0:
            out[dst] = src
        else:
            out[dst] = out[dst] + src                      # dst holds every group at most once: a plain gather / scatter
    return out


def chunked_backward(g: torch.Tensor, idx: torch.Tensor, table_rows, clamp=None, chunk: int = 256, dtype=torch.float32):
    """Per table the gradient [R_t, F] in the kernel's documented order, one add of ``dtype`` per step: nodes are cut into
    chunks of ``chunk``; per destination row and chunk the first contribution row is assigned and the later ones are added
    in ascending n; a destination's chunk sums are combined the same way in ascending chunk; a row nobody indexes is 0.
    ``g``: the already masked contribution rows (masked_rows).  In float32 this is what the device must give bit for bit."""
    assert g.device.type == "cpu" and g.dim() == 2
    k, valid = keys(idx, table_rows, clamp)
    g = g.to(dtype)
    n = g.size(0)
    n_chunks = (n + chunk - 1) // chunk if n else 0
    res = []
    for t, r in enumerate(table_rows):
        sel = torch.nonzero(valid[:, t]).view(-1)          # ascending n
        slot = (sel // chunk) * r + k[sel, t]              # (chunk, destination row)
        used, inv = torch.unique(slot, return_inverse=True)      # ascending: chunk-major, so ascending chunk per destination
        partial = _ordered_list_sums(g[sel], inv, used.numel())
        res.append(_ordered_list_sums(partial, used % r, r))
        assert used.numel() == 0 or int(used.max()) // r < n_chunks
    return res


def sequential_backward(g: torch.Tensor, idx: torch.Tensor, table_rows, clamp=None):
    """The plain loop over the nodes, one float32 add per contribution (the first is assigned): what chunked_backward
    is NOT once a list spans two chunks."""
    k, valid = keys(idx, table_rows, clamp)
    res = []
    for t, r in enumerate(table_rows):
        d = torch.zeros(r, g.size(1), dtype=torch.float32)
        seen = [False] * r
        for n in torch.nonzero(valid[:, t]).view(-1).tolist():
            v = int(k[n, t])
            d[v] = g[n] if not seen[v] else d[v] + g[n]
            seen[v] = True
        res.append(d)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_encoder_shapes_gpu.py (guarded without a GPU by tests/test_encoder_shapes_cpu.py).
# ---------------------------------------------------------------------------------------------------------------------
ENC_CHUNK = 256                    # nodes of a workgroup of the backward's first pass
ENC_RD_AHEAD = 8                   # rows (first pass) / chunk sums (second pass) requested together
ENC_FWD_BATCH = 4                  # table rows requested together in the forward
SWEEP_NODES = 600                  # 256 + 256 + 88
# one and two lanes; a small scalar width; 64 / 65 lanes; 128 / 129 lanes (two nodes, then one node per workgroup of the
# forward; one lane group per workgroup in the backward); 256 lanes, the limit
SWEEP_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 77, 255, 256, 257, 509, 512, 513, 1021, 1024)
SWEEP_TABLE_COUNTS = (1, 3, 4, 5, 8, 9, 16)
ROW_EDGES = (1, 2, 255, 256, 257, 600)     # around min(256, R_t) partial slots per chunk; 600: one row per node and more
T_SWEEP_WIDTHS = (256, 77)         # every table count at one vector and one scalar width


def sweep_tables(n_tables):
    """(rows, clamp, beyond) of the sweep's table set with n_tables tables: rows cycle through ROW_EDGES; from three tables
    on the last one is clamped to its last row and drawn 40 beyond it (the depth table of the AST encoder)."""
    rows = [ROW_EDGES[(t + n_tables) % len(ROW_EDGES)] for t in range(n_tables)]
    clamp, beyond = [None] * n_tables, [None] * n_tables
    if n_tables >= 3:
        if rows[-1] < 255:
            rows[-1] = 257
        clamp[-1], beyond[-1] = rows[-1] - 1, rows[-1] + 40
    return rows, clamp, beyond


def sweep_indices(n, rows, dist, seed, beyond=None):
    """int64 [n, T].  "uniform": every table uniform over its rows (or to ``beyond[t]``); "skewed": every node the same row
    of every table, so each chunk is one list of 256."""
    g = torch.Generator().manual_seed(seed)
    cols = []
    for t, r in enumerate(rows):
        hi = r if beyond is None or beyond[t] is None else beyond[t]
        cols.append(torch.randint(0, hi, (n,), generator=g) if dist == "uniform" else torch.full((n,), (r - 1) // 2, dtype=torch.int64))
    return torch.stack(cols, dim=1)


def sweep_cases():
    """(width, n_tables, dist): every width with nine tables, every table count at T_SWEEP_WIDTHS."""
    cases = [(w, 9, d) for w in SWEEP_WIDTHS for d in ("uniform", "skewed")]
    cases += [(w, t, d) for t in SWEEP_TABLE_COUNTS if t != 9 for w in T_SWEEP_WIDTHS for d in ("uniform", "skewed")]
    return cases


LADDER_LENGTHS = (1, 7, 8, 9, 15, 16, 17)          # around ENC_RD_AHEAD and twice it; the rest of the chunk is one more list
LADDER_ROWS = [9, 5]                               # table 0 carries the ladder (row 8 is indexed by nobody), table 1 is uniform


def ladder_indices(seed=3):
    """int64 [600, 2]: chunk 0 holds, in table 0, lists of LADDER_LENGTHS and one list of the remaining 183 nodes, shuffled
    so that no list is contiguous; the 256 nodes of chunk 1 share one key; chunk 2 (88 nodes) is uniform."""
    g = torch.Generator().manual_seed(seed)
    lengths = list(LADDER_LENGTHS) + [ENC_CHUNK - sum(LADDER_LENGTHS)]
    first = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths))[torch.randperm(ENC_CHUNK, generator=g)]
    col0 = torch.cat([first, torch.full((ENC_CHUNK,), 4, dtype=torch.int64), torch.randint(0, 8, (SWEEP_NODES - 2 * ENC_CHUNK,), generator=g)])
    return torch.stack([col0, torch.randint(0, LADDER_ROWS[1], (SWEEP_NODES,), generator=g)], dim=1)


NODE_LADDER = (1, 255, 256, 257, 511, 512, 513)                         # around one and two chunks
CHUNK_LADDER = tuple(ENC_CHUNK * k for k in (7, 8, 9, 16, 17)) + (ENC_CHUNK * 16 + 3,)    # around one and two batches of chunk sums
LADDER_WIDTH = 8
NODE_LADDER_ROWS = [2, 257, 600]       # a row of every chunk; rows that many chunks miss, in both tables
