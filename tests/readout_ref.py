"""The sequential CPU reference of the graph-level readouts (egc_amd.global_add_pool / global_mean_pool / global_max_pool):
what a scatter loop over the rows in input order computes, vectorised over the segments.  torch's CPU float32 add, divide and
compare are single correctly rounded IEEE operations, so these ARE the order rule of egc_amd/csrc/egc_readout.hip restated;
nothing here calls the code under test."""
import torch


def seg_ptr_of(batch: torch.Tensor, n_graphs: int) -> torch.Tensor:
    """Offsets of the graphs of a sorted batch vector: int64 [n_graphs + 1]."""
    return torch.searchsorted(batch.contiguous(), torch.arange(n_graphs + 1, dtype=batch.dtype))


def forward(x: torch.Tensor, seg: torch.Tensor, op: str):
    """(out float32 [G, C], arg int32 [G, C] or None): acc = 0; for k in range(longest segment):
    acc[live] = acc[live] + x[r0[live] + k] (sum, mean), or take = x_k > cur (first step: take all) with arg updated where
    take (max).  Mean divides by clamp(count, 1).  Empty segments give 0 and arg -1."""
    assert x.dtype == torch.float32 and x.device.type == "cpu"
    G, C = seg.numel() - 1, x.size(1)
    r0, cnt = seg[:-1], seg[1:] - seg[:-1]
    acc = torch.zeros(G, C, dtype=torch.float32)
    arg = torch.full((G, C), -1, dtype=torch.int32) if op == "max" else None
    for k in range(int(cnt.max()) if G else 0):
        live = torch.nonzero(cnt > k).view(-1)
        rows = r0[live] + k
        xk = x[rows]
        if op == "max":
            cur = acc[live]
            take = torch.ones_like(xk, dtype=torch.bool) if k == 0 else xk > cur
            acc[live] = torch.where(take, xk, cur)
            arg[live] = torch.where(take, rows.to(torch.int32)[:, None].expand_as(xk), arg[live])
        else:
            acc[live] = acc[live] + xk
    if op == "mean":
        acc = acc / cnt.clamp(min=1).to(torch.float32)[:, None]
    return acc, arg


def backward(d_out: torch.Tensor, seg: torch.Tensor, op: str, n_rows: int, arg=None) -> torch.Tensor:
    """d x [n_rows, C]: sum d_out[batch]; mean (d_out / clamp(count, 1))[batch]; max a zero tensor with d_out[g, c] placed at
    (arg[g, c], c).  Rows outside every segment stay 0."""
    assert d_out.dtype == torch.float32 and d_out.device.type == "cpu"
    G, C = d_out.shape
    cnt = seg[1:] - seg[:-1]
    d_x = torch.zeros(n_rows, C, dtype=torch.float32)
    if op == "max":
        g, c = torch.nonzero(arg >= 0, as_tuple=True)
        d_x[arg[g, c].long(), c] = d_out[g, c]
        return d_x
    rows = torch.arange(int(seg[0]), int(seg[-1])) if G else torch.zeros(0, dtype=torch.int64)
    owner = torch.repeat_interleave(torch.arange(G), cnt)
    src = d_out / cnt.clamp(min=1).to(torch.float32)[:, None] if op == "mean" else d_out
    d_x[rows] = src[owner]
    return d_x


# ---------------------------------------------------------------------------------------------------------------------
# The sweep of tests/test_readout_shapes_gpu.py (its properties are asserted without a GPU in tests/test_readout_shapes_cpu.py).
# ---------------------------------------------------------------------------------------------------------------------
RD_AHEAD = 8                   # rows requested together by the forward kernel
# segment lengths around one, two and three batches of rows, the empty one and a long one
LADDER = (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 25, 64)
# one lane; two; a scalar width; 63 / 64 / 65 lanes; 256 / 257 / 258 lanes, a group wider than a workgroup; both forms
WIDTHS = (1, 2, 3, 4, 5, 8, 77, 252, 256, 260, 1024, 1028, 1030)


def ladder_sizes(order):
    """Segment sizes: the ladder ("up": as listed, "down": reversed) with an empty segment first, in the middle and last."""
    body = list(LADDER if order == "up" else LADDER[::-1])
    body = [n for n in body if n != 0]
    half = len(body) // 2
    return [0] + body[:half] + [0] + body[half:] + [0]


def ladder_batch(order):
    """(batch vector int64 [N], number of graphs) of ladder_sizes(order)."""
    sizes = torch.tensor(ladder_sizes(order))
    return torch.repeat_interleave(torch.arange(sizes.numel()), sizes), int(sizes.numel())


def same_bits_or_both_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equality of two float tensors where a NaN equals a NaN (an add that makes a NaN need not make the same payload on
    two machines); everything else must be equal."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(torch.where(na, torch.zeros_like(a), a), torch.where(nb, torch.zeros_like(b), b))
