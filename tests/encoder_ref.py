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
