"""Attention dropout of GATConv and GATv2Conv, restated for the tests: the generator, the mask and a plain per-edge composition.

``philox4x32_10``: Philox4x32-10 in numpy (what egc_amd/csrc/egc_philox.h computes on the host and on the device).

``keep_mask``: the mask of a destination-keyed CSR as egc_amd/csrc/egc_gat_dev.h defines it.  Key = (low, high 32 bits of the
int64 seed); the entry at position q of the CSR draws counter (q, h >> 2, 0, 0), the self entry of row i (i, h >> 2, 1, 0);
head h takes output word h & 3 and is DROPPED iff word < floor(p 2^32).  Entries skipped for the self loops keep their position.

``gat_composition`` / ``gatv2_composition``: the layers' propagate as PyG composes it -- one score per (edge, head), a softmax
per destination over all of its edges, alpha multiplied by the mask as a constant (0 or scale = float32(1 / (1 - p))),
index_add -- in torch on the CPU in the dtype asked for, gradients by autograd.  In float64 it is the truth, in float32 the
yardstick; it knows nothing of the kernels' summation order.  The rowptr / col it masks are the device CSRGraph's in the GPU
tests and mpnn_ref.csr_by_destination's on the CPU."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
SEED = 20240229          # the seed of the GPU tests (tests/test_gat_dropout_cpu.py checks the kept fractions under it)


def philox4x32_10(counter, key):
    """[..., 4] uint32 words from counter [..., 4] and key [..., 2] (anything that broadcasts, any integer type)."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) & 0xFFFFFFFF for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) & 0xFFFFFFFF for i in range(2)]
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(W0)) & mask, (k[1] + np.uint64(W1)) & mask]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def threshold(p):
    return int(np.floor(np.float64(p) * 4294967296.0))


def scale_of(p):
    return np.float32(1.0 / (1.0 - np.float64(p)))


def _words(c0, heads, stream, seed):
    """[len(c0), heads] uint32: head h's word for every counter value c0 of one stream (0: entries, 1: self entries)."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    groups = (heads + 3) // 4
    c0 = np.asarray(c0, dtype=np.uint64)
    counter = np.zeros((len(c0), groups, 4), dtype=np.uint64)
    counter[..., 0], counter[..., 1], counter[..., 2] = c0[:, None], np.arange(groups)[None, :], stream
    return philox4x32_10(counter, key).reshape(len(c0), groups * 4)[:, :heads]


def keep_mask(n_entries, n_rows, heads, p, seed):
    """(keep of every CSR position [E, H], keep of every row's self entry [N, H]) as bool; True = kept."""
    t = threshold(p)
    return _words(np.arange(n_entries), heads, 0, seed) >= t, _words(np.arange(n_rows), heads, 1, seed) >= t


def edge_list(rowptr, col, loops):
    """(src, dst, position) of the entries the layer sums over, as int64 arrays: the CSR's entries -- without those whose
    source is their row when self loops are added -- and then one self entry per row, position -1 - row."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    dst = np.repeat(np.arange(n), np.diff(rowptr))
    pos = np.arange(len(dst))
    src = col[:len(dst)]
    if loops:
        keep = src != dst
        src, dst, pos = src[keep], dst[keep], pos[keep]
        src, dst, pos = np.concatenate([src, np.arange(n)]), np.concatenate([dst, np.arange(n)]), np.concatenate([pos, -1 - np.arange(n)])
    return src, dst, pos


def multipliers(rowptr, col, heads, loops, p, seed, mask=None):
    """m' [E', H] float32 for edge_list's entries: scale where kept, 0 where dropped.  ``mask``: (entries, selves) to use instead
    of keep_mask's (the all-ones mask of the CPU tests)."""
    n = len(rowptr) - 1
    _, _, pos = edge_list(rowptr, col, loops)
    keep_e, keep_s = mask if mask is not None else keep_mask(int(np.asarray(rowptr)[-1]), n, heads, p, seed)
    keep = np.where((pos >= 0)[:, None], keep_e[np.maximum(pos, 0)], keep_s[np.maximum(-1 - pos, 0)])
    return keep.astype(np.float32) * scale_of(p)


def _propagate(s, xl, src, dst, n, mult):
    """(out [N, H, C], lse [N, H]) from the scores s [E', H]: softmax per destination over ALL entries, then the mask."""
    h = s.size(1)
    idx = dst.view(-1, 1).expand(-1, h)
    top = torch.full((n, h), -float("inf"), dtype=s.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    ex = torch.exp(s - top.index_select(0, dst))
    den = torch.zeros((n, h), dtype=s.dtype).index_add(0, dst, ex)
    alpha = ex / den.index_select(0, dst)
    out = torch.zeros((n,) + tuple(xl.shape[1:]), dtype=s.dtype).index_add(0, dst, (alpha * mult).unsqueeze(-1) * xl.index_select(0, src))
    with torch.no_grad():
        lse = torch.where(den > 0, top + torch.log(den), torch.full_like(den, -float("inf")))
    return out, lse


def _finish(out, lse, leaves, gout, dtype):
    res = [out.detach().numpy().reshape(out.size(0), -1), lse.numpy()]
    if gout is not None:
        out.backward(torch.from_numpy(np.asarray(gout)).to(dtype).view_as(out))
        res += [t.grad.numpy() for t in leaves]
    return tuple(res)


def gat_propagate(xl, a_src, a_dst, src, dst, mult, slope=0.2):
    """(out [N, H, C], lse [N, H]) of GAT v1 from torch tensors xl [N, H C], a_src, a_dst [N, H] (differentiable), the entries
    (src, dst) and their multipliers mult [E', H]."""
    n, h = a_dst.shape
    s = torch.nn.functional.leaky_relu(a_src.index_select(0, src) + a_dst.index_select(0, dst), slope)
    return _propagate(s, xl.view(n, h, -1), src, dst, n, mult)


def gatv2_propagate(xl, xr, att, src, dst, mult, slope=0.2):
    """(out [N, H, C], lse [N, H]) of GATv2 from torch tensors xl, xr [N, H C] and att [H, C] (differentiable)."""
    h, c = att.shape
    n = xr.size(0)
    x3 = xl.view(n, h, c)
    z = x3.index_select(0, src) + xr.view(n, h, c).index_select(0, dst)
    s = (torch.nn.functional.leaky_relu(z, slope) * att).sum(dim=-1)
    return _propagate(s, x3, src, dst, n, mult)


def gat_composition(xl, a_src, a_dst, rowptr, col, mult, gout=None, slope=0.2, loops=True, dtype=torch.float64):
    """(out [N, H C], lse [N, H]) and, with gout, (d xl, d a_src, d a_dst) of GAT v1 under the multipliers ``mult`` [E', H]."""
    leaves = tuple(torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (xl, a_src, a_dst))
    src, dst, _ = (torch.from_numpy(a) for a in edge_list(rowptr, col, loops))
    out, lse = gat_propagate(*leaves, src, dst, torch.from_numpy(mult).to(dtype), slope)
    return _finish(out, lse, leaves, gout, dtype)


def gatv2_composition(xl, xr, att, rowptr, col, mult, gout=None, slope=0.2, loops=True, dtype=torch.float64):
    """(out [N, H C], lse [N, H]) and, with gout, (d xl, d xr [N, H C], d att [H, C]) of GATv2 under the multipliers ``mult``."""
    leaves = tuple(torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_(True) for a in (xl, xr, att))
    src, dst, _ = (torch.from_numpy(a) for a in edge_list(rowptr, col, loops))
    out, lse = gatv2_propagate(*leaves, src, dst, torch.from_numpy(mult).to(dtype), slope)
    return _finish(out, lse, leaves, gout, dtype)


def layer_composition(kind, x, params, heads, channels, rowptr, col, mult, gout, concat=True, slope=0.2, loops=True, dtype=torch.float64):
    """(out, {name: gradient}) of GATConv (kind "gat") or GATv2Conv ("gatv2") as a per-edge composition in ``dtype``: params is the
    layer's state dict as numpy arrays (lin_dst.weight, an alias, is left out of the gradients), gradients by autograd."""
    x = torch.from_numpy(np.asarray(x)).to(dtype)
    q = {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in params.items() if k != "lin_dst.weight"}
    src, dst, _ = (torch.from_numpy(a) for a in edge_list(rowptr, col, loops))
    m = torch.from_numpy(mult).to(dtype)
    if kind == "gat":
        xl = x @ q["lin_src.weight"].t()
        x3 = xl.view(-1, heads, channels)
        out, _ = gat_propagate(xl, (x3 * q["att_src"]).sum(-1), (x3 * q["att_dst"]).sum(-1), src, dst, m, slope)
    else:
        xl, xr = x @ q["lin_l.weight"].t() + q["lin_l.bias"], x @ q["lin_r.weight"].t() + q["lin_r.bias"]
        out, _ = gatv2_propagate(xl, xr, q["att"].view(heads, channels), src, dst, m, slope)
    out = out.reshape(out.size(0), -1) if concat else out.mean(dim=1)
    out = out + q["bias"]
    out.backward(torch.from_numpy(np.asarray(gout)).to(dtype))
    return out.detach().numpy(), {k: v.grad.numpy() for k, v in q.items()}
