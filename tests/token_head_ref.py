"""Float64 reference of the token head (egc_amd/csrc/egc_token_head.hip) and the float32 error bounds the GPU tests hold the
kernels to.  Everything takes and returns CPU tensors; float32 inputs are widened exactly.

Formulae (include/egc_hip.h), with logit[t, g, c] = b_t[c] + sum_k x[g, k] W_t[c, k]:
    lse = log sum_c exp(logit),  loss = sum_{g, t} (lse - logit[y]) / (G T),  grad = s (exp(logit - lse) - [c == y]),
    s = grad_loss / (G T),  d_W_t = grad_t^T x,  d_b_t = sum_g grad_t,  d_x = sum_t grad_t W_t;
a label outside [0, V) contributes 0 to the loss (and still counts in G T) and a zero gradient row.

Bounds.  u = 2^-24, gamma_n = n u / (1 - n u), C = V.  None of them is fitted to an observed error.
  logit   The kernel's logit is one fma chain of K exact products (the padding products are exact zeros) and one add of the
          bias: K + 1 roundings, |err| <= gamma_{K+1} (sum_k |x_k w_k| + |b|) =: E[t, g, c].
  lse     lse is 1-Lipschitz in the largest logit error, so the logits' errors shift it by at most max_c E.  On top, the
          argument of tests/test_softmax_gpu.py with one change: the kernel sums exp(logit - m_i) inside a slab of 64 columns
          (m_i the slab's maximum) and then sum_i s_i exp(m_i - M).  The two differences round with u |logit - m_i| and
          u |m_i - M|, together u |logit - M| (both have the same sign), whose softmax-weighted mean is at most ln C as there;
          there are two expf (3u each) and one product (u) per term instead of one expf: 7u instead of 3u; the C positive terms
          add up within gamma_{C-1} in ANY order (zeros add exactly); logf adds 3u ln C and m + log s rounds once:
              |err| <= max_c E + u (|lse| + 4 ln C + 7) + (C - 1) u.
  loss    term = lse - logit[y] carries lse's bound, E[y] and one rounding u |term|.  The documented order of the sum has a
          longest chain of k = ceil(G T / 256) + 3 + 6 adds: gamma_k sum |term|; the quotient by float(G T) (exact below 2^24)
          rounds once.  1.01 covers the second-order terms, as in softmax_ref.loss_bound.
  grad    p = exp(logit - lse): the argument carries E, lse's bound and its own rounding u |logp|, all of which become relative
          errors of p; expf adds 3u; p - [c == y] rounds once, s = grad_loss / float(G T) once, the product once:
              |err| <= |s| (p (E + lse_bound + u |logp| + 3u) + 3u |p - onehot|) 1.01 + TINY (1 + |s|) =: e[t, g, c]
          (TINY: the subnormal range, as softmax_ref.nll_grad_bound).
  d_b     a sum of G terms in float32 (a block's rows ascending, blocks ascending): sum_g e + gamma_G sum_g |grad|.
  d_W     products exact inside the fma chain over the rows, one more add per later row block:
          sum_g e |x| + gamma_{G+2} sum_g |grad x|.
  d_x     an fma chain over a workgroup's columns, then the partial arrays: every term passes through fewer than T V adds
          whatever the split: sum_{t, c} e |W| + gamma_{T V} sum |grad W|.
Each gradient bound adds TINY for sums that end in the subnormal range."""
import math

import torch

from softmax_ref import TINY, U


def gamma(n):
    return n * U / (1.0 - n * U)


def loss_chain(n_rows, seq_len):
    """The longest chain of float32 adds behind the loss (include/egc_hip.h)."""
    return (n_rows * seq_len + 255) // 256 + 3 + 6


def make_inputs(g, k, v, t, kind, seed):
    """CPU float32 (x [g, k], weights, biases, y [g, t]).  Weights ~ N(0, 1 / k), so a row of x of scale s gives logits of
    standard deviation s.  "mixed": row scales 1, 10, 0 (the logits are the biases) and 3 in turn; "large": scale 10, logits
    spread over +-30 and more."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g, k, generator=gen)
    scale = torch.tensor([1.0, 10.0, 0.0, 3.0])[torch.arange(g) % 4] if kind == "mixed" else torch.full((g,), 10.0)
    x = x * scale[:, None]
    ws = [torch.randn(v, k, generator=gen) / math.sqrt(k) for _ in range(t)]
    bs = [0.1 * torch.randn(v, generator=gen) for _ in range(t)]
    y = torch.randint(0, v, (g, t), generator=gen)
    return x, ws, bs, y


def first_argmax(logits):
    """[G, T] first maximal column of logits [T, G, V]."""
    v = logits.size(2)
    cols = torch.arange(v).expand_as(logits)
    return torch.where(logits == logits.max(dim=2, keepdim=True).values, cols, v).min(dim=2).values.t().contiguous()


def reference(x, ws, bs, y=None, grad_loss=1.0):
    """A dict of the float64 results and their float32 bounds: logits / logit_bound [T, G, V], lse / lse_bound [G, T], and
    with y: loss / loss_bound (floats), dx / dx_bound [G, K], dw / dw_bound and db / db_bound (lists of T)."""
    x64 = x.double()
    g, k = x.shape
    t, v = len(ws), ws[0].size(0)
    w64 = [w.double() for w in ws]
    logits = torch.stack([x64 @ w.t() + b.double() for w, b in zip(w64, bs)])
    absdot = torch.stack([x64.abs() @ w.abs().t() + b.double().abs() for w, b in zip(w64, bs)])
    lb = gamma(k + 1) * absdot
    if g:
        m = logits.max(dim=2, keepdim=True).values
        lse = (m + (logits - m).exp().sum(dim=2, keepdim=True).log()).squeeze(2)
        lb_max = lb.max(dim=2).values
    else:
        lse = lb_max = logits.new_zeros((t, 0))
    lse_b = lb_max + U * (lse.abs() + 4.0 * math.log(v) + 7.0) + (v - 1) * U
    out = dict(logits=logits, logit_bound=lb, logit_bound_row=lb_max.t(), lse=lse.t().contiguous(),
               lse_bound=lse_b.t().contiguous())
    if y is None:
        return out
    n = g * t
    yt = y.t()
    ok = (yt >= 0) & (yt < v)
    ys = yt.clamp(0, v - 1)[..., None]
    zero = torch.zeros((), dtype=torch.float64)
    term = torch.where(ok, lse - logits.gather(2, ys).squeeze(2), zero)
    term_err = torch.where(ok, lse_b + lb.gather(2, ys).squeeze(2) + U * term.abs(), zero)
    loss = float(term.sum()) / n if n else float("nan")
    out["loss"] = loss
    out["loss_bound"] = (1.01 * (float(term_err.sum()) + (loss_chain(g, t) + 1) * U * float(term.abs().sum())) / max(n, 1)
                         + U * abs(loss if n else 0.0))
    s = float(grad_loss) / n if n else 0.0
    logp = logits - lse[..., None]
    p = logp.exp()
    d = p.clone()
    d.scatter_add_(2, ys, -torch.ones_like(ys, dtype=torch.float64))
    d = d * ok[..., None]
    grad = s * d
    e = (abs(s) * (p * (lb + lse_b[..., None] + U * logp.abs() + 3.0 * U) + 3.0 * U * d.abs()) * 1.01 * ok[..., None]
         + TINY * (1.0 + abs(s)))
    xa = x64.abs()
    out["dx"] = sum(grad[i] @ w64[i] for i in range(t))
    out["dx_bound"] = sum(e[i] @ w64[i].abs() + gamma(t * v) * (grad[i].abs() @ w64[i].abs()) for i in range(t)) + TINY
    out["dw"] = [grad[i].t() @ x64 for i in range(t)]
    out["dw_bound"] = [e[i].t() @ xa + gamma(g + 2) * (grad[i].abs().t() @ xa) + TINY for i in range(t)]
    out["db"] = [grad[i].sum(dim=0) for i in range(t)]
    out["db_bound"] = [e[i].sum(dim=0) + gamma(max(g, 1)) * grad[i].abs().sum(dim=0) + TINY for i in range(t)]
    return out


def torch_composition(x, ws, bs, y):
    """The reference's expression (code/models.py:121-125 with code/configs.py:94) on whatever dtype and device it is given."""
    import torch.nn.functional as F
    return sum(F.cross_entropy(F.linear(x, w, b), y[:, i]) for i, (w, b) in enumerate(zip(ws, bs))) / len(ws)
