"""Float64 reference of the graph-level MLP head (egc_amd/csrc/egc_head.hip), stage by stage, and the float32 bounds the GPU
tests hold the kernels to.  Everything takes and returns CPU tensors; float32 inputs are widened exactly.

Every stage is evaluated from the DEVICE'S OWN inputs to that stage (the z_l, affine_l, g_l, coef_l and dz_l the previous
launch wrote), so a bound covers only the roundings of one launch, and the ReLU decision -- the float32 expression
fl(fl(z * scale) + shift) > 0 -- is formed here from the same float32 numbers with a separately rounded multiply and add
(``pre32``): it is the kernel's decision bit for bit, no mask can differ and no element is left out of a comparison.

Bounds.  u = 2^-24, gamma_n = n u / (1 - n u), TINY covers results that end in the subnormal range.  None is fitted to an
observed error.
  linear   z = a W^T + b: one fma chain of K exact products and one add of the bias, K + 1 roundings:
           |err| <= gamma_{K+1} (sum_k |a_k w_k| + |b|).
  stats    float64 sums of float32 values (exact squares): the budgets of tests/test_bn_tail_gpu.py -- a chain of L adds
           (16 rows of a block, ceil(blocks / 8) partials of a lane, 8 lanes) errs by k = max(4, 2 sqrt(L)) units of 2^-52 of
           E|z| (mean) and E[z^2] (variance); rstd inherits the variance's through -rstd^3 / 2; scale and shift one float32 ulp
           from their float64 values plus what the statistics' budgets propagate.
  running  against nn.BatchNorm1d in float64: one float32 rounding (half an ulp) and as much again for the statistics.
  loss     float64 terms from float32 operands, float64 sums, ONE rounding to float32: u |loss| + 2^-40 mean |term| (the
           float64 exp / log1p and the sums, a few units of 2^-53 each).  The count is exact.
  d out    float64, one rounding: u |ref| + 2^-40 |scale|.
  d a      d a = dz W: one fma chain of N exact products: gamma_N sum_n |dz_n w_n|; g = d a where pre32 > 0, else 0.
  coef     sum g and sum g z in float64 as the statistics; d gamma, d beta and the three coefficients are float64
           expressions rounded once: 2u |ref| + 2^-40 of the terms added (test_bn_tail_gpu._check_backward), which reach c_h
           and c_1 through the two sums.
  dz       fl(fl(fl(c_g g) + fl(c_h z)) + c_1) from the device's own float32 coefficients: four roundings, each within the
           terms: 3 u (|c_g g| + |c_h z| + |c_1|) (1.01 for the second order).
  d W, d b one chain over all G rows: gamma_G sum_g |dz a| and gamma_G sum_g |dz|.
  eval     no stage is exposed (one launch), so the bound is propagated: e_z = e_a |W|^T + gamma_{K+1} (|a| |W|^T + |b|);
           relu is 1-Lipschitz: e_a = |scale| e_z + 1.01 u (3 |z scale| + 2 |shift|) (scale and shift are rounded once from
           float64, the multiply and the add once each).

The dispatch, restated as data (``ROW_TILE`` .. ``launches``): every (G, widths) in the envelope is served by the same
tiling -- a row block is 16 rows; the forward's grid is row blocks x 64-column tiles; the last block adds the row blocks'
partials in 8 lanes (64 for the loss); the parameter gradients stage 256 rows at a time in 16 x 16 tiles."""
import math

import torch

U = 2.0 ** -24
U64 = 2.0 ** -53
TINY = 2.0 ** -126
LOSS_NONE, LOSS_L1, LOSS_BCE = 0, 1, 2

# ---- the tiling -------------------------------------------------------------------------------------------------------------
ROW_TILE = 16            # rows of a block (EGC_HEAD_ROW_TILE)
COL_TILE = 64            # output columns of a forward block
PARTIAL_LANES = 8        # lanes that add the row blocks' column partials
LOSS_LANES = 64          # lanes that add the row blocks' loss partials
PARAM_CHUNK = 256        # rows the parameter-gradient launch stages at a time
MAX_WIDTH, MAX_OUT, MAX_ROWS, MAX_LINEARS = 384, 64, 65536, 4

# one below / at / above: a row block; a second row block; the 8 partial lanes (8 x 16 rows); the staged chunk
ROW_BOUNDARIES = [15, 16, 17, 31, 32, 33, 127, 128, 129, 255, 256, 257]
LOSS_LANE_ROWS = [LOSS_LANES * ROW_TILE, LOSS_LANES * ROW_TILE + 1]      # 64 row blocks / the 65th


def grid(g, sizes, layer):
    """(row blocks, column tiles) of the training forward's launch of Linear ``layer`` (0-based)."""
    return -(-g // ROW_TILE), -(-sizes[layer + 1] // COL_TILE)


def launches(sizes, kind, want_dx=True, want_params=True, train=True):
    """(forward, backward) launch counts of one call (include/egc_hip.h)."""
    n_lin = len(sizes) - 1
    if not train:
        return 1, 0
    rows = n_lin
    if kind == LOSS_NONE and n_lin == 1 and not want_dx:
        rows = 0                               # the top pass has nothing to form
    if not want_dx and not want_params:
        return n_lin, 0
    return n_lin, rows + (1 if want_params else 0)


def gamma(n):
    return n * U / (1.0 - n * U)


def chain(g):
    """The longest chain of float64 adds behind a column total."""
    return ROW_TILE + -(-(-(-g // ROW_TILE)) // PARTIAL_LANES) + PARTIAL_LANES


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def make_case(sizes, g, seed, kind=LOSS_NONE, all_nan=False):
    """CPU float32 inputs of one case: x [g, K0] with row scales 1, 10, 0 and 3 in turn and column 0 constant; Linear weights
    ~ N(0, 1 / K) and biases, BatchNorm gamma / beta; hidden unit 0 of the first layer reads the constant column only, so its
    batch variance is 0 but for rounding.  y: L1 -> N(0, 1); BCE -> {0, 1} with about 30 % NaN (all NaN on request)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g, sizes[0], generator=gen) * torch.tensor([1.0, 10.0, 0.0, 3.0])[torch.arange(g) % 4][:, None]
    x[:, 0] = 0.75
    ws = [torch.randn(b, a, generator=gen) / math.sqrt(a) for a, b in zip(sizes[:-1], sizes[1:])]
    bs = [0.1 * torch.randn(b, generator=gen) for b in sizes[1:]]
    if len(sizes) > 2:
        ws[0][0].zero_()
        ws[0][0, 0] = 1.0
    gs = [1.0 + 0.1 * torch.randn(b, generator=gen) for b in sizes[1:-1]]
    bes = [0.1 * torch.randn(b, generator=gen) for b in sizes[1:-1]]
    out = sizes[-1]
    if kind == LOSS_BCE:
        y = torch.randint(0, 2, (g, out), generator=gen).float()
        y[torch.rand(g, out, generator=gen) < (2.0 if all_nan else 0.3)] = float("nan")
    else:
        y = torch.randn(g, out, generator=gen)
    return dict(x=x, ws=ws, bs=bs, gammas=gs, betas=bes, y=y)


def load_case(head, case):
    """The case's parameters into a GraphHead / head_mlp (the Sequential's children in order)."""
    import torch.nn as nn
    lin = [m for m in head if isinstance(m, nn.Linear)]
    bn = [m for m in head if isinstance(m, nn.BatchNorm1d)]
    with torch.no_grad():
        for m, w, b in zip(lin, case["ws"], case["bs"]):
            m.weight.copy_(w)
            m.bias.copy_(b)
        for m, g, b in zip(bn, case["gammas"], case["betas"]):
            if m.weight is not None:
                m.weight.copy_(g)
                m.bias.copy_(b)
    return head


# ---- the stages ---------------------------------------------------------------------------------------------------------------
def pre32(z, affine):
    """fl(fl(z * scale) + shift) in float32, the multiply and the add rounded separately: the kernels' ReLU argument."""
    assert z.dtype == torch.float32 and affine.dtype == torch.float32
    return torch.add(torch.mul(z, affine[0]), affine[1])


def act32(z, affine):
    """a = relu(pre32) as the float32 numbers the next launch loads."""
    p = pre32(z, affine)
    return torch.where(p > 0, p, torch.zeros_like(p))


def linear(a, w, b):
    """(z, bound) of z = a W^T + b from the float32 a the launch loaded."""
    a64, w64 = a.double(), w.double()
    k = a.size(1)
    return a64 @ w64.t() + b.double(), gamma(k + 1) * (a64.abs() @ w64.abs().t() + b.double().abs()) + TINY


def stats(z, gamma_, beta, eps):
    """dict of (value, bound) for mean, var, rstd, scale, shift of the columns of the device's z (two-pass float64)."""
    z64 = z.double()
    g = z.size(0)
    mean = z64.mean(0)
    var = ((z64 - mean) ** 2).mean(0)
    rstd = 1.0 / torch.sqrt(var + eps)
    e2, eabs = (z64 ** 2).mean(0), z64.abs().mean(0)
    k = max(4.0, 2.0 * math.sqrt(chain(g)))
    b_mean = k * 2 * U64 * eabs
    b_var = k * 2 * U64 * e2
    b_rstd = 0.5 * rstd ** 3 * b_var + 4 * U64 * rstd
    g64 = gamma_.double() if gamma_ is not None else torch.ones_like(mean)
    be64 = beta.double() if beta is not None else torch.zeros_like(mean)
    ulp = lambda v: torch.finfo(torch.float32).eps * 2.0 ** torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -126)))
    scale = g64 * rstd
    shift = be64 - mean * g64 * rstd
    return dict(mean=(mean, b_mean + 1e-300), var=(var, b_var + 1e-300), rstd=(rstd, b_rstd),
                scale=(scale, ulp(scale) + g64.abs() * b_rstd),
                shift=(shift, ulp(shift) + b_mean * (g64 * rstd).abs() + b_rstd * (mean * g64).abs()))


def loss(out, y, kind):
    """(loss, bound, count) from the device's float32 out."""
    o, t = out.double(), y.double().view_as(out)
    if kind == LOSS_L1:
        term, cnt = (o - t).abs(), float(o.numel())
    else:
        ok = t == t
        t0 = torch.where(ok, t, torch.zeros_like(t))
        term = torch.where(ok, o.clamp(min=0) - o * t0 + torch.log1p(torch.exp(-o.abs())), torch.zeros_like(o))
        cnt = float(ok.sum())
    if cnt == 0:
        return float("nan"), 0.0, 0.0
    val = float(term.sum()) / cnt
    return val, U * abs(val) + 2.0 ** -40 * float(term.abs().sum()) / cnt + TINY, cnt


def d_out(out, y, kind, grad_loss):
    """(d out, bound) of the fused loss from the device's float32 out."""
    o, t = out.double(), y.double().view_as(out)
    if kind == LOSS_L1:
        sc = float(grad_loss) / o.numel()
        ref = torch.sign(o - t) * sc
    else:
        ok = t == t
        cnt = float(ok.sum())
        sc = float(grad_loss) / cnt if cnt else 0.0
        ref = torch.where(ok, (torch.sigmoid(o) - torch.where(ok, t, torch.zeros_like(t))) * sc, torch.zeros_like(o))
    return ref, U * ref.abs() + 2.0 ** -40 * abs(sc) + 2.0 ** -149


def d_act(dz, w, z_lo=None, affine_lo=None):
    """(g or d x, bound): d a = dz W from the device's float32 dz, masked by the layer below's own ReLU decision."""
    d64, w64 = dz.double(), w.double()
    ref = d64 @ w64
    bound = gamma(dz.size(1)) * (d64.abs() @ w64.abs()) + 2.0 ** -149
    if z_lo is not None:
        keep = pre32(z_lo, affine_lo) > 0
        ref, bound = ref * keep, torch.where(keep, bound, torch.full_like(bound, 2.0 ** -149))
    return ref, bound


def coef(g, z, stats_dev, gamma_):
    """dict of (value, bound) for dgamma, dbeta, cg, ch, c1 from the device's float32 g and z and its float64 stats [3][K]."""
    n = z.size(0)
    g64, z64 = g.double(), z.double()
    mean, rstd = stats_dev[0], stats_dev[2]
    s1, sgz = g64.sum(0), (g64 * z64).sum(0)
    s2 = (sgz - mean * s1) * rstd
    a = (gamma_.double() if gamma_ is not None else torch.ones_like(mean)) * rstd
    cg, ch, c1 = a, -(a / n) * rstd * s2, -(a / n) * (s1 - mean * rstd * s2)
    ut = 2.0 ** -40
    t_dg = ((g64 * z64).abs().sum(0) + mean.abs() * g64.abs().sum(0)) * rstd
    t_db = g64.abs().sum(0)
    an = (a / n).abs()
    return dict(dgamma=(s2, 2 * U * s2.abs() + ut * t_dg + 2.0 ** -149), dbeta=(s1, 2 * U * s1.abs() + ut * t_db + 2.0 ** -149),
                cg=(cg, 2 * U * cg.abs() + 2.0 ** -149), ch=(ch, 2 * U * ch.abs() + an * rstd * ut * t_dg + 2.0 ** -149),
                c1=(c1, 2 * U * c1.abs() + an * ut * (t_db + mean.abs() * rstd * t_dg) + 2.0 ** -149))


def dz(g, z, coef_dev):
    """(dz, bound) from the device's g, z and its own float32 coef [5][K]."""
    cg, ch, c1 = coef_dev[2].double(), coef_dev[3].double(), coef_dev[4].double()
    tg, tz = cg * g.double(), ch * z.double()
    return tg + tz + c1, 1.01 * 3 * U * (tg.abs() + tz.abs() + c1.abs()) + 2.0 ** -149


def param_grads(dz_, a):
    """(dW, bound, db, bound) from the device's dz_l and the float32 a_{l-1} its loads form."""
    d64, a64 = dz_.double(), a.double()
    n = max(dz_.size(0), 1)
    return (d64.t() @ a64, gamma(n) * (d64.abs().t() @ a64.abs()) + 2.0 ** -149, d64.sum(0),
            gamma(n) * d64.abs().sum(0) + 2.0 ** -149)


def eval_forward(x, ws, bs, gammas, betas, means, variances, eps):
    """(out, bound) of the evaluation forward with running statistics, the bound propagated through the layers."""
    a, e = x.double(), torch.zeros_like(x, dtype=torch.float64)
    for i, (w, b) in enumerate(zip(ws, bs)):
        w64 = w.double()
        k = w.size(1)
        z = a @ w64.t() + b.double()
        e = e @ w64.abs().t() + gamma(k + 1) * (a.abs() @ w64.abs().t() + b.double().abs()) + TINY
        if i == len(ws) - 1:
            return z, e
        rstd = 1.0 / torch.sqrt(variances[i].double() + eps[i])
        g64 = gammas[i].double() if gammas[i] is not None else torch.ones_like(rstd)
        be64 = betas[i].double() if betas[i] is not None else torch.zeros_like(rstd)
        sc, sh = g64 * rstd, be64 - means[i].double() * g64 * rstd
        e = sc.abs() * e + 1.01 * U * (3 * (z * sc).abs() + 2 * sh.abs()) + TINY
        a = torch.relu(z * sc + sh)


# ---- the whole head in float64 (the CPU tests compare it with torch's composition and autograd) --------------------------------
def head64(case, kind, eps=1e-5, grad=None):
    """Textbook float64 forward and backward of the head in training mode: dict(out, loss, dx, dw, db, dgamma, dbeta)."""
    x = case["x"].double()
    n_lin = len(case["ws"])
    acts, zs, hats, rstds = [x], [], [], []
    for i in range(n_lin):
        z = acts[-1] @ case["ws"][i].double().t() + case["bs"][i].double()
        if i == n_lin - 1:
            out = z
            break
        mean = z.mean(0)
        rstd = 1.0 / torch.sqrt(((z - mean) ** 2).mean(0) + eps)
        hat = (z - mean) * rstd
        zs.append(z)
        hats.append(hat)
        rstds.append(rstd)
        acts.append(torch.relu(hat * case["gammas"][i].double() + case["betas"][i].double()))
    res = dict(out=out)
    if kind == LOSS_NONE:
        d = grad.double()
    else:
        res["loss"] = loss(out, case["y"], kind)[0]
        d = d_out(out, case["y"], kind, 1.0)[0]
    n = x.size(0)
    dw, db, dg, dbe = [None] * n_lin, [None] * n_lin, [None] * (n_lin - 1), [None] * (n_lin - 1)
    for i in range(n_lin - 1, -1, -1):
        dw[i] = d.t() @ acts[i]
        db[i] = d.sum(0)
        da = d @ case["ws"][i].double()
        if i == 0:
            res["dx"] = da
            break
        gm = case["gammas"][i - 1].double()
        g = da * (hats[i - 1] * gm + case["betas"][i - 1].double() > 0)
        dg[i - 1] = (g * hats[i - 1]).sum(0)
        dbe[i - 1] = g.sum(0)
        d = gm * rstds[i - 1] * (g - (dbe[i - 1] + hats[i - 1] * dg[i - 1]) / n)
    res.update(dw=dw, db=db, dgamma=dg, dbeta=dbe)
    return res


def torch_composition(head, x, y, kind):
    """The reference's expression on whatever dtype and device it is given: head is the nn.Sequential."""
    import torch.nn.functional as F
    out = torch.nn.Sequential.forward(head, x)
    if kind == LOSS_NONE:
        return out
    if kind == LOSS_L1:
        return F.l1_loss(out, y.view_as(out))
    t = y.view_as(out)
    ok = t == t
    return F.binary_cross_entropy_with_logits(out[ok], t[ok])


# ---- the GPU cases: a sparse product of the issue's widths and row counts --------------------------------------------------------
SIZES = [[128, 64, 32, 1], [168, 84, 42, 1], [300, 150, 75, 1], [304, 152, 76, 10], [384, 192, 96, 10], [4, 2, 1, 1], [36, 1],
         [40, 20, 1], [64, 32, 16, 8, 3]]
ROWS = [2, 15, 17, 128, 200] + [r for r in ROW_BOUNDARIES if r not in (15, 17, 128)] + LOSS_LANE_ROWS


def gpu_cases():
    """[(sizes, G, kind)]: every width list and every row count at least once, the loss kinds in turn; one case at 2,048."""
    cases = []
    for i, g in enumerate(ROWS):
        cases.append((SIZES[i % len(SIZES)], g, (LOSS_L1, LOSS_BCE, LOSS_NONE)[i % 3]))
    for i, s in enumerate(SIZES):
        g = ROWS[(3 * i + 4) % len(ROWS)]
        kind = (LOSS_BCE, LOSS_NONE, LOSS_L1)[i % 3]
        if (s, g, kind) not in cases:
            cases.append((s, g, kind))
    cases.append(([296, 148, 74, 1], 2048, LOSS_BCE))
    return cases
