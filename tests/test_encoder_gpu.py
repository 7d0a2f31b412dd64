"""The node encoders on the GPU -- egc_amd.Embedding / AtomEncoder / ASTNodeEncoder / NodeEncoder and the C entry points
under them (egc_encoder_forward_f32, egc_encoder_backward_f32, egc_encoder_workspace_bytes) -- against the sequential CPU
reference of tests/encoder_ref.py.  The forward is compared bit for bit.  The backward's summation order is fixed but is
not the reference's, so every element of every table gradient is held to the bound that is valid for ANY order of a
float32 sum of k terms, |got - exact| <= gamma_(k-1) * sum |g_i|, gamma_m = m u / (1 - m u), u = 2^-24 (Higham, Accuracy and
Stability of Numerical Algorithms, section 4.2, eq. 4.4), with k and sum |g_i| per destination row from the reference:
rows indexed once are bit-equal to their one gradient row, rows nobody indexes are exactly 0.  That bound alone cannot see
a lost row in a long list (33.8 for the two-row tables of atom-296-uniform, whose largest |g| is 5.45), so next to it the
gradients are compared BIT FOR BIT with encoder_ref.chunked_backward, the float32 restatement of the kernel's documented
order: chunks of 256 nodes, ascending n inside a chunk, ascending chunk after that."""
import copy
import ctypes as C
import functools

import pytest
import torch
import torch.nn as nn

import encoder_ref as ref

pytestmark = pytest.mark.gpu

ATOM_ROWS = [119, 4, 12, 12, 10, 6, 6, 2, 2]
AST_ROWS, AST_CLAMP = [98, 10030, 21], [None, None, 20]
ZINC_ROWS = [28]


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _n_nodes(workload):
    from egc_amd import workloads as wl
    if workload == "molecule2048":
        return wl.molecule_batch(2048)[1]
    if workload == "code128":
        return wl.code_like_batch(128)[1]
    if workload == "zinc128":
        return wl.zinc_like_batch(128)[2]
    raise KeyError(workload)


def _indices(n, rows, dist, seed, beyond=None):
    """int64 [n, T]: uniform over each table, or every node the same row of every table (the longest possible lists).
    ``beyond[t]``: the upper end of table t's draw where it is to exceed the table (depths beyond max_depth)."""
    g = torch.Generator().manual_seed(seed)
    cols = []
    for t, r in enumerate(rows):
        hi = r if beyond is None or beyond[t] is None else beyond[t]
        cols.append(torch.randint(0, hi, (n,), generator=g) if dist == "uniform" else torch.full((n,), (hi - 1) // 2 + (hi > r) * r))
    return torch.stack(cols, dim=1)


def _tables(rows, width, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(r, width, generator=g) for r in rows]


# (name, rows, clamp, draw beyond, workload or n, widths)
SHAPES = [
    ("atom", ATOM_ROWS, None, None, "molecule2048", (128, 224, 296)),
    ("ast", AST_ROWS, AST_CLAMP, [None, None, 60], "code128", (300, 304)),
    ("zinc", ZINC_ROWS, None, None, "zinc128", (128, 168)),
    ("atom76", ATOM_ROWS, None, None, 777, (76,)),
    ("empty", ATOM_ROWS, None, None, 0, (128,)),
    ("one", AST_ROWS, AST_CLAMP, [None, None, 60], 1, (128,)),
]
CASES = [pytest.param(name, rows, clamp, beyond, n, width, dist, id=f"{name}-{width}-{dist}")
         for name, rows, clamp, beyond, n, widths in SHAPES for width in widths for dist in ("uniform", "skewed")]


def _case(rows, clamp, beyond, n, width, dist, seed=11):
    n = _n_nodes(n) if isinstance(n, str) else n
    idx = _indices(n, rows, dist, seed, beyond)
    if clamp is not None and n > 1 and dist == "uniform":
        assert int(idx[:, 2].max()) > clamp[2]         # depths beyond max_depth are in the input
    return idx, _tables(rows, width, seed + 1)


def _assert_grads_within_bound(got, g, idx, rows, clamp, what=""):
    """Every element of every table gradient: |got - ref64| <= gamma_(k-1) * sum |g|; finite; nothing left out."""
    for t, ((s, a, k), d) in enumerate(zip(ref.backward(g, idx, rows, clamp), got)):
        d = d.cpu()
        assert d.shape == s.shape and bool(torch.isfinite(d).all()), (what, t)
        bound = ref.gamma((k - 1).clamp(min=0))[:, None] * a
        err = (d.to(torch.float64) - s).abs()
        worst = float((err - bound).max()) if err.numel() else 0.0
        print(f"{what} table {t}: rows {s.size(0)} max k {int(k.max()) if k.numel() else 0} max err {float(err.max()) if err.numel() else 0.0:.3e} "
              f"max bound {float(bound.max()) if bound.numel() else 0.0:.3e}")
        assert worst <= 0.0, (what, t, worst)
        assert bool((d[k == 0] == 0).all()), (what, t, "rows nobody indexes must be exactly 0")
        assert torch.equal(d[k == 1].to(torch.float64), s[k == 1]), (what, t, "rows indexed once are the one gradient row")


def _assert_grads_equal_the_documented_order(got, g, idx, rows, clamp, what=""):
    """Every table gradient equals the float32 restatement of the kernel's summation order, bit for bit."""
    for t, (d, want) in enumerate(zip(got, ref.chunked_backward(g, idx, rows, clamp))):
        assert torch.equal(d.cpu(), want), (what, t, "not the sum in the documented order")


@pytest.mark.parametrize("name, rows, clamp, beyond, n, width, dist", CASES)
def test_forward_equals_the_cpu_loop(name, rows, clamp, beyond, n, width, dist):
    from egc_amd import functional as F
    dev = _dev()
    idx, tables = _case(rows, clamp, beyond, n, width, dist)
    before = idx.clone()
    got = F.encoder_forward([w.to(dev) for w in tables], idx.to(dev), clamp)
    want = ref.forward(tables, idx, clamp)
    assert got.shape == (idx.size(0), width)
    assert torch.equal(got.cpu(), want)
    assert torch.equal(idx, before)
    F._IndexFlag.poll()         # every index was inside its table (after the clamp): nothing was reported


def test_single_table_takes_a_vector_of_indices():
    from egc_amd import functional as F
    dev = _dev()
    idx, tables = _case(ZINC_ROWS, None, None, "zinc128", 168, "uniform")
    got = F.encoder_forward([tables[0].to(dev)], idx[:, 0].contiguous().to(dev))
    assert torch.equal(got.cpu(), tables[0][idx[:, 0]])
    d = torch.randn(idx.size(0), 168, generator=torch.Generator().manual_seed(2))
    (gw,) = F.encoder_backward(d.to(dev), idx[:, 0].contiguous().to(dev), ZINC_ROWS)
    _assert_grads_within_bound([gw], d, idx, ZINC_ROWS, None, "zinc vector idx")


@pytest.mark.parametrize("name, rows, clamp, beyond, n, width, dist", CASES)
def test_backward_within_the_summation_bound_of_float64(name, rows, clamp, beyond, n, width, dist):
    from egc_amd import functional as F
    dev = _dev()
    idx, _ = _case(rows, clamp, beyond, n, width, dist)
    d = torch.randn(idx.size(0), width, generator=torch.Generator().manual_seed(5))
    got = F.encoder_backward(d.to(dev), idx.to(dev), rows, clamp)
    _assert_grads_within_bound(got, d, idx, rows, clamp, f"{name}-{width}-{dist}")
    _assert_grads_equal_the_documented_order(got, d, idx, rows, clamp, f"{name}-{width}-{dist}")


@pytest.mark.parametrize("name, rows, clamp, beyond, n, width", [("atom", ATOM_ROWS, None, None, "molecule2048", 296),
                                                                   ("ast", AST_ROWS, AST_CLAMP, [None, None, 60], "code128", 304),
                                                                   ("atom76", ATOM_ROWS, None, None, 777, 76)])
def test_backward_with_dropout_mask(name, rows, clamp, beyond, n, width):
    from egc_amd import functional as F
    dev = _dev()
    idx, _ = _case(rows, clamp, beyond, n, width, "uniform")
    gen = torch.Generator().manual_seed(6)
    d = torch.randn(idx.size(0), width, generator=gen)
    keep = (torch.rand(idx.size(0), width, generator=gen) < 0.8).to(torch.uint8)
    scale = 1.0 / (1.0 - 0.2)
    got = F.encoder_backward(d.to(dev), idx.to(dev), rows, clamp, keep.to(dev), scale)
    _assert_grads_within_bound(got, ref.masked_rows(d, keep, scale), idx, rows, clamp, f"{name}-{width}-dropout")
    _assert_grads_equal_the_documented_order(got, ref.masked_rows(d, keep, scale), idx, rows, clamp, f"{name}-{width}-dropout")


def test_backward_is_bit_reproducible():
    from egc_amd import functional as F
    dev = _dev()
    for rows, clamp, beyond, n, width in ((ATOM_ROWS, None, None, "molecule2048", 296), (AST_ROWS, AST_CLAMP, [None, None, 60], "code128", 304)):
        idx, _ = _case(rows, clamp, beyond, n, width, "uniform")
        idx = idx.to(dev)
        d = torch.randn(idx.size(0), width, device=dev)
        first = [g.clone() for g in F.encoder_backward(d, idx, rows, clamp)]
        second = [g.clone() for g in F.encoder_backward(d, idx, rows, clamp)]
        a = torch.randn(2048, 2048, device=dev)
        (a @ a).sum().item()                               # unrelated work on the stream, other contents in the caches
        third = F.encoder_backward(d, idx, rows, clamp)
        for x, y, z in zip(first, second, third):
            assert torch.equal(x, y) and torch.equal(x, z)


def test_backward_writes_every_element():
    from egc_amd import functional as F
    dev = _dev()
    for rows, clamp, n, width in ((ATOM_ROWS, None, 5000, 296), (AST_ROWS, AST_CLAMP, 300, 76), (ATOM_ROWS, None, 0, 128)):
        idx = _indices(n, rows, "uniform", 3).to(dev)
        d = torch.randn(n, width, device=dev)
        out = [torch.full((r, width), float("nan"), device=dev) for r in rows]
        got = F.encoder_backward(d, idx, rows, clamp, out=out)
        for o, g in zip(out, got):
            assert g is o and bool(torch.isfinite(o).all())
        for o, g in zip(out, F.encoder_backward(d, idx, rows, clamp)):
            assert torch.equal(o, g)


def _modules(dev, width=128):
    import egc_amd
    torch.manual_seed(0)
    n = 3000
    x_ast = _indices(n, AST_ROWS, "uniform", 8, [None, None, 60])
    return [
        (egc_amd.Embedding(28, width).to(dev), (_indices(n, ZINC_ROWS, "uniform", 7)[:, 0].to(dev),), ZINC_ROWS, None),
        (egc_amd.AtomEncoder(width).to(dev), (_indices(n, ATOM_ROWS, "uniform", 7).to(dev),), ATOM_ROWS, None),
        (egc_amd.ASTNodeEncoder(width, 98, 10030, 20).to(dev), (x_ast[:, :2].contiguous().to(dev), x_ast[:, 2].contiguous().to(dev)),
         AST_ROWS, AST_CLAMP),
    ]


def test_autograd_through_the_modules_equals_the_direct_call():
    from egc_amd import functional as F
    dev = _dev()
    for mod, inputs, rows, clamp in _modules(dev):
        idx = inputs[0].view(-1, 1) if len(rows) == 1 else torch.cat([inputs[0], inputs[1][:, None]], 1) if len(inputs) == 2 else inputs[0]
        tables = [p.detach() for p in mod.parameters()]
        depth_before = inputs[-1].clone()
        out = mod(*inputs)
        assert torch.equal(out, F.encoder_forward(tables, idx, clamp))
        assert torch.equal(out.cpu(), ref.forward([w.cpu() for w in tables], idx.cpu(), clamp))
        assert torch.equal(inputs[-1], depth_before)
        go = torch.randn_like(out)
        out.backward(go)
        direct = F.encoder_backward(go, idx, rows, clamp)
        for p, g in zip(mod.parameters(), direct):
            assert torch.equal(p.grad, g)
        mod(*inputs).backward(go)                          # a second backward: autograd's own add, g + g = 2 g exactly
        for p, g in zip(mod.parameters(), direct):
            assert torch.equal(p.grad, 2.0 * g)


def test_dropout_in_the_store_and_in_the_backward():
    import egc_amd
    from egc_amd import functional as F
    dev = _dev()
    enc = egc_amd.AtomEncoder(296, dropout=0.25).to(dev)
    idx = _indices(4000, ATOM_ROWS, "uniform", 9).to(dev)
    tables = [p.detach() for p in enc.parameters()]
    base = F.encoder_forward(tables, idx)
    enc.eval()
    assert torch.equal(enc(idx), base) and enc.last_keep_mask is None      # eval mode draws nothing
    enc.train()
    torch.manual_seed(12)
    out = enc(idx)
    keep = enc.last_keep_mask
    assert keep.dtype == torch.uint8 and keep.shape == out.shape
    torch.manual_seed(12)
    assert torch.equal(keep, torch.empty_like(keep).bernoulli_(0.75))      # torch's generator on the device
    assert 0.70 < float(keep.float().mean()) < 0.80
    scale = torch.tensor(1.0 / (1.0 - 0.25), dtype=torch.float32, device=dev)
    assert torch.equal(out, torch.where(keep.bool(), base * scale, torch.zeros((), device=dev)))
    go = torch.randn_like(out)
    out.backward(go)
    got = [p.grad for p in enc.parameters()]
    masked = ref.masked_rows(go.cpu(), keep.cpu(), 1.0 / (1.0 - 0.25))
    _assert_grads_within_bound(got, masked, idx.cpu(), ATOM_ROWS, None, "dropout")
    _assert_grads_equal_the_documented_order(got, masked, idx.cpu(), ATOM_ROWS, None, "dropout")
    plain = egc_amd.AtomEncoder(296, dropout=0.0).to(dev).train()
    plain.load_state_dict(enc.state_dict())
    assert torch.equal(plain(idx), base) and plain.last_keep_mask is None


def test_index_outside_its_table_is_handled_and_reported():
    from egc_amd import functional as F
    dev = _dev()
    F._IndexFlag.poll()
    idx = _indices(1000, ATOM_ROWS, "uniform", 13)
    idx[5, 1] = ATOM_ROWS[1]         # one past the end of table 1
    idx[9, 0] = -1                   # negative index into table 0
    idx[700, 8] = 2 ** 40
    tables = _tables(ATOM_ROWS, 128, 14)
    want = ref.forward(tables, idx, None)        # the reference's rule: such a table contributes a zero row
    rest5 = ref.forward([w for t, w in enumerate(tables) if t != 1], idx[5:6, [t for t in range(9) if t != 1]])
    assert torch.equal(want[5:6], rest5)
    dtab = [w.to(dev) for w in tables]
    got = F.encoder_forward(dtab, idx.to(dev))
    d = torch.randn(1000, 128, generator=torch.Generator().manual_seed(15))
    grads = F.encoder_backward(d.to(dev), idx.to(dev), ATOM_ROWS)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got).all()) and torch.equal(got.cpu(), want)
    _assert_grads_within_bound(grads, d, idx, ATOM_ROWS, None, "bad index")
    with pytest.raises(RuntimeError, match="index outside its embedding table"):
        F.encoder_forward(dtab, idx[:4].to(dev))             # the deferred flag surfaces at the next call
    F.encoder_forward(dtab, idx[:4].to(dev))                 # reported once
    torch.cuda.synchronize()
    F._IndexFlag.poll()


def test_embedding_module_without_gradients_handles_and_reports_a_bad_index():
    """egc_amd.Embedding in eval mode, under no_grad and with frozen weights runs the same kernel as in training: same
    bits, and an index outside the table is never used as an address -- zero row, finite output, deferred flag."""
    import egc_amd
    from egc_amd import functional as F
    dev = _dev()
    F._IndexFlag.poll()
    torch.manual_seed(4)
    emb = egc_amd.Embedding(28, 168).to(dev)
    w = emb.weight.detach().cpu()
    idx = _indices(3000, ZINC_ROWS, "uniform", 17)[:, 0].contiguous()
    want = ref.forward([w], idx)
    train_out = emb(idx.to(dev))
    assert train_out.requires_grad and torch.equal(train_out.detach().cpu(), want)
    emb.eval()
    with torch.no_grad():
        out = emb(idx.to(dev))
    assert not out.requires_grad and torch.equal(out.cpu(), want)
    emb.weight.requires_grad_(False)
    assert torch.equal(emb(idx.to(dev)).cpu(), want)
    F._IndexFlag.poll()                                      # nothing reported so far
    bad = idx.clone()
    bad[7], bad[11], bad[2999] = 28, -3, 2 ** 33
    want = ref.forward([w], bad)
    assert bool((want[[7, 11, 2999]] == 0).all())
    for mode in ("no_grad", "frozen", "train"):
        emb.weight.requires_grad_(mode == "train")
        emb.train(mode == "train")
        if mode == "no_grad":
            with torch.no_grad():
                out = emb(bad.to(dev))
        else:
            out = emb(bad.to(dev))
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all()) and torch.equal(out.detach().cpu(), want), mode
        with pytest.raises(RuntimeError, match="index outside its embedding table"):
            F._IndexFlag.poll()
        F._IndexFlag.poll()


def test_c_abi_workspace_contract():
    from egc_amd import _C
    from egc_amd import functional as F
    dev = _dev()
    lib = _C.load()
    rows, width, n = AST_ROWS, 304, 2000
    idx = _indices(n, rows, "uniform", 21, [None, None, 60]).to(dev)
    tables = [w.to(dev) for w in _tables(rows, width, 22)]
    d = torch.randn(n, width, device=dev)
    c_rows = (C.c_int32 * 3)(*rows)
    c_clamp = (C.c_int32 * 3)(-1, -1, 20)
    stream = torch.cuda.current_stream().cuda_stream
    out = torch.empty(n, width, device=dev)
    ptrs = (C.c_void_p * 3)(*[w.data_ptr() for w in tables])
    assert lib.egc_encoder_forward_f32(ptrs, c_rows, c_clamp, 3, idx.data_ptr(), n, width, None, 1.0, out.data_ptr(), None, stream) == 0
    assert torch.equal(out, F.encoder_forward(tables, idx, AST_CLAMP))
    need = lib.egc_encoder_workspace_bytes(n, 3, sum(rows), width)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    grads = [torch.full((r, width), float("nan"), device=dev) for r in rows]
    gptrs = (C.c_void_p * 3)(*[g.data_ptr() for g in grads])
    args = (d.data_ptr(), None, 1.0, idx.data_ptr(), n, width, c_rows, c_clamp, 3, gptrs, ws.data_ptr())
    assert lib.egc_encoder_backward_f32(*args, need - 1, stream) == 2          # EGC_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(g).all()) for g in grads)                       # and nothing was launched
    assert lib.egc_encoder_backward_f32(*args, need, stream) == 0
    for g, want in zip(grads, F.encoder_backward(d, idx, rows, AST_CLAMP)):
        assert torch.equal(g, want)
    assert lib.egc_encoder_backward_f32(*args[:4], -1, *args[5:], need, stream) == 1      # EGC_ERR_INVALID
    big = (C.c_int32 * 3)(98, (1 << 20) + 1, 21)
    assert lib.egc_encoder_forward_f32(ptrs, big, c_clamp, 3, idx.data_ptr(), n, width, None, 1.0, out.data_ptr(), None, stream) == 4


class _PlainAtomHead(nn.Module):
    """What the parent commit's users run: nine nn.Embedding summed from 0 (ogb's AtomEncoder)."""

    def __init__(self, hidden):
        super().__init__()
        self.atom_embedding_list = nn.ModuleList([nn.Embedding(r, hidden) for r in ATOM_ROWS])

    def forward(self, x):
        out = 0
        for i in range(x.shape[1]):
            out = out + self.atom_embedding_list[i](x[:, i])
        return out


def test_atom_encoder_net_trained_on_padded_batches_through_one_recording():
    """The padded-batch loop of tests/test_hipgraph_gpu.py with egc_amd.AtomEncoder at the head and an [n_pad, 9] index
    buffer (padding rows index row 0 of every table; the masked loss gives them zero gradient): ONE recording replayed
    over six batches.  Replays are bit-reproducible and bit-equal to the eager call of the same padded step; against the
    eager loop on the unpadded batches with plain nn.Embedding modules the parameters after six steps meet that test's
    bound, 1e-4 * max(1, |b|max).  The eager side's index_add_ runs in torch's deterministic order: by default it sums
    with float atomics in arrival order, and six steps of this net carry a last-bit change of one pooled row to anything
    between 1e-5 and 3e-4 in the parameters (three runs of one process on an MI355X: 0.13, 0.10 and 3.1 of the bound, the
    last one failing; in the suite's file order it failed more often than not), while the recorded side's bits never
    moved.  With the fixed order both sides are reproducible: the same figures in every run, the largest 0.08 of its bound."""
    import egc_amd
    from egc_amd import workloads as wl
    from egc_amd.fusion import FusedEGCBlock
    dev = _dev()
    hidden = 64
    torch.manual_seed(0)
    enc = egc_amd.AtomEncoder(hidden).to(dev)
    blocks = nn.ModuleList([FusedEGCBlock(egc_amd.EGConv(hidden, hidden, aggrs=["sum", "max", "symnorm"], num_heads=4, num_bases=4),
                                          nn.BatchNorm1d(hidden)) for _ in range(2)]).to(dev).train()
    head = nn.Linear(hidden, 1).to(dev)
    net = nn.ModuleList([enc, blocks, head])
    plain = _PlainAtomHead(hidden).to(dev)
    plain.load_state_dict(enc.state_dict(), strict=True)
    ref_net = nn.ModuleList([plain, copy.deepcopy(blocks), copy.deepcopy(head)])
    twin = copy.deepcopy(net)                              # the eager call of the same padded step
    data = []
    for k, seed in ((24, 1), (40, 2), (31, 3), (40, 4), (17, 5), (36, 6)):
        _, ei, n, batch = wl.zinc_like_batch(k, seed=seed)
        atom = _indices(n, ATOM_ROWS, "uniform", 100 + seed)
        data.append((atom.to(dev), ei.to(dev), n, batch.to(dev), k, torch.randn(k, 1, device=dev)))
    n_pad = max(d[2] for d in data) + 4
    e_pad = max(d[1].size(1) for d in data) + 8
    g_pad = max(d[4] for d in data) + 1                   # + a spare graph that owns the padding rows

    def forward(net_, atom, ei, batch, n_graphs, counts, n_valid=None):
        emb_, blocks_, head_ = net_
        h = emb_(atom)
        for b in blocks_:
            h = b(h, ei, n_valid=n_valid)
        if n_valid is not None:      # the recorded side: the library's readout (size given: nothing read back)
            pooled = egc_amd.global_mean_pool(h, batch, size=n_graphs)
        else:                        # the eager side: index_add_ in its fixed order (its default here is float atomics)
            was = torch.are_deterministic_algorithms_enabled()
            torch.use_deterministic_algorithms(True)
            try:
                pooled = torch.zeros(n_graphs, hidden, device=dev).index_add_(0, batch, h) / counts
            finally:
                torch.use_deterministic_algorithms(was)
        return head_(pooled)

    s_atom = torch.zeros(n_pad, 9, dtype=torch.int64, device=dev)
    s_ei = torch.full((2, e_pad), n_pad - 1, dtype=torch.int64, device=dev)
    s_batch = torch.full((n_pad,), g_pad - 1, dtype=torch.int64, device=dev)
    s_counts = torch.ones(g_pad, 1, device=dev)
    s_target = torch.zeros(g_pad, 1, device=dev)
    s_gmask = torch.zeros(g_pad, 1, device=dev)
    s_inv_g = torch.ones((), device=dev)
    s_nvalid = torch.zeros((), dtype=torch.int64, device=dev)

    def load(atom, ei, n, batch, k, target):
        s_atom.zero_(); s_atom[:n] = atom
        s_ei.fill_(n_pad - 1); s_ei[:, :ei.size(1)] = ei
        s_batch.fill_(g_pad - 1); s_batch[:n] = batch
        s_counts.fill_(1.0); s_counts[:k, 0] = torch.bincount(batch, minlength=k).float()
        s_target.zero_(); s_target[:k] = target
        s_gmask.zero_(); s_gmask[:k] = 1.0
        s_inv_g.fill_(1.0 / k)
        s_nvalid.fill_(n)

    def make_step(net_, opt_):
        def step():      # the recorded backward WRITES .grad; the eager twin starts from .grad = None: no zero_grad here
            out = forward(net_, s_atom, s_ei, s_batch, g_pad, s_counts, s_nvalid)
            (((out - s_target) ** 2 * s_gmask).sum() * s_inv_g).backward()     # mean over the real graphs
            opt_.step()
        return step

    params = list(net.parameters())
    opt = torch.optim.SGD(params, lr=0.05, foreach=True)
    twin_opt = torch.optim.SGD(list(twin.parameters()), lr=0.05, foreach=True)
    ref_opt = torch.optim.SGD(list(ref_net.parameters()), lr=0.05, foreach=True)
    load(*data[0])
    start = copy.deepcopy(net.state_dict())
    graphed = egc_amd.GraphedStep(make_step(net, opt), params=params, warmup=2)

    def snapshot(net_):
        return [p.grad.clone() for p in net_.parameters()], copy.deepcopy(net_.state_dict())

    def assert_same(a, b):
        for x, y in zip(a[0], b[0]):
            assert torch.equal(x, y)
        for (name, x), (_, y) in zip(a[1].items(), b[1].items()):
            assert torch.equal(x, y), name

    net.load_state_dict(start)                             # (the warm-up runs and the recording pass were real steps)
    graphed()
    first = snapshot(net)
    net.load_state_dict(start)
    graphed()
    second = snapshot(net)
    assert_same(first, second)
    assert any(bool((g != 0).any()) for g in first[0][:9])
    twin.load_state_dict(start)
    make_step(twin, twin_opt)()
    assert_same(first, snapshot(twin))

    net.load_state_dict(start)
    for atom, ei, n, batch, k, target in data:
        load(atom, ei, n, batch, k, target)
        graphed()
        ref_opt.zero_grad(set_to_none=True)
        counts = torch.bincount(batch, minlength=k).float()[:, None]
        out = forward(ref_net, atom, ei, batch, k, counts)
        ((out - target) ** 2).mean().backward()
        ref_opt.step()
    torch.cuda.synchronize()
    for (name, a), (_, b) in zip(net.state_dict().items(), ref_net.state_dict().items()):
        if a.dtype.is_floating_point:
            print(f"{name}: max |a - b| {float((a - b).abs().max()):.3e}  bound {1e-4 * max(1.0, float(b.abs().max())):.3e}")
    for (name, a), (_, b) in zip(net.state_dict().items(), ref_net.state_dict().items()):
        if a.dtype.is_floating_point:
            assert float((a - b).abs().max()) <= 1e-4 * max(1.0, float(b.abs().max())), name
        else:
            assert torch.equal(a, b), name
