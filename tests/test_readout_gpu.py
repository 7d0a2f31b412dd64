"""The graph-level readouts -- egc_amd.global_add_pool / global_mean_pool / global_max_pool, egc_amd.readout(name), and the C
entry points under them (egc_segment_reduce_f32 / egc_segment_reduce_backward_f32) -- against the sequential float32 loop on
the CPU (tests/readout_ref.py), bit for bit: forward, the max readout's arg, and the gradient through .backward().  No
tolerance appears anywhere: the kernels sum in input order and give a tie to the first row in input order, so the result is a
pure function of the input.  No comparison with torch's device scatter, whose order is not fixed and whose amax backward
splits a tie."""
import functools

import pytest
import torch
import torch.nn as nn

import readout_ref as ref

pytestmark = pytest.mark.gpu

OPS = ["sum", "mean", "max"]


def _dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _batch_vector(workload):
    from egc_amd import workloads as wl
    if workload == "zinc200":
        return wl.zinc_like_batch(200)[3]
    if workload == "molecule2048":
        return wl.molecule_batch(2048)[2]
    if workload == "knn256":
        return wl.knn_superpixel_batch(256)[2]
    raise KeyError(workload)


def _check_pool(op, x, batch, size, n_graphs=None):
    """forward, arg (max) and the gradient through .backward(go) of egc_amd.readout(op) on the GPU against the CPU loop."""
    import egc_amd
    from egc_amd import functional as F
    dev = _dev()
    n_graphs = (int(batch.max()) + 1 if batch.numel() else 0) if size is None else size
    seg = ref.seg_ptr_of(batch, n_graphs)
    want, want_arg = ref.forward(x, seg, op)
    xg = x.clone().to(dev).requires_grad_(True)
    out = egc_amd.readout(op)(xg, batch.to(dev), size)
    assert out.shape == want.shape and out.dtype == torch.float32
    assert torch.equal(out.detach().cpu(), want), (op, "forward")
    if op == "max":
        got, got_arg = F.segment_reduce(xg.detach(), seg.to(dev), "max", want_arg=True)
        assert got_arg.dtype == torch.int32
        assert torch.equal(got.cpu(), want) and torch.equal(got_arg.cpu(), want_arg), (op, "arg")
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(5))
    out.backward(go.to(dev))
    want_dx = ref.backward(go, seg, op, x.size(0), want_arg)
    assert xg.grad.shape == x.shape
    assert torch.equal(xg.grad.cpu(), want_dx), (op, "backward")
    # without autograd the same kernel answers
    with torch.no_grad():
        assert torch.equal(egc_amd.readout(op)(xg.detach(), batch.to(dev), size).cpu(), want)
    return want, want_arg, want_dx


# 1. the batch workloads at the widths of the reference's nets (77: the scalar form of the kernels)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("width", [128, 168, 296, 77])
@pytest.mark.parametrize("workload", ["zinc200", "molecule2048", "knn256"])
def test_readout_equals_the_sequential_loop(workload, width, op):
    batch = _batch_vector(workload)
    x = torch.randn(batch.numel(), width, generator=torch.Generator().manual_seed(width))
    _check_pool(op, x, batch, None)


# 2. ties: the first row in input order wins, and it alone receives the gradient
@pytest.mark.parametrize("op", OPS)
def test_ties_go_to_the_first_row_in_input_order(op):
    from egc_amd import workloads as wl
    batch = wl.zinc_like_batch(200, seed=2)[3]
    n_graphs = int(batch.max()) + 1
    x = torch.randint(-3, 4, (batch.numel(), 128), generator=torch.Generator().manual_seed(2)).to(torch.float32)
    # the case tests what it is for: at least half of the (segment, column) pairs have several rows at the maximum
    seg = ref.seg_ptr_of(batch, n_graphs)
    mx = ref.forward(x, seg, "max")[0]
    at_max = torch.zeros(n_graphs, 128).index_add_(0, batch, (x == mx[batch]).to(torch.float32))
    assert float((at_max >= 2).to(torch.float32).mean()) >= 0.5
    _, arg, dx = _check_pool(op, x, batch, None)
    if op == "max":
        assert int((dx != 0).sum(0).max()) <= n_graphs          # at most one row per (segment, column) has a gradient
        first = torch.full((n_graphs, 128), x.size(0), dtype=torch.int64)
        rows = torch.arange(x.size(0))[:, None].expand_as(x)
        first.scatter_reduce_(0, batch[:, None].expand_as(x), torch.where(x == mx[batch], rows, x.size(0)), "amin")
        assert torch.equal(arg.long(), first)


# 3. edges of the contract
@pytest.mark.parametrize("op", OPS)
def test_trailing_empty_graphs(op):
    batch = _batch_vector("zinc200")[:600]
    n = int(batch.max()) + 1
    x = torch.randn(600, 128, generator=torch.Generator().manual_seed(3))
    want, arg, dx = _check_pool(op, x, batch, n + 3)
    assert want.shape[0] == n + 3 and not want[n:].any()
    if op == "max":
        assert bool((arg[n:] == -1).all())


@pytest.mark.parametrize("op", OPS)
def test_no_rows_at_all(op):
    x = torch.randn(5, 128)[:0]
    want, arg, dx = _check_pool(op, x, torch.zeros(0, dtype=torch.int64), 2)
    assert want.shape == (2, 128) and not want.any() and dx.shape == (0, 128)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("rows", [1, 37])
def test_a_single_graph(op, rows):
    x = torch.randn(rows, 168, generator=torch.Generator().manual_seed(rows))
    _check_pool(op, x, torch.zeros(rows, dtype=torch.int64), None)
    _check_pool(op, x, torch.zeros(rows, dtype=torch.int64), 1)


@pytest.mark.parametrize("op", OPS)
def test_segments_of_one_row_and_leading_empty_graphs(op):
    sizes = torch.tensor([1, 1, 9, 1, 8, 17, 1])
    batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes) + 2          # graphs 0 and 1 have no rows
    x = torch.randn(batch.numel(), 128, generator=torch.Generator().manual_seed(7))
    want, arg, _ = _check_pool(op, x, batch, None)
    assert not want[:2].any()
    _check_pool(op, x, batch, int(sizes.numel()) + 2)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("width", [128, 77])
def test_rows_outside_every_segment_get_a_zero_gradient(op, width):
    """The C-level wrappers take any seg_ptr: here the first 3 and the last 5 rows lie in no segment."""
    from egc_amd import functional as F
    dev = _dev()
    n_rows = 30
    seg = torch.tensor([3, 10, 10, 11, 25], dtype=torch.int64)
    x = torch.randn(n_rows, width, generator=torch.Generator().manual_seed(9))
    want, want_arg = ref.forward(x, seg, op)
    if op == "max":
        out, arg = F.segment_reduce(x.to(dev), seg.to(dev), op, want_arg=True)
        assert torch.equal(arg.cpu(), want_arg)
    else:
        out, arg = F.segment_reduce(x.to(dev), seg.to(dev), op), None
    assert torch.equal(out.cpu(), want)
    go = torch.randn(want.shape, generator=torch.Generator().manual_seed(10))
    dx = F.segment_reduce_backward(go.to(dev), seg.to(dev), op, n_rows, arg).cpu()
    assert torch.equal(dx, ref.backward(go, seg, op, n_rows, want_arg))
    assert not dx[:3].any() and not dx[25:].any() and dx[3:25].any()


# 4. one long segment: one group of lanes walks it -- correct and slow
@pytest.mark.parametrize("op", OPS)
def test_one_long_segment(op):
    x = torch.randn(40000, 128, generator=torch.Generator().manual_seed(4))
    _check_pool(op, x, torch.zeros(40000, dtype=torch.int64), 1)


# 5. the mean readout keeps its bits
@pytest.mark.parametrize("width", [128, 168, 77])
def test_mean_through_the_new_entry_equals_segment_mean(width):
    import egc_amd
    from egc_amd import functional as F
    dev = _dev()
    batch = _batch_vector("molecule2048")
    n_graphs = int(batch.max()) + 1
    seg = ref.seg_ptr_of(batch, n_graphs).to(dev)
    x = torch.randn(batch.numel(), width, generator=torch.Generator().manual_seed(width + 1)).to(dev)
    old = F.segment_mean(x, seg)
    assert torch.equal(F.segment_reduce(x, seg, "mean"), old)
    assert torch.equal(egc_amd.global_mean_pool(x, batch.to(dev)), old)
    assert torch.equal(old.cpu(), ref.forward(x.cpu(), seg.cpu(), "mean")[0])


def test_global_mean_pool_gradient_equals_the_sequential_reference():
    import egc_amd
    dev = _dev()
    batch = _batch_vector("zinc200")
    n_graphs = int(batch.max()) + 1
    x = torch.randn(batch.numel(), 128, generator=torch.Generator().manual_seed(12))
    go = torch.randn(n_graphs, 128, generator=torch.Generator().manual_seed(13))
    xg = x.to(dev).requires_grad_(True)
    egc_amd.global_mean_pool(xg, batch.to(dev), n_graphs).backward(go.to(dev))
    counts = torch.bincount(batch, minlength=n_graphs).clamp(min=1).to(torch.float32)
    assert torch.equal(xg.grad.cpu(), (go / counts[:, None])[batch])


# 6. the readout inside a net
@pytest.mark.parametrize("name", ["mean", "sum", "max"])
def test_readout_inside_a_training_step_of_the_zinc_net(name):
    """tests/callers.py's ZincNetLike with FusedEGCBlock blocks on a GraphBatch (d = 128, H = 8, B = 4: the configuration whose
    blocks tests/test_determinism_gpu.py shows bit-reproducible without a readout) and pool = egc_amd.readout(name)."""
    import egc_amd
    from egc_amd import workloads as wl
    from callers import ZincNetLike, zinc_loss
    dev = _dev()
    atom, ei, n, bvec = wl.zinc_like_batch(128, seed=0)
    n_graphs = int(bvec.max()) + 1
    torch.manual_seed(0)
    net = ZincNetLike(128, 4, lambda d: egc_amd.EGConv(d, d, aggrs=["sum", "mean", "max", "symnorm"], num_heads=8, num_bases=4),
                      residual=True).to(dev).train()
    blocks = {}

    def fuse(conv, bn, residual):
        if id(conv) not in blocks:
            blocks[id(conv)] = egc_amd.FusedEGCBlock(conv, bn, relu=True, residual=residual)
        blocks[id(conv)].train(bn.training)
        return blocks[id(conv)]

    kept = {}

    def pool(x, b, k):
        x.retain_grad()
        y = egc_amd.readout(name)(x, b, k)
        y.retain_grad()
        kept["x"], kept["y"] = x, y
        return y

    atom, ei, batch = atom.to(dev), ei.to(dev), bvec.to(dev)
    sizes = torch.bincount(batch)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(sizes, 0)])
    y = torch.randn(n_graphs, generator=torch.Generator().manual_seed(1)).to(dev)
    params = list(net.parameters())

    def step():
        for p in params:
            p.grad = None
        gb = egc_amd.GraphBatch(ei, ptr=ptr, max_nodes=int(sizes.max()), num_nodes=n)
        loss = zinc_loss(net(atom, gb, batch, n_graphs, fuse=fuse, pool=pool), y)
        loss.backward()
        gb.check()
        return loss.item(), [p.grad.detach().clone() for p in params]

    loss, grads = step()
    assert loss == loss and abs(loss) != float("inf")
    seg = ref.seg_ptr_of(bvec, n_graphs)
    entered, pooled = kept["x"].detach().cpu(), kept["y"].detach().cpu()
    want, want_arg = ref.forward(entered, seg, name)
    assert torch.equal(pooled, want)
    assert torch.equal(kept["x"].grad.cpu(), ref.backward(kept["y"].grad.cpu(), seg, name, n, want_arg))
    loss2, grads2 = step()
    assert loss2 == loss
    for (p, _), a, b in zip(net.named_parameters(), grads, grads2):
        assert torch.equal(a, b), f"gradient of {p} differs between two identical steps"


# 7. inside a recorded step
@pytest.mark.parametrize("op", OPS)
def test_readout_inside_a_recorded_step(op):
    """loss = head(readout(block(x))) recorded by egc_amd.GraphedStep with `size` given (nothing read back to the host): each
    replay on fresh contents of the static buffers gives the eager call's pooled output and d x, bit for bit."""
    import egc_amd
    from egc_amd import workloads as wl
    from egc_amd.fusion import FusedEGCBlock
    dev = _dev()
    hidden = 64
    _, ei, n, bvec = wl.zinc_like_batch(64, seed=3)
    n_graphs = int(bvec.max()) + 1
    ei, batch = ei.to(dev), bvec.to(dev)
    torch.manual_seed(0)
    block = FusedEGCBlock(egc_amd.EGConv(hidden, hidden, aggrs=["sum", "max", "symnorm"], num_heads=4, num_bases=4),
                          nn.BatchNorm1d(hidden)).to(dev).train()
    head = nn.Linear(hidden, 1).to(dev)
    graph = egc_amd.CSRGraph.from_edge_index(ei, n).trim_launches()
    x = torch.randn(n, hidden, device=dev).requires_grad_(True)
    leaves = list(block.parameters()) + list(head.parameters()) + [x]
    kept = {}

    def step():
        kept["pooled"] = egc_amd.readout(op)(block(x, graph), batch, size=n_graphs + 1)     # (+ one trailing empty graph)
        (head(kept["pooled"]) ** 2).sum().backward()

    graphed = egc_amd.GraphedStep(step, params=leaves)
    recorded = kept["pooled"]                                # the recording's output buffer
    for trial in range(3):
        with torch.no_grad():
            x.copy_(torch.randn(n, hidden, device=dev))      # new contents of the static buffer
        graphed()
        got_pooled, got_dx = recorded.detach().clone(), x.grad.detach().clone()
        held = [p.grad for p in leaves]
        for p in leaves:
            p.grad = None
        step()
        assert torch.equal(got_pooled, kept["pooled"].detach()), (op, trial, "pooled output")
        assert torch.equal(got_dx, x.grad), (op, trial, "d x")
        assert not got_pooled[n_graphs:].any()
        for p, h in zip(leaves, held):                       # give the recording its gradient buffers back
            p.grad = h
