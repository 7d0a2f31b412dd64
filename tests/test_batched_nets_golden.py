"""The reference's molhiv, CIFAR and ogbg-code NETS as fixtures (tests/golden/bnets/*.npz: EgcHIVNet, MpnnHIVNet, EgcCifarNet,
EgcCodeNet, MpnnCodeNet -- eval forward, training forward, the training loop's scalar loss, its backward and the BatchNorm
running statistics after that one forward, float32 and float64, captured from the reference by make_golden_batched_nets.py).

CPU: the counterparts of tests/callers.py (same module names: the fixtures' state dicts load with strict=True) over torch's
operators, the CPU restatement of the EGC layer (oracle/egc_torch_ref.py) and of Mpnn (tests/mpnn_ref.py) reproduce the
float64 fixtures to 1e-9 (1e-7 where gcn_norm's float32 constants enter): the counterparts are pinned to the reference, not
to the device code.

GPU: the same counterparts assembled from the device components a user would put there -- egc_amd.AtomEncoder /
ASTNodeEncoder, EfficientGraphConv alone / in FusedEGCBlock / in FusedEGCBlock on a GraphBatch, egc_amd.Mpnn alone / in
FusedEGCBlock, egc_amd.readout(name), GraphHead with the fused masked BCE (mol) or egc_amd.cross_entropy behind it (CIFAR),
TokenHead.loss / .predict (code) -- against the float64 fixtures, every quantity bounded by max(1e-5, 5 x the distance between
the reference's OWN float32 and float64 runs on that fixture), gradients with the denominators of
test_nets_golden.py::test_nets_on_the_hip_layers_match_the_reference_float64.  Then one net per family on the padded
buffers of a BatchCollator (same bounds; every intermediate row finite, padding included), and one of them recorded in a
GraphedStep with the collation inside."""
import json
import os

import numpy as np
import pytest
import torch

import egc_amd
import callers
import head_ref
import mpnn_ref
from golden_util import GOLDEN_DIR
from test_nets_golden import _restated

BNETS = os.path.join(GOLDEN_DIR, "bnets")
with open(os.path.join(BNETS, "MANIFEST.json")) as _f:
    MANIFEST = json.load(_f)
NAMES = sorted(MANIFEST)
_CACHE = {}


def _load(name):
    """(arrays, meta) of a fixture, read once and shared: nothing may write to the arrays."""
    if name not in _CACHE:
        z = {}
        for part in (f"{name}.npz", f"{name}.grad.npz"):
            with np.load(os.path.join(BNETS, part)) as f:
                z.update({k: f[k] for k in f.files})
        _CACHE[name] = (z, json.loads(bytes(z["meta"]).decode()))
    return _CACHE[name]


def _is_mpnn(meta):
    return "aggr" in meta


def _build(meta, device):
    if _is_mpnn(meta):
        make = lambda d: egc_amd.Mpnn(meta["aggr"], d, d)                                           # noqa: E731
    else:
        make = lambda d: egc_amd.EfficientGraphConv(d, d, num_heads=meta["heads"], num_bases=meta["bases"],   # noqa: E731
                                                    softmax_weights=False, aggrs=meta["aggrs"])
    h, n_layers, fam = meta["hidden"], meta["layers"], meta["family"]
    if fam == "mol":
        kw = dict(encoder=egc_amd.AtomEncoder, head=egc_amd.GraphHead) if device else {}
        return callers.HIVNetLike(h, n_layers, make, residual=meta["residual"], **kw)
    if fam == "cifar":
        kw = dict(head=egc_amd.GraphHead) if device else {}
        return callers.CifarNetLike(h, n_layers, make, residual=meta["residual"], **kw)
    kw = dict(encoder=egc_amd.ASTNodeEncoder, head=egc_amd.TokenHead) if device else {}
    return callers.CodeNetLike(h, n_layers, make, meta["n_classes"], meta["seq_len"], residual=meta["residual"], **kw)


def _state(z):
    return {k[len("param:"):]: torch.from_numpy(z[k].copy()) for k in z if k.startswith("param:")}


def _head_sizes(meta):
    h = meta["hidden"]
    return [h, h // 2, h // 4, 1 if meta["family"] == "mol" else 10]


def _label_key(meta):
    return "y_arr" if meta["family"] == "code" else "y"


def _args(z, meta, dev, dtype):
    """(the net's positional inputs up to the batch vector, the labels) of the fixture's batch."""
    t = lambda k: torch.from_numpy(z[f"in:{k}"].copy()).to(dev)                                      # noqa: E731
    x = t("x").to(dtype) if meta["family"] == "cifar" else t("x")
    first = (x, t("node_depth")) if meta["family"] == "code" else (x,)
    y = t(_label_key(meta))
    return first + (t("edge_index"), t("batch")), (y.to(dtype) if y.is_floating_point() else y)


def _want_grad(z, key, shape):
    if f"grad64:{key}" in z:
        return torch.from_numpy(z[f"grad64:{key}"]).double()
    dense = torch.zeros(shape, dtype=torch.float64)                    # stored as (row ids, rows): zero elsewhere
    dense[torch.from_numpy(z[f"grad64:{key}:ids"])] = torch.from_numpy(z[f"grad64:{key}:rows"]).double()
    return dense


def _stat_keys(z):
    return [k[len("stat64:"):] for k in z if k.startswith("stat64:")]


def _rel(a, b):
    b = torch.as_tensor(b).double()
    return float((a.detach().cpu().double() - b).abs().max() / max(1.0, float(b.abs().max())))


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the counterparts are the reference's nets
# ---------------------------------------------------------------------------------------------------------------------
def _cpu_conv(conv, x, edge_index):
    if hasattr(conv, "aggs"):
        return _restated(conv, x, edge_index)
    return mpnn_ref.layer_forward(x, edge_index.numpy(), dict(conv.named_parameters()), conv.towers, conv.aggr)


def _cpu_loss(meta, out, y):
    if meta["family"] == "mol":
        return callers.mol_loss(out, y)
    if meta["family"] == "cifar":
        return torch.nn.functional.cross_entropy(out, y)
    return callers.code_loss(out, y)


def _stacked(out):
    return torch.stack(out, dim=1) if isinstance(out, list) else out


@pytest.mark.parametrize("name", NAMES)
def test_callers_and_restatements_reproduce_the_reference_batched_nets_in_float64(name):
    z, meta = _load(name)
    net = _build(meta, device=False)
    net.load_state_dict(_state(z), strict=True)          # the reference's state dict, key for key
    net = net.double()
    args, y = _args(z, meta, torch.device("cpu"), torch.float64)
    kw = dict(conv_fn=_cpu_conv, pool=callers.POOLS[meta["readout"]])
    net.eval()
    with torch.no_grad():
        out_eval = net(*args, meta["n_graphs"], **kw)
        loss_eval = _cpu_loss(meta, out_eval, y)
    net.train()
    out = net(*args, meta["n_graphs"], **kw)
    loss = _cpu_loss(meta, out, y)
    loss.backward()
    # 1e-9, except where gcn_norm's FLOAT32 constants enter (test_nets_golden.py): 1e-7 there
    tol = 1e-7 if any(a in ("symnorm", "symadd") for a in meta.get("aggrs", ())) else 1e-9
    assert _rel(_stacked(out_eval), z["net_eval64"]) <= tol and _rel(_stacked(out), z["net_train64"]) <= tol
    assert _rel(loss_eval, z["loss_eval64"]) <= tol and _rel(loss, z["loss_train64"]) <= tol
    gscale = meta["grad_scale"]
    for k, p in net.named_parameters():
        assert float((p.grad - _want_grad(z, k, p.shape)).abs().max()) <= tol * max(gscale, 1.0), k
    state = net.state_dict()
    assert _stat_keys(z)
    for k in _stat_keys(z):
        assert _rel(state[k], z[f"stat64:{k}"]) <= tol, k


def test_fixture_sizes_are_inside_their_caps():
    total = 0
    for name in NAMES:
        sizes = [os.path.getsize(os.path.join(BNETS, part)) for part in (f"{name}.npz", f"{name}.grad.npz")]
        assert max(sizes) <= 1 << 20 and sum(sizes) <= 2_000_000, (name, sizes)
        total += sum(sizes)
    assert total <= 10_000_000


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the nets on the device components
# ---------------------------------------------------------------------------------------------------------------------
def _dev():
    return torch.device("cuda:0")


def _launches():
    from egc_amd import _C
    return _C.load().egc_head_launches()


def _fuser():
    blocks = {}

    def fuse(conv, bn, residual):          # one block per (conv, bn) pair, sharing the net's modules
        if id(conv) not in blocks:
            blocks[id(conv)] = egc_amd.FusedEGCBlock(conv, bn, relu=True, residual=residual)
        blocks[id(conv)].train(bn.training)
        return blocks[id(conv)]
    return fuse


def _device_net(z, meta):
    net = _build(meta, device=True)
    net.load_state_dict(_state(z), strict=True)
    return net.to(_dev())


def _step(net, meta, args, y, n_slots, kw, g):
    """Evaluation forward, then ONE training forward + loss + backward, on the heads a user would call; rows [:g] of the pooled
    array go to the head (all of them, or all but the spare graph of a padded batch).  Launch counts of GraphHead asserted."""
    fam, res = meta["family"], {}
    net.eval()
    with torch.no_grad():
        pooled = net.body(*args, n_slots, **kw)[:g]
        n0 = _launches()
        if fam == "code":
            res["out_eval"] = torch.stack(net.token_predictors(pooled), dim=1)
            res["pred"] = net.token_predictors.predict(pooled)
            res["loss_eval"] = net.token_predictors.loss(pooled, y)
        else:
            res["out_eval"] = net.mlp(pooled)
            assert _launches() - n0 == 1                                       # the one-launch evaluation head
            res["loss_eval"] = (egc_amd.masked_bce_with_logits if fam == "mol" else egc_amd.cross_entropy)(res["out_eval"], y)
    net.train()
    for p in net.parameters():
        p.grad = None
    taps = []
    pooled = net.body(*args, n_slots, taps=taps, **kw)[:g]
    n0 = _launches()
    if fam == "mol":
        loss, kind = net.mlp.bce_with_logits_loss(pooled, y), head_ref.LOSS_BCE
    elif fam == "cifar":
        loss, kind = egc_amd.cross_entropy(net.mlp(pooled), y), head_ref.LOSS_NONE
    else:
        loss = net.token_predictors.loss(pooled, y)
    loss.backward()
    if fam != "code":
        assert _launches() - n0 == sum(head_ref.launches(_head_sizes(meta), kind))
    res["loss"], res["taps"] = loss.detach(), taps
    res["stats"] = {k: v.detach().clone() for k, v in net.state_dict().items() if "running_" in k or "num_batches" in k}
    with torch.no_grad():                # the training-mode output of the same pooled rows (after the statistics were kept)
        res["out_train"] = torch.stack(net.token_predictors(pooled.detach()), dim=1) if fam == "code" else net.mlp(pooled.detach())
    return res


def _hold_to_fixture(label, z, meta, net, res):
    """Every quantity against the float64 fixture, within max(1e-5, 5 x the reference's own float32-vs-float64 distance)."""
    worst = {}

    def hold(what, ratio):
        assert ratio == ratio, (what, "NaN")
        worst[what] = max(worst.get(what, 0.0), ratio)

    b_out = max(1e-5, 5.0 * meta["f32_vs_f64_out_train"])
    hold("out_eval", _rel(res["out_eval"], z["net_eval64"]) / max(1e-5, 5.0 * meta["f32_vs_f64_out_eval"]))
    hold("out_train", _rel(res["out_train"], z["net_train64"]) / b_out)
    hold("loss_eval", _rel(res["loss_eval"], z["loss_eval64"]) / max(1e-5, 5.0 * meta["f32_vs_f64_loss_eval"]))
    hold("loss", _rel(res["loss"], z["loss_train64"]) / max(1e-5, 5.0 * meta["f32_vs_f64_loss"]))
    gscale = meta["grad_scale"]
    for k, p in net.named_parameters():
        want = _want_grad(z, k, p.shape)
        bound = max(1e-5, 5.0 * meta["f32_vs_f64_grad"][k])
        wmax = float(want.abs().max())
        # (the denominators of test_nets_golden.py: an analytically zero gradient is held to the net's gradient scale)
        denom = gscale if wmax < 1e-6 * gscale else max(1e-2 * gscale, wmax)
        assert p.grad is not None, k
        hold("grad " + k, float((p.grad.cpu().double() - want).abs().max() / denom) / bound)
    assert _stat_keys(z)
    for k in _stat_keys(z):
        if k.endswith("num_batches_tracked"):
            assert int(res["stats"][k]) == int(z[f"stat64:{k}"]), k
        else:
            hold("stat " + k, _rel(res["stats"][k], z[f"stat64:{k}"]) / max(1e-5, 5.0 * meta["f32_vs_f64_stat"][k]))
    if meta["family"] == "code":
        # arg-max: a column whose float64 logit lies within twice the output bound of the row's float64 maximum
        logits = torch.from_numpy(z["net_eval64"])                                    # [G, T, classes]
        pred = res["pred"].cpu()
        assert pred.shape == logits.shape[:2] and pred.dtype == torch.int64
        gap = logits.max(dim=2).values - logits.gather(2, pred.unsqueeze(2)).squeeze(2)
        share = float((pred == logits.argmax(dim=2)).double().mean())
        print(f"{label}: {share:.4f} of the predictions equal the float64 arg-max, largest gap {float(gap.max()):.3e}")
        hold("argmax", float(gap.max()) / (2.0 * max(1e-5, 5.0 * meta["f32_vs_f64_out_eval"]) * max(1.0, float(logits.abs().max()))))
    top = max(worst, key=worst.get)
    groups = {}
    for k, v in worst.items():
        groups[k.split(" ")[0]] = max(groups.get(k.split(" ")[0], 0.0), v)
    print(f"{label}: worst ratio to bound {worst[top]:.3g} ({top}); " + " ".join(f"{k}={v:.3g}" for k, v in groups.items()))
    assert worst[top] <= 1.0, {k: v for k, v in worst.items() if v > 1.0}
    return worst[top]


def _gpu_cases():
    out = []
    for name in NAMES:
        for fused in ((False, True) if _is_mpnn(MANIFEST[name]) else (False, True, "batch")):
            out.append((name, fused))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name,fused", _gpu_cases())
def test_batched_nets_on_the_device_components_match_the_reference_float64(name, fused):
    """fused False: the layer modules alone, torch's BatchNorm / ReLU / add between them; True: FusedEGCBlock around each (the
    CIFAR net with ``identity=``); "batch": FusedEGCBlock on an egc_amd.GraphBatch (the one-launch paths of a batch)."""
    z, meta = _load(name)
    dev, g = _dev(), meta["n_graphs"]
    net = _device_net(z, meta)
    args, y = _args(z, meta, dev, torch.float32)
    pool = egc_amd.readout(meta["readout"])
    kw = dict(pool=lambda x, batch, n: pool(x, batch, n))
    if fused:
        kw["fuse"] = _fuser()
    gb = None
    if fused == "batch":
        sizes = np.bincount(z["in:batch"], minlength=g)
        gb = egc_amd.GraphBatch(args[-2], batch=args[-1], num_graphs=g, max_nodes=int(sizes.max()))
        args = args[:-2] + (gb, args[-1])
    res = _step(net, meta, args, y, g, kw, g)
    label = f"{name} fused={fused}"
    if gb is not None:
        gb.check()
        ran = sorted({k[-1] for k, v in gb._setups.items() if isinstance(k, tuple) and isinstance(k[-1], str) and v})
        label += f" (batch paths that ran: {','.join(ran)})"
    _hold_to_fixture(label, z, meta, net, res)


PADDED = ["hiv_egc_max", "hiv_mpnn_add", "cifar_egc", "code_egc"]


def _store(z, meta, copies=1):
    """The fixture's batch split into a GraphStore (``copies`` times back to back): node fields are the inputs, graph fields
    the labels.  Returns (store, N, E)."""
    dev, g = _dev(), meta["n_graphs"]
    batch, ei = torch.from_numpy(z["in:batch"].copy()), torch.from_numpy(z["in:edge_index"].copy())
    node_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(batch, minlength=g).cumsum(0)])
    graph_of_edge = batch[ei[0]]
    assert bool((graph_of_edge[1:] >= graph_of_edge[:-1]).all())          # a graph's edges are contiguous, in graph order
    edge_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(graph_of_edge, minlength=g).cumsum(0)])
    ei_local = ei - node_ptr[graph_of_edge]
    n, e = int(node_ptr[-1]), int(edge_ptr[-1])
    node_keys = ("x", "node_depth") if meta["family"] == "code" else ("x",)
    rep = lambda t: torch.cat([t] * copies).contiguous().to(dev)                                    # noqa: E731
    node_fields = {k: rep(torch.from_numpy(z[f"in:{k}"].copy())) for k in node_keys}
    graph_fields = {_label_key(meta): rep(torch.from_numpy(z[f"in:{_label_key(meta)}"].copy()))}
    ptrs = [torch.cat([p] + [p[1:] + (c + 1) * int(p[-1]) for c in range(copies - 1)]).to(dev) for p in (node_ptr, edge_ptr)]
    store = egc_amd.GraphStore(ptrs[0], ptrs[1], torch.cat([ei_local] * copies, dim=1).contiguous().to(dev), node_fields, graph_fields)
    return store, n, e


def _collator(z, meta, copies=1):
    store, n, e = _store(z, meta, copies)
    fill = {"y": float("nan")} if meta["family"] == "mol" else None
    return egc_amd.BatchCollator(store, meta["n_graphs"], n_pad=n + 1 + 37, e_pad=e + 19, graph_fill=fill)


def _padded_call(meta, col):
    """(positional inputs, labels, keywords) of the net on the collator's buffers as they are: n_valid on every block, the
    readout over G + 1 slots."""
    g = meta["n_graphs"]
    first = (col.fields["x"], col.fields["node_depth"]) if meta["family"] == "code" else (col.fields["x"],)
    pool = egc_amd.readout(meta["readout"])
    kw = dict(fuse=_fuser(), n_valid=col.n_valid, pool=lambda x, batch, n: pool(x, batch, size=n))
    return first + (col.edge_index, col.batch), col.fields[_label_key(meta)][:g], kw


@pytest.mark.gpu
@pytest.mark.parametrize("name", PADDED)
def test_batched_nets_on_a_collators_padded_buffers_match_the_reference_float64(name):
    """The composition BatchCollator's docstring names: encoder, FusedEGCBlock(..., n_valid=) (Mpnn inside it too),
    global_*_pool(size=G + 1), the loss heads on the first G pooled rows.  (a) loss, outputs and every gradient within the
    fixture's bounds; (b) so are the running statistics: padding rows are not counted; (c) every element of every layer's
    output and of the pooled [G + 1, h] array is finite, padding rows and the spare graph included; (d) check() is clean."""
    z, meta = _load(name)
    g = meta["n_graphs"]
    net = _device_net(z, meta)
    col = _collator(z, meta)
    col.collate(torch.arange(g, device=_dev()))
    assert int(col.n_valid) == meta["n"] == col.n_pad - 38 and int(col.e_valid) == meta["n_edges"] == col.e_pad - 19
    args, y, kw = _padded_call(meta, col)
    res = _step(net, meta, args, y, g + 1, kw, g)
    _hold_to_fixture(f"{name} padded", z, meta, net, res)
    assert len(res["taps"]) == meta["layers"] + 1
    assert tuple(res["taps"][-1].shape) == (g + 1, meta["hidden"]) and res["taps"][0].size(0) == col.n_pad
    for i, t in enumerate(res["taps"]):
        assert bool(torch.isfinite(t).all()), f"a non-finite element in the output of stage {i}"
    col.check()


@pytest.mark.gpu
def test_a_padded_molhiv_step_with_the_collation_inside_a_graphed_step_replays_to_the_eager_bits():
    """hiv_egc_max on a store that holds the fixture's graphs twice: an epoch of two batches of the same graphs, col.next()
    recorded inside the step; each of two replays reproduces the eager padded step's loss and gradients bit for bit."""
    name = "hiv_egc_max"
    z, meta = _load(name)
    g, dev = meta["n_graphs"], _dev()
    net = _device_net(z, meta).train()
    col = _collator(z, meta, copies=2)
    args, y, kw = _padded_call(meta, col)
    params = list(net.parameters())

    def run():
        pooled = net.body(*args, g + 1, **kw)[:g]
        loss = net.mlp.bce_with_logits_loss(pooled, y)
        loss.backward()
        return loss.detach()

    col.collate(torch.arange(g, device=dev))
    eager_loss = run().clone()
    eager_grads = [p.grad.clone() for p in params]
    assert _rel(eager_loss, z["loss_train64"]) <= max(1e-5, 5.0 * meta["f32_vs_f64_loss"])
    loss_buf = torch.zeros((), device=dev)

    def fn():
        col.next()
        loss_buf.copy_(run())

    step = egc_amd.GraphedStep(fn, params=params, warmup=2)
    col.set_epoch(torch.arange(2 * g, device=dev))
    assert col.batches_per_epoch() == 2
    for _ in range(2):
        loss_buf.zero_()
        step()
        torch.cuda.synchronize()
        assert torch.equal(loss_buf, eager_loss)
        for p, want in zip(params, eager_grads):
            assert torch.equal(p.grad, want)
    col.check()
