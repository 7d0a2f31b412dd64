"""The graph-level MLP head on the device (egc_amd/csrc/egc_head.hip): every stage of the training forward and backward
against the float64 reference of head_ref.py from the device's own inputs to that stage, within the bounds derived there; the
running statistics against nn.BatchNorm1d in float64; the one-launch evaluation forward; bit-reproducibility; launch counts;
gradients that are not required; the stand-alone losses; a step recorded in GraphedStep; out-of-envelope inputs on torch's
operators; and the reference's own ZINC nets (tests/golden/net_zinc_*.npz) with GraphHead in place of their mlp, held to the
bounds test_nets_golden.py applies."""
import copy

import numpy as np
import pytest
import torch
import torch.nn as nn

import egc_amd
from egc_amd import _C
import callers
import head_ref as ref
from test_nets_golden import _build, _call, _load, _names, _state

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _ratio(got, want, bound):
    got, want = got.detach().cpu().double(), want.double()
    assert got.shape == want.shape, (got.shape, want.shape)
    r = float(((got - want).abs() / bound).max()) if got.numel() else 0.0
    assert r == r, "a NaN in the comparison"
    return r


def _head(sizes, case, momentum=0.1, track=True):
    head = ref.load_case(egc_amd.GraphHead(sizes), case)
    for m in head:
        if isinstance(m, nn.BatchNorm1d):
            m.momentum = momentum
            if not track:
                m.track_running_stats = False
                m.running_mean = m.running_var = m.num_batches_tracked = None
    return head.to(DEV)


def _grad_for(kind, g, out, seed):
    if kind == ref.LOSS_NONE:
        return torch.randn(g, out, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return torch.tensor(1.75, device=DEV)


def _case_on_device(sizes, g, kind, all_nan=False, plant=False):
    case = ref.make_case(sizes, g, seed=17 * g + len(sizes), kind=kind, all_nan=all_nan)
    head = _head(sizes, case)
    x = case["x"].to(DEV)
    if plant:                                     # out == y on every third entry: sign(0) = 0
        with torch.no_grad():
            out = head(x).cpu()
        case["y"].view(-1)[::3] = out.view(-1)[::3]
    y = case["y"].to(DEV) if kind != ref.LOSS_NONE else None
    return case, head, x, y


def _launches():
    return _C.load().egc_head_launches()


def _check_stages(sizes, g, kind, all_nan=False, plant=False):
    case, head, x, y = _case_on_device(sizes, g, kind, all_nan, plant)
    n_lin = len(sizes) - 1
    grad = _grad_for(kind, g, sizes[-1], g)
    n0 = _launches()
    st = head._launch_train(x, y, kind)
    n1 = _launches()
    dx, grads = head._launch_backward(st, x, y, kind, grad, True, True)
    n2 = _launches()
    torch.cuda.synchronize()
    assert (n1 - n0, n2 - n1) == ref.launches(sizes, kind)
    assert int(head._sync_word(DEV)) == 0                         # the arrival counter is back at zero
    worst = {}

    def hold(name, got, want, bound):
        r = _ratio(got, want, bound)
        worst[name] = max(worst.get(name, 0.0), r)

    bn = [m for m in head if isinstance(m, nn.BatchNorm1d)]
    a = case["x"]
    acts = [a]
    for i in range(n_lin - 1):
        z_dev, aff_dev = st["z"][i].cpu(), st["affine"][i].cpu()
        want, bound = ref.linear(a, case["ws"][i], case["bs"][i])
        hold(f"z{i + 1}", z_dev, want, bound)
        s = ref.stats(z_dev, case["gammas"][i], case["betas"][i], bn[i].eps)
        for row, key in enumerate(("mean", "var", "rstd")):
            hold(key, st["stats"][i][row], *s[key])
        hold("scale", aff_dev[0], *s["scale"])
        hold("shift", aff_dev[1], *s["shift"])
        a = ref.act32(z_dev, aff_dev)
        acts.append(a)
    out_dev = st["out"].cpu()
    want, bound = ref.linear(a, case["ws"][-1], case["bs"][-1])
    hold("out", out_dev, want, bound)
    if kind != ref.LOSS_NONE:
        loss2 = st["loss2"].cpu()
        val, bound, cnt = ref.loss(out_dev, case["y"], kind)
        assert float(loss2[1]) == cnt
        if cnt == 0:
            assert bool(torch.isnan(loss2[0]))
        else:
            hold("loss", loss2[0], torch.tensor(val, dtype=torch.float64), bound)
        want, bound = ref.d_out(out_dev, case["y"], kind, float(grad))
        hold("dout", st["dz"][-1], want, bound)
        dz_dev = st["dz"][-1].cpu()
        if plant:
            assert int((dz_dev.view(-1)[::3] != 0).sum()) == 0
        if all_nan:
            assert int((dz_dev != 0).sum()) == 0
    else:
        dz_dev = grad.cpu()
    it = iter(grads)
    got_w = [(next(it), next(it)) for _ in range(n_lin)]
    got_bn = [(next(it), next(it)) for _ in range(n_lin - 1)]
    for i in range(n_lin - 1, -1, -1):
        dw, bw, db, bb = ref.param_grads(dz_dev, acts[i])
        hold(f"dW{i + 1}", got_w[i][0], dw, bw)
        hold(f"db{i + 1}", got_w[i][1], db, bb)
        if i == 0:
            hold("dx", dx, *ref.d_act(dz_dev, case["ws"][0]))
            break
        z_lo, aff_lo = st["z"][i - 1].cpu(), st["affine"][i - 1].cpu()
        g_dev = st["g"][i - 1].cpu()
        hold(f"g{i}", g_dev, *ref.d_act(dz_dev, case["ws"][i], z_lo, aff_lo))
        coef_dev = st["coef"][i - 1].cpu()
        c = ref.coef(g_dev, z_lo, st["stats"][i - 1].cpu(), case["gammas"][i - 1])
        for row, key in enumerate(("dgamma", "dbeta", "cg", "ch", "c1")):
            hold(key, coef_dev[row], *c[key])
        assert torch.equal(got_bn[i - 1][0].cpu(), coef_dev[0]) and torch.equal(got_bn[i - 1][1].cpu(), coef_dev[1])
        dz_dev = st["dz"][i - 1].cpu()
        hold(f"dz{i}", dz_dev, *ref.dz(g_dev, z_lo, coef_dev))
    print(f"head {sizes} G={g} kind={kind}: worst ratio to bound " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, {k: v for k, v in worst.items() if v > 1.0}


@pytest.mark.parametrize("sizes,g,kind", ref.gpu_cases())
def test_every_stage_against_float64_from_the_devices_own_inputs(sizes, g, kind):
    _check_stages(sizes, g, kind)


def test_bce_with_every_target_nan_gives_nan_and_a_zero_gradient():
    _check_stages([168, 84, 42, 1], 128, ref.LOSS_BCE, all_nan=True)


def test_l1_with_out_equal_to_y_planted_has_a_zero_gradient_there():
    _check_stages([128, 64, 32, 1], 200, ref.LOSS_L1, plant=True)


def _step(head, x, y, kind, grad):
    """One public training call and its backward: (value, d x, the parameters' gradients)."""
    for p in head.parameters():
        p.grad = None
    xr = x.clone().requires_grad_(True)
    val = {ref.LOSS_NONE: lambda: head(xr), ref.LOSS_L1: lambda: head.l1_loss(xr, y),
           ref.LOSS_BCE: lambda: head.bce_with_logits_loss(xr, y)}[kind]()
    val.backward(grad)
    return val.detach().clone(), xr.grad.clone(), [p.grad.clone() for p in head.parameters()]


@pytest.mark.parametrize("sizes,g,kind", [([168, 84, 42, 1], 128, ref.LOSS_L1), ([300, 150, 75, 1], 257, ref.LOSS_BCE),
                                          ([304, 152, 76, 10], 33, ref.LOSS_NONE), ([36, 1], 17, ref.LOSS_L1)])
def test_two_runs_give_the_same_bits_and_the_public_path_is_the_staged_one(sizes, g, kind):
    case, head, x, y = _case_on_device(sizes, g, kind)
    grad = _grad_for(kind, g, sizes[-1], g)
    n0 = _launches()
    a = _step(head, x, y, kind, grad)
    assert _launches() - n0 == sum(ref.launches(sizes, kind))
    b = _step(head, x, y, kind, grad)
    st = head._launch_train(x, y, kind)
    dx, grads = head._launch_backward(st, x, y, kind, grad, True, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], st["out"] if kind == ref.LOSS_NONE else st["loss2"][0]) and torch.equal(a[1], dx)
    # parameters() order: the Sequential's children; the staged order: Linears, then BatchNorms
    by_param = {id(p): gr for p, gr in zip(head._params(), grads)}
    for p, ga, gb in zip(head.parameters(), a[2], b[2]):
        assert torch.equal(ga, gb) and torch.equal(ga, by_param[id(p)])


def test_a_gradient_that_is_not_required_is_none_and_not_computed():
    sizes, g = [40, 20, 1], 31
    case, head, x, y = _case_on_device(sizes, g, ref.LOSS_L1)
    full = _step(head, x, y, ref.LOSS_L1, torch.tensor(1.0, device=DEV))
    for p in head.parameters():
        p.grad = None
    n0 = _launches()
    head.l1_loss(x, y).backward()                                  # x needs no gradient: every launch still runs but d x
    assert _launches() - n0 == sum(ref.launches(sizes, ref.LOSS_L1, want_dx=False))
    for p, want in zip(head.parameters(), full[2]):
        assert torch.equal(p.grad, want)
    frozen = copy.deepcopy(head).requires_grad_(False)
    xr = x.clone().requires_grad_(True)
    n0 = _launches()
    frozen.l1_loss(xr, y).backward()                               # no parameter gradient: no parameter launch
    assert _launches() - n0 == sum(ref.launches(sizes, ref.LOSS_L1, want_params=False))
    assert torch.equal(xr.grad, full[1]) and all(p.grad is None for p in frozen.parameters())
    head[0].weight.requires_grad_(False)
    for p in head.parameters():
        p.grad = None
    head.l1_loss(x, y).backward()
    assert head[0].weight.grad is None and torch.equal(head[0].bias.grad, full[2][1])
    n0 = _launches()
    with torch.no_grad():
        assert torch.equal(head.l1_loss(x, y), full[0])
    assert _launches() - n0 == len(sizes) - 1


@pytest.mark.parametrize("momentum,track", [(0.1, True), (None, True), (0.1, False)])
def test_running_statistics_after_one_and_two_steps_against_batchnorm_float64(momentum, track):
    sizes, g = [168, 84, 42, 1], 129
    case = ref.make_case(sizes, g, seed=5)
    head = _head(sizes, case, momentum, track)
    bn = [m for m in head if isinstance(m, nn.BatchNorm1d)]
    theirs = [nn.BatchNorm1d(w, momentum=momentum, track_running_stats=track).double() for w in sizes[1:-1]]
    xs = [case["x"].to(DEV), (0.5 * case["x"] + 0.25).to(DEV)]
    carried = {}
    for step, x in enumerate(xs):
        st = head._launch_train(x, None, ref.LOSS_NONE)
        torch.cuda.synchronize()
        for i, (m, t) in enumerate(zip(bn, theirs)):
            t(st["z"][i].cpu().double())                           # the stage's own input: the device's z
            if not track:
                assert m.running_mean is None and m.running_var is None and m.num_batches_tracked is None
                continue
            assert int(m.num_batches_tracked) == step + 1 == int(t.num_batches_tracked)
            f = momentum if momentum is not None else 1.0 / (step + 1)
            for key, got, want in (("mean", m.running_mean, t.running_mean), ("var", m.running_var, t.running_var)):
                err = (got.cpu().double() - want).abs()
                # running = (1 - f) running + f stat: one float32 rounding of the new value (half an ulp) and as much again
                # for the statistics' budget; the previous step's error comes along with the factor 1 - f
                bound = (1.0 - f) * carried.get((i, key), 0.0) + 2 * ref.U * want.abs() + 1e-30
                carried[(i, key)] = bound
                assert bool((err <= bound).all()), (step, i, key, float((err / bound).max()))
    if not track:                                                  # no running statistics: evaluation uses the batch's
        head.eval()
        with torch.no_grad():
            assert torch.equal(head(xs[1]), st["out"])


@pytest.mark.parametrize("sizes,g", [([168, 84, 42, 1], 128), ([300, 150, 75, 1], 17), ([304, 152, 76, 10], 200), ([36, 1], 15),
                                     ([64, 32, 16, 8, 3], 33), ([4, 2, 1, 1], 2), ([384, 192, 96, 10], 1)])
def test_evaluation_forward_is_one_launch_and_matches_float64(sizes, g):
    case = ref.make_case(sizes, max(g, 2), seed=3 * g)
    head = _head(sizes, case)
    bn = [m for m in head if isinstance(m, nn.BatchNorm1d)]
    head._launch_train(case["x"].to(DEV), None, ref.LOSS_NONE)       # running statistics away from (0, 1)
    head.eval()
    x = case["x"][:g].to(DEV)
    n0 = _launches()
    with torch.no_grad():
        out = head(x)
    assert _launches() - n0 == 1
    assert torch.equal(head.predict(x), out)
    want, bound = ref.eval_forward(case["x"][:g], case["ws"], case["bs"], case["gammas"], case["betas"],
                                   [m.running_mean.cpu() for m in bn], [m.running_var.cpu() for m in bn], [m.eps for m in bn])
    r = _ratio(out, want, bound)
    print(f"eval {sizes} G={g}: worst ratio to bound {r:.3g}")
    assert r <= 1.0
    n0 = _launches()
    with torch.no_grad():
        assert head(x[:0]).shape == (0, sizes[-1])
    assert _launches() == n0
    head.train()
    assert torch.equal(head.predict(x), out) and head.training     # predict is the evaluation forward whatever the mode


@pytest.mark.parametrize("g,out", [(1, 1), (17, 1), (200, 10)])
@pytest.mark.parametrize("kind", [ref.LOSS_L1, ref.LOSS_BCE])
def test_stand_alone_losses_against_float64(g, out, kind):
    gen = torch.Generator().manual_seed(g + out + kind)
    o = (3.0 * torch.randn(g, out, generator=gen))
    if kind == ref.LOSS_BCE:
        y = torch.randint(0, 2, (g, out), generator=gen).float()
        if g > 1:
            y[torch.rand(g, out, generator=gen) < 0.3] = float("nan")
    else:
        y = torch.randn(g, out, generator=gen)
        y.view(-1)[::4] = o.view(-1)[::4]
    od = o.to(DEV).requires_grad_(True)
    fn = egc_amd.l1_loss if kind == ref.LOSS_L1 else egc_amd.masked_bce_with_logits
    n0 = _launches()
    val = fn(od, y.to(DEV))
    (2.5 * val).backward()
    assert _launches() - n0 == 2
    want, bound, _ = ref.loss(o, y, kind)
    assert abs(float(val.detach()) - want) <= bound, (float(val.detach()), want, bound)
    dwant, dbound = ref.d_out(o, y, kind, 2.5)
    assert _ratio(od.grad, dwant, dbound) <= 1.0
    od2 = o.to(DEV).requires_grad_(True)
    val2 = fn(od2, y.to(DEV))
    (2.5 * val2).backward()
    assert torch.equal(val2, val) and torch.equal(od2.grad, od.grad)


def test_a_training_step_recorded_in_graphed_step_replays_to_the_eager_bits():
    sizes, g = [168, 84, 42, 1], 128
    case, head, x, y = _case_on_device(sizes, g, ref.LOSS_L1)
    eager = _step(head, x, y, ref.LOSS_L1, torch.tensor(1.0, device=DEV))
    loss_buf = torch.zeros((), device=DEV)
    xr = x.clone().requires_grad_(True)

    def fn():
        xr.grad = None
        loss = head.l1_loss(xr, y)
        loss.backward()
        loss_buf.copy_(loss.detach())

    step = egc_amd.GraphedStep(fn, params=list(head.parameters()), warmup=2)
    for _ in range(2):
        loss_buf.zero_()
        step()
        torch.cuda.synchronize()
        assert torch.equal(loss_buf, eager[0])
        for p, want in zip(head.parameters(), eager[2]):
            assert torch.equal(p.grad, want)


def test_out_of_envelope_inputs_take_torchs_composition():
    def pair(sizes, **kw):
        torch.manual_seed(1)
        ours = egc_amd.GraphHead(sizes, **kw).to(DEV)
        theirs = callers.head_mlp(sizes).to(DEV)
        if "act" in kw:
            theirs = nn.Sequential(*[kw["act"]() if isinstance(m, nn.ReLU) else m for m in theirs])
        if "dropout" in kw:
            for m in theirs:
                if isinstance(m, nn.Dropout):
                    m.p = kw["dropout"]
        theirs.load_state_dict(ours.state_dict(), strict=True)
        return ours, theirs

    n0 = _launches()
    x385 = torch.randn(9, 385, device=DEV)
    ours, theirs = pair([385, 8, 1])
    assert torch.equal(ours(x385), theirs(x385))
    ours, theirs = pair([12, 6, 1])
    ours, theirs = ours.double(), theirs.double()
    x64 = torch.randn(9, 12, device=DEV, dtype=torch.float64)
    assert torch.equal(ours(x64), theirs(x64))
    y64 = torch.randn(9, 1, device=DEV, dtype=torch.float64)
    assert torch.equal(ours.l1_loss(x64, y64), torch.nn.functional.l1_loss(theirs(x64), y64))
    ours, theirs = pair([12, 6, 1], act=nn.ELU)
    x = torch.randn(9, 12, device=DEV)
    assert torch.equal(ours(x), theirs(x))
    ours, theirs = pair([12, 6, 1], dropout=0.1)
    torch.manual_seed(7)
    a = ours(x)
    torch.manual_seed(7)
    assert torch.equal(a, theirs(x))
    assert _launches() == n0                                         # none of it reached the head's kernels
    ours.eval()                                                      # dropout is the identity in evaluation: the kernels take it
    theirs.eval()
    with torch.no_grad():
        assert ours(x).shape == theirs(x).shape
    assert _launches() == n0 + 1


@pytest.mark.parametrize("name", _names("net_zinc_"))
def test_reference_zinc_nets_with_the_head_in_place_of_their_mlp(name):
    z, meta = _load(name)
    h = meta["hidden"]
    net = _build(meta)
    net.mlp = egc_amd.GraphHead([h, h // 2, h // 4, 1])
    net.load_state_dict(_state(z), strict=True)
    net = net.to(DEV)
    n0 = _launches()
    net.eval()
    with torch.no_grad():
        out_eval, _ = _call(net, meta, z, DEV, torch.float32, False)
    assert _launches() - n0 == 1
    net.train()
    out, _ = _call(net, meta, z, DEV, torch.float32, True)
    out.backward(torch.from_numpy(z["gout"]).to(DEV))
    assert _launches() - n0 == 1 + sum(ref.launches([h, h // 2, h // 4, 1], ref.LOSS_NONE))

    def rel(a, b):
        b = torch.from_numpy(b).double()
        return float((a.detach().cpu().double() - b).abs().max() / max(1.0, float(b.abs().max())))
    d_out = max(1e-5, 5.0 * meta["f32_vs_f64_out_train"])
    assert rel(out_eval, z["out_eval64"]) <= d_out, rel(out_eval, z["out_eval64"])
    assert rel(out, z["out_train64"]) <= d_out, rel(out, z["out_train64"])
    gscale = meta["grad_scale"]
    for k, p in net.named_parameters():
        want = torch.from_numpy(z[f"grad64:{k}"]).double()
        bound = max(1e-5, 5.0 * meta["f32_vs_f64_grad"][k])
        wmax = float(want.abs().max())
        denom = gscale if wmax < 1e-6 * gscale else max(1e-2 * gscale, wmax)
        err = float((p.grad.cpu().double() - want).abs().max() / denom)
        assert err <= bound, (k, err, bound)
