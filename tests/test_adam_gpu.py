"""egc_amd.Adam on the device (egc_adam.hip) against the float64 oracle of tests/adam_ref.py.

The bound, per tensor and per element: |ours - float64| <= max(floor, 4 x d32).  d32 is the distance of torch's own float32 CPU
Adam (foreach=False) from float64 on the same inputs, taken over the whole tensor; the margin of 4 is there because the order of
the products differs from torch's lerp, which shifts roundings, not their size.  floor is
1 ulp(max(|x_old|, |x_new|)) + 2^-20 |x_new - x_old| (sixteen float32 roundings of the update) for x = p and alike for the two
moments.  Over several steps d32 is taken over the same steps and the floors add up.
The inputs are the states Adam produces: |p| in [0.5, 2), gradients N(0, 1), m = 0.1 N(0, 1), v >= m^2.
Every test prints the largest distances it met (ours and d32) before it asserts."""
import copy
import json
import os

import numpy as np
import pytest
import torch

import adam_ref

pytestmark = pytest.mark.gpu

BE = adam_ref.BLOCK_ELEMS
DEV = "cuda:0"


# ---- inputs, the two references and the comparison ---------------------------------------------------------------------------
def _inputs(rng, numels, with_state):
    p = [(rng.choice([-1.0, 1.0], size=n) * (0.5 + 1.5 * rng.random(n))).astype(np.float32) for n in numels]
    if not with_state:
        return p, [np.zeros(n, np.float32) for n in numels], [np.zeros(n, np.float32) for n in numels]
    m = [(0.1 * rng.standard_normal(n)).astype(np.float32) for n in numels]
    v = [(a.astype(np.float64) ** 2 + 1e-3 * rng.random(a.size)).astype(np.float32) for a in m]
    return p, m, v


def _grads(rng, numels):
    return [rng.standard_normal(n).astype(np.float32) for n in numels]


def _references(groups, grads_seq):
    """groups: [dict(params=, m=, v=, t=, lr=, wd=)] of float32 arrays; grads_seq: per step, per group, arrays or None.
    Returns (the float64 oracle after the steps, per tensor the summed floors of p / m / v, per tensor d32 of p / m / v)."""
    ref = adam_ref.RefAdam(groups)
    floors = [[[np.zeros(p.shape), np.zeros(p.shape), np.zeros(p.shape)] for p in g["params"]] for g in groups]
    for grads in grads_seq:
        before = [[(g["params"][k], g["m"][k], g["v"][k]) for k in range(len(g["params"]))] for g in ref.groups]
        ref.step(grads)
        for gi, g in enumerate(ref.groups):
            for k, grad in enumerate(grads[gi]):
                if grad is None:
                    continue
                for q, (old, new) in enumerate(zip(before[gi][k], (g["params"][k], g["m"][k], g["v"][k]))):
                    floors[gi][k][q] += adam_ref.floor_of_step(old, new)
    # torch's own float32 on the CPU, one tensor at a time
    tp = [[torch.nn.Parameter(torch.from_numpy(np.array(p, dtype=np.float32))) for p in g["params"]] for g in groups]
    opt = torch.optim.Adam([dict(params=ps, lr=g["lr"], weight_decay=g.get("wd", 0.0)) for ps, g in zip(tp, groups)], foreach=False)
    for ps, g in zip(tp, groups):
        for k, p in enumerate(ps):
            if "t" in g and (g["t"][k] or np.any(g["m"][k]) or np.any(g["v"][k])):
                opt.state[p] = dict(step=torch.tensor(float(g["t"][k])), exp_avg=torch.from_numpy(np.array(g["m"][k], dtype=np.float32)),
                                    exp_avg_sq=torch.from_numpy(np.array(g["v"][k], dtype=np.float32)))
    for grads in grads_seq:
        for ps, gs in zip(tp, grads):
            for p, grad in zip(ps, gs):
                p.grad = None if grad is None else torch.from_numpy(grad.copy())
        opt.step()
    d32 = []
    for gi, ps in enumerate(tp):
        d32.append([])
        for k, p in enumerate(ps):
            st = opt.state.get(p, {})
            m32 = st["exp_avg"].numpy() if st else np.zeros(p.shape)
            v32 = st["exp_avg_sq"].numpy() if st else np.zeros(p.shape)
            r = ref.groups[gi]
            d32[-1].append((adam_ref.dist(p.detach().numpy(), r["params"][k]), adam_ref.dist(m32, r["m"][k]), adam_ref.dist(v32, r["v"][k])))
    return ref, floors, d32


def _check(opt, params, ref, floors, d32, label):
    """Every p, m, v and step count of ``params`` ([[Parameter]] per group) against the oracle; prints the figures."""
    worst = dict(ours=[0.0] * 3, d32=[0.0] * 3, ratio=[0.0] * 3)
    bad = []
    for gi, ps in enumerate(params):
        for k, p in enumerate(ps):
            st = opt.state.get(p, {})
            r = ref.groups[gi]
            assert (int(st["step"]) if st else 0) == r["t"][k], (label, gi, k)
            got = (p.detach(), st["exp_avg"] if st else torch.zeros_like(p), st["exp_avg_sq"] if st else torch.zeros_like(p))
            for q, (name, a, want) in enumerate(zip("pmv", got, (r["params"][k], r["m"][k], r["v"][k]))):
                err = np.abs(a.cpu().numpy().astype(np.float64) - want)
                bound = np.maximum(floors[gi][k][q], 4 * d32[gi][k][q])
                if err.size:
                    worst["ours"][q] = max(worst["ours"][q], float(err.max()))
                    worst["d32"][q] = max(worst["d32"][q], d32[gi][k][q])
                    worst["ratio"][q] = max(worst["ratio"][q], float(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max()))
                    if (err > bound).any():
                        bad.append((gi, k, name, float(err.max()), float(bound[err.argmax()]), d32[gi][k][q]))
    print("ADAM_FIGURES " + json.dumps(dict(test=label, max_abs_err_p_m_v=worst["ours"], max_d32_p_m_v=worst["d32"],
                                            max_err_over_bound_p_m_v=worst["ratio"])))
    assert not bad, (label, bad[:5])


def _device_params(arrays, views=()):
    """Parameters on the device; index in ``views``: a view that starts 4 bytes past a 16-byte boundary."""
    out = []
    for k, a in enumerate(arrays):
        t = torch.from_numpy(a).to(DEV)
        if k in views:
            base = torch.zeros(a.size + 8, device=DEV)
            assert base.data_ptr() % 16 == 0
            base[1:1 + a.size] = t
            t = base[1:1 + a.size]
        out.append(torch.nn.Parameter(t))
        assert out[-1].data_ptr() % 16 == (4 if k in views else 0) or a.size == 0
    return out


def _set_grads(params, grads, views=()):
    for gi, (ps, gs) in enumerate(zip(params, grads)):
        for k, (p, g) in enumerate(zip(ps, gs)):
            if g is None:
                p.grad = None
                continue
            t = torch.from_numpy(g).to(DEV)
            if (gi, k) in views:
                base = torch.zeros(g.size + 8, device=DEV)
                base[1:1 + g.size] = t
                t = base[1:1 + g.size]
            p.grad = t


def _load_state(opt, groups):
    """The given (m, v, t) through load_state_dict, in torch's layout."""
    sd = opt.state_dict()
    index = 0
    for g in groups:
        for k in range(len(g["params"])):
            sd["state"][index] = dict(step=torch.tensor(float(g["t"][k])), exp_avg=torch.from_numpy(g["m"][k]),
                                      exp_avg_sq=torch.from_numpy(g["v"][k]))
            index += 1
    opt.load_state_dict(sd)


# ---- one step from a given state -----------------------------------------------------------------------------------------------
ONE_STEP_NUMELS = [1, 3, 4, 5, 255, 256, 257, BE - 1, BE, BE + 1, 0, 2 * BE + 5, 261]
ONE_STEP_P_VIEW, ONE_STEP_G_VIEW = 11, 12          # p, respectively g, 4 bytes past a 16-byte boundary


@pytest.mark.parametrize("wd", [0.0, 1e-2])
@pytest.mark.parametrize("t", [0, 1, 999])
def test_one_step_from_a_given_state(t, wd):
    import egc_amd
    rng = np.random.default_rng(1000 * t + int(wd * 100))
    p, m, v = _inputs(rng, ONE_STEP_NUMELS, with_state=t > 0)
    groups = [dict(params=p, m=m, v=v, t=[t] * len(p), lr=1e-3, wd=wd)]
    grads = [_grads(rng, ONE_STEP_NUMELS)]
    ref, floors, d32 = _references(groups, [grads])
    params = [_device_params(p, views=(ONE_STEP_P_VIEW,))]
    opt = egc_amd.Adam(params[0], lr=1e-3, weight_decay=wd)
    if t > 0:
        _load_state(opt, groups)
    _set_grads(params, grads, views=((0, ONE_STEP_G_VIEW),))
    assert params[0][ONE_STEP_P_VIEW].data_ptr() % 16 == 4 and params[0][ONE_STEP_G_VIEW].grad.data_ptr() % 16 == 4
    opt.step()
    torch.cuda.synchronize()
    _check(opt, params, ref, floors, d32, f"one_step t={t} wd={wd}")
    own = opt._owned[0]          # every workgroup's copy of a tensor's step count agrees
    words = own.steps.cpu().numpy()
    assert sum(own.blocks) == len(words) and (words == t + 1).all()
    assert own.blocks[ONE_STEP_NUMELS.index(2 * BE + 5)] == 3 and all(o % 4 == 0 for o in own.state_off)


# ---- twenty steps, two groups, a tensor skipped on some steps --------------------------------------------------------------------
TWENTY = dict(numels=[[37, BE + 1, 5], [300, 256]], lr=[1e-3, 5e-3], wd=[1e-2, 0.0], steps=20)


def _twenty_inputs():
    rng = np.random.default_rng(20)
    groups = []
    for numels, lr, wd in zip(TWENTY["numels"], TWENTY["lr"], TWENTY["wd"]):
        p, m, v = _inputs(rng, numels, with_state=False)
        groups.append(dict(params=p, m=m, v=v, t=[0] * len(p), lr=lr, wd=wd))
    seq = []
    for s in range(TWENTY["steps"]):
        grads = [_grads(rng, numels) for numels in TWENTY["numels"]]
        if s % 3 == 1:
            grads[0][2] = None
        seq.append(grads)
    return groups, seq


_TWENTY_CACHE = {}


def _twenty(upto=None):
    """The shared references of the twenty-step run (and of its first ``upto`` steps), computed once."""
    if "inputs" not in _TWENTY_CACHE:
        _TWENTY_CACHE["inputs"] = _twenty_inputs()
    groups, seq = _TWENTY_CACHE["inputs"]
    n = TWENTY["steps"] if upto is None else upto
    if n not in _TWENTY_CACHE:
        _TWENTY_CACHE[n] = _references(groups, seq[:n])
    return groups, seq[:n], _TWENTY_CACHE[n]


def _ours(groups, cls=None, **kw):
    import egc_amd
    params = [_device_params(g["params"]) for g in groups]
    opt = (cls or egc_amd.Adam)([dict(params=ps, lr=g["lr"], weight_decay=g["wd"]) for ps, g in zip(params, groups)], **kw)
    return params, opt


def test_twenty_steps_two_groups_and_a_skipped_tensor():
    groups, seq, (ref, floors, d32) = _twenty()
    params, opt = _ours(groups)
    for grads in seq:
        _set_grads(params, grads)
        opt.step()
    torch.cuda.synchronize()
    assert ref.groups[0]["t"] == [20, 20, 13] and ref.groups[1]["t"] == [20, 20]
    _check(opt, params, ref, floors, d32, "twenty_steps")


# ---- capacity ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 1])
def test_a_full_launch_and_one_tensor_more(extra):
    import egc_amd
    from egc_amd import _optim
    lib = _optim.load()
    n = lib.egc_adam_max_tensors() + extra
    rng = np.random.default_rng(7 + extra)
    numels = [1 + k % 5 for k in range(n)]
    p, m, v = _inputs(rng, numels, with_state=False)
    groups = [dict(params=p, m=m, v=v, t=[0] * n, lr=1e-3, wd=0.0)]
    grads = [_grads(rng, numels)]
    ref, floors, d32 = _references(groups, [grads])
    params, opt = _ours(groups)
    _set_grads(params, grads)
    n0 = lib.egc_adam_launch_count()
    opt.step()
    torch.cuda.synchronize()
    assert lib.egc_adam_launch_count() - n0 == lib.egc_adam_launches(n) == 1 + extra
    _check(opt, params, ref, floors, d32, f"capacity n={n}")
    for q, a in zip(params[0], p):                  # every tensor moved, by about lr in every element
        assert (np.abs(q.detach().cpu().numpy() - a) > 0.5e-3).all()


# ---- zero_grad, reproducibility ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("zero", [True, False])
def test_zero_grad_in_the_launch(zero):
    groups, seq, _ = _twenty(upto=2)
    params, opt = _ours(groups)
    _set_grads(params, seq[0], views=((1, 0),))
    held = [[p.grad for p in ps] for ps in params]
    before = [[g.clone() for g in gs] for gs in held]
    versions = [[(p._version, g._version) for p, g in zip(ps, gs)] for ps, gs in zip(params, held)]
    opt.step(zero_grad=zero)
    torch.cuda.synchronize()
    # what the kernel wrote counts as an in-place change (the layers key their caches of packed weights on the counters)
    for ps, hs, vs in zip(params, held, versions):
        for p, h, (vp, vg) in zip(ps, hs, vs):
            assert p._version > vp and (h._version > vg) == zero and opt.state[p]["exp_avg"]._version > 0
    for ps, hs, bs in zip(params, held, before):
        for p, h, b in zip(ps, hs, bs):
            assert p.grad is h
            assert torch.equal(h, torch.zeros_like(h) if zero else b)
            assert not torch.equal(b, torch.zeros_like(b))


def test_two_runs_from_the_same_state_are_bit_identical():
    groups, seq, _ = _twenty(upto=3)
    runs = []
    for _ in range(2):
        params, opt = _ours(groups)
        for grads in seq:
            _set_grads(params, grads)
            opt.step(zero_grad=True)
        torch.cuda.synchronize()
        runs.append([t.clone() for ps in params for p in ps for t in (p.detach(), opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]
                    + [own.steps.clone() for own in opt._owned])
    assert len(runs[0]) == 3 * 5 + 2
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ---- the learning rate ---------------------------------------------------------------------------------------------------------
def test_plateau_scheduler_halves_the_device_scalar():
    groups, seq, _ = _twenty(upto=2)
    params, opt = _ours(groups)
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "min", factor=0.5, patience=0)
    held = [g["lr"] for g in opt.param_groups]
    _set_grads(params, seq[0])
    opt.step()
    sched.step(1.0)
    sched.step(2.0)                                # worse: patience 0 -> halve
    assert all(g["lr"] is h for g, h in zip(opt.param_groups, held))
    assert [h.item() for h in held] == [1e-3 * 0.5, 5e-3 * 0.5] and all(h.is_cuda and h.dtype == torch.float64 for h in held)
    _set_grads(params, seq[1])
    opt.step()
    torch.cuda.synchronize()
    # the oracle: step 2 at half the rate
    # (the second step is judged from the DEVICE's state after the first, so that its bound is a one-step bound)
    mid = [dict(t=[1] * len(g["params"]), lr=g["lr"] * 0.5, wd=g["wd"]) for g in groups]
    params2, opt2 = _ours(groups)
    _set_grads(params2, seq[0])
    opt2.step()
    torch.cuda.synchronize()
    for g, ps in zip(mid, params2):
        g["params"] = [p.detach().cpu().numpy() for p in ps]
        g["m"] = [opt2.state[p]["exp_avg"].cpu().numpy() for p in ps]
        g["v"] = [opt2.state[p]["exp_avg_sq"].cpu().numpy() for p in ps]
    ref, floors, d32 = _references(mid, seq[1:2])
    _check(opt, params, ref, floors, d32, "after_plateau")
    # a Python float assigned later reaches the scalar at the next step
    opt.param_groups[0]["lr"] = 0.125
    _set_grads(params, seq[0])
    opt.step()
    assert opt.param_groups[0]["lr"] is held[0] and held[0].item() == 0.125


# ---- the whole iteration as one recording --------------------------------------------------------------------------------------
def test_whole_iteration_recorded_with_the_fused_adam():
    """forward + loss + backward + egc_amd.Adam.step(zero_grad=True) as ONE recording: after the warm-up iterations and k
    replays, parameters, both moments, step counts and BatchNorm statistics equal those of as many eager iterations, bit for
    bit; the scheduler halves the rate between two replays and the recording follows."""
    import egc_amd
    from egc_amd import _optim, workloads as wl
    from test_hipgraph_gpu import _blocks
    dev = torch.device(DEV)
    _, ei, n, _ = wl.zinc_like_batch(32, seed=2)
    ei = ei.to(dev)
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(n, 64, generator=gen).to(dev)
    tgt = torch.randn(n, 64, generator=gen).to(dev)
    warmup, k, halve_after = 2, 5, 2

    def run(recorded):
        blocks = _blocks(dev, "opt")
        params = list(blocks.parameters())
        opt = egc_amd.Adam(params, lr=1e-2, weight_decay=1e-3)
        sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "min", factor=0.5, patience=0)
        sched.step(1.0)

        def step():
            h = x
            for b in blocks:
                h = b(h, ei)
            ((h - tgt) ** 2).mean().backward()
            opt.step(zero_grad=True)
        if recorded:
            n0 = _optim.load().egc_adam_launch_count()
            g = egc_amd.GraphedStep(step, params=params, warmup=warmup)
            assert _optim.load().egc_adam_launch_count() - n0 == warmup + 1       # one launch per call of the step
        for i in range(k if recorded else warmup + k):
            if i == (halve_after if recorded else warmup + halve_after):
                sched.step(2.0)
                assert opt.param_groups[0]["lr"].item() == 5e-3
            if recorded:
                g()
            else:
                for p in params:
                    p.grad = None
                step()
        torch.cuda.synchronize()
        assert all(torch.equal(p.grad, torch.zeros_like(p)) for p in params)
        assert [int(opt.state[p]["step"]) for p in params] == [warmup + k] * len(params)
        return ([p.detach().clone() for p in params] + [opt.state[p][key].clone() for p in params for key in ("exp_avg", "exp_avg_sq", "step")]
                + [own.steps.clone() for own in opt._owned] + [b.bn.running_var.clone() for b in blocks])

    got, want = run(True), run(False)
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


def test_a_float_lr_assigned_under_a_capture_raises():
    """The recorded step reads the optimizer's device scalar: a Python float put in its place while a capture is under way
    cannot reach it, so step() raises instead of recording a stale rate; outside a capture the next step() copies it in."""
    groups, seq, _ = _twenty(upto=2)
    params, opt = _ours(groups)
    held = opt.param_groups[0]["lr"]
    _set_grads(params, seq[0])
    opt.step()
    tmp = torch.zeros(4, device=DEV)
    torch.cuda.synchronize()
    opt.param_groups[0]["lr"] = 0.5
    with pytest.raises(RuntimeError, match="capture is under way"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            tmp.add_(1.0)
            opt.step()
    torch.cuda.synchronize()
    assert opt.param_groups[0]["lr"] == 0.5 and held.item() == 1e-3
    opt.step()
    assert opt.param_groups[0]["lr"] is held and held.item() == 0.5


# ---- state dicts ---------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trips_and_torch_exchange():
    import egc_amd
    groups, seq, (ref, floors, d32) = _twenty(upto=6)

    def cont(params, opt, lo, hi):
        for grads in seq[lo:hi]:
            _set_grads(params, grads)
            opt.step()
        torch.cuda.synchronize()
        return [p.detach().clone() for ps in params for p in ps]

    params, opt = _ours(groups)
    cont(params, opt, 0, 3)
    snap = [[p.detach().cpu().numpy().copy() for p in ps] for ps in params]
    sd = copy.deepcopy(opt.state_dict())
    assert [float(s["step"]) for s in sd["state"].values()] == [3.0, 3.0, 2.0, 3.0, 3.0]
    assert all(s["step"].dtype == torch.float32 and s["exp_avg"].shape == p.shape for s, p in
               zip(sd["state"].values(), [p for ps in params for p in ps]))
    assert [g["lr"] for g in sd["param_groups"]] == TWENTY["lr"]
    # exp_avg / exp_avg_sq are views into the owned buffers
    own = opt._owned[0]
    st = opt.state[params[0][1]]
    assert st["exp_avg"].data_ptr() == own.exp_avg.data_ptr() + 4 * own.state_off[1]
    assert st["exp_avg_sq"].data_ptr() == own.exp_avg_sq.data_ptr() + 4 * own.state_off[1] and st["exp_avg"].data_ptr() % 16 == 0
    uninterrupted = cont(params, opt, 3, 6)
    at3 = [dict(g, params=s) for g, s in zip(groups, snap)]
    # own -> own
    params_b, opt_b = _ours(at3)
    opt_b.load_state_dict(copy.deepcopy(sd))
    for a, b in zip(cont(params_b, opt_b, 3, 6), uninterrupted):
        assert torch.equal(a, b)
    # own -> torch.optim.Adam -> own
    params_t, opt_t = _ours(at3, cls=torch.optim.Adam)
    opt_t.load_state_dict(copy.deepcopy(sd))
    params_c, opt_c = _ours(at3)
    opt_c.load_state_dict(copy.deepcopy(opt_t.state_dict()))
    for a, b in zip(cont(params_c, opt_c, 3, 6), uninterrupted):
        assert torch.equal(a, b)
    assert [int(opt_c.state[p]["step"]) for ps in params_c for p in ps] == [6, 6, 4, 6, 6]
    # continued by torch.optim.Adam itself: within the bound of the six steps against the float64 oracle
    cont(params_t, opt_t, 3, 6)
    _check(opt_t, params_t, ref, floors, d32, "continued_by_torch")
    _check(opt, params, ref, floors, d32, "six_steps")


# ---- the reference's loop ------------------------------------------------------------------------------------------------------
def test_reference_zinc_loop_with_the_fused_adam():
    """tests/golden/train_zinc_plateau.npz rerun with fit_zinc's schedule (tests/callers.py, restated here with egc_amd.Adam in
    place of torch's) on the fused blocks, held to exactly the bounds of
    tests/test_train_golden.py::test_hip_layers_follow_the_reference_trajectory, the learning-rate list included."""
    import egc_amd
    from callers import evaluate, train_epoch
    from golden_util import GOLDEN_DIR
    from test_train_golden import _data, _load, _net
    name = "train_zinc_plateau"
    z, meta = _load(name)
    man = json.load(open(os.path.join(GOLDEN_DIR, "MANIFEST_TRAIN.json")))[name]
    dev = torch.device(DEV)
    net = _net(z, meta).to(dev)
    data = _data(z, meta, dev, torch.float32)
    blocks = {}

    def fuse(conv, bn, residual):
        if id(conv) not in blocks:
            blocks[id(conv)] = egc_amd.FusedEGCBlock(conv, bn, relu=True, residual=residual)
        blocks[id(conv)].train(bn.training)
        return blocks[id(conv)]

    def forward(b):
        return net(b["atom"], b["edge_index"], b["batch"], b["n_graphs"], fuse=fuse,
                   pool=lambda x, batch, n_graphs: egc_amd.global_mean_pool(x, batch, n_graphs))
    # fit_zinc (zinc/configs.py:128-154), the optimizer swapped
    opt = egc_amd.Adam(net.parameters(), lr=meta["lr"], weight_decay=meta["wd"])
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "min", factor=0.5, patience=10, min_lr=1e-5)
    tr, va, lrs = [], [], []
    for _ in range(meta["iterations"]):
        tr.append(train_epoch(forward, [net], opt, data["train"]))
        val = evaluate(forward, [net], data["val"])
        sched.step(val)
        va.append(val)
        lrs.append(opt.param_groups[0]["lr"].item())
    te = evaluate(forward, [net], data["test"])
    head = slice(0, 10)
    d_tr, d_va = np.abs(np.array(tr) - z["train_loss64"]), np.abs(np.array(va) - z["val_loss64"])
    r_tr, r_va = np.abs(z["train_loss32"] - z["train_loss64"]), np.abs(z["val_loss32"] - z["val_loss64"])
    tol_tr = max(1e-5, 5 * float(r_tr[head].max()))
    tol_va = max(1e-5, 10 * float(r_va[head].max()))
    if {"std", "var"} & set(meta["aggrs"]):
        tol_va = max(tol_va, 2e-4)
    print("ADAM_FIGURES " + json.dumps(dict(test="zinc_loop", d_train_head=float(d_tr[head].max()), tol_train=tol_tr,
                                            d_val_head=float(d_va[head].max()), tol_val=tol_va, d_train=float(d_tr.max()),
                                            d_val=float(d_va.max()), lrs_equal=bool(np.array_equal(np.array(lrs), z["lr64"])))))
    assert d_tr[head].max() <= tol_tr, (d_tr, tol_tr)
    assert d_va[head].max() <= tol_va, (d_va, tol_va)
    assert d_tr.max() <= max(2e-3, 5 * man["f32_vs_f64_train_loss"]) and d_va.max() <= max(2e-3, 5 * man["f32_vs_f64_val_loss"])
    assert abs(te - float(z["test_loss64"])) <= max(2e-3, 5 * man["f32_vs_f64_val_loss"])
    if np.array_equal(z["lr32"], z["lr64"]):
        assert np.array_equal(np.array(lrs), z["lr64"])
    assert tr[-1] < tr[0]
    assert lrs[0] == meta["lr"] and lrs[-1] == meta["lr"] / 2        # the scheduler acted inside the run
