"""egc_amd.Adam without a GPU: the float64 oracle of the GPU tests (tests/adam_ref.py) against torch.optim.Adam, the host plan
of the launch (egc_adam_plan) against its Python restatement, the second public header's binding, and the constructor's and
step's validation."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import adam_ref
import egc_amd
from egc_amd import _C, _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 1e-3])
def test_oracle_agrees_with_torch_adam_in_float64(wd):
    """5 steps, two groups with different lr, one parameter whose grad is None on odd steps: 1e-14 relative.  (This test is
    about the oracle alone: it is the one test of the two files that passes without egc_amd.Adam.)"""
    rng = np.random.default_rng(0)
    shapes = [[(7, 5), (11,), (3, 4)], [(6,), (2, 9)]]
    lrs = [1e-2, 3e-3]
    init = [[rng.standard_normal(s) for s in group] for group in shapes]
    params = [[torch.nn.Parameter(torch.from_numpy(a.copy())) for a in group] for group in init]
    opt = torch.optim.Adam([dict(params=ps, lr=lr) for ps, lr in zip(params, lrs)], weight_decay=wd)
    ref = adam_ref.RefAdam([dict(params=group, lr=lr, wd=wd) for group, lr in zip(init, lrs)])
    for step in range(5):
        grads = [[rng.standard_normal(s) for s in group] for group in shapes]
        if step % 2 == 1:
            grads[0][1] = None
        for ps, gs in zip(params, grads):
            for p, g in zip(ps, gs):
                p.grad = None if g is None else torch.from_numpy(g.copy())
        opt.step()
        ref.step(grads)
    for gi, ps in enumerate(params):
        for k, p in enumerate(ps):
            st = opt.state[p]
            assert int(st["step"]) == ref.groups[gi]["t"][k]
            for got, want in ((p.detach(), ref.groups[gi]["params"][k]), (st["exp_avg"], ref.groups[gi]["m"][k]),
                              (st["exp_avg_sq"], ref.groups[gi]["v"][k])):
                assert np.abs(got.numpy() - want).max() <= 1e-14 * np.abs(want).max()
    assert ref.groups[0]["t"] == [5, 3, 5]


# ---- the plan -----------------------------------------------------------------------------------------------------------
def _lib():
    from egc_amd import _optim
    return _optim, _optim.load()


def _plan(lib, numels):
    n = len(numels)
    arr = (C.c_int64 * max(n, 1))(*numels)
    blocks, offsets = (C.c_int32 * max(n, 1))(), (C.c_int64 * max(n, 1))()
    total = lib.egc_adam_plan(arr, n, blocks, offsets)
    return list(blocks[:n]), list(offsets[:n]), total


def test_plan_equals_its_restatement():
    _optim, lib = _lib()
    assert adam_ref.BLOCK_ELEMS == _optim.ADAM_BLOCK_ELEMS and adam_ref.MAX_TENSORS == _optim.ADAM_MAX_TENSORS
    cap = lib.egc_adam_max_tensors()
    assert cap == _optim.ADAM_MAX_TENSORS
    be = _optim.ADAM_BLOCK_ELEMS
    pool = [0, 1, 3, 4, 5, 255, 256, 257, be - 1, be, be + 1]
    rng = np.random.default_rng(1)
    for n in (1, cap, cap + 1):
        for trial in range(4):
            numels = [pool[(trial + k) % len(pool)] for k in range(n)] if trial == 0 else [int(x) for x in rng.choice(pool, size=n)]
            blocks, offsets, total = _plan(lib, numels)
            want = adam_ref.plan(numels)
            assert (blocks, offsets, total) == want
            assert all(o % 4 == 0 for o in offsets) and total % 4 == 0
            assert all(o2 - o1 >= m for o1, o2, m in zip(offsets, offsets[1:] + [total], numels))      # slices do not overlap
            prefix = np.concatenate([[0], np.cumsum(blocks)])
            assert all(b >= 1 and (b - 1) * be < max(m, 1) <= b * be for b, m in zip(blocks, numels))
            assert prefix[-1] == sum(max(1, -(-m // be)) for m in numels)
        assert lib.egc_adam_launches(n) == adam_ref.launches(n)
    assert (lib.egc_adam_launches(cap), lib.egc_adam_launches(cap + 1), lib.egc_adam_launches(0), lib.egc_adam_launches(-3)) == (1, 2, 0, 0)
    assert _plan(lib, []) == ([], [], 0)
    one = (C.c_int64 * 1)(1)
    assert lib.egc_adam_plan(one, -1, (C.c_int32 * 1)(), (C.c_int64 * 1)()) == -1
    assert lib.egc_adam_plan(None, 1, (C.c_int32 * 1)(), (C.c_int64 * 1)()) == -1
    assert lib.egc_adam_plan(one, 1, None, (C.c_int64 * 1)()) == -1
    assert _plan(lib, [2 ** 31])[2] == -1 and _plan(lib, [-1])[2] == -1 and _plan(lib, [2 ** 31 - 1])[2] == 2 ** 31
    assert _plan(lib, [2 ** 31 - 4, 2 ** 31 - 4])[2] == 2 ** 32 - 8 and _plan(lib, [2 ** 31 - 4, 2 ** 31 - 4, 8])[2] == -1


def test_step_rejects_bad_arguments_before_any_launch():
    """Null pointers, negative counts and a tensor of 2^31 elements return EGC_ERR_INVALID from the host checks: nothing
    is launched (this runs without a GPU, the counter of launches stays)."""
    _optim, lib = _lib()
    T = _optim.EgcAdamTensor
    n0 = lib.egc_adam_launch_count()
    ok = (T * 1)(T(16, 32, 0, 0, 4))
    buf = 4096          # (a non-null, aligned address; never dereferenced: every call below fails its checks)
    args = (buf, buf, buf, buf, 0.9, 0.999, 1e-8, 0.0, 0, None)
    assert lib.egc_adam_step_f32(ok, -1, *args) == _C.ERR_INVALID
    assert lib.egc_adam_step_f32(None, 1, *args) == _C.ERR_INVALID
    for hole in range(4):
        bad = list(args)
        bad[hole] = None
        assert lib.egc_adam_step_f32(ok, 1, *bad) == _C.ERR_INVALID
    for tensor in (T(None, 32, 0, 0, 4), T(16, None, 0, 0, 4), T(16, 32, 0, 0, 2 ** 31), T(16, 32, 0, 0, -1), T(16, 32, 2, 0, 4),
                   T(18, 32, 0, 0, 4)):
        assert lib.egc_adam_step_f32((T * 2)(ok[0], tensor), 2, *args) == _C.ERR_INVALID
    assert lib.egc_adam_step_f32(ok, 0, *args) == _C.OK          # nothing to do
    assert lib.egc_adam_launch_count() == n0


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_second_header_is_read_and_every_symbol_is_exported():
    _optim, lib = _lib()
    with open(os.path.join(ROOT, "include", "egc_optim.h")) as f:
        abi = _abi.read_header(f.read())
    assert set(abi.prototypes) == set(_optim.SYMBOLS) == {"egc_adam_step_f32", "egc_adam_plan", "egc_adam_launches",
                                                         "egc_adam_max_tensors", "egc_adam_launch_count"}
    raw = C.CDLL(_C.lib_path())
    for name in abi.prototypes:
        assert hasattr(raw, name), name
    P, I, L, D = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    restype, args = _optim.SYMBOLS["egc_adam_step_f32"]
    assert restype is C.c_int and issubclass(args[0], C._Pointer) and args[0]._type_ is _optim.EgcAdamTensor
    assert args[1:] == [L, P, P, P, P, D, D, D, D, I, P]
    assert _optim.SYMBOLS["egc_adam_plan"] == (L, [P, L, P, P]) and _optim.SYMBOLS["egc_adam_launches"] == (L, [L])
    assert _optim.SYMBOLS["egc_adam_max_tensors"] == (I, [])
    T = _optim.EgcAdamTensor
    assert C.sizeof(T) == 32 and (T.p.offset, T.g.offset, T.state_offset.offset, T.step_offset.offset, T.numel.offset) == (0, 8, 16, 20, 24)
    assert abi.constants == {"EGC_ADAM_MAX_TENSORS": 120, "EGC_ADAM_BLOCK_ELEMS": 1024} and not abi.enums
    # the new table stands beside _C.SYMBOLS, it does not touch it
    assert not set(_optim.SYMBOLS) & set(_C.SYMBOLS) and len(_C.SYMBOLS) == 128
    assert not any(k.startswith("EGC_ADAM") for k in _C.ABI.constants) and "egc_adam_tensor" not in _C.ABI.structs
    # a full launch fits the 4 KB of kernel arguments: per tensor p, g (8 each), state offset, step offset, numel and a prefix
    # entry (4 each), one more prefix entry, and 88 bytes of pointers and hyper-parameters
    assert (8 + 8 + 4 + 4 + 4 + 4) * _optim.ADAM_MAX_TENSORS + 4 + 88 <= 4096


# ---- the class ----------------------------------------------------------------------------------------------------------
def _params(*shapes, dtype=torch.float32):
    torch.manual_seed(0)
    return [torch.nn.Parameter(torch.randn(*s, dtype=dtype)) for s in shapes]


def test_constructor_validation():
    ps = _params((3, 4), (5,))
    for kw in (dict(lr=-1.0), dict(eps=-1e-8), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):
            egc_amd.Adam(ps, **kw)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        egc_amd.Adam(ps, amsgrad=True)
    with pytest.raises(NotImplementedError, match="maximize"):
        egc_amd.Adam(ps, maximize=True)
    with pytest.raises(NotImplementedError, match="amsgrad"):
        egc_amd.Adam([dict(params=ps[:1]), dict(params=ps[1:], amsgrad=True)])
    with pytest.raises(ValueError, match="float32"):
        egc_amd.Adam(_params((3,), dtype=torch.float64))
    with pytest.raises(ValueError, match="contiguous"):
        egc_amd.Adam([torch.nn.Parameter(torch.randn(4, 6).t())])
    with pytest.raises(ValueError):
        egc_amd.Adam([])
    with pytest.raises(TypeError):
        egc_amd.Adam(ps[0])
    with pytest.raises(ValueError, match="1-element"):
        egc_amd.Adam(ps, lr=torch.tensor([1e-3, 1e-2]))
    with pytest.raises(TypeError):
        egc_amd.Adam(ps, 1e-3, (0.9, 0.999), 1e-8, 0, False, True)          # maximize is keyword-only
    import copy
    import pickle
    opt = egc_amd.Adam(ps)
    with pytest.raises(TypeError, match="state_dict"):                      # it owns device buffers: no silent half copy
        copy.deepcopy(opt)
    with pytest.raises(TypeError, match="state_dict"):
        pickle.dumps(opt)


def test_step_validation_and_no_cpu_fallback():
    ps = _params((3, 4), (5,))
    opt = egc_amd.Adam(ps, lr=1e-2)
    assert opt.step() is None                                   # no gradients: nothing to do, nothing raised
    assert opt.step(lambda: 1.5) == 1.5
    if hasattr(ps[0], "grad_dtype"):
        ps[0].grad_dtype = None                                  # (this torch otherwise refuses the assignment itself)
    ps[0].grad = torch.zeros(3, 4, dtype=torch.float64)
    with pytest.raises(ValueError, match="float32"):
        opt.step()
    ps[0].grad = None
    ps[1].grad = torch.zeros(10)[::2]
    with pytest.raises(ValueError, match="contiguous"):
        opt.step()
    ps[1].grad = torch.zeros(5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step(zero_grad=True)
    assert opt.state_dict()["state"] == {}                       # a failed step leaves no state behind
    opt.param_groups[0]["amsgrad"] = True
    with pytest.raises(NotImplementedError):
        opt.step()


def test_groups_keys_and_empty_state_dict_equal_torchs():
    ps = _params((3, 4), (5,), (2, 2))
    groups = lambda: [dict(params=ps[:2]), dict(params=ps[2:], lr=0.5, betas=(0.8, 0.9), eps=1e-6, weight_decay=1e-3)]  # noqa: E731
    ours, theirs = egc_amd.Adam(groups(), lr=3e-3, weight_decay=1e-4), torch.optim.Adam(groups(), lr=3e-3, weight_decay=1e-4)
    assert isinstance(ours, torch.optim.Optimizer)
    for a, b in zip(ours.param_groups, theirs.param_groups):
        assert list(a) == list(b)
        assert {k: v for k, v in a.items() if k not in ("params", "lr")} == {k: v for k, v in b.items() if k not in ("params", "lr")}
        lr = a["lr"]
        assert isinstance(lr, torch.Tensor) and lr.dtype == torch.float64 and lr.dim() == 0 and lr.item() == b["lr"]
    assert ours.param_groups[0]["lr"] is not ours.param_groups[1]["lr"]
    assert ours.state_dict() == theirs.state_dict()
    # a tensor lr is accepted; each group owns its scalar
    t = egc_amd.Adam(groups(), lr=torch.tensor(0.25))
    assert t.param_groups[0]["lr"].item() == 0.25 and t.param_groups[1]["lr"].item() == 0.5
    # a scheduler accepts it and writes the scalar in place: exactly the double it computed
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(ours, "min", factor=0.5, patience=0)
    held = [g["lr"] for g in ours.param_groups]
    sched.step(1.0)
    sched.step(2.0)
    assert [g["lr"] for g in ours.param_groups] == held and all(g["lr"] is h for g, h in zip(ours.param_groups, held))
    assert ours.param_groups[0]["lr"].item() == 3e-3 * 0.5 and ours.param_groups[1]["lr"].item() == 0.25
    # torch's empty state dict loads, learning rate included
    ours.load_state_dict(theirs.state_dict())
    assert ours.param_groups[0]["lr"] is held[0] and held[0].item() == 3e-3 and ours.state_dict() == theirs.state_dict()
    theirs.load_state_dict(ours.state_dict())
    assert theirs.param_groups[1]["lr"] == 0.5
