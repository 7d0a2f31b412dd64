"""The graph-level MLP head without a GPU: GraphHead is the reference's ``mlp`` Sequential (state dict, key list, repr), on CPU
tensors it IS torch's composition bit for bit for the three loss kinds, arguments are checked, the header, the binding and the
host-only queries agree, and the float64 head of head_ref.py is torch's float64 composition and autograd."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import egc_amd
from egc_amd import _C
import callers
import head_ref as ref


@pytest.mark.parametrize("sizes", [[128, 64, 32, 1], [300, 150, 75, 1], [36, 1], [40, 20, 1], [64, 32, 16, 8, 3]])
def test_state_dict_round_trip_key_list_and_repr(sizes):
    theirs, ours = callers.head_mlp(sizes), egc_amd.GraphHead(sizes)
    assert list(ours.state_dict()) == list(theirs.state_dict())
    assert [k for k, _ in ours.named_parameters()] == [k for k, _ in theirs.named_parameters()]
    assert [k for k, _ in ours.named_buffers()] == [k for k, _ in theirs.named_buffers()]
    assert repr(ours) == repr(theirs)
    ours.load_state_dict(theirs.state_dict(), strict=True)
    theirs.load_state_dict(ours.state_dict(), strict=True)
    for a, b in zip(ours.parameters(), theirs.parameters()):
        assert torch.equal(a, b)

    class Net(nn.Module):          # the reference's nets keep it as self.mlp
        def __init__(self, head):
            super().__init__()
            self.mlp = head

    a, b = Net(egc_amd.GraphHead(sizes)), Net(callers.head_mlp(sizes))
    assert list(a.state_dict()) == list(b.state_dict())
    a.load_state_dict(b.state_dict(), strict=True)


def test_other_activation_and_dropout_build_the_reference_children():
    ours = egc_amd.GraphHead([8, 4, 2], act=nn.ELU, dropout=0.25)
    assert [type(m) for m in ours] == [nn.Linear, nn.BatchNorm1d, nn.ELU, nn.Dropout, nn.Linear]
    assert ours[3].p == 0.25


@pytest.mark.parametrize("sizes,g", [([12, 6, 3, 1], 7), ([5, 1], 1), ([6, 3, 2], 4), ([9, 5, 4, 3, 2], 6)])
@pytest.mark.parametrize("kind", [ref.LOSS_NONE, ref.LOSS_L1, ref.LOSS_BCE])
def test_cpu_tensors_take_torchs_composition_bit_for_bit(sizes, g, kind):
    case = ref.make_case(sizes, g, seed=g + kind, kind=kind)
    ours = ref.load_case(egc_amd.GraphHead(sizes), case)
    theirs = ref.load_case(callers.head_mlp(sizes), case)
    xa, xb = case["x"].clone().requires_grad_(True), case["x"].clone().requires_grad_(True)
    y = case["y"]
    if kind == ref.LOSS_BCE:
        y[0, 0] = 1.0                                   # at least one labelled entry
    want = ref.torch_composition(theirs, xa, y, kind)
    got = {ref.LOSS_NONE: lambda: ours(xb), ref.LOSS_L1: lambda: ours.l1_loss(xb, y),
           ref.LOSS_BCE: lambda: ours.bce_with_logits_loss(xb, y)}[kind]()
    assert torch.equal(got, want)
    want.sum().backward()
    got.sum().backward()
    assert torch.equal(xa.grad, xb.grad)
    for a, b in zip(ours.parameters(), theirs.parameters()):
        assert torch.equal(a.grad, b.grad)
    for a, b in zip(ours.buffers(), theirs.buffers()):
        assert torch.equal(a, b)                        # the running statistics moved alike
    theirs.eval()
    assert torch.equal(ours.predict(case["x"]), theirs(case["x"]))
    assert ours.training                                # predict leaves the mode alone
    # the stand-alone losses
    out = theirs(case["x"]).detach()
    if kind == ref.LOSS_L1:
        assert torch.equal(egc_amd.l1_loss(out, y), torch.nn.functional.l1_loss(out, y.view_as(out)))
    if kind == ref.LOSS_BCE:
        ok = y == y
        assert torch.equal(egc_amd.masked_bce_with_logits(out, y),
                           torch.nn.functional.binary_cross_entropy_with_logits(out[ok], y[ok]))


def test_argument_errors():
    with pytest.raises(ValueError, match="positive widths"):
        egc_amd.GraphHead([8])
    with pytest.raises(ValueError, match="positive widths"):
        egc_amd.GraphHead([8, 0, 1])
    head = egc_amd.GraphHead([8, 4, 2])
    x = torch.randn(5, 8)
    with pytest.raises(ValueError, match="one target per output"):
        head.l1_loss(x, torch.randn(5))
    with pytest.raises(ValueError, match="one target per output"):
        head.bce_with_logits_loss(x, torch.randn(4, 2))
    with pytest.raises(ValueError, match="as many targets"):
        egc_amd.l1_loss(torch.randn(4, 2), torch.randn(4))
    with pytest.raises(ValueError, match="as many targets"):
        egc_amd.masked_bce_with_logits(torch.randn(4, 2), torch.randn(3, 2))


def test_one_training_row_raises_value_error_as_batchnorm_does():
    head = egc_amd.GraphHead([8, 4, 2])
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        head(torch.randn(1, 8))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        head.l1_loss(torch.randn(1, 8), torch.randn(1, 2))
    head.eval()
    assert head(torch.randn(1, 8)).shape == (1, 2)
    assert head(torch.randn(0, 8)).shape == (0, 2)
    assert egc_amd.GraphHead([8, 2])(torch.randn(1, 8)).shape == (1, 2)    # no hidden layer: no BatchNorm to object


def test_header_constants_and_signatures_match_the_binding():
    for name, value in [("MAX_LINEARS", _C.HEAD_MAX_LINEARS), ("MAX_WIDTH", _C.HEAD_MAX_WIDTH), ("MAX_OUT", _C.HEAD_MAX_OUT),
                        ("MAX_ROWS", _C.HEAD_MAX_ROWS), ("ROW_TILE", _C.HEAD_ROW_TILE), ("LOSS_NONE", _C.HEAD_LOSS_NONE),
                        ("LOSS_L1", _C.HEAD_LOSS_L1), ("LOSS_BCE_MASKED", _C.HEAD_LOSS_BCE_MASKED)]:
        assert _C.ABI.constants["EGC_HEAD_" + name] == value, name
    assert (_C.HEAD_LOSS_NONE, _C.HEAD_LOSS_L1, _C.HEAD_LOSS_BCE_MASKED) == (ref.LOSS_NONE, ref.LOSS_L1, ref.LOSS_BCE)
    assert (_C.HEAD_MAX_WIDTH, _C.HEAD_MAX_OUT, _C.HEAD_MAX_ROWS, _C.HEAD_ROW_TILE) == (ref.MAX_WIDTH, ref.MAX_OUT, ref.MAX_ROWS,
                                                                                      ref.ROW_TILE)
    assert _C.HEAD_MAX_LINEARS == ref.MAX_LINEARS
    lib = _C.load()
    for name, n_args in (("egc_head_workspace_bytes", 2), ("egc_head_forward_train_f32", 11), ("egc_head_forward_eval_f32", 5),
                         ("egc_head_backward_f32", 14), ("egc_l1_loss_forward_f32", 5), ("egc_l1_loss_backward_f32", 7),
                         ("egc_bce_masked_forward_f32", 5), ("egc_bce_masked_backward_f32", 7), ("egc_head_launches", 0)):
        assert name in _C.SYMBOLS and hasattr(lib, name), name
        assert len(_C.SYMBOLS[name][1]) == n_args, name                # one ctypes argument per declared parameter
    # the struct of the binding has the header's members in the header's order
    assert [f[0] for f in _C.EgcHead._fields_] == [
        "n_linears", "sizes", "weight", "bias", "gamma", "beta", "running_mean", "running_var", "num_batches_tracked", "eps",
        "momentum", "z", "stats", "affine", "dz", "g", "coef", "d_weight", "d_bias"]


def _descriptor(sizes):
    d = _C.EgcHead()
    d.n_linears = len(sizes) - 1
    for i, s in enumerate(sizes):
        d.sizes[i] = s
    keep = []
    for i in range(len(sizes) - 1):                     # any non-null address: the query and the checks never touch them
        buf = (C.c_float * 4)()
        keep.append(buf)
        d.weight[i] = d.bias[i] = C.addressof(buf)
    return d, keep


def test_host_only_queries_and_envelope_errors_before_any_launch():
    lib = _C.load()
    n0 = lib.egc_head_launches()
    d, _keep = _descriptor([300, 150, 75, 1])
    assert lib.egc_head_workspace_bytes(C.byref(d), 128) >= 8 * 2 * 151 * 8
    assert lib.egc_head_workspace_bytes(C.byref(d), _C.HEAD_MAX_ROWS) > 0
    assert lib.egc_head_workspace_bytes(C.byref(d), _C.HEAD_MAX_ROWS + 1) == 0
    assert lib.egc_head_workspace_bytes(C.byref(d), -1) == 0
    for bad in ([385, 4, 1], [8, 385, 1], [8, 4, 65], [8, 4, 4, 4, 4, 1]):
        if len(bad) - 1 > _C.HEAD_MAX_LINEARS:
            db = _C.EgcHead()
            db.n_linears = len(bad) - 1
        else:
            db, _k = _descriptor(bad)
        assert lib.egc_head_workspace_bytes(C.byref(db), 16) == 0, bad
        assert lib.egc_head_forward_eval_f32(C.byref(db), None, 16, None, None) == 4, bad          # EGC_ERR_UNSUPPORTED
    dz, _k = _descriptor([8, 0, 1])
    assert lib.egc_head_forward_eval_f32(C.byref(dz), None, 16, None, None) == 1                   # EGC_ERR_INVALID
    # training with one row, a missing pointer, an unknown loss: EGC_ERR_INVALID, nothing launched
    assert lib.egc_head_forward_train_f32(C.byref(d), None, 1, 0, None, None, None, None, 0, None, None) == 1
    assert lib.egc_head_forward_train_f32(C.byref(d), None, 16, 7, None, None, None, None, 0, None, None) == 1
    assert lib.egc_head_backward_f32(C.byref(d), None, 16, 0, None, None, None, None, None, 1, None, 0, None, None) == 1
    assert lib.egc_l1_loss_forward_f32(None, None, -1, None, None) == 1
    assert lib.egc_bce_masked_backward_f32(None, None, None, None, 4, None, None) == 1
    assert lib.egc_head_launches() == n0


def test_dispatch_table_of_the_reference_module():
    assert (ref.ROW_TILE, ref.LOSS_NONE, ref.LOSS_L1, ref.LOSS_BCE) == (_C.HEAD_ROW_TILE, _C.HEAD_LOSS_NONE, _C.HEAD_LOSS_L1,
                                                                       _C.HEAD_LOSS_BCE_MASKED)
    assert ref.grid(128, [168, 84, 42, 1], 0) == (8, 2) and ref.grid(17, [300, 150, 75, 1], 1) == (2, 2)
    assert ref.launches([168, 84, 42, 1], ref.LOSS_L1) == (3, 4)
    assert ref.launches([168, 84, 42, 1], ref.LOSS_NONE, want_dx=False) == (3, 4)
    assert ref.launches([168, 84, 42, 1], ref.LOSS_L1, want_params=False) == (3, 3)
    assert ref.launches([36, 1], ref.LOSS_NONE, want_dx=False) == (1, 1)
    assert ref.launches([36, 1], ref.LOSS_L1, train=False) == (1, 0)
    cases = ref.gpu_cases()
    assert {tuple(s) for s, _, _ in cases} >= {tuple(s) for s in ref.SIZES}
    assert {g for _, g, _ in cases} >= set(ref.ROWS) | {2048}
    assert {k for _, _, k in cases} == {ref.LOSS_NONE, ref.LOSS_L1, ref.LOSS_BCE}


@pytest.mark.parametrize("sizes,g,kind", ref.gpu_cases())
def test_float64_head_is_torchs_float64_composition_and_autograd(sizes, g, kind):
    case = ref.make_case(sizes, g, seed=g + len(sizes), kind=kind)
    if kind == ref.LOSS_BCE:
        case["y"][0, 0] = 0.0
    head = ref.load_case(egc_amd.GraphHead(sizes), case).double()     # float64 on the CPU: torch's operators
    x = case["x"].double().requires_grad_(True)
    grad = torch.randn(g, sizes[-1], generator=torch.Generator().manual_seed(g)).double()
    res = ref.head64(case, kind, grad=grad)
    y = case["y"].double()
    val = ref.torch_composition(head, x, y, kind)
    if kind == ref.LOSS_NONE:
        val.backward(grad)
    else:
        val.backward()
        assert abs(res["loss"] - float(val.detach())) <= 1e-12 * max(1.0, abs(float(val.detach())))

    def close(a, b):
        return float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max()))

    if kind == ref.LOSS_NONE:
        assert close(res["out"], val.detach())
    assert close(res["dx"], x.grad)
    lin = [m for m in head if isinstance(m, nn.Linear)]
    bn = [m for m in head if isinstance(m, nn.BatchNorm1d)]
    for i, m in enumerate(lin):
        assert close(res["dw"][i], m.weight.grad) and close(res["db"][i], m.bias.grad), i
    for i, m in enumerate(bn):
        assert close(res["dgamma"][i], m.weight.grad) and close(res["dbeta"][i], m.bias.grad), i
