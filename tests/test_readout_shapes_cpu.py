"""The segment ladder and the width list behind tests/test_readout_shapes_gpu.py, without a GPU (tests/readout_ref.py: LADDER,
WIDTHS, ladder_sizes, ladder_batch), and the NaN / Inf rule of the max readout as the reference states it.  This guards the
INPUTS and the REFERENCE, not the kernels."""
import math

import torch

import readout_ref as ref


def test_the_ladder_sits_on_the_batches_of_rows():
    a = ref.RD_AHEAD
    assert a == 8
    for k in (1, 2, 3):
        assert {k * a - 1, k * a, k * a + 1} <= set(ref.LADDER)
    assert {0, 1, 64} <= set(ref.LADDER)
    for order in ("up", "down"):
        sizes = ref.ladder_sizes(order)
        assert sorted(n for n in sizes if n) == sorted(n for n in ref.LADDER if n)
        zeros = [i for i, n in enumerate(sizes) if n == 0]
        assert zeros[0] == 0 and zeros[-1] == len(sizes) - 1 and len(zeros) == 3 and 0 < zeros[1] < len(sizes) - 1
        batch, n_graphs = ref.ladder_batch(order)
        assert n_graphs == len(sizes) and batch.numel() == sum(sizes) and bool((batch[1:] >= batch[:-1]).all())
        seg = ref.seg_ptr_of(batch, n_graphs)
        assert (seg[1:] - seg[:-1]).tolist() == sizes
    assert ref.ladder_sizes("up") != ref.ladder_sizes("down")


def test_the_widths_reach_every_group_shape_in_both_forms():
    lanes = {w: (w + 3) // 4 for w in ref.WIDTHS}
    assert {1, 2, 63, 64, 65, 256, 257, 258} <= set(lanes.values())
    assert {w for w, n in lanes.items() if n == 1} == {1, 2, 3, 4}
    assert any(64 % n != 0 and n < 64 for n in lanes.values())                # groups that straddle wavefronts
    for side in (lambda n: n <= 2, lambda n: 2 < n <= 65, lambda n: n > 256):
        assert {w % 4 == 0 for w, n in lanes.items() if side(n)} == {True, False}
    assert lanes[1030] == 258 and 1030 % 4 == 2 and lanes[1028] == 257 and 1028 % 4 == 0


def test_the_reference_follows_the_strict_compare():
    """NaN in the first row stays and owns arg; NaN later is never taken; +Inf wins at its first occurrence; a segment of
    -Inf returns -Inf with arg at its first row; the backward routes the gradient to exactly that row."""
    nan, inf = math.nan, math.inf
    x = torch.tensor([[nan, 1.0, inf, -inf, 2.0],
                      [3.0, nan, 0.0, -inf, inf],
                      [4.0, 5.0, inf, -inf, inf],
                      [7.0, 7.0, 7.0, 7.0, 7.0]])
    seg = torch.tensor([0, 3, 4])
    out, arg = ref.forward(x, seg, "max")
    assert math.isnan(float(out[0, 0])) and out[0, 1:].tolist() == [5.0, inf, -inf, inf]
    assert arg.tolist() == [[0, 2, 0, 0, 1], [3, 3, 3, 3, 3]]
    go = torch.arange(1.0, 11.0).view(2, 5)
    dx = ref.backward(go, seg, "max", 4, arg)
    assert dx.tolist() == [[1.0, 0.0, 3.0, 4.0, 0.0], [0.0, 0.0, 0.0, 0.0, 5.0], [0.0, 2.0, 0.0, 0.0, 0.0], [6.0, 7.0, 8.0, 9.0, 10.0]]
    s, _ = ref.forward(x, seg, "sum")
    assert torch.isnan(s[0]).tolist() == [True, True, False, False, False] and s[0, 2:].tolist() == [inf, -inf, inf]
    assert ref.same_bits_or_both_nan(s, s.clone()) and not ref.same_bits_or_both_nan(s, torch.zeros_like(s))
    assert not ref.same_bits_or_both_nan(torch.tensor([nan, 1.0]), torch.tensor([nan, 2.0]))
