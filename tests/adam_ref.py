"""torch.optim.Adam's step (L2 weight decay, no amsgrad, no maximize) restated in numpy float64, one tensor at a time:

    g' = g + wd * p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2;  t += 1
    p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

Every tensor carries its own step count; a tensor whose gradient is None is skipped and its count does not advance.  Also the
distances and the bound of the GPU tests (tests/test_adam_gpu.py) and a Python restatement of egc_adam_plan."""
import numpy as np

BLOCK_ELEMS = 1024      # EGC_ADAM_BLOCK_ELEMS, restated (tests/test_adam_cpu.py compares it with the header's)
MAX_TENSORS = 120       # EGC_ADAM_MAX_TENSORS, restated


def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """(p, m, v, t) after one step of one tensor, all float64; unchanged if g is None."""
    if g is None:
        return p, m, v, t
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    if wd != 0:
        g = g + wd * p
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    t = int(t) + 1
    step_size = lr / (1 - b1 ** t)
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - step_size * m / denom, m, v, t


class RefAdam:
    """The optimizer over lists of tensors: ``groups`` = [dict(params=[arrays], lr=, betas=, eps=, wd=)], optionally with a
    given state m=[arrays], v=[arrays], t=[ints] (default: zeros)."""

    def __init__(self, groups):
        self.groups = [dict(g) for g in groups]
        for g in self.groups:
            g["params"] = [np.array(p, dtype=np.float64) for p in g["params"]]
            g["m"] = [np.array(a, dtype=np.float64) for a in g["m"]] if "m" in g else [np.zeros_like(p) for p in g["params"]]
            g["v"] = [np.array(a, dtype=np.float64) for a in g["v"]] if "v" in g else [np.zeros_like(p) for p in g["params"]]
            g["t"] = [int(t) for t in g["t"]] if "t" in g else [0] * len(g["params"])

    def step(self, grads):
        """``grads``: per group a list of arrays or None."""
        for g, gs in zip(self.groups, grads):
            for k, grad in enumerate(gs):
                g["params"][k], g["m"][k], g["v"][k], g["t"][k] = adam_step(
                    g["params"][k], grad, g["m"][k], g["v"][k], g["t"][k], g["lr"], g.get("betas", (0.9, 0.999)),
                    g.get("eps", 1e-8), g.get("wd", 0.0))


def plan(numels):
    """egc_adam_plan restated: (workgroups per tensor, 16-byte aligned state offsets in elements, state length)."""
    blocks, offsets, total = [], [], 0
    for n in numels:
        blocks.append(max(1, -(-n // BLOCK_ELEMS)))
        offsets.append(total)
        total += -(-n // 4) * 4
    return blocks, offsets, total


def launches(n_tensors):
    return -(-n_tensors // MAX_TENSORS) if n_tensors > 0 else 0


def ulp32(x):
    """One unit in the last place of float32 at |x| (the spacing above |x|; the smallest subnormal at 0)."""
    x = np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def floor_of_step(p_old, p_new):
    """Per element: 1 ulp(max(|p_old|, |p_new|)) + 2^-20 |p_new - p_old| -- the rounding of the stored parameter plus sixteen
    float32 roundings (16 * 2^-24) of the update, whatever the order of its products.  The one floor of the bound
    max(floor, 4 x d32): applied alike to the parameter and to both moments (old and new value of the quantity judged)."""
    p_old, p_new = np.asarray(p_old, dtype=np.float64), np.asarray(p_new, dtype=np.float64)
    return ulp32(np.maximum(np.abs(p_old), np.abs(p_new))) + 2.0 ** -20 * np.abs(p_new - p_old)


def dist(a, ref):
    """max |a - ref| (0 for an empty tensor)."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max()) if a.size else 0.0
