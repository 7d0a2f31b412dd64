"""``egc_amd.Adam``: the optimizer of every config of the reference as one launch per parameter group (egc_adam.hip).

The reference trains all its nets with ``Adam(model.parameters(), lr=hparams["lr"], weight_decay=hparams["wd"])`` under a
``ReduceLROnPlateau`` (experiments/*/configs.py, exp_config.py).  torch composes that step from about a dozen ``_foreach_*``
launches per chunk of tensors; here ``step()`` is ONE launch that updates the parameter and both moments of every tensor of a
group and, with ``zero_grad=True``, writes zeros to the gradients it has read (instead of the launches of
``zero_grad(set_to_none=False)``).  It records into a ``GraphedStep``: the tensors' addresses travel in the kernel arguments,
and the learning rate is a device scalar the kernel reads, so a scheduler changes the rate of a recorded step.
Arithmetic, capture argument, bounds and timings: DESIGN.md section 3.33; C ABI: include/egc_optim.h.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _C, _optim
from .graph import _device_guard, _stream_ptr

_TORCH_DEFAULTS = None


def _torch_defaults() -> dict:
    """The group keys of torch.optim.Adam in this torch (foreach, capturable, fused, ... beyond the six this class acts on):
    a state dict carries them, so that it loads into torch's class."""
    global _TORCH_DEFAULTS
    if _TORCH_DEFAULTS is None:
        _TORCH_DEFAULTS = dict(torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).defaults)
    return _TORCH_DEFAULTS


class _Owned:
    """What the optimizer owns for one parameter group: both moment buffers, the step words, the learning-rate scalar and the
    host descriptor array of the launch."""
    __slots__ = ("device", "numels", "state_off", "step_off", "blocks", "exp_avg", "exp_avg_sq", "steps", "lr", "desc")


class Adam(torch.optim.Optimizer):
    """Drop-in for ``torch.optim.Adam`` at the reference's settings: Adam with L2 weight decay added to the gradient (not
    AdamW), no amsgrad, no maximize; float32, contiguous parameters and gradients on a ROCm device.  Parameter groups carry
    their own hyper-parameters, and a ``torch.optim.lr_scheduler`` accepts it.

    ``step(zero_grad=True)`` also zeroes every ``.grad`` it read (the same tensor objects stay attached).  A parameter whose
    ``.grad`` is None is left out and its step count does not advance, as in torch.

    ``param_groups[i]["lr"]`` is a 0-dim float64 tensor on the parameters' device, read by the kernel.  torch's schedulers
    write a tensor-valued ``lr`` in place, so the new rate reaches a recorded step with nothing recorded again; a Python float
    assigned to it later is copied into the scalar by the next ``step()`` outside a capture (inside one it raises).  The other
    hyper-parameters are call arguments: a recording keeps the values it was made with.

    ``state[p]`` has torch's keys once ``p`` has taken a step: ``exp_avg`` and ``exp_avg_sq`` are views into one owned buffer
    each per group, ``step`` a view of the tensor's int32 device counter.  ``state_dict()`` / ``load_state_dict()`` use torch's
    layout (``step`` as a float32 scalar, ``lr`` as a float) and exchange with ``torch.optim.Adam`` in both directions.
    There is no CPU fallback: ``step()`` on CPU tensors raises."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, maximize=False):
        if isinstance(lr, torch.Tensor) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not 0.0 <= float(lr):
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 0: {betas[0]}")
        if not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameter at index 1: {betas[1]}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        defaults = dict(_torch_defaults())
        defaults.update(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        self._owned = []
        super().__init__(params, defaults)

    def __getstate__(self):
        raise TypeError("egc_amd.Adam cannot be pickled or deep-copied: it owns device buffers (both moments, the step words, the "
                        "learning-rate scalar) whose addresses a recording may hold; carry its state with state_dict() / "
                        "load_state_dict()")

    # ---- groups -----------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_group(group):
        if group["amsgrad"]:
            raise NotImplementedError("egc_amd.Adam: amsgrad is not implemented (no config of the reference uses it)")
        if group["maximize"]:
            raise NotImplementedError("egc_amd.Adam: maximize is not implemented (no config of the reference uses it)")

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            self._owned.append(self._own(group))
        except Exception:
            self.param_groups.pop()
            raise

    def _own(self, group) -> _Owned:
        params = group["params"]
        for p in params:
            if p.dtype != torch.float32:
                raise ValueError(f"egc_amd.Adam: parameters must be float32 (got {p.dtype})")
            if not p.is_contiguous():
                raise ValueError(f"egc_amd.Adam: parameters must be contiguous (got strides {p.stride()} for shape {tuple(p.shape)})")
            if p.device != params[0].device:
                raise ValueError(f"egc_amd.Adam: the parameters of a group must live on one device (got {p.device} and "
                                 f"{params[0].device})")
        own = _Owned()
        dev = own.device = params[0].device if params else torch.device("cpu")
        n = len(params)
        own.numels = [p.numel() for p in params]
        numels, blocks, offsets = (C.c_int64 * max(n, 1))(*own.numels), (C.c_int32 * max(n, 1))(), (C.c_int64 * max(n, 1))()
        total = _optim.load().egc_adam_plan(numels, n, blocks, offsets)
        if total < 0:
            raise ValueError("egc_amd.Adam: a parameter of 2^31 elements or more, or a group of 2^32 or more")
        own.blocks, own.state_off, own.step_off, words = list(blocks[:n]), list(offsets[:n]), [], 0
        for b in own.blocks:
            own.step_off.append(words)
            words += b
        own.exp_avg = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        own.exp_avg_sq = torch.zeros(max(total, 4), dtype=torch.float32, device=dev)
        own.steps = torch.zeros(max(words, 1), dtype=torch.int32, device=dev)
        lr = group["lr"]
        own.lr = torch.tensor(lr.item() if isinstance(lr, torch.Tensor) else float(lr), dtype=torch.float64, device=dev)
        group["lr"] = own.lr
        own.desc = (_optim.EgcAdamTensor * max(n, 1))()
        return own

    def _views(self, own, k, p):
        off, numel = own.state_off[k], own.numels[k]
        return dict(step=own.steps[own.step_off[k]], exp_avg=own.exp_avg[off:off + numel].view(p.shape),
                    exp_avg_sq=own.exp_avg_sq[off:off + numel].view(p.shape))

    def _sync_lr(self, group, own):
        lr = group["lr"]
        if lr is not own.lr:        # a float (or another tensor) assigned since the last step
            if own.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("egc_amd.Adam: param_groups[...]['lr'] was replaced and a capture is under way: the recorded "
                                   "step reads the optimizer's device scalar; change it in place (lr.fill_(value), as torch's "
                                   "schedulers do) or assign before recording")
            own.lr.fill_(lr.item() if isinstance(lr, torch.Tensor) else float(lr))
            group["lr"] = own.lr

    # ---- the step ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure=None, *, zero_grad=False):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group, own in zip(self.param_groups, self._owned):
            self._check_group(group)
            dev, desc, n, touched = own.device, own.desc, 0, []
            for k, p in enumerate(group["params"]):
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32 or p.dtype != torch.float32:
                    raise ValueError(f"egc_amd.Adam: parameters and gradients must be float32 (got {p.dtype} / {g.dtype})")
                if g.is_sparse or not g.is_contiguous() or not p.is_contiguous():
                    raise ValueError("egc_amd.Adam: parameters and gradients must be dense and contiguous")
                if dev.type != "cuda" or not p.is_cuda or not g.is_cuda:
                    raise RuntimeError(f"egc_amd.Adam: parameters and gradients must live on a ROCm device (got {p.device} / "
                                       f"{g.device}); the step is HIP-only, there is no CPU fallback")
                if p.device != dev or g.device != dev or g.shape != p.shape or p.numel() != own.numels[k]:
                    raise ValueError(f"egc_amd.Adam: parameter {k} or its gradient changed device or shape since the optimizer "
                                     f"was built ({tuple(p.shape)} on {p.device}, grad {tuple(g.shape)} on {g.device})")
                d = desc[n]
                d.p, d.g = p.data_ptr(), g.data_ptr()
                d.state_offset, d.step_offset, d.numel = own.state_off[k], own.step_off[k], own.numels[k]
                if "step" not in self.state[p]:
                    self.state[p].update(self._views(own, k, p))
                touched.append(p)
                if zero_grad:
                    touched.append(g)
                n += 1
            if n == 0:
                continue
            self._sync_lr(group, own)
            beta1, beta2 = group["betas"]
            with _device_guard(dev):
                _C.check(_optim.load().egc_adam_step_f32(desc, n, own.exp_avg.data_ptr(), own.exp_avg_sq.data_ptr(),
                                                         own.steps.data_ptr(), own.lr.data_ptr(), beta1, beta2, group["eps"],
                                                         group["weight_decay"], 1 if zero_grad else 0, _stream_ptr(dev)),
                         "egc_adam_step_f32")
            # the kernel wrote through raw addresses: the layers' caches of packed weights are keyed on the version counters
            touched += [own.exp_avg, own.exp_avg_sq, own.steps]
            torch.autograd.graph.increment_version(touched)
        return loss

    # ---- state dict -------------------------------------------------------------------------------------------------
    def state_dict(self):
        """torch's layout; synchronises (the step counts and learning rates are read back)."""
        sd = super().state_dict()
        steps = [own.steps.cpu() for own in self._owned]
        state = {}
        for gi, (group, packed) in enumerate(zip(self.param_groups, sd["param_groups"])):
            lr = group["lr"]
            packed["lr"] = lr.item() if isinstance(lr, torch.Tensor) else float(lr)
            for k, p in enumerate(group["params"]):
                if p in self.state and "step" in self.state[p]:
                    t = int(steps[gi][self._owned[gi].step_off[k]])
                    state[packed["params"][k]] = dict(self.state[p], step=torch.tensor(float(t), dtype=torch.float32))
        sd["state"] = state
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        """A state dict of this class or of ``torch.optim.Adam``: the moments and step counts are copied into the owned buffers
        (whose addresses a recording holds) and the learning rate into the device scalar."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        for group, own in zip(self.param_groups, self._owned):
            lr = group["lr"]
            if lr is not own.lr:
                own.lr.fill_(lr.item() if isinstance(lr, torch.Tensor) else float(lr))
                group["lr"] = own.lr
            for k, p in enumerate(group["params"]):
                loaded = self.state.get(p)
                views = self._views(own, k, p)
                words = own.steps[own.step_off[k]:own.step_off[k] + own.blocks[k]]
                if not loaded:
                    views["exp_avg"].zero_()
                    views["exp_avg_sq"].zero_()
                    words.zero_()
                    self.state.pop(p, None)
                    continue
                views["exp_avg"].copy_(loaded["exp_avg"])
                views["exp_avg_sq"].copy_(loaded["exp_avg_sq"])
                words.fill_(int(round(float(loaded["step"]))))
                self.state[p] = views
