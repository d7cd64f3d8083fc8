"""HipAdamW / HipAdam: the optimizer step of the training hot path as ONE kernel launch over every parameter tensor
(csrc/optim.hip, ``ffa_adamw_multi``: three launches for the U-Net's 186 tensors).

Drop-in for ``torch.optim.AdamW`` / ``torch.optim.Adam`` as the reference constructs them
(flair_hub/tasks/tasks_module.py:385-389: lr, betas, weight_decay; amsgrad / foreach / differentiable are not used there
and are refused here).  Same update rule and operation order as torch's fused implementation and the SAME state layout
(``step`` -- a device f32 scalar per parameter --, ``exp_avg``, ``exp_avg_sq``), so ``state_dict()`` /
``load_state_dict()`` are interchangeable with torch's optimizer and LR schedulers see the usual ``param_groups``.
``load_state_dict()`` takes a state saved by torch's optimizer in any of its modes -- the default one keeps ``step`` on the
host and says ``capturable: False`` -- and moves it to this layout; ``step()`` refuses, before it launches anything, a
state that is not in it (the kernel would dereference a host address).
``lr`` may be a float or a device tensor (the captured step keeps it on the device: flairhip.graph.make_capturable);
everything the step launches is capturable into a hipGraph.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Tuple

import torch

from . import lib as _l


class HipAdamW(torch.optim.Optimizer):
    decoupled = True  # AdamW: p -= lr * wd * p;  Adam: g += wd * p

    def __init__(self, params: Iterable, lr=1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, maximize: bool = False, capturable: bool = True):
        if amsgrad:
            raise NotImplementedError("HipAdamW: amsgrad is not implemented (the reference does not use it)")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0 or eps < 0 or weight_decay < 0:
            raise ValueError("HipAdamW: invalid hyper-parameter")
        # the keys torch's Adam / AdamW keep in their param_groups (2.10: AdamW = Adam with decoupled_weight_decay), so that
        # a state dict moves between the two implementations without changing the update rule
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False,
                                      maximize=maximize, capturable=capturable, foreach=None, fused=None,
                                      differentiable=False, decoupled_weight_decay=self.decoupled))
        self._tables = {}  # group index -> (pointer key, ctypes arrays): rebuilt only when a tensor moved

    def _arrays(self, gi, params):
        st = self.state
        try:
            key = tuple((p.data_ptr(), p.grad.data_ptr(), st[p]["exp_avg"].data_ptr(), st[p]["exp_avg_sq"].data_ptr(),
                         st[p]["step"].data_ptr(), p.numel()) for p in params)
        except (AttributeError, KeyError):  # an entry that is no tensor, or is missing: say which
            for p in params:
                self._check_state(p, st[p])
            raise
        hit = self._tables.get(gi)
        if hit is None or hit[0] != key:
            for p in params:  # new addresses: look at what they belong to before the kernel is handed them
                self._check_state(p, st[p])
            n = len(params)
            cols = [(C.c_void_p * n)(*[k[j] for k in key]) for j in range(5)]
            hit = (key, cols, (C.c_longlong * n)(*[k[5] for k in key]))
            self._tables[gi] = hit
        return hit

    def load_state_dict(self, state_dict) -> None:
        """Accepts what ``state_dict()`` of this class or of torch's Adam / AdamW gives, in any of torch's modes: ``step`` a
        Python number, a CPU tensor (torch's default, not capturable and not fused -- what the reference constructs), an
        f64 tensor or a device tensor; the moments on any device.  ``torch.optim.Optimizer.load_state_dict`` leaves ``step``
        as it was saved unless the SAVED groups say capturable or fused, and takes ``capturable`` from the saved groups;
        the kernel reads ``step`` and ``lr`` through device pointers.  So afterwards: every ``step`` is a 0-dim f32 tensor
        on its parameter's device, ``exp_avg`` / ``exp_avg_sq`` are contiguous f32 tensors there, ``capturable`` is True in
        every group, the keys this class fixes (amsgrad, foreach, fused, differentiable, decoupled_weight_decay) are its
        own, and a device-tensor ``lr`` this optimizer held before the load is the same tensor with the loaded value in it
        (a captured step reads that address); a loaded tensor ``lr`` where a number was held becomes a number."""
        for g in state_dict["param_groups"]:
            if g.get("amsgrad", False):
                raise NotImplementedError("HipAdamW: a state saved with amsgrad=True cannot be continued (not implemented)")
        held = [g["lr"] for g in self.param_groups]
        super().load_state_dict(state_dict)
        for g, lr0 in zip(self.param_groups, held):
            g.update(capturable=True, amsgrad=False, foreach=None, fused=None, differentiable=False,
                     decoupled_weight_decay=self.decoupled)
            if torch.is_tensor(lr0):
                with torch.no_grad():
                    lr0.fill_(float(g["lr"]))
                g["lr"] = lr0
            elif torch.is_tensor(g["lr"]):
                g["lr"] = float(g["lr"])
            for p in g["params"]:
                if p not in self.state:
                    continue
                s = self.state[p]
                if "step" in s:
                    step = s["step"]
                    if torch.is_tensor(step):  # (copy: torch hands a saved step tensor through as it is)
                        step = step.detach().to(device=p.device, dtype=torch.float32, copy=True).reshape(())
                    else:
                        step = torch.tensor(float(step), dtype=torch.float32, device=p.device)
                    s["step"] = step
                for k in ("exp_avg", "exp_avg_sq"):
                    if torch.is_tensor(s.get(k)):
                        s[k] = s[k].detach().to(device=p.device, dtype=torch.float32).contiguous()
        self._tables = {}

    @staticmethod
    def _check_state(p, s) -> None:
        """the kernel dereferences these on the device: anything else (a state assigned by hand, a step counter on the
        host) is refused before a launch"""
        for k in ("step", "exp_avg", "exp_avg_sq"):
            t = s.get(k)
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.device != p.device:
                raise TypeError(f"HipAdamW: state['{k}'] must be an f32 tensor on the parameter's device ({p.device}), got "
                                f"{f'{t.dtype} on {t.device}' if torch.is_tensor(t) else type(t).__name__}; "
                                "load_state_dict() converts a torch state")
        if s["step"].numel() != 1 or s["exp_avg"].numel() != p.numel() or s["exp_avg_sq"].numel() != p.numel() or \
                not s["exp_avg"].is_contiguous() or not s["exp_avg_sq"].is_contiguous():
            raise ValueError("HipAdamW: state['step'] holds one element, the moments are contiguous and of the parameter's size")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _l.load()
        work = []
        for gi, group in enumerate(self.param_groups):  # every check of every group before the first launch
            params = [p for p in group["params"] if p.grad is not None]
            if not params:
                continue
            for p in params:
                if not p.is_cuda or p.dtype != torch.float32 or p.grad.dtype != torch.float32:
                    raise TypeError("HipAdamW: f32 parameters and gradients on the GPU (there is no CPU path)")
                if not p.is_contiguous() or not p.grad.is_contiguous():
                    raise ValueError("HipAdamW: parameters and gradients must be contiguous")
                s = self.state[p]
                if not s:
                    s["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
                    s["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    s["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            # (the table is rebuilt, and the state behind it checked, whenever an address differs from the last step's)
            work.append((group, params, self._arrays(gi, params)))
        for group, params, (_, cols, numel) in work:
            torch._foreach_add_([self.state[p]["step"] for p in params], 1.0)  # one launch; the kernel reads the new count
            lr = group["lr"]
            if not torch.is_tensor(lr):  # eager use with a host-side learning rate: a fill kernel, no host-to-device copy
                lr = torch.full((), float(lr), dtype=torch.float32, device=params[0].device)
            elif lr.device != params[0].device or lr.dtype != torch.float32:
                lr = lr.to(params[0].device, torch.float32)
            b1, b2 = group["betas"]
            _l.check(lib.ffa_adamw_multi(len(params), *cols, numel, lr.data_ptr(), float(b1), float(b2), float(group["eps"]),
                                         float(group["weight_decay"]), 1 if self.decoupled else 0,
                                         1 if group["maximize"] else 0, torch.cuda.current_stream().cuda_stream),
                      "adamw_multi")
        return loss


class HipAdam(HipAdamW):
    decoupled = False

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, **kw):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **kw)
