"""Derived copies of parameters -- packed MFMA conv operands, transposed dgrad operands, eval-mode BatchNorm folds,
bf16 GEMM operands, column blocks of fusion weights -- and the ONE rule that says when such a copy is stale.

Imports torch only: usable (and tested) without libflairhip.
"""
from __future__ import annotations

import torch
from torch.optim.optimizer import register_optimizer_step_post_hook as _register_step_hook

_STATE_EPOCH = 0


def state_epoch() -> int:
    return _STATE_EPOCH


def bump_state_epoch() -> None:
    """Parameters / buffers changed on the device without Python noticing (a hipGraph replay runs the optimizer and
    the BatchNorm running-statistics updates in place: no tensor ``_version`` moves).  Every stamp carries this epoch,
    so every cached operand is rebuilt on next use."""
    global _STATE_EPOCH
    _STATE_EPOCH += 1


def _after_optimizer_step(optimizer, args, kwargs) -> None:
    bump_state_epoch()


# torch's fused (single-kernel) Adam / AdamW / SGD update parameters WITHOUT moving their ``_version`` (checked on
# torch 2.10: fused=True leaves p._version unchanged, the foreach / single-tensor paths bump it), so a cache keyed on
# versions alone would keep feeding the convolutions the weights of the first step.  Every optimizer step in the
# process therefore advances the state epoch.
_register_step_hook(_after_optimizer_step)


def stamp(*tensors, bn=None, extra=()):
    """What a derived operand was built from; it is valid while a new stamp of the same sources compares equal.
    Per tensor the build reads (None allowed): version counter (in-place writes) and address (re-allocation,
    ``.to()``, a replaced parameter).  The state epoch: fused optimizers and graph replays, which move neither.
    ``bn``: a BatchNorm module whose affine parameters and running statistics the build folds in, with its statistics
    epoch (the training kernels rewrite the statistics through raw pointers even when no optimizer step follows).
    ``extra``: anything else the build depends on (compute dtype ...), compared verbatim."""
    stats = None
    if bn is not None:
        tensors += (bn.weight, bn.bias, bn.running_mean, bn.running_var)
        stats = getattr(bn, "_stats_epoch", 0)
    return ([None if t is None else (t._version, t.data_ptr()) for t in tensors], _STATE_EPOCH, stats, extra)


class Entry:
    """One cached operand with everything needed to take its stamp again later"""
    __slots__ = ("stamp", "value", "sources", "bn", "extra", "repack")

    def __init__(self, stamp, value, sources, bn, extra, repack):
        self.stamp, self.value = stamp, value
        self.sources, self.bn, self.extra, self.repack = sources, bn, extra, repack

    def current(self) -> bool:
        return self.stamp == stamp(*self.sources, bn=self.bn, extra=self.extra)

    def restamp(self) -> None:
        """declare ``value`` up to date with the sources as they are now (someone rewrote it in place from them)"""
        self.stamp = stamp(*self.sources, bn=self.bn, extra=self.extra)


class OperandCache:
    """key -> Entry.  The key says WHICH operand is wanted (layout request, dtype, column block ...), the stamp
    whether the stored one still matches its sources."""

    def __init__(self):
        self.entries = {}

    def get(self, key, *sources, build, bn=None, extra=(), repack=None):
        """The value cached under ``key`` if it was built from these sources as they are now, else ``build()``, stored.
        ``repack``: not None marks a value that is a function of sources[0] alone and can be rewritten in place from it
        (nn.PackPlan's batched re-pack, which receives ``repack`` as the description of how)."""
        now = stamp(*sources, bn=bn, extra=extra)
        e = self.entries.get(key)
        if e is None or e.stamp != now:
            e = self.entries[key] = Entry(now, build(), sources, bn, extra, repack)
        return e.value
