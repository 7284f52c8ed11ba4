"""Exponential moving average of the weights (``--ema-decay D``, ``--ema-warmup``).

The Polyak / EMA model of timm's ``ModelEmaV2``, Keras' ``ExponentialMovingAverage`` and
``torch.optim.swa_utils``: beside the training weights ``p`` the run keeps an averaged copy
``e`` in a second flat fp32 buffer in the arena's layout, advanced once after every optimizer
step, which evaluation, the ``model_best`` choice and the checkpoint's ``ema_state_dict`` use.
Training never reads it.

The ``k``-th update (k = 1, 2, ...; counted over the whole run, restored on ``--resume``)::

    d_k = D                                   without --ema-warmup
    d_k = min(D, (1 + k) / (10 + k))          with it (the early average follows the weights)
    w_k = float32(1 - d_k)                    evaluated in fp64, rounded to fp32 once
    e   = e + w_k * (p - e)                   three separately rounded fp32 operations

``ema_weight`` below is that definition on the host: the CPU path uses its value, the GPU
kernel (``csrc/kernels/ema.hip``) takes it as an argument without warmup and evaluates the
same fp64 expression from the device optimizer-step word with it, and the tests re-evaluate
it in NumPy.  On the GPU the update is the last launch of every step, inside the step graphs
(``runtime/gpu_step.py`` ``launch_ema``); on the CPU it follows ``optimizer.step()``.
"""
from __future__ import annotations

from collections import OrderedDict
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from ..runtime.arena import FlatArena


@dataclass(frozen=True)
class EmaSpec:
    """A run's average: the decay ``D`` in (0, 1) and whether the warmup is on."""
    decay: float
    warmup: bool = False

    def __post_init__(self):
        object.__setattr__(self, "decay", float(self.decay))
        object.__setattr__(self, "warmup", bool(self.warmup))
        if not 0.0 < self.decay < 1.0:                           # (also rejects nan)
            raise ValueError(f"argument --ema-decay: {self.decay!r} is outside 0 < D < 1")

    def weight(self, k: int) -> float:
        return ema_weight(self.decay, k, self.warmup)


def ema_weight(decay: float, k: int = 1, warmup: bool = False) -> float:
    """w_k of the module docstring as a Python float that holds a float32 value: the weight of
    the k-th update (k >= 1; without warmup k does not matter)."""
    d = float(decay)
    if warmup:
        if int(k) < 1:
            raise ValueError(f"EMA updates are counted from 1, got k = {k}")
        d = min(d, (1.0 + int(k)) / (10.0 + int(k)))
    return float(np.float32(1.0 - d))


def spec_from_args(args) -> Optional[EmaSpec]:
    """The EmaSpec of a parsed command line; None without --ema-decay (or with 0: off)."""
    decay = getattr(args, "ema_decay", 0.0)
    if not decay:
        return None
    return EmaSpec(decay, bool(getattr(args, "ema_warmup", False)))


class WeightEma:
    """The averaged weights of one program: ``arena`` (a FlatArena without gradients, so the
    name views and ``state_dict`` come for free) and ``updates``, the number of updates that
    went into it.  Every rank keeps its own; the replicas' weights are identical, so theirs
    are too, with no communication."""

    def __init__(self, spec: EmaSpec, arena: FlatArena):
        self.spec = spec
        self.arena = FlatArena(arena.spec, arena.device, grads=False)
        self.updates = 0
        self.reset(arena)

    @property
    def params(self) -> torch.Tensor:
        return self.arena.params

    @torch.no_grad()
    def reset(self, arena: FlatArena) -> None:
        """Start the average at the weights of ``arena`` (after the rank-0 broadcast, or a
        resume from a checkpoint without an average)."""
        self.arena.params.copy_(arena.params)
        self.updates = 0

    @torch.no_grad()
    def update_cpu(self, params: torch.Tensor) -> None:
        """One update from the whole weights ``params`` (CPU path, after optimizer.step())."""
        w = self.spec.weight(self.updates + 1)
        e = self.arena.params
        e.add_((params - e).mul_(w))
        self.updates += 1

    def state_dict(self) -> "OrderedDict[str, torch.Tensor]":
        return self.arena.state_dict(prefix="module.")

    def load_state_dict(self, sd, updates: int) -> None:
        self.arena.load_state_dict(sd)
        self.updates = int(updates)
        if self.updates < 0:
            raise ValueError(f"ema_updates must be >= 0, got {updates}")
