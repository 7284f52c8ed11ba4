"""Per-step learning-rate schedules: warmup, then step / constant / linear / cosine.

The reference sets ``lr0 * 0.1 ** (epoch // 10)`` once per epoch on the host
(``multi_proc_single_gpu.py:257-261``; ``optim.flat.adjust_learning_rate``).  A schedule that
moves every optimizer step cannot be a host loop here: a ``train_steps`` call replays
multi-step hipGraphs with no host involvement.  So the whole run's rates are computed once, on
the host, in Python floats (fp64), into one table with an entry per optimizer step; the CPU
path reads it per step, and on the GPU it is uploaded once and the launch that advances the
optimizer-step counter copies the step's entry into the optimizer's learning-rate word
(``csrc/kernels.h`` LrSched; ``docs/kernels.md`` "Device-resident learning-rate schedule").
Both paths consume the same table, so neither evaluates ``cos`` on its own.

With ``spe`` this rank's steps per epoch (ragged tail step included), ``T = epochs * spe``,
``g = epoch * spe + i`` the 0-based global step (counted from epoch 0 whatever --start-epoch /
--resume say), ``W`` warmup steps, ``lr0 = --lr``, ``m = --lr-min`` and
``p(g) = max(0, g - W) / max(1, T - 1 - W)``::

    base(g):  step      lr0 * 0.1 ** ((g // spe) // 10)
              constant  lr0
              linear    lr0 * (m + (1 - m) * (1 - p))
              cosine    lr0 * (m + (1 - m) * 0.5 * (1 + cos(pi * p)))
    lr(g)  =  base(g) * ((g + 1) / W)   if g < W   else base(g)

``lr(g)`` depends on (flags, epoch, i) only: runs are reproducible, ``--resume`` with the flags
given again continues as an uninterrupted run would, and two world sizes with the same ``spe``
see the same schedule.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

KINDS = ("step", "constant", "linear", "cosine")


@dataclass(frozen=True)
class ScheduleSpec:
    """A run's schedule: ``kind`` (KINDS), the initial rate ``lr0``, ``warmup`` steps, the
    final rate ``lr_min`` as a fraction of lr0 (linear / cosine), and the run's geometry,
    ``epochs`` epochs of ``spe`` optimizer steps."""
    kind: str
    lr0: float
    epochs: int
    spe: int
    warmup: int = 0
    lr_min: float = 0.0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"--lr-schedule: {self.kind!r} is not one of {KINDS}")
        if int(self.epochs) < 1 or int(self.spe) < 1:
            raise ValueError(f"a schedule needs at least one step: {self.epochs} epochs of "
                             f"{self.spe} steps")
        object.__setattr__(self, "epochs", int(self.epochs))
        object.__setattr__(self, "spe", int(self.spe))
        object.__setattr__(self, "warmup", int(self.warmup))
        object.__setattr__(self, "lr0", float(self.lr0))
        object.__setattr__(self, "lr_min", float(self.lr_min))
        if not 0 <= self.warmup < self.total:
            raise ValueError(f"argument --lr-warmup: {self.warmup} warmup steps do not fit a run "
                             f"of {self.total} optimizer steps ({self.epochs} epochs of "
                             f"{self.spe}): give 0..{self.total - 1}")
        if not 0.0 <= self.lr_min <= 1.0:                        # (also rejects nan)
            raise ValueError(f"argument --lr-min: {self.lr_min!r} is outside 0..1")
        if self.lr_min != 0.0 and self.kind in ("step", "constant"):
            raise ValueError(f"argument --lr-min: --lr-schedule {self.kind} has no final rate "
                             "(use linear or cosine)")

    @property
    def total(self) -> int:
        """T: the run's optimizer steps."""
        return self.epochs * self.spe

    def base(self, g: int) -> float:
        lr0, m, W, T = self.lr0, self.lr_min, self.warmup, self.total
        if self.kind == "step":
            return lr0 * 0.1 ** ((g // self.spe) // 10)
        if self.kind == "constant":
            return lr0
        p = max(0, g - W) / max(1, T - 1 - W)
        if self.kind == "linear":
            return lr0 * (m + (1 - m) * (1 - p))
        return lr0 * (m + (1 - m) * 0.5 * (1 + math.cos(math.pi * p)))

    def lr(self, g: int) -> float:
        b = self.base(g)
        # (g + 1) / W first: the last warmup step's factor is exactly 1
        return b * ((g + 1) / self.warmup) if g < self.warmup else b

    def table(self) -> np.ndarray:
        """fp64 [T]: the rate of every optimizer step of the run (computed once, then cached;
        read-only)."""
        t = self.__dict__.get("_table")
        if t is None:
            t = np.array([self.lr(g) for g in range(self.total)], dtype=np.float64)
            t.setflags(write=False)
            object.__setattr__(self, "_table", t)
        return t


def spec_from_args(args, spe: int):
    """The ScheduleSpec of a parsed command line for a rank of ``spe`` steps per epoch.  None
    with ``--lr-schedule step`` and ``--lr-warmup 0`` (the defaults): the host's per-epoch
    ``adjust_learning_rate`` then runs as ever, and there is no table.  A flag that does not
    fit the run (warmup >= the run's steps) raises ValueError("argument --lr-...")."""
    kind = getattr(args, "lr_schedule", "step")
    warmup = getattr(args, "lr_warmup", 0)
    lr_min = getattr(args, "lr_min", 0.0)
    if kind == "step" and warmup == 0 and lr_min == 0.0:
        return None
    return ScheduleSpec(kind, args.lr, args.epochs, spe, warmup, lr_min)
