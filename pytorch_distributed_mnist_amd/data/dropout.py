"""Dropout on the CNN's 128 hidden units (in front of fc2): the integer mask spec.

The mask is integer-only, so the GPU head (``csrc/kernels/cnn_head_drop.hip``), this NumPy
implementation (the CPU path's, and the kernel's oracle) and the tests agree bit for bit.  A
unit's draw depends only on ``(seed, epoch, dataset index, unit)`` -- not on the rank, the
world size, the batch or the sample's position in the epoch's order -- so world-size invariance
holds and ``--resume`` reproduces an uninterrupted run.

For the sample with dataset index ``i``, epoch ``e`` and hidden unit ``n`` (0..127)::

    (r0, r1, r2, r3) = Philox4x32-10(counter (i, e, 1, n >> 3), key (seed & 0xffffffff, seed >> 32))
    r = r[(n >> 1) & 3]
    u = r & 0xffff for even n,  r >> 16 for odd n
    keep  <=>  u >= T,          T = round(p * 65536)
    kept units are multiplied by scale = fp32(65536 / (65536 - T)), dropped units by 0

Counter word 2 is 1 where the augmentation's draws (``data/augment.py``) have 0: the two
streams never meet.  ``p`` is accepted in [0, 0.9]; p = 0 (T = 0) keeps everything at scale 1,
and is off.  Evaluation and prediction never drop.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .augment import philox4x32_10

HIDDEN = 128
MAX_P = 0.9
INDEX_BITS = 27          # the GPU step carries the dataset index in the label word: index << 4
_MASK32 = 0xFFFFFFFF


@dataclass(frozen=True)
class DropoutSpec:
    """Drop probability ``p`` (0..0.9) of each hidden unit and the 64-bit ``seed`` of the
    Philox key."""
    p: float = 0.0
    seed: int = 0

    def __post_init__(self):
        if not 0.0 <= self.p <= MAX_P:                           # (also rejects nan)
            raise ValueError(f"dropout p must be in 0..{MAX_P}, got {self.p!r}")
        object.__setattr__(self, "p", float(self.p))
        object.__setattr__(self, "seed", int(self.seed) & 0xFFFFFFFFFFFFFFFF)

    @property
    def T(self) -> int:
        """The 16-bit threshold: a unit is kept iff its draw is >= T."""
        return int(round(self.p * 65536))

    @property
    def scale(self) -> float:
        """The kept units' multiplier, rounded to fp32 (what the kernel multiplies by)."""
        return float(np.float32(65536.0 / (65536.0 - self.T)))

    @property
    def enabled(self) -> bool:
        return self.T > 0

    @property
    def key(self):
        return self.seed & _MASK32, self.seed >> 32


def keep_mask(dataset_index, epoch: int, spec: DropoutSpec, stream: int = 1) -> np.ndarray:
    """uint8 [N, 128]: 1 where hidden unit n of sample ``dataset_index[k]`` is kept in epoch
    ``epoch``.  ``stream`` is counter word 2 (1: the dropout stream; tests pass the
    augmentation's 0 to show the streams differ)."""
    idx = np.asarray(dataset_index.numpy() if isinstance(dataset_index, torch.Tensor)
                     else dataset_index, dtype=np.int64).reshape(-1)
    blocks = HIDDEN // 8
    ctr = np.zeros((idx.shape[0], blocks, 4), dtype=np.uint64)
    ctr[:, :, 0] = (idx.astype(np.uint64) & _MASK32)[:, None]
    ctr[:, :, 1] = int(epoch) & _MASK32
    ctr[:, :, 2] = int(stream) & _MASK32
    ctr[:, :, 3] = np.arange(blocks, dtype=np.uint64)[None, :]
    r = philox4x32_10(ctr, np.array(spec.key, dtype=np.uint64))          # [N, 16, 4] uint32
    # unit n = 8 q + 2 w + b: block q, word w, half b (0: low 16 bits)
    u = np.stack([r & np.uint32(0xFFFF), r >> np.uint32(16)], axis=-1)   # [N, 16, 4, 2]
    return (u.reshape(idx.shape[0], HIDDEN) >= np.uint32(spec.T)).astype(np.uint8)


def multiplier(dataset_index, epoch: int, spec: DropoutSpec) -> torch.Tensor:
    """fp32 [N, 128]: ``spec.scale`` where the unit is kept, 0 where it is dropped."""
    keep = torch.from_numpy(keep_mask(dataset_index, epoch, spec))
    return keep.to(torch.float32) * spec.scale


def tag_labels(labels: torch.Tensor) -> torch.Tensor:
    """int32 [N]: ``label | (dataset index << 4)``, the label word that carries a training row's
    dataset index through the epoch gather and the forward kernels to the dropout head."""
    n = labels.numel()
    if n > 1 << INDEX_BITS:
        raise ValueError(f"dropout tags the label word with the dataset index, which must be "
                         f"< 2^{INDEX_BITS}; the training set has {n} samples")
    lab = labels.to(torch.int64).reshape(-1)
    if n and (int(lab.min()) < 0 or int(lab.max()) > 15):
        raise ValueError("labels must fit the label word's low 4 bits")
    return (lab | (torch.arange(n, dtype=torch.int64) << 4)).to(torch.int32)


def spec_from_args(args):
    """The DropoutSpec of a parsed command line (None when --dropout is absent or 0):
    --dropout-seed defaults to --seed when that is given, else 0."""
    p = getattr(args, "dropout", 0.0)
    seed = getattr(args, "dropout_seed", None)
    if seed is None:
        seed = args.seed if getattr(args, "seed", None) is not None else 0
    spec = DropoutSpec(p, seed)
    return spec if spec.enabled else None
