"""Mixup (Zhang et al. 2018): every training sample is blended with a partner sample, and its
target with the partner's label; the integer spec.

The draw and the blend are integer-only, so the GPU kernels (``gather_epoch_mixup`` in
``csrc/kernels/augment.hip``, ``cnn_head_mixup`` in ``csrc/kernels/cnn_head_mix.hip``), this
NumPy implementation (the CPU path's, and the kernels' oracle) and the tests agree bit for bit.
A sample's draw depends only on ``(seed, epoch, dataset index)`` -- not on the rank, the world
size, the batch or the sample's position in the epoch's order -- so world-size invariance holds
and ``--resume`` reproduces an uninterrupted run.

For the sample with dataset index ``i`` in epoch ``e``, with ``N`` the size of the training set::

    (r0, r1, _, _) = Philox4x32-10(counter (i, e, 3, 0), key (seed & 0xffffffff, seed >> 32))
    j = (r0 * N) >> 32             the partner: any training sample, j == i allowed
    q = QT[r1 >> 22]               QT int32 [1024], 128..256; lambda = q / 256
    m = (q a + (256 - q) b + 128) >> 8       per byte, a from image i, b from image j

Counter word 2 is 3 where the augmentation's draws have 0, dropout's 1 and the elastic control
points' 2: the streams never meet.  ``QT[k] = rint(256 max(x, 1 - x))`` with ``x`` the
Beta(A, A) quantile at ``(k + 0.5) / 1024``, computed once, on the host, in float64
(:func:`beta_quantile`); folding to lambda >= 1/2 keeps ``i`` the primary sample, so a row's
``correct`` keeps its meaning.  q = 256 leaves the image as it is: ``(256 a + 128) >> 8 = a``.

The blend replaces each source byte of sample ``i``'s geometric transform
(``data/augment.py``), which keeps ``i``'s parameters: mixing the uint8 images first and
transforming the result is the same thing.  The target is
``lambda t(y_i) + (1 - lambda) t(y_j)`` with ``t`` the (label-smoothed) one-hot, the row loss
``lambda loss(y_i) + (1 - lambda) loss(y_j)``.  Evaluation and prediction are never mixed.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from .augment import philox4x32_10

MAX_ALPHA = 10.0
LEVELS = 1024
STREAM = 3               # counter word 2 of the mixup draws
_MASK32 = 0xFFFFFFFF


def _betacf(a: float, b: float, x: np.ndarray) -> np.ndarray:
    """The continued fraction of the incomplete beta function (modified Lentz), float64 [n];
    converges quickly for x < (a + 1) / (a + b + 2)."""
    tiny = 1e-300
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c = np.ones_like(x)
    d = 1.0 - qab * x / qap
    d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
    h = d.copy()
    for m in range(1, 400):
        m2 = 2 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)),
                   -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / np.where(np.abs(d) < tiny, tiny, d)
            c = 1.0 + aa / c
            c = np.where(np.abs(c) < tiny, tiny, c)
            h = h * d * c
        if np.all(np.abs(d * c - 1.0) < 1e-16):
            break
    return h


def beta_cdf(a: float, x) -> np.ndarray:
    """The regularised incomplete beta function I_x(a, a) for x in [0, 1/2], float64."""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros_like(x)
    pos = x > 0.0
    xp = x[pos]
    lnb = 2.0 * math.lgamma(a) - math.lgamma(2.0 * a)
    front = np.exp(a * np.log(xp) + a * np.log1p(-xp) - lnb) / a
    out[pos] = front * _betacf(a, a, xp)
    return out


def beta_quantile(a: float, p) -> np.ndarray:
    """The Beta(a, a) quantile at p in (0, 1/2]: x in [0, 1/2] with I_x(a, a) = p, by bisection
    in float64 (the CDF is monotone, so this needs no derivative and no starting guess)."""
    p = np.asarray(p, dtype=np.float64)
    if np.any(p <= 0.0) or np.any(p > 0.5):
        raise ValueError("beta_quantile takes p in (0, 1/2] (the density is symmetric)")
    lo, hi = np.zeros_like(p), np.full_like(p, 0.5)
    for _ in range(1100):            # (a small `a` puts the first quantiles near 1e-15)
        mid = 0.5 * (lo + hi)
        if np.all((mid == lo) | (mid == hi)):        # every bracket is down to neighbours
            break
        below = beta_cdf(a, mid) < p
        lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
    return 0.5 * (lo + hi)


@lru_cache(maxsize=16)
def quantile_table(alpha: float) -> np.ndarray:
    """QT, int32 [1024], read-only: rint(256 max(x, 1 - x)), x the Beta(alpha, alpha) quantile
    at (k + 0.5) / 1024.  The lower half is computed (x <= 1/2) and mirrored.  About a second of
    host time, once per alpha."""
    k = np.arange(LEVELS // 2, dtype=np.float64)
    x = beta_quantile(float(alpha), (k + 0.5) / LEVELS)
    half = np.rint(256.0 * (1.0 - x)).astype(np.int32)
    qt = np.concatenate([half, half[::-1]])
    qt.setflags(write=False)
    return qt


@dataclass(frozen=True)
class MixupSpec:
    """``alpha`` (0..10; 0 = off): lambda ~ Beta(alpha, alpha), folded to >= 1/2, and the 64-bit
    ``seed`` of the Philox key."""
    alpha: float = 0.0
    seed: int = 0

    def __post_init__(self):
        if not 0.0 <= self.alpha <= MAX_ALPHA:                   # (also rejects nan)
            raise ValueError(f"mixup alpha must be in 0..{MAX_ALPHA}, got {self.alpha!r}")
        object.__setattr__(self, "alpha", float(self.alpha))
        object.__setattr__(self, "seed", int(self.seed) & 0xFFFFFFFFFFFFFFFF)

    @property
    def enabled(self) -> bool:
        return self.alpha > 0.0

    @property
    def key(self):
        return self.seed & _MASK32, self.seed >> 32

    def table(self) -> np.ndarray:
        """QT of this alpha."""
        return quantile_table(self.alpha)


def _indices(dataset_index) -> np.ndarray:
    return np.asarray(dataset_index.numpy() if isinstance(dataset_index, torch.Tensor)
                      else dataset_index, dtype=np.int64).reshape(-1)


def draw(dataset_index, epoch: int, spec: MixupSpec, n_train: int, table=None):
    """The per-sample draws (j, q), int64 [n] each: the partner's dataset index in 0..n_train-1
    and the blend weight in 128..256.  ``table``: ``spec.table()``, or any int32 [1024]."""
    idx = _indices(dataset_index)
    if not 1 <= int(n_train) <= _MASK32:
        raise ValueError(f"the training set's size must be in 1..2^32-1, got {n_train}")
    qt = np.asarray(spec.table() if table is None else table, dtype=np.int64)
    ctr = np.zeros((idx.shape[0], 4), dtype=np.uint64)
    ctr[:, 0] = idx.astype(np.uint64) & _MASK32
    ctr[:, 1] = int(epoch) & _MASK32
    ctr[:, 2] = STREAM
    r = philox4x32_10(ctr, np.array(spec.key, dtype=np.uint64)).astype(np.uint64)
    j = (r[:, 0] * np.uint64(n_train)) >> np.uint64(32)         # < 2^64: exact in uint64
    return j.astype(np.int64), qt[(r[:, 1] >> np.uint64(22)).astype(np.int64)]


def blend(a_u8, b_u8, q) -> np.ndarray:
    """uint8: (q a + (256 - q) b + 128) >> 8, ``q`` (128..256) broadcast from the left ([n] for
    [n, 784] images)."""
    a = np.asarray(a_u8).astype(np.int64)
    b = np.asarray(b_u8).astype(np.int64)
    qq = np.asarray(q, dtype=np.int64)
    qq = qq.reshape(qq.shape + (1,) * (a.ndim - qq.ndim))
    return ((qq * a + (256 - qq) * b + 128) >> 8).astype(np.uint8)


def mix_batch(train_images, dataset_index, epoch: int, spec: MixupSpec, table=None):
    """(mixed uint8 [n, 784], j int64 [n], q int64 [n]): the samples ``dataset_index`` of the
    training set ``train_images`` (uint8 [N, 784], NumPy or host torch), each blended with its
    partner of epoch ``epoch``; the images come back as the kind that went in."""
    src = train_images.numpy() if isinstance(train_images, torch.Tensor) else \
        np.asarray(train_images)
    if src.dtype != np.uint8 or src.ndim != 2 or src.shape[1] != 784:
        raise ValueError(f"images must be uint8 [N, 784], got {src.dtype} {src.shape}")
    idx = _indices(dataset_index)
    j, q = draw(idx, epoch, spec, src.shape[0], table)
    out = blend(src[idx], src[j], q)
    return (torch.from_numpy(out) if isinstance(train_images, torch.Tensor) else out), j, q


def spec_from_args(args):
    """The MixupSpec of a parsed command line (None when --mixup is absent or 0): --mixup-seed
    defaults to --seed when that is given, else 0."""
    alpha = getattr(args, "mixup", 0.0)
    seed = getattr(args, "mixup_seed", None)
    if seed is None:
        seed = args.seed if getattr(args, "seed", None) is not None else 0
    spec = MixupSpec(alpha, seed)
    return spec if spec.enabled else None
