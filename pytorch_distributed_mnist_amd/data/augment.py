"""Train-time augmentation: a small random shift, rotation and zoom per sample and epoch, and
an elastic distortion (Simard et al. 2003).

The transform is integer-only, so the GPU kernel (``csrc/kernels/augment.hip``), this NumPy
implementation (the CPU path's, and the kernel's oracle) and the tests agree bit for bit.
A sample's transform depends only on ``(seed, epoch, dataset index)`` -- not on the rank, the
world size or the sample's position in the epoch's order -- so world-size invariance holds
and ``--resume`` reproduces an uninterrupted run.

Random numbers: Philox4x32-10, counter ``(dataset_index, epoch, 0, 0)``, key
``(seed & 0xffffffff, seed >> 32)``, output words ``r0..r3``.  With S the shift range in
pixels, R the rotation range in degrees and Z the zoom range (a fraction)::

    k = r0 >> 22 (angle level, 0..1023)      j = r1 >> 26 (zoom level, 0..63)
    dx = r2 % (2S+1) - S                     dy = r3 % (2S+1) - S

Tables (float64, ``np.rint`` to int32)::

    theta_k = radians(R (2k - 1023) / 1023)  cosq[k] = rint(cos theta_k 2^14), sinq likewise
    z_j = 1 + Z (2j - 63) / 63               invz[j] = rint(2^14 / z_j)

Inverse map (every ``>>`` is an arithmetic shift, i.e. floor)::

    A = (cosq[k] invz[j] + 8192) >> 14       B = (sinq[k] invz[j] + 8192) >> 14
    output pixel (x, y) in 0..27:  u = 2x - 27, v = 2y - 27
    SX = (( A u + B v + 64) >> 7) + 3456 - 256 dx          source x in 1/256 px
    SY = ((-B u + A v + 64) >> 7) + 3456 - 256 dy
    x0 = SX >> 8, fx = SX & 255, y0 = SY >> 8, fy = SY & 255
    out = ((256-fx)(256-fy) p(x0,y0) + fx (256-fy) p(x0+1,y0)
           + (256-fx) fy p(x0,y0+1) + fx fy p(x0+1,y0+1) + 32768) >> 16

with ``p`` zero outside the 28 x 28 image.  Everything fits int32.  S = R = Z = 0 is exactly
the identity.  Labels are never changed; evaluation and prediction are never augmented.

Elastic distortion (``elastic`` = A pixels, 0..3; E = rint(256 A), in 1/256 px) adds a smooth
per-sample displacement (ex, ey) to SX and SY.  A 6 x 6 grid of control displacements at a
spacing of 8 pixels, control point q = 6 cy + cx drawn with counter
``(dataset_index, epoch, 2, q)`` (word 2: 0 is the draw above, 1 is dropout's)::

    gx[q] = (((r0 >> 16) (2E+1)) >> 16) - E      gy[q] likewise from r1: uniform in [-E, E]

and a uniform quadratic B-spline over the 3 x 3 control points around the output pixel, exact
in integers because a cell is 16 half-pixels::

    hx = 2x + 1, cx0 = hx >> 4 (0..3), f = hx & 15;  hy, cy0, g likewise from y
    wx = [(16-f)^2, 256 + 32f - 2f^2, f^2]       (sums to 512)      wy the same in g
    ex = (sum_{b,a in 0..2} wy[b] wx[a] gx[6 (cy0+b) + cx0+a] + 2^17) >> 18;  ey with gy
    SX += ex, SY += ey

The sums are at most 2^18 * 768; |ex| <= E; neighbouring pixels differ by at most E/4 + 1, so
with A <= 3 the map never folds (256 + the difference >= 63).  E = 0 gives ex = ey = 0.  The
grid spacing is fixed: a second one would need more control points than a wave has lanes.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

MAX_SHIFT = 8
MAX_ROTATE = 45.0
MAX_ZOOM = 0.5
MAX_ELASTIC = 3.0
ELASTIC_GRID = 6                  # control points per axis, at a spacing of 8 pixels
ANGLE_LEVELS = 1024
ZOOM_LEVELS = 64

_M0, _M1 = 0xD2511F53, 0xCD9E8D57
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


@dataclass(frozen=True)
class AugmentSpec:
    """Ranges of the per-sample transform: ``shift`` pixels (0..8), ``rotate`` degrees
    (0..45), ``zoom`` fraction (0..0.5), the 64-bit ``seed`` of the Philox key, and
    ``elastic`` pixels (0..3), the range of the elastic field's control displacements (last,
    behind ``seed``: the first four are given positionally)."""
    shift: int = 0
    rotate: float = 0.0
    zoom: float = 0.0
    seed: int = 0
    elastic: float = 0.0

    def __post_init__(self):
        if int(self.shift) != self.shift or not 0 <= self.shift <= MAX_SHIFT:
            raise ValueError(f"shift must be an integer in 0..{MAX_SHIFT}, got {self.shift!r}")
        if not 0.0 <= self.rotate <= MAX_ROTATE:
            raise ValueError(f"rotate must be in 0..{MAX_ROTATE} degrees, got {self.rotate!r}")
        if not 0.0 <= self.zoom <= MAX_ZOOM:
            raise ValueError(f"zoom must be in 0..{MAX_ZOOM}, got {self.zoom!r}")
        if not 0.0 <= self.elastic <= MAX_ELASTIC:
            raise ValueError(f"elastic must be in 0..{MAX_ELASTIC} pixels, got {self.elastic!r}")
        object.__setattr__(self, "shift", int(self.shift))
        object.__setattr__(self, "rotate", float(self.rotate))
        object.__setattr__(self, "zoom", float(self.zoom))
        object.__setattr__(self, "seed", int(self.seed) & 0xFFFFFFFFFFFFFFFF)
        object.__setattr__(self, "elastic", float(self.elastic))

    @property
    def enabled(self) -> bool:
        return self.shift > 0 or self.rotate > 0.0 or self.zoom > 0.0 or self.elastic > 0.0

    @property
    def elastic_q(self) -> int:
        """E: the elastic range in 1/256 px, 0..768."""
        return int(np.rint(256.0 * self.elastic))

    @property
    def key(self):
        return self.seed & _MASK32, self.seed >> 32

    def tables(self):
        """(cosq int32 [1024], sinq int32 [1024], invz int32 [64]): the Q14 tables."""
        k = np.arange(ANGLE_LEVELS, dtype=np.float64)
        theta = np.radians(self.rotate * (2.0 * k - (ANGLE_LEVELS - 1)) / (ANGLE_LEVELS - 1))
        j = np.arange(ZOOM_LEVELS, dtype=np.float64)
        z = 1.0 + self.zoom * (2.0 * j - (ZOOM_LEVELS - 1)) / (ZOOM_LEVELS - 1)
        q = float(1 << 14)
        return (np.rint(np.cos(theta) * q).astype(np.int32),
                np.rint(np.sin(theta) * q).astype(np.int32),
                np.rint(q / z).astype(np.int32))


def philox4x32_10(counter, key):
    """Philox4x32-10, vectorised: ``counter`` [..., 4] and ``key`` [..., 2] (broadcast against
    each other) of 32-bit words -> uint32 [..., 4]."""
    c = np.asarray(counter, dtype=np.uint64) & _MASK32
    k = np.asarray(key, dtype=np.uint64) & _MASK32
    shape = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], shape).copy() for i in range(2))
    m0, m1 = np.uint64(_M0), np.uint64(_M1)
    mask, s32 = np.uint64(_MASK32), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                   # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(_W0)) & mask
        k1 = (k1 + np.uint64(_W1)) & mask
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def draw(dataset_index, epoch: int, spec: AugmentSpec):
    """The per-sample draws (k, j, dx, dy), int64 [N] each."""
    idx = np.asarray(dataset_index, dtype=np.int64).reshape(-1)
    ctr = np.zeros((idx.shape[0], 4), dtype=np.uint64)
    ctr[:, 0] = idx.astype(np.uint64) & _MASK32
    ctr[:, 1] = int(epoch) & _MASK32
    r = philox4x32_10(ctr, np.array(spec.key, dtype=np.uint64)).astype(np.int64)
    span = 2 * spec.shift + 1
    return r[:, 0] >> 22, r[:, 1] >> 26, r[:, 2] % span - spec.shift, r[:, 3] % span - spec.shift


def elastic_controls(dataset_index, epoch: int, spec: AugmentSpec):
    """The elastic field's control displacements (gx, gy), int64 [N, 6, 6] each (indexed
    [sample, cy, cx]), in 1/256 px."""
    idx = np.asarray(dataset_index, dtype=np.int64).reshape(-1)
    q = ELASTIC_GRID * ELASTIC_GRID
    ctr = np.zeros((idx.shape[0], q, 4), dtype=np.uint64)
    ctr[:, :, 0] = (idx.astype(np.uint64) & _MASK32)[:, None]
    ctr[:, :, 1] = int(epoch) & _MASK32
    ctr[:, :, 2] = 2
    ctr[:, :, 3] = np.arange(q, dtype=np.uint64)[None, :]
    r = philox4x32_10(ctr, np.array(spec.key, dtype=np.uint64)).astype(np.int64)
    e = spec.elastic_q
    g = (((r[..., :2] >> 16) * (2 * e + 1)) >> 16) - e
    shape = (idx.shape[0], ELASTIC_GRID, ELASTIC_GRID)
    return g[..., 0].reshape(shape), g[..., 1].reshape(shape)


def _spline_weights(h):
    """Quadratic B-spline weights of the half-pixel coordinate ``h`` = 2x + 1 (int64 [28]):
    the first cell index [28] and the three weights [3, 28], which sum to 512."""
    f = h & 15
    return h >> 4, np.stack([(16 - f) ** 2, 256 + 32 * f - 2 * f * f, f * f])


def elastic_field(dataset_index, epoch: int, spec: AugmentSpec):
    """The elastic displacements (ex, ey), int64 [N, 784] each, in 1/256 px."""
    gx, gy = elastic_controls(dataset_index, epoch, spec)
    c0, w = _spline_weights(2 * np.arange(28, dtype=np.int64) + 1)
    cols = c0[None, :] + np.arange(3)[:, None]                  # [3, 28] control index per tap

    def field(g):
        # along x, then along y: rows[n, cy, x], then out[n, y, x]; exact, so the order is free
        rows = (g[:, :, cols] * w[None, None]).sum(axis=2)
        out = (rows[:, cols, :] * w[None, :, :, None]).sum(axis=1)
        return ((out + (1 << 17)) >> 18).reshape(g.shape[0], 784)

    return field(gx), field(gy)


def _u8_rows(images):
    a = images.numpy() if isinstance(images, torch.Tensor) else np.asarray(images)
    if a.dtype != np.uint8 or a.ndim != 2 or a.shape[1] != 784:
        raise ValueError(f"images must be uint8 [N, 784], got {a.dtype} {a.shape}")
    return a


def augment_batch(images_u8, dataset_index, epoch: int, spec: AugmentSpec, tables=None):
    """The transform of ``images_u8`` (uint8 [N, 784], NumPy or host torch) whose rows are the
    samples ``dataset_index`` [N] of the data set, in epoch ``epoch``: uint8 [N, 784] of the
    same kind.  ``tables``: ``spec.tables()`` if the caller keeps them."""
    src = _u8_rows(images_u8)
    n = src.shape[0]
    idx = np.asarray(dataset_index.numpy() if isinstance(dataset_index, torch.Tensor)
                     else dataset_index, dtype=np.int64).reshape(-1)
    if idx.shape[0] != n:
        raise ValueError(f"{idx.shape[0]} dataset indices for {n} images")
    cosq, sinq, invz = tables if tables is not None else spec.tables()
    k, j, dx, dy = draw(idx, epoch, spec)
    iz = invz.astype(np.int64)[j]
    A = ((cosq.astype(np.int64)[k] * iz + 8192) >> 14)[:, None]
    B = ((sinq.astype(np.int64)[k] * iz + 8192) >> 14)[:, None]
    pix = np.arange(784, dtype=np.int64)
    u = (2 * (pix % 28) - 27)[None, :]
    v = (2 * (pix // 28) - 27)[None, :]
    sx = ((A * u + B * v + 64) >> 7) + 3456 - 256 * dx[:, None]
    sy = ((-B * u + A * v + 64) >> 7) + 3456 - 256 * dy[:, None]
    if spec.elastic > 0.0:
        ex, ey = elastic_field(idx, epoch, spec)
        sx, sy = sx + ex, sy + ey
    x0, fx, y0, fy = sx >> 8, sx & 255, sy >> 8, sy & 255
    rows = np.arange(n)[:, None]

    def p(xx, yy):
        ok = (xx >= 0) & (xx < 28) & (yy >= 0) & (yy < 28)
        return np.where(ok, src[rows, np.where(ok, yy * 28 + xx, 0)], 0).astype(np.int64)

    out = ((256 - fx) * (256 - fy) * p(x0, y0) + fx * (256 - fy) * p(x0 + 1, y0)
           + (256 - fx) * fy * p(x0, y0 + 1) + fx * fy * p(x0 + 1, y0 + 1) + 32768) >> 16
    out = out.astype(np.uint8)
    return torch.from_numpy(out) if isinstance(images_u8, torch.Tensor) else out


# Test-time augmentation (--tta V): view v = 1..V-1 of row r is augment_batch(images, [r],
# TTA_EPOCH + v, spec) -- bit 31 of the epoch word keeps the draws apart from every training
# epoch's (set_train_indices takes epochs below 2^31) -- and view 0 is the image itself.
TTA_EPOCH = 0x80000000
MAX_TTA = 32


def tta_view(images_u8, start: int, size: int, v: int, spec: AugmentSpec, tables=None):
    """View ``v`` (0..MAX_TTA-1) of the rows ``start .. start + size`` of ``images_u8`` (uint8
    [N, 784], NumPy or host torch): uint8 [size, 784] of the same kind.  A row's view depends on
    its position in ``images_u8`` only, not on the chunk it is asked for in."""
    if not 0 <= int(v) < MAX_TTA:
        raise ValueError(f"view {v} is outside 0..{MAX_TTA - 1}")
    rows = images_u8[start:start + size]
    if v == 0:
        return rows
    return augment_batch(rows, np.arange(start, start + rows.shape[0], dtype=np.int64),
                         TTA_EPOCH + int(v), spec, tables)


def check_tta(views, spec) -> int:
    """The view count of a test-time augmentation as an int in 1..MAX_TTA; more than one view
    needs an enabled ``spec`` (all views would be the same image otherwise).  ValueError."""
    if int(views) != views or not 1 <= int(views) <= MAX_TTA:
        raise ValueError(f"tta must be an integer in 1..{MAX_TTA}, got {views!r}")
    if int(views) > 1 and (spec is None or not spec.enabled):
        raise ValueError(f"tta = {views} needs an augmentation range (shift, rotate, zoom or "
                         "elastic): without one every view is the same image")
    return int(views)


def spec_from_args(args):
    """The AugmentSpec of a parsed command line (None when no --aug-* range was given):
    --aug-seed defaults to --seed when that is given, else 0."""
    shift = getattr(args, "aug_shift", 0)
    rotate = getattr(args, "aug_rotate", 0.0)
    zoom = getattr(args, "aug_zoom", 0.0)
    seed = getattr(args, "aug_seed", None)
    if seed is None:
        seed = args.seed if getattr(args, "seed", None) is not None else 0
    spec = AugmentSpec(shift, rotate, zoom, seed, getattr(args, "aug_elastic", 0.0))
    return spec if spec.enabled else None
