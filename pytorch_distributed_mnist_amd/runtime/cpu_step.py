"""CPU execution of one training / eval step (the gloo plumbing path and the oracle).

Semantics are the reference Trainer's (``multi_proc_single_gpu.py:77-116``):
normalise the gathered uint8 batch, forward, ``F.cross_entropy`` (mean), backward,
then optimizer step.  Parameters are taken from the flat arena in kernel
layout and exposed to autograd through the (permuting) torch-layout views, so
the gradients land in kernel layout directly in the gradient arena.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from ..data.mnist import normalize_reference
from ..models.reference import functional_forward


def _leaf_params(arena):
    leaves, torch_views = {}, {}
    for p in arena.spec.params:
        leaf = arena.param(p.name).detach().requires_grad_(True)
        leaves[p.name] = leaf
        torch_views[p.name] = p.to_torch(leaf)
    return leaves, torch_views


def train_step_cpu(model: str, arena, images_u8, labels, reducer, optimizer, metrics_buf,
                   dropout=None, dataset_index=None, epoch=None, lr=None, label_smoothing=0.0,
                   ema=None, mixup=None):
    """dropout (a data.dropout.DropoutSpec, CNN): the hidden units of the batch's samples
    `dataset_index` are masked by their (seed, epoch, sample, unit) draws.  lr: this step's
    scheduled learning rate (optim/schedule.py), set on the optimizer before its step.
    label_smoothing (E in 0..1): the criterion's targets are (1 - E) onehot + E / 10, and the
    loss added to the metrics is the smoothed one.  ema (an optim.ema.WeightEma): the averaged
    weights take in the step's updated weights, ema += w (p - ema), after the optimizer.
    mixup ((partner labels int64 [N], lambda fp32 [N]), data/mixup.py; `images_u8` are the mixed
    images): the criterion is the per-sample weighted one, mean of lambda loss(y) +
    (1 - lambda) loss(y2); correct still counts `labels`."""
    x = normalize_reference(images_u8)
    mult = None
    if dropout is not None:
        from ..data.dropout import multiplier
        mult = multiplier(dataset_index, epoch, dropout)
    with torch.enable_grad():
        leaves, views = _leaf_params(arena)
        logits = functional_forward(model, views, x, mult)
        if mixup is not None:
            y2, lam = mixup
            e = float(label_smoothing)
            loss = (lam * F.cross_entropy(logits, labels, reduction="none", label_smoothing=e) +
                    (1.0 - lam) * F.cross_entropy(logits, y2, reduction="none",
                                                  label_smoothing=e)).mean()
        elif label_smoothing > 0.0:
            loss = F.cross_entropy(logits, labels, label_smoothing=label_smoothing)
        else:
            loss = F.cross_entropy(logits, labels)
        names = [p.name for p in arena.spec.params]
        grads = torch.autograd.grad(loss, [leaves[n] for n in names])
    with torch.no_grad():
        for n, g in zip(names, grads):
            arena.grad(n).copy_(g)
        # buckets become ready in arena (backward) order; on CPU the all-reduces
        # are issued async and joined before the optimizer, like the GPU path.
        for b in range(reducer.num_buckets):
            reducer.bucket_ready(b)
        reducer.finalize()
        if lr is not None:
            optimizer.param_groups[0]["lr"] = lr
        sh = getattr(reducer, "shard", None)
        if sh is None:
            optimizer.step_cpu(grad_scale=reducer.grad_scale)
        else:
            # sharded fc1 update: this rank's rows only (the other rows and their optimizer
            # state are left as they are), then every rank's updated rows all-gathered
            _, start, count = sh
            ws, r = reducer.comm.world_size, reducer.comm.rank
            own = (start + r * count, start + (r + 1) * count)
            frozen = [(start, own[0]), (own[1], start + ws * count)]
            optimizer.step_cpu(grad_scale=reducer.grad_scale, frozen=frozen)
            reducer.gather(arena.params[start:start + ws * count])
        if ema is not None:
            ema.update_cpu(arena.params)
        bsz = images_u8.shape[0]
        correct = logits.argmax(dim=1).eq(labels).sum().item()
        metrics_buf[0] += loss.item() * bsz
        metrics_buf[1] += correct
        metrics_buf[2] += bsz


@torch.no_grad()
def predict_step_cpu(model: str, arena, images_u8, labels=None):
    """What the model says about every row (the oracle of the GPU prediction heads):
    (log_probs fp32 [N, 10], pred int64 [N], confusion int64 [10, 10] or None without labels;
    confusion[y][pred] counts the rows of class y predicted as pred)."""
    x = normalize_reference(images_u8)
    views = {p.name: p.to_torch(arena.param(p.name)) for p in arena.spec.params}
    return _prediction(functional_forward(model, views, x), labels)


def _prediction(logits, labels):
    """predict_step_cpu's triple from the logits."""
    log_probs = F.log_softmax(logits, dim=1)
    pred = logits.argmax(dim=1)
    confusion = None
    if labels is not None:
        ncls = logits.shape[1]
        confusion = torch.bincount(labels.to(torch.int64) * ncls + pred,
                                   minlength=ncls * ncls).view(ncls, ncls)
    return log_probs, pred, confusion


def check_quantize(model: str, quantize):
    """`quantize` as None, "int8", "mxfp4" or "sparse24"; anything else, or a model other than the
    two MLPs (whose fc1 takes the raw image bytes: csrc/kernels/mlp_i8.hip, mlp_mx4.hip,
    mlp_sp24.hip), is a ValueError."""
    if quantize is None:
        return None
    if quantize in ("mxfp4", "sparse24"):
        if model not in ("mlp", "mlp2"):
            raise ValueError(f"no {quantize} kernel for quantize='{quantize}' on the {model} model: "
                             f"quantize=\"{quantize}\" is built for --arch mlp and mlp2 only")
        return quantize
    if quantize != "int8" or model not in ("mlp", "mlp2"):
        raise ValueError(f"no int8 kernel for quantize={quantize!r} on the {model} model: "
                         "quantize=\"int8\" is built for --arch mlp and mlp2 only")
    return quantize


# the normalisation x = alpha u8 - beta as the fc1 kernels fold it, and gamma = 128 alpha - beta
I8_ALPHA = np.float32(1.0 / (255.0 * 0.3081))
I8_GAMMA = np.float32(128.0 / (255.0 * 0.3081) - 0.1307 / 0.3081)


def quantize_fc1(arena) -> dict:
    """Per-row int8 quantisation of `arena`'s fc1 (docs/kernels.md "int8 evaluation"; the CPU twin
    and oracle of mlp_quant_w1, bit for bit: NumPy float32, every operation rounded on its own).
    Per hidden unit n: s1 = max_k |W1[n][k]| / 127 (1 for an all-zero row), q1 = clamp(rint(W1 /
    s1), -127, 127) with ties to even, r1 = sum_k q1, c1 = alpha s1, d1 = b1 + (s1 r1) gamma.
    {"q1": int8 [128, 784], "s1", "c1", "d1": float32 [128], "r1": int32 [128]}, NumPy."""
    w = arena.param("fc1.weight").detach().cpu().numpy().astype(np.float32).reshape(128, 784)
    b = arena.param("fc1.bias").detach().cpu().numpy().astype(np.float32)
    m = np.abs(w).max(axis=1)
    s1 = np.where(m == 0, np.float32(1), m / np.float32(127)).astype(np.float32)
    q1 = np.clip(np.rint(w / s1[:, None]), -127, 127).astype(np.int8)
    r1 = q1.sum(axis=1, dtype=np.int32)
    d1 = b + (s1 * r1.astype(np.float32)) * I8_GAMMA
    return {"q1": q1, "s1": s1, "r1": r1, "c1": I8_ALPHA * s1, "d1": d1.astype(np.float32)}


@torch.no_grad()
def predict_step_cpu_int8(model: str, arena, q: dict, images_u8, labels=None):
    """predict_step_cpu with fc1 quantised (`q`: quantize_fc1 of `arena`): pre = c1 I + d1 with
    I = sum_k q1 (u8 - 128) an exact integer product, then the reference forward's remaining
    layers in fp32."""
    acc = (images_u8.reshape(-1, 784).to(torch.int32) - 128) @ torch.from_numpy(q["q1"]).to(torch.int32).t()
    pre = torch.from_numpy(q["c1"]) * acc.to(torch.float32) + torch.from_numpy(q["d1"])
    return _prediction(_behind_fc1(model, arena, pre), labels)


def _behind_fc1(model: str, arena, pre):
    """The logits of an MLP from fc1's pre-activations: the reference forward's remaining layers."""
    views = {p.name: p.to_torch(arena.param(p.name)) for p in arena.spec.params}
    h = F.relu(pre)
    if model == "mlp2":
        h = F.relu(F.linear(h, views["fc2.weight"], views["fc2.bias"]))
        return F.linear(h, views["fc3.weight"], views["fc3.bias"])
    return F.linear(h, views["fc2.weight"], views["fc2.bias"])


MX4_BETA = np.float32(0.1307 / 0.3081)
E2M1_GRID = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float32)


def quantize_fc1_mxfp4(arena) -> dict:
    """OCP MXFP4 quantisation of `arena`'s fc1 (docs/kernels.md "MXFP4 evaluation"; the CPU twin
    and oracle of mlp_quant_mx4, bit for bit).  Each row, padded with zeros to 896 columns, is 28
    blocks of 32 consecutive k; a block with m = max |w| > 0 has e8 = clamp(floor(log2 m) - 2 +
    127, 0, 254), taken from m's exponent field, and X = 2^(e8 - 127); m = 0 has e8 = 127.  v = w
    / X (exact) goes to the nearest of 0, .5, 1, 1.5, 2, 3, 4, 6, ties to the code with mantissa
    bit 0, above 6 to 6; code = sign << 3 | magnitude code, no negative zero.  R = the block sums
    of the dequantised weights (exact) added in block order in float32, d1 = b1 - beta R in two
    roundings.  {"codes": uint8 [128, 448] (even k in the low nibble), "scales": uint8 [128, 28],
    "wq": float32 [128, 784] the dequantised weights, "d1": float32 [128]}, NumPy."""
    w = arena.param("fc1.weight").detach().cpu().numpy().astype(np.float32).reshape(128, 784)
    b = arena.param("fc1.bias").detach().cpu().numpy().astype(np.float32)
    blk = np.zeros((128, 896), np.float32)
    blk[:, :784] = w
    blk = blk.reshape(128, 28, 32)
    m = np.ascontiguousarray(np.abs(blk).max(axis=2))
    field = ((m.view(np.uint32) >> 23) & 0xff).astype(np.int32)
    e8 = np.where(m == 0, 127, np.maximum(field - 2, 0)).astype(np.int32)
    a = np.abs(np.ldexp(blk, (127 - e8)[:, :, None]))
    mag = ((a > 0.25).astype(np.uint8) + (a >= 0.75) + (a > 1.25) + (a >= 1.75) + (a > 2.5) +
           (a >= 3.5) + (a > 5)).astype(np.uint8)
    neg = (blk < 0) & (mag != 0)
    code = (mag | (neg.astype(np.uint8) << 3)).reshape(128, 896)
    wq = np.ldexp(np.where(neg, -E2M1_GRID[mag], E2M1_GRID[mag]), (e8 - 127)[:, :, None])
    wq = wq.astype(np.float32)
    sums = wq.sum(axis=2, dtype=np.float32)          # exact: 32 values of 2 bits on one scale
    r = sums[:, 0]
    for k in range(1, 25):
        r = r + sums[:, k]
    t = MX4_BETA * r
    return {"codes": code[:, 0::2] | (code[:, 1::2] << 4), "scales": e8.astype(np.uint8),
            "wq": np.ascontiguousarray(wq.reshape(128, 896)[:, :784]), "d1": (b - t).astype(np.float32)}


@torch.no_grad()
def predict_step_cpu_mxfp4(model: str, arena, q: dict, images_u8, labels=None):
    """predict_step_cpu with fc1 in MXFP4 (`q`: quantize_fc1_mxfp4 of `arena`): pre = alpha I + d1
    with I = sum_k wq u8 computed in float64 and rounded once to float32, then the reference
    forward's remaining layers in fp32."""
    acc = images_u8.reshape(-1, 784).to(torch.float64) @ torch.from_numpy(q["wq"]).to(torch.float64).t()
    pre = torch.from_numpy(np.asarray(I8_ALPHA)) * acc.to(torch.float32) + torch.from_numpy(q["d1"])
    return _prediction(_behind_fc1(model, arena, pre), labels)


def prune_fc1_24(arena) -> dict:
    """2:4 magnitude pruning of `arena`'s fc1 (docs/kernels.md "2:4 sparse evaluation"; the CPU twin
    and oracle of mlp_prune_24).  A row is 196 groups of 4 consecutive columns; a group keeps the
    two entries that rank first by (|w| descending, column ascending) with their fp32 bits (an
    all-zero group: columns 0 and 1), the others become zero.  Weights are finite: NaN and Inf
    are out of scope.  {"wp": float32 [128, 784] the dense pruned weights; "hi", "lo": int16 [128,
    416] the bf16 bits of the survivors in column order, hi = bf16(w), lo = bf16(w - hi), rows
    zero-padded from 392 on; "index": int32 [128, 28], word 4 kp + g holding the nibbles p0 |
    p1 << 2 (the survivors' positions, p0 < p1) of groups 32 kp + 16 h + 4 g + q at bits 16 h +
    4 q, zero for groups >= 196; "d1": float32 [128] = b1 - beta sum_k wp (the sum in float64,
    rounded once; the kernel's fixed-order fp32 sum is within its bound of it)}, NumPy."""
    w = arena.param("fc1.weight").detach().cpu().numpy().astype(np.float32).reshape(128, 196, 4)
    b = arena.param("fc1.bias").detach().cpu().numpy().astype(np.float32)
    a = np.abs(w)
    i, j = np.arange(4)[:, None], np.arange(4)[None, :]
    # entry j survives if fewer than two entries i rank before it
    first = (a[..., :, None] > a[..., None, :]) | ((a[..., :, None] == a[..., None, :]) & (i < j))
    keep = first.sum(axis=2) < 2
    p0, p1 = keep.argmax(axis=2), 3 - keep[..., ::-1].argmax(axis=2)
    nib = np.zeros((128, 7, 2, 4, 4), np.int64)                      # [n][kp][h][g][q]
    nib.reshape(128, 224)[:, :196] = p0 | (p1 << 2)
    shift = (16 * np.arange(2)[:, None, None] + 4 * np.arange(4)[None, None, :])
    index = (nib << shift).sum(axis=(2, 4)).astype(np.uint32).view(np.int32).reshape(128, 28)
    kept = torch.zeros(128, 416)
    kept[:, :392] = torch.from_numpy(np.take_along_axis(w, np.stack([p0, p1], axis=2), axis=2).reshape(128, 392))
    hi = kept.to(torch.bfloat16)
    lo = (kept - hi.float()).to(torch.bfloat16)
    wp = np.where(keep, w, np.float32(0)).reshape(128, 784)
    t = MX4_BETA * wp.sum(axis=1, dtype=np.float64).astype(np.float32)
    return {"wp": wp, "hi": hi.view(torch.int16).numpy(), "lo": lo.view(torch.int16).numpy(),
            "index": index, "d1": (b - t).astype(np.float32)}


@torch.no_grad()
def predict_step_cpu_sparse24(model: str, arena, q: dict, images_u8, labels=None):
    """predict_step_cpu with fc1 pruned 2:4 (`q`: prune_fc1_24 of `arena`): pre = alpha I + d1 with
    I = sum_k wp u8 computed in float64 and rounded once to float32, then the reference forward's
    remaining layers in fp32."""
    acc = images_u8.reshape(-1, 784).to(torch.float64) @ torch.from_numpy(q["wp"]).to(torch.float64).t()
    pre = torch.from_numpy(np.asarray(I8_ALPHA)) * acc.to(torch.float32) + torch.from_numpy(q["d1"])
    return _prediction(_behind_fc1(model, arena, pre), labels)


def check_attack(eps, steps, alpha):
    """(eps, steps, alpha) of an attack as ints: eps in 0..255 grey levels (0 returns the images),
    steps in 1..100, alpha in 1..255 or None for the default, eps at one step (FGSM), else
    max(1, round(2.5 eps / steps)) (PGD, Madry et al. 2018)."""
    eps, steps = int(eps), int(steps)
    if not 0 <= eps <= 255:
        raise ValueError(f"eps must be in 0..255 grey levels, got {eps}")
    if not 1 <= steps <= 100:
        raise ValueError(f"steps must be in 1..100, got {steps}")
    if alpha is None:
        alpha = max(1, eps if steps == 1 else int(2.5 * eps / steps + 0.5))
    alpha = int(alpha)
    if not 1 <= alpha <= 255:
        raise ValueError(f"alpha must be in 1..255 grey levels, got {alpha}")
    return eps, steps, alpha


def attack_step_cpu(model: str, arena, images_u8, labels, eps: int, steps: int, alpha: int):
    """FGSM / PGD on raw bytes (the CPU twin of csrc/kernels/mlp_attack.hip): `steps` times from
    x = x0 = images_u8 (uint8 [N, 784]),
        x = clamp(x + alpha sign(g), max(0, x0 - eps), min(255, x0 + eps)),   sign(0) = 0,
    g the autograd gradient of the per-sample plain NLL of `labels` with respect to the normalised
    pixels (the normalisation's slope is positive: the sign with respect to the byte).  uint8
    [N, 784]."""
    eps, steps, alpha = check_attack(eps, steps, alpha)
    views = {p.name: p.to_torch(arena.param(p.name)).detach() for p in arena.spec.params}
    x0 = images_u8.to(torch.int16)
    lo, hi = (x0 - eps).clamp_(min=0), (x0 + eps).clamp_(max=255)
    x = x0
    y = labels.to(torch.int64)
    for _ in range(steps):
        with torch.enable_grad():
            xn = normalize_reference(x.to(torch.uint8)).requires_grad_(True)
            loss = F.cross_entropy(functional_forward(model, views, xn), y, reduction="sum")
            g, = torch.autograd.grad(loss, xn)
        x = torch.minimum(torch.maximum(x + alpha * torch.sign(g).to(torch.int16).view_as(x), lo), hi)
    return x.to(torch.uint8)


@torch.no_grad()
def tta_reduce_cpu(logp_views, labels=None):
    """Test-time augmentation's combination (the CPU twin and oracle of csrc/kernels/tta.hip):
    ``logp_views`` fp32 [V, N, 10], the V per-view log-softmax rows, to the log of the mean
    probability, per class in fp32 as docs/kernels.md "Test-time augmentation" has it --
    m = max_v l, s = sum over v ascending of exp(l - m), out = (m + log(s)) - lnV with lnV =
    float32(log(float64(V))).  Returns predict_step_cpu's triple: (out fp32 [N, 10], pred int64
    [N], the first maximum of out, confusion int64 [10, 10] or None without labels)."""
    import math
    lv = torch.as_tensor(logp_views)
    if lv.dim() != 3 or lv.dtype != torch.float32 or lv.shape[0] < 1:
        raise ValueError(f"logp_views must be fp32 [V >= 1, N, C], got {lv.dtype} {tuple(lv.shape)}")
    m = lv.amax(dim=0)
    s = torch.zeros_like(m)
    for v in range(lv.shape[0]):
        s = s + torch.exp(lv[v] - m)
    lnv = torch.tensor(math.log(float(lv.shape[0])), dtype=torch.float64).to(torch.float32)
    out = (m + torch.log(s)) - lnv
    pred = out.argmax(dim=1)
    confusion = None
    if labels is not None:
        ncls = out.shape[1]
        confusion = torch.bincount(labels.to(torch.int64) * ncls + pred,
                                   minlength=ncls * ncls).view(ncls, ncls)
    return out, pred, confusion


@torch.no_grad()
def eval_step_cpu(model: str, arena, images_u8, labels, metrics_buf):
    x = normalize_reference(images_u8)
    views = {p.name: p.to_torch(arena.param(p.name)) for p in arena.spec.params}
    logits = functional_forward(model, views, x)
    loss = F.cross_entropy(logits, labels)
    bsz = images_u8.shape[0]
    metrics_buf[0] += loss.item() * bsz
    metrics_buf[1] += logits.argmax(dim=1).eq(labels).sum().item()
    metrics_buf[2] += bsz
