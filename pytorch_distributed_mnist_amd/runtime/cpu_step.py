"""CPU execution of one training / eval step (the gloo plumbing path and the oracle).

Semantics are the reference Trainer's (``multi_proc_single_gpu.py:77-116``):
normalise the gathered uint8 batch, forward, ``F.cross_entropy`` (mean), backward,
then optimizer step.  Parameters are taken from the flat arena in kernel
layout and exposed to autograd through the (permuting) torch-layout views, so
the gradients land in kernel layout directly in the gradient arena.
"""
from __future__ import annotations

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
    logits = functional_forward(model, views, x)
    log_probs = F.log_softmax(logits, dim=1)
    pred = logits.argmax(dim=1)
    confusion = None
    if labels is not None:
        ncls = logits.shape[1]
        confusion = torch.bincount(labels.to(torch.int64) * ncls + pred,
                                   minlength=ncls * ncls).view(ncls, ncls)
    return log_probs, pred, confusion


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
