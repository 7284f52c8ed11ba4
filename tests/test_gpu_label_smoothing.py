"""Label smoothing in the training heads on the GPU (--label-smoothing E): cnn_head_smooth
(csrc/kernels/cnn_head.hip), cnn_head_dropout with its E argument and lin_train with its,
called directly against fp64 models of the definition

    t_c = (1 - E) [c = y] + E / 10
    row loss = lse - ((1 - E) l_y + E mean_c l_c)
    dlogits_c = (softmax_c - t_c) / B

at test_gpu_cnn_head.py's edge shapes, layouts and rule (the kernel's relative-norm error
against fp64 at most 8 x that of the same model in fp32 torch, floor 2e-6); E = 0 against the
unparameterised launches bit for bit; the schedule argument; one training step of the three
programs against fp64 autograd; two epochs through the graphs; and the CLI against the CPU path.

Measured on MI355X, relative-norm error against fp64: kernel | fp32 torch (bound = 8 x the
second column, at least 2e-6):

    head     B    S  scale  E    dh               dWfc2            dbfc2            dbfc1            loss sum
    smooth   1    32  1      0.1  9.7e-08|9.7e-08  1.3e-07|1.2e-07  7.3e-08|7.0e-08  9.7e-08|9.7e-08  2.8e-08|9.0e-08
    smooth   1    32  1      1.0  1.5e-07|1.2e-07  1.9e-07|1.5e-07  1.5e-07|1.2e-07  1.5e-07|1.2e-07  8.1e-08|5.4e-09
    smooth   1    32  40     0.1  6.6e-08|6.9e-08  1.1e-07|8.8e-08  2.6e-08|2.6e-08  6.6e-08|6.9e-08  7.0e-08|7.0e-08
    smooth   1    32  40     1.0  4.8e-08|7.6e-08  1.1e-07|8.9e-08  2.6e-08|2.6e-08  4.8e-08|7.6e-08  8.9e-08|8.8e-09
    smooth   37   32  1      0.1  1.8e-07|2.0e-07  2.8e-07|2.3e-07  3.2e-07|1.6e-07  2.9e-07|2.4e-07  2.0e-10|3.8e-08
    smooth   37   32  1      1.0  2.3e-07|2.5e-07  2.1e-07|1.7e-07  1.7e-07|1.4e-07  1.6e-07|1.4e-07  1.0e-08|7.4e-09
    smooth   37   32  40     0.1  6.5e-07|3.4e-07  5.4e-07|2.9e-07  5.5e-07|3.1e-07  5.8e-07|3.1e-07  9.6e-09|4.0e-08
    smooth   37   32  40     1.0  6.3e-07|3.2e-07  3.8e-07|2.1e-07  3.2e-07|1.8e-07  3.6e-07|1.9e-07  1.2e-08|1.0e-07
    smooth   64   16  1      0.1  1.9e-07|1.7e-07  1.6e-07|2.3e-07  1.4e-07|2.1e-07  1.5e-07|2.2e-07  1.6e-08|1.1e-08
    smooth   64   16  1      1.0  2.1e-07|2.0e-07  7.2e-08|1.4e-07  3.4e-08|1.8e-07  6.4e-08|1.3e-07  1.0e-08|3.8e-08
    smooth   64   16  40     0.1  7.5e-07|1.1e-06  6.4e-07|9.5e-07  4.4e-07|6.5e-07  4.6e-07|6.8e-07  7.5e-10|6.4e-08
    smooth   64   16  40     1.0  7.4e-07|1.1e-06  4.3e-07|6.2e-07  2.7e-07|3.0e-07  3.2e-07|4.5e-07  2.6e-08|7.6e-08
    smooth   40   2   1      0.1  1.2e-07|1.4e-07  1.1e-07|1.5e-07  1.0e-07|1.2e-07  1.1e-07|1.3e-07  8.5e-10|8.5e-10
    smooth   40   2   1      1.0  1.4e-07|1.8e-07  8.8e-08|1.4e-07  7.9e-08|1.0e-07  7.0e-08|8.3e-08  7.5e-09|8.3e-08
    smooth   40   2   40     0.1  2.1e-07|2.2e-07  1.7e-07|2.0e-07  1.2e-07|1.6e-07  1.3e-07|1.5e-07  2.2e-08|6.2e-08
    smooth   40   2   40     1.0  2.0e-07|2.0e-07  1.7e-07|1.7e-07  1.3e-07|1.2e-07  1.4e-07|1.3e-07  8.6e-09|9.4e-10
    smooth   40   1   1      0.1  1.3e-07|1.5e-07  1.5e-07|1.6e-07  1.5e-07|1.7e-07  1.6e-07|1.8e-07  1.7e-08|6.9e-08
    smooth   40   1   1      1.0  1.6e-07|1.8e-07  1.2e-07|1.3e-07  9.7e-08|1.0e-07  1.0e-07|1.1e-07  1.3e-08|7.0e-08
    smooth   40   1   40     0.1  2.4e-07|8.9e-07  2.3e-07|8.9e-07  2.0e-07|7.3e-07  2.0e-07|7.3e-07  3.2e-08|2.8e-08
    smooth   40   1   40     1.0  2.5e-07|9.0e-07  2.3e-07|8.4e-07  2.0e-07|6.6e-07  2.1e-07|6.3e-07  2.7e-08|5.9e-08
    smooth   33   48  1      0.1  2.6e-07|2.1e-07  2.2e-07|2.1e-07  1.7e-07|1.7e-07  2.0e-07|2.0e-07  5.3e-09|5.3e-08
    smooth   33   48  1      1.0  3.1e-07|2.6e-07  1.2e-07|1.3e-07  8.2e-08|8.4e-08  9.6e-08|1.1e-07  4.5e-08|5.4e-08
    smooth   33   48  40     0.1  4.5e-07|8.5e-07  3.9e-07|7.1e-07  3.3e-07|5.8e-07  3.4e-07|6.1e-07  2.1e-08|6.0e-08
    smooth   33   48  40     1.0  4.1e-07|8.0e-07  2.8e-07|5.3e-07  1.8e-07|3.9e-07  2.3e-07|4.5e-07  3.4e-09|1.0e-07
    smooth   1030 4   1      0.1  1.4e-07|1.5e-07  1.7e-07|2.1e-07  1.7e-07|1.7e-07  1.7e-07|1.5e-07  1.0e-08|8.8e-08
    smooth   1030 4   1      1.0  1.7e-07|1.8e-07  4.6e-08|1.3e-07  4.2e-08|5.3e-08  4.5e-08|6.4e-08  2.5e-09|4.7e-09
    smooth   1030 4   40     0.1  5.3e-07|9.2e-07  1.9e-07|3.1e-07  1.6e-07|1.8e-07  1.8e-07|2.2e-07  9.8e-09|1.8e-09
    smooth   1030 4   40     1.0  5.1e-07|8.8e-07  8.3e-08|1.7e-07  6.5e-08|9.9e-08  1.1e-07|1.4e-07  5.8e-09|3.2e-08
    drop+sm  37   32  1      0.1  2.0e-07|2.0e-07  2.7e-07|2.6e-07  3.6e-07|2.9e-07  2.6e-07|2.7e-07  1.4e-08|3.4e-08
    drop+sm  1030 4   1      0.1  1.5e-07|1.6e-07  1.7e-07|2.2e-07  1.9e-07|2.0e-07  1.6e-07|1.6e-07  9.5e-09|6.3e-08

(drop+sm: cnn_head_dropout at T = 16384 with E).  The largest kernel error is 7.5e-07, so the
2e-6 floor alone holds every case; `correct` was exact everywhere (one near-tie row at
B = 1030 scale 1).  dh / dht were bit-identical to bf16(dh32), the slab to the other mode's and
the second launch's, and every E = 0 launch to the unparameterised one.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_mnist_amd.data.dropout import DropoutSpec, keep_mask
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.models.reference import functional_forward
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_gpu_app import EPOCH_RE, cli
from test_gpu_cnn_f32 import _kernel_a1_active, _reference_net, rel
from test_gpu_cnn_head import (GUARD, HID, M0, NCLS, QUANT, SHAPES, SLAB, _C, _ldt, bits,
                               check_bf16_layout, check_common, make_inputs, nanbuf, relerr,
                               slab_sums)
from test_gpu_dropout import _indices

pytestmark = pytest.mark.gpu

EPOCH = 3
DROP = DropoutSpec(0.25, seed=(9 << 32) + 41)
E0_SHAPES = [(37, 32), (1030, 4)]


def reference(part, bf1, wf2, bf2, y, e, dt, mult=None):
    """test_gpu_cnn_head.reference with the smoothed target and loss (and, with mult [B, 128] =
    keep * scale, test_gpu_dropout.reference's mask), every operation in dtype `dt`."""
    part, bf1, wf2, bf2 = (t.to(dt) for t in (part, bf1, wf2, bf2))
    mult = torch.ones(1, dtype=dt) if mult is None else mult.to(dt)
    B = part.shape[1]
    h = torch.relu(part.sum(0) + bf1)
    hd = h * mult
    lg = hd @ wf2.t() + bf2
    yl = y.long()
    t = F.one_hot(yl, NCLS).to(dt) * (1.0 - e) + e / NCLS
    ly = lg.gather(1, yl[:, None])[:, 0]
    rowloss = torch.logsumexp(lg, 1) - ((1.0 - e) * ly + e * lg.mean(1))
    dl = (torch.softmax(lg, 1) - t) / B
    dh = (dl @ wf2) * mult * (h > 0).to(dt)
    return dict(logits=lg, dh=dh, dWfc2=dl.t() @ hd, dbfc2=dl.sum(0), dbfc1=dh.sum(0),
                loss=rowloss.sum(), correct=int((lg.argmax(1) == yl).sum()))


def _near(r64):
    top2 = r64["logits"].topk(2, dim=1).values
    return int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())


@functools.lru_cache(maxsize=None)
def case(B, S, scale, e):
    """test_gpu_cnn_head.case's inputs with the smoothed references; computed once on the CPU,
    shared and never modified."""
    inp = make_inputs(B, S, scale, 1000 * B + S)
    r64 = reference(*inp, e, torch.float64)
    r32 = reference(*inp, e, torch.float32)
    assert all(torch.isfinite(torch.as_tensor(r64[q])).all() for q in QUANT)
    return inp, r64, r32, _near(r64)


@functools.lru_cache(maxsize=None)
def drop_case(B, S, e):
    """Inputs with labels tagged by dataset indices, the NumPy mask of DROP and the smoothed,
    masked references (test_gpu_dropout.case's construction)."""
    part, bf1, wf2, bf2, y = make_inputs(B, S, 1, 1000 * B + S)
    idx = _indices(B, 7 * B + S)
    keep = torch.from_numpy(keep_mask(idx, EPOCH, DROP))
    mult = keep.float() * DROP.scale
    am = reference(part, bf1, wf2, bf2, y, e, torch.float64, mult)["logits"].argmax(1)
    y = torch.where(torch.arange(B) % 2 == 1, am.to(torch.int32), y)
    word = (y.long() | (idx << 4)).to(torch.int32)
    r64 = reference(part, bf1, wf2, bf2, y, e, torch.float64, mult)
    r32 = reference(part, bf1, wf2, bf2, y, e, torch.float32, mult)
    return (part, bf1, wf2, bf2, word), keep, r64, r32, _near(r64)


def launch(C, dev, inp, bf16_mode, head, e=None, sched=None):
    """One training-head launch into NaN-guarded buffers -> dict of CPU results
    (test_gpu_cnn_head.launch_train's).  head: "plain" (cnn_head), "smooth" (cnn_head_smooth, E
    required) or "drop" (cnn_head_dropout with DROP; E passed only when given); inp's labels
    are tagged words for "drop"."""
    part, bf1, wf2, bf2, y = inp
    S, B = part.shape[0], part.shape[1]
    ldt = _ldt(B)
    nblk = C.cnn_head_nblk(ldt)
    slab = nanbuf(nblk * SLAB, torch.float32, dev)
    metrics = torch.tensor(M0, dtype=torch.float64, device=dev)
    c0 = torch.tensor([41], dtype=torch.int64, device=dev)
    c1 = torch.tensor([7], dtype=torch.int64, device=dev)
    dh = dht = dh32 = None
    if bf16_mode:
        dh, dht = nanbuf(ldt * HID, torch.bfloat16, dev), nanbuf(ldt * HID, torch.bfloat16, dev)
    else:
        dh32 = nanbuf(ldt * HID, torch.float32, dev)
    args = (part.reshape(-1).to(dev), S, B, bf1.to(dev), wf2.reshape(-1).to(dev), bf2.to(dev),
            y.to(dev))
    kw = {} if sched is None else {"lr_sched": sched}
    if head == "plain":
        assert e is None
        C.cnn_head(*args, True, dh, dht, ldt, slab, metrics, c0, c1, None, dh32, **kw)
    elif head == "smooth":
        C.cnn_head_smooth(*args, dh, dht, ldt, slab, metrics, c0, c1, None, dh32, e, **kw)
    else:
        if e is not None:
            kw["label_smoothing"] = e
        C.cnn_head_dropout(*args, dh, dht, ldt, slab, metrics, c0, c1, None, dh32,
                           torch.tensor([EPOCH], dtype=torch.int32, device=dev), DROP.seed, DROP.T,
                           DROP.scale, **kw)
    torch.cuda.synchronize()
    out = dict(slab=slab.cpu(), metrics=metrics.cpu(), c0=int(c0.item()), c1=int(c1.item()),
               nblk=nblk, ldt=ldt)
    for k, t in (("dh", dh), ("dht", dht), ("dh32", dh32)):
        if t is not None:
            out[k] = t.cpu()
    for k in ("slab", "dh", "dht", "dh32"):            # nothing written past the buffer
        if k in out:
            assert torch.isnan(out[k][-GUARD:].float()).all(), k
            out[k] = out[k][:-GUARD]
    return out


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in ("slab", "dh", "dht", "dh32"):
        if k in a:
            assert torch.equal(bits(a[k]), bits(b[k])), k
    assert torch.equal(a["metrics"].view(torch.int64), b["metrics"].view(torch.int64))
    assert (a["c0"], a["c1"], a["nblk"], a["ldt"]) == (b["c0"], b["c1"], b["nblk"], b["ldt"])


def check_against_fp64(name, f32, b16, B, r64, r32, near):
    """The rule of test_head_train_vs_fp64 on one fp32-mode and one bf16-mode launch."""
    for out in (f32, b16):
        check_common(out, B)
    ldt = f32["ldt"]
    dh32 = f32["dh32"].view(ldt, HID)
    assert torch.isfinite(dh32).all()
    assert (bits(dh32[B:]) == 0).all()                            # padding rows exactly zero
    check_bf16_layout(f32, b16, B)
    assert torch.equal(bits(f32["slab"]), bits(b16["slab"]))      # the slab: mode-independent
    got = slab_sums(f32)
    got["dh"] = dh32[:B]
    errs = {q: (relerr(torch.as_tensor(got[q]), r64[q]), relerr(torch.as_tensor(r32[q]), r64[q]))
            for q in QUANT}
    print(f"\n{name}: " + "  ".join(f"{q} {k:.1e}|{t:.1e}" for q, (k, t) in errs.items()) +
          f"  correct {got['correct']:.0f}/{r64['correct']} near {near}")
    for q, (k, t) in errs.items():
        assert k <= max(8 * t, 2e-6), (q, k, t)
    assert got["correct"] == int(got["correct"])
    assert abs(got["correct"] - r64["correct"]) <= near, (got["correct"], r64["correct"], near)
    return dh32


@pytest.mark.parametrize("e", [0.1, 1.0])
@pytest.mark.parametrize("scale", [1, 40])
@pytest.mark.parametrize("B,S", SHAPES)
def test_smooth_head_vs_fp64(gpu, B, S, scale, e):
    """cnn_head_smooth: dh32, the bf16 dh / dht copies, the slab sums (the smoothed loss among
    them), `correct`, the untouched train metrics and the counters."""
    C = _C()
    inp, r64, r32, near = case(B, S, scale, e)
    assert near <= (0 if B <= 64 else B // 100), near            # from the reference alone
    f32 = launch(C, gpu, inp, False, "smooth", e)
    b16 = launch(C, gpu, inp, True, "smooth", e)
    b16b = launch(C, gpu, inp, True, "smooth", e)
    check_against_fp64(f"smooth head B={B} S={S} scale={scale} E={e}", f32, b16, B, r64, r32, near)
    same_bits(b16, b16b)                                          # and between two launches
    # the smoothing matters: the hard-target loss sum is another number
    hard = reference(*inp, 0.0, torch.float64)["loss"]
    assert abs(hard - r64["loss"]) > 1e-3 * abs(r64["loss"])


def _lin_inputs(B, seed):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (B, 784), generator=g, dtype=torch.uint8)
    labels = torch.randint(0, 10, (B,), generator=g)
    W = torch.randn(10, 784, generator=g) * 0.05
    b = torch.randn(10, generator=g) * 0.1
    return images, labels, W, b


def _lin_launch(C, dev, inputs, e=None, sched=None):
    """One lin_train launch over the B rows of an epoch buffer -> (slab [nblk, LIN_SLAB], metrics,
    optimizer-step counter), on the CPU."""
    images, labels, W, b = inputs
    B = images.shape[0]
    nblk = (B + C.LIN_ROWS - 1) // C.LIN_ROWS
    slab = nanbuf(nblk * C.LIN_SLAB, torch.float32, dev)
    ctr = torch.zeros(1, dtype=torch.int64, device=dev)
    c1 = torch.tensor([7], dtype=torch.int64, device=dev)
    metrics = torch.tensor(M0, dtype=torch.float64, device=dev)
    kw = {} if e is None else {"label_smoothing": e}
    if sched is not None:
        kw["lr_sched"] = sched
    C.lin_train(images.to(dev), labels.to(dev, torch.int32), None, ctr, B, B, W.to(dev), b.to(dev),
                slab[:-GUARD], metrics, c1, **kw)
    torch.cuda.synchronize()
    s = slab.cpu()
    assert torch.isnan(s[-GUARD:]).all()
    return s[:-GUARD].view(nblk, C.LIN_SLAB), metrics.cpu(), int(c1.item())


@pytest.mark.parametrize("B,S", E0_SHAPES)
def test_zero_smoothing_has_the_unparameterised_bits(gpu, B, S):
    """E = 0 through every launch that takes E: cnn_head_smooth against cnn_head,
    cnn_head_dropout and lin_train with the argument against the calls without it -- every
    output, bit for bit."""
    C = _C()
    inp = make_inputs(B, S, 1, 1000 * B + S)
    word = (inp[4].long() | (_indices(B, B) << 4)).to(torch.int32)
    for bf16_mode in (False, True):
        same_bits(launch(C, gpu, inp, bf16_mode, "smooth", 0.0),
                  launch(C, gpu, inp, bf16_mode, "plain"))
        same_bits(launch(C, gpu, inp[:4] + (word,), bf16_mode, "drop", 0.0),
                  launch(C, gpu, inp[:4] + (word,), bf16_mode, "drop"))
    lin = _lin_inputs(B, B)
    a, b = _lin_launch(C, gpu, lin, 0.0), _lin_launch(C, gpu, lin)
    # (the slab's padding columns 7852.. are never written: NaN in both)
    assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]) and a[2] == b[2] == 8
    assert torch.isfinite(a[0][:, :7852]).all()


@pytest.mark.parametrize("B,S", E0_SHAPES)
def test_dropout_head_with_smoothing_vs_fp64(gpu, B, S):
    """cnn_head_dropout at T = round(0.25 * 65536) and E = 0.1 against the fp64 model with the
    mask of data/dropout.py and the smoothed target, at the same rule; dropped units' dh
    entries are exactly +0."""
    C = _C()
    e = 0.1
    assert DROP.T == round(0.25 * 65536)
    inp, keep, r64, r32, near = drop_case(B, S, e)
    assert near <= (0 if B <= 64 else B // 100), near            # from the reference alone
    f32 = launch(C, gpu, inp, False, "drop", e)
    b16 = launch(C, gpu, inp, True, "drop", e)
    dh32 = check_against_fp64(f"dropout x smoothing head B={B} S={S} E={e}", f32, b16, B, r64, r32,
                              near)
    assert (bits(dh32[:B])[keep == 0] == 0).all()                 # dropped units exactly +0
    assert 0 < int((keep == 0).sum()) < keep.numel()
    # neither the mask nor the smoothing is a detail
    y = inp[4] & 15
    assert relerr(dh32[:B], reference(*inp[:4], y, e, torch.float64)["dh"]) > 0.1
    hard = reference(*inp[:4], y, 0.0, torch.float64, keep.float() * DROP.scale)
    assert relerr(dh32[:B], hard["dh"]) > 1e-2


@pytest.mark.parametrize("B", [1, 5, 256])
def test_lin_train_with_smoothing_vs_fp64(gpu, B):
    """lin_train at E = 0.1 (B = 1: one row; 5: a partial group of LIN_ROWS = 4): the slab sums
    of dW, db, loss and correct against fp64, at tests/test_gpu_linear.py's tolerances for the
    unsmoothed kernel."""
    C = _C()
    e = 0.1
    assert C.LIN_ROWS == 4
    images, labels, W, b = lin = _lin_inputs(B, 100 + B)
    x = normalize_reference(images).double()
    lg = x @ W.double().t() + b.double()
    t = F.one_hot(labels, 10).double() * (1.0 - e) + e / 10
    rowloss = torch.logsumexp(lg, 1) - ((1.0 - e) * lg.gather(1, labels[:, None])[:, 0] +
                                        e * lg.mean(1))
    dl = (torch.softmax(lg, 1) - t) / B
    slab, metrics, c1 = _lin_launch(C, gpu, lin, e)
    s = slab.double().sum(0)
    gW, gb = s[:7840].view(10, 784), s[7840:7850]
    print(f"\nlin_train B={B}: dW {relerr(gW, dl.t() @ x):.1e} db {relerr(gb, dl.sum(0)):.1e} "
          f"loss {s[7850].item()} vs {rowloss.sum().item()}")
    assert torch.allclose(gW, dl.t() @ x, atol=2e-6, rtol=1e-4)
    assert torch.allclose(gb, dl.sum(0), atol=2e-6, rtol=1e-4)
    assert abs(s[7850].item() - rowloss.sum().item()) < 1e-4 * B
    assert s[7851].item() == int((lg.argmax(1) == labels).sum())
    # lin_train adds the sample count only (the slab's loss / correct are summed downstream)
    assert metrics.tolist() == [M0[0], M0[1], M0[2] + B] and c1 == 8
    # the smoothing matters: the hard-target dW is somewhere else
    hard = (torch.softmax(lg, 1) - F.one_hot(labels, 10).double()) / B
    assert relerr(gW, hard.t() @ x) > 1e-2


@pytest.mark.parametrize("B,S", [(1, 32), (37, 32)])
@pytest.mark.parametrize("bf16_mode", [False, True])
def test_smooth_head_advances_the_schedule(gpu, B, S, bf16_mode):
    """cnn_head_smooth with an LrSched (tests/test_gpu_lr_schedule.py's direct call): the rate
    word takes the table's entries from the cursor on, the cursor moves, every other output has
    the bits of the call without a schedule."""
    C = _C()
    table_host, start = [0.125, 0.3, 1e-3, 0.07, 2.5e-4], 2
    inp = make_inputs(B, S, 1, 1000 * B + S)
    plain = launch(C, gpu, inp, bf16_mode, "smooth", 0.1)
    table = torch.tensor(table_host, dtype=torch.float64, device=gpu)
    cursor = torch.tensor([start], dtype=torch.int64, device=gpu)
    lr = torch.tensor([-1.0], dtype=torch.float64, device=gpu)
    for call in range(3):
        got = launch(C, gpu, inp, bf16_mode, "smooth", 0.1, sched=(table, cursor, lr))
        assert lr.item() == table_host[start + call], (call, lr.item())
        assert cursor.item() == start + call + 1
        same_bits(got, plain)
    assert table.cpu().tolist() == table_host                    # the table is only read
    slab, metrics, c1 = _lin_launch(C, gpu, _lin_inputs(5, 5), 0.1, sched=(table, cursor.zero_(), lr))
    ref = _lin_launch(C, gpu, _lin_inputs(5, 5), 0.1)
    assert lr.item() == table_host[0] and cursor.item() == 1
    assert torch.equal(bits(slab), bits(ref[0])) and torch.equal(metrics, ref[1]) and c1 == ref[2]


def test_smoothing_argument_is_checked(gpu):
    C = _C()
    inp = make_inputs(4, 1, 1, 5)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(RuntimeError, match="label_smoothing"):
            launch(C, gpu, inp, False, "smooth", bad)
        with pytest.raises(RuntimeError, match="label_smoothing"):
            launch(C, gpu, inp, False, "drop", bad)
        with pytest.raises(RuntimeError, match="label_smoothing"):
            _lin_launch(C, gpu, _lin_inputs(4, 4), bad)


# ---- the programs --------------------------------------------------------------------------

E = 0.1


def _program(arch, dtype, B, n, lr=0.0, graphs=False, seed=0, e=E, dropout=None, opt="sgd"):
    train = synthetic_split(n, True)
    test = synthetic_split(128, False)
    prog = build_local_program(arch, dtype, "cuda", B, train, test, optimizer=opt, lr=lr,
                               momentum=0.0 if lr in (0.0, 1.0) else 0.9,
                               weight_decay=0.0 if lr in (0.0, 1.0) else 1e-4, seed=seed,
                               use_graphs=graphs, label_smoothing=e, dropout=dropout)
    prog.optimizer.sync_hyperparams()
    return prog, train


# B = 32: the row-band kernels (tests/test_gpu_dropout.py's one-step batch); B = 300: the
# one-image kernels, at the smallest batch for which the bf16 one-step bounds are established
# (tests/test_gpu_cnn.py test_cnn_step_gradients_match_autograd).  They are bounds on the bf16
# program's own rounding noise, which depends on the batch and not on E: at B = 129, the
# smallest batch the one-image kernels take, fc1.bias measured 6.2e-2 against fp64 both at
# E = 0 (6.15e-2) and at E = 0.1 (6.22e-2); at B = 300, 4.67e-2 and 4.61e-2.
@pytest.mark.parametrize("B", [32, 300])
def test_bf16_program_gradients_with_smoothing(gpu, B):
    """One bf16 training step at E = 0.1 against fp64 autograd with label_smoothing = 0.1, at
    test_bf16_program_gradients_with_dropout's bounds for plain autograd (5e-2, conv 1.2e-1;
    loss 2e-2)."""
    prog, train = _program("cnn", "bf16", B, 600)
    assert (prog.gpu.bands(B) > 1) == (B == 32)
    prog.gpu.keep_grads = True
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx)
    tp = prog.arena.torch_tensors(prog.arena.params)
    prog.gpu.begin_epoch()
    prog.metrics.reset(0)
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    x, y = normalize_reference(train.images[sel]), train.labels[sel]
    got = prog.arena.torch_tensors(prog.arena.grads)
    leaves = {k: v.double().requires_grad_() for k, v in tp.items()}
    logits = functional_forward("cnn", leaves, x.double())
    loss = F.cross_entropy(logits, y, label_smoothing=E)
    loss.backward()
    for name, leaf in leaves.items():
        r = rel(got[name].double(), leaf.grad)
        print(f"bf16 smoothing step B={B} vs fp64 {name}: {r:.2e}")
        assert r < (1.2e-1 if name.startswith("conv") else 5e-2), (name, r)
    mt = prog.metrics.buf[0:3].cpu()
    print(f"loss {mt[0].item() / B} vs {loss.item()} (hard {F.cross_entropy(logits, y).item()})")
    assert abs(mt[0].item() / B - loss.item()) < 2e-2 * max(1.0, loss.item())
    assert mt[2].item() == B
    # the fc2 bias gradient is sum_rows (softmax - t) / B: nearer the smoothed model's than the
    # hard-target one's
    plain = {k: v.double().requires_grad_() for k, v in tp.items()}
    F.cross_entropy(functional_forward("cnn", plain, x.double()), y).backward()
    assert rel(got["fc2.bias"].double(), leaves["fc2.bias"].grad) < \
        rel(got["fc2.bias"].double(), plain["fc2.bias"].grad)


@pytest.mark.parametrize("B,conv", [(32, "exact"), (32, "x3"), (129, "exact")])
def test_f32_program_gradients_with_smoothing(gpu, B, conv):
    """One fp32 training step at E = 0.1 against fp64 autograd with label_smoothing = 0.1
    (max-pool and, in split-bf16 mode, conv1's ReLU routed as the kernels routed them), at
    test_f32_program_gradients_with_dropout's 1e-4."""
    prog, train = _program("cnn", "fp32", B, 300)
    prog.gpu.conv_x3 = conv == "x3"
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx)
    prog.gpu.begin_epoch()
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    x = normalize_reference(train.images[sel]).view(B, 1, 28, 28)
    y = train.labels[sel]
    a1_active = _kernel_a1_active(prog, B) if conv == "x3" else None
    net = _reference_net(prog).double()
    z1 = net.conv1(x.double())
    zero = torch.zeros((), dtype=torch.float64)
    a1 = F.relu(z1) if a1_active is None else torch.where(a1_active, z1, zero)
    z2 = net.conv2(a1)
    mk = prog.gpu.pmask[:B * 9216].view(B, 12, 12, 64).permute(0, 3, 1, 2).cpu().long()
    pos = (mk & 0x80) != 0
    sidx = torch.where(pos, (mk & 0xf).float().log2().long(), torch.zeros_like(mk))
    py = torch.arange(12).view(1, 1, 12, 1)
    px = torch.arange(12).view(1, 1, 1, 12)
    flat = (2 * py + (sidx >> 1)) * 24 + 2 * px + (sidx & 1)
    pooled = torch.where(pos, z2.flatten(2).gather(2, flat.flatten(2)).view(B, 64, 12, 12), zero)
    out = net.fc2(F.relu(net.fc1(pooled.flatten(1))))
    loss = F.cross_entropy(out, y, label_smoothing=E)
    loss.backward()
    got = prog.arena.torch_tensors(prog.arena.grads)
    for name, p in net.named_parameters():
        r = rel(got[name].double(), p.grad)
        print(f"fp32 ({conv}) smoothing step B={B} vs fp64 {name}: {r:.2e}")
        assert r < 1e-4, (name, r)
    assert abs(prog.metrics.buf[0].item() - loss.item() * B) <= 1e-4 * B
    assert prog.metrics.buf[1].item() == (out.argmax(1) == y).sum().item()
    # the smoothing matters: fc2's hard-target bias gradient is somewhere else
    hard = (torch.softmax(out.detach(), 1) - F.one_hot(y, 10)).sum(0) / B
    assert rel(got["fc2.bias"].double(), hard) > 1e-2


@pytest.mark.parametrize("B", [32, 129])
def test_linear_program_step_with_smoothing(gpu, B):
    """One Linear step (SGD, lr = 1, no momentum or decay: the update is the gradient) at
    E = 0.1 against fp64 autograd with label_smoothing = 0.1, at tests/test_gpu_linear.py's
    tolerances."""
    prog, train = _program("linear", "fp32", B, 300, lr=1.0)
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx)
    before = {k: v.clone() for k, v in prog.arena.torch_tensors(prog.arena.params).items()}
    prog.gpu.begin_epoch()
    prog.metrics.reset(0)
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    after = prog.arena.torch_tensors(prog.arena.params)
    sel = idx[:B]
    x, y = normalize_reference(train.images[sel]).double(), train.labels[sel]
    leaves = {k: v.double().cpu().requires_grad_() for k, v in before.items()}
    logits = functional_forward("linear", leaves, x)
    loss = F.cross_entropy(logits, y, label_smoothing=E)
    loss.backward()
    for name, leaf in leaves.items():
        g = (before[name].double() - after[name].double()).cpu()
        print(f"linear smoothing step B={B} {name}: {rel(g, leaf.grad):.2e}")
        assert torch.allclose(g, leaf.grad, atol=2e-6, rtol=1e-4), name
    mt = prog.metrics.buf[0:3].cpu()
    assert abs(mt[0].item() - loss.item() * B) < 1e-4 * B
    assert mt[1].item() == (logits.argmax(1) == y).sum().item() and mt[2].item() == B


@pytest.mark.parametrize("arch,dtype", [("cnn", "bf16"), ("linear", "fp32")])
def test_two_epochs_through_the_graphs(gpu, arch, dtype):
    """5 full batches of 64 and a tail of 40, two epochs at E = 0.1: the graph path equals the
    eager one bit for bit (E is baked into the captured launches), and not a run at E = 0."""
    n = 64 * 5 + 40
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(3)]
    res = {}
    for name, graphs, e in (("graphs", True, E), ("eager", False, E), ("hard", True, 0.0)):
        prog, _ = _program(arch, dtype, 64, n, lr=0.02, graphs=graphs, seed=7, e=e)
        losses = []
        for ep in range(2):
            prog.set_train_indices(order[ep], order[ep + 1], epoch=ep)
            tl, _ = prog.train_epoch()
            losses.append(tl.average)
        torch.cuda.synchronize()
        assert prog.gpu.use_graphs == graphs and bool(prog.gpu.graphs) == graphs
        res[name] = (prog.arena.params.clone(), losses)
    assert torch.equal(res["graphs"][0], res["eager"][0]) and res["graphs"][1] == res["eager"][1]
    assert not torch.equal(res["hard"][0], res["graphs"][0])
    assert res["hard"][1][0] != res["graphs"][1][0]


def test_program_composes_dropout_and_smoothing(gpu):
    """launch_head_train with both on: one bf16 step at B = 32 against fp64 autograd with the
    NumPy mask and label_smoothing = 0.1 (the dropout one-step test's bounds)."""
    B = 32
    spec = DropoutSpec(0.5, seed=(9 << 32) + 41)
    prog, train = _program("cnn", "bf16", B, 600, dropout=spec)
    prog.gpu.keep_grads = True
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx, epoch=EPOCH)
    tp = prog.arena.torch_tensors(prog.arena.params)
    prog.gpu.begin_epoch()
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    x, y = normalize_reference(train.images[sel]), train.labels[sel]
    mult = torch.from_numpy(keep_mask(sel, EPOCH, spec)).double() * spec.scale
    got = prog.arena.torch_tensors(prog.arena.grads)
    leaves = {k: v.double().requires_grad_() for k, v in tp.items()}
    F.cross_entropy(functional_forward("cnn", leaves, x.double(), mult), y,
                    label_smoothing=E).backward()
    for name, leaf in leaves.items():
        r = rel(got[name].double(), leaf.grad)
        print(f"bf16 dropout x smoothing step vs fp64 {name}: {r:.2e}")
        assert r < (1.2e-1 if name.startswith("conv") else 5e-2), (name, r)


@pytest.mark.parametrize("conv,loss_tol,acc_tol", [("exact", 5e-5, 0.1), ("x3", 2e-3, 0.5)])
def test_cnn_fp32_cli_gpu_matches_cpu_with_smoothing(gpu, tmp_path, monkeypatch, conv, loss_tol,
                                                     acc_tol):
    """test_cnn_fp32_cli_gpu_matches_cpu_with_dropout's comparison with --label-smoothing 0.1:
    its epochs and tolerances (exact products: both epochs; split-bf16: the first)."""
    monkeypatch.setenv("PDM_F32_CONV", conv)
    d1, d2 = tmp_path / "gpu", tmp_path / "cpu"
    d1.mkdir()
    d2.mkdir()
    common = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.05", "--dtype", "fp32",
              "--synthetic-size", "1024", "--epochs", "2" if conv == "exact" else "1", "--seed", "4",
              "--label-smoothing", "0.1"]
    g = [l for l in cli(common, d1) if l.startswith("Epoch:")]
    c = [l for l in cli(common, d2, device="cpu", backend="gloo") if l.startswith("Epoch:")]
    assert len(g) == len(c) == (2 if conv == "exact" else 1)
    for lg, lc in zip(g, c):
        print(lg, "|", lc)
        mg, mc = EPOCH_RE.match(lg), EPOCH_RE.match(lc)
        for i in (3, 5):
            assert abs(float(mg.group(i)) - float(mc.group(i))) < loss_tol, (lg, lc)
        for i in (4, 6):
            assert abs(float(mg.group(i)) - float(mc.group(i))) <= acc_tol, (lg, lc)
        assert float(mg.group(3)) >= 0.5 - 1e-3          # the smoothed loss's floor H(0.1)
