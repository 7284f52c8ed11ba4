"""Mixup on the GPU (--mixup): the mixing epoch gather (csrc/kernels/augment.hip
gather_epoch_mixup_kernel) against its NumPy oracle (data/mixup.py, data/augment.py) bit for bit
and, with a table of 256, against the elastic gather; the pairs (mixup_pairs_rows) against the
oracle; the two-class head (csrc/kernels/cnn_head_mix.hip) called directly against an fp64 model
of the head (test_gpu_cnn_head.py's edge shapes, layouts and tolerance rule), with a table of
256 against cnn_head_dropout bit for bit, with y2 == y against the single-label model, and with
the schedule argument; one training step of both CNN programs against fp64 autograd on the
oracle-mixed images; two epochs through the graphs; and the CLI against the CPU path."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_mnist_amd.data.augment import AugmentSpec, augment_batch
from pytorch_distributed_mnist_amd.data.dropout import DropoutSpec, keep_mask, tag_labels
from pytorch_distributed_mnist_amd.data.mixup import MixupSpec, draw, mix_batch
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.models.reference import functional_forward
from pytorch_distributed_mnist_amd.optim.schedule import ScheduleSpec
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_gpu_app import EPOCH_RE, cli
from test_gpu_cnn_f32 import _kernel_a1_active, _reference_net, rel
from test_gpu_cnn_head import SHAPES as HEAD_SHAPES
from test_gpu_cnn_head import (GUARD, HID, M0, NCLS, QUANT, SLAB, _C, _ldt, bits, check_bf16_layout,
                               check_common, make_inputs, nanbuf, relerr, slab_sums)
from test_gpu_dropout import _indices

pytestmark = pytest.mark.gpu

EPOCH = 3
MIX = MixupSpec(0.4, seed=(5 << 32) + 19)
DROP = DropoutSpec(0.5, seed=(9 << 32) + 41)
NIMG = 97
ONES = np.full(1024, 256, dtype=np.int32)            # the table that mixes nothing


def _epoch_word(e, dev):
    return torch.tensor([e], dtype=torch.int32, device=dev)


def _dev(a, dev="cuda"):
    return torch.from_numpy(np.array(a)).to(dev)          # (a copy: the cached table is read-only)


# ---------------------------------------------------------------------------- the gather

SETTINGS = {"identity": AugmentSpec(0, 0.0, 0.0, seed=30),
            "affine": AugmentSpec(2, 10.0, 0.1, seed=(9 << 32) + 32),
            "elastic": AugmentSpec(0, 0.0, 0.0, seed=31, elastic=2.0)}
GATHER_EPOCHS = (0, EPOCH)


@pytest.fixture(scope="module")
def source():
    """97 random source images and labels and, per (setting, epoch), the oracle's output for
    every one of them: its blend with its partner, transformed with its own parameters.
    Computed once, shared by the shapes below."""
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (NIMG, 784), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (NIMG,), dtype=torch.int32, generator=g)
    every = torch.arange(NIMG)
    expect = {}
    for ep in GATHER_EPOCHS:
        mixed, j, q = mix_batch(images, every, ep, MIX)
        assert (q < 256).any() and (j != np.arange(NIMG)).any() and j.max() < NIMG
        assert not torch.equal(mixed, images)
        for name, spec in SETTINGS.items():
            expect[(name, ep)] = augment_batch(mixed, every, ep, spec)
    assert torch.equal(expect[("identity", 0)], mix_batch(images, every, 0, MIX)[0])
    return images, labels, expect


def _gather_mixup(C, d_images, d_labels, d_idx, n, max_wgs, spec, ep, qt, mix=MIX, ntrain=NIMG):
    out_i = torch.full((n + 3, 784), 7, dtype=torch.uint8, device="cuda")
    out_l = torch.full((n + 3,), -1, dtype=torch.int32, device="cuda")
    ctr = torch.full((4,), 9, dtype=torch.int64, device="cuda")
    step = torch.full((1,), 5, dtype=torch.int64, device="cuda")
    cosq, sinq, invz = (_dev(t) for t in spec.tables())
    C.gather_epoch_mixup(d_images, d_labels, d_idx, out_i, out_l, ctr, step, 11, max_wgs, cosq,
                         sinq, invz, spec.shift, ep, spec.seed, spec.elastic_q, qt, ntrain,
                         mix.seed)
    torch.cuda.synchronize()
    assert int(ctr.abs().sum()) == 0 and int(step.item()) == 11
    assert bool((out_i[n:] == 7).all()) and bool((out_l[n:] == -1).all())
    return out_i[:n].cpu(), out_l[:n].cpu()


@pytest.mark.parametrize("n,max_wgs", [(1, 0), (15, 0), (16, 0), (17, 0), (63, 0), (64, 0), (65, 0),
                                       (130, 0), (130, 1)])
def test_gather_epoch_mixup_matches_oracle(gpu, source, n, max_wgs):
    """gather_epoch_mixup equals the oracle bit for bit (images) and plain indexing (labels): at
    less than a wave's 16 rows, exactly 16, one more, around one 64-row pass, and two passes and
    a ragged third (once on a one-workgroup grid that strides); nimg = 97, so n = 130 has
    duplicates; identity, shift + rotate + zoom and elastic transforms; epochs 0 and 3.  Nothing
    is written past row n and the counters are reset."""
    C = _C()
    images, labels, expect = source
    d_images, d_labels = images.cuda(), labels.cuda()
    idx = torch.randint(0, NIMG, (n,), dtype=torch.int32, generator=torch.Generator().manual_seed(n))
    il = idx.long()
    qt = _dev(MIX.table())
    for name, spec in SETTINGS.items():
        for ep in GATHER_EPOCHS:
            got, lab = _gather_mixup(C, d_images, d_labels, idx.cuda(), n, max_wgs, spec, ep, qt)
            want = expect[(name, ep)][il]
            assert torch.equal(got, want), (name, ep, int((got != want).any(1).sum()), "rows differ")
            assert torch.equal(lab, labels[il])
    assert not torch.equal(expect[("identity", 0)], expect[("identity", EPOCH)])
    assert not torch.equal(expect[("identity", 0)], expect[("elastic", 0)])


@pytest.mark.parametrize("n,max_wgs", [(65, 0), (130, 1)])
def test_gather_with_a_table_of_256_equals_the_elastic_gather(gpu, source, n, max_wgs):
    """QT == 256 everywhere: gather_epoch_elastic's output bit for bit ((256 a + 128) >> 8 = a),
    with all four ranges on."""
    C = _C()
    images, labels, _ = source
    d_images, d_labels = images.cuda(), labels.cuda()
    idx = torch.randint(0, NIMG, (n,), dtype=torch.int32,
                        generator=torch.Generator().manual_seed(n)).cuda()
    spec = AugmentSpec(2, 10.0, 0.1, seed=23, elastic=1.5)
    got, lab = _gather_mixup(C, d_images, d_labels, idx, n, max_wgs, spec, 2, _dev(ONES))
    out_i = torch.full((n, 784), 7, dtype=torch.uint8, device="cuda")
    out_l = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    cosq, sinq, invz = (_dev(t) for t in spec.tables())
    C.gather_epoch_elastic(d_images, d_labels, idx, out_i, out_l, None, None, 0, max_wgs, cosq, sinq,
                           invz, spec.shift, 2, spec.seed, spec.elastic_q)
    torch.cuda.synchronize()
    assert torch.equal(got, out_i.cpu()) and torch.equal(lab, out_l.cpu())
    mixed, _ = _gather_mixup(C, d_images, d_labels, idx, n, max_wgs, spec, 2, _dev(MIX.table()))
    assert not torch.equal(mixed, got)
    for bad in (0, NIMG + 1):
        with pytest.raises(RuntimeError, match="ntrain"):
            _gather_mixup(C, d_images, d_labels, idx, n, max_wgs, spec, 2, _dev(ONES), ntrain=bad)


# ---------------------------------------------------------------------------- the pairs

def _train_labels(seed=1):
    """The tagged labels of a 97-sample training set."""
    lab = torch.randint(0, 10, (NIMG,), generator=torch.Generator().manual_seed(seed))
    return lab, tag_labels(lab)


@pytest.mark.parametrize("B", [1, 5, 256])
def test_pairs_match_oracle(gpu, B):
    """mixup_pairs_rows == data/mixup.py's draw and the partners' labels, bit for bit (indices 0
    and 2^27 - 1 among them), for two seeds, tables and epochs."""
    C = _C()
    lab, tagged = _train_labels()
    idx = _indices(B, B)
    word = ((torch.arange(B) % 10) | (idx << 4)).to(torch.int32)
    for spec, e in ((MIX, EPOCH), (MixupSpec(2.0, seed=2 ** 64 - 1), 2 ** 31 - 1)):
        got = C.mixup_pairs_rows(word.to(gpu), _epoch_word(e, gpu), spec.seed, tagged.to(gpu), NIMG,
                                 _dev(spec.table()))
        torch.cuda.synchronize()
        j, q = draw(idx, e, spec, NIMG)
        assert got.dtype == torch.int32 and got.shape == (B, 3)
        want = torch.stack([torch.from_numpy(j), torch.from_numpy(q), lab[torch.from_numpy(j)]], 1)
        assert torch.equal(got.cpu().long(), want), (B, spec)
    # a smaller training set: the partners stay inside it
    got = C.mixup_pairs_rows(word.to(gpu), _epoch_word(1, gpu), MIX.seed, tagged.to(gpu), 7,
                             _dev(MIX.table())).cpu().long()
    j, q = draw(idx, 1, MIX, 7)
    assert torch.equal(got[:, 0], torch.from_numpy(j)) and int(got[:, 0].max()) < 7


# ---------------------------------------------------------------------------- the head

def reference(part, bf1, wf2, bf2, y, y2, lam, mult, e, dt):
    """The head with mixup (and dropout, label smoothing) in plain torch, every operation in
    dtype `dt`: t = lam t(y) + (1 - lam) t(y2), row loss = lam loss_E(y) + (1 - lam) loss_E(y2);
    y2 None: the single-label head."""
    part, bf1, wf2, bf2, mult = (t.to(dt) for t in (part, bf1, wf2, bf2, mult))
    B = part.shape[1]
    h = torch.relu(part.sum(0) + bf1)
    hd = h * mult
    lg = hd @ wf2.t() + bf2
    lse = torch.logsumexp(lg, 1)

    def target(yy):
        return (1.0 - e) * F.one_hot(yy.long(), NCLS).to(dt) + e / NCLS

    def rowloss(yy):
        return lse - ((1.0 - e) * lg.gather(1, yy.long()[:, None])[:, 0] + e * lg.mean(1))

    if y2 is None:
        t, rl = target(y), rowloss(y)
    else:
        lam = lam.to(dt)
        t = lam[:, None] * target(y) + (1.0 - lam[:, None]) * target(y2)
        rl = lam * rowloss(y) + (1.0 - lam) * rowloss(y2)
    dl = (torch.softmax(lg, 1) - t) / B
    dh = (dl @ wf2) * mult * (h > 0).to(dt)
    return dict(logits=lg, dh=dh, dWfc2=dl.t() @ hd, dbfc2=dl.sum(0), dbfc1=dh.sum(0),
                loss=rl.sum(), correct=int((lg.argmax(1) == y.long()).sum()))


@functools.lru_cache(maxsize=None)
def case(B, S, scale, e, p):
    """Inputs (labels tagged with dataset indices), the pairs and the mask from the NumPy
    oracles, the fp64 and fp32-torch references and the near-tie row count of one shape;
    computed once, never modified."""
    drop = DropoutSpec(p, DROP.seed)
    part, bf1, wf2, bf2, y = make_inputs(B, S, scale, 1000 * B + S)
    idx = _indices(B, 7 * B + S)
    lab, tagged = _train_labels()
    j, q = draw(idx, EPOCH, MIX, NIMG)
    y2 = lab[torch.from_numpy(j)].to(torch.int32)
    lam = torch.from_numpy(q).double() / 256.0
    mult = torch.from_numpy(keep_mask(idx, EPOCH, drop)).float() * drop.scale
    word = (y.long() | (idx << 4)).to(torch.int32)
    r64 = reference(part, bf1, wf2, bf2, y, y2, lam, mult, e, torch.float64)
    r32 = reference(part, bf1, wf2, bf2, y, y2, lam, mult, e, torch.float32)
    top2 = r64["logits"].topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())
    return (part, bf1, wf2, bf2, word), drop, tagged, (y, y2, lam, mult), r64, r32, near


def launch_mix(C, dev, inp, drop, tagged, e, bf16_mode, qt=None, epoch=EPOCH, sched=None,
               keep_guard=False):
    """test_gpu_cnn_head.launch_train for cnn_head_mixup: one launch into NaN-filled buffers ->
    dict of CPU results."""
    part, bf1, wf2, bf2, word = inp
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
    kw = {} if sched is None else {"lr_sched": sched}
    C.cnn_head_mixup(part.reshape(-1).to(dev), S, B, bf1.to(dev), wf2.reshape(-1).to(dev),
                     bf2.to(dev), word.to(dev), dh, dht, ldt, slab, metrics, c0, c1, None, dh32,
                     _epoch_word(epoch, dev), drop.seed, drop.T, drop.scale, tagged.to(dev),
                     tagged.numel(), _dev(MIX.table() if qt is None else qt, dev), MIX.seed,
                     label_smoothing=e, **kw)
    torch.cuda.synchronize()
    out = dict(slab=slab.cpu(), metrics=metrics.cpu(), c0=int(c0.item()), c1=int(c1.item()),
               nblk=nblk, ldt=ldt)
    for k, t in (("dh", dh), ("dht", dht), ("dh32", dh32)):
        if t is not None:
            out[k] = t.cpu()
    for k in ("slab", "dh", "dht", "dh32"):            # nothing written past the buffer
        if k in out:
            assert torch.isnan(out[k][-GUARD:].float()).all(), k
            if not keep_guard:
                out[k] = out[k][:-GUARD]
    return out


def _check_against(out32, r64, r32, B, near, what):
    ldt = out32["ldt"]
    dh32 = out32["dh32"].view(ldt, HID)
    got = slab_sums(out32)
    got["dh"] = dh32[:B]
    errs = {q: (relerr(torch.as_tensor(got[q]), r64[q]), relerr(torch.as_tensor(r32[q]), r64[q]))
            for q in QUANT}
    print(f"\n{what}: " + "  ".join(f"{q} {k:.1e}|{t:.1e}" for q, (k, t) in errs.items()) +
          f"  correct {got['correct']:.0f}/{r64['correct']} near {near}")
    for q, (k, t) in errs.items():
        assert k <= max(8 * t, 2e-6), (q, k, t)
    assert got["correct"] == int(got["correct"])
    assert abs(got["correct"] - r64["correct"]) <= near, (got["correct"], r64["correct"], near)


# test_gpu_cnn_head.py's shapes, each at scale 1 with and without label smoothing and dropout,
# and at its scale 40 with both on
@pytest.mark.parametrize("B,S,scale,e,p",
                         [(B, S, 1, e, p) for B, S in HEAD_SHAPES for e in (0.0, 0.1)
                          for p in (0.0, 0.5)] + [(B, S, 40, 0.1, 0.5) for B, S in HEAD_SHAPES])
def test_mixup_head_vs_fp64(gpu, B, S, scale, e, p):
    """dh32, the bf16 dh / dht copies in their fragment-major layouts, every slab column (dWfc2,
    dbfc2, dbfc1, the mixed loss, correct against y), the untouched train metrics and the
    counters, under test_gpu_cnn_head.py's rule: the kernel's relative-norm error against fp64
    at most 8 x that of the same model in fp32 torch, floor 2e-6."""
    C = _C()
    inp, drop, tagged, (y, y2, lam, mult), r64, r32, near = case(B, S, scale, e, p)
    assert near <= (0 if B <= 64 else B // 100), near            # from the reference alone
    f32 = launch_mix(C, gpu, inp, drop, tagged, e, False)
    b16 = launch_mix(C, gpu, inp, drop, tagged, e, True)
    for out in (f32, b16):
        check_common(out, B)
    ldt = f32["ldt"]
    dh32 = f32["dh32"].view(ldt, HID)
    assert torch.isfinite(dh32).all()
    assert (bits(dh32[B:]) == 0).all()                            # padding rows exactly zero
    assert (bits(dh32[:B])[mult == 0] == 0).all()                 # dropped units exactly zero
    check_bf16_layout(f32, b16, B)
    assert torch.equal(bits(f32["slab"]), bits(b16["slab"]))
    _check_against(f32, r64, r32, B, near, f"mixup head B={B} S={S} scale={scale} E={e} p={p}")
    if B > 1:
        # the partner's label matters: the single-label model is far away
        assert bool((y2 != y).any()) and bool((lam < 1).any())
        single = reference(*inp[:4], y, None, None, mult, e, torch.float64)
        assert relerr(slab_sums(f32)["dbfc2"], single["dbfc2"]) > 1e-2


@pytest.mark.parametrize("B,S", [(5, 32), (37, 32), (33, 48), (1030, 4)])
@pytest.mark.parametrize("e,p", [(0.0, 0.0), (0.1, 0.5)])
def test_table_of_256_equals_the_dropout_head(gpu, B, S, e, p):
    """QT == 256 everywhere (lambda = 1): every output of the mixup head has cnn_head_dropout's
    bits, whatever the partners' labels are."""
    C = _C()
    inp, drop, tagged, _, _, _, _ = case(B, S, 1, e, p)
    for bf16_mode in (False, True):
        a = _launch_drop_smooth(C, gpu, inp, drop, e, bf16_mode)
        b = launch_mix(C, gpu, inp, drop, tagged, e, bf16_mode, qt=ONES)
        for k in ("slab", "dh", "dht", "dh32"):
            assert (k in a) == (k in b)
            if k in a:
                assert torch.equal(bits(a[k]), bits(b[k])), (k, bf16_mode)
        assert torch.equal(a["metrics"], b["metrics"])
        assert (a["c0"], a["c1"], a["nblk"]) == (b["c0"], b["c1"], b["nblk"])
        c = launch_mix(C, gpu, inp, drop, tagged, e, bf16_mode)
        assert not torch.equal(bits(c["slab"]), bits(b["slab"]))      # the real table mixes


def _launch_drop_smooth(C, dev, inp, drop, e, bf16_mode):
    """test_gpu_dropout.launch_drop with the label smoothing passed on."""
    part, bf1, wf2, bf2, word = inp
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
    C.cnn_head_dropout(part.reshape(-1).to(dev), S, B, bf1.to(dev), wf2.reshape(-1).to(dev),
                       bf2.to(dev), word.to(dev), dh, dht, ldt, slab, metrics, c0, c1, None, dh32,
                       _epoch_word(EPOCH, dev), drop.seed, drop.T, drop.scale, label_smoothing=e)
    torch.cuda.synchronize()
    out = dict(slab=slab.cpu()[:-GUARD], metrics=metrics.cpu(), c0=int(c0.item()),
               c1=int(c1.item()), nblk=nblk, ldt=ldt)
    for k, t in (("dh", dh), ("dht", dht), ("dh32", dh32)):
        if t is not None:
            out[k] = t.cpu()[:-GUARD]
    return out


@pytest.mark.parametrize("B,S", [(37, 32), (33, 48)])
@pytest.mark.parametrize("e", [0.0, 0.1])
def test_equal_labels_give_the_single_label_loss(gpu, B, S, e):
    """Every training label (so every partner's) and every row's own label the same class:
    y2 == y in every row, and the outputs are the single-label head's, under the same rule."""
    C = _C()
    inp, drop, _, (_, _, _, mult), _, _, _ = case(B, S, 1, e, 0.5)
    part, bf1, wf2, bf2, word = inp
    y = torch.full((B,), 6, dtype=torch.int32)
    word = ((word >> 4 << 4) | 6).to(torch.int32)
    tagged = tag_labels(torch.full((NIMG,), 6))
    r64 = reference(part, bf1, wf2, bf2, y, None, None, mult, e, torch.float64)
    r32 = reference(part, bf1, wf2, bf2, y, None, None, mult, e, torch.float32)
    top2 = r64["logits"].topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())
    out = launch_mix(C, gpu, (part, bf1, wf2, bf2, word), drop, tagged, e, False)
    check_common(out, B)
    _check_against(out, r64, r32, B, near, f"mixup head, y2 == y, B={B} S={S} E={e}")


@pytest.mark.parametrize("B,S", [(1, 32), (37, 32)])
@pytest.mark.parametrize("bf16_mode", [False, True])
def test_head_schedule_moves_the_cursor_and_nothing_else(gpu, B, S, bf16_mode):
    """tests/test_gpu_lr_schedule.py's head test for cnn_head_mixup: three launches with a
    5-entry table and the cursor at 2 take table[2..4] and leave the cursor at 5; every other
    output, the guards behind the buffers included, has the bits of the launch without it."""
    C = _C()
    inp, drop, tagged, _, _, _, _ = case(B, S, 1, 0.1, 0.5)
    table_h = [0.5, 0.25, 0.125, 0.0625, 0.03125]
    plain = launch_mix(C, gpu, inp, drop, tagged, 0.1, bf16_mode, keep_guard=True)
    assert (plain["c0"], plain["c1"]) == (42, 8)
    table = torch.tensor(table_h, dtype=torch.float64, device=gpu)
    cursor = torch.tensor([2], dtype=torch.int64, device=gpu)
    lr = torch.tensor([-1.0], dtype=torch.float64, device=gpu)
    for call in range(3):
        got = launch_mix(C, gpu, inp, drop, tagged, 0.1, bf16_mode, sched=(table, cursor, lr),
                         keep_guard=True)
        assert lr.item() == table_h[2 + call] and cursor.item() == 3 + call
        assert got.keys() == plain.keys()
        for k in got:
            a, b = got[k], plain[k]
            if torch.is_tensor(a):
                a = a.view(torch.int64) if a.dtype == torch.float64 else bits(a)
                b = b.view(torch.int64) if b.dtype == torch.float64 else bits(b)
                assert torch.equal(a, b), k
            else:
                assert a == b, k
    assert table.cpu().tolist() == table_h


def test_head_argument_checks(gpu):
    C = _C()
    inp, drop, tagged, _, _, _, _ = case(5, 32, 1, 0.0, 0.0)
    with pytest.raises(RuntimeError, match="ntrain"):
        launch_mix(C, gpu, inp, drop, tagged[:0], 0.0, False)
    with pytest.raises(RuntimeError, match="qt"):
        launch_mix(C, gpu, inp, drop, tagged, 0.0, False, qt=ONES[:100])


# ---------------------------------------------------------------------------- the programs

def _mix_program(dtype, B, n, lr=0.0, graphs=False, seed=0, **kw):
    train = synthetic_split(n, True)
    test = synthetic_split(128, False)
    prog = build_local_program("cnn", dtype, "cuda", B, train, test, optimizer="sgd", lr=lr,
                               momentum=0.0 if lr == 0.0 else 0.9,
                               weight_decay=0.0 if lr == 0.0 else 1e-4, seed=seed,
                               use_graphs=graphs, mixup=MIX, **kw)
    prog.optimizer.sync_hyperparams()
    return prog, train


def _mixed_batch(train, sel, aug=None):
    """The oracle's batch: (normalised mixed images, y, y2, lambda)."""
    mixed, j, q = mix_batch(train.images, sel, EPOCH, MIX)
    if aug is not None:
        mixed = augment_batch(mixed, sel, EPOCH, aug)
    return mixed, train.labels[sel], train.labels[torch.from_numpy(j)], \
        torch.from_numpy(q).double() / 256.0


def _mixed_criterion(logits, y, y2, lam, e):
    return (lam * F.cross_entropy(logits, y, reduction="none", label_smoothing=e) +
            (1.0 - lam) * F.cross_entropy(logits, y2, reduction="none", label_smoothing=e)).mean()


def test_bf16_program_gradients_with_mixup(gpu):
    """One bf16 training step at B = 32 with mixup and dropout (gradients kept, as
    test_gpu_dropout.py arranges): the epoch buffer holds the oracle's mixed images bit for bit,
    and the gradients match fp64 autograd on them with the mixed criterion at that test's bounds
    against fp64 (5e-2, conv 1.2e-1; loss 2e-2)."""
    B = 32
    prog, train = _mix_program("bf16", B, 600, dropout=DROP)
    prog.gpu.keep_grads = True
    idx = distributed_indices(len(train), 1, 0, 0)
    with pytest.raises(ValueError, match="epoch"):
        prog.set_train_indices(idx)
    prog.set_train_indices(idx, epoch=EPOCH)
    tp = prog.arena.torch_tensors(prog.arena.params)
    prog.gpu.begin_epoch()
    prog.metrics.reset(0)
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    assert torch.equal(prog.gpu.ylab[:B].cpu(), tag_labels(train.labels)[sel])
    mixed, y, y2, lam = _mixed_batch(train, sel)
    assert torch.equal(prog.gpu.ep_images.view(-1, 784)[:B].cpu(), mixed)
    assert not torch.equal(mixed, train.images[sel]) and bool((y2 != y).any())
    x = normalize_reference(mixed)
    mult = torch.from_numpy(keep_mask(sel, EPOCH, DROP)).float() * DROP.scale
    got = prog.arena.torch_tensors(prog.arena.grads)
    leaves = {k: v.double().requires_grad_() for k, v in tp.items()}
    logits = functional_forward("cnn", leaves, x.double(), mult.double())
    loss = _mixed_criterion(logits, y, y2, lam, 0.0)
    loss.backward()
    for name, leaf in leaves.items():
        r = rel(got[name].double(), leaf.grad)
        print(f"bf16 mixup step vs fp64 {name}: {r:.2e}")
        assert r < (1.2e-1 if name.startswith("conv") else 5e-2), (name, r)
    mt = prog.metrics.buf[0:3].cpu()
    print(f"bf16 mixup step loss {mt[0].item() / B} vs {loss.item()}")
    assert abs(mt[0].item() / B - loss.item()) < 2e-2 * max(1.0, loss.item())
    assert mt[2].item() == B
    # with the single-label criterion the fc2 bias gradient is somewhere else
    plain = {k: v.double().requires_grad_() for k, v in tp.items()}
    F.cross_entropy(functional_forward("cnn", plain, x.double(), mult.double()), y).backward()
    assert rel(got["fc2.bias"].double(), plain["fc2.bias"].grad) > 0.05


@pytest.mark.parametrize("conv,e,drop", [("exact", 0.1, DROP), ("x3", 0.0, None)])
def test_f32_program_gradients_with_mixup(gpu, conv, e, drop):
    """One fp32 training step at B = 32 with mixup (exact products: with label smoothing,
    dropout and an elastic + affine transform alongside): against fp64 autograd on the
    oracle-mixed images with the mixed criterion (max-pool and, in split-bf16 mode, conv1's ReLU
    routed as the kernels routed them, as test_gpu_dropout.py does), at its 1e-4."""
    B = 32
    aug = AugmentSpec(1, 10.0, 0.1, seed=4, elastic=1.5) if conv == "exact" else None
    prog, train = _mix_program("fp32", B, 300, dropout=drop, label_smoothing=e, augment=aug)
    prog.gpu.conv_x3 = conv == "x3"
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx, epoch=EPOCH)
    prog.gpu.begin_epoch()
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    mixed, y, y2, lam = _mixed_batch(train, sel, aug)
    assert torch.equal(prog.gpu.ep_images.view(-1, 784)[:B].cpu(), mixed)
    x = normalize_reference(mixed).view(B, 1, 28, 28)
    mult = 1.0 if drop is None else torch.from_numpy(keep_mask(sel, EPOCH, drop)).double() * drop.scale
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
    out = net.fc2(F.relu(net.fc1(pooled.flatten(1))) * mult)
    loss = _mixed_criterion(out, y, y2, lam, e)
    loss.backward()
    got = prog.arena.torch_tensors(prog.arena.grads)
    for name, p in net.named_parameters():
        r = rel(got[name].double(), p.grad)
        print(f"fp32 ({conv}) mixup step vs fp64 {name}: {r:.2e}")
        assert r < 1e-4, (name, r)
    print(f"fp32 ({conv}) mixup step loss {prog.metrics.buf[0].item() / B} vs {loss.item()}")
    assert abs(prog.metrics.buf[0].item() - loss.item() * B) <= 1e-4 * B
    assert prog.metrics.buf[1].item() == (out.argmax(1) == y).sum().item()


def test_two_epochs_through_the_graphs(gpu):
    """bf16 CNN, 5 full batches of 64 and a tail of 40, epochs 0 and 1 with epoch 1 gathered
    ahead, dropout and a cosine schedule on: the graph path equals the eager one bit for bit;
    after each epoch its half of the epoch buffer holds the oracle's mixed images, and the other
    half the next epoch's once the ahead gather has completed; a run whose epoch word is held
    at 0 differs in epoch 1 (the head would mix the targets of other pairs than the gather)."""
    n = 64 * 5 + 40
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(3)]
    sched = ScheduleSpec("cosine", 0.02, 2, 6, warmup=3, lr_min=0.1)
    res = {}
    for name, graphs, hold in (("graphs", True, False), ("eager", False, False),
                               ("held", True, True)):
        prog, train = _mix_program("bf16", 64, n, lr=0.02, graphs=graphs, seed=7, dropout=DROP,
                                   schedule=sched)
        losses = []
        for e in range(2):
            prog.set_train_indices(order[e], order[e + 1], epoch=e)
            assert int(prog.gpu._epoch_dev.item()) == e
            if hold:
                prog.gpu._epoch_dev.zero_()
            tl, _ = prog.train_epoch()
            losses.append(tl.average)
            if name == "graphs":
                buf = prog.gpu.ep_images.view(2, n, 784)
                o = order[e].long()
                assert torch.equal(buf[e & 1].cpu(), mix_batch(train.images, o, e, MIX)[0]), e
                assert torch.equal(prog.gpu.ep_labels.view(2, n)[e & 1].cpu(),
                                   tag_labels(train.labels)[o])
            if e == 0:
                pend = prog.gpu._pending
                assert pend is not None and pend[2] is not None and pend[3] == 1
                if name == "graphs":
                    pend[2].synchronize()
                    o = order[1].long()
                    assert torch.equal(buf[1].cpu(), mix_batch(train.images, o, 1, MIX)[0])
        torch.cuda.synchronize()
        assert prog.gpu.use_graphs == graphs and bool(prog.gpu.graphs) == graphs
        res[name] = (prog.arena.params.clone(), losses)
    assert torch.equal(res["graphs"][0], res["eager"][0]) and res["graphs"][1] == res["eager"][1]
    assert res["held"][1][0] == res["graphs"][1][0]               # epoch 0 is epoch 0 either way
    assert not torch.equal(res["held"][0], res["graphs"][0])


def test_default_path_holds_no_mixup_state(gpu):
    """Without mixup the program holds no table, no tagged labels and no epoch word."""
    train, test = synthetic_split(128, True), synthetic_split(64, False)
    p = build_local_program("cnn", "bf16", "cuda", 64, train, test, use_graphs=False)
    assert p.mixup is None and p.gpu.mixup is None and p.gpu._mix_table is None
    assert p.gpu._epoch_dev is None and p.gpu._aug_tables is None
    assert torch.equal(p.gpu.train_labels.cpu(), train.labels.to(torch.int32))


# ---------------------------------------------------------------------------- CLI

def test_cnn_fp32_cli_gpu_matches_cpu_with_mixup(gpu, tmp_path, monkeypatch):
    """tests/test_gpu_dropout.py's GPU-vs-CPU CLI comparison with --mixup 0.4 (and label
    smoothing), at that test's tolerances for the exact fp32 products (loss 5e-5, accuracy 0.1,
    both epochs): the gather and the head on the GPU, and the CPU path's blend and criterion,
    mix the same pairs.  2000 samples, as tests/test_gpu_lr_schedule.py's comparison: one sample
    is 0.05 points of accuracy.

    --lr 0.01, not those tests' 0.05: with mixed targets the run at 0.05 is in a regime where
    the CPU path does not reproduce itself at the bound -- its test loss rises from 1.56 to 2.05
    in the second epoch, and a relative perturbation of 1e-7 of its initial weights (half an
    fp32 ulp) moves its second epoch's train loss by 1.5e-5 and test loss by 1.4e-4 (the GPU run
    differed from it by 1.0e-5 and 1.4e-4 there, by 1e-6 in the first epoch).  At 0.01 the same
    perturbation moves the CPU path's numbers by at most 6.2e-7."""
    monkeypatch.setenv("PDM_F32_CONV", "exact")
    d1, d2 = tmp_path / "gpu", tmp_path / "cpu"
    d1.mkdir()
    d2.mkdir()
    common = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.01", "--dtype", "fp32",
              "--synthetic-size", "2000", "--epochs", "2", "--seed", "4", "--mixup", "0.4",
              "--label-smoothing", "0.1"]
    g = [l for l in cli(common, d1) if l.startswith("Epoch:")]
    c = [l for l in cli(common, d2, device="cpu", backend="gloo") if l.startswith("Epoch:")]
    assert len(g) == len(c) == 2
    for lg, lc in zip(g, c):
        print(lg, "|", lc)
        mg, mc = EPOCH_RE.match(lg), EPOCH_RE.match(lc)
        for i in (3, 5):
            assert abs(float(mg.group(i)) - float(mc.group(i))) < 5e-5, (lg, lc)
        for i in (4, 6):
            assert abs(float(mg.group(i)) - float(mc.group(i))) <= 0.1, (lg, lc)
