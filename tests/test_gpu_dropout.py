"""The dropout head (csrc/kernels/cnn_head_drop.hip) on the GPU: its mask against the NumPy
oracle (data/dropout.py keep_mask) bit for bit, the kernel called directly against an fp64 model
of the head that applies that mask (test_gpu_cnn_head.py's edge shapes, layouts and tolerances),
T = 0 against cnn_head bit for bit, exact zeros for dropped units, one training step of both CNN
programs against fp64 autograd with the same mask, two epochs through the graphs, and the CLI
against the CPU path."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_mnist_amd.data.dropout import DropoutSpec, keep_mask, tag_labels
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.models.reference import functional_forward
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_gpu_app import EPOCH_RE, cli
from test_gpu_cnn import _RoundFwd, _RoundGrad
from test_gpu_cnn import rel as rel32
from test_gpu_cnn_f32 import _kernel_a1_active, _reference_net, rel
from test_gpu_cnn_head import (GUARD, HID, M0, NCLS, QUANT, SLAB, _C, _ldt, bits, check_bf16_layout,
                               check_common, launch_train, make_inputs, nanbuf, relerr, slab_sums)

pytestmark = pytest.mark.gpu

EPOCH = 3
SPEC = DropoutSpec(0.5, seed=(9 << 32) + 41)
MAX_INDEX = (1 << 27) - 1
# B: one valid row; partial row groups; ldt = 64; more row groups (264) than workgroups (256).
# S: 32 (all partials at once), 1 and 17 (batches of 16 with selects, 17 = one whole + a partial)
SHAPES = [(1, 32), (3, 17), (5, 1), (5, 32), (33, 17), (33, 32), (1028, 17)]


def _epoch_word(e, dev):
    return torch.tensor([e], dtype=torch.int32, device=dev)


def _indices(B, seed):
    """B dataset indices below 2^27, the first 0 and the last 2^27 - 1."""
    idx = torch.randint(0, MAX_INDEX + 1, (B,), generator=torch.Generator().manual_seed(seed))
    idx[0] = 0
    idx[-1] = MAX_INDEX if B > 1 else 0
    return idx


@pytest.mark.parametrize("B", [1, 5, 256])
def test_mask_matches_oracle(gpu, B):
    """dropout_mask_rows == keep_mask bit for bit (indices 0 and 2^27 - 1 among them, every
    class in the label bits), for two thresholds, seeds and epochs."""
    C = _C()
    idx = _indices(B, B)
    if B == 1:
        idx[0] = MAX_INDEX
    lab = torch.arange(B) % 10
    word = (lab | (idx << 4)).to(torch.int32)
    assert int(word.min()) >= 0
    for spec, e in ((SPEC, EPOCH), (DropoutSpec(0.9, seed=7), 0), (DropoutSpec(0.25, seed=2 ** 64 - 1), 2 ** 31 - 1)):
        got = C.dropout_mask_rows(word.to(gpu), _epoch_word(e, gpu), spec.seed, spec.T)
        torch.cuda.synchronize()
        want = torch.from_numpy(keep_mask(idx, e, spec))
        assert got.dtype == torch.uint8 and got.shape == (B, HID)
        assert torch.equal(got.cpu(), want), (B, spec, int((got.cpu() != want).sum()))
        assert 0 < int(want.sum()) < want.numel()
    # index 0 with another label draws the same mask; another epoch does not
    a = C.dropout_mask_rows(torch.tensor([3], dtype=torch.int32, device=gpu), _epoch_word(1, gpu),
                            SPEC.seed, SPEC.T)
    b = C.dropout_mask_rows(torch.tensor([9], dtype=torch.int32, device=gpu), _epoch_word(1, gpu),
                            SPEC.seed, SPEC.T)
    c = C.dropout_mask_rows(torch.tensor([9], dtype=torch.int32, device=gpu), _epoch_word(2, gpu),
                            SPEC.seed, SPEC.T)
    assert torch.equal(a, b) and not torch.equal(b, c)


def reference(part, bf1, wf2, bf2, y, mult, dt):
    """The head with dropout in plain torch, every operation in dtype `dt`: mult [B, 128] is
    keep * scale (the fp32 scale the kernel multiplies by)."""
    part, bf1, wf2, bf2, mult = (t.to(dt) for t in (part, bf1, wf2, bf2, mult))
    B = part.shape[1]
    h = torch.relu(part.sum(0) + bf1)
    hd = h * mult
    lg = hd @ wf2.t() + bf2
    yl = y.long()
    onehot = F.one_hot(yl, NCLS).to(dt)
    rowloss = torch.logsumexp(lg, 1) - lg.gather(1, yl[:, None])[:, 0]
    dl = (torch.softmax(lg, 1) - onehot) / B
    dh = (dl @ wf2) * mult * (h > 0).to(dt)
    return dict(logits=lg, dh=dh, dWfc2=dl.t() @ hd, dbfc2=dl.sum(0), dbfc1=dh.sum(0),
                loss=rowloss.sum(), correct=int((lg.argmax(1) == yl).sum()))


@functools.lru_cache(maxsize=None)
def case(B, S, p):
    """Inputs (labels tagged with dataset indices), the NumPy mask, the fp64 and fp32-torch
    references and the near-tie row count of one shape; computed once, never modified."""
    spec = DropoutSpec(p, SPEC.seed)
    part, bf1, wf2, bf2, y = make_inputs(B, S, 1, 1000 * B + S)
    idx = _indices(B, 7 * B + S)
    keep = torch.from_numpy(keep_mask(idx, EPOCH, spec))
    mult = keep.float() * spec.scale
    # labels: every other row the masked fp64 model's argmax, the rest as drawn
    am = reference(part, bf1, wf2, bf2, y, mult, torch.float64)["logits"].argmax(1)
    y = torch.where(torch.arange(B) % 2 == 1, am.to(torch.int32), y)
    word = (y.long() | (idx << 4)).to(torch.int32)
    r64 = reference(part, bf1, wf2, bf2, y, mult, torch.float64)
    r32 = reference(part, bf1, wf2, bf2, y, mult, torch.float32)
    top2 = r64["logits"].topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())
    return (part, bf1, wf2, bf2, word), spec, keep, r64, r32, near


def launch_drop(C, dev, inp, spec, bf16_mode, epoch=EPOCH):
    """test_gpu_cnn_head.launch_train for cnn_head_dropout: one launch into NaN-filled
    buffers -> dict of CPU results."""
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
                       _epoch_word(epoch, dev), spec.seed, spec.T, spec.scale)
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


@pytest.mark.parametrize("B,S,p", [(B, S, 0.5) for B, S in SHAPES] + [(33, 32, 0.9)])
def test_dropout_head_vs_fp64(gpu, B, S, p):
    """dh32, the bf16 dh / dht copies in their fragment-major layouts, every slab column (dWfc2,
    dbfc2, dbfc1, loss, correct), the untouched train metrics and the counters, at
    test_gpu_cnn_head.py's bound: the kernel's relative-norm error against fp64 at most 8 x that
    of the same model in fp32 torch, floor 2e-6."""
    C = _C()
    inp, spec, keep, r64, r32, near = case(B, S, p)
    assert near <= (0 if B <= 64 else B // 100), near            # from the reference alone
    f32 = launch_drop(C, gpu, inp, spec, False)
    b16 = launch_drop(C, gpu, inp, spec, True)
    for out in (f32, b16):
        check_common(out, B)
    ldt = f32["ldt"]
    dh32 = f32["dh32"].view(ldt, HID)
    assert torch.isfinite(dh32).all()
    assert (bits(dh32[B:]) == 0).all()                            # padding rows exactly zero
    assert (bits(dh32[:B])[keep == 0] == 0).all()                 # dropped units exactly zero
    check_bf16_layout(f32, b16, B)
    assert torch.equal(bits(f32["slab"]), bits(b16["slab"]))
    got = slab_sums(f32)
    got["dh"] = dh32[:B]
    errs = {q: (relerr(torch.as_tensor(got[q]), r64[q]), relerr(torch.as_tensor(r32[q]), r64[q]))
            for q in QUANT}
    print(f"\ndropout head B={B} S={S} p={p}: " +
          "  ".join(f"{q} {k:.1e}|{t:.1e}" for q, (k, t) in errs.items()) +
          f"  correct {got['correct']:.0f}/{r64['correct']} near {near}")
    for q, (k, t) in errs.items():
        assert k <= max(8 * t, 2e-6), (q, k, t)
    assert got["correct"] == int(got["correct"])
    assert abs(got["correct"] - r64["correct"]) <= near, (got["correct"], r64["correct"], near)
    # the mask matters: the unmasked model is far away
    plain = reference(*inp[:4], inp[4] & 15, torch.ones(B, HID), torch.float64)
    assert relerr(dh32[:B], plain["dh"]) > 0.1


@pytest.mark.parametrize("B", [5, 256])
def test_threshold_zero_equals_cnn_head(gpu, B):
    """T = 0 (scale 1): every output of the dropout head has cnn_head's bits, whatever the
    dataset indices in the label words."""
    C = _C()
    part, bf1, wf2, bf2, y = make_inputs(B, 32, 1, 77 + B)
    word = (y.long() | (_indices(B, B) << 4)).to(torch.int32)
    off = DropoutSpec(0.0, seed=5)
    assert off.T == 0 and off.scale == 1.0
    for bf16_mode in (False, True):
        a = launch_train(C, gpu, (part, bf1, wf2, bf2, y), bf16_mode)
        b = launch_drop(C, gpu, (part, bf1, wf2, bf2, word), off, bf16_mode)
        for k in ("slab", "dh", "dht", "dh32"):
            assert (k in a) == (k in b)
            if k in a:
                assert torch.equal(bits(a[k]), bits(b[k])), (k, bf16_mode)
        assert torch.equal(a["metrics"], b["metrics"])
        assert (a["c0"], a["c1"], a["nblk"]) == (b["c0"], b["c1"], b["nblk"])


def test_dropped_units_are_exact_zeros(gpu):
    """A single-row batch at p = 0.5: a dropped unit's dh32 entry and its dWfc2 slab column are
    exactly 0 (the kept ones are not)."""
    C = _C()
    inp, spec, keep, r64, _, _ = case(1, 32, 0.5)
    out = launch_drop(C, gpu, inp, spec, False)
    dropped = keep[0] == 0
    assert 30 < int(dropped.sum()) < 98
    dh32 = out["dh32"].view(out["ldt"], HID)[0]
    dw = out["slab"].view(out["nblk"], SLAB)[:, :NCLS * HID].view(-1, NCLS, HID)
    assert (dh32[dropped] == 0).all() and (dw[:, :, dropped] == 0).all()
    active = (r64["dh"][0] != 0)
    assert bool((dh32[active] != 0).all()) and int(active.sum()) > 0
    assert bool((dw[0][:, ~dropped & (r64["dWfc2"] != 0).any(0)] != 0).all())
    assert (dw[1:] == 0).all()                                   # the padding groups' slabs


def _drop_program(dtype, B, n, spec, lr=0.0, graphs=False, seed=0):
    train = synthetic_split(n, True)
    test = synthetic_split(128, False)
    prog = build_local_program("cnn", dtype, "cuda", B, train, test, optimizer="sgd", lr=lr,
                               momentum=0.0 if lr == 0.0 else 0.9,
                               weight_decay=0.0 if lr == 0.0 else 1e-4, seed=seed,
                               use_graphs=graphs, dropout=spec)
    prog.optimizer.sync_hyperparams()
    return prog, train


def test_bf16_program_gradients_with_dropout(gpu):
    """One bf16 training step at B = 32 with dropout (gradients kept, as
    test_cnn_step_gradients_match_autograd arranges): against fp64 autograd with the NumPy
    mask at that test's bounds for plain autograd (5e-2, conv 1.2e-1), and against fp32
    autograd with the kernels' bf16 rounding points mirrored at its tight ones (3e-3, conv
    1e-2)."""
    B = 32
    prog, train = _drop_program("bf16", B, 600, SPEC)
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
    x = normalize_reference(train.images[sel])
    y = train.labels[sel]
    mult = torch.from_numpy(keep_mask(sel, EPOCH, SPEC)).float() * SPEC.scale
    got = prog.arena.torch_tensors(prog.arena.grads)
    leaves = {k: v.double().requires_grad_() for k, v in tp.items()}
    loss = F.cross_entropy(functional_forward("cnn", leaves, x.double(), mult.double()), y)
    loss.backward()
    for name, leaf in leaves.items():
        r = rel(got[name].double(), leaf.grad)
        print(f"bf16 dropout step vs fp64 {name}: {r:.2e}")
        assert r < (1.2e-1 if name.startswith("conv") else 5e-2), (name, r)
    fr, gr = _RoundFwd.apply, _RoundGrad.apply
    m = {k: v.clone().requires_grad_() for k, v in tp.items()}
    h = fr(x.reshape(B, 1, 28, 28))
    a1 = fr(F.relu(gr(F.conv2d(h, fr(m["conv1.weight"]), m["conv1.bias"]))))
    z2 = F.relu(F.conv2d(a1, fr(m["conv2.weight"]), m["conv2.bias"]))
    pool = gr(fr(F.max_pool2d(z2, 2)))
    h = F.relu(gr(F.linear(torch.flatten(pool, 1), fr(m["fc1.weight"]), m["fc1.bias"])))
    F.cross_entropy(F.linear(h * mult, m["fc2.weight"], m["fc2.bias"]), y).backward()
    for name, leaf in m.items():
        r = rel32(got[name], leaf.grad)
        print(f"bf16 dropout step vs mirrored {name}: {r:.2e}")
        assert r < (1e-2 if name.startswith("conv") else 3e-3), (name, r)
    mt = prog.metrics.buf[0:3].cpu()
    assert abs(mt[0].item() / B - loss.item()) < 2e-2 * max(1.0, loss.item())
    assert mt[2].item() == B
    # without the mask the fc2 gradient is somewhere else entirely
    plain = {k: v.double().requires_grad_() for k, v in tp.items()}
    F.cross_entropy(functional_forward("cnn", plain, x.double()), y).backward()
    assert rel(got["fc2.weight"].double(), plain["fc2.weight"].grad) > 0.2


@pytest.mark.parametrize("conv", ["exact", "x3"])
def test_f32_program_gradients_with_dropout(gpu, conv):
    """One fp32 training step at B = 32 with dropout: against fp64 autograd with the NumPy mask
    (max-pool and, in split-bf16 mode, conv1's ReLU routed as the kernels routed them, as
    test_f32_gradients_match_fp32_autograd does), at its 1e-4."""
    B = 32
    prog, train = _drop_program("fp32", B, 300, SPEC)
    prog.gpu.conv_x3 = conv == "x3"
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx, epoch=EPOCH)
    prog.gpu.begin_epoch()
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    x = normalize_reference(train.images[sel]).view(B, 1, 28, 28)
    y = train.labels[sel]
    mult = torch.from_numpy(keep_mask(sel, EPOCH, SPEC)).double() * SPEC.scale
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
    loss = F.cross_entropy(out, y)
    loss.backward()
    got = prog.arena.torch_tensors(prog.arena.grads)
    for name, p in net.named_parameters():
        r = rel(got[name].double(), p.grad)
        print(f"fp32 ({conv}) dropout step vs fp64 {name}: {r:.2e}")
        assert r < 1e-4, (name, r)
    assert abs(prog.metrics.buf[0].item() - loss.item() * B) <= 1e-4 * B
    assert prog.metrics.buf[1].item() == (out.argmax(1) == y).sum().item()


def test_two_epochs_through_the_graphs(gpu):
    """bf16 CNN, 5 full batches of 64 and a tail of 40, epochs 0 and 1 with epoch 1 gathered
    ahead: the graph path equals the eager one (--no-graphs) bit for bit, and differs from a
    run whose epoch word is held at 0 -- the head reads the epoch the program installed in
    stream order, behind epoch 0's steps and ahead of epoch 1's."""
    n = 64 * 5 + 40
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(3)]
    res = {}
    for name, graphs, hold in (("graphs", True, False), ("eager", False, False),
                               ("held", True, True)):
        prog, _ = _drop_program("bf16", 64, n, SPEC, lr=0.02, graphs=graphs, seed=7)
        losses = []
        for e in range(2):
            prog.set_train_indices(order[e], order[e + 1], epoch=e)
            assert int(prog.gpu._epoch_dev.item()) == e
            if hold:
                prog.gpu._epoch_dev.zero_()
            tl, _ = prog.train_epoch()
            losses.append(tl.average)
            if e == 0:
                pend = prog.gpu._pending
                assert pend is not None and pend[2] is not None and pend[3] == 1
        torch.cuda.synchronize()
        assert prog.gpu.use_graphs == graphs and bool(prog.gpu.graphs) == graphs
        res[name] = (prog.arena.params.clone(), losses)
    assert torch.equal(res["graphs"][0], res["eager"][0]) and res["graphs"][1] == res["eager"][1]
    assert res["held"][1][0] == res["graphs"][1][0]               # epoch 0 is epoch 0 either way
    assert not torch.equal(res["held"][0], res["graphs"][0])


@pytest.mark.parametrize("conv,loss_tol,acc_tol", [("exact", 5e-5, 0.1), ("x3", 2e-3, 0.5)])
def test_cnn_fp32_cli_gpu_matches_cpu_with_dropout(gpu, tmp_path, monkeypatch, conv, loss_tol,
                                                   acc_tol):
    """test_cnn_fp32_cli_train_resume_evaluate_matches_cpu's GPU-vs-CPU comparison with
    --dropout 0.5: the dropout head and the CPU path's multiplier draw the same masks, so that
    test's tolerances carry over (exact products: both epochs; split-bf16: the first)."""
    monkeypatch.setenv("PDM_F32_CONV", conv)
    d1, d2 = tmp_path / "gpu", tmp_path / "cpu"
    d1.mkdir()
    d2.mkdir()
    common = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.05", "--dtype", "fp32",
              "--synthetic-size", "1024", "--epochs", "2" if conv == "exact" else "1", "--seed", "4",
              "--dropout", "0.5"]
    g = [l for l in cli(common, d1) if l.startswith("Epoch:")]
    c = [l for l in cli(common, d2, device="cpu", backend="gloo") if l.startswith("Epoch:")]
    assert len(g) == len(c) == (2 if conv == "exact" else 1)
    for lg, lc in zip(g, c) if conv == "exact" else zip(g[:1], c[:1]):
        print(lg, "|", lc)
        mg, mc = EPOCH_RE.match(lg), EPOCH_RE.match(lc)
        for i in (3, 5):
            assert abs(float(mg.group(i)) - float(mc.group(i))) < loss_tol, (lg, lc)
        for i in (4, 6):
            assert abs(float(mg.group(i)) - float(mc.group(i))) <= acc_tol, (lg, lc)
