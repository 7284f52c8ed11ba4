"""The two-hidden-layer MLP (--arch mlp2, csrc/kernels/mlp_hid.hip) on the GPU.  Kernel measure, as
tests/test_gpu_mlp.py: s = the sum of the magnitudes of an output's terms in fp64, e = max |got -
ref| / s, bound 2 K 2^-24 with K the fp32 roundings on the output's path (the worst case of K
single-rounded operations in any order, doubled: the MFMA's internal order is not documented).
Outputs are sentinel-filled and over-allocated; padding rows of the inputs are NaN."""
import pytest
import torch
import torch.nn.functional as F

import pytorch_distributed_mnist_amd.runtime.gpu_step as gpu_step
from test_gpu_app import EPOCH_RE, cli
from pytorch_distributed_mnist_amd.data.dropout import DropoutSpec, keep_mask
from pytorch_distributed_mnist_amd.data.mixup import MixupSpec
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.models.reference import functional_forward
from pytorch_distributed_mnist_amd.optim.ema import EmaSpec
from pytorch_distributed_mnist_amd.optim.schedule import ScheduleSpec
from pytorch_distributed_mnist_amd.ops import _ext
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

pytestmark = pytest.mark.gpu
D = torch.float64
HID, K1, GUARD, SENT = 128, 784, 256, -7.0
U24 = 2.0 ** -24
DROP = DropoutSpec(0.2, seed=(9 << 32) + 41)
rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()   # noqa: E731


def measure(tag, got, ref, s, nround):
    """max |got - ref| / s against 2 nround 2^-24; an output without terms is exactly zero."""
    assert torch.isfinite(got).all() and (got[s == 0] == 0).all(), tag
    e = ((got.to(D) - ref).abs()[s > 0] / s[s > 0]).max().item() if (s > 0).any() else 0.0
    print(f"{tag}: e = {e:.2e} (bound {2 * nround * U24:.2e})")
    assert e <= 2 * nround * U24, (tag, e)


def sentinel(n):
    return torch.full((n + GUARD,), SENT, dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("S", [1, 5, 25])
@pytest.mark.parametrize("B", [1, 16, 17, 33])
def test_mlp_hid_fwd(gpu, B, S):
    """h1 = relu(b1 + sum_s part[s]) and pre2 = h1 . W2^T at both workgroup splits; nothing is
    written behind [B][128]."""
    g = torch.Generator().manual_seed(100 * B + S)
    part = torch.randn(S, B, HID, generator=g)          # zero mean: about half the units off
    b1, w2 = torch.randn(HID, generator=g) * 0.1, torch.randn(HID, HID, generator=g) * 0.1
    sh = b1.to(D).abs() + part.to(D).abs().sum(0)
    h_ref = (b1.to(D) + part.to(D).sum(0)).clamp_min(0)
    for ngroups in (1, 2):
        h1, pre2 = sentinel(B * HID), sentinel(B * HID)
        _ext.require().mlp_hid_fwd(part.to(gpu), S, B, b1.to(gpu), w2.to(gpu), h1, pre2,
                                   ngroups=ngroups)
        h1, pre2 = h1.cpu(), pre2.cpu()
        assert (h1[B * HID:] == SENT).all() and (pre2[B * HID:] == SENT).all()
        measure(f"mlp_hid_fwd h1 B={B} S={S} g={ngroups}", h1[:B * HID].view(B, HID), h_ref, sh, S + 1)
        measure(f"mlp_hid_fwd pre2 B={B} S={S} g={ngroups}", pre2[:B * HID].view(B, HID),
                h_ref @ w2.to(D).t(), sh @ w2.to(D).abs().t(), HID + S + 1)


@pytest.mark.parametrize("B", [1, 16, 17, 33, "round + 1"])
def test_mlp_hid_bwd(gpu, B):
    """dh1 and dW2 with NaN in the padding rows of both inputs (the last case: one row more than
    a round of the dW2 role); a second launch's bits."""
    B = _ext.require().MLP_HID_ROUND + 1 if B == "round + 1" else B
    ldt = -(-B // 32) * 32
    g = torch.Generator().manual_seed(B)
    h1 = torch.full((ldt, HID), float("nan"))
    dh = torch.full((ldt, HID), float("nan"))
    h1[:B] = torch.randn(B, HID, generator=g).clamp_min(0)
    dh[:B] = torch.randn(B, HID, generator=g) * 0.01
    w2 = torch.randn(HID, HID, generator=g) * 0.1
    runs = []
    for _ in range(2):
        dh1, gw2 = sentinel(ldt * HID), sentinel(HID * HID)
        _ext.require().mlp_hid_bwd(dh.to(gpu), h1.to(gpu), w2.to(gpu), B, dh1, gw2[:HID * HID])
        runs.append((dh1.cpu(), gw2.cpu()))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))
    dh1, gw2 = runs[0]
    assert (dh1[ldt * HID:] == SENT).all() and (gw2[HID * HID:] == SENT).all()
    pad = dh1[B * HID:ldt * HID]
    assert ((pad == SENT) | (pad == 0)).all()            # rows >= B: not written, or zero
    a, x, w = dh[:B].to(D), h1[:B].to(D), w2.to(D)
    measure(f"mlp_hid_bwd dW2 B={B}", gw2[:HID * HID].view(HID, HID), a.t() @ x, a.abs().t() @ x.abs(), B)
    on = (x > 0).to(D)
    measure(f"mlp_hid_bwd dh1 B={B}", dh1[:B * HID].view(B, HID), (a @ w) * on, (a.abs() @ w.abs()) * on, HID)


@pytest.mark.parametrize("B", [1, 129])
def test_mlp_bwd_column_sums(gpu, B):
    """mlp_bwd's optional output = the column sums of dh; gw1's bits do not depend on it."""
    C = _ext.require()
    ldt = -(-B // 32) * 32
    g = torch.Generator().manual_seed(B)
    dh = torch.zeros(ldt, HID)
    dh[:B] = torch.randn(B, HID, generator=g) * 0.01
    x = torch.randint(0, 256, (B, K1), generator=g, dtype=torch.uint8).to(gpu)
    slab = torch.randn(C.cnn_head_nblk(ldt) * C.CNN_HEAD_SLAB, generator=g).to(gpu)
    gw1 = []
    for cs in (None, sentinel(HID)):
        outs = [torch.zeros(n, device=gpu) for n in (HID * K1, 1280, 10, HID)]
        C.mlp_bwd(x, None, B, B, dh.reshape(-1).to(gpu), ldt, *outs[:1], slab, *outs[1:],
                  torch.zeros(3, dtype=D, device=gpu), dh_colsum=None if cs is None else cs[:HID])
        gw1.append(outs[0].cpu())
    assert torch.equal(gw1[0].view(torch.int32), gw1[1].view(torch.int32))
    cs = cs.cpu()
    assert (cs[HID:] == SENT).all()
    measure(f"mlp_bwd colsum B={B}", cs[:HID], dh.to(D).sum(0), dh.to(D).abs().sum(0), B)


def _program(B, n, optimizer="sgd", lr=0.0, graphs=False, seed=0, **kw):
    train, test = synthetic_split(n, True), synthetic_split(2085, False)
    prog = build_local_program("mlp2", "fp32", "cuda", B, train, test, optimizer=optimizer, lr=lr,
                               momentum=0.9, weight_decay=1e-4, seed=seed, use_graphs=graphs, **kw)
    prog.optimizer.sync_hyperparams()
    return prog, train, test


@pytest.mark.parametrize("recipe", ["plain", "dropout+smoothing"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("B", [5, 256])
def test_one_training_step_vs_fp64_autograd(gpu, B, optimizer, recipe):
    """The six gradients and the updated weights, per parameter <= 1e-4 relative to fp64 autograd
    of functional_forward("mlp2") and torch's optimizer on it (tests/test_gpu_mlp.py's rule),
    with the oracle's mask and torch's smoothed criterion in the second recipe."""
    kw, E = ({}, 0.0) if recipe == "plain" else (dict(dropout=DROP, label_smoothing=0.1), 0.1)
    lr = 0.05 if optimizer == "sgd" else 1e-3
    prog, train, _ = _program(B, max(2 * B, 300), optimizer, lr, **kw)
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx, epoch=3)
    leaves = {k: v.to(D).requires_grad_()
              for k, v in prog.arena.torch_tensors(prog.arena.params).items()}
    prog.gpu.begin_epoch()
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    mult = None if not kw else torch.from_numpy(keep_mask(sel, 3, DROP)).to(D) * DROP.scale
    out = functional_forward("mlp2", leaves, normalize_reference(train.images[sel]).to(D), mult)
    loss = F.cross_entropy(out, train.labels[sel], label_smoothing=E)
    loss.backward()
    opt = (torch.optim.SGD(leaves.values(), lr, momentum=0.9, weight_decay=1e-4)
           if optimizer == "sgd" else torch.optim.Adam(leaves.values(), lr))
    got = prog.arena.torch_tensors(prog.arena.grads)
    assert len(leaves) == 6
    for name, leaf in leaves.items():
        r = rel(got[name].to(D), leaf.grad)
        print(f"mlp2 step B={B} {optimizer} {recipe} grad {name}: {r:.2e}")
        assert r < 1e-4, (name, r)
    opt.step()
    new = prog.arena.torch_tensors(prog.arena.params)
    for name, leaf in leaves.items():
        r = rel(new[name].to(D), leaf.detach())
        print(f"mlp2 step B={B} {optimizer} {recipe} weight {name}: {r:.2e}")
        assert r < 1e-4, (name, r)
    assert abs(prog.metrics.buf[0].item() - loss.item() * B) <= 1e-4 * B
    assert prog.metrics.buf[2].item() == B


def test_graphs_equal_eager(gpu):
    """5 full batches of 64 and a tail of 40, two epochs with epoch 1 gathered ahead, mixup and
    a cosine schedule on: graphs = eager, bit for bit."""
    n = 64 * 5 + 40
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(3)]
    sched = ScheduleSpec("cosine", 0.02, 2, 6, warmup=3, lr_min=0.1)
    res = {}
    for graphs in (True, False):
        prog, _, _ = _program(64, n, lr=0.02, graphs=graphs, seed=7, schedule=sched,
                              mixup=MixupSpec(0.4, seed=(5 << 32) + 19))
        losses = []
        for e in range(2):
            prog.set_train_indices(order[e], order[e + 1], epoch=e)
            losses.append(prog.train_epoch()[0].average)
        torch.cuda.synchronize()
        assert bool(prog.gpu.graphs) == graphs
        res[graphs] = (prog.arena.params.clone(), losses)
    assert torch.equal(res[True][0], res[False][0]) and res[True][1] == res[False][1]


@pytest.mark.parametrize("ema", [None, EmaSpec(0.9)])
def test_evaluate_equals_the_sums_of_predict(gpu, monkeypatch, ema):
    """On weights three epochs old (with `ema`: the averaged ones, through weight_set) evaluate()
    equals the sums of predict() over the 2085 test images, which cross a chunk; predict() on 21
    images in chunks of 8 is within tests/test_gpu_predict.py's 1e-4 of an fp64 log-softmax."""
    prog, train, test = _program(64, 360, lr=0.05, seed=7, ema=ema)
    for e in range(3):                    # (18 steps: few rows are left near a tie)
        prog.set_train_indices(distributed_indices(360, 1, 0, e).to(torch.int32), epoch=e)
        prog.train_epoch()
    tl, ta = prog.evaluate()
    p = prog.predict()
    y = test.labels.to(torch.int64)
    nll = -p.log_probs.to(D).gather(1, y[:, None]).sum().item()
    top2 = p.log_probs.topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())      # (the two heads may split a tie)
    assert tl.count == len(y) and abs(nll - tl.sum) <= 1e-6 * tl.sum, (nll, tl.sum)
    assert near <= len(y) // 100 and abs(int(p.confusion.trace()) - ta.correct) <= near
    monkeypatch.setattr(gpu_step, "EVAL_CHUNK", 8)
    rows, hook = [], prog.gpu._eval_forward
    with monkeypatch.context() as m:
        m.setattr(prog.gpu, "_eval_forward", lambda *a: rows.append(a[2]) or hook(*a))
        q = prog.predict(test.images[:21], test.labels[:21])
    assert rows == [8, 8, 5]              # three forwards: the patched chunk size was the loop's
    arena = prog.arena if ema is None else prog.ema.arena
    tp = {k: v.to(D) for k, v in arena.torch_tensors(arena.params).items()}
    ref = F.log_softmax(functional_forward("mlp2", tp, normalize_reference(test.images[:21]).to(D)), 1)
    assert rel(q.log_probs.to(D), ref) < 1e-4
    assert q.confusion.sum().item() == 21 and int((q.pred != p.pred[:21]).sum()) <= near


def test_mlp2_cli_gpu_tracks_cpu(gpu, tmp_path):
    """--arch mlp2 on the GPU against --device cpu over two epochs, at the MLP CLI test's
    tolerances (tests/test_gpu_mlp.py: loss 2e-3, accuracy 0.5)."""
    common = ["--arch", "mlp2", "--optimizer", "sgd", "--lr", "0.05", "--synthetic-size", "2048",
              "--epochs", "2", "--seed", "4"]
    lines = []
    for name, kw in (("gpu", {}), ("cpu", dict(device="cpu", backend="gloo"))):
        (tmp_path / name).mkdir()
        lines.append([l for l in cli(common, tmp_path / name, **kw) if l.startswith("Epoch:")])
    assert len(lines[0]) == len(lines[1]) == 2
    for mg, mc in ((EPOCH_RE.match(a), EPOCH_RE.match(b)) for a, b in zip(*lines)):
        assert all(abs(float(mg.group(i)) - float(mc.group(i))) < 2e-3 for i in (3, 5)), lines
        assert all(abs(float(mg.group(i)) - float(mc.group(i))) <= 0.5 for i in (4, 6)), lines
