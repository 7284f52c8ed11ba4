"""The MLP program (--arch mlp, csrc/kernels/mlp.hip) on the GPU.  Kernel measure, as
tests/test_gpu_cnn_f32_kernels.py: s = sum |terms| in fp64 over both halves of the normalisation
fold (alpha sum |w| u8 + beta sum |w|), e = max |got - ref| / s, bound K 2^-24 + 2^-18 with K the
number of terms (2 x 784 forward, 2 B for dW1).  Outputs are NaN-filled and over-allocated.

Measured on MI355X, largest e over the image kinds (and splits) of a case | the bound:
    mlp_fwd  B = 1 .. 33, S = 1, 5, 25    2.3e-07 .. 3.2e-07 | 9.73e-05
    mlp_bwd  B = 1    1.32e-07 | 3.93e-06      mlp_bwd  B = 33   1.01e-07 | 7.75e-06
    mlp_bwd  B = 31   1.17e-07 | 7.51e-06      mlp_bwd  B = 129  1.06e-07 | 1.92e-05
    mlp_bwd  B = 32   8.14e-08 | 7.63e-06
(With dh in two bf16 planes mlp_bwd measured 5.21e-06 at B = 1, above the bound: two planes leave
2^-17 |dh|, which one row cannot average; the kernel splits dh three ways.)  One training step
against fp64 autograd: fc1.weight 2.3e-07 .. 4.8e-07, fc2.weight <= 2.7e-06 (bound 1e-4)."""
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
from pytorch_distributed_mnist_amd.optim.schedule import ScheduleSpec
from pytorch_distributed_mnist_amd.ops import _ext
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

pytestmark = pytest.mark.gpu
D = torch.float64
HID, K, SLAB, GUARD = 128, 784, 1420, 256
ALPHA, BETA = 1.0 / (255.0 * 0.3081), 0.1307 / 0.3081
U24, SPLIT = 2.0 ** -24, 2.0 ** -18
M0 = (5.0, 3.0, 11.0)
KINDS = ("random", "zeros", "full")
DROP = DropoutSpec(0.2, seed=(9 << 32) + 41)
rel = lambda a, b: ((a - b).norm() / b.norm().clamp_min(1e-30)).item()   # noqa: E731
nan_f32 = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")   # noqa: E731


def images(kind, n, g):
    if kind == "random":
        return torch.randint(0, 256, (n, K), generator=g, dtype=torch.uint8)
    return torch.full((n, K), 0 if kind == "zeros" else 255, dtype=torch.uint8)


def folded(tag, got, a, x, nterms):
    """got [n][m] against alpha a^T x - beta sum a (a [k][n], x [k][m] bytes) by the measure."""
    a, x = a.to(D), x.to(D)
    ref = ALPHA * a.t() @ x - BETA * a.sum(0)[:, None]
    s = ALPHA * a.abs().t() @ x + BETA * a.abs().sum(0)[:, None]
    assert torch.isfinite(got).all() and (got[s == 0] == 0).all(), tag
    e = ((got.to(D) - ref).abs()[s > 0] / s[s > 0]).max().item()
    print(f"{tag}: e = {e:.2e} (bound {nterms * U24 + SPLIT:.2e})")
    assert e <= nterms * U24 + SPLIT, (tag, e)


@pytest.fixture(scope="module")
def w1(gpu):
    """fc1's weight and its hi / lo planes on the device."""
    w = torch.randn(HID, K, generator=torch.Generator().manual_seed(1)) * 0.05
    hi = w.to(torch.bfloat16)
    return w, hi.to(gpu), (w - hi.float()).to(torch.bfloat16).to(gpu)


@pytest.mark.parametrize("S", [1, 5, 25])
@pytest.mark.parametrize("B", [1, 5, 16, 17, 33])
def test_mlp_fwd(gpu, w1, B, S):
    """The split-summed part [B][128] per image kind; ylab = the label words verbatim (plain,
    and tagged with a dataset index); nothing is written behind the contract."""
    g = torch.Generator().manual_seed(100 * B + S)
    for kind in KINDS:
        x = images(kind, B + 2, g)
        y = torch.randint(0, 10, (B + 2,), generator=g, dtype=torch.int32)
        if kind == "random":
            y |= torch.randint(0, 60000, (B + 2,), generator=g, dtype=torch.int32) << 4
        part = nan_f32(S * B * HID + GUARD)
        ylab = torch.full((B + GUARD,), -7, dtype=torch.int32, device=gpu)
        _ext.require().mlp_fwd(x.to(gpu), y.to(gpu), None, B, B, w1[1], w1[2], part, ylab, S)
        part, ylab = part.cpu(), ylab.cpu()
        assert torch.isnan(part[S * B * HID:]).all() and (ylab[B:] == -7).all()
        assert torch.equal(ylab[:B], y[:B])
        got = part[:S * B * HID].view(S, B, HID)
        assert torch.isfinite(got).all()
        folded(f"mlp_fwd B={B} S={S} {kind}", got.to(D).sum(0).t(), w1[0].t(), x[:B].t(), 2 * K)


def test_mlp_fwd_counter_mode(gpu, w1):
    """Epochs of 40 rows in steps of 16: steps 1 and 2 (the ragged tail of 8) of epoch 0 and
    step 0 of epoch 1 (the buffer's other half) give the bits of the flat mode on those rows."""
    g = torch.Generator().manual_seed(7)
    x = images("random", 80, g).to(gpu)
    y = torch.randint(0, 10, (80,), generator=g, dtype=torch.int32).to(gpu)
    for c, B, r0 in ((1, 16, 16), (2, 8, 32), (3, 16, 40)):
        out = []
        for ctr in (torch.tensor([c], dtype=torch.int64, device=gpu), None):
            part, ylab = nan_f32(5 * B * HID), torch.zeros(B, dtype=torch.int32, device=gpu)
            xs, ys = (x, y) if ctr is not None else (x[r0:r0 + B], y[r0:r0 + B])
            _ext.require().mlp_fwd(xs, ys, ctr, 16 if ctr is not None else B, B, w1[1], w1[2], part,
                                   ylab, 5, spe=3)
            out.append((part.cpu(), ylab.cpu()))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), c
        assert torch.equal(out[0][1], y[r0:r0 + B].cpu())


@pytest.mark.parametrize("B,ldt,nslab", [(1, 32, 1), (31, 32, 2), (32, 32, -1), (33, 64, -1),
                                         (129, 1024, -1)])
def test_mlp_bwd(gpu, B, ldt, nslab):
    """dW1 per image kind; the head-slab role at 1, 2, 8, 16 and 256 (the most) slabs with the
    pre-set metrics advanced; a second run's bits."""
    C = _ext.require()
    g = torch.Generator().manual_seed(B)
    dh = torch.zeros(ldt, HID)
    dh[:B] = torch.randn(B, HID, generator=g) * 0.01        # the head's contract: rows >= B zero
    hb = C.cnn_head_nblk(ldt) if nslab < 0 else nslab
    slab = torch.randn(hb, SLAB, generator=g)
    d_dh = torch.cat((dh.reshape(-1), torch.full((GUARD,), float("nan")))).to(gpu)
    sizes = (HID * K, 1280, 10, HID)
    for kind in KINDS:
        x = images(kind, B + 2, g)
        runs = []
        for _ in range(2):
            outs = [nan_f32(n + GUARD) for n in sizes]
            metrics = torch.tensor(M0, dtype=D, device=gpu)
            C.mlp_bwd(x.to(gpu), None, B, B, d_dh, ldt, outs[0][:HID * K], slab.reshape(-1).to(gpu),
                      outs[1][:1280], outs[2][:10], outs[3][:HID], metrics, head_blocks=nslab)
            runs.append([t.cpu() for t in outs] + [metrics.cpu()])
        assert all(torch.equal(a.view(torch.int64 if a.dtype == D else torch.int32),
                               b.view(torch.int64 if b.dtype == D else torch.int32))
                   for a, b in zip(*runs))
        for t, n in zip(runs[0], sizes):
            assert torch.isnan(t[n:]).all() and torch.isfinite(t[:n]).all()
        folded(f"mlp_bwd B={B} {kind}", runs[0][0][:HID * K].view(HID, K), dh[:B], x[:B], 2 * B)
        hs, sabs = slab.to(D).sum(0), slab.to(D).abs().sum(0)[:1418]
        got = torch.cat([t[:n] for t, n in zip(runs[0][1:4], sizes[1:])]).to(D)
        assert ((got - hs[:1418]).abs() <= hb * U24 * sabs).all()         # hb fp32 roundings
        m = runs[0][4]
        assert abs(m[0] - M0[0] - hs[1418]) < 1e-9 * hb and abs(m[1] - M0[1] - hs[1419]) < 1e-9 * hb
        assert m[2] == M0[2] + B


def _program(B, n, optimizer="sgd", lr=0.0, graphs=False, seed=0, **kw):
    train, test = synthetic_split(n, True), synthetic_split(2085, False)
    prog = build_local_program("mlp", "fp32", "cuda", B, train, test, optimizer=optimizer, lr=lr,
                               momentum=0.9 * (lr != 0.0), weight_decay=1e-4 * (lr != 0.0),
                               seed=seed, use_graphs=graphs, **kw)
    prog.optimizer.sync_hyperparams()
    return prog, train, test


@pytest.mark.parametrize("recipe", ["plain", "dropout+smoothing"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("B", [5, 256])
def test_one_training_step_vs_fp64_autograd(gpu, B, optimizer, recipe):
    """lr = 0: the gradient arena holds the step's gradients; per parameter <= 1e-4 relative to
    fp64 autograd of functional_forward("mlp") (tests/test_gpu_cnn_f32.py's rule), with the
    oracle's mask and torch's smoothed criterion in the second recipe."""
    kw, E = ({}, 0.0) if recipe == "plain" else (dict(dropout=DROP, label_smoothing=0.1), 0.1)
    prog, train, _ = _program(B, max(2 * B, 300), optimizer, **kw)
    idx = distributed_indices(len(train), 1, 0, 0)
    prog.set_train_indices(idx, epoch=3)
    tp = prog.arena.torch_tensors(prog.arena.params)
    prog.gpu.begin_epoch()
    prog.gpu.train_step(B)
    torch.cuda.synchronize()
    sel = idx[:B]
    mult = None if not kw else torch.from_numpy(keep_mask(sel, 3, DROP)).to(D) * DROP.scale
    leaves = {k: v.to(D).requires_grad_() for k, v in tp.items()}
    out = functional_forward("mlp", leaves, normalize_reference(train.images[sel]).to(D), mult)
    loss = F.cross_entropy(out, train.labels[sel], label_smoothing=E)
    loss.backward()
    got = prog.arena.torch_tensors(prog.arena.grads)
    for name, leaf in leaves.items():
        r = rel(got[name].to(D), leaf.grad)
        print(f"mlp step B={B} {optimizer} {recipe} {name}: {r:.2e}")
        assert r < 1e-4, (name, r)
    assert abs(prog.metrics.buf[0].item() - loss.item() * B) <= 1e-4 * B
    assert prog.metrics.buf[2].item() == B


def test_graphs_equal_eager_and_predict(gpu, monkeypatch):
    """5 full batches of 64 and a tail of 40, two epochs with epoch 1 gathered ahead, mixup and
    a cosine schedule on: graphs = eager, bit for bit.  Then on the trained weights evaluate()
    equals the sums of predict() over the 2085 test images, and predict() on 21 images in
    chunks of 8 is within tests/test_gpu_predict.py's 1e-4 of an fp64 log-softmax."""
    n = 64 * 5 + 40
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(3)]
    sched = ScheduleSpec("cosine", 0.02, 2, 6, warmup=3, lr_min=0.1)
    res = {}
    for graphs in (True, False):
        prog, _, test = _program(64, n, lr=0.02, graphs=graphs, seed=7, schedule=sched,
                                 mixup=MixupSpec(0.4, seed=(5 << 32) + 19))
        losses = []
        for e in range(2):
            prog.set_train_indices(order[e], order[e + 1], epoch=e)
            losses.append(prog.train_epoch()[0].average)
        torch.cuda.synchronize()
        assert bool(prog.gpu.graphs) == graphs
        res[graphs] = (prog.arena.params.clone(), losses)
    assert torch.equal(res[True][0], res[False][0]) and res[True][1] == res[False][1]
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
    tp = {k: v.to(D) for k, v in prog.arena.torch_tensors(prog.arena.params).items()}
    ref = F.log_softmax(functional_forward("mlp", tp, normalize_reference(test.images[:21]).to(D)), 1)
    assert rel(q.log_probs.to(D), ref) < 1e-4
    assert q.confusion.sum().item() == 21 and int((q.pred != p.pred[:21]).sum()) <= near


def test_mlp_cli_gpu_tracks_cpu(gpu, tmp_path):
    """--arch mlp on the GPU against --device cpu over two epochs, at the split-bf16 fp32 CLI
    tolerances of tests/test_gpu_app.py (loss 2e-3, accuracy 0.5)."""
    common = ["--arch", "mlp", "--optimizer", "sgd", "--lr", "0.05", "--synthetic-size", "2048",
              "--epochs", "2", "--seed", "4"]
    lines = []
    for name, kw in (("gpu", {}), ("cpu", dict(device="cpu", backend="gloo"))):
        (tmp_path / name).mkdir()
        lines.append([l for l in cli(common, tmp_path / name, **kw) if l.startswith("Epoch:")])
    assert len(lines[0]) == len(lines[1]) == 2
    for mg, mc in ((EPOCH_RE.match(a), EPOCH_RE.match(b)) for a, b in zip(*lines)):
        assert all(abs(float(mg.group(i)) - float(mc.group(i))) < 2e-3 for i in (3, 5)), lines
        assert all(abs(float(mg.group(i)) - float(mc.group(i))) <= 0.5 for i in (4, 6)), lines
