"""Test-time augmentation on the GPU (--tta V; docs/kernels.md "Test-time augmentation"):
tta_reduce (csrc/kernels/tta.hip) alone against a float64 log-mean-exp at the bound of
tests/test_tta_cpu.py, with its pred / confusion / metrics outputs, its guard rows and its
unlabelled form; the views the TTA path feeds to predict() against the NumPy oracle bit for bit;
the three programs end to end against an oracle composed of the NumPy views, the program's own
one-view predict() and a float64 reduce; evaluate() against predict(); the weight average; a TTA
evaluation between two training epochs through the graphs; and the CLI against the CPU path."""
import math

import numpy as np
import pytest
import torch

from pytorch_distributed_mnist_amd.data.augment import AugmentSpec, augment_batch, tta_view
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.optim.ema import EmaSpec
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_gpu_app import EPOCH_RE, cli
from test_tta_cpu import AFFINE, ELASTIC, NC, first_argmax, make_views, reference, within_bound

pytestmark = pytest.mark.gpu

GUARD = 4                      # rows behind the n the kernel is asked for
PROGRAMS = [("cnn", "bf16"), ("cnn", "fp32"), ("linear", "fp32")]
IDS = ["cnn-bf16", "cnn-fp32", "linear"]


def _C():
    from pytorch_distributed_mnist_amd.ops import _ext
    return _ext.require()


# ---------------------------------------------------------------------------- tta_reduce alone

@pytest.fixture(scope="module")
def cases():
    """Per (V, n): the views and their float64 reference, computed once."""
    out = {}
    for V in (1, 2, 3, 32):
        for n in (1, 5, 63, 64, 65, 257):
            lp = make_views(V, n)
            out[(V, n)] = (lp, reference(lp))
    return out


def _labels(n):
    """Labels 0..9 over the rows, with (n > 2) one below and one above the range."""
    y = (torch.arange(n, dtype=torch.int32) * 7 + 3) % NC
    if n > 2:
        y[1], y[n - 1] = -1, NC
    return y


def _launch(lp, y, guard=GUARD):
    """tta_reduce over lp (host [V, n, 10]) with output buffers `guard` rows longer than n,
    pre-filled with a pattern; returns the host copies (logp, pred, confusion, metrics)."""
    V, n = lp.shape[0], lp.shape[1]
    dev = "cuda"
    logp = torch.full((n + guard, NC), -123.5, dtype=torch.float32, device=dev)
    pred = torch.full((n + guard,), -77, dtype=torch.int32, device=dev)
    conf = torch.full((NC, NC), 5, dtype=torch.int64, device=dev)
    met = torch.tensor([1.5, 2.0, 3.0], dtype=torch.float64, device=dev)
    labelled = y is not None
    _C().tta_reduce(lp.to(dev), y.to(dev) if labelled else None, logp, pred,
                    conf if labelled else None, met if labelled else None)
    torch.cuda.synchronize()
    return logp.cpu(), pred.cpu(), conf.cpu(), met.cpu()


@pytest.mark.parametrize("n", [1, 5, 63, 64, 65, 257])
@pytest.mark.parametrize("V", [1, 2, 3, 32])
def test_tta_reduce_vs_fp64(gpu, cases, V, n):
    lp, ref = cases[(V, n)]
    y = _labels(n)
    logp, pred, conf, met = _launch(lp, y)
    out = logp[:n]
    ok, worst = within_bound(out, ref)
    print(f"V={V} n={n}: worst error / bound = {worst:.3f}")
    assert ok, worst
    if V == 1:
        assert torch.equal(out.view(torch.int32), lp[0].view(torch.int32))
    # pred: the first maximum of the row as stored (rows 0 and 3 hold two equal maxima)
    assert torch.equal(pred[:n].to(torch.int64), first_argmax(out))
    assert torch.equal(pred[:n].to(torch.int64), out.argmax(dim=1))
    assert out[0, 2] == out[0, 7] and pred[0] == 2
    # rows >= n: untouched
    assert (logp[n:] == -123.5).all() and (pred[n:] == -77).all()
    # confusion: exact counts on top of what was there; labels outside 0..9 count nowhere
    inside = (y >= 0) & (y < NC)
    want = torch.bincount(y[inside].long() * NC + pred[:n][inside].long(), minlength=NC * NC)
    assert torch.equal(conf, want.view(NC, NC) + 5)
    assert int(conf.sum()) - 500 == int(inside.sum())
    # metrics: the fp64 sums of the stored values, on top of what was there
    yi = y[inside].long()
    loss = float((-out[inside].gather(1, yi[:, None])).to(torch.float64).sum())
    correct = int((pred[:n][inside].long() == yi).sum())
    assert abs((float(met[0]) - 1.5) - loss) <= 1e-12 * max(abs(loss), abs(float(met[0])))
    assert float(met[1]) - 2.0 == correct and float(met[2]) - 3.0 == n


@pytest.mark.parametrize("V,n", [(3, 65), (1, 5)])
def test_tta_reduce_without_labels(gpu, cases, V, n):
    lp, ref = cases[(V, n)]
    logp, pred, conf, met = _launch(lp, None)
    labelled = _launch(lp, _labels(n))
    assert torch.equal(logp, labelled[0]) and torch.equal(pred, labelled[1])
    assert (conf == 5).all() and met.tolist() == [1.5, 2.0, 3.0]


def test_tta_reduce_argument_checks(gpu):
    C = _C()
    dev = "cuda"
    lp = make_views(2, 5).to(dev)
    logp = torch.empty(5, NC, device=dev)
    pred = torch.empty(5, dtype=torch.int32, device=dev)
    y = torch.zeros(5, dtype=torch.int32, device=dev)
    conf = torch.zeros(NC, NC, dtype=torch.int64, device=dev)
    met = torch.zeros(3, dtype=torch.float64, device=dev)
    C.tta_reduce(lp, y, logp, pred, conf, met)
    for bad in (lambda: C.tta_reduce(lp[0], y, logp, pred),                       # not [V, n, 10]
                lambda: C.tta_reduce(lp[:, :, :9].contiguous(), y, logp, pred),
                lambda: C.tta_reduce(lp.double(), y, logp, pred),
                lambda: C.tta_reduce(lp.transpose(0, 1), y, logp, pred),          # strided
                lambda: C.tta_reduce(lp.repeat(17, 1, 1), y, logp, pred),         # 34 views
                lambda: C.tta_reduce(lp, y[:4], logp, pred),
                lambda: C.tta_reduce(lp, y.long(), logp, pred),
                lambda: C.tta_reduce(lp, y, logp[:4], pred),
                lambda: C.tta_reduce(lp, y, logp, pred[:4]),
                lambda: C.tta_reduce(lp, y, logp, pred.long()),
                lambda: C.tta_reduce(lp, None, logp, pred, conf),                 # needs labels
                lambda: C.tta_reduce(lp, None, logp, pred, None, met),
                lambda: C.tta_reduce(lp, y, logp, pred, conf[:5]),
                lambda: C.tta_reduce(lp, y, logp, pred, conf, met[:2])):
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------- the views

@pytest.fixture(scope="module")
def images():
    g = torch.Generator().manual_seed(4)
    return torch.randint(0, 256, (21, 784), dtype=torch.uint8, generator=g)


def _program(arch, dtype, spec=AFFINE, tta=1, n_test=64, graphs=False, **kw):
    train, test = synthetic_split(128, True), synthetic_split(n_test, False)
    p = build_local_program(arch, dtype, "cuda", 32, train, test, optimizer="sgd", lr=0.05,
                            seed=4, use_graphs=graphs, augment=spec, tta=tta, **kw)
    p.sync_fn = lambda what: torch.cuda.synchronize()
    return p


@pytest.mark.parametrize("spec", [AFFINE, ELASTIC], ids=["affine", "elastic"])
def test_views_match_the_oracle(gpu, images, spec):
    """20 rows in chunks of 7: what the step's view helper hands to predict() is the NumPy
    view of those rows, bit for bit, whichever chunk a row falls in."""
    step = _program("linear", "fp32", spec).gpu
    src = images[:20].to("cuda")
    for v in (0, 1, 2, 31):
        want = tta_view(images[:20], 0, 20, v, spec)
        if v:
            assert torch.equal(want, augment_batch(images[:20], torch.arange(20),
                                                   0x80000000 + v, spec))
        got = torch.cat([step.tta_view(src, s, min(7, 20 - s), v, spec).clone()
                         for s in range(0, 20, 7)])
        assert torch.equal(got.cpu(), want), v
        assert torch.equal(step.tta_view(src, 13, 1, v, spec).cpu(), want[13:14])
    with pytest.raises(ValueError):
        step.tta_view(src, 15, 7, 1, spec)
    with pytest.raises(ValueError):
        step.tta_view(src, 0, 7, 32, spec)


# ---------------------------------------------------------------------------- end to end

@pytest.mark.parametrize("arch,dtype", PROGRAMS, ids=IDS)
def test_predict_tta_vs_composed_oracle(gpu, images, arch, dtype):
    """N = 21, chunks of 8, V = 3: NumPy views -> the program's own one-view predict() ->
    float64 reduce.  The per-view rows are the TTA path's bit for bit, so only tta_reduce's
    arithmetic is compared, at its bound."""
    prog = _program(arch, dtype)
    y = torch.arange(21) % NC
    lv = torch.stack([prog.predict(tta_view(images, 0, 21, v, AFFINE), tta=1).log_probs
                      for v in range(3)])
    met = torch.zeros(3, dtype=torch.float64, device="cuda")
    logp, pred, conf = prog.gpu.predict_tta(images, y, None, AFFINE, 3, chunk=8, metrics=met)
    torch.cuda.synchronize()
    logp, pred = logp.cpu(), pred.cpu().long()
    # the three chunks' metric additions: the sums of the stored rows
    want = float((-logp.gather(1, y[:, None])).to(torch.float64).sum())
    assert abs(float(met[0]) - want) <= 1e-12 * abs(want)
    assert met[1:].tolist() == [float(pred.eq(y).sum()), 21.0]
    ok, worst = within_bound(logp, reference(lv))
    print(f"{arch}/{dtype}: worst error / bound = {worst:.3f}")
    assert ok, worst
    assert torch.equal(pred, first_argmax(logp))
    assert torch.equal(conf.cpu(), torch.bincount(y * NC + pred, minlength=100).view(NC, NC))
    # the public entry, the default chunk: the same rows
    got = prog.predict(images, y, tta=3)
    assert torch.equal(got.log_probs, logp) and torch.equal(got.pred, pred)
    assert torch.equal(got.confusion, conf.cpu())
    assert prog.predict(images, tta=3).confusion is None
    # one chunk, and a chunk of one row
    for chunk in (21, 1):
        assert torch.equal(prog.gpu.predict_tta(images, None, None, AFFINE, 3,
                                                chunk=chunk)[0].cpu(), logp)
    # V = 1 is the plain path
    assert torch.equal(prog.predict(images, tta=1).log_probs, lv[0])
    with pytest.raises(ValueError):
        prog.predict(images, tta=33)


@pytest.mark.parametrize("arch,dtype", PROGRAMS, ids=IDS)
def test_evaluate_is_the_sum_of_predict(gpu, arch, dtype):
    """2085 test images (past one 2048-row chunk of the CNN programs' predict()), V = 3."""
    prog = _program(arch, dtype, tta=3, n_test=2085)
    loss, acc = prog.evaluate()
    p = prog.predict()
    y = prog.test_split.labels.to(torch.int64)
    want = float((-p.log_probs.gather(1, y[:, None])).to(torch.float64).sum())
    print(f"{arch}/{dtype}: loss sum {loss.sum!r} vs {want!r}")
    assert loss.count == acc.count == 2085
    assert abs(loss.sum - want) <= 1e-12 * abs(want)
    assert acc.correct == int(p.confusion.trace()) == int(p.pred.eq(y).sum())
    assert int(p.confusion.sum()) == 2085
    # a second pass starts from zero, and the plain pass differs
    again = prog.evaluate()
    assert abs(again[0].sum - loss.sum) <= 1e-12 * abs(want) and again[1].correct == acc.correct
    prog.set_tta(1, AFFINE)
    assert prog.evaluate()[0].sum != loss.sum


@pytest.mark.parametrize("arch,dtype", PROGRAMS, ids=IDS)
def test_tta_between_epochs_uses_the_average_and_leaves_training_alone(gpu, images, arch, dtype):
    """Two epochs through the graphs with the weight average on, a TTA evaluation and
    prediction after the first: weights, optimizer state and average equal those of the run
    without --tta; the TTA passes read the averaged weights."""
    n = 128
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(3)]
    state = {}
    for tta in (1, 3):
        prog = _program(arch, dtype, tta=tta, graphs=True, ema=EmaSpec(0.9))
        prog.optimizer.sync_hyperparams()
        for e in range(2):
            prog.set_train_indices(order[e], order[e + 1], epoch=e)
            prog.train_epoch()
            if e == 0:
                ev = prog.evaluate()
                if tta > 1:
                    seen = prog.predict(images)
                    raw = prog.predict(images, average=False)
                    fresh = _program(arch, dtype, tta=3)
                    fresh.arena.load_state_dict(prog.ema.state_dict())
                    if hasattr(fresh.gpu, "refresh_shadows"):
                        fresh.gpu.refresh_shadows()
                    assert torch.equal(fresh.predict(images).log_probs, seen.log_probs)
                    assert not torch.equal(raw.log_probs, seen.log_probs)
                    fl, fa = fresh.evaluate()
                    assert abs(fl.sum - ev[0].sum) <= 1e-12 * abs(fl.sum)
                    assert fa.correct == ev[1].correct
        torch.cuda.synchronize()
        assert prog.gpu.use_graphs and prog.gpu.graphs
        state[tta] = [prog.arena.params.clone(), prog.ema.params.clone()] + \
            [b.clone() for b in prog.optimizer.state_buffers().values()]
    assert len(state[1]) == len(state[3]) >= 3
    for i, (a, b) in enumerate(zip(state[1], state[3])):
        assert torch.equal(a, b), i


# ---------------------------------------------------------------------------- CLI

def test_cnn_fp32_cli_gpu_matches_cpu_with_tta(gpu, tmp_path, monkeypatch):
    """tests/test_gpu_mixup.py's GPU-vs-CPU CLI comparison, its flags but for --tta 4 with shift
    and rotation in place of mixup and smoothing, at its tolerances for the exact fp32 products
    (loss 5e-5, accuracy 0.1, both epochs): the gathers and tta_reduce on the GPU and the CPU
    path's NumPy views and torch reduce draw the same views and combine them alike."""
    monkeypatch.setenv("PDM_F32_CONV", "exact")
    d1, d2 = tmp_path / "gpu", tmp_path / "cpu"
    d1.mkdir()
    d2.mkdir()
    common = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.01", "--dtype", "fp32",
              "--synthetic-size", "2000", "--epochs", "2", "--seed", "4", "--tta", "4",
              "--aug-shift", "2", "--aug-rotate", "10"]
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
