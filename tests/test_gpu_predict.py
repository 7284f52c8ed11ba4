"""The prediction heads (csrc/kernels/predict.hip) and everything above them on the GPU.

cnn_predict_head and lin_predict are called directly on synthetic inputs against an fp64
reference written in plain torch; then TrainProgram.predict end to end for the three GPU
programs, and the CLI's --predict-out.

cnn_predict_head runs on the inputs of tests/test_gpu_cnn_head.py (the same construction and
seeds, 1000 * B + S, copied here), at the shapes that reach each path of the kernel:

    B     S    reaches
    1     32   one valid row of the row group, the S == 32 path
    37    32   last row group has 1 valid row of 4
    64    16   exactly one 16-wide batch of partial loads
    40    2    clamp path (s0 + q >= S selects)
    40    1    no split
    33    48   three 16-wide batches
    1030  4    258 row groups on 256 workgroups (workgroups 0 and 1 take two groups)

each at scale 1 and at scale 40 (logits to about +-350).

Tolerances.  log_probs: the project's rule for the head (test_gpu_cnn_head.py): the same
reference is evaluated once more in fp32 torch on the CPU and the kernel's relative-norm error
against fp64 must stay below 8 x that fp32-torch error, floor 2e-6.  pred: may differ from the
fp64 argmax only on near-tie rows (fp64 top-2 logit gap below 1e-3), whose number `near` is
first bounded from the reference alone.  Counts are exact.  The end-to-end comparison against
the CPU oracle uses 1e-4 on the relative norm, the bound test_gpu_cnn_f32.py holds every tensor
of the fp32 program to (its split-bf16 conv2 / fc1 products carry 4.5e-6 per output) and the
rtol of test_gpu_linear.py's tensor comparisons.

Measured on MI355X, relative-norm error of log_probs against fp64, kernel | fp32 torch: between
5.6e-08|8.0e-08 and 1.5e-07|7.3e-08 over the fourteen cnn_predict_head cases, 7.3e-08|2.0e-07 to
9.4e-08|1.4e-07 for lin_predict; pred matched the fp64 argmax on every row (one near-tie row, at
B = 1030 scale 1).  End to end, sum(-log_probs[y]) and trace(confusion) equalled evaluate()'s
loss sum and correct count for all three programs (1, 2 and 1 near-tie rows of 2085); against
the CPU oracle log_probs were within 3.3e-07 (cnn fp32) and 1.2e-07 (linear), pred equal.
"""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, free_port
from pytorch_distributed_mnist_amd.data.mnist import MNIST_MEAN, MNIST_STD, normalize_reference, \
    synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.runtime.arena import FlatArena
from pytorch_distributed_mnist_amd.runtime.cpu_step import predict_step_cpu
from pytorch_distributed_mnist_amd.runtime.program import build_local_program
from pytorch_distributed_mnist_amd.utils.checkpoint import make_state, save_checkpoint

pytestmark = pytest.mark.gpu

HID, NCLS = 128, 10
SHAPES = [(1, 32), (37, 32), (64, 16), (40, 2), (40, 1), (33, 48), (1030, 4)]
M0 = (5.0, 3.0, 11.0)        # metrics pre-set
GUARD = 256                  # sentinel elements behind every output buffer: nothing is written there
PRED_FILL = -7               # int32 has no NaN: pred's guard (and unwritten rows) hold this


def _C():
    from pytorch_distributed_mnist_amd.ops import _ext
    return _ext.require()


def relerr(a, b):
    return ((a.double() - b).norm() / b.norm().clamp_min(1e-300)).item()


def bits(t):
    return t.view(torch.int32)


# ---- cnn_predict_head ---------------------------------------------------------------------

def head_logits(part, bf1, wf2, bf2, dt):
    """fc1 reduce + bias + ReLU, fc2 in plain torch, every operation in dtype `dt`."""
    part, bf1, wf2, bf2 = (t.to(dt) for t in (part, bf1, wf2, bf2))
    h = torch.relu(part.sum(0) + bf1)
    return h @ wf2.t() + bf2


def make_inputs(B, S, scale, seed):
    g = torch.Generator().manual_seed(seed)
    part = torch.randn(S, B, HID, generator=g) * (scale / math.sqrt(S))
    bf1 = torch.randn(HID, generator=g) * 0.5
    wf2 = torch.randn(NCLS, HID, generator=g) * 0.3
    bf2 = torch.randn(NCLS, generator=g) * 0.1
    # labels: every other row the fp64 reference's argmax, the rest random classes
    am = head_logits(part, bf1, wf2, bf2, torch.float64).argmax(1)
    rnd = torch.randint(0, NCLS, (B,), generator=g)
    y = torch.where(torch.arange(B) % 2 == 1, am, rnd).to(torch.int32)
    return part, bf1, wf2, bf2, y


def summarize(lg64, lg32, y):
    """fp64 / fp32-torch log-softmax of reference logits, the fp64 argmax, loss sum and correct
    count, and the number of near-tie rows."""
    lp64, lp32 = torch.log_softmax(lg64, 1), torch.log_softmax(lg32, 1)
    top2 = lg64.topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())
    am = lg64.argmax(1)
    yl = y.long()
    return dict(lp64=lp64, lp32=lp32, am=am, near=near,
                loss=-lp64.gather(1, yl[:, None]).sum().item(), correct=int((am == yl).sum()))


@functools.lru_cache(maxsize=None)
def case(B, S, scale):
    """Inputs and references of one (B, S, scale); computed once on the CPU, shared by the
    tests and never modified."""
    inp = make_inputs(B, S, scale, 1000 * B + S)
    ref = summarize(head_logits(*inp[:4], torch.float64), head_logits(*inp[:4], torch.float32),
                    inp[4])
    assert torch.isfinite(ref["lp64"]).all()
    return inp, ref


def guarded(n, dtype, dev, fill):
    return torch.full((n + GUARD,), fill, dtype=dtype, device=dev)


class Out:
    """Sentinel-filled output buffers with a guard behind each."""

    def __init__(self, B, dev, confusion=True, metrics=True):
        self.B = B
        self.logp = guarded(B * NCLS, torch.float32, dev, float("nan"))
        self.pred = guarded(B, torch.int32, dev, PRED_FILL)
        self.conf = guarded(NCLS * NCLS, torch.int64, dev, 0) if confusion else None
        if confusion:
            self.conf[NCLS * NCLS:] = PRED_FILL
        self.metrics = torch.tensor(M0, dtype=torch.float64, device=dev) if metrics else None

    def args(self):
        B = self.B
        return (self.logp[:B * NCLS], self.pred[:B],
                None if self.conf is None else self.conf[:NCLS * NCLS], self.metrics)

    def read(self):
        """CPU copies (logp [B, 10], pred [B], confusion [10, 10] | None, metrics | None) after
        checking the guards."""
        torch.cuda.synchronize()
        B = self.B
        logp, pred = self.logp.cpu(), self.pred.cpu()
        assert torch.isnan(logp[B * NCLS:]).all() and (pred[B:] == PRED_FILL).all()
        conf = None
        if self.conf is not None:
            conf = self.conf.cpu()
            assert (conf[NCLS * NCLS:] == PRED_FILL).all()
            conf = conf[:NCLS * NCLS].view(NCLS, NCLS)
        return (logp[:B * NCLS].view(B, NCLS), pred[:B], conf,
                None if self.metrics is None else self.metrics.cpu())


def launch_head(C, dev, inp, out, labelled=True):
    part, bf1, wf2, bf2, y = inp
    S, B = part.shape[0], part.shape[1]
    C.cnn_predict_head(part.reshape(-1).to(dev), S, B, bf1.to(dev), wf2.reshape(-1).to(dev),
                       bf2.to(dev), y.to(dev) if labelled else None, *out.args())


def check_rows(name, logp, pred, ref, y, cap):
    """log_probs and pred of one launch against the references (shared by both heads)."""
    near = ref["near"]
    assert near <= cap, near                                     # from the reference alone
    assert torch.isfinite(logp).all()                            # every row written
    k, t = relerr(logp, ref["lp64"]), relerr(ref["lp32"], ref["lp64"])
    wrong = int((pred.long() != ref["am"]).sum())
    print(f"\n{name}: logp {k:.1e}|{t:.1e}  pred off {wrong} near {near}")
    assert k <= max(8 * t, 2e-6), (k, t)
    assert ((pred >= 0) & (pred < NCLS)).all()
    assert wrong <= near, (wrong, near)
    # the kernel's own outputs agree with each other: pred attains the row's largest log_prob
    assert torch.equal(logp.gather(1, pred.long()[:, None])[:, 0], logp.max(1).values)


@pytest.mark.parametrize("scale", [1, 40])
@pytest.mark.parametrize("B,S", SHAPES)
def test_cnn_predict_head_vs_fp64(gpu, B, S, scale):
    C = _C()
    inp, ref = case(B, S, scale)
    y = inp[4]
    out = Out(B, gpu)
    launch_head(C, gpu, inp, out)
    logp, pred, conf, m = out.read()
    check_rows(f"cnn_predict_head B={B} S={S} scale={scale}", logp, pred, ref, y,
               0 if B <= 64 else B // 100)
    near = ref["near"]
    # confusion: the kernel's own (y, pred), exactly
    assert torch.equal(conf, torch.bincount(NCLS * y.long() + pred.long(),
                                            minlength=NCLS * NCLS).view(NCLS, NCLS))
    assert conf.sum().item() == B
    # metrics: the evaluation head's three additions
    want = ref["loss"] + M0[0]
    assert abs(m[0].item() - want) <= 1e-6 * want, (m[0].item(), want)
    assert m[2].item() == M0[2] + B
    me = torch.tensor(M0, dtype=torch.float64, device=gpu)
    C.cnn_head(inp[0].reshape(-1).to(gpu), S, B, inp[1].to(gpu), inp[2].reshape(-1).to(gpu),
               inp[3].to(gpu), y.to(gpu), False, None, None, 32, None, me, None, None)
    me = me.cpu()
    assert m[1].item() == int(m[1].item())
    assert abs(m[1].item() - me[1].item()) <= near, (m[1].item(), me[1].item(), near)
    assert m[1].item() - M0[1] == conf.trace().item()
    assert abs(m[0].item() - me[0].item()) <= 1e-12 * want      # the same row losses summed
    # a second launch into the same buffers: the same rows, the counts doubled
    launch_head(C, gpu, inp, out)
    logp2, pred2, conf2, m2 = out.read()
    assert torch.equal(bits(logp2), bits(logp)) and torch.equal(pred2, pred)
    assert torch.equal(conf2, 2 * conf)
    assert m2[2].item() == M0[2] + 2 * B
    # without labels: the same bits, no counts
    un = Out(B, gpu, confusion=False, metrics=False)
    launch_head(C, gpu, inp, un, labelled=False)
    logp3, pred3, _, _ = un.read()
    assert torch.equal(bits(logp3), bits(logp)) and torch.equal(pred3, pred)


def test_cnn_predict_head_takes_first_maximum(gpu):
    """wf2 = 0 and bf2 = [0.3, 0.3, 0, ...]: every row's logits are bf2, classes 0 and 1 tied at
    the top; the first wins, as torch.argmax."""
    C = _C()
    B, S = 8, 1
    part, bf1, _, _, _ = make_inputs(B, S, 1, 8001)
    wf2, bf2 = torch.zeros(NCLS, HID), torch.zeros(NCLS)
    bf2[:2] = 0.3
    y = torch.ones(B, dtype=torch.int32)
    out = Out(B, gpu)
    launch_head(C, gpu, (part, bf1, wf2, bf2, y), out)
    logp, pred, conf, m = out.read()
    assert (pred == 0).all()
    assert relerr(logp, torch.log_softmax(bf2.double(), 0).expand(B, NCLS)) <= 2e-6
    assert conf[1, 0].item() == B and conf.sum().item() == B
    assert m[1].item() == M0[1]


def test_predict_bindings_reject_bad_buffers(gpu):
    """Short or mistyped outputs, and counts without labels, raise before any launch."""
    C = _C()
    inp, _ = case(37, 32, 1)
    B = 37
    dev = gpu
    args = (inp[0].reshape(-1).to(dev), 32, B, inp[1].to(dev), inp[2].reshape(-1).to(dev),
            inp[3].to(dev))
    y = inp[4].to(dev)
    logp = torch.zeros(B * NCLS, device=dev)
    pred = torch.zeros(B, dtype=torch.int32, device=dev)
    conf = torch.zeros(NCLS, NCLS, dtype=torch.int64, device=dev)
    bad = [
        (y, logp[:-1], pred, None, None),                               # short logp
        (y, logp, pred[:-1], None, None),                               # short pred
        (y, logp, pred.long(), None, None),                             # pred dtype
        (y, logp.cpu(), pred, None, None),                              # host buffer
        (y, logp.view(B, NCLS).t(), pred, None, None),                  # not contiguous
        (y[:-1], logp, pred, None, None),                               # short labels
        (None, logp, pred, conf, None),                                 # counts without labels
        (y, logp, pred, conf.view(-1)[:99], None),                      # short confusion
        (y, logp, pred, conf.int(), None),                              # confusion dtype
    ]
    for tail in bad:
        with pytest.raises(RuntimeError):
            C.cnn_predict_head(*args, *tail)
    images = torch.zeros(17, 784, dtype=torch.uint8, device=dev)
    W, b = torch.zeros(10, 784, device=dev), torch.zeros(10, device=dev)
    for tail in [(None, W, b, logp[:169], pred[:17]), (None, W, b, logp[:170], pred[:16]),
                 (None, W, b, logp[:170], pred[:17], conf.view(-1))]:
        with pytest.raises(RuntimeError):
            C.lin_predict(images, *tail)
    torch.cuda.synchronize()
    assert (logp == 0).all() and (pred == 0).all() and (conf == 0).all()


# ---- lin_predict --------------------------------------------------------------------------

LIN_SEED = {1: 1, 17: 17, 16: 16, 33: 33}     # chosen on the CPU: no near-tie row (asserted)


@functools.lru_cache(maxsize=None)
def lin_case(N):
    g = torch.Generator().manual_seed(LIN_SEED[N])
    images = torch.randint(0, 256, (N, 784), generator=g, dtype=torch.uint8)
    W = torch.randn(10, 784, generator=g) * 0.05
    b = torch.randn(10, generator=g) * 0.1
    y = torch.randint(0, NCLS, (N,), generator=g).to(torch.int32)
    x64 = (images.double() / 255.0 - MNIST_MEAN) / MNIST_STD
    lg64 = x64 @ W.double().t() + b.double()
    lg32 = torch.nn.functional.linear(normalize_reference(images), W, b)
    return (images, W, b, y), summarize(lg64, lg32, y)


@pytest.mark.parametrize("N", [1, 17, 16, 33])
def test_lin_predict_vs_fp64(gpu, N):
    C = _C()
    (images, W, b, y), ref = lin_case(N)
    out = Out(N, gpu)
    C.lin_predict(images.to(gpu), y.to(gpu), W.to(gpu), b.to(gpu), *out.args())
    logp, pred, conf, m = out.read()
    check_rows(f"lin_predict N={N}", logp, pred, ref, y, 0)
    assert torch.equal(conf, torch.bincount(NCLS * y.long() + pred.long(),
                                            minlength=NCLS * NCLS).view(NCLS, NCLS))
    want = ref["loss"] + M0[0]
    assert abs(m[0].item() - want) <= 1e-6 * want, (m[0].item(), want)
    assert m[1].item() - M0[1] == conf.trace().item() == ref["correct"]
    assert m[2].item() == M0[2] + N
    me = torch.tensor(M0, dtype=torch.float64, device=gpu)
    C.lin_eval(images.to(gpu), y.to(gpu), W.to(gpu), b.to(gpu), me)
    me = me.cpu()                                                # lin_eval's additions
    assert abs(me[0].item() - m[0].item()) <= 1e-12 * want and torch.equal(me[1:], m[1:])
    un = Out(N, gpu, confusion=False, metrics=False)
    C.lin_predict(images.to(gpu), None, W.to(gpu), b.to(gpu), *un.args())
    logp3, pred3, _, _ = un.read()
    assert torch.equal(bits(logp3), bits(logp)) and torch.equal(pred3, pred)


# ---- end to end ---------------------------------------------------------------------------

N_E2E = 2048 + 37            # one chunk boundary and one partial row group


@pytest.mark.parametrize("arch,dtype", [("cnn", "bf16"), ("cnn", "fp32"), ("linear", "fp32")])
def test_program_predict_matches_evaluate(gpu, arch, dtype):
    """predict() on the test split after one short epoch (a trained model leaves few near-tie
    rows): its log_probs carry evaluate()'s loss, its confusion matrix evaluate()'s correct
    count, twice the same; the fp32 programs also against the CPU oracle."""
    train, test = synthetic_split(2048, True), synthetic_split(N_E2E, False)
    p = build_local_program(arch, dtype, "cuda", 256, train, test, optimizer="sgd", lr=0.05,
                            seed=11)
    p.optimizer.sync_hyperparams()
    p.set_train_indices(distributed_indices(len(train), 1, 0, 0))
    p.train_epoch()
    loss, acc = p.evaluate()
    before = p.metrics.buf.clone()
    a = p.predict()
    b = p.predict()
    assert torch.equal(p.metrics.buf, before)
    assert tuple(a.log_probs.shape) == (N_E2E, 10) and a.log_probs.dtype == torch.float32
    assert tuple(a.pred.shape) == (N_E2E,) and a.pred.dtype == torch.int64
    assert torch.equal(bits(a.log_probs), bits(b.log_probs))
    assert torch.equal(a.pred, b.pred) and torch.equal(a.confusion, b.confusion)
    y = test.labels
    nll = -a.log_probs.double().gather(1, y[:, None]).sum().item()
    top2 = a.log_probs.topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())
    print(f"\npredict {arch} {dtype}: nll {nll:.6f} | evaluate {loss.sum:.6f}  trace "
          f"{a.confusion.trace().item()} | correct {acc.correct}  near {near}")
    assert near <= N_E2E // 100, near
    assert abs(nll - loss.sum) <= 1e-6 * loss.sum, (nll, loss.sum)
    assert a.confusion.sum().item() == N_E2E
    assert torch.equal(a.confusion, torch.bincount(10 * y + a.pred, minlength=100).view(10, 10))
    assert abs(a.confusion.trace().item() - acc.correct) <= near
    # any N, without labels: the same rows (a 5-row chunk may run another fc1 split-K than a
    # 2048-row one: another fp32 summation order, held to the head rule's 2e-6 floor)
    un = p.predict(test.images[:5])
    assert un.confusion is None and tuple(un.pred.shape) == (5,)
    assert relerr(un.log_probs, a.log_probs[:5].double()) <= 2e-6
    if dtype == "fp32":
        cpu = FlatArena(p.arena.spec, torch.device("cpu"))
        cpu.params.copy_(p.arena.params.cpu())
        lp, pr, _ = predict_step_cpu(arch, cpu, test.images, y)
        err = relerr(a.log_probs, lp.double())
        off = int((a.pred != pr).sum())
        print(f"predict {arch} fp32 vs CPU oracle: log_probs {err:.1e}  pred off {off}")
        assert err <= 1e-4, err
        assert off <= near, (off, near)


def test_load_predictor_on_gpu(gpu, tmp_path):
    """load_predictor on the GPU gives the program's predictions, bit for bit."""
    from pytorch_distributed_mnist_amd.predict import load_predictor
    train, test = synthetic_split(256, True), synthetic_split(41, False)
    p = build_local_program("cnn", "bf16", "cuda", 256, train, test, seed=2)
    save_checkpoint(make_state(1, p.arena, 0.0, p.optimizer), True, 0, directory=str(tmp_path))
    want = p.predict()
    pr = load_predictor(str(tmp_path / "model_best.pth.tar"), "cnn")
    assert pr.device.type == "cuda" and pr.dtype == "bf16"
    got = pr.predict(test.images.numpy().reshape(41, 28, 28), test.labels.numpy())
    assert torch.equal(bits(got.log_probs), bits(want.log_probs))
    assert torch.equal(got.pred, want.pred) and torch.equal(got.confusion, want.confusion)


def test_cli_predict_out_on_gpu(gpu, tmp_path):
    """--evaluate --resume CKPT --predict-out P on the GPU (bf16 CNN): P is written and the
    eval line is the one printed without the flag."""
    train, test = synthetic_split(256, True), synthetic_split(16, False)
    p = build_local_program("cnn", "fp32", "cpu", 256, train, test, optimizer="sgd", seed=4)
    save_checkpoint(make_state(1, p.arena, 0.0, p.optimizer), False, 0, directory=str(tmp_path))
    ck = str(tmp_path / "checkpoint_0.pth.tar")
    env = dict(os.environ, PYTHONPATH=REPO + os.pathsep + os.environ.get("PYTHONPATH", ""))
    outs = []
    for extra in ([], ["--predict-out", str(tmp_path / "pred.npz")]):
        cmd = [sys.executable, os.path.join(REPO, "multi_proc_single_gpu.py"), "--device", "cuda",
               "-i", f"tcp://127.0.0.1:{free_port()}", "--synthetic", "--synthetic-size", "256",
               "--arch", "cnn", "--optimizer", "sgd", "--evaluate", "--resume", ck] + extra
        r = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        outs.append(r.stdout.splitlines())
    ev = [[l for l in o if l.startswith("test loss:")] for o in outs]
    assert len(ev[0]) == 1 and ev[0] == ev[1]
    assert [l for l in outs[1] if l.startswith("class ")] == outs[1][-10:]
    assert not [l for l in outs[0] if l.startswith("class ")]
    with np.load(tmp_path / "pred.npz") as z:
        lp, pred, lab, conf = z["log_probs"], z["pred"], z["labels"], z["confusion"]
    assert lp.shape == (10000, 10) and lp.dtype == np.float32 and np.isfinite(lp).all()
    assert np.array_equal(lp[np.arange(10000), pred], lp.max(1)) and pred.dtype == np.int64
    assert np.array_equal(conf, np.bincount(10 * lab + pred, minlength=100).reshape(10, 10))
    assert "{:.2f}%".format(100.0 * conf.trace() / 10000) in ev[1][0]
