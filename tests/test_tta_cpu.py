"""Test-time augmentation on the CPU path (--tta V; docs/kernels.md "Test-time augmentation"):
the combination tta_reduce_cpu against a float64 log-mean-exp, the views against the NumPy
augmentation, the program's evaluate() / predict(), the CLI on CPU / gloo, the usage errors and
the built kernel's resources.

The bound of the combination, |err| <= 1e-5 + 2^-22 |ref|: m is exact; the log term lies in
[0, ln 32] and carries at most about V + 4 roundings of 2^-24 (V exps and additions of terms
<= 1, one log), at most 36 * 2^-24 * 3.5 < 1e-5; the two last roundings (the addition of m, the
subtraction of lnV) are relative to the result's magnitude, 2 * 2^-24 < 2^-22.
"""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

from conftest import REPO

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.augment import (MAX_TTA, TTA_EPOCH, AugmentSpec,
                                                        augment_batch, check_tta, tta_view)
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.runtime.cpu_step import tta_reduce_cpu
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_dropout_cpu import _run_cli

AFFINE = AugmentSpec(2, 10.0, 0.1, seed=(9 << 32) + 32)
ELASTIC = AugmentSpec(0, 0.0, 0.0, seed=31, elastic=2.0)
NC = 10


# ---------------------------------------------------------------- inputs and the reference

def make_views(V, n, seed=0):
    """fp32 [V, n, 10] log-softmax rows of three families, interleaved by row: (0) random
    logits whose scale grows with the row up to values of -700, (1) one view dominating (its
    row near 0 in one class where the others are hundreds below), (2) all views equal.  Row 0
    (when n > 3: row 3 as well) has two equal maxima in every view.  No -0.0 anywhere."""
    g = torch.Generator().manual_seed(1000 * V + n + seed)
    scale = torch.logspace(-1, math.log10(320.0), max(n, 2), dtype=torch.float64)[:n]
    logits = torch.randn(V, n, NC, generator=g, dtype=torch.float64) * scale[None, :, None]
    fam = torch.arange(n) % 3
    dom = torch.randint(0, V, (n,), generator=g)
    cls = torch.randint(0, NC, (n,), generator=g)
    for r in range(n):
        if fam[r] == 1:
            logits[:, r] = torch.randn(V, NC, generator=g, dtype=torch.float64) - 300.0 * \
                torch.rand(V, 1, generator=g, dtype=torch.float64)
            logits[dom[r], r, cls[r]] += 650.0
        elif fam[r] == 2:
            logits[:, r] = logits[0, r].clone()
    for r in (0, 3):
        if r < n:
            logits[:, r] = logits[0, r].clone()
            logits[:, r, 7] = logits[:, r, 2] = logits[:, r].amax(dim=-1) + 0.5
    lp = torch.log_softmax(logits, dim=-1).clamp_min(-700.0).to(torch.float32) + 0.0
    assert torch.isfinite(lp).all() and not torch.signbit(lp[lp == 0]).any()
    return lp


def reference(lp):
    """The log of the mean probability over the views, in float64: [n, 10]."""
    return torch.logsumexp(lp.to(torch.float64), dim=0) - math.log(lp.shape[0])


def within_bound(out, ref):
    err = (out.to(torch.float64) - ref).abs()
    bound = 1e-5 + 2.0 ** -22 * ref.abs()
    return bool((err <= bound).all()), float((err / bound).max())


def first_argmax(rows):
    """The first maximum of every row, by the definition (not torch.argmax)."""
    a = rows.numpy()
    return torch.tensor([int(np.flatnonzero(r == r.max())[0]) for r in a], dtype=torch.int64)


# ---------------------------------------------------------------- the combination

@pytest.mark.parametrize("V", [1, 2, 3, 4, 8, 32])
def test_reduce_against_float64(V):
    lp = make_views(V, 257)
    assert lp.min() <= -690.0                       # the scaled family reaches -700
    out, pred, conf = tta_reduce_cpu(lp)
    assert out.dtype == torch.float32 and out.shape == (257, NC) and conf is None
    ok, worst = within_bound(out, reference(lp))
    print(f"V={V}: worst error / bound = {worst:.3f}")
    assert ok, worst
    assert pred.dtype == torch.int64 and torch.equal(pred, first_argmax(out))
    # rows 0 and 3: classes 2 and 7 tie in every view, so they tie in the result: the first
    assert out[0, 2] == out[0, 7] and pred[0] == 2 and out[3, 2] == out[3, 7] and pred[3] == 2


def test_one_view_returns_the_input_bits():
    lp = make_views(1, 65)
    out, pred, _ = tta_reduce_cpu(lp)
    assert torch.equal(out.view(torch.int32), lp[0].view(torch.int32))
    assert torch.equal(pred, first_argmax(lp[0]))


def test_equal_views_return_the_view():
    """V equal views: the mean probability is the view's; within the bound of it, whatever V."""
    one = make_views(1, 64)[0]
    for V in (2, 3, 32):
        out, _, _ = tta_reduce_cpu(one[None].repeat(V, 1, 1))
        assert within_bound(out, one.to(torch.float64))[0]


def test_reduce_confusion_and_argument_checks():
    lp = make_views(3, 40)
    y = torch.arange(40) % NC
    out, pred, conf = tta_reduce_cpu(lp, y)
    want = torch.bincount(y * NC + pred, minlength=100).view(NC, NC)
    assert torch.equal(conf, want) and int(conf.sum()) == 40
    with pytest.raises(ValueError):
        tta_reduce_cpu(lp[0])
    with pytest.raises(ValueError):
        tta_reduce_cpu(lp.to(torch.float64))


# ---------------------------------------------------------------- the views

@pytest.fixture(scope="module")
def images():
    g = torch.Generator().manual_seed(4)
    return torch.randint(0, 256, (20, 784), dtype=torch.uint8, generator=g)


@pytest.mark.parametrize("spec", [AFFINE, ELASTIC], ids=["affine", "elastic"])
def test_views_match_the_augmentation(images, spec):
    assert TTA_EPOCH == 0x80000000 and MAX_TTA == 32
    assert torch.equal(tta_view(images, 0, 20, 0, spec), images)          # view 0: the bytes
    rows = torch.arange(20)
    seen = []
    for v in (1, 2, 31):
        want = augment_batch(images, rows, 0x80000000 + v, spec)
        got = tta_view(images, 0, 20, v, spec)
        assert torch.equal(got, want) and not torch.equal(got, images)
        # not a training epoch's draw
        assert not torch.equal(got, augment_batch(images, rows, v, spec))
        assert all(not torch.equal(got, s) for s in seen)
        seen.append(got)
        # the absolute row decides, not the chunk
        chunks = torch.cat([tta_view(images, s, 7, v, spec) for s in range(0, 20, 7)])
        assert torch.equal(chunks, want)
        assert torch.equal(tta_view(images, 13, 1, v, spec), want[13:14])
        assert np.array_equal(tta_view(images.numpy(), 5, 9, v, spec), want[5:14].numpy())
    for bad in (-1, 32):
        with pytest.raises(ValueError):
            tta_view(images, 0, 20, bad, spec)


def test_check_tta():
    assert check_tta(1, None) == 1 and check_tta(1, AugmentSpec()) == 1
    assert check_tta(32, AFFINE) == 32 and check_tta(2, ELASTIC) == 2
    for views, spec in ((0, AFFINE), (33, AFFINE), (2.5, AFFINE), (2, None), (2, AugmentSpec())):
        with pytest.raises(ValueError):
            check_tta(views, spec)


# ---------------------------------------------------------------- the program

@pytest.mark.parametrize("arch", ["cnn", "linear"])
def test_cpu_program_predict_and_evaluate(arch, images):
    train, test = synthetic_split(64, True), synthetic_split(300, False)
    prog = build_local_program(arch, "fp32", "cpu", 32, train, test, optimizer="sgd", lr=0.01,
                               augment=AFFINE, tta=3)
    plain = build_local_program(arch, "fp32", "cpu", 32, train, test, optimizer="sgd", lr=0.01)
    plain.arena.params.copy_(prog.arena.params)
    y = torch.arange(20) % NC
    got = prog.predict(images, y)
    # the oracle: the NumPy views through the plain program's predict(), a float64 reduce
    lv = torch.stack([plain.predict(tta_view(images, 0, 20, v, AFFINE)).log_probs
                      for v in range(3)])
    assert torch.equal(lv[0], plain.predict(images).log_probs)
    assert torch.equal(got.log_probs, tta_reduce_cpu(lv)[0])
    assert within_bound(got.log_probs, reference(lv))[0]
    assert torch.equal(got.pred, first_argmax(got.log_probs))
    assert torch.equal(got.confusion, torch.bincount(y * NC + got.pred, minlength=100).view(NC, NC))
    assert prog.predict(images).confusion is None
    # tta= overrides the program's count; 1 is the plain path, bit for bit
    assert torch.equal(prog.predict(images, tta=1).log_probs, lv[0])
    assert torch.equal(plain.predict(images, tta=1).log_probs, lv[0])
    assert not torch.equal(prog.predict(images, tta=2).log_probs, got.log_probs)
    for bad in (0, 33):
        with pytest.raises(ValueError):
            prog.predict(images, tta=bad)
    with pytest.raises(ValueError):
        plain.predict(images, tta=2)                 # no ranges to draw the views from
    with pytest.raises(ValueError):
        build_local_program(arch, "fp32", "cpu", 32, train, test, tta=2)
    # evaluate(): the test split's combined rows, summed
    loss, acc = prog.evaluate()
    p = prog.predict()
    yt = test.labels.to(torch.int64)
    want = float((-p.log_probs.gather(1, yt[:, None])).to(torch.float64).sum())
    assert loss.count == acc.count == 300
    assert abs(loss.sum - want) <= 1e-12 * abs(want)
    assert acc.correct == int(p.confusion.trace()) == int(p.pred.eq(yt).sum())
    l1, a1 = plain.evaluate()
    assert l1.sum != loss.sum
    # nothing of the training state moved
    assert torch.equal(plain.arena.params, prog.arena.params)


def test_cpu_program_uses_the_average(images):
    from pytorch_distributed_mnist_amd.optim.ema import EmaSpec
    train, test = synthetic_split(64, True), synthetic_split(40, False)
    prog = build_local_program("cnn", "fp32", "cpu", 32, train, test, optimizer="sgd", lr=0.05,
                               augment=AFFINE, tta=2, ema=EmaSpec(0.5))
    prog.set_train_indices(torch.arange(64), epoch=0)
    prog.train_epoch()
    fresh = build_local_program("cnn", "fp32", "cpu", 32, train, test, optimizer="sgd",
                                augment=AFFINE, tta=2)
    fresh.arena.params.copy_(prog.ema.params)
    assert torch.equal(prog.predict(images).log_probs, fresh.predict(images).log_probs)
    fresh.arena.params.copy_(prog.arena.params)
    assert torch.equal(prog.predict(images, average=False).log_probs,
                       fresh.predict(images).log_probs)
    assert not torch.equal(prog.predict(images).log_probs,
                           prog.predict(images, average=False).log_probs)


def test_load_predictor(tmp_path, images):
    from pytorch_distributed_mnist_amd.predict import load_predictor
    from pytorch_distributed_mnist_amd.utils.checkpoint import make_state, save_checkpoint
    train, test = synthetic_split(64, True), synthetic_split(40, False)
    prog = build_local_program("linear", "fp32", "cpu", 32, train, test, augment=ELASTIC, tta=4)
    save_checkpoint(make_state(1, prog.arena, 0.0, prog.optimizer, None), False, 0,
                    directory=str(tmp_path))
    ck = str(tmp_path / "checkpoint_0.pth.tar")
    p = load_predictor(ck, "linear", device="cpu", tta=4, augment=ELASTIC)
    assert torch.equal(p.predict(images).log_probs, prog.predict(images).log_probs)
    p1 = load_predictor(ck, "linear", device="cpu")
    assert torch.equal(p1.predict(images).log_probs, prog.predict(images, tta=1).log_probs)
    for kw in (dict(tta=2), dict(tta=2, augment=AugmentSpec()), dict(tta=0, augment=ELASTIC),
               dict(tta=33, augment=ELASTIC)):
        with pytest.raises(ValueError):
            load_predictor(ck, "linear", device="cpu", **kw)


# ---------------------------------------------------------------- the flags

def test_cli_flags(capsys):
    a = parse_args(["--tta", "4", "--aug-shift", "2"])
    assert a.tta == 4
    a = parse_args([])
    assert not hasattr(a, "tta") and "tta" not in repr(a)
    assert parse_args(["--tta", "1"]).tta == 1                 # off: no range needed
    assert parse_args(["--tta", "32", "--aug-elastic", "1", "--evaluate"]).tta == 32
    for bad in (["--tta", "0"], ["--tta", "33"], ["--tta", "-1"], ["--tta", "2.5"], ["--tta", "2"],
                ["--tta", "2", "--aug-shift", "0"], ["--tta", "3", "--aug-seed", "5"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert "error: argument --tta" in capsys.readouterr().err, bad


# ---------------------------------------------------------------- the CLI on CPU / gloo

CNN = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.01", "--batch-size", "64",
       "--synthetic-size", "128", "--seed", "3"]
TTA = ["--tta", "4", "--aug-shift", "2", "--aug-rotate", "10"]
TEST_RE = re.compile(r"test loss: (\d+\.\d{6}), test acc: (\d+\.\d{2})%\.$")


def _epochs(out):
    return [l for l in out.splitlines() if l.startswith("Epoch:")]


def _test_part(line):
    return line[line.index("test loss: "):]


def _ckpt(d, i):
    return torch.load(d / "checkpoints" / f"checkpoint_{i}.pth.tar", weights_only=True)


def _same_bits(a, b):
    assert set(a) == set(b) and a["epoch"] == b["epoch"] and a["best_acc"] == b["best_acc"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v),
                               torch.as_tensor(b["optimizer"]["state"][i][name])), (i, name)


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """The CPU / gloo runs shared below: no flag, --tta 1, --tta 4 for two epochs, and --tta 4
    with the weight average for one."""
    root = tmp_path_factory.mktemp("tta_cli")
    runs = {}
    for name, args in (("plain", ["--epochs", "1"]),
                       ("one", ["--epochs", "1", "--tta", "1"]),
                       ("tta", ["--epochs", "2"] + TTA),
                       ("ema", ["--epochs", "1", "--ema-decay", "0.9"] + TTA)):
        d = root / name
        d.mkdir()
        runs[name] = (d, _run_cli(CNN + args, d))
    return runs


def test_cli_one_view_equals_no_flag(cli_runs):
    (dp, plain), (d1, one) = cli_runs["plain"], cli_runs["one"]
    assert "tta=1" in one and "tta" not in plain and "notice: test-time" not in one

    def norm(out):
        out = re.sub(r"init_method='[^']*'", "init_method=''", out)
        return re.sub(r", tta=1", "", out).splitlines()

    assert norm(plain) == norm(one)
    assert any(l.startswith("Namespace(") for l in norm(plain)) and len(_epochs(plain)) == 1
    _same_bits(_ckpt(dp, 0), _ckpt(d1, 0))


def test_cli_tta_changes_the_test_line_not_training(cli_runs):
    (dp, plain), (dt, tta) = cli_runs["plain"], cli_runs["tta"]
    assert tta.count("notice: test-time augmentation") == 1
    e0, p0 = _epochs(tta)[0], _epochs(plain)[0]
    assert _test_part(e0) != _test_part(p0)
    # the same samples are augmented for training with and without --tta: compare with a run
    # that trains with the ranges and tests plainly
    d = dt / "notta"
    d.mkdir()
    out = _run_cli(CNN + ["--epochs", "1"] + TTA[2:], d)
    n0 = _epochs(out)[0]
    train_part = lambda l: l[l.index("train loss: "):l.index("test loss: ")]
    assert train_part(n0) == train_part(e0)
    assert _test_part(n0) != _test_part(e0)
    a, b = _ckpt(d, 0), _ckpt(dt, 0)
    b["best_acc"] = a["best_acc"]            # (the model_best choice follows the test line)
    _same_bits(a, b)
    assert set(_ckpt(dt, 1)) == set(_ckpt(dp, 0))          # the checkpoint format


@pytest.mark.parametrize("run,extra", [("tta", []), ("ema", ["--ema-decay", "0.9"])])
def test_cli_evaluate_reproduces_the_epochs_and_writes_the_combined_rows(cli_runs, run, extra):
    d, out = cli_runs[run]
    ep = _epochs(out)
    for i, line in enumerate(ep):
        ck = str(d / "checkpoints" / f"checkpoint_{i}.pth.tar")
        npz = d / f"pred_{i}.npz"
        # (--seed with them: it is --aug-seed's default, the key of the views' draws)
        ev = _run_cli(["--arch", "cnn", "--optimizer", "sgd", "--evaluate", "--resume", ck,
                       "--seed", "3", "--predict-out", str(npz)] + TTA + extra, d)
        tl = [l for l in ev.splitlines() if l.startswith("test loss:")]
        assert len(tl) == 1 and tl[0] == _test_part(line)
        # the printed numbers are those of the file's combined rows
        z = np.load(npz)
        assert sorted(z.files) == ["confusion", "labels", "log_probs", "pred"]
        lp, y = z["log_probs"], z["labels"]
        assert lp.dtype == np.float32 and lp.shape == (len(y), NC)
        loss = float((-lp[np.arange(len(y)), y]).astype(np.float64).sum()) / len(y)
        m = TEST_RE.search(tl[0])
        assert m.group(1) == "{:.6f}".format(loss)
        correct = int(np.trace(z["confusion"]))
        assert m.group(2) == "{:.2f}".format(100.0 * correct / len(y))
        assert correct == int((z["pred"] == y).sum())
        assert np.array_equal(z["pred"], lp.argmax(axis=1))
        # they are not one softmax's rows: the mean of V distributions sums to 1 all the same
        assert np.allclose(np.exp(lp.astype(np.float64)).sum(axis=1), 1.0, atol=1e-5)
    if run == "tta":
        # without --tta the same checkpoint evaluates to another line: --evaluate read the flags
        ev = _run_cli(["--arch", "cnn", "--optimizer", "sgd", "--evaluate", "--resume", ck], d)
        tl = [l for l in ev.splitlines() if l.startswith("test loss:")]
        assert len(tl) == 1 and tl[0] != _test_part(ep[-1])


@pytest.mark.slow
def test_cli_world_size_invariance(cli_runs, tmp_path):
    """World size 2 evaluates unsharded, on every rank, the views of world size 1.  The weights
    of the two runs agree to 1e-6 (tests/test_augment_cpu.py's comparison: the gradient sum's
    order differs), so the printed loss may differ in its last digit."""
    out = _run_cli(CNN + ["--epochs", "1", "--world-size", "2", "--rank-prefix"] + TTA, tmp_path)
    ep = _epochs(re.sub(r"(?m)^\[rank \d\] ", "", out))
    assert len(ep) == 2 and _test_part(ep[0]) == _test_part(ep[1])       # both ranks, one line
    a, b = TEST_RE.search(ep[0]), TEST_RE.search(_epochs(cli_runs["tta"][1])[0])
    assert abs(float(a.group(1)) - float(b.group(1))) <= 2e-6
    assert abs(float(a.group(2)) - float(b.group(2))) <= 0.011
    assert out.count("notice: test-time augmentation") == 1


def test_cli_usage_errors(tmp_path):
    for bad in (["--tta", "0"], ["--tta", "33"], ["--tta", "2"], ["--tta", "2", "--evaluate"]):
        err = _run_cli(bad, tmp_path, ok=False)
        assert "error: argument --tta" in err and "usage:" in err, bad


# ---------------------------------------------------------------- the built kernel

SO = sorted(glob.glob(os.path.join(REPO, "pytorch_distributed_mnist_amd", "_C*.so")))


@pytest.mark.skipif(not SO or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="extension not built or ROCm llvm tools absent")
def test_kernel_resources():
    """tta_reduce keeps its ten maxima and ten sums in registers: no scratch, and no LDS."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernels as read
    hit = [v for k, v in read(SO[0]).items() if "tta_reduce_kernel" in k]
    assert len(hit) == 1
    assert hit[0].get("private_segment_fixed_size", 0) == 0
    assert hit[0]["group_segment_fixed_size"] == 0
    assert hit[0]["vgpr_count"] + hit[0].get("agpr_count", 0) <= 128
