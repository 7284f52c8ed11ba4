"""Mixup on the host (data/mixup.py, --mixup): the draws against a scalar re-implementation of
the spec, the partners' range and spread, the quantile table (shape, the uniform case, other
shapes against sampled Beta variates), the integer blend, one CPU training step against an fp64
evaluation of the definition, the CLI on CPU/gloo, and the built kernels' resources.

The spec (N = size of the training set):
    (r0, r1, _, _) = Philox4x32-10(counter (i, e, 3, 0), key (seed lo, seed hi))
    j = (r0 * N) >> 32,  q = QT[r1 >> 22],  lambda = q / 256
    m = (q a + (256 - q) b + 128) >> 8
    QT[k] = round(256 max(x, 1 - x)),  x the Beta(A, A) quantile at (k + 0.5) / 1024
    t = lambda t(y) + (1 - lambda) t(y2),  row loss = lambda loss_E(y) + (1 - lambda) loss_E(y2)
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
from pytorch_distributed_mnist_amd.data.augment import AugmentSpec, augment_batch
from pytorch_distributed_mnist_amd.data.dropout import DropoutSpec, multiplier
from pytorch_distributed_mnist_amd.data.mixup import (MixupSpec, beta_cdf, blend, draw, mix_batch,
                                                      quantile_table, spec_from_args)
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.models.reference import functional_forward
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_dropout_cpu import _run_cli
from test_label_smoothing_cpu import rel, smoothed_loss_fp64

M32 = 0xFFFFFFFF


# ---------------------------------------------------------------- the draws

def _philox_scalar(c, k):
    """Philox4x32-10 on Python integers, one round at a time."""
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("counter,key,expected", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_scalar_philox_known_answers(counter, key, expected):
    """The scalar generator the next test relies on, on Random123's known-answer vectors."""
    assert _philox_scalar(_words(counter), _words(key)) == _words(expected)


def _draw_scalar(i, e, seed, n_train, qt):
    r = _philox_scalar([i & M32, e & M32, 3, 0], [seed & M32, seed >> 32])
    return (r[0] * n_train) >> 32, int(qt[r[1] >> 22])


@pytest.mark.parametrize("seed", [0, (7 << 32) + 12345])
@pytest.mark.parametrize("n_train", [1, 7, 60000])
def test_draws_match_the_spec_and_partners_stay_in_range(seed, n_train):
    spec = MixupSpec(0.4, seed)
    qt = spec.table()
    idx = np.concatenate([[0, 1, 59999, (1 << 27) - 1], np.random.default_rng(1).integers(0, 60000, 60)])
    for e in (0, 7):
        j, q = draw(idx, e, spec, n_train)
        assert j.dtype == np.int64 and q.dtype == np.int64 and j.shape == q.shape == (64,)
        want = [_draw_scalar(int(i), e, seed, n_train, qt) for i in idx]
        assert j.tolist() == [w[0] for w in want] and q.tolist() == [w[1] for w in want]
    # the range, over many more draws
    j, q = draw(np.arange(60000), 3, spec, n_train)
    assert j.min() >= 0 and j.max() < n_train
    assert q.min() >= 128 and q.max() <= 256
    if n_train == 60000:
        assert j.max() > 59000 and j.min() < 1000 and (j == np.arange(60000)).sum() < 20
    # a sample's draw does not depend on the batch it is drawn in; it does on epoch and key
    j2, q2 = draw(np.arange(100, 200), 3, spec, n_train)
    assert np.array_equal(j2, j[100:200]) and np.array_equal(q2, q[100:200])
    if n_train > 1:
        assert not np.array_equal(j, draw(np.arange(60000), 4, spec, n_train)[0])
        assert not np.array_equal(j, draw(np.arange(60000), 3, MixupSpec(0.4, seed + 1), n_train)[0])
        assert not np.array_equal(j, draw(np.arange(60000), 3, MixupSpec(0.4, seed + (1 << 32)),
                                          n_train)[0])


def test_partner_spread():
    """600,000 fixed draws at N = 10 (60,000 samples x epochs 0..9, seed 12345): each partner's
    share is within 5 sigma of 1/10.  Seen: at most 1.63 sigma."""
    spec = MixupSpec(1.0, 12345)
    cnt = np.zeros(10)
    for e in range(10):
        cnt += np.bincount(draw(np.arange(60000), e, spec, 10)[0], minlength=10)
    n = 600000
    assert cnt.sum() == n
    sigma = math.sqrt(0.1 * 0.9 / n)
    dev = (cnt / n - 0.1) / sigma
    print("\npartner shares, in sigma:", np.round(dev, 2))
    assert np.abs(dev).max() <= 5.0, dev


def test_draws_leave_the_other_streams_alone():
    """Counter word 2 = 3: the pair's Philox block is none of the augmentation's (0), dropout's
    (1) or the elastic control points' (2)."""
    from pytorch_distributed_mnist_amd.data.augment import philox4x32_10
    key = np.array([5, 0], dtype=np.uint64)
    blocks = [philox4x32_10(np.array([9, 2, w, 0], dtype=np.uint64), key).tolist() for w in range(4)]
    assert len({tuple(b) for b in blocks}) == 4
    qt = MixupSpec(1.0, 5).table()
    j, q = draw([9], 2, MixupSpec(1.0, 5), 60000)
    assert (int(j[0]), int(q[0])) == ((blocks[3][0] * 60000) >> 32, int(qt[blocks[3][1] >> 22]))


# ---------------------------------------------------------------- the quantile table

@pytest.mark.parametrize("alpha", [0.2, 0.4, 1.0, 2.0, 10.0])
def test_table_shape(alpha):
    """Monotone (falling to the fold, rising after it), in 128..256, symmetric about the fold."""
    qt = quantile_table(alpha)
    assert qt.dtype == np.int32 and qt.shape == (1024,)
    assert qt.min() >= 128 and qt.max() <= 256
    assert np.array_equal(qt, qt[::-1])
    assert (np.diff(qt[:512]) <= 0).all() and (np.diff(qt[512:]) >= 0).all()
    assert qt[511] == qt[512] == 128
    spec = MixupSpec(alpha, 3)
    assert np.array_equal(spec.table(), qt) and spec.table() is spec.table()


def test_uniform_case_is_exact():
    u = (np.arange(1024) + 0.5) / 1024
    want = [int(math.floor(256 * max(x, 1 - x) + 0.5)) for x in u]      # (no ties: .125 steps)
    assert quantile_table(1.0).tolist() == want


# n = 4,000,000 variates per shape.  Largest deviation seen: 0.75 (A = 0.2), 0.62 (A = 0.4),
# 0.57 (A = 2) levels of 256 -- up to 0.5 of it is the table's own rounding, the rest the
# sampling noise of the empirical quantiles (1,000,000 variates give 1.009 at A = 0.2: too few).
@pytest.mark.parametrize("alpha", [0.2, 0.4, 2.0])
def test_other_shapes_against_sampled_beta(alpha):
    x = np.random.default_rng(0).beta(alpha, alpha, 4_000_000)
    xq = np.quantile(x, (np.arange(1024) + 0.5) / 1024)
    emp = 256.0 * np.maximum(xq, 1.0 - xq)
    dev = np.abs(quantile_table(alpha) - emp).max()
    print(f"\nA = {alpha}: largest deviation {dev:.3f} levels")
    assert dev <= 1.0, dev


def test_cdf_known_values():
    """I_x(a, a) in closed form: a = 1 (x), a = 2 (3x^2 - 2x^3), a = 1/2 (2/pi asin sqrt x)."""
    x = np.array([0.0, 1e-9, 0.01, 0.2, 0.37, 0.5])
    assert np.allclose(beta_cdf(1.0, x), x, rtol=1e-13, atol=0)
    assert np.allclose(beta_cdf(2.0, x), 3 * x ** 2 - 2 * x ** 3, rtol=1e-13, atol=0)
    assert np.allclose(beta_cdf(0.5, x), 2 / np.pi * np.arcsin(np.sqrt(x)), rtol=1e-12, atol=0)


# ---------------------------------------------------------------- the blend

def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 784), dtype=np.uint8)


def test_blend_identity_mean_and_float():
    a, b = _noise(64, 1), _noise(64, 2)
    assert np.array_equal(blend(a, b, np.full(64, 256)), a)                 # q = 256: a itself
    for va, vb in ((10, 20), (10, 21), (255, 0), (0, 255), (7, 7)):
        out = blend(np.full((1, 784), va, np.uint8), np.full((1, 784), vb, np.uint8), [128])
        assert out.dtype == np.uint8 and (out == (va + vb + 1) // 2).all()  # the rounded mean
    # against a float64 blend on white noise: at most 1 grey level (1/2 from rounding)
    q = np.random.default_rng(3).integers(128, 257, 64)
    lam = q[:, None] / 256.0
    exact = lam * a + (1.0 - lam) * b
    err = np.abs(blend(a, b, q).astype(np.float64) - exact).max()
    print(f"\nblend against float64: {err:.3f} levels")
    assert err <= 1.0
    assert err <= 0.5                        # (what round-to-nearest gives; the issue asks 1)


def test_mix_batch_is_the_blend_of_the_pairs():
    train = _noise(97, 4)
    spec = MixupSpec(0.4, 9)
    idx = np.random.default_rng(5).permutation(97)[:40]
    out, j, q = mix_batch(train, idx, 2, spec)
    jj, qq = draw(idx, 2, spec, 97)
    assert np.array_equal(j, jj) and np.array_equal(q, qq) and (q < 256).any()
    assert np.array_equal(out, blend(train[idx], train[j], q))
    t, _, _ = mix_batch(torch.from_numpy(train), torch.from_numpy(idx), 2, spec)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), out)
    # a table of 256 everywhere leaves the images alone
    same, _, q1 = mix_batch(train, idx, 2, spec, np.full(1024, 256, np.int32))
    assert (q1 == 256).all() and np.array_equal(same, train[idx])


# ---------------------------------------------------------------- the flags, the program

def test_cli_flags(capsys):
    a = parse_args(["--arch", "cnn", "--mixup", "0.4", "--mixup-seed", "77"])
    assert (a.mixup, a.mixup_seed) == (0.4, 77)
    assert spec_from_args(a) == MixupSpec(0.4, 77)
    a = parse_args([])
    assert not hasattr(a, "mixup") and not hasattr(a, "mixup_seed") and "mixup" not in repr(a)
    assert spec_from_args(a) is None
    assert spec_from_args(parse_args(["--arch", "cnn", "--mixup", "0"])) is None
    assert spec_from_args(parse_args(["--arch", "cnn", "--mixup-seed", "4"])) is None
    assert spec_from_args(parse_args(["--arch", "cnn", "--mixup", "1"])).seed == 0
    assert spec_from_args(parse_args(["--arch", "cnn", "--mixup", "1", "--seed", "6"])).seed == 6
    assert spec_from_args(parse_args(["--arch", "cnn", "--mixup", "10", "--seed", "6",
                                      "--mixup-seed", "8"])) == MixupSpec(10.0, 8)
    parse_args(["--arch", "linear", "--mixup", "0"])         # off: nothing to object to
    for bad in (["--arch", "cnn", "--mixup", "-0.1"], ["--arch", "cnn", "--mixup", "10.5"],
                ["--arch", "cnn", "--mixup", "nan"], ["--arch", "cnn", "--mixup-seed", "-1"],
                ["--arch", "linear", "--mixup", "0.4"], ["--mixup", "0.4"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert "error: argument --mixup" in capsys.readouterr().err, bad
    for bad in (-0.1, 10.5, float("nan")):
        with pytest.raises(ValueError):
            MixupSpec(bad)


def test_program_needs_the_epoch_and_the_cnn():
    train, test = synthetic_split(64, True), synthetic_split(32, False)
    spec = MixupSpec(0.4, seed=1)
    with pytest.raises(ValueError, match="head"):
        build_local_program("linear", "fp32", "cpu", 32, train, test, mixup=spec)
    p = build_local_program("cnn", "fp32", "cpu", 32, train, test, mixup=spec)
    idx = distributed_indices(len(train), 1, 0, 0)
    with pytest.raises(ValueError, match="epoch"):
        p.set_train_indices(idx)
    q = build_local_program("cnn", "fp32", "cpu", 32, train, test, mixup=MixupSpec(0.0, 1))
    assert q.mixup is None
    q.set_train_indices(idx)                                 # off: no epoch needed


@pytest.mark.parametrize("drop", [None, DropoutSpec(0.5, 5)], ids=["nodrop", "drop"])
@pytest.mark.parametrize("e", [0.0, 0.1])
def test_cpu_step_matches_the_definition(e, drop):
    """One CNN train_step_cpu at B = 8 with mixup (and an elastic + affine transform, so that the
    order -- mix the bytes, then transform with the primary sample's parameters -- matters): the
    gradients in the arena and the metric loss against the fp64 evaluation of the definition
    written out here, at tests/test_label_smoothing_cpu.py's 1e-5 relative (fp32 autograd
    against fp64); evaluate() and predict() are not mixed."""
    B, ep = 8, 3
    train, test = synthetic_split(64, True), synthetic_split(16, False)
    mix = MixupSpec(0.4, 11)
    aug = AugmentSpec(1, 10.0, 0.1, 4, 1.5)
    kw = dict(optimizer="sgd", lr=0.0, momentum=0.0, weight_decay=0.0, seed=3, label_smoothing=e,
              dropout=drop, augment=aug)
    p = build_local_program("cnn", "fp32", "cpu", B, train, test, mixup=mix, **kw)
    plain = build_local_program("cnn", "fp32", "cpu", B, train, test, **kw)
    assert p.evaluate()[0].average == plain.evaluate()[0].average
    assert torch.equal(p.predict().log_probs, plain.predict().log_probs)
    idx = distributed_indices(len(train), 1, 0, 0)[:B]
    tp = {k: v.clone() for k, v in p.arena.torch_tensors(p.arena.params).items()}
    p.set_train_indices(idx, epoch=ep)
    tl, ta = p.train_epoch()
    got = p.arena.torch_tensors(p.arena.grads)

    # the definition, from the spec's pieces
    j, q = draw(idx, ep, mix, len(train))
    assert (q < 256).any() and (j != idx.numpy()).any()
    mixed = blend(train.images.numpy()[idx.numpy()], train.images.numpy()[j], q)
    images = torch.from_numpy(augment_batch(mixed, idx.numpy(), ep, aug))
    assert torch.equal(images, p.train_images_cpu(idx))
    x, y, y2 = normalize_reference(images).double(), train.labels[idx], train.labels[torch.from_numpy(j)]
    lam = torch.from_numpy(q).double() / 256.0
    leaves = {k: v.double().requires_grad_() for k, v in tp.items()}
    mult = None if drop is None else multiplier(idx, ep, drop).double()
    logits = functional_forward("cnn", leaves, x, mult)
    logits.retain_grad()
    rows = []
    t = torch.zeros_like(logits)
    for i in range(B):
        l1, t1 = smoothed_loss_fp64(logits[i:i + 1], y[i:i + 1], e)
        l2, t2 = smoothed_loss_fp64(logits[i:i + 1], y2[i:i + 1], e)
        rows.append(lam[i] * l1 + (1.0 - lam[i]) * l2)
        t[i] = (lam[i] * t1 + (1.0 - lam[i]) * t2)[0].detach()
    loss = torch.stack(rows).mean()
    loss.backward()
    want_dl = (torch.softmax(logits.detach(), 1) - t) / B
    assert rel(logits.grad, want_dl) <= 1e-12
    assert abs(t.sum(1) - 1.0).max() <= 1e-15
    for name, leaf in leaves.items():
        r = rel(got[name], leaf.grad)
        print(f"E={e} drop={drop is not None} {name}: {r:.2e}")
        assert r <= 1e-5, (name, r)
    print(f"E={e} loss: {tl.average} vs {loss.item()}")
    assert abs(tl.average - loss.item()) <= 1e-5 * abs(loss.item())
    assert ta.correct == int((logits.argmax(1) == y).sum())            # against the primary label
    # the unmixed step is another number
    plain.set_train_indices(idx, epoch=ep)
    assert abs(plain.train_epoch()[0].average - loss.item()) > 1e-3


# ---------------------------------------------------------------- the CLI on CPU / gloo

CNN = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.01", "--batch-size", "64",
       "--synthetic-size", "256", "--seed", "3"]
MIX = ["--mixup", "0.4", "--dropout", "0.5", "--aug-elastic", "2", "--label-smoothing", "0.1"]


def _epochs(out):
    return [l for l in out.splitlines() if l.startswith("Epoch:")]


def _ckpt(d, i):
    return torch.load(d / "checkpoints" / f"checkpoint_{i}.pth.tar", weights_only=True)


def _same_checkpoint(a, b):
    assert a["epoch"] == b["epoch"] and a["best_acc"] == b["best_acc"]
    assert set(a) == set(b)
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v),
                               torch.as_tensor(b["optimizer"]["state"][i][name])), (i, name)


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """The CPU/gloo runs the tests below share: one epoch without the flag, with --mixup 0, with
    --mixup 0.4 alone, and one and two epochs with dropout, elastic distortion and label
    smoothing alongside."""
    root = tmp_path_factory.mktemp("mixup_cli")
    runs = {}
    for name, args in (("plain", ["--epochs", "1"]),
                       ("zero", ["--epochs", "1", "--mixup", "0"]),
                       ("alone", ["--epochs", "1", "--mixup", "0.4"]),
                       ("one", ["--epochs", "1"] + MIX),
                       ("two", ["--epochs", "2"] + MIX)):
        d = root / name
        d.mkdir()
        runs[name] = (d, _run_cli(CNN + args, d))
    return runs


def test_cli_zero_equals_no_flag(cli_runs):
    """--mixup 0 prints and checkpoints what the run without the flag does: every line of the
    output, but for the flag itself (and the rendezvous port) in the Namespace line."""
    (dp, plain), (dz, zero) = cli_runs["plain"], cli_runs["zero"]
    assert "mixup=0.0" in zero and "mixup" not in plain
    assert len(_epochs(plain)) == 1

    def norm(out):
        out = re.sub(r"init_method='[^']*'", "init_method=''", out)
        return re.sub(r", mixup=0\.0", "", out).splitlines()

    assert norm(plain) == norm(zero)
    assert any(l.startswith("Namespace(") for l in norm(plain))
    _same_checkpoint(_ckpt(dp, 0), _ckpt(dz, 0))


def test_cli_mixup_changes_training_not_evaluation(cli_runs):
    (dp, plain), (da, alone), (d2, two) = cli_runs["plain"], cli_runs["alone"], cli_runs["two"]
    assert "mixup=0.4" in alone and "mixup=0.4" in two
    loss = lambda l: l.split("train loss: ")[1].split(",")[0]
    assert loss(_epochs(alone)[0]) != loss(_epochs(plain)[0])
    assert not torch.equal(_ckpt(dp, 0)["state_dict"]["module.fc2.weight"],
                           _ckpt(da, 0)["state_dict"]["module.fc2.weight"])
    # --evaluate ignores the flag: the same test line with and without it, and it is the
    # training run's own test loss of that epoch
    ep = _epochs(two)
    assert len(ep) == 2
    ck = str(d2 / "checkpoints" / "checkpoint_1.pth.tar")
    lines = []
    for extra in (MIX, []):
        out = _run_cli(["--arch", "cnn", "--optimizer", "sgd", "--evaluate", "--resume", ck] + extra,
                       d2)
        line = [l for l in out.splitlines() if l.startswith("test loss:")]
        assert len(line) == 1
        lines.append(line[0])
    assert lines[0] == lines[1]
    assert lines[0].split("test loss: ")[1] == ep[1].split("test loss: ")[1]


def test_cli_resume_reproduces_uninterrupted_run(cli_runs):
    """Two epochs straight equal one epoch plus --resume for the second, the flags given again,
    with --dropout, --aug-elastic and --label-smoothing alongside."""
    (d1, _), (d2, _) = cli_runs["one"], cli_runs["two"]
    _same_checkpoint(_ckpt(d1, 0), _ckpt(d2, 0))
    out = _run_cli(CNN + MIX + ["--epochs", "2", "--resume",
                                str(d1 / "checkpoints" / "checkpoint_0.pth.tar")], d1)
    ep = _epochs(out)
    assert len(ep) == 1 and ep[0].startswith("Epoch: 1/2,")
    assert ep[0] == _epochs(cli_runs["two"][1])[1]
    _same_checkpoint(_ckpt(d1, 1), _ckpt(d2, 1))
    # the checkpoint format is the plain run's
    assert set(_ckpt(d1, 1)) == set(_ckpt(cli_runs["plain"][0], 0))


@pytest.mark.slow
def test_cli_world_size_invariance(cli_runs, tmp_path):
    """World size 1 and 2 with --mixup train on the same mixed samples (a partner may live in
    the other rank's shard): the same weights, under tests/test_augment_cpu.py's comparison."""
    _run_cli(CNN + MIX + ["--epochs", "1", "--world-size", "2"], tmp_path)
    a = _ckpt(cli_runs["one"][0], 0)["state_dict"]
    b = _ckpt(tmp_path, 0)["state_dict"]
    for k in a:
        assert torch.allclose(a[k], b[k], atol=1e-6, rtol=0), (k, (a[k] - b[k]).abs().max())
    c = _ckpt(cli_runs["plain"][0], 0)["state_dict"]
    assert not torch.allclose(a["module.fc2.weight"], c["module.fc2.weight"], atol=1e-6, rtol=0)


def test_cli_usage_errors(tmp_path):
    for bad in (["--arch", "cnn", "--mixup", "-1"], ["--arch", "cnn", "--mixup", "10.5"],
                ["--arch", "linear", "--mixup", "0.4"]):
        err = _run_cli(bad, tmp_path, ok=False)
        assert "error: argument --mixup" in err and "usage:" in err, bad


# ---------------------------------------------------------------- the built kernels

SO = sorted(glob.glob(os.path.join(REPO, "pytorch_distributed_mnist_amd", "_C*.so")))


@pytest.mark.skipif(not SO or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="extension not built or ROCm llvm tools absent")
def test_kernel_resources():
    """The mixup gather runs beside cnn_bwd as the elastic gather does: no LDS, no scratch, two
    waves per SIMD.  The mixup head has no scratch and the dropout head's LDS."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernels as read
    ks = read(SO[0])

    def one(name):
        hit = [v for k, v in ks.items() if name in k]
        assert len(hit) == 1, (name, [k for k in ks if name in k])
        return hit[0]

    g = one("gather_epoch_mixup_kernel")
    assert g["group_segment_fixed_size"] == 0
    assert g.get("private_segment_fixed_size", 0) == 0
    assert g["vgpr_count"] + g.get("agpr_count", 0) <= 256
    h, d = one("cnn_head_mixup_kernel"), one("cnn_head_dropout_kernel")
    assert h.get("private_segment_fixed_size", 0) == 0
    assert h["group_segment_fixed_size"] == d["group_segment_fixed_size"] > 0
    assert one("mixup_pairs_rows_kernel").get("private_segment_fixed_size", 0) == 0
    # the kernels the twins were copied from are still there, without LDS either
    for name in ("gather_epoch_elastic_kernel", "gather_epoch_augment_kernel"):
        assert one(name)["group_segment_fixed_size"] == 0
