"""Adversarial evaluation (--attack-eps, --arch mlp) on the CPU path, and the float64 oracle that
tests/test_gpu_attack.py shares: the input gradient of the 784-128-10 MLP from fc1's
pre-activation on, its summed magnitude s and its error bound (docs/kernels.md "Adversarial
evaluation": the derivation), and the integer step rule.

Measured on the CPU path (21 synthetic images, fresh weights): pixels under the threshold
0.22 % .. 0.27 % of 16464 at every step of every (steps, eps) below; every other byte equals the oracle's."""
import re

import numpy as np
import pytest
import torch

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_dropout_cpu import _run_cli

U24, PLANES = 2.0 ** -24, 2.0 ** -18
A_N, B_N = 1.0 / (255.0 * 0.3081), 0.1307 / 0.3081


def path_bound(S, forward=False):
    """The bound on e = |g - g_ref| / s (docs/kernels.md "Adversarial evaluation"): K 2^-24 plus
    the planes' 2^-18, K = twice the fp32 roundings on the path from the partials -- S split
    adds, 9 for a logit, 14 for softmax and dl, 10 for dh, 768 MFMA accumulations -- and, from
    the bytes (`forward`), fc1's forward with its own planes as well (1568 accumulations)."""
    k = 2 * (S + 9 + 14 + 10 + 768 + (1568 if forward else 0))
    return k * U24 + (2 if forward else 1) * PLANES


def oracle(pre, w2, b2, w1, y):
    """float64, from fc1's pre-activation `pre` [B, 128] (bias included): the gradient g [B, 784]
    of -log_softmax(logits)[y] with respect to the normalised pixels and s, the summed magnitude
    of its terms, sum_n [h > 0] (sum_c |dl_c| |W2[c][n]|) |W1[n][px]|."""
    pre, w2, b2, w1 = (np.asarray(a, dtype=np.float64) for a in (pre, w2, b2, w1))
    y = np.asarray(y, dtype=np.int64)
    mask = pre > 0
    lg = (pre * mask) @ w2.T + b2
    p = np.exp(lg - lg.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    dl = p.copy()
    dl[np.arange(len(y)), y] -= 1.0
    return ((dl @ w2) * mask) @ w1, ((np.abs(dl) @ np.abs(w2)) * mask) @ np.abs(w1)


def step_rule(x, x0, g, eps, alpha):
    """clamp(x + alpha sign(g), max(0, x0 - eps), min(255, x0 + eps)) on bytes."""
    x, x0 = np.asarray(x, dtype=np.int64), np.asarray(x0, dtype=np.int64)
    v = x + alpha * np.sign(g).astype(np.int64)
    return np.minimum(np.maximum(v, np.maximum(x0 - eps, 0)), np.minimum(x0 + eps, 255)).astype(np.uint8)


def model_oracle(arena, x, y):
    """oracle() of the mlp weights in `arena` on the bytes x [B, 784], the forward in float64."""
    w = {n: arena.param(n).detach().cpu().double().numpy()
         for n in ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")}
    w1 = w["fc1.weight"]
    pre = A_N * np.asarray(x, dtype=np.float64) @ w1.T - B_N * w1.sum(1) + w["fc1.bias"]
    return oracle(pre, w["fc2.weight"], w["fc2.bias"], w1, y)


def check_one_step(tag, got, arena, x, x0, y, eps, alpha):
    """`got` = one attack step from x: the oracle's bytes at every pixel with |g| > bound * s,
    and at most 1 % of the pixels under that."""
    g, s = model_oracle(arena, x, y)
    sure = np.abs(g) > path_bound(25, forward=True) * s
    skipped = 1.0 - sure.mean()
    print(f"{tag}: {100 * skipped:.3f} % of {sure.size} pixels under the threshold")
    assert skipped <= 0.01, tag
    assert np.array_equal(np.asarray(got)[sure], step_rule(x, x0, g, eps, alpha)[sure]), tag


@pytest.fixture(scope="module")
def prog():
    return build_local_program("mlp", "fp32", "cpu", 8, synthetic_split(64, True),
                               synthetic_split(21, False), seed=5)


@pytest.mark.parametrize("eps", [8, 64])
@pytest.mark.parametrize("steps", [1, 3])
def test_cpu_attack_against_float64(prog, steps, eps):
    """Every step of the chain against the oracle.  With steps * alpha <= eps the box of x0 never
    binds, so the K-step call equals K chained one-step calls (each its own x0) bit for bit."""
    x0, y = prog.test_split.images.numpy(), prog.test_split.labels.numpy()
    alpha = eps // steps
    x = x0
    for k in range(steps):
        nxt = prog.attack(x, y, eps, 1, alpha).numpy()
        check_one_step(f"cpu steps={steps} eps={eps} step {k}", nxt, prog.arena, x, x, y, eps,
                       alpha)
        x = nxt
    assert np.array_equal(prog.attack(x0, y, eps, steps, alpha).numpy(), x)
    # the test split and the default alpha (eps at one step, else round(2.5 eps / steps)): inside
    # the box, and at one step the call above
    d = prog.attack(eps=eps, steps=steps).numpy()
    assert d.dtype == np.uint8 and (np.abs(d.astype(np.int64) - x0) <= eps).all()
    assert steps > 1 or np.array_equal(d, x)


def test_predictor_attack_takes_numpy_and_square_images(tmp_path, prog):
    from pytorch_distributed_mnist_amd.predict import load_predictor
    from pytorch_distributed_mnist_amd.utils.checkpoint import make_state, save_checkpoint
    save_checkpoint(make_state(1, prog.arena, 0.0, prog.optimizer, None), False, 0,
                    directory=str(tmp_path))
    p = load_predictor(str(tmp_path / "checkpoint_0.pth.tar"), "mlp", device="cpu")
    x0, y = prog.test_split.images, prog.test_split.labels
    want = prog.attack(x0, y, 16, 2)
    assert want.dtype == torch.uint8 and tuple(want.shape) == (21, 784)
    assert torch.equal(p.attack(x0.numpy().reshape(21, 28, 28), y.numpy(), 16, steps=2), want)
    assert torch.equal(p.attack(x0, y, 0), x0)                       # eps = 0 returns the images
    for bad in (dict(eps=256), dict(eps=8, steps=0), dict(eps=8, alpha=0)):
        with pytest.raises(ValueError):
            p.attack(x0, y, **bad)
    lin = build_local_program("linear", "fp32", "cpu", 8, prog.train_split, prog.test_split)
    with pytest.raises(ValueError, match="no input-gradient kernel"):
        lin.attack(x0, y, 8)


def test_flags(capsys):
    a = parse_args(["--evaluate", "--arch", "mlp", "--attack-eps", "25", "--attack-steps", "10"])
    assert (a.attack_eps, a.attack_steps) == (25, 10) and not hasattr(a, "attack_alpha")
    assert "attack" not in repr(parse_args([]))
    assert parse_args(["--attack-eps", "0"]).attack_eps == 0         # off: nothing else is asked
    mlp = ["--evaluate", "--arch", "mlp"]
    for bad, word in ((["--arch", "mlp", "--attack-eps", "8"], "--attack-eps"),
                      (["--evaluate", "--attack-eps", "8"], "no input-gradient kernel"),
                      (["--evaluate", "--arch", "cnn", "--attack-eps", "8"], "no input-gradient kernel"),
                      (["--evaluate", "--arch", "mlp2", "--attack-eps", "8"], "no input-gradient kernel"),
                      (mlp + ["--attack-eps", "8", "--tta", "2", "--aug-shift", "1"], "--attack-eps"),
                      (mlp + ["--attack-eps", "256"], "--attack-eps"),
                      (mlp + ["--attack-eps", "-1"], "--attack-eps"),
                      (mlp + ["--attack-eps", "8", "--attack-steps", "0"], "--attack-steps"),
                      (mlp + ["--attack-eps", "8", "--attack-steps", "101"], "--attack-steps"),
                      (mlp + ["--attack-eps", "8", "--attack-alpha", "0"], "--attack-alpha"),
                      (mlp + ["--attack-steps", "2"], "--attack-steps"),
                      (mlp + ["--attack-alpha", "2"], "--attack-alpha")):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert word in capsys.readouterr().err, bad


ADV_RE = re.compile(r"adversarial \(eps 25/255, 2 steps, alpha 31/255\) loss: (\d+\.\d{6}), "
                    r"acc: (\d+\.\d{2})%\.$")


def adv_line_matches_file(lines, npz):
    """The one adversarial line of a run's stdout, its numbers recomputed from the file's
    adv_log_probs / adv_pred / adv_confusion and labels: (line, the file)."""
    adv = [l for l in lines if l.startswith("adversarial")]
    assert len(adv) == 1 and ADV_RE.match(adv[0]), adv
    z, m = np.load(npz), ADV_RE.match(adv[0])
    lp, y = z["adv_log_probs"], z["labels"]
    assert m.group(1) == "{:.6f}".format(float((-lp[np.arange(len(y)), y]).astype(np.float64).sum()) / len(y))
    assert m.group(2) == "{:.2f}".format(100.0 * int((z["adv_pred"] == y).sum()) / len(y))
    assert int(np.trace(z["adv_confusion"])) == int((z["adv_pred"] == y).sum())
    return adv[0], z


def test_cli(tmp_path):
    """Training prints nothing new; --evaluate with the flags adds one line after the unchanged
    test line and three arrays to the file; world size 2 prints world size 1's line."""
    train = _run_cli(["--arch", "mlp", "--optimizer", "sgd", "--lr", "0.05", "--batch-size", "64",
                      "--synthetic-size", "256", "--epochs", "1", "--seed", "3"], tmp_path)
    assert "adversarial" not in train and "attack" not in train
    ev = ["--arch", "mlp", "--optimizer", "sgd", "--evaluate", "--resume",
          str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar")]
    atk = ["--attack-eps", "25", "--attack-steps", "2"]
    plain = _run_cli(ev + ["--predict-out", str(tmp_path / "p.npz")], tmp_path).splitlines()
    adv = _run_cli(ev + atk + ["--predict-out", str(tmp_path / "a.npz")], tmp_path).splitlines()
    assert sorted(np.load(tmp_path / "p.npz").files) == ["confusion", "labels", "log_probs", "pred"]
    assert not any("adversarial" in l for l in plain)
    rest = [l for l in adv if not l.startswith(("Namespace(", "adversarial"))]
    assert rest == [l for l in plain if not l.startswith("Namespace(")]
    line, z = adv_line_matches_file(adv, tmp_path / "a.npz")
    assert adv[adv.index(line) - 1].startswith("test loss:")
    assert sorted(z.files) == ["adv_confusion", "adv_log_probs", "adv_pred", "confusion", "labels",
                               "log_probs", "pred"]
    y, m = z["labels"], ADV_RE.match(line)
    # the attack costs accuracy, and cannot gain any loss-wise
    clean = -z["log_probs"][np.arange(len(y)), y].astype(np.float64).sum() / len(y)
    assert float(m.group(1)) > clean
    two = _run_cli(ev + atk + ["--world-size", "2", "--rank-prefix"], tmp_path)
    lines = [re.sub(r"^\[rank \d\] ", "", l) for l in two.splitlines() if "adversarial" in l]
    assert lines == [line] * 2
