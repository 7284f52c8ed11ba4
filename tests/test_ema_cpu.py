"""The exponential moving average of the weights on the host (optim/ema.py, --ema-decay /
--ema-warmup): the update's weight against a NumPy re-evaluation, the CPU path's average against a
float32 NumPy replay over the per-step weights, and the CLI on CPU/gloo -- the flag off changes
nothing, the flag on leaves training untouched, world-size invariance, resume, which weights an
evaluation reads, the usage errors and --shard-fc."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, free_port

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.optim.ema import EmaSpec, ema_weight, spec_from_args
from pytorch_distributed_mnist_amd.runtime.program import build_local_program
from pytorch_distributed_mnist_amd.utils.checkpoint import make_state


def _numpy_weight(D, k, warmup):
    """The issue's definition: d_k in fp64, w = float32(1 - d_k)."""
    d = np.float64(D)
    if warmup:
        d = np.minimum(d, (np.float64(1.0) + np.float64(k)) / (np.float64(10.0) + np.float64(k)))
    return np.float32(np.float64(1.0) - d)


def _first_k_at_decay(D):
    k = 1
    while (1.0 + k) / (10.0 + k) < D:
        k += 1
    return k


def numpy_ema(e, p, w):
    """e + w (p - e) in three float32 roundings."""
    w = np.float32(w)
    return (e + (w * (p - e)).astype(np.float32)).astype(np.float32)


@pytest.mark.parametrize("D", [0.5, 0.9, 0.999, 1.0 - 2.0 ** -20])
def test_weight_without_warmup(D):
    w = ema_weight(D)
    assert isinstance(w, float) and np.float32(w) == w           # a float32 value
    assert np.float32(w) == np.float32(1.0 - D) == _numpy_weight(D, 1, False)
    assert ema_weight(D, 12345) == w and EmaSpec(D).weight(7) == w


@pytest.mark.parametrize("D", [0.9, 0.999])
def test_weight_with_warmup(D):
    kd = _first_k_at_decay(D)
    assert {0.9: 80, 0.999: 8990}[D] == kd       # (1 + k) / (10 + k) = D exactly: 81 / 90, 8991 / 9000
    for k in (1, 2, 9, kd - 1, kd, kd + 1, 10 * kd):
        w = ema_weight(D, k, warmup=True)
        assert np.float32(w) == w and np.float32(w) == _numpy_weight(D, k, True), k
    assert ema_weight(D, 1, True) == float(np.float32(1.0 - 2.0 / 11.0))
    assert ema_weight(D, kd - 1, True) > ema_weight(D, kd, True) == ema_weight(D) \
        == ema_weight(D, 10 * kd, True)
    with pytest.raises(ValueError):
        ema_weight(D, 0, True)


def test_cli_flags_and_usage_errors(capsys):
    a = parse_args(["--ema-decay", "0.99", "--ema-warmup"])
    assert a.ema_decay == 0.99 and a.ema_warmup is True
    assert spec_from_args(a) == EmaSpec(0.99, True)
    assert spec_from_args(parse_args(["--ema-decay", "0.5"])) == EmaSpec(0.5, False)
    a = parse_args([])
    assert not hasattr(a, "ema_decay") and not hasattr(a, "ema_warmup")
    assert "ema" not in repr(a)                       # the Namespace line is unchanged
    assert spec_from_args(a) is None
    assert spec_from_args(parse_args(["--ema-decay", "0"])) is None        # 0 = off
    for bad in (["--ema-decay", "-0.5"], ["--ema-decay", "1"], ["--ema-decay", "1.5"],
                ["--ema-decay", "nan"], ["--ema-decay", "x"], ["--ema-warmup"],
                ["--ema-decay", "0", "--ema-warmup"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert "error: argument --ema-" in capsys.readouterr().err, bad
    for D in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(ValueError):
            EmaSpec(D)


@pytest.mark.parametrize("warmup", [False, True])
def test_cpu_average_is_the_numpy_replay(warmup):
    """Three epochs of the Linear model, the program called step by step (a one-batch epoch
    order per call): the final average is the float32 NumPy replay over the per-step weights,
    bit for bit, and so is what the checkpoint would hold."""
    train, test = synthetic_split(100, True), synthetic_split(32, False)
    spec = EmaSpec(0.9, warmup)
    p = build_local_program("linear", "fp32", "cpu", 32, train, test, optimizer="sgd", lr=0.05,
                            ema=spec)
    e = p.arena.params.numpy().copy()
    assert np.array_equal(p.ema.params.numpy(), e) and p.ema.updates == 0
    k = 0
    for epoch in range(3):
        order = distributed_indices(len(train), 1, 0, epoch)
        for s in range(0, len(order), 32):                     # 3 full steps and a tail of 4
            p.set_train_indices(order[s:s + 32], epoch=epoch)
            p.train_epoch()
            k += 1
            e = numpy_ema(e, p.arena.params.numpy(), _numpy_weight(0.9, k, warmup))
    assert k == 12 and p.ema.updates == 12
    assert np.array_equal(p.ema.params.numpy(), e)
    assert not np.array_equal(e, p.arena.params.numpy())
    state = make_state(3, p.arena, 0.0, p.optimizer, p.ema)
    assert list(state) == ["epoch", "state_dict", "best_acc", "optimizer", "ema_state_dict",
                           "ema_updates"]
    assert state["ema_updates"] == 12
    assert list(state["ema_state_dict"]) == list(state["state_dict"])
    w = p.arena.spec.by_name("fc.weight")
    assert np.array_equal(state["ema_state_dict"]["module.fc.weight"].numpy(),
                          w.to_torch(p.ema.arena.param("fc.weight")).numpy())
    assert list(make_state(3, p.arena, 0.0, p.optimizer)) == ["epoch", "state_dict", "best_acc",
                                                               "optimizer"]


def test_cpu_evaluate_reads_the_average_and_touches_nothing():
    train, test = synthetic_split(100, True), synthetic_split(64, False)
    mk = lambda **kw: build_local_program("linear", "fp32", "cpu", 32, train, test,
                                          optimizer="sgd", lr=0.05, seed=2, **kw)
    p, q = mk(ema=EmaSpec(0.9)), mk()
    for prog in (p, q):
        prog.set_train_indices(distributed_indices(len(train), 1, 0, 0), epoch=0)
        prog.train_epoch()
    assert torch.equal(p.arena.params, q.arena.params)        # training untouched
    before = p.arena.params.clone(), p.ema.params.clone()
    avg, plain = p.evaluate(), p.evaluate(average=False)
    assert torch.equal(p.arena.params, before[0]) and torch.equal(p.ema.params, before[1])
    assert plain[0].average == q.evaluate()[0].average != avg[0].average
    q.arena.params.copy_(p.ema.params)                        # the average as training weights
    assert q.evaluate()[0].average == avg[0].average
    assert torch.equal(p.predict().log_probs, q.predict().log_probs)
    assert not torch.equal(p.predict(average=False).log_probs, q.predict().log_probs)
    with pytest.raises(ValueError, match="average"):
        mk().evaluate(average=True)


# ---------------------------------------------------------------------------------------- CLI
LIN = ["--synthetic-size", "500", "--batch-size", "64", "--optimizer", "sgd", "--lr", "0.05"]
CNN = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.01", "--batch-size", "64",
       "--synthetic-size", "256"]


def _run_cli(args, cwd, timeout=600, ok=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(REPO, "multi_proc_single_gpu.py"), "--device", "cpu",
           "--backend", "gloo", "-i", f"tcp://127.0.0.1:{free_port()}", "--synthetic"] + args
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout if ok else r.stderr


def _ckpt(d, name="checkpoint_0.pth.tar"):
    return torch.load(d / "checkpoints" / name, weights_only=True)


def _same_training_state(a, b):
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    assert a["optimizer"]["state"].keys() == b["optimizer"]["state"].keys()
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v),
                               torch.as_tensor(b["optimizer"]["state"][i][name])), (i, name)
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]


def _same_average(a, b):
    assert a["ema_updates"] == b["ema_updates"]
    assert list(a["ema_state_dict"]) == list(b["ema_state_dict"])
    for k, v in a["ema_state_dict"].items():
        assert torch.equal(v, b["ema_state_dict"][k]), k


def _epoch_lines(out):
    return [l for l in out.splitlines() if l.startswith("Epoch:")]


def _no_port(out):
    return re.sub(r"tcp://127\.0\.0\.1:\d+", "tcp://127.0.0.1:PORT", out)


def test_cli_flag_off_and_training_untouched(tmp_path):
    """Without the flag: today's four checkpoint keys, and the stdout of a second run of the same
    command (but the rendezvous port in the Namespace line).  With it: the training weights
    and optimizer state of the run without, bit for bit, the training half of every epoch line
    too, two more keys, and test figures from other weights."""
    dirs = [tmp_path / n for n in ("off", "off2", "on")]
    for d in dirs:
        d.mkdir()
    common = LIN + ["--epochs", "2", "--seed", "5"]
    out1 = _run_cli(common, dirs[0])
    out2 = _run_cli(common, dirs[1])
    out3 = _run_cli(common + ["--ema-decay", "0.9"], dirs[2])
    assert _no_port(out1) == _no_port(out2)
    assert "ema" not in out1
    a, c = _ckpt(dirs[0], "checkpoint_1.pth.tar"), _ckpt(dirs[2], "checkpoint_1.pth.tar")
    assert list(a) == ["epoch", "state_dict", "best_acc", "optimizer"]
    assert list(c) == ["epoch", "state_dict", "best_acc", "optimizer", "ema_state_dict",
                       "ema_updates"]
    _same_training_state(a, c)
    assert c["ema_updates"] == 2 * 8 and type(c["ema_updates"]) is int
    assert list(c["ema_state_dict"]) == list(c["state_dict"])
    assert not torch.equal(c["ema_state_dict"]["module.fc.weight"],
                           c["state_dict"]["module.fc.weight"])
    assert "ema_decay=0.9" in out3
    l1, l3 = _epoch_lines(out1), _epoch_lines(out3)
    assert len(l1) == len(l3) == 2
    for x, y in zip(l1, l3):
        assert x.split(" test loss")[0] == y.split(" test loss")[0]     # the training half
        assert x != y                                                   # the test half


@pytest.mark.slow
def test_cli_world_size_invariance(tmp_path):
    """World sizes 1 and 2 give the same average, by tests/test_app_cpu.py's rule for the
    weights (atol 1e-6: the two all-reduce orders differ in the last bit)."""
    d1, d2 = tmp_path / "ws1", tmp_path / "ws2"
    d1.mkdir()
    d2.mkdir()
    common = LIN + ["--epochs", "1", "--seed", "11", "--ema-decay", "0.9", "--ema-warmup"]
    _run_cli(common + ["--world-size", "1"], d1)
    _run_cli(common + ["--world-size", "2"], d2)
    a, b = _ckpt(d1), _ckpt(d2)
    assert a["ema_updates"] == b["ema_updates"] == 8
    for name in ("state_dict", "ema_state_dict"):
        for k in a[name]:
            x, y = a[name][k], b[name][k]
            assert torch.allclose(x, y, atol=1e-6, rtol=0), (name, k, (x - y).abs().max())
    assert not torch.allclose(a["ema_state_dict"]["module.fc.weight"],
                              a["state_dict"]["module.fc.weight"], atol=1e-6, rtol=0)


def test_cli_resume_continues_the_average(tmp_path):
    """Four epochs uninterrupted equal their first two plus a resumed two: state_dict,
    ema_state_dict, ema_updates and the epoch lines, with dropout and the EMA warmup on (the
    update index has to carry over: at 4 steps per epoch the warmup is still moving)."""
    flags = CNN + ["--seed", "3", "--dropout", "0.5", "--ema-decay", "0.9", "--ema-warmup"]
    d1, d2 = tmp_path / "straight", tmp_path / "resumed"
    d1.mkdir()
    d2.mkdir()
    out1 = _run_cli(flags + ["--epochs", "4"], d1)
    # the second leg in a fresh process and directory, from the straight run's two-epoch state
    out2 = _run_cli(flags + ["--epochs", "4", "--resume",
                             str(d1 / "checkpoints" / "checkpoint_1.pth.tar")], d2)
    assert len(_epoch_lines(out1)) == 4 and _epoch_lines(out1)[2:] == _epoch_lines(out2)
    assert "notice:" not in out2
    assert _ckpt(d1, "checkpoint_1.pth.tar")["ema_updates"] == 8
    for name in ("checkpoint_2.pth.tar", "checkpoint_3.pth.tar"):
        a, b = _ckpt(d1, name), _ckpt(d2, name)
        assert a["epoch"] == b["epoch"] and a["best_acc"] == b["best_acc"]
        _same_training_state(a, b)
        _same_average(a, b)
    assert _ckpt(d2, "checkpoint_3.pth.tar")["ema_updates"] == 16


def test_cli_evaluation_source_and_resume_without_an_average(tmp_path):
    """The epoch's test line is --evaluate --resume checkpoint --ema-decay D, and not
    --evaluate without the flag; --predict-out follows; a checkpoint without the key is an
    error with the flag, and resumes training with one notice line and a fresh average."""
    d, plain = tmp_path / "ema", tmp_path / "plain"
    d.mkdir()
    plain.mkdir()
    common = LIN + ["--seed", "7"]
    out = _run_cli(common + ["--epochs", "1", "--ema-decay", "0.9"], d)
    test_half = _epoch_lines(out)[0].split(", test loss")[1]
    ck = str(d / "checkpoints" / "checkpoint_0.pth.tar")
    ev = _run_cli(common + ["--evaluate", "--resume", ck, "--ema-decay", "0.9", "--predict-out",
                            str(d / "avg.npz")], d)
    line = [l for l in ev.splitlines() if l.startswith("test loss")]
    assert len(line) == 1 and line[0] == "test loss" + test_half
    ev2 = _run_cli(common + ["--evaluate", "--resume", ck, "--predict-out", str(d / "raw.npz")], d)
    line2 = [l for l in ev2.splitlines() if l.startswith("test loss")]
    assert len(line2) == 1 and line2[0] != line[0]
    assert not np.array_equal(np.load(d / "avg.npz")["log_probs"],
                              np.load(d / "raw.npz")["log_probs"])

    from pytorch_distributed_mnist_amd.predict import load_predictor
    from pytorch_distributed_mnist_amd.data.mnist import load_split
    images = load_split("data", False, synthetic=True).images[:32]    # the CLI's test split
    avg = load_predictor(ck, "linear", device="cpu", ema=True).predict(images)
    raw = load_predictor(ck, "linear", device="cpu").predict(images)
    assert np.array_equal(avg.log_probs.numpy(), np.load(d / "avg.npz")["log_probs"][:32])
    assert np.array_equal(raw.log_probs.numpy(), np.load(d / "raw.npz")["log_probs"][:32])

    _run_cli(common + ["--epochs", "1"], plain)
    ck0 = str(plain / "checkpoints" / "checkpoint_0.pth.tar")
    err = _run_cli(common + ["--evaluate", "--resume", ck0, "--ema-decay", "0.9"], plain, ok=False)
    assert "ema_state_dict" in err and "Traceback" not in err
    with pytest.raises(KeyError, match="ema_state_dict"):
        load_predictor(ck0, "linear", device="cpu", ema=True)
    out = _run_cli(common + ["--epochs", "2", "--resume", ck0, "--ema-decay", "0.9"], plain)
    notice = [l for l in out.splitlines() if l.startswith("notice:")]
    assert len(notice) == 1 and "no averaged weights" in notice[0]
    assert _ckpt(plain, "checkpoint_1.pth.tar")["ema_updates"] == 8


def test_cli_usage_errors(tmp_path):
    for bad in (["--ema-decay", "-0.5"], ["--ema-decay", "1"], ["--ema-decay", "1.0001"],
                ["--ema-warmup"]):
        err = _run_cli(bad, tmp_path, ok=False)
        assert "error: argument --ema-" in err and "usage:" in err, bad


@pytest.mark.slow
def test_cli_shard_fc_runs_unsharded(tmp_path):
    """--shard-fc with the average at gloo world size 2: the existing warning, once, naming
    the average; the run goes on unsharded and writes its average."""
    common = CNN + ["--epochs", "1", "--seed", "2", "--world-size", "2", "--ema-decay", "0.9"]
    out = _run_cli(common + ["--shard-fc"], tmp_path)
    warn = [l for l in out.splitlines() if l.startswith("warning: --shard-fc:")]
    assert len(warn) == 1 and "--ema-decay" in warn[0] and warn[0].endswith("running unsharded")
    ck = _ckpt(tmp_path)
    # 128 samples per rank in batches of 32; every rank prints its epoch line
    assert ck["ema_updates"] == 4 and len(_epoch_lines(out)) == 2
