"""Per-step learning-rate schedules on the host (optim/schedule.py): the run's table against a
NumPy re-implementation of the formulas, its exact points (end of warmup, final rate, the
reference's per-epoch decay), the --lr-* flags and their usage errors, the CPU step, and the CLI
on CPU/gloo (defaults bit-identical, world-size invariance at equal steps per epoch, resume,
the checkpoint's learning rate)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, free_port

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.optim.flat import adjust_learning_rate
from pytorch_distributed_mnist_amd.optim.schedule import KINDS, ScheduleSpec, spec_from_args
from pytorch_distributed_mnist_amd.runtime.program import build_local_program


def _numpy_table(kind, lr0, epochs, spe, W, m):
    """The issue's formulas, vectorised (np.cos, not math.cos)."""
    T = epochs * spe
    g = np.arange(T, dtype=np.int64)
    p = np.maximum(g - W, 0).astype(np.float64) / max(1, T - 1 - W)
    if kind == "step":
        base = lr0 * np.power(0.1, ((g // spe) // 10).astype(np.float64))
    elif kind == "constant":
        base = np.full(T, lr0, dtype=np.float64)
    elif kind == "linear":
        base = lr0 * (m + (1.0 - m) * (1.0 - p))
    else:
        base = lr0 * (m + (1.0 - m) * 0.5 * (1.0 + np.cos(np.pi * p)))
    ramp = (g + 1).astype(np.float64) / max(W, 1)
    return np.where(g < W, base * ramp, base), base


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W", [0, 1, 7, 30])
def test_table_matches_the_formulas(kind, W):
    lr0, epochs, spe = 0.05, 23, 9                    # 23 epochs: two decades of `step`
    m = 0.1 if kind in ("linear", "cosine") else 0.0
    spec = ScheduleSpec(kind, lr0, epochs, spe, W, m)
    t = spec.table()
    T = epochs * spe
    assert t.dtype == np.float64 and t.shape == (T,) and spec.total == T
    assert spec.table() is t and not t.flags.writeable         # computed once
    want, base = _numpy_table(kind, lr0, epochs, spe, W, m)
    rel = np.abs(t - want) / np.abs(want)
    print(f"\n{kind} W={W}: max rel err {rel.max():.3e}")
    assert rel.max() <= 1e-12
    assert [spec.lr(g) for g in range(T)] == t.tolist()
    if W:
        assert t[W - 1] == spec.base(W - 1)                     # exactly: the ramp ends at 1
        assert np.all(np.diff(t[:W]) > 0) and t[0] > 0          # strictly increasing
        assert abs(t[0] - base[0] / W) <= 1e-12 * base[0]
    if kind in ("linear", "cosine"):
        assert abs(t[-1] - lr0 * m) <= 1e-12 * lr0 * m
        assert np.all(np.diff(t[W:]) < 0)                       # the anneal never rises
        assert t[W] == lr0
    if kind == "constant":
        assert np.all(t[W:] == lr0)


def test_final_rate_zero_and_one():
    for kind in ("linear", "cosine"):
        assert ScheduleSpec(kind, 0.1, 3, 4, 2, 0.0).table()[-1] == 0.0
        assert np.all(ScheduleSpec(kind, 0.1, 3, 4, 0, 1.0).table() == 0.1)


def test_step_is_the_reference_decay():
    """`step` with warmup 1 (a ramp of one step, factor exactly 1) holds the reference's
    per-epoch values exactly; `step` with warmup 0 gives no spec at all."""
    from types import SimpleNamespace
    args = parse_args(["--lr", "0.003", "--epochs", "31", "--lr-warmup", "1"])
    spe = 4
    spec = spec_from_args(args, spe)
    assert spec == ScheduleSpec("step", 0.003, 31, spe, 1, 0.0)
    opt = SimpleNamespace(param_groups=[{"lr": None}])
    t = spec.table()
    for epoch in range(31):
        adjust_learning_rate(opt, epoch, args)
        assert np.all(t[epoch * spe:(epoch + 1) * spe] == opt.param_groups[0]["lr"]), epoch
    assert spec_from_args(parse_args(["--epochs", "31"]), spe) is None
    assert spec_from_args(parse_args(["--lr-schedule", "step", "--lr-warmup", "0"]), spe) is None
    assert spec_from_args(parse_args(["--lr-schedule", "constant"]), spe) is not None


def test_cli_flags_and_usage_errors(capsys):
    a = parse_args(["--lr-schedule", "cosine", "--lr-warmup", "3", "--lr-min", "0.1", "--lr", "0.2",
                    "--epochs", "2"])
    assert (a.lr_schedule, a.lr_warmup, a.lr_min) == ("cosine", 3, 0.1)
    assert spec_from_args(a, 5) == ScheduleSpec("cosine", 0.2, 2, 5, 3, 0.1)
    a = parse_args([])
    assert not any(hasattr(a, k) for k in ("lr_schedule", "lr_warmup", "lr_min"))
    assert "lr_" not in repr(a)                       # the Namespace line is unchanged
    for bad in (["--lr-schedule", "cosine", "--lr-min", "1.5"],
                ["--lr-schedule", "cosine", "--lr-min", "-0.1"],
                ["--lr-schedule", "linear", "--lr-min", "nan"],
                ["--lr-min", "0.1"], ["--lr-schedule", "step", "--lr-min", "0.1"],
                ["--lr-schedule", "constant", "--lr-min", "0.1"],
                ["--lr-warmup", "-1"], ["--lr-schedule", "exp"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert "error: argument --lr-" in capsys.readouterr().err, bad
    # warmup against the run's steps, known once the steps per epoch are: T = 2 * 5
    ok = spec_from_args(parse_args(["--epochs", "2", "--lr-warmup", "9"]), 5)
    assert ok.warmup == 9 and ok.total == 10
    for w in ("10", "11"):
        with pytest.raises(ValueError, match="argument --lr-warmup"):
            spec_from_args(parse_args(["--epochs", "2", "--lr-warmup", w]), 5)
    for kw in (dict(lr_min=1.5), dict(lr_min=0.5, kind="step"), dict(kind="exp"), dict(warmup=-1)):
        with pytest.raises(ValueError):
            ScheduleSpec(**{**dict(kind="cosine", lr0=0.1, epochs=2, spe=5), **kw})


def test_cpu_program_sets_every_steps_rate(monkeypatch):
    """The CPU path sets param_groups[0]['lr'] = table[epoch * spe + i] before each optimizer
    step, whatever epoch it is started at, and needs the epoch number."""
    train, test = synthetic_split(100, True), synthetic_split(32, False)
    spec = ScheduleSpec("cosine", 0.1, 3, 4, 3, 0.1)          # 100 / 32: 3 full steps + a tail
    p = build_local_program("linear", "fp32", "cpu", 32, train, test, optimizer="sgd", lr=0.1,
                            schedule=spec)
    seen = []
    step_cpu = p.optimizer.step_cpu
    monkeypatch.setattr(p.optimizer, "step_cpu",
                        lambda **kw: (seen.append(p.optimizer.param_groups[0]["lr"]), step_cpu(**kw)))
    idx = distributed_indices(len(train), 1, 0, 0)
    with pytest.raises(ValueError, match="epoch"):
        p.set_train_indices(idx)
    for epoch in (0, 2):                                      # (a resume skips epoch 1)
        p.set_train_indices(idx, epoch=epoch)
        p.train_epoch()
    t = spec.table().tolist()
    assert seen == t[0:4] + t[8:12]
    assert p.optimizer.param_groups[0]["lr"] == t[11]
    with pytest.raises(ValueError, match="schedule"):
        p.set_train_indices(idx, epoch=3)                     # past the run
    with pytest.raises(ValueError, match="schedule"):
        p.set_train_indices(idx[:64], epoch=0)                # another steps-per-epoch


# 500 samples: 7 full batches and a ragged tail at world size 1 (batch 64, tail 52) and at world
# size 2 (batch 32, tail 26): 8 steps per epoch either way
SIZE = ["--synthetic-size", "500", "--batch-size", "64"]
SPE = 8


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


def _assert_same_checkpoint(a, b):
    assert a["epoch"] == b["epoch"] and a["best_acc"] == b["best_acc"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    assert a["optimizer"]["state"].keys() == b["optimizer"]["state"].keys()
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["optimizer"]["state"][i][name])), \
                (i, name)
    assert a["optimizer"]["param_groups"] == b["optimizer"]["param_groups"]


def test_cli_defaults_are_no_flags(tmp_path):
    """--lr-schedule step --lr-warmup 0 is the run without the flags, bit for bit (and its
    checkpoint's rate the reference's); a warmup that does not fit the run is a usage error."""
    d1, d2 = tmp_path / "none", tmp_path / "explicit"
    d1.mkdir()
    d2.mkdir()
    common = SIZE + ["--epochs", "1", "--seed", "5", "--lr", "0.002"]
    _run_cli(common, d1)
    out = _run_cli(common + ["--lr-schedule", "step", "--lr-warmup", "0"], d2)
    assert "lr_schedule='step'" in out                # the Namespace line shows the given flags
    a, b = _ckpt(d1), _ckpt(d2)
    _assert_same_checkpoint(a, b)
    assert a["optimizer"]["param_groups"][0]["lr"] == 0.002
    err = _run_cli(common + ["--lr-warmup", str(SPE)], d1, ok=False)
    assert "error: argument --lr-warmup" in err and "usage:" in err
    err = _run_cli(common + ["--lr-schedule", "constant", "--lr-min", "0.5"], d1, ok=False)
    assert "error: argument --lr-min" in err and "usage:" in err


@pytest.mark.slow
def test_cli_world_size_invariance_with_a_schedule(tmp_path):
    """World size 1 and 2 with the same steps per epoch follow the same schedule: the same
    weights (tests/test_app_cpu.py's comparison), and not those of a run without."""
    dirs = [tmp_path / n for n in ("ws1", "ws2", "plain")]
    for d in dirs:
        d.mkdir()
    common = SIZE + ["--epochs", "1", "--seed", "11", "--lr", "0.01"]
    sched = ["--lr-schedule", "cosine", "--lr-warmup", "3", "--lr-min", "0.1"]
    _run_cli(common + sched + ["--world-size", "1"], dirs[0])
    _run_cli(common + sched + ["--world-size", "2"], dirs[1])
    _run_cli(common + ["--world-size", "1"], dirs[2])
    a, b, c = (_ckpt(d) for d in dirs)
    for k in a["state_dict"]:
        x, y = a["state_dict"][k], b["state_dict"][k]
        assert torch.allclose(x, y, atol=1e-6, rtol=0), (k, (x - y).abs().max())
    assert not torch.allclose(a["state_dict"]["module.fc.weight"], c["state_dict"]["module.fc.weight"],
                              atol=1e-6, rtol=0)
    want = ScheduleSpec("cosine", 0.01, 1, SPE, 3, 0.1).table()[-1]
    assert a["optimizer"]["param_groups"][0]["lr"] == want
    assert b["optimizer"]["param_groups"][0]["lr"] == want


def test_cli_resume_continues_the_schedule(tmp_path):
    """A run resumed from the first epoch's checkpoint, the flags given again, ends where the
    uninterrupted run does, bit for bit; the checkpoints hold the rate of their last step.
    Cosine's table depends on --epochs, so that run resumes the straight run's first checkpoint
    in a fresh process; a constant rate behind a warmup does not, so there the first leg is a
    run of its own with --epochs 1."""
    sched = ["--lr-schedule", "cosine", "--lr-warmup", "3", "--lr-min", "0.1"]
    common = SIZE + ["--seed", "3", "--lr", "0.01"]
    d1, d2 = tmp_path / "straight", tmp_path / "resumed"
    d1.mkdir()
    d2.mkdir()
    _run_cli(common + sched + ["--epochs", "2"], d1)
    out = _run_cli(common + sched + ["--epochs", "2", "--resume",
                                     str(d1 / "checkpoints" / "checkpoint_0.pth.tar")], d2)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 1 and ep[0].startswith("Epoch: 1/2,")
    a0, a1, b1 = _ckpt(d1), _ckpt(d1, "checkpoint_1.pth.tar"), _ckpt(d2, "checkpoint_1.pth.tar")
    _assert_same_checkpoint(a1, b1)
    t = ScheduleSpec("cosine", 0.01, 2, SPE, 3, 0.1).table()
    assert a0["optimizer"]["param_groups"][0]["lr"] == t[SPE - 1]
    assert a1["optimizer"]["param_groups"][0]["lr"] == t[2 * SPE - 1] == b1["optimizer"]["param_groups"][0]["lr"]

    sched = ["--lr-schedule", "constant", "--lr-warmup", "5"]
    d3, d4 = tmp_path / "straight2", tmp_path / "resumed2"
    d3.mkdir()
    d4.mkdir()
    _run_cli(common + sched + ["--epochs", "2"], d3)
    _run_cli(common + sched + ["--epochs", "1"], d4)
    _run_cli(common + sched + ["--epochs", "2", "--resume",
                               str(d4 / "checkpoints" / "checkpoint_0.pth.tar")], d4)
    _assert_same_checkpoint(_ckpt(d3), _ckpt(d4))
    _assert_same_checkpoint(_ckpt(d3, "checkpoint_1.pth.tar"), _ckpt(d4, "checkpoint_1.pth.tar"))
    assert _ckpt(d4, "checkpoint_1.pth.tar")["optimizer"]["param_groups"][0]["lr"] == 0.01
