"""Dropout on the CNN's hidden layer, on the host (data/dropout.py): the integer mask against a
per-unit re-implementation of its spec, the kept share, its dependence on (seed, epoch, index,
unit), the --dropout flags, and the CLI on CPU/gloo (world-size invariance, resume, --dropout 0,
evaluation without a mask).  Philox itself is pinned to the Random123 vectors by
tests/test_augment_cpu.py."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import REPO, free_port

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.augment import philox4x32_10
from pytorch_distributed_mnist_amd.data.dropout import (DropoutSpec, keep_mask, multiplier,
                                                        spec_from_args, tag_labels)
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import batch_bounds, distributed_indices
from pytorch_distributed_mnist_amd.models.reference import MODULES, functional_forward
from pytorch_distributed_mnist_amd.runtime.program import build_local_program


def _unit(i, e, n, seed, T, stream=1):
    """One unit's keep bit, straight from the spec."""
    r = philox4x32_10(np.array([i, e, stream, n >> 3], dtype=np.uint64),
                      np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
    word = int(r[(n >> 1) & 3])
    u = (word >> 16) if n & 1 else (word & 0xFFFF)
    return 1 if u >= T else 0


@pytest.mark.parametrize("p", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("seed", [0, (7 << 32) + 12345])
def test_keep_mask_matches_the_spec(p, seed):
    spec = DropoutSpec(p, seed)
    T = int(round(p * 65536))
    assert spec.T == T and spec.enabled == (T > 0)
    assert spec.scale == float(np.float32(65536.0 / (65536.0 - T)))
    idx = [0, 1, 59999]
    for e in (0, 7):
        got = keep_mask(idx, e, spec)
        assert got.dtype == np.uint8 and got.shape == (3, 128)
        want = np.array([[_unit(i, e, n, seed, T) for n in range(128)] for i in idx], dtype=np.uint8)
        assert np.array_equal(got, want), (p, seed, e)
        if p == 0.0:
            assert got.all()                                 # p = 0 keeps everything
    m = multiplier(torch.tensor(idx), 7, spec)
    assert m.dtype == torch.float32 and m.shape == (3, 128)
    assert torch.equal(m, torch.from_numpy(keep_mask(idx, 7, spec)).float() * spec.scale)


@pytest.mark.parametrize("p", [0.5, 0.25])
def test_kept_share(p):
    """60000 x 128 draws: the kept share is within 5 sigma of 1 - T / 65536."""
    spec = DropoutSpec(p, seed=3)
    keep = keep_mask(np.arange(60000), 2, spec)
    n = keep.size
    q = 1.0 - spec.T / 65536.0
    sigma = math.sqrt(q * (1.0 - q) / n)
    share = float(keep.mean(dtype=np.float64))
    print(f"\np={p}: kept {share:.6f}, expected {q:.6f}, sigma {sigma:.2e}")
    assert n == 60000 * 128 and abs(share - q) <= 5.0 * sigma, (share, q, sigma)


def test_mask_depends_on_epoch_seed_and_stream():
    spec = DropoutSpec(0.5, seed=9)
    idx = np.arange(64)
    base = keep_mask(idx, 0, spec)
    assert np.array_equal(base, keep_mask(idx, 0, spec))
    assert not np.array_equal(base, keep_mask(idx, 1, spec))                     # the epoch
    assert not np.array_equal(base, keep_mask(idx, 0, DropoutSpec(0.5, seed=10)))
    assert not np.array_equal(base, keep_mask(idx, 0, spec, stream=0))            # word 2: the
    assert not np.array_equal(base[0], base[1])                                  # augmentation's
    # a sample's mask does not depend on the batch it is drawn in
    assert np.array_equal(keep_mask(idx[10:20], 0, spec), base[10:20])


def test_spec_and_tags():
    for bad in (-0.1, 0.91, float("nan")):
        with pytest.raises(ValueError):
            DropoutSpec(bad)
    assert DropoutSpec(0.9).T == 58982 and not DropoutSpec(0.0).enabled
    assert not DropoutSpec(1e-6).enabled                     # rounds to T = 0: off
    lab = torch.tensor([3, 9, 0, 7])
    t = tag_labels(lab)
    assert t.dtype == torch.int32 and t.tolist() == [3, 9 | 16, 0 | 32, 7 | 48]
    assert torch.equal(t & 15, lab.to(torch.int32)) and torch.equal(t >> 4, torch.arange(4).int())
    with pytest.raises(ValueError):
        tag_labels(torch.tensor([16]))


def test_cli_flags(capsys):
    a = parse_args(["--arch", "cnn", "--dropout", "0.5", "--dropout-seed", "77"])
    assert (a.dropout, a.dropout_seed) == (0.5, 77)
    assert spec_from_args(a) == DropoutSpec(0.5, 77)
    a = parse_args([])
    assert not hasattr(a, "dropout") and not hasattr(a, "dropout_seed") and "dropout" not in repr(a)
    assert spec_from_args(a) is None
    assert spec_from_args(parse_args(["--arch", "cnn", "--dropout", "0"])) is None
    assert spec_from_args(parse_args(["--arch", "cnn", "--dropout-seed", "4"])) is None
    assert spec_from_args(parse_args(["--arch", "cnn", "--dropout", "0.2"])).seed == 0
    assert spec_from_args(parse_args(["--arch", "cnn", "--dropout", "0.2", "--seed", "6"])).seed == 6
    s = spec_from_args(parse_args(["--arch", "cnn", "--dropout", "0.2", "--seed", "6",
                                   "--dropout-seed", "8"]))
    assert s == DropoutSpec(0.2, 8)
    parse_args(["--arch", "linear", "--dropout", "0"])       # off: nothing to object to
    for bad in (["--arch", "cnn", "--dropout", "0.91"], ["--arch", "cnn", "--dropout", "-0.1"],
                ["--arch", "cnn", "--dropout", "nan"], ["--arch", "cnn", "--dropout-seed", "-1"],
                ["--arch", "linear", "--dropout", "0.5"], ["--dropout", "0.5"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert "error: argument --dropout" in capsys.readouterr().err, bad


def test_program_needs_the_epoch_and_a_hidden_layer():
    train, test = synthetic_split(64, True), synthetic_split(32, False)
    spec = DropoutSpec(0.5, seed=1)
    with pytest.raises(ValueError, match="hidden"):
        build_local_program("linear", "fp32", "cpu", 32, train, test, dropout=spec)
    p = build_local_program("cnn", "fp32", "cpu", 32, train, test, dropout=spec)
    idx = distributed_indices(len(train), 1, 0, 0)
    with pytest.raises(ValueError, match="epoch"):
        p.set_train_indices(idx)
    q = build_local_program("cnn", "fp32", "cpu", 32, train, test, dropout=DropoutSpec(0.0, 1))
    assert q.dropout is None
    q.set_train_indices(idx)                                 # off: no epoch needed


def test_cpu_step_applies_the_mask_and_evaluation_does_not():
    """One CPU training step with dropout equals autograd of the masked forward written out
    here; a program without dropout, and one at another epoch, leave other weights; evaluate()
    and predict() give what they give without dropout."""
    train, test = synthetic_split(64, True), synthetic_split(48, False)
    spec = DropoutSpec(0.5, seed=5)
    idx = distributed_indices(len(train), 1, 0, 0)
    out = {}
    for name, sp, ep in (("drop", spec, 3), ("other epoch", spec, 4), ("plain", None, 3)):
        p = build_local_program("cnn", "fp32", "cpu", 32, train, test, optimizer="sgd", lr=0.1,
                                momentum=0.0, weight_decay=0.0, seed=2, dropout=sp)
        if name == "drop":
            net = MODULES["cnn"]()
            net.load_state_dict({k[len("module."):]: v for k, v in p.arena.state_dict().items()})
            ev0 = p.evaluate()[0].average
            pr0 = p.predict().log_probs
        elif name == "plain":
            assert p.evaluate()[0].average == ev0 and torch.equal(p.predict().log_probs, pr0)
        p.set_train_indices(idx[:32], epoch=ep)
        p.train_epoch()
        out[name] = {k[len("module."):]: v.clone() for k, v in p.arena.state_dict().items()}
    sel = idx[:32]
    x = normalize_reference(train.images[sel]).view(32, 1, 28, 28)
    h = F.relu(net.fc1(torch.flatten(F.max_pool2d(F.relu(net.conv2(F.relu(net.conv1(x)))), 2), 1)))
    keep = torch.from_numpy(keep_mask(sel, 3, spec)).float()
    assert 0.3 < keep.mean() < 0.7
    F.cross_entropy(net.fc2(h * keep * spec.scale), train.labels[sel]).backward()
    for name, prm in net.named_parameters():
        want = prm.detach() - 0.1 * prm.grad
        assert torch.allclose(out["drop"][name], want, atol=1e-6, rtol=0), name
    assert not torch.allclose(out["drop"]["fc2.weight"], out["plain"]["fc2.weight"], atol=1e-6)
    assert not torch.allclose(out["drop"]["fc2.weight"], out["other epoch"]["fc2.weight"], atol=1e-6)


DROP = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.01", "--batch-size", "64",
        "--synthetic-size", "256"]


def _run_cli(args, cwd, timeout=600, ok=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(REPO, "multi_proc_single_gpu.py"), "--device", "cpu",
           "--backend", "gloo", "-i", f"tcp://127.0.0.1:{free_port()}", "--synthetic"] + args
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    return r.stdout if ok else r.stderr


def _weights(d, name="checkpoint_0.pth.tar"):
    return torch.load(d / "checkpoints" / name, weights_only=True)


@pytest.mark.slow
def test_cli_world_size_invariance_with_dropout(tmp_path):
    """World size 1 and 2 with --dropout 0.5 draw the same masks for the same samples: the same
    weights (tests/test_augment_cpu.py's comparison), and not those of a run without."""
    dirs = [tmp_path / n for n in ("ws1", "ws2", "plain")]
    for d in dirs:
        d.mkdir()
    common = DROP + ["--epochs", "1", "--seed", "11"]
    _run_cli(common + ["--dropout", "0.5", "--world-size", "1"], dirs[0])
    _run_cli(common + ["--dropout", "0.5", "--world-size", "2"], dirs[1])
    _run_cli(common + ["--world-size", "1"], dirs[2])
    a, b, c = (_weights(d)["state_dict"] for d in dirs)
    for k in a:
        assert torch.allclose(a[k], b[k], atol=1e-6, rtol=0), (k, (a[k] - b[k]).abs().max())
    assert not torch.allclose(a["module.fc2.weight"], c["module.fc2.weight"], atol=1e-6, rtol=0)


def test_cli_resume_and_evaluate_with_dropout(tmp_path):
    """Two epochs straight equal one epoch plus --resume for the second (the flag given
    again): the masks depend on the epoch number, not on the process that draws them.  The
    printed test loss is that of a forward pass with no mask, and --evaluate ignores the
    flag."""
    d1, d2 = tmp_path / "straight", tmp_path / "resumed"
    d1.mkdir()
    d2.mkdir()
    common = DROP + ["--seed", "3", "--dropout", "0.5"]
    straight = _run_cli(common + ["--epochs", "2"], d1)
    assert "dropout=0.5" in straight                 # the Namespace line shows the given flag
    _run_cli(common + ["--epochs", "1"], d2)
    out = _run_cli(common + ["--epochs", "2", "--resume",
                             str(d2 / "checkpoints" / "checkpoint_0.pth.tar")], d2)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 1 and ep[0].startswith("Epoch: 1/2,")
    a, b = _weights(d1, "checkpoint_1.pth.tar"), _weights(d2, "checkpoint_1.pth.tar")
    assert a["epoch"] == b["epoch"] == 2 and a["best_acc"] == b["best_acc"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["optimizer"]["state"][i][name])), \
                (i, name)
    # the epoch line's test loss: the plain forward of the saved weights, batch by batch
    ep1 = [l for l in straight.splitlines() if l.startswith("Epoch: 1/2")][0]
    printed = float(re.search(r"test loss: (\d+\.\d+)", ep1).group(1))
    test = synthetic_split(10000, False)
    params = {k[len("module."):]: v for k, v in a["state_dict"].items()}
    total = 0.0
    with torch.no_grad():
        for start, size in batch_bounds(len(test), 64):
            logits = functional_forward("cnn", params,
                                        normalize_reference(test.images[start:start + size]))
            total += F.cross_entropy(logits, test.labels[start:start + size]).item() * size
    assert abs(printed - total / len(test)) <= 1e-6, (printed, total / len(test))
    ev = _run_cli(DROP + ["--dropout", "0.5", "--evaluate", "--resume",
                          str(d1 / "checkpoints" / "checkpoint_1.pth.tar")], d1)
    line = [l for l in ev.splitlines() if l.startswith("test loss:")]
    assert len(line) == 1 and line[0].split("test loss: ")[1] == ep1.split("test loss: ")[1]


def test_cli_dropout_zero_is_no_flag_and_linear_is_an_error(tmp_path):
    """--dropout 0 trains bit-identical weights to no flag at all; --arch linear --dropout 0.5
    exits with the argparse error."""
    d1, d2 = tmp_path / "zero", tmp_path / "none"
    d1.mkdir()
    d2.mkdir()
    common = DROP + ["--epochs", "1", "--seed", "5"]
    _run_cli(common + ["--dropout", "0"], d1)
    _run_cli(common, d2)
    a, b = _weights(d1), _weights(d2)
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["optimizer"]["state"][i][name]))
    err = _run_cli(["--arch", "linear", "--dropout", "0.5"], d1, ok=False)
    assert "error: argument --dropout" in err and "usage:" in err
