"""Label smoothing (--label-smoothing E) on the host: one CPU training step against an fp64
evaluation of the definition written out here, the floor of the smoothed loss, the plain NLL
of the test line, the flag absent / 0, world-size invariance, resume, --evaluate and the usage
errors.

The definition (torch's F.cross_entropy(logits, y, label_smoothing=E), mean reduction, C = 10):
    t_c = (1 - E) [c = y] + E / C
    row loss = lse - ((1 - E) l_y + E mean_c l_c)
    dlogits_c = (softmax_c - t_c) / B
"""
import math
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import REPO, free_port

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import batch_bounds, distributed_indices
from pytorch_distributed_mnist_amd.models.reference import functional_forward
from pytorch_distributed_mnist_amd.runtime.cpu_step import eval_step_cpu
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

NCLS = 10


def entropy_floor(e):
    """H(E): the entropy of a smoothed target, which no row's smoothed loss can go below."""
    on, off = 1.0 - e + e / NCLS, e / NCLS
    return -on * math.log(on) - (NCLS - 1) * (off * math.log(off) if off > 0 else 0.0)


def smoothed_loss_fp64(logits, y, e):
    """(mean loss, target) from the definition, in the dtype of `logits` (fp64 here)."""
    t = torch.full_like(logits, e / NCLS)
    t[torch.arange(len(y)), y] += 1.0 - e
    lse = torch.logsumexp(logits, 1)
    ly = logits[torch.arange(len(y)), y]
    row = lse - ((1.0 - e) * ly + e * logits.mean(1))
    return row.mean(), t


def rel(a, b):
    return ((a.double() - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize("e", [0.1, 1.0])
@pytest.mark.parametrize("arch", ["cnn", "linear"])
def test_cpu_step_matches_the_definition(arch, e):
    """One train_step_cpu at B = 5: the gradients in the arena and the metric loss against the
    fp64 evaluation of the definition (autograd through the fp64 model for the layers below the
    logits; dlogits itself against (softmax - t) / B), at 1e-5 relative: fp32 autograd against
    fp64."""
    B = 5
    train, test = synthetic_split(64, True), synthetic_split(16, False)
    p = build_local_program(arch, "fp32", "cpu", B, train, test, optimizer="sgd", lr=0.0,
                            momentum=0.0, weight_decay=0.0, seed=3, label_smoothing=e)
    assert p.label_smoothing == e
    idx = distributed_indices(len(train), 1, 0, 0)[:B]
    tp = {k: v.clone() for k, v in p.arena.torch_tensors(p.arena.params).items()}
    p.set_train_indices(idx)
    tl, ta = p.train_epoch()
    got = p.arena.torch_tensors(p.arena.grads)
    x, y = normalize_reference(train.images[idx]).double(), train.labels[idx]
    leaves = {k: v.double().requires_grad_() for k, v in tp.items()}
    logits = functional_forward(arch, leaves, x)
    logits.retain_grad()
    loss, t = smoothed_loss_fp64(logits, y, e)
    loss.backward()
    # dlogits of the definition
    want_dl = (torch.softmax(logits.detach(), 1) - t) / B
    assert rel(logits.grad, want_dl) <= 1e-12
    assert abs(t.sum(1) - 1.0).max() <= 1e-15
    for name, leaf in leaves.items():
        r = rel(got[name], leaf.grad)
        print(f"{arch} E={e} {name}: {r:.2e}")
        assert r <= 1e-5, (name, r)
    print(f"{arch} E={e} loss: {tl.average} vs {loss.item()}")
    assert abs(tl.average - loss.item()) <= 1e-5 * abs(loss.item())
    assert tl.average >= entropy_floor(e) - 1e-6
    assert ta.correct == int((logits.argmax(1) == y).sum())
    # the hard-target loss of the same rows is another number
    hard = (torch.logsumexp(logits, 1) - logits[torch.arange(B), y]).mean().item()
    assert abs(hard - loss.item()) > 1e-3


def test_program_rejects_values_outside_0_1():
    train, test = synthetic_split(16, True), synthetic_split(16, False)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="label_smoothing"):
            build_local_program("linear", "fp32", "cpu", 8, train, test, label_smoothing=bad)


def test_flag_parsing_and_usage_errors(capsys):
    a = parse_args(["--label-smoothing", "0.1"])
    assert a.label_smoothing == 0.1 and "label_smoothing=0.1" in repr(a)
    a = parse_args([])
    assert not hasattr(a, "label_smoothing") and "label_smoothing" not in repr(a)
    for arch in ("linear", "cnn"):
        for opt in ("adam", "sgd"):
            for v in ("0", "1", "0.25"):
                got = parse_args(["--arch", arch, "--optimizer", opt, "--label-smoothing", v])
                assert got.label_smoothing == float(v)
    for bad in ("-0.1", "1.5", "nan", "x"):
        with pytest.raises(SystemExit) as ex:
            parse_args(["--label-smoothing", bad])
        assert ex.value.code == 2, bad
        assert "error: argument --label-smoothing" in capsys.readouterr().err, bad


# ---- the CLI on CPU / gloo -----------------------------------------------------------------

CNN = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.01", "--batch-size", "64",
       "--synthetic-size", "256"]
SMOOTH = ["--label-smoothing", "0.1", "--dropout", "0.25"]
LINEAR = ["--batch-size", "64", "--synthetic-size", "512"]
EPOCH_RE = re.compile(r"^Epoch: (\d+)/(\d+), train loss: (\d+\.\d+), train acc: (\d+\.\d+)%, "
                      r"test loss: (\d+\.\d+), test acc: (\d+\.\d+)%\.$")


def _run_cli(args, cwd, timeout=600, ok=True):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(REPO, "multi_proc_single_gpu.py"), "--device", "cpu",
           "--backend", "gloo", "-i", f"tcp://127.0.0.1:{free_port()}", "--synthetic"] + args
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert (r.returncode == 0) == ok, r.stdout + r.stderr
    assert ok or r.returncode == 2, r.returncode
    return r.stdout if ok else r.stderr


def _weights(d, name="checkpoint_0.pth.tar"):
    return torch.load(d / "checkpoints" / name, weights_only=True)


def _same_checkpoint(a, b):
    assert a["epoch"] == b["epoch"] and a["best_acc"] == b["best_acc"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["optimizer"]["state"][i][name])), \
                (i, name)


def _plain_test_loss(arch, state_dict, batch):
    """The plain NLL of the test split under the saved weights, as the epoch loop evaluates it:
    eval_step_cpu batch by batch."""
    test = synthetic_split(10000, False)
    p = build_local_program(arch, "fp32", "cpu", batch, synthetic_split(batch, True), test)
    p.arena.load_state_dict(state_dict)
    buf = torch.zeros(3, dtype=torch.float64)
    for start, size in batch_bounds(len(test), batch):
        eval_step_cpu(arch, p.arena, test.images[start:start + size],
                      test.labels[start:start + size], buf)
    assert buf[2].item() == len(test)
    return buf[0].item() / len(test)


@pytest.fixture(scope="module")
def cnn_runs(tmp_path_factory):
    """The CNN runs several tests read: two epochs straight, and one epoch (world size 1), with
    --label-smoothing 0.1 --dropout 0.25."""
    d1, d2 = tmp_path_factory.mktemp("straight"), tmp_path_factory.mktemp("one")
    common = CNN + ["--seed", "3"] + SMOOTH
    straight = _run_cli(common + ["--epochs", "2"], d1)
    _run_cli(common + ["--epochs", "1"], d2)
    return common, d1, straight, d2


def test_cli_train_loss_floor_and_plain_test_loss(cnn_runs, tmp_path):
    """Every printed training loss of a --label-smoothing 0.1 run is at least H(0.1) - 1e-6 (a
    smoothed row loss cannot go below its target's entropy, about 0.500), and the test loss
    of the same line is the plain NLL of the saved weights: CNN (with dropout alongside) and
    Linear."""
    H = entropy_floor(0.1)
    assert abs(H - 0.500) < 1e-3
    _, d1, straight, _ = cnn_runs
    assert "label_smoothing=0.1" in straight          # the Namespace line shows the given flag
    lin = _run_cli(LINEAR + ["--seed", "2", "--lr", "0.05", "--epochs", "2", "--label-smoothing",
                             "0.1"], tmp_path)
    for arch, out, d, batch, n in (("cnn", straight, d1, 64, 2), ("linear", lin, tmp_path, 64, 2)):
        ep = [EPOCH_RE.match(l) for l in out.splitlines() if l.startswith("Epoch:")]
        assert len(ep) == n and all(ep), out
        for m in ep:
            print(arch, m.group(0))
            assert float(m.group(3)) >= H - 1e-6, m.group(0)
        ck = _weights(d, f"checkpoint_{n - 1}.pth.tar")
        want = _plain_test_loss(arch, ck["state_dict"], batch)
        assert abs(float(ep[-1].group(5)) - want) <= 1e-6, (ep[-1].group(0), want)


def test_cli_flag_absent_equals_zero(tmp_path):
    """No flag and --label-smoothing 0 print the same lines (but the Namespace line, which shows
    a given flag) and write the same checkpoint bits; --label-smoothing 0.1 does not."""
    dirs = [tmp_path / n for n in ("none", "zero", "on")]
    outs = []
    for d, extra in zip(dirs, ([], ["--label-smoothing", "0"], ["--label-smoothing", "0.1"])):
        d.mkdir()
        out = _run_cli(LINEAR + ["--seed", "5", "--epochs", "1"] + extra, d).splitlines()
        out = [l for l in out if not l.startswith("[Gloo]")]     # (the transport's own chatter)
        assert len(out) >= 3 and out[-1].startswith("Epoch: 0/1,")
        outs.append(out)
    assert outs[0][0].startswith("Namespace(") and "label_smoothing" not in outs[0][0]
    assert "label_smoothing=0.0" in outs[1][0]
    assert outs[0][1:] == outs[1][1:]
    assert outs[0][1:] != outs[2][1:]
    a, b, c = (_weights(d) for d in dirs)
    _same_checkpoint(a, b)
    assert not torch.equal(a["state_dict"]["module.fc.weight"], c["state_dict"]["module.fc.weight"])
    assert a.keys() == c.keys() and a["optimizer"].keys() == c["optimizer"].keys()   # same format


@pytest.mark.slow
def test_cli_world_size_invariance(cnn_runs, tmp_path):
    """World size 1 and 2 (gloo) with --label-smoothing 0.1 --dropout 0.25 train the same
    weights (tests/test_dropout_cpu.py's comparison and tolerance)."""
    common, _, _, d2 = cnn_runs
    _run_cli(common + ["--epochs", "1", "--world-size", "2"], tmp_path)
    a, b = _weights(d2)["state_dict"], _weights(tmp_path)["state_dict"]
    for k in a:
        assert torch.allclose(a[k], b[k], atol=1e-6, rtol=0), (k, (a[k] - b[k]).abs().max())


def test_cli_resume_and_evaluate(cnn_runs):
    """Two epochs straight equal one epoch plus --resume for the second, the flag given again;
    --evaluate prints the same line with and without the flag."""
    common, d1, straight, d2 = cnn_runs
    out = _run_cli(common + ["--epochs", "2", "--resume",
                             str(d2 / "checkpoints" / "checkpoint_0.pth.tar")], d2)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 1 and ep[0].startswith("Epoch: 1/2,")
    assert ep[0] == [l for l in straight.splitlines() if l.startswith("Epoch: 1/2,")][0]
    _same_checkpoint(_weights(d1, "checkpoint_1.pth.tar"), _weights(d2, "checkpoint_1.pth.tar"))
    ck = str(d1 / "checkpoints" / "checkpoint_1.pth.tar")
    lines = []
    for extra in ([], ["--label-smoothing", "0.1"]):
        ev = _run_cli(CNN + ["--evaluate", "--resume", ck] + extra, d1)
        line = [l for l in ev.splitlines() if l.startswith("test loss:")]
        assert len(line) == 1
        lines.append(line[0])
    assert lines[0] == lines[1]
    assert lines[0].split("test loss: ")[1] == ep[0].split("test loss: ")[1]


def test_cli_usage_errors(tmp_path):
    for bad in ("-0.1", "1.5"):
        err = _run_cli(["--label-smoothing", bad], tmp_path, ok=False)
        assert "error: argument --label-smoothing" in err and "usage:" in err, err
