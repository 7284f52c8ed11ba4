"""Per-sample predictions on the CPU path: TrainProgram.predict against a plain torch module,
load_predictor from a checkpoint, and the --predict-out flag of the CLI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, free_port
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.models.reference import MODULES
from pytorch_distributed_mnist_amd.runtime.program import build_local_program
from pytorch_distributed_mnist_amd.utils.checkpoint import best_path, make_state, save_checkpoint

N_TEST = 300          # one forward of 256 rows and a ragged one of 44


@pytest.mark.parametrize("arch", ["linear", "cnn"])
def test_cpu_predict_matches_plain_torch(arch):
    """predict() on the test split == an independent forward of the torch module holding the
    same weights: log_probs to 1e-6 (the parity test's checkpoint bound), pred and the
    confusion matrix exactly; the matrix's trace is evaluate()'s correct count."""
    train, test = synthetic_split(256, True), synthetic_split(N_TEST, False)
    p = build_local_program(arch, "fp32", "cpu", 256, train, test, seed=7)
    before = p.metrics.buf.clone()
    out = p.predict()
    assert torch.equal(p.metrics.buf, before)              # the accumulators are not touched
    module = MODULES[arch]()
    module.load_state_dict({k[len("module."):]: v for k, v in p.arena.state_dict().items()})
    with torch.no_grad():
        want = torch.log_softmax(module(normalize_reference(test.images)), 1)
    assert out.log_probs.dtype == torch.float32 and tuple(out.log_probs.shape) == (N_TEST, 10)
    assert out.pred.dtype == torch.int64 and tuple(out.pred.shape) == (N_TEST,)
    assert (out.log_probs - want).abs().max().item() <= 1e-6
    assert torch.equal(out.pred, want.argmax(1))
    y = test.labels
    assert out.confusion.dtype == torch.int64
    assert torch.equal(out.confusion, torch.bincount(10 * y + out.pred, minlength=100).view(10, 10))
    assert out.confusion.sum().item() == N_TEST
    _, acc = p.evaluate()
    assert out.confusion.trace().item() == acc.correct


def _trained_checkpoint(tmp_path, arch):
    train, test = synthetic_split(256, True), synthetic_split(N_TEST, False)
    p = build_local_program(arch, "fp32", "cpu", 64, train, test, optimizer="sgd", lr=0.05, seed=3)
    p.set_train_indices(distributed_indices(len(train), 1, 0, 0))
    p.train_epoch()
    save_checkpoint(make_state(1, p.arena, 0.5, p.optimizer), True, 0, directory=str(tmp_path))
    return p, test


@pytest.mark.parametrize("arch", ["linear", "cnn"])
def test_load_predictor_round_trip(tmp_path, arch):
    """One short epoch, model_best written as the app writes it; load_predictor reproduces the
    program's predictions exactly, without labels there is no confusion matrix, and NumPy
    [N, 28, 28] input works."""
    from pytorch_distributed_mnist_amd.predict import load_predictor
    p, test = _trained_checkpoint(tmp_path, arch)
    want = p.predict()
    pr = load_predictor(best_path(str(tmp_path)), arch, device="cpu")
    got = pr.predict(test.images, test.labels)
    assert torch.equal(got.log_probs, want.log_probs)
    assert torch.equal(got.pred, want.pred)
    assert torch.equal(got.confusion, want.confusion)
    un = pr.predict(test.images.numpy().reshape(N_TEST, 28, 28)[:37])
    assert un.confusion is None
    assert torch.equal(un.pred, want.pred[:37])
    assert torch.equal(un.log_probs, want.log_probs[:37])
    lab = pr.predict(test.images.numpy()[:1], test.labels.numpy()[:1])        # N = 1, NumPy labels
    assert lab.confusion.sum().item() == 1
    assert lab.confusion[test.labels[0], want.pred[0]].item() == 1


def test_load_predictor_rejects_other_arch(tmp_path):
    from pytorch_distributed_mnist_amd.predict import load_predictor
    _trained_checkpoint(tmp_path, "linear")
    with pytest.raises(RuntimeError, match="Error\\(s\\) in loading state_dict"):
        load_predictor(best_path(str(tmp_path)), "cnn", device="cpu")


def _cli(args, cwd):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(REPO, "multi_proc_single_gpu.py"), "--device", "cpu",
           "--backend", "gloo", "-i", f"tcp://127.0.0.1:{free_port()}", "--synthetic"] + args
    return subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=300)


def test_cli_predict_out(tmp_path):
    """--evaluate --resume CKPT --predict-out P: the file, the ten class lines after the
    unchanged eval line."""
    _trained_checkpoint(tmp_path, "linear")
    ck = best_path(str(tmp_path))
    base = ["--optimizer", "sgd", "--evaluate", "--resume", ck]
    plain = _cli(base, tmp_path)
    assert plain.returncode == 0, plain.stdout + plain.stderr
    out = tmp_path / "sub" / "pred.npz"
    r = _cli(base + ["--predict-out", str(out)], tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    ev = [l for l in plain.stdout.splitlines() if l.startswith("test loss:")]
    lines = r.stdout.splitlines()
    assert len(ev) == 1 and "class 0" not in plain.stdout
    i = lines.index(ev[0])                                      # the same eval line
    cls = lines[i + 1:]
    assert len(cls) == 10
    with np.load(out) as z:
        assert sorted(z.files) == ["confusion", "labels", "log_probs", "pred"]
        lp, pred, lab, conf = z["log_probs"], z["pred"], z["labels"], z["confusion"]
    n = 10000
    assert lp.shape == (n, 10) and lp.dtype == np.float32
    assert pred.shape == (n,) and pred.dtype == np.int64
    assert lab.shape == (n,) and lab.dtype == np.int64
    assert conf.shape == (10, 10) and conf.dtype == np.int64
    assert np.array_equal(lab, synthetic_split(n, False).labels.numpy())
    assert np.array_equal(lp[np.arange(n), pred], lp.max(1))
    assert np.array_equal(conf, np.bincount(10 * lab + pred, minlength=100).reshape(10, 10))
    for c, line in enumerate(cls):
        m = re.fullmatch(r"class (\d): (\d+)/(\d+) \((\d+\.\d{2})%\)", line)
        assert m and int(m.group(1)) == c, line
        assert (int(m.group(2)), int(m.group(3))) == (conf[c, c], conf[c].sum())
        assert m.group(4) == "{:.2f}".format(100.0 * conf[c, c] / conf[c].sum())
    acc = re.search(r"test acc: (\d+\.\d{2})%", ev[0]).group(1)
    assert acc == "{:.2f}".format(100.0 * conf.trace() / n)
    assert not [f for f in os.listdir(out.parent) if f.startswith(".tmp_pred_")]


def test_cli_predict_out_needs_evaluate(tmp_path):
    r = _cli(["--predict-out", str(tmp_path / "p.npz"), "--epochs", "1"], tmp_path)
    assert r.returncode != 0
    assert "--predict-out" in r.stderr and "--evaluate" in r.stderr
    assert not (tmp_path / "p.npz").exists()
