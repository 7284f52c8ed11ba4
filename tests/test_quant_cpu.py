"""int8 evaluation (--quantize int8, --arch mlp / mlp2) on the CPU path, and the oracles shared with
tests/test_gpu_quant.py: the definition one float32 operation at a time, and the quantised model
(W = s1 q1) in float64 with fc1's measure carried to the output (docs/kernels.md "int8 evaluation":
e = |got - ref| / s <= K 2^-24, K = 164 / 293 roundings).  Measured here: e = 2.0e-9 / 3.2e-10."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.runtime.cpu_step import quantize_fc1
from pytorch_distributed_mnist_amd.runtime.program import build_local_program
from test_dropout_cpu import _run_cli

F, D = np.float32, np.float64
ALPHA, GAMMA = 1.0 / (255.0 * 0.3081), 128.0 / (255.0 * 0.3081) - 0.1307 / 0.3081
SETS = ("trained", "zero row", "negative max", "ties")


def weight_set(kind):
    """An arena stub of float32 fc1.weight [128 x 784] / fc1.bias of trained magnitude; row 5 all
    zero; row 7's largest magnitude negative; row 9 with s1 = 1 exactly and weights on .5 ties."""
    g = torch.Generator().manual_seed(3)
    w, b = torch.randn(128, 784, generator=g) * 0.05, torch.randn(128, generator=g) * 0.1
    if kind == "zero row":
        w[5] = 0
    if kind == "negative max":
        w[7, 100] = -1.0
    if kind == "ties":
        w[9], w[9, :9] = 0, torch.tensor([127.0, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, 126.5])
    return SimpleNamespace(param={"fc1.weight": w.reshape(-1), "fc1.bias": b}.__getitem__)


def definition(w, b):
    q = dict(q1=np.zeros((128, 784), np.int8), r1=np.zeros(128, np.int32),
             **{k: np.zeros(128, F) for k in ("s1", "c1", "d1")})
    for n in range(128):
        m = max(abs(v) for v in w[n])
        s = F(1) if m == 0 else m / F(127)
        q["q1"][n] = [int(min(max(np.rint(v / s), F(-127)), F(127))) for v in w[n]]
        r = sum(int(v) for v in q["q1"][n])
        q["s1"][n], q["r1"][n], q["c1"][n], q["d1"][n] = s, r, F(ALPHA) * s, b[n] + (s * F(r)) * F(GAMMA)
    return q


@pytest.mark.parametrize("kind", SETS)
def test_quantize_fc1(kind):
    arena = weight_set(kind)
    w, got = arena.param("fc1.weight").numpy().reshape(128, 784), quantize_fc1(arena)
    for k, v in definition(w, arena.param("fc1.bias").numpy()).items():
        assert got[k].dtype == v.dtype and np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), k
    q, live = got["q1"].astype(np.int64), np.abs(w).max(1) > 0
    assert (np.abs(q).max(1)[live] == 127).all() and np.array_equal(q.sum(1), got["r1"])
    assert live.sum() == 128 - (kind == "zero row") and (q[~live] == 0).all() and (got["s1"][~live] == 1).all()
    assert kind != "ties" or q[9, :9].tolist() == [127, 0, 2, 2, 0, -2, -2, 4, 126]
    assert kind != "negative max" or (q[7, 100] == -127 and q[7].max() < 127)


def check_forward(tag, arch, arena, x, log_probs, pred):
    """log_probs / pred of the int8 path on the bytes x against the float64 quantised model."""
    P = {p.name: p.to_torch(arena.param(p.name)).detach().cpu().double().numpy() for p in arena.spec.params}
    q = quantize_fc1(arena)
    W, x8 = q["s1"].astype(D)[:, None] * q["q1"], x.numpy().astype(D) - 128
    h = ALPHA * x8 @ W.T + GAMMA * W.sum(1) + P["fc1.bias"]
    s = ALPHA * np.abs(x8) @ np.abs(W).T + np.abs(GAMMA * W.sum(1)) + np.abs(P["fc1.bias"])
    for name in ("fc2", "fc3")[:1 + (arch == "mlp2")]:
        w, b = P[name + ".weight"], P[name + ".bias"]
        h, s = np.maximum(h, 0) @ w.T + b, s @ np.abs(w).T + np.abs(b)
    ref = h - np.log(np.exp(h - h.max(1, keepdims=True)).sum(1, keepdims=True)) - h.max(1, keepdims=True)
    e = (np.abs(log_probs.double().numpy() - ref) / (s + s.max(1, keepdims=True) + np.log(10.0))).max()
    bound = (13 + 8 + 129 * (1 + (arch == "mlp2")) + 14) * 2.0 ** -24
    print(f"{tag} {arch}: e = {e:.2e} (bound {bound:.2e})")
    assert e <= bound and np.array_equal(pred.numpy(), ref.argmax(1))


@pytest.mark.parametrize("arch", ["mlp", "mlp2"])
def test_cpu_forward(arch):
    prog = build_local_program(arch, "fp32", "cpu", 8, synthetic_split(64, True), synthetic_split(21, False), seed=5)
    x, y = prog.test_split.images, prog.test_split.labels
    p = prog.predict(x, y, quantize="int8")
    check_forward("cpu", arch, prog.arena, x, p.log_probs, p.pred)
    assert int(p.confusion.sum()) == 21 and not torch.equal(p.log_probs, prog.predict(x, y).log_probs)


def test_usage_errors(capsys):
    assert parse_args(["--evaluate", "--arch", "mlp2", "--quantize", "int8"]).quantize == "int8"
    assert "quantize" not in repr(parse_args([]))
    ev = ["--evaluate", "--arch", "mlp", "--quantize", "int8"]
    for bad, word in ((ev[1:], "--quantize"), (["--evaluate"] + ev[3:], "no int8 kernel"),
                      (["--evaluate", "--arch", "cnn"] + ev[3:], "no int8 kernel"),
                      (ev[:4] + ["int4"], "--quantize"), (ev + ["--attack-eps", "8"], "--quantize"),
                      (ev + ["--tta", "2", "--aug-shift", "1"], "--quantize")):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    for arch, kind in (("linear", "int8"), ("mlp", "int4")):
        with pytest.raises(ValueError, match="no int8 kernel"):
            build_local_program(arch, "fp32", "cpu", 8, synthetic_split(8, True),
                                synthetic_split(8, False)).predict(quantize=kind)


INT8_RE = re.compile(r"int8 \(fc1: per-row weights, exact pixels\) loss: (\d+\.\d{6}), acc: (\d+\.\d{2})%\.$")


def int8_line_matches_file(lines, npz):
    """The one int8 line of a run's stdout, right behind the test line, its numbers recomputed from
    the file's int8_* arrays: (line, the file)."""
    i, = [i for i, l in enumerate(lines) if l.startswith("int8")]
    m, z = INT8_RE.match(lines[i]), np.load(npz)
    lp, y, hits = z["int8_log_probs"], z["labels"], int((z["int8_pred"] == z["labels"]).sum())
    assert lines[i - 1].startswith("test loss:") and int(np.trace(z["int8_confusion"])) == hits
    assert m.group(1) == "{:.6f}".format(float((-lp[np.arange(len(y)), y]).astype(D).sum()) / len(y))
    assert m.group(2) == "{:.2f}".format(100.0 * hits / len(y))
    return lines[i], z


@pytest.mark.parametrize("arch", ["mlp", "mlp2"])
def test_cli(tmp_path, arch):
    """No flag: today's stdout and .npz keys; with it one more line and three more arrays and
    nothing else differs; world size 2 prints world size 1's line."""
    _run_cli(["--arch", arch, "--optimizer", "sgd", "--lr", "0.05", "--batch-size", "64",
              "--synthetic-size", "256", "--epochs", "1", "--seed", "3"], tmp_path)
    ev = ["--arch", arch, "--optimizer", "sgd", "--evaluate", "--resume",
          str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar"), "--predict-out"]
    plain = _run_cli(ev + [str(tmp_path / "p.npz")], tmp_path).splitlines()
    quant = _run_cli(ev + [str(tmp_path / "q.npz"), "--quantize", "int8"], tmp_path).splitlines()
    line, z = int8_line_matches_file(quant, tmp_path / "q.npz")
    quant.remove(line)
    assert [l for l in quant if l[:10] != "Namespace("] == [l for l in plain if l[:10] != "Namespace("]
    pz = np.load(tmp_path / "p.npz")
    assert sorted(pz.files) == ["confusion", "labels", "log_probs", "pred"]
    assert sorted(z.files) == sorted(pz.files + ["int8_confusion", "int8_log_probs", "int8_pred"])
    assert np.array_equal(z["log_probs"], pz["log_probs"]) and not np.array_equal(z["int8_log_probs"], z["log_probs"])
    two = _run_cli(ev[:-1] + ["--quantize", "int8", "--world-size", "2", "--rank-prefix"], tmp_path)
    assert [l[9:] for l in two.splitlines() if "int8 (" in l] == [line] * 2
