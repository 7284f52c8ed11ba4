"""MXFP4 evaluation (--quantize mxfp4, --arch mlp / mlp2) on the CPU path, and the oracles shared
with tests/test_gpu_mxfp4.py: the definition one scalar at a time, and the float64 model on the
dequantised weights with fc1's summed-magnitude measure carried to the output (docs/kernels.md
"MXFP4 evaluation": e = |got - ref| / s <= K 2^-24, K = 2 (2 * 896 + 2) half-ulps for fc1's sum,
8 for the fold and the bias, 129 per later layer, 14 for the log-softmax, as the int8 test's)."""
import math
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.runtime.cpu_step import quantize_fc1_mxfp4
from pytorch_distributed_mnist_amd.runtime.program import build_local_program
from test_dropout_cpu import _run_cli
from test_quant_cpu import ALPHA, weight_set

F, D = np.float32, np.float64
BETA = 0.1307 / 0.3081
GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
TIES = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
SETS = ("trained", "edges")


def mx_weight_set(kind):
    """test_quant_cpu's trained arena stub; "edges": row 5 with an all-zero block 3, row 6 block 2
    with the maximum 2^-3, row 7 a negative maximum, row 9 block 0 on X = 1 with every tie
    midpoint of both signs and the saturating range (6, 8), row 10 block 1 on X = 2^-5 likewise,
    row 11 its maximum in the 16-element tail block, row 12 an all-zero tail."""
    a = weight_set("trained")
    w = a.param("fc1.weight").clone().reshape(128, 784)
    if kind == "edges":
        w[5, 96:128] = 0
        w[6, 64:96] = w[6, 64:96].clamp(-0.1, 0.1)
        w[6, 70] = 0.125
        w[7, 100] = -1.0
        pat = torch.tensor(TIES + [-t for t in TIES] + [6.0, 6.5, 7.5, -7.999, -0.2, 0.26, 5.01, 0.0])
        w[9, :32], w[9, :len(pat)] = 0, pat
        w[10, 32:64], w[10, 32:32 + len(pat)] = 0, pat / 32
        w[11, 783], w[12, 768:] = -3.0, 0
    return SimpleNamespace(param={"fc1.weight": w.reshape(-1), "fc1.bias": a.param("fc1.bias")}.__getitem__)


def definition(w, b):
    """The spec, scalar by scalar: Python floats (doubles) hold every intermediate exactly."""
    codes, scales = np.zeros((128, 896), np.uint8), np.zeros((128, 28), np.uint8)
    wq, d1 = np.zeros((128, 896), F), np.zeros(128, F)
    for n in range(128):
        r = F(0)
        for blk in range(28):
            ws = [float(v) for v in w[n, 32 * blk:32 * blk + 32]]
            m = max([abs(v) for v in ws], default=0.0)
            e8 = 127 if m == 0 else min(max(math.frexp(m)[1] - 1 - 2 + 127, 0), 254)
            scales[n, blk], X, tot = e8, 2.0 ** (e8 - 127), 0.0
            for j, v in enumerate(ws):
                a = abs(v) / X
                # nearest grid point; of two equally near ones the even code (mantissa bit 0)
                c = min(range(8), key=lambda c: (abs(a - GRID[c]), c & 1))
                neg = v < 0 and c != 0
                codes[n, 32 * blk + j] = c | (8 if neg else 0)
                wq[n, 32 * blk + j] = (-GRID[c] if neg else GRID[c]) * X
                tot += float(wq[n, 32 * blk + j])
            assert float(F(tot)) == tot             # the spec's claim: a block's sum is exact
            if blk < 25:
                r = r + F(tot) if blk else F(tot)
        t = F(BETA) * r
        d1[n] = b[n] - t
    return {"codes": codes[:, 0::2] | (codes[:, 1::2] << 4), "scales": scales, "wq": wq[:, :784], "d1": d1}


@pytest.mark.parametrize("kind", SETS)
def test_quantize_fc1_mxfp4(kind):
    arena = mx_weight_set(kind)
    w, got = arena.param("fc1.weight").numpy().reshape(128, 784), quantize_fc1_mxfp4(arena)
    for k, v in definition(w, arena.param("fc1.bias").numpy()).items():
        assert got[k].dtype == v.dtype and got[k].shape == v.shape, k
        assert np.array_equal(got[k].view(np.uint8), v.view(np.uint8)), k
    assert (got["codes"][:, 392:] == 0).all() and (got["scales"][:, 25:] == 127).all()
    if kind == "edges":
        nib = lambda n, k: int(got["codes"][n, k // 2] >> (4 * (k & 1))) & 15   # noqa: E731
        assert [nib(9, k) for k in range(22)] == [0, 2, 2, 4, 4, 6, 6, 0, 10, 10, 12, 12, 14, 14,
                                                  7, 7, 7, 15, 0, 1, 7, 0]
        assert [nib(10, 32 + k) for k in range(22)] == [nib(9, k) for k in range(22)]
        assert got["scales"][[9, 10, 6, 5, 12], [0, 1, 2, 3, 24]].tolist() == [127, 122, 122, 127, 127]
        assert nib(7, 100) == 14 and nib(11, 783) == 15 and nib(6, 70) == 6


def check_forward_mx(tag, arch, arena, x, log_probs, pred):
    """log_probs / pred of the MXFP4 path on the bytes x against the float64 model on wq."""
    P = {p.name: p.to_torch(arena.param(p.name)).detach().cpu().double().numpy() for p in arena.spec.params}
    W, x8 = quantize_fc1_mxfp4(arena)["wq"].astype(D), x.numpy().astype(D).reshape(-1, 784)
    h = ALPHA * x8 @ W.T - BETA * W.sum(1) + P["fc1.bias"]
    s = ALPHA * x8 @ np.abs(W).T + np.abs(BETA * W.sum(1)) + np.abs(P["fc1.bias"])
    for name in ("fc2", "fc3")[:1 + (arch == "mlp2")]:
        w, b = P[name + ".weight"], P[name + ".bias"]
        h, s = np.maximum(h, 0) @ w.T + b, s @ np.abs(w).T + np.abs(b)
    ref = h - np.log(np.exp(h - h.max(1, keepdims=True)).sum(1, keepdims=True)) - h.max(1, keepdims=True)
    e = (np.abs(log_probs.double().numpy() - ref) / (s + s.max(1, keepdims=True) + np.log(10.0))).max()
    bound = (2 * (2 * 896 + 2) + 8 + 129 * (1 + (arch == "mlp2")) + 14) * 2.0 ** -24
    print(f"{tag} {arch}: e = {e:.2e} (bound {bound:.2e})")
    assert e <= bound and np.array_equal(pred.numpy(), ref.argmax(1))


@pytest.mark.parametrize("arch", ["mlp", "mlp2"])
def test_cpu_forward(arch):
    prog = build_local_program(arch, "fp32", "cpu", 8, synthetic_split(64, True), synthetic_split(21, False), seed=5)
    x, y = prog.test_split.images, prog.test_split.labels
    p = prog.predict(x, y, quantize="mxfp4")
    check_forward_mx("cpu", arch, prog.arena, x, p.log_probs, p.pred)
    assert int(p.confusion.sum()) == 21
    for other in (None, "int8"):
        assert not torch.equal(p.log_probs, prog.predict(x, y, quantize=other).log_probs)


def test_usage_errors(capsys):
    ev = ["--evaluate", "--arch", "mlp", "--quantize", "mxfp4"]
    assert parse_args(ev).quantize == "mxfp4"
    for bad, word in ((ev[1:], "--quantize"), (["--evaluate"] + ev[3:], "no mxfp4 kernel"),
                      (["--evaluate", "--arch", "cnn"] + ev[3:], "no mxfp4 kernel"),
                      (ev + ["--attack-eps", "8"], "--quantize"),
                      (ev + ["--tta", "2", "--aug-shift", "1"], "--quantize")):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    with pytest.raises(ValueError, match="no mxfp4 kernel"):
        build_local_program("linear", "fp32", "cpu", 8, synthetic_split(8, True),
                            synthetic_split(8, False)).predict(quantize="mxfp4")


MX_RE = re.compile(r"mxfp4 \(fc1: 32-weight blocks, exact pixels\) loss: (\d+\.\d{6}), acc: (\d+\.\d{2})%\.$")


def mxfp4_line_matches_file(lines, npz):
    """The one mxfp4 line of a run's stdout, right behind the test line, its numbers recomputed
    from the file's mxfp4_* arrays: (line, the file)."""
    i, = [i for i, l in enumerate(lines) if l.startswith("mxfp4")]
    m, z = MX_RE.match(lines[i]), np.load(npz)
    lp, y, hits = z["mxfp4_log_probs"], z["labels"], int((z["mxfp4_pred"] == z["labels"]).sum())
    assert lines[i - 1].startswith("test loss:") and int(np.trace(z["mxfp4_confusion"])) == hits
    assert m.group(1) == "{:.6f}".format(float((-lp[np.arange(len(y)), y]).astype(D).sum()) / len(y))
    assert m.group(2) == "{:.2f}".format(100.0 * hits / len(y))
    return lines[i], z


def test_cli(tmp_path):
    """No flag: today's stdout and .npz keys; with it one more line and three more arrays and
    nothing else differs; world size 2 prints world size 1's line."""
    _run_cli(["--arch", "mlp", "--optimizer", "sgd", "--lr", "0.05", "--batch-size", "64",
              "--synthetic-size", "256", "--epochs", "1", "--seed", "3"], tmp_path)
    ev = ["--arch", "mlp", "--optimizer", "sgd", "--evaluate", "--resume",
          str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar"), "--predict-out"]
    plain = _run_cli(ev + [str(tmp_path / "p.npz")], tmp_path).splitlines()
    quant = _run_cli(ev + [str(tmp_path / "q.npz"), "--quantize", "mxfp4"], tmp_path).splitlines()
    line, z = mxfp4_line_matches_file(quant, tmp_path / "q.npz")
    quant.remove(line)
    assert [l for l in quant if l[:10] != "Namespace("] == [l for l in plain if l[:10] != "Namespace("]
    pz = np.load(tmp_path / "p.npz")
    assert sorted(pz.files) == ["confusion", "labels", "log_probs", "pred"]
    assert sorted(z.files) == sorted(pz.files + ["mxfp4_confusion", "mxfp4_log_probs", "mxfp4_pred"])
    assert np.array_equal(z["log_probs"], pz["log_probs"]) and not np.array_equal(z["mxfp4_log_probs"], z["log_probs"])
    two = _run_cli(ev[:-1] + ["--quantize", "mxfp4", "--world-size", "2", "--rank-prefix"], tmp_path)
    assert [l[9:] for l in two.splitlines() if "mxfp4 (" in l] == [line] * 2
