"""2:4 sparse evaluation (--quantize sparse24) on the CPU path, and the oracles shared with
tests/test_gpu_sparse24.py: the rule group by group, and the float64 model on the pruned weights
(docs/kernels.md "2:4 sparse evaluation": the carried measure and its bound)."""
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.runtime.cpu_step import prune_fc1_24
from pytorch_distributed_mnist_amd.runtime.program import build_local_program
from test_dropout_cpu import _run_cli
from test_quant_cpu import ALPHA, weight_set

D, BETA, SETS = np.float64, 0.1307 / 0.3081, ("trained", "crafted")
PAIRS, T = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)], np.arange(196)
WORD, SHIFT = (T >> 5) * 4 + ((T >> 2) & 3), 16 * ((T >> 4) & 1) + 4 * (T & 3)   # group t's nibble


def sp_weight_set(kind):
    """test_quant_cpu's trained stub; "crafted": in every wave and unit tile, in both index halves and
    the last k-steps: the six position pairs, a zero group, ties of both signs, a negative maximum."""
    a = weight_set("trained")
    w = a.param("fc1.weight").clone().reshape(128, 196, 4)
    if kind == "crafted":
        pat = torch.full((10, 4), 0.01)
        for t, (i, j) in enumerate(PAIRS):
            pat[t, i], pat[t, j] = 0.5, -0.25
        pat[6:] = torch.tensor([[0, 0, 0, 0], [0.3, -0.3, 0.3, -0.3], [0.1, 0.3, -0.3, 0.3], [-0.9, 0.1, 0.2, 0.05]])
        for t0 in (0, 16, 182):
            w[[9, 40, 50, 127], t0:t0 + 10] = pat
    return SimpleNamespace(param={"fc1.weight": w.reshape(-1), "fc1.bias": a.param("fc1.bias")}.__getitem__)


def definition(w):
    """The rule, group by group: (wp float32 [128, 784], positions int [128, 196, 2])."""
    wp, pos = np.zeros_like(w), np.zeros((128, 196, 2), np.int64)
    for n in range(128):
        for t in range(196):
            grp = w[n, 4 * t:4 * t + 4]
            pos[n, t] = sorted(sorted(range(4), key=lambda j: (-abs(float(grp[j])), j))[:2])
            wp[n, 4 * t + pos[n, t]] = grp[pos[n, t]]
    return wp, pos


@pytest.mark.parametrize("kind", SETS)
def test_prune_fc1_24(kind):
    arena = sp_weight_set(kind)
    w, got = arena.param("fc1.weight").numpy().reshape(128, 784), prune_fc1_24(arena)
    wp, pos = definition(w)
    assert got["wp"].dtype == np.float32 and np.array_equal(got["wp"].view(np.int32), wp.view(np.int32))
    assert got["index"].shape == (128, 28) and got["index"].dtype == np.int32
    nib = (got["index"].view(np.uint32)[:, WORD] >> SHIFT) & 15
    assert np.array_equal(nib & 3, pos[..., 0]) and np.array_equal(nib >> 2, pos[..., 1]) and (nib & 3 < nib >> 2).all()
    assert (got["index"][:, 25:] == 0).all() and (got["index"].view(np.uint32)[:, 24] >> 16 == 0).all()
    kept = torch.from_numpy(np.take_along_axis(w.reshape(128, 196, 4), pos, axis=2).reshape(128, 392))
    hi = kept.to(torch.bfloat16)
    for name, plane in (("hi", hi), ("lo", (kept - hi.float()).to(torch.bfloat16))):
        assert got[name].shape == (128, 416) and got[name].dtype == np.int16, name
        assert np.array_equal(got[name][:, :392], plane.view(torch.int16).numpy()), name
        assert (got[name][:, 392:] == 0).all(), name
    if kind == "crafted":
        assert {tuple(p) for p in pos[9, :6].tolist()} == set(PAIRS)
        assert pos[9, 6:10].tolist() == pos[127, 188:192].tolist() == [[0, 1], [0, 1], [1, 2], [0, 2]]


def check_forward_sp(tag, arch, arena, x, log_probs, pred):
    """Against the float64 model on wp: e <= K 2^-24 + 2^-18, K = 2 (2 * 416 + 2) for fc1 (two planes
    of 416 terms, the scaling), 8 fold and bias, 129 per later layer, 14 log-softmax, 2^-18 the bf16
    planes; pred's reference log-probability is within twice the bound of the largest (near ties)."""
    P = {p.name: p.to_torch(arena.param(p.name)).detach().cpu().double().numpy() for p in arena.spec.params}
    W, x8 = prune_fc1_24(arena)["wp"].astype(D), x.numpy().astype(D).reshape(-1, 784)
    h = ALPHA * x8 @ W.T - BETA * W.sum(1) + P["fc1.bias"]
    s = ALPHA * x8 @ np.abs(W).T + np.abs(BETA * W.sum(1)) + np.abs(P["fc1.bias"])
    for name in ("fc2", "fc3")[:1 + (arch == "mlp2")]:
        w, b = P[name + ".weight"], P[name + ".bias"]
        h, s = np.maximum(h, 0) @ w.T + b, s @ np.abs(w).T + np.abs(b)
    ref = h - np.log(np.exp(h - h.max(1, keepdims=True)).sum(1, keepdims=True)) - h.max(1, keepdims=True)
    den = s + s.max(1, keepdims=True) + np.log(10.0)
    e = (np.abs(log_probs.double().numpy() - ref) / den).max()
    bound = (2 * (2 * 416 + 2) + 8 + 129 * (1 + (arch == "mlp2")) + 14) * 2.0 ** -24 + 2.0 ** -18
    gap = ref.max(1) - ref[np.arange(len(ref)), pred.numpy()]
    print(f"{tag} {arch}: e = {e:.2e} (bound {bound:.2e}), {int((gap > 0).sum())} near-tie rows "
          f"(largest gap {gap.max():.1e})")
    assert e <= bound and (gap <= 2 * bound * den.max(1)).all()


@pytest.mark.parametrize("arch", ["mlp", "mlp2"])
def test_cpu_forward(arch):
    prog = build_local_program(arch, "fp32", "cpu", 8, synthetic_split(64, True), synthetic_split(21, False), seed=5)
    x, y = prog.test_split.images, prog.test_split.labels
    p = prog.predict(x, y, quantize="sparse24")
    check_forward_sp("cpu", arch, prog.arena, x, p.log_probs, p.pred)
    assert int(p.confusion.sum()) == 21
    for other in (None, "int8", "mxfp4"):
        assert not torch.equal(p.log_probs, prog.predict(x, y, quantize=other).log_probs)


def test_usage_errors(capsys):
    ev = ["--evaluate", "--arch", "mlp", "--quantize", "sparse24"]
    assert parse_args(ev).quantize == "sparse24"
    for bad, word in ((ev[1:], "--quantize"), (["--evaluate"] + ev[3:], "no sparse24 kernel"),
                      (["--evaluate", "--arch", "cnn"] + ev[3:], "no sparse24 kernel"),
                      (ev + ["--attack-eps", "8"], "--quantize"),
                      (ev + ["--tta", "2", "--aug-shift", "1"], "--quantize")):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2 and word in capsys.readouterr().err, bad
    with pytest.raises(ValueError, match="no sparse24 kernel"):
        build_local_program("linear", "fp32", "cpu", 8, synthetic_split(8, True),
                            synthetic_split(8, False)).predict(quantize="sparse24")


SP_RE = re.compile(r"sparse24 \(fc1: 2 of every 4 weights, exact pixels\) loss: (\d+\.\d{6}), acc: (\d+\.\d{2})%\.$")


def sparse24_line_matches_file(lines, npz):
    """The one sparse24 line, right behind the test line, recomputed from the file: (line, file)."""
    i, = [i for i, l in enumerate(lines) if l.startswith("sparse24")]
    m, z = SP_RE.match(lines[i]), np.load(npz)
    lp, y, hits = z["sparse24_log_probs"], z["labels"], int((z["sparse24_pred"] == z["labels"]).sum())
    assert lines[i - 1].startswith("test loss:") and int(np.trace(z["sparse24_confusion"])) == hits
    assert m.group(1) == "{:.6f}".format(float((-lp[np.arange(len(y)), y]).astype(D).sum()) / len(y))
    assert m.group(2) == "{:.2f}".format(100.0 * hits / len(y))
    return lines[i], z


def test_cli(tmp_path):
    """No flag: today's stdout and .npz keys; with it one more line, three more arrays; ws 2 = 1."""
    _run_cli(["--arch", "mlp", "--optimizer", "sgd", "--lr", "0.05", "--batch-size", "64",
              "--synthetic-size", "256", "--epochs", "1", "--seed", "3"], tmp_path)
    ev = ["--arch", "mlp", "--optimizer", "sgd", "--evaluate", "--resume",
          str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar"), "--predict-out"]
    plain = _run_cli(ev + [str(tmp_path / "p.npz")], tmp_path).splitlines()
    quant = _run_cli(ev + [str(tmp_path / "q.npz"), "--quantize", "sparse24"], tmp_path).splitlines()
    line, z = sparse24_line_matches_file(quant, tmp_path / "q.npz")
    quant.remove(line)
    assert [l for l in quant if l[:10] != "Namespace("] == [l for l in plain if l[:10] != "Namespace("]
    pz = np.load(tmp_path / "p.npz")
    assert sorted(pz.files) == ["confusion", "labels", "log_probs", "pred"]
    assert sorted(z.files) == sorted(pz.files + ["sparse24_confusion", "sparse24_log_probs", "sparse24_pred"])
    assert np.array_equal(z["log_probs"], pz["log_probs"]) and not np.array_equal(z["sparse24_log_probs"], z["log_probs"])
    two = _run_cli(ev[:-1] + ["--quantize", "sparse24", "--world-size", "2", "--rank-prefix"], tmp_path)
    assert [l[9:] for l in two.splitlines() if "sparse24 (" in l] == [line] * 2
