"""int8 evaluation on the GPU (csrc/kernels/mlp_i8.hip): mlp_quant_w1 against the CPU oracle and
mlp_fwd_i8 against NumPy, bit for bit; the program at tests/test_quant_cpu.py's measure (measured
on MI355X: docs/kernels.md "int8 evaluation"); the CLI."""
import numpy as np
import pytest
import torch

from test_gpu_app import cli
from test_quant_cpu import SETS, check_forward, int8_line_matches_file, weight_set
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.ops import _ext
from pytorch_distributed_mnist_amd.runtime.cpu_step import quantize_fc1
from pytorch_distributed_mnist_amd.runtime.mlp_step import mlp_i8_splitk
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

pytestmark = pytest.mark.gpu
HID, K, KP, GUARD = 128, 784, 832, 256
bits = lambda t: t.cpu().numpy().view(np.int32)   # noqa: E731


@pytest.mark.parametrize("kind", SETS)
def test_mlp_quant_w1(gpu, kind):
    """q1 with its zero padding, s1, r1, c1, d1; the guards behind every output stay."""
    arena = weight_set(kind)
    want = quantize_fc1(arena)
    q1 = torch.full((HID * KP + GUARD,), 0x5A, dtype=torch.int8, device=gpu)
    o = {k: torch.full((HID + GUARD,), -7, dtype=torch.int32 if k == "r1" else torch.float32, device=gpu)
         for k in ("s1", "r1", "c1", "d1")}
    _ext.require().mlp_quant_w1(arena.param("fc1.weight").to(gpu), arena.param("fc1.bias").to(gpu),
                                q1[:HID * KP], *(o[k][:HID] for k in o))
    q = q1[:HID * KP].view(HID, KP).cpu().numpy()
    assert np.array_equal(q[:, :K], want["q1"]) and (q[:, K:] == 0).all() and (q1[HID * KP:] == 0x5A).all()
    for k, t in o.items():
        assert np.array_equal(bits(t[:HID]), want[k].view(np.int32)) and (t[HID:] == -7).all(), k


@pytest.mark.parametrize("S", [1, 13])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 624, 625])    # 624 | 625: mlp_i8_splitk's switch
def test_mlp_fwd_i8(gpu, B, S):
    """part = float32(I_s) * c1 split by split per image kind, twice the same bits; NaN padding
    behind part and the guards behind ylab stay; the image buffer ends 32 B behind row B - 1, where
    the last k-step's lanes g >= 1 would read 48 B if they were not clamped."""
    assert (mlp_i8_splitk(624), mlp_i8_splitk(625)) == (13, 1)
    g = torch.Generator().manual_seed(100 * B + S)
    q = torch.zeros(HID, KP, dtype=torch.int8)
    q[:, :K] = torch.randint(-127, 128, (HID, K), generator=g, dtype=torch.int8)
    q[3], q[4, :2] = 0, torch.tensor([127, -127], dtype=torch.int8)
    c1 = torch.randn(HID, generator=g)
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32) | \
        (torch.randint(0, 60000, (B,), generator=g, dtype=torch.int32) << 4)
    for x in (torch.randint(0, 256, (B, K), generator=g, dtype=torch.uint8),
              torch.zeros(B, K, dtype=torch.uint8), torch.full((B, K), 255, dtype=torch.uint8)):
        xbuf = torch.cat([x.flatten(), torch.full((32,), 0xFF, dtype=torch.uint8)]).to(gpu)
        x8 = torch.zeros(B, KP, dtype=torch.int64)
        x8[:, :K] = x.to(torch.int64) - 128
        I = torch.einsum("bsk,nsk->sbn", x8.view(B, S, KP // S), q.to(torch.int64).view(HID, S, KP // S))
        want, runs = I.numpy().astype(np.float32) * c1.numpy(), []
        for _ in range(2):
            part = torch.full((S * B * HID + GUARD,), float("nan"), device=gpu)
            ylab = torch.full((B + GUARD,), -7, dtype=torch.int32, device=gpu)
            _ext.require().mlp_fwd_i8(xbuf[:B * K].view(B, K), y.to(gpu), B, q.flatten().to(gpu),
                                      c1.to(gpu), part, ylab, S)
            assert torch.isnan(part[S * B * HID:]).all() and (ylab[B:] == -7).all()
            assert torch.equal(ylab[:B].cpu(), y)
            runs.append(bits(part[:S * B * HID].view(S, B, HID)))
        assert np.array_equal(runs[0], want.view(np.int32)) and np.array_equal(runs[0], runs[1]), int(x[0, 0])


@pytest.mark.parametrize("arch", ["mlp", "mlp2"])
def test_program(gpu, arch):
    """21 images: predict(quantize="int8") against the float64 quantised model and the CPU path's
    pred, the weight set of another arena (as the averaged weights'), the training state untouched."""
    data = synthetic_split(64, True), synthetic_split(21, False)
    prog, cpu, other = (build_local_program(arch, "fp32", dev, 8, *data, seed=seed, use_graphs=False)
                        for dev, seed in (("cuda", 5), ("cpu", 5), ("cuda", 6)))
    st, (x, y) = prog.gpu, (data[1].images, data[1].labels)
    state = lambda: [t.clone() for t in (prog.arena.params, st.metrics.buf, st.ctr,   # noqa: E731
                                         *prog.optimizer.state_buffers().values())]
    before = state()
    p = prog.predict(x, y, quantize="int8")
    check_forward("gpu", arch, prog.arena, x, p.log_probs, p.pred)
    assert torch.equal(p.pred, cpu.predict(x, y, quantize="int8").pred) and int(p.confusion.sum()) == 21
    assert not torch.equal(p.log_probs, prog.predict(x, y).log_probs)        # the path is taken
    logp, pred, _ = st.predict(x, y, st.weight_set_int8(other.arena))
    check_forward("gpu weight set", arch, other.arena, x, logp.cpu(), pred.cpu())
    assert not torch.equal(logp.cpu(), p.log_probs)
    assert all(torch.equal(a, b) for a, b in zip(before, state()))


def test_cli(gpu, tmp_path):
    from pytorch_distributed_mnist_amd.predict import load_predictor
    cli(["--arch", "mlp2", "--optimizer", "sgd", "--lr", "0.05", "--synthetic-size", "2048",
         "--epochs", "1", "--seed", "1"], tmp_path)
    ck = str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar")
    ev = ["--arch", "mlp2", "--optimizer", "sgd", "--evaluate", "--resume", ck]
    plain = [l for l in cli(ev, tmp_path) if l.startswith("test loss:")]
    out = cli(ev + ["--quantize", "int8", "--predict-out", str(tmp_path / "q.npz")], tmp_path)
    assert [l for l in out if l.startswith("test loss:")] == plain and len(plain) == 1
    _, z = int8_line_matches_file(out, tmp_path / "q.npz")
    p = load_predictor(ck, "mlp2", device="cuda", quantize="int8")
    assert np.array_equal(p.predict(synthetic_split(10000, False).images).pred.numpy(), z["int8_pred"])
