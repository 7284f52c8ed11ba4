"""MXFP4 evaluation on the GPU (csrc/kernels/mlp_mx4.hip): mlp_quant_mx4 bit for bit against the
CPU oracle; mlp_fwd_mx4 bit for bit on a flat weight set and within the summed-magnitude bound on
a wide one; the program at tests/test_mxfp4_cpu.py's measure; the CLI (measured on MI355X:
docs/kernels.md "MXFP4 evaluation")."""
import numpy as np
import pytest
import torch

from test_gpu_app import cli
from test_mxfp4_cpu import ALPHA, GRID, SETS, check_forward_mx, mx_weight_set, mxfp4_line_matches_file
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.ops import _ext
from pytorch_distributed_mnist_amd.runtime.cpu_step import quantize_fc1_mxfp4
from pytorch_distributed_mnist_amd.runtime.mlp_step import mlp_mx4_splitk
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

pytestmark = pytest.mark.gpu
HID, K, KP, GUARD = 128, 784, 896, 256
bits = lambda t: t.cpu().numpy().view(np.int32)   # noqa: E731


@pytest.mark.parametrize("kind", SETS)
def test_mlp_quant_mx4(gpu, kind):
    """codes with their zero padding, scales with the three padding bytes, d1; the guards behind
    every output stay."""
    arena = mx_weight_set(kind)
    want = quantize_fc1_mxfp4(arena)
    codes = torch.full((HID * KP // 2 + GUARD,), 0x5A, dtype=torch.uint8, device=gpu)
    scales = torch.full((HID * KP // 32 + GUARD,), 0x5A, dtype=torch.uint8, device=gpu)
    d1 = torch.full((HID + GUARD,), -7.0, device=gpu)
    _ext.require().mlp_quant_mx4(arena.param("fc1.weight").to(gpu), arena.param("fc1.bias").to(gpu),
                                 codes[:HID * KP // 2], scales[:HID * KP // 32], d1[:HID])
    assert np.array_equal(codes[:HID * KP // 2].view(HID, KP // 2).cpu().numpy(), want["codes"])
    assert np.array_equal(scales[:HID * KP // 32].view(HID, KP // 32).cpu().numpy(), want["scales"])
    assert np.array_equal(bits(d1[:HID]), want["d1"].view(np.int32))
    assert (codes[HID * KP // 2:] == 0x5A).all() and (scales[HID * KP // 32:] == 0x5A).all()
    assert (d1[HID:] == -7).all()


def fwd_set(kind, g):
    """Random codes (negative zeros included; columns >= 784 zero) and block scales: "flat" from
    three adjacent exponents, so that every term is a multiple of 2^(118 - 127 - 1) and the sum
    stays below 2^24 of them: exact in any order; "wide" over 2^-30 .. 2^-1, where a row's sum
    rounds.  (codes uint8 [128, 448], scales uint8 [128, 28], wq float64 [128, 896])."""
    nib = torch.randint(0, 16, (HID, KP), generator=g, dtype=torch.uint8)
    nib[:, K:], nib[3] = 0, 0
    lo, hi = (118, 121) if kind == "flat" else (97, 127)
    e8 = torch.randint(lo, hi, (HID, KP // 32), generator=g, dtype=torch.uint8)
    e8[:, 25:] = 127
    mag = torch.tensor(GRID, dtype=torch.float64)[(nib & 7).long()] * (1 - 2 * (nib >> 3).double())
    wq = mag * torch.exp2(e8.double() - 127).repeat_interleave(32, dim=1)
    return nib[:, 0::2] | (nib[:, 1::2] << 4), e8, wq


@pytest.mark.parametrize("kind", ["flat", "wide"])
@pytest.mark.parametrize("S", [1, 7])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 1168, 1169])   # 1168 | 1169: mlp_mx4_splitk's switch
def test_mlp_fwd_mx4(gpu, B, S, kind):
    """part split by split per image kind, twice the same bits.  flat: part = float32(alpha *
    float32(I)) bit for bit (I is exact in float64: integers of the unit below 2^24); wide: |part -
    alpha I| <= K 2^-23 alpha sum_k |Wq| u8 with K = 2 * 896 + 2, the products on the path (high
    and low nibble), the scaling and the rounding at one ulp each.  NaN padding behind part and
    the guards behind ylab stay; the image buffer is exactly B rows with 32 poisoned bytes behind
    it, where the last k-step's pieces past column 783 would read if they were not clamped."""
    assert (mlp_mx4_splitk(1168), mlp_mx4_splitk(1169)) == (7, 1)
    g = torch.Generator().manual_seed(100 * B + S)
    codes, e8, wq = fwd_set(kind, g)
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32) | \
        (torch.randint(0, 60000, (B,), generator=g, dtype=torch.int32) << 4)
    for x in (torch.randint(0, 256, (B, K), generator=g, dtype=torch.uint8),
              torch.zeros(B, K, dtype=torch.uint8), torch.full((B, K), 255, dtype=torch.uint8)):
        xbuf = torch.cat([x.flatten(), torch.full((32,), 0xFF, dtype=torch.uint8)]).to(gpu)
        x8 = torch.zeros(B, KP, dtype=torch.float64)
        x8[:, :K] = x.double()
        I, mag = (torch.einsum("bsk,nsk->sbn", x8.view(B, S, KP // S), w.view(HID, S, KP // S)).numpy()
                  for w in (wq, wq.abs()))
        runs = []
        for _ in range(2):
            part = torch.full((S * B * HID + GUARD,), float("nan"), device=gpu)
            ylab = torch.full((B + GUARD,), -7, dtype=torch.int32, device=gpu)
            _ext.require().mlp_fwd_mx4(xbuf[:B * K].view(B, K), y.to(gpu), B, codes.flatten().to(gpu),
                                       e8.flatten().to(gpu), part, ylab, S)
            assert torch.isnan(part[S * B * HID:]).all() and (ylab[B:] == -7).all()
            assert torch.equal(ylab[:B].cpu(), y)
            runs.append(part[:S * B * HID].view(S, B, HID).cpu().numpy())
        assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32)), int(x[0, 0])
        if kind == "flat":
            want = np.float32(ALPHA) * I.astype(np.float32)
            assert np.array_equal(runs[0].view(np.int32), want.view(np.int32)), int(x[0, 0])
        else:
            e = np.abs(runs[0].astype(np.float64) - ALPHA * I) / np.maximum(ALPHA * mag, 1e-300)
            print(f"wide B={B} S={S} x0={int(x[0, 0])}: e = {e.max() * 2.0 ** 23:.2f} ulp-sums (bound {2 * KP + 2})")
            assert (e <= (2 * KP + 2) * 2.0 ** -23).all()


@pytest.mark.parametrize("arch", ["mlp", "mlp2"])
def test_program(gpu, arch):
    """2069 images (chunks of 2048 and 21: both splits): predict(quantize="mxfp4") against the
    float64 quantised model and the CPU path's pred, the weight set of another arena (as the
    averaged weights'), the training state untouched."""
    data = synthetic_split(64, True), synthetic_split(2069, False)
    prog, cpu, other = (build_local_program(arch, "fp32", dev, 8, *data, seed=seed, use_graphs=False)
                        for dev, seed in (("cuda", 5), ("cpu", 5), ("cuda", 6)))
    st, (x, y) = prog.gpu, (data[1].images, data[1].labels)
    state = lambda: [t.clone() for t in (prog.arena.params, st.metrics.buf, st.ctr,   # noqa: E731
                                         *prog.optimizer.state_buffers().values())]
    before = state()
    p = prog.predict(x, y, quantize="mxfp4")
    check_forward_mx("gpu", arch, prog.arena, x, p.log_probs, p.pred)
    assert torch.equal(p.pred, cpu.predict(x, y, quantize="mxfp4").pred) and int(p.confusion.sum()) == 2069
    for q in (None, "int8"):
        assert not torch.equal(p.log_probs, prog.predict(x, y, quantize=q).log_probs)   # the path is taken
    logp, pred, _ = st.predict(x, y, st.weight_set_mxfp4(other.arena))
    check_forward_mx("gpu weight set", arch, other.arena, x, logp.cpu(), pred.cpu())
    assert not torch.equal(logp.cpu(), p.log_probs)
    assert all(torch.equal(a, b) for a, b in zip(before, state()))


def test_cli(gpu, tmp_path):
    """The mxfp4 line against the file; log_probs as without the flag; mxfp4_log_probs of this run
    and of the --device cpu run both within the carried bound of the float64 model."""
    from pytorch_distributed_mnist_amd.predict import load_predictor
    cli(["--arch", "mlp2", "--optimizer", "sgd", "--lr", "0.05", "--synthetic-size", "2048",
         "--epochs", "1", "--seed", "1"], tmp_path)
    ck = str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar")
    ev = ["--arch", "mlp2", "--optimizer", "sgd", "--evaluate", "--resume", ck, "--predict-out"]
    cli(ev + [str(tmp_path / "p.npz")], tmp_path)
    out = cli(ev + [str(tmp_path / "q.npz"), "--quantize", "mxfp4"], tmp_path)
    _, z = mxfp4_line_matches_file(out, tmp_path / "q.npz")
    assert np.array_equal(z["log_probs"], np.load(tmp_path / "p.npz")["log_probs"])
    cli(ev + [str(tmp_path / "c.npz"), "--quantize", "mxfp4"], tmp_path, device="cpu", backend="gloo")
    arena, x = load_predictor(ck, "mlp2", device="cpu").program.arena, synthetic_split(10000, False).images
    for tag, f in (("cli gpu", z), ("cli cpu", np.load(tmp_path / "c.npz"))):
        check_forward_mx(tag, "mlp2", arena, x, torch.from_numpy(f["mxfp4_log_probs"]),
                         torch.from_numpy(f["mxfp4_pred"]))
