"""2:4 sparse evaluation on the GPU (csrc/kernels/mlp_sp24.hip): mlp_prune_24 against the CPU oracle,
mlp_fwd_sp24 against float64 on the pruned weights (K 2^-24 + 2^-18, K = 2 * 416 + 2), the program
and the CLI at tests/test_sparse24_cpu.py's measure (figures: docs/kernels.md "2:4 sparse evaluation")."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_app import cli
from test_sparse24_cpu import ALPHA, BETA, SETS, check_forward_sp, sp_weight_set, sparse24_line_matches_file
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.ops import _ext
from pytorch_distributed_mnist_amd.runtime.cpu_step import prune_fc1_24
from pytorch_distributed_mnist_amd.runtime.mlp_step import mlp_sp24_splitk
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

pytestmark = pytest.mark.gpu
HID, K, KP, NW, GUARD = 128, 784, 832, 28, 256


@functools.lru_cache(maxsize=None)
def oracle(kind):
    arena = sp_weight_set(kind)
    return arena, prune_fc1_24(arena)


@pytest.mark.parametrize("kind", SETS)
def test_mlp_prune_24(gpu, kind):
    """Planes, index bit for bit; d1 within 394 2^-24 (|b1| + beta sum |wp|), same bits twice; guards stay."""
    arena, want = oracle(kind)
    w, b = arena.param("fc1.weight").to(gpu), arena.param("fc1.bias").to(gpu)
    runs = []
    for _ in range(2):
        whi, wlo = (torch.full((HID * KP // 2 + GUARD,), -3.0, dtype=torch.bfloat16, device=gpu) for _ in range(2))
        index = torch.full((HID * NW + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=gpu)
        d1 = torch.full((HID + GUARD,), -7.0, device=gpu)
        _ext.require().mlp_prune_24(w, b, whi[:HID * KP // 2], wlo[:HID * KP // 2], index[:HID * NW], d1[:HID])
        for name, t in (("hi", whi), ("lo", wlo)):
            assert np.array_equal(t[:HID * KP // 2].view(torch.int16).view(HID, KP // 2).cpu().numpy(), want[name]), name
            assert (t[HID * KP // 2:] == -3).all(), name
        assert np.array_equal(index[:HID * NW].view(HID, NW).cpu().numpy(), want["index"])
        assert (index[HID * NW:] == 0x5A5A5A5A).all() and (d1[HID:] == -7).all()
        runs.append(d1[:HID].cpu().numpy())
    wp, b64 = want["wp"].astype(np.float64), b.cpu().numpy().astype(np.float64)
    err = np.abs(runs[0] - (b64 - BETA * wp.sum(1))) / (np.abs(b64) + BETA * np.abs(wp).sum(1))
    print(f"{kind}: d1 e = {err.max() * 2.0 ** 24:.2f} half-ulps (bound 394)")
    assert (err <= 394 * 2.0 ** -24).all() and np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32))


@pytest.mark.parametrize("kind", SETS)
@pytest.mark.parametrize("S", [1, 13])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 624, 625])   # 624 | 625: mlp_sp24_splitk's switch
def test_mlp_fwd_sp24(gpu, B, S, kind):
    """part per split and image kind: e = |got - alpha I| / (alpha sum_k |wp| u8) <= (2 * 416 + 2)
    2^-24 + 2^-18 (zero magnitude: got is 0), twice the same bits; NaN padding and guards stay; 32
    poisoned bytes behind the B image rows, where the last k-step's unclamped pieces would read."""
    assert (mlp_sp24_splitk(624), mlp_sp24_splitk(625)) == (13, 1)
    q = oracle(kind)[1]
    whi, wlo = (torch.from_numpy(q[n]).to(gpu).view(torch.bfloat16).flatten() for n in ("hi", "lo"))
    index = torch.from_numpy(q["index"]).to(gpu).flatten()
    wp = torch.zeros(HID, KP, dtype=torch.float64)
    wp[:, :K] = torch.from_numpy(q["wp"]).double()
    g = torch.Generator().manual_seed(100 * B + S)
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32) | \
        (torch.randint(0, 60000, (B,), generator=g, dtype=torch.int32) << 4)
    for x in (torch.randint(0, 256, (B, K), generator=g, dtype=torch.uint8),
              torch.zeros(B, K, dtype=torch.uint8), torch.full((B, K), 255, dtype=torch.uint8)):
        xbuf = torch.cat([x.flatten(), torch.full((32,), 0xFF, dtype=torch.uint8)]).to(gpu)
        x8 = torch.zeros(B, KP, dtype=torch.float64)
        x8[:, :K] = x.double()
        I, mag = (ALPHA * torch.einsum("bsk,nsk->sbn", x8.view(B, S, KP // S), w.view(HID, S, KP // S)).numpy()
                  for w in (wp, wp.abs()))
        runs = []
        for _ in range(2):
            part = torch.full((S * B * HID + GUARD,), float("nan"), device=gpu)
            ylab = torch.full((B + GUARD,), -7, dtype=torch.int32, device=gpu)
            _ext.require().mlp_fwd_sp24(xbuf[:B * K].view(B, K), y.to(gpu), B, whi, wlo, index, part, ylab, S)
            assert torch.isnan(part[S * B * HID:]).all() and (ylab[B:] == -7).all()
            assert torch.equal(ylab[:B].cpu(), y)
            runs.append(part[:S * B * HID].view(S, B, HID).cpu().numpy())
        assert np.array_equal(runs[0].view(np.int32), runs[1].view(np.int32)), int(x[0, 0])
        e = (np.abs(runs[0].astype(np.float64) - I) / np.maximum(mag, 1e-300)).max()
        print(f"{kind} B={B} S={S} x0={int(x[0, 0])}: e = {e:.2e} (bound {(KP + 2) * 2.0 ** -24 + 2.0 ** -18:.2e})")
        assert e <= (2 * KP // 2 + 2) * 2.0 ** -24 + 2.0 ** -18, (int(x[0, 0]), e)


@pytest.mark.parametrize("arch", ["mlp", "mlp2"])
def test_program(gpu, arch):
    """2069 images = chunks of 2048 and 21, both splits; another arena's set; training state untouched."""
    data = synthetic_split(64, True), synthetic_split(2069, False)
    prog, cpu, other = (build_local_program(arch, "fp32", dev, 8, *data, seed=seed, use_graphs=False)
                        for dev, seed in (("cuda", 5), ("cpu", 5), ("cuda", 6)))
    st, (x, y) = prog.gpu, (data[1].images, data[1].labels)
    state = lambda: [t.clone() for t in (prog.arena.params, st.metrics.buf, st.ctr,   # noqa: E731
                                         *prog.optimizer.state_buffers().values())]
    before, plain = state(), prog.predict(x, y)
    p = prog.predict(x, y, quantize="sparse24")
    check_forward_sp("gpu", arch, prog.arena, x, p.log_probs, p.pred)
    assert torch.equal(p.pred, cpu.predict(x, y, quantize="sparse24").pred) and int(p.confusion.sum()) == 2069
    assert not torch.equal(p.log_probs, plain.log_probs)                     # the path is taken
    logp, pred, _ = st.predict(x, y, st.weight_set_sparse24(other.arena))
    check_forward_sp("gpu weight set", arch, other.arena, x, logp.cpu(), pred.cpu())
    assert not torch.equal(logp.cpu(), p.log_probs)
    assert torch.equal(prog.predict(x, y).log_probs, plain.log_probs)
    assert all(torch.equal(a, b) for a, b in zip(before, state()))


def test_cli(gpu, tmp_path):
    """The line against the file; this run and the --device cpu run against the float64 model."""
    from pytorch_distributed_mnist_amd.predict import load_predictor
    cli(["--arch", "mlp2", "--optimizer", "sgd", "--lr", "0.05", "--synthetic-size", "512",
         "--epochs", "1", "--seed", "1"], tmp_path)
    ck = str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar")
    ev = ["--arch", "mlp2", "--optimizer", "sgd", "--evaluate", "--resume", ck, "--quantize", "sparse24",
          "--predict-out"]
    _, z = sparse24_line_matches_file(cli(ev + [str(tmp_path / "q.npz")], tmp_path), tmp_path / "q.npz")
    cli(ev + [str(tmp_path / "c.npz")], tmp_path, device="cpu", backend="gloo")
    arena, x = load_predictor(ck, "mlp2", device="cpu").program.arena, synthetic_split(10000, False).images
    for tag, f in (("cli gpu", z), ("cli cpu", np.load(tmp_path / "c.npz"))):
        check_forward_sp(tag, "mlp2", arena, x, torch.from_numpy(f["sparse24_log_probs"]),
                         torch.from_numpy(f["sparse24_pred"]))
