"""mlp_attack (csrc/kernels/mlp_attack.hip) on the GPU: the input gradient of --arch mlp against
float64, the integer FGSM / PGD step, its clamp edges, the program's attack() and the CLI.  The
oracle, the measure e = |g - g_ref| / s and its bound are tests/test_attack_cpu.py's
(docs/kernels.md "Adversarial evaluation")."""

import numpy as np
import pytest
import torch

from test_attack_cpu import adv_line_matches_file, check_one_step, oracle, path_bound, step_rule
from test_gpu_app import cli
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.ops import _ext
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

pytestmark = pytest.mark.gpu
HID, K, GUARD = 128, 784, 256


@pytest.fixture(scope="module")
def weights(gpu):
    """Weights of trained magnitude: fp32 masters on the host, and on the device fc1's bias, fc2
    and the hi / lo planes split from the fp32 fc1.weight the reference uses."""
    g = torch.Generator().manual_seed(11)
    w1 = torch.randn(HID, K, generator=g) * 0.05
    b1, w2, b2 = torch.randn(HID, generator=g) * 0.1, torch.randn(10, HID, generator=g) * 0.15, \
        torch.randn(10, generator=g) * 0.1
    hi = w1.to(torch.bfloat16)
    dev = [t.to(gpu) for t in (b1, w2, b2, hi, (w1 - hi.float()).to(torch.bfloat16))]
    return (w1, b1, w2, b2), dev


def make_case(B, S, weights, eps=16, alpha=5):
    """Constructed partials (|pre| >= 1e-3 everywhere; the last row of B > 1 all dead), labels, an
    iterate inside x0's box, and the launch: (reference g, s, x, x0, out bytes, grad, raw buffers)."""
    (w1, b1, w2, b2), dev = weights
    g = torch.Generator().manual_seed(1000 * B + S)
    pre = torch.randn(B, HID, generator=g, dtype=torch.float64) * 0.5
    pre = torch.where(pre.abs() < 1e-2, torch.full_like(pre, 1e-2), pre)
    if B > 1:
        pre[B - 1] = -pre[B - 1].abs()
    part = torch.randn(S, B, HID, generator=g, dtype=torch.float64) * 0.3
    part[S - 1] = pre - b1.double() - part[:S - 1].sum(0)
    part = part.float()
    y = torch.randint(0, 10, (B,), generator=g, dtype=torch.int32)
    x0 = torch.randint(0, 256, (B, K), generator=g, dtype=torch.uint8)
    x = (x0.int() + torch.randint(-eps, eps + 1, (B, K), generator=g)).clamp(0, 255).to(torch.uint8)
    pre64 = b1.double().numpy() + part.double().numpy().sum(0)      # from the fp32 partials
    assert (np.abs(pre64) >= 1e-3).all()
    gref, s = oracle(pre64, w2, b2, w1, y.numpy())
    # padding: NaN partials behind the last row, guard bytes and NaN behind row B - 1
    pbuf = torch.cat([part.flatten(), torch.full((GUARD,), float("nan"))]).cuda()
    out = torch.full((B + 2, K), 0x5A, dtype=torch.uint8, device="cuda")
    grad = torch.full((B * K + GUARD,), float("nan"), device="cuda")
    run = lambda o, gr, e=eps, a=alpha, xx=x, c=x0, pb=0: _ext.require().mlp_attack(   # noqa: E731
        pbuf, S, B, y.cuda(), *dev, c.cuda(), xx.cuda(), o, e, a, gr, pb)
    run(out, grad)
    return gref, s, x, x0, out, grad, run


@pytest.mark.parametrize("S", [1, 5, 25])
@pytest.mark.parametrize("B", [1, 15, 16, 17, 33])
def test_gradient_and_step(gpu, weights, B, S):
    """Measured on MI355X, largest e per case | the bound: see docs/kernels.md."""
    gref, s, x, x0, out, grad, run = make_case(B, S, weights)
    got = grad[:B * K].view(B, K).cpu().double().numpy()
    assert np.isfinite(got).all() and torch.isnan(grad[B * K:]).all()
    assert (out[B:] == 0x5A).all()
    assert (got[s == 0] == 0).all() and (B == 1 or (s[B - 1] == 0).all())
    bound = path_bound(S)
    e = (np.abs(got - gref)[s > 0] / s[s > 0]).max()
    print(f"mlp_attack B={B} S={S}: e = {e:.2e} (bound {bound:.2e})")
    assert e <= bound
    # the step: the rule on the reference's sign wherever it is decided; s == 0 pixels unchanged
    sure = (np.abs(gref) > bound * s) | (s == 0)
    assert 1.0 - sure.mean() <= 0.01
    o = out[:B].cpu().numpy()
    assert np.array_equal(o[sure], step_rule(x, x0, gref, 16, 5)[sure])
    assert np.array_equal(o[s == 0], x.numpy()[s == 0])          # (x lies inside the box)
    # run to run, and with one workgroup per m-tile instead of seven, the same bits
    for pb in (0, 1):
        out2, grad2 = torch.zeros_like(out), torch.zeros_like(grad)
        run(out2, grad2, pb=pb)
        assert torch.equal(out2[:B], out[:B]) and torch.equal(grad2[:B * K], grad[:B * K])


@pytest.mark.parametrize("case", ["black", "white", "alpha>eps", "boundary", "eps0"])
def test_clamp_edges(gpu, weights, case):
    B, S = 17, 5
    gref, s, x, x0, _, _, run = make_case(B, S, weights)
    eps, alpha = {"alpha>eps": (3, 200), "eps0": (0, 7)}.get(case, (16, 5))
    if case in ("black", "white"):
        x0 = torch.full_like(x0, 0 if case == "black" else 255)
        x = x0.clone()
    elif case == "boundary":        # an iterate already on the box: x0 +- eps, clipped
        sign = torch.where(torch.arange(K) % 2 == 0, 16, -16)
        x = (x0.int() + sign).clamp(0, 255).to(torch.uint8)
    elif case == "alpha>eps":
        x = x0.clone()
    out = torch.zeros(B, K, dtype=torch.uint8, device="cuda")
    run(out, None, eps, alpha, x, x0)
    o = out.cpu().numpy()
    sure = (np.abs(gref) > path_bound(S) * s) | (s == 0)
    assert np.array_equal(o[sure], step_rule(x, x0, gref, eps, alpha)[sure])
    assert (np.abs(o.astype(np.int64) - x0.numpy()) <= eps).all()
    if case == "eps0":
        assert np.array_equal(o, x0.numpy())


@pytest.fixture(scope="module")
def prog(gpu):
    return build_local_program("mlp", "fp32", "cuda", 8, synthetic_split(64, True),
                               synthetic_split(21, False), seed=5, use_graphs=False)


def test_program_attack(gpu, prog):
    """21 images in chunks of 8: one step against the oracle; three steps = three chained calls
    (3 alpha <= eps: the box never binds); the training state untouched; a weight set attacked."""
    st = prog.gpu
    x0, y = prog.test_split.images, prog.test_split.labels
    state = lambda: [t.clone() for t in (prog.arena.params, st.metrics.buf, st.ctr,   # noqa: E731
                                         *prog.optimizer.state_buffers().values())]
    before = state()
    one = st.attack(x0, y, 24, 1, 8, None, chunk=8).cpu()
    check_one_step("gpu program", one.numpy(), prog.arena, x0.numpy(), x0.numpy(), y.numpy(), 24, 8)
    x = x0
    for _ in range(3):
        x = st.attack(x, y, 24, 1, 8, None, chunk=8).cpu()
    full = prog.attack(x0, y, 24, 3, 8)
    assert torch.equal(full, x) and torch.equal(st.attack(x0, y, 24, 3, 8).cpu(), x)
    assert ((prog.attack(x0.numpy().reshape(21, 28, 28), y, 24, 3).int() - x0.int()).abs() <= 24).all()
    assert all(torch.equal(a, b) for a, b in zip(before, state()))
    other = build_local_program("mlp", "fp32", "cuda", 8, prog.train_split, prog.test_split,
                                seed=6, use_graphs=False)
    avg = st.attack(x0, y, 24, 1, 8, st.weight_set(other.arena), chunk=8).cpu()
    check_one_step("gpu weight set", avg.numpy(), other.arena, x0.numpy(), x0.numpy(), y.numpy(), 24, 8)
    assert not torch.equal(avg, one)


def test_cli(gpu, tmp_path):
    from pytorch_distributed_mnist_amd.predict import load_predictor
    cli(["--arch", "mlp", "--optimizer", "sgd", "--lr", "0.05", "--synthetic-size", "2048",
         "--epochs", "1", "--seed", "1"], tmp_path)
    ck = str(tmp_path / "checkpoints" / "checkpoint_0.pth.tar")
    ev = ["--arch", "mlp", "--optimizer", "sgd", "--evaluate", "--resume", ck]
    plain = [l for l in cli(ev, tmp_path) if l.startswith("test loss:")]
    out = cli(ev + ["--attack-eps", "25", "--attack-steps", "2", "--predict-out",
                    str(tmp_path / "a.npz")], tmp_path)
    assert [l for l in out if l.startswith("test loss:")] == plain and len(plain) == 1
    _, z = adv_line_matches_file(out, tmp_path / "a.npz")
    y = z["labels"]
    p = load_predictor(ck, "mlp", device="cuda")
    images = synthetic_split(10000, False).images
    assert np.array_equal(p.predict(p.attack(images, y, 25, steps=2)).pred.numpy(), z["adv_pred"])
