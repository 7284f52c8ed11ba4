"""cnn_head (head_body in csrc/kernels/cnn_head.hip) called directly on synthetic inputs, every
output against an fp64 reference written in plain torch.

The head reduces fc1's split-K partials, applies bias + ReLU, fc2, log-softmax / NLL and
argmax, and (train) writes dh twice in fragment-major layouts (or once as fp32 dh32) plus the
per-workgroup slab (dWfc2, dbfc2, dbfc1, loss, correct); in eval it adds the fp64 metrics.

Shapes (ldt = ceil(B / 32) * 32) are the smallest at which each path can go wrong:

    B     S    reaches
    1     32   one valid row, 31 padding rows, the S == 32 path
    37    32   last row group has 1 valid row of 4; ldt = 64
    64    16   exactly one 16-wide batch, no padding
    40    2    clamp path (s0 + q >= S selects)
    40    1    no split
    33    48   three 16-wide batches
    1030  4    ldt = 1056 -> 264 row groups on 256 workgroups (workgroups 0-7 take two groups,
               slab accumulators carry across them); 258 eval groups wrap as well

each at scale 1 and at scale 40 (logits to about +-350: expf without the max subtraction
overflows).

Tolerance of the fp32 outputs (dh32 and the slab sums): the same reference is evaluated once
more in fp32 torch on the CPU, and the kernel's relative-norm error against fp64 must stay
below 8 x that fp32-torch error, floor 2e-6 (expf / logf at a few ulp, another summation tree
over the 128 hidden units, up to 96 splits).  dh / dht (bf16) must be bit-identical to
bf16(dh32) laid out by runtime.cnn_step.frag_major / frag_major_t.

Measured on MI355X, relative-norm error against fp64: kernel | fp32 torch (bound = 8 x the
second column, at least 2e-6):

    B    S  scale  dh               dWfc2            dbfc2            dbfc1            loss sum
    1    32   1    9.6e-08|6.3e-08  1.3e-07|1.1e-07  6.5e-08|4.2e-08  9.6e-08|6.3e-08  2.7e-09|6.5e-08
    1    32  40    2.6e-08|2.6e-08  9.5e-08|7.9e-08  1.9e-11|1.9e-11  2.6e-08|2.6e-08  8.7e-08|8.7e-08
    37   32   1    1.7e-07|1.8e-07  2.6e-07|2.2e-07  2.4e-07|1.6e-07  2.4e-07|2.4e-07  3.6e-08|7.8e-09
    37   32  40    6.2e-07|3.2e-07  5.3e-07|2.8e-07  5.6e-07|2.9e-07  5.8e-07|3.1e-07  1.2e-09|7.6e-08
    64   16   1    1.6e-07|1.5e-07  1.4e-07|2.2e-07  1.0e-07|1.9e-07  1.2e-07|2.2e-07  1.1e-08|3.5e-08
    64   16  40    7.1e-07|1.0e-06  6.7e-07|9.8e-07  4.9e-07|7.2e-07  4.9e-07|7.2e-07  8.3e-10|4.0e-09
    40   2    1    1.1e-07|1.3e-07  9.5e-08|1.3e-07  8.8e-08|1.1e-07  8.9e-08|9.8e-08  4.0e-09|3.1e-10
    40   2   40    2.0e-07|2.0e-07  1.7e-07|1.7e-07  1.2e-07|1.3e-07  1.4e-07|1.5e-07  1.4e-08|7.5e-08
    40   1    1    1.2e-07|1.3e-07  1.2e-07|1.4e-07  1.2e-07|1.2e-07  1.3e-07|1.6e-07  1.7e-09|9.4e-08
    40   1   40    2.2e-07|8.5e-07  2.3e-07|8.5e-07  2.0e-07|7.3e-07  1.9e-07|6.8e-07  2.1e-08|4.5e-08
    33   48   1    2.5e-07|1.9e-07  2.2e-07|2.0e-07  1.5e-07|9.9e-08  2.1e-07|1.8e-07  4.2e-09|3.5e-08
    33   48  40    4.2e-07|8.1e-07  3.8e-07|7.1e-07  3.0e-07|6.3e-07  3.3e-07|6.4e-07  2.5e-09|6.3e-08
    1030 4    1    1.3e-07|1.3e-07  9.2e-08|1.8e-07  9.1e-08|9.5e-08  9.1e-08|9.4e-08  9.6e-09|2.9e-08
    1030 4   40    5.1e-07|8.8e-07  1.8e-07|2.8e-07  1.4e-07|2.4e-07  1.5e-07|2.1e-07  5.0e-09|5.0e-08

(the fp32-torch column depends on the host's BLAS; the largest kernel error is 7.1e-07, so the
2e-6 floor alone holds every case).  `correct` was exact in all cases (one near-tie row, at
B = 1030 scale 1); the eval loss sum was within 1.4e-08 relative (bound 1e-6).  dh / dht were
bit-identical to torch's bf16(dh32) everywhere: the device conversion rounds to nearest even.
"""
import functools
import math

import pytest
import torch

from pytorch_distributed_mnist_amd.runtime.cnn_step import frag_major, frag_major_t

pytestmark = pytest.mark.gpu

HID, NCLS, SLAB = 128, 10, 1420
SHAPES = [(1, 32), (37, 32), (64, 16), (40, 2), (40, 1), (33, 48), (1030, 4)]
QUANT = ("dh", "dWfc2", "dbfc2", "dbfc1", "loss")
M0 = (5.0, 3.0, 11.0)        # metrics pre-set
GUARD = 256                  # NaN elements behind every output buffer: nothing is written there


def _C():
    from pytorch_distributed_mnist_amd.ops import _ext
    return _ext.require()


def _ldt(B):
    return -(-B // 32) * 32


def relerr(a, b):
    return ((a.double() - b).norm() / b.norm().clamp_min(1e-300)).item()


def reference(part, bf1, wf2, bf2, y, dt):
    """The head in plain torch, every operation in dtype `dt`."""
    part, bf1, wf2, bf2 = (t.to(dt) for t in (part, bf1, wf2, bf2))
    B = part.shape[1]
    h = torch.relu(part.sum(0) + bf1)
    lg = h @ wf2.t() + bf2
    out = {"logits": lg}
    if y is not None:
        yl = y.long()
        onehot = torch.nn.functional.one_hot(yl, NCLS).to(dt)
        rowloss = torch.logsumexp(lg, 1) - lg.gather(1, yl[:, None])[:, 0]
        dl = (torch.softmax(lg, 1) - onehot) / B
        dh = (dl @ wf2) * (h > 0).to(dt)
        out.update(dh=dh, dWfc2=dl.t() @ h, dbfc2=dl.sum(0), dbfc1=dh.sum(0), loss=rowloss.sum(),
                   correct=int((lg.argmax(1) == yl).sum()))
    return out


def make_inputs(B, S, scale, seed):
    g = torch.Generator().manual_seed(seed)
    part = torch.randn(S, B, HID, generator=g) * (scale / math.sqrt(S))
    bf1 = torch.randn(HID, generator=g) * 0.5
    wf2 = torch.randn(NCLS, HID, generator=g) * 0.3
    bf2 = torch.randn(NCLS, generator=g) * 0.1
    # labels: every other row the fp64 reference's argmax, the rest random classes
    am = reference(part, bf1, wf2, bf2, None, torch.float64)["logits"].argmax(1)
    rnd = torch.randint(0, NCLS, (B,), generator=g)
    y = torch.where(torch.arange(B) % 2 == 1, am, rnd).to(torch.int32)
    return part, bf1, wf2, bf2, y


@functools.lru_cache(maxsize=None)
def case(B, S, scale):
    """Inputs, the fp64 reference, the fp32-torch reference and the number of near-tie rows of
    one (B, S, scale); computed once on the CPU, shared by the tests and never modified."""
    inp = make_inputs(B, S, scale, 1000 * B + S)
    r64 = reference(*inp, torch.float64)
    r32 = reference(*inp, torch.float32)
    assert all(torch.isfinite(torch.as_tensor(r64[q])).all() for q in QUANT)
    top2 = r64["logits"].topk(2, dim=1).values
    near = int(((top2[:, 0] - top2[:, 1]) < 1e-3).sum())
    return inp, r64, r32, near


def nanbuf(n, dtype, dev):
    return torch.full((n + GUARD,), float("nan"), dtype=dtype, device=dev)


def launch_train(C, dev, inp, bf16_mode):
    """One train-mode launch into NaN-filled buffers -> dict of CPU results."""
    part, bf1, wf2, bf2, y = inp
    S, B = part.shape[0], part.shape[1]
    ldt = _ldt(B)
    nblk = C.cnn_head_nblk(ldt)
    assert nblk == min(ldt // 4, 256)
    slab = nanbuf(nblk * SLAB, torch.float32, dev)
    metrics = torch.tensor(M0, dtype=torch.float64, device=dev)
    c0 = torch.tensor([41], dtype=torch.int64, device=dev)
    c1 = torch.tensor([7], dtype=torch.int64, device=dev)
    dh = dht = dh32 = None
    if bf16_mode:
        dh, dht = nanbuf(ldt * HID, torch.bfloat16, dev), nanbuf(ldt * HID, torch.bfloat16, dev)
    else:
        dh32 = nanbuf(ldt * HID, torch.float32, dev)
    C.cnn_head(part.reshape(-1).to(dev), S, B, bf1.to(dev), wf2.reshape(-1).to(dev), bf2.to(dev),
               y.to(dev), True, dh, dht, ldt, slab, metrics, c0, c1, None, dh32)
    torch.cuda.synchronize()
    out = dict(slab=slab.cpu(), metrics=metrics.cpu(), c0=int(c0.item()), c1=int(c1.item()),
               nblk=nblk, ldt=ldt)
    for k, t in (("dh", dh), ("dht", dht), ("dh32", dh32)):
        if t is not None:
            out[k] = t.cpu()
    for k in ("slab", "dh", "dht", "dh32"):            # nothing written past the buffer
        if k in out:
            assert torch.isnan(out[k][-GUARD:].float()).all(), k
            out[k] = out[k][:-GUARD]
    return out


def slab_sums(out):
    s = out["slab"].view(out["nblk"], SLAB).double().sum(0)
    return {"dWfc2": s[:1280].view(NCLS, HID), "dbfc2": s[1280:1290], "dbfc1": s[1290:1418],
            "loss": s[1418], "correct": s[1419].item()}


def bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def check_common(out, B):
    """What every train launch must leave behind, whatever the inputs."""
    assert torch.isfinite(out["slab"]).all()           # every slab element written, none NaN
    assert torch.equal(out["metrics"].view(torch.int64),
                       torch.tensor(M0, dtype=torch.float64).view(torch.int64))   # fc1_bwd owns them
    assert (out["c0"], out["c1"]) == (42, 8)


def check_bf16_layout(f32, b16, B):
    """dh / dht of the bf16 launch == bf16(dh32) in the fragment-major layouts, bit for bit."""
    ldt = f32["ldt"]
    want = f32["dh32"].view(ldt, HID).to(torch.bfloat16)          # torch: round to nearest even
    ar = torch.arange(ldt * HID).view(ldt, HID)
    for name, perm in (("dh", frag_major(ar)), ("dht", frag_major_t(ar))):
        got = torch.empty(ldt * HID, dtype=torch.bfloat16)
        got[perm] = b16[name]                                      # un-permute: flat p holds perm[p]
        got = got.view(ldt, HID)
        bad = (bits(got) != bits(want)).nonzero()
        assert bad.numel() == 0, (name, len(bad), bad[:4].tolist(),
                                  [(got[i, j].item(), want[i, j].item()) for i, j in bad[:4].tolist()])
        assert (bits(got[B:]) == 0).all(), name                    # padding rows: +0


@pytest.mark.parametrize("scale", [1, 40])
@pytest.mark.parametrize("B,S", SHAPES)
def test_head_train_vs_fp64(gpu, B, S, scale):
    """Train mode: dh32, the bf16 dh / dht copies, the slab sums, `correct`, the untouched
    train metrics and the counters."""
    C = _C()
    inp, r64, r32, near = case(B, S, scale)
    assert near <= (0 if B <= 64 else B // 100), near            # from the reference alone
    f32 = launch_train(C, gpu, inp, False)
    b16 = launch_train(C, gpu, inp, True)
    b16b = launch_train(C, gpu, inp, True)
    for out in (f32, b16, b16b):
        check_common(out, B)
    ldt = f32["ldt"]
    dh32 = f32["dh32"].view(ldt, HID)
    assert torch.isfinite(dh32).all()
    assert (bits(dh32[B:]) == 0).all()                            # padding rows exactly zero
    check_bf16_layout(f32, b16, B)
    # fixed split order: the slab does not depend on the dh mode, nor on the launch
    assert torch.equal(bits(f32["slab"]), bits(b16["slab"]))
    assert torch.equal(bits(b16["slab"]), bits(b16b["slab"]))
    assert torch.equal(bits(b16["dh"]), bits(b16b["dh"]))
    assert torch.equal(bits(b16["dht"]), bits(b16b["dht"]))

    got = slab_sums(f32)
    got["dh"] = dh32[:B]
    errs = {q: (relerr(torch.as_tensor(got[q]), r64[q]), relerr(torch.as_tensor(r32[q]), r64[q]))
            for q in QUANT}
    print(f"\nhead B={B} S={S} scale={scale}: " +
          "  ".join(f"{q} {k:.1e}|{t:.1e}" for q, (k, t) in errs.items()) +
          f"  correct {got['correct']:.0f}/{r64['correct']} near {near}")
    for q, (k, t) in errs.items():
        assert k <= max(8 * t, 2e-6), (q, k, t)
    assert got["correct"] == int(got["correct"])
    assert abs(got["correct"] - r64["correct"]) <= near, (got["correct"], r64["correct"], near)


@pytest.mark.parametrize("B,S", SHAPES)
def test_head_eval_adds_metrics(gpu, B, S):
    """Eval mode (dh / dht / slab None, ldt 32 as CnnStep.evaluate passes): the kernel adds
    (loss sum, correct, B) to the fp64 metrics and leaves the counters alone."""
    C = _C()
    (part, bf1, wf2, bf2, y), r64, _, near = case(B, S, 1)
    metrics = torch.tensor(M0, dtype=torch.float64, device=gpu)
    c0 = torch.tensor([41], dtype=torch.int64, device=gpu)
    c1 = torch.tensor([7], dtype=torch.int64, device=gpu)
    C.cnn_head(part.reshape(-1).to(gpu), S, B, bf1.to(gpu), wf2.reshape(-1).to(gpu), bf2.to(gpu),
               y.to(gpu), False, None, None, 32, None, metrics, c0, c1)
    torch.cuda.synchronize()
    m = metrics.cpu()
    want = r64["loss"].item() + M0[0]
    print(f"\nhead eval B={B} S={S}: loss sum rel {abs(m[0].item() - want) / want:.1e}  "
          f"correct {m[1].item() - M0[1]:.0f}/{r64['correct']} near {near}")
    assert abs(m[0].item() - want) <= 1e-6 * want, (m[0].item(), want)
    assert abs(m[1].item() - M0[1] - r64["correct"]) <= near
    assert m[1].item() == int(m[1].item())
    assert m[2].item() == M0[2] + B
    assert (int(c0.item()), int(c1.item())) == (41, 7)


@pytest.mark.parametrize("label,correct", [(0, 8), (1, 0)])
def test_head_argmax_takes_first_maximum(gpu, label, correct):
    """wf2 = 0 and bf2 = [0.3, 0.3, 0, ...]: every row's logits are bf2, classes 0 and 1 tied at
    the top.  The first maximum wins (as torch.argmax), dh is exactly zero and dbfc2 is
    softmax(bf2) - onehot."""
    C = _C()
    B, S = 8, 1
    part, bf1, _, _, _ = make_inputs(B, S, 1, 8001)
    wf2 = torch.zeros(NCLS, HID)
    bf2 = torch.zeros(NCLS)
    bf2[:2] = 0.3
    y = torch.full((B,), label, dtype=torch.int32)
    inp = (part, bf1, wf2, bf2, y)
    r64 = reference(*inp, torch.float64)
    assert r64["correct"] == correct                       # torch takes the first maximum too
    f32 = launch_train(C, gpu, inp, False)
    b16 = launch_train(C, gpu, inp, True)
    for out in (f32, b16):
        check_common(out, B)
        assert slab_sums(out)["correct"] == correct
    assert (f32["dh32"] == 0).all()
    assert (b16["dh"].float() == 0).all() and (b16["dht"].float() == 0).all()
    got = slab_sums(f32)
    p = torch.softmax(bf2.double(), 0)
    p[label] -= 1.0
    assert relerr(got["dbfc2"], p) <= 2e-6
    assert relerr(got["dWfc2"], r64["dWfc2"]) <= 2e-6
    assert (got["dbfc1"] == 0).all()
    assert abs(got["loss"].item() - r64["loss"].item()) <= 2e-6 * r64["loss"].item()
