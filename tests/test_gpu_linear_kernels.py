"""The Linear program's kernels (csrc/kernels/linear.hip, lin_common.h, and the Linear geometry of
optim.hip's slab segments), each called directly and compared slab by slab with fp64.

test_gpu_linear.py compares only the sum over all slabs, at allclose(atol=2e-6, rtol=1e-4); no
direct call passed spe > 0; lin_reduce's order was tested for reproducibility only; the fused
optimizer's Linear segments only after an epoch.  Here:

1. One-row blocks, exact (B = 1 and the tail block of B = 5).  The block's one valid row holds
   every byte value, so dW[n][k] == fl32(db[n] * x32[k]) as values for all n, k, with x32 =
   normalize_reference(byte): the fp32 arithmetic ((v / 255 - 0.1307) / 0.3081) in correctly
   rounded operations (checked against numpy float32 scalars on the CPU first).  That pins all
   256 table entries, put_pixels' byte order and that rows >= nrows add exactly nothing.
2. lin_train, every block of LIN_ROWS = 4 rows on its own: dW_blk = dl_blk^T x_blk, db_blk, the
   block's loss and correct count, for (B, bfull) in (1, 8), (5, 8), (13, 32), (64, 64),
   (96, 256), (256, 256), each in four row modes: flat buffer at counter 1, the two-half buffer
   (spe = 3, halves of 2 bfull + B rows) at counter 4 (epoch 1: second half) and 7 (epoch 2:
   first half), and the sampler gather.  The rows follow test_gpu_cnn_f32_kernels.step_row and
   satisfy bind.cpp's step_rows check; they start neither at row 0 nor end at the buffer's end,
   and every other row of the buffer is a different image.  The four modes must give the same
   bits.  Plus: W scaled by 40 (largest |logit| 266 > 88.7, where expf overflows); exact ties
   between classes 2 and 5 (zero W with equal biases; two identical W rows) for lin_train and
   lin_eval, label on either class; a second launch (B = 13) into the slab a B = 256 launch left.
3. lin_reduce on random slabs, nblk in 1, 7, 8, 9, 17, 64 through B = 4 nblk - {0, 3}: gW / gb
   equal, as values, the fp32 sum over the slabs one after the other in ascending order (a
   Python loop: np.sum / torch.sum add pairwise); two NaN slabs lie behind the nblk valid ones.
4. optim_step with exactly LinearStep._fused_segments' two segments on one shared slab (10 x 784
   at column 0, 1 x 10 at column 7840, stride 7856), the metrics tuple (column 7850) and bump,
   SGD and Adam (test_gpu_optim.KIND_HYPER), nblk in 1, 13, 16, 17, 64.  The gradient left in the
   arena equals test_gpu_optim.slab_sum (group rg adds slabs rg, rg + 16, ...; then the 16 group
   sums in order) as values; for nblk <= 16 also the sequential sum of 3. and lin_reduce's output
   on the same slabs.  p, m, v then follow test_gpu_optim.measure from that gradient.  Every
   arena element outside the two segments keeps its bits in p, g, m, v: slab columns 7850 / 7851
   (they share the float4 group of the bias' last two elements) reach no parameter.
5. lin_eval at N in 1, 15, 16, 17, 33, 1000 from a preset; a second call adds the same again.

Every output buffer is NaN-filled with a 256-element guard behind the kernel's contract; what
the contract covers must be finite afterwards, the guard NaN.  Slab columns 7852..7855 are NaN
before and after (lin_reduce and the optimizer leave every bit of the slab as uploaded), and no
output of lin_reduce, the optimizer or the metrics is NaN.  Blocks of
the slab behind ceil(B / 4) stay NaN.  Metrics start from M0 = (5, 3, 11) (test_gpu_predict.py);
lin_train must leave exactly [5, 3, 11 + B]; counters start from 7, 41 and the step counter >= 1
with a second word (977) behind it; the data-step counter is not touched by lin_train.

Rules (none is new):
- dW, db, loss per block, and lin_eval's loss sum: the head's rule (test_gpu_cnn_head.py,
  test_gpu_predict.py): the same reference once more in fp32 torch on the CPU; the relative-norm
  error against fp64 must stay below 8 x the fp32-torch error of the same block, floor 2e-6.
- correct is exact outside near-tie rows (fp64 top-2 logit gap < 1e-3, test_gpu_predict.py),
  whose number is first bounded from the reference alone: 0 for B <= 64, else B // 100.
- Metrics sums: against math.fsum of the preset and the nblk column values within
  nblk * 2^-53 * sum |term|: the launch makes at most nblk - 1 rounded fp64 additions for the
  column and one for the preset, which is therefore one of the terms (with nblk = 1 the only
  rounding is preset + value, relative to their sum, not to the value).
- lin_eval's second call: the loss additions of the two calls differ by at most the roundings of
  the fp64 atomic adds (one per 16-row block and call, each <= 2^-53 of the running sum, and the
  two subtractions): (2 nblk + 2) * 2^-53 * the final sum.
- The update: test_gpu_optim.py's two assertions (8 x step_cpu's error; R * 2^-23), unchanged.

Measured on MI355X (kernel | fp32 torch, relative-norm error against fp64 of the worst block;
"ratio" = the largest kernel / fp32-torch quotient of any block; the four row modes gave the
same bits, so one line per case):

    lin_train       dW               db               loss             ratio dW/db/loss correct near
    B=1/8           1.9e-07|1.3e-07  1.7e-07|1.1e-07  7.9e-08|1.5e-07  1.47/1.61/0.54    0/0     0
    B=5/8           2.0e-07|3.0e-07  2.5e-07|3.9e-07  8.5e-08|8.5e-08  1.03/0.96/1.00    2/2     0
    B=13/32         1.8e-07|1.9e-07  1.9e-07|1.7e-07  2.2e-07|3.8e-07  0.97/1.10/0.98    6/6     0
    B=64/64         2.7e-07|2.7e-07  3.4e-07|2.5e-07  1.2e-07|8.6e-09  1.41/1.62/14.1    33/33   0
    B=96/256        2.2e-07|2.4e-07  2.4e-07|2.8e-07  1.7e-07|1.7e-07  1.46/1.24/4.16    58/58   0
    B=256/256       3.0e-07|3.1e-07  3.5e-07|2.5e-07  2.1e-07|8.4e-08  1.43/1.46/12.6    140/140 0
    B=13/32 x40     1.3e-05|1.5e-05  1.3e-05|1.5e-05  3.5e-05|4.3e-05  1.00/1.00/0.82    8/8     0
    B=13 after 256  1.7e-07|2.5e-07  1.1e-07|1.3e-07  7.0e-08|7.7e-09  0.93/0.88/9.05

A block's loss is one fp32 number, so its fp32-torch error is now and then nearly 0 and the
quotient passes 8 (5 of 119 blocks); the floor holds those, as it does the head's loss sum: the
largest kernel error at scale 1 is 3.5e-07.  At scale 40 the errors are those of logits of size
266 (the kernel 0.82 to 1.00 of fp32 torch), far from the inf / NaN of a missing max subtraction.

    lin_eval N   loss sum         correct  near
    1            1.3e-07|8.4e-07  0/0      0
    15           8.6e-11|1.4e-07  8/8      0
    16           9.7e-09|9.9e-08  8/8      0
    17           3.6e-08|3.1e-08  9/9      0
    33           5.4e-08|5.0e-08  16/16    0
    1000         3.6e-08|8.0e-09  552/552  1

    fused update    out  e(kernel)  e(cpu32)   (largest over nblk; fc.weight, then fc.bias)
    SGD             p    1.30e-07   8.40e-08    7.86e-08  7.35e-08
                    m    1.13e-07   1.13e-07    7.94e-08  7.94e-08
    Adam            p    6.62e-08   4.66e-06    4.44e-08  4.44e-08
                    m    1.60e-07   3.48e-07    8.36e-08  2.07e-07
                    v    2.22e-07   1.30e-05    6.55e-08  2.78e-06

1. was bit-equal: 0 of 7840 elements differed from fl32(db * x32), for B = 1 and B = 5, from the
epoch buffer and from the gather.  No build flag relaxes the fp32 division (hipcc divides
correctly rounded by default and the build passes no fast-math option), so the fp64-normalisation
fall-back of the plan was not needed.  lin_reduce, the optimizer's reduced gradient and the ties
were exact as stated; `correct` matched the fp64 argmax in every block.

One thing the code does differently from its comment: rows >= nrows of lin_train's xs are not
zeros but normalize(0) = -0.4242 (zero bytes through the table).  They add exactly nothing
because dl of such a row is exactly 0 (fmaf(0, x, s) = s), which is what 1. pins.

Mutations, one scratch build each (arithmetic or in-bounds index only), run once against this
file and the parent's Linear tests ("old": test_gpu_linear.py, lin_predict and the program test
of test_gpu_predict.py, the two Linear tests of test_gpu_label_smoothing.py):

    pdm_normalize mean 0.1306   1. (4), 2. (all 8), 5. (6) fail.  old: 21 fail
    a table entry added to x    nothing fails, old or new, and nothing can: that x is multiplied
    of rows >= nrows            by dl = 0 (see above), so the slab keeps its bits.  Its
                                observable counterpart:
    dl of rows >= nrows 2^-30   1. fails (all 4 cases).  old: passes
    db over ROWS - 1 rows       2. fails (all but B = 1, whose one row is row 0).  old: 14 fail
    lin_reduce descending       3. fails (all 10 cases with nblk > 1), 4. fails at nblk 13 and 16
                                (the lin_reduce cross-check).  old: passes
    step_row half by e & 2      1. (the epoch-buffer cases) and 2. (all 8) fail.  old: passes
"""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from pytorch_distributed_mnist_amd.data.mnist import MNIST_MEAN, MNIST_STD, normalize_reference
from pytorch_distributed_mnist_amd.models import get_spec
from test_gpu_cnn_f32_kernels import step_row
from test_gpu_optim import KIND_HYPER, Guarded, launch, measure, slab_sum
from test_gpu_predict import M0

pytestmark = pytest.mark.gpu

D, F32 = torch.float64, torch.float32
K, NC, NK = 784, 10, 7840
ROWS, SLAB, EVAL_ROWS = 4, 7856, 16             # kernels.h LIN_ROWS, LIN_SLAB, LIN_EVAL_ROWS
COL_DB, COL_LOSS, COL_OK, COL_PAD = 7840, 7850, 7851, 7852
GUARD = 256                                     # NaN elements behind every output buffer
FLOOR = 2e-6                                    # test_gpu_cnn_head.py's floor of the 8 x rule
NEAR_GAP = 1e-3                                 # test_gpu_predict.py: fp64 top-2 logit gap
U53 = 2.0 ** -53
NAN = float("nan")
C1_0, SPARE = 7, 977                            # optimizer-step counter preset; ctr[1]


def _C():
    from pytorch_distributed_mnist_amd.ops import _ext
    C = _ext.require()
    assert (C.LIN_ROWS, C.LIN_SLAB) == (ROWS, SLAB)
    return C


def nanbuf(n, dev):
    return torch.full((n + GUARD,), NAN, dtype=F32, device=dev)


def read_guarded(buf, n, name):
    out = buf.cpu()
    assert torch.isnan(out[n:]).all(), name + ": guard overwritten"
    return out[:n]


def preset(dev):
    return torch.tensor(M0, dtype=D, device=dev)


def blocked(t, rows):
    """[B, ...] -> [ceil(B / rows), rows, ...], zero rows behind B."""
    pad = -t.shape[0] % rows
    return torch.cat([t, t.new_zeros((pad,) + tuple(t.shape[1:]))]).view(-1, rows, *t.shape[1:])


def blockerr(a, ref):
    """Relative-norm error of every block (first dimension) on its own."""
    a, ref = a.double().reshape(a.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    return (a - ref).norm(dim=1) / ref.norm(dim=1).clamp_min(1e-300)


def rule(tag, name, got, r64, r32):
    """test_gpu_cnn_head.py's rule, block by block: error against fp64 <= max(8 x the fp32-torch
    error of the same block, 2e-6).  A NaN fails."""
    k, t = blockerr(got, r64), blockerr(r32, r64)
    j = int(torch.nan_to_num(k, nan=math.inf).argmax())
    ratio = (k / t.clamp_min(1e-300))[t > 0]
    print(f"LIN {tag} {name}: worst block {j} {k[j].item():.1e}|{t[j].item():.1e}  "
          f"largest ratio {ratio.max().item() if ratio.numel() else 0.0:.2f}  "
          f"blocks above 8x {int((k > 8 * t).sum())}/{k.numel()}")
    ok = k <= torch.clamp_min(8 * t, FLOOR)
    bad = (~ok).nonzero()[:4, 0].tolist()
    assert ok.all(), (tag, name, [(i, k[i].item(), t[i].item()) for i in bad])


# ------------------------------------------------------------------ the references
def x64(images):
    return (images.double() / 255.0 - MNIST_MEAN) / MNIST_STD


def reference(images, y, W, b, dt):
    """lin_train / lin_eval in plain torch, every operation in dtype `dt`: per block of ROWS rows
    dW = dl^T x, db, the loss sum and the correct count; per row the loss and the logits."""
    B = images.shape[0]
    x = x64(images) if dt == D else normalize_reference(images)
    lg = F.linear(x, W.to(dt), b.to(dt))
    yl = y.long()
    rowloss = torch.logsumexp(lg, 1) - lg.gather(1, yl[:, None])[:, 0]
    dl = (torch.softmax(lg, 1) - F.one_hot(yl, NC).to(dt)) / B
    dlb, xb = blocked(dl, ROWS), blocked(x, ROWS)
    hit = (lg.argmax(1) == yl).to(dt)
    return dict(logits=lg, rowloss=rowloss, hit=hit, dW=torch.einsum("jrn,jrk->jnk", dlb, xb),
                db=dlb.sum(1), loss=blocked(rowloss, ROWS).sum(1),
                correct=blocked(hit, ROWS).sum(1))


def near_rows(lg64):
    top2 = lg64.topk(2, dim=1).values
    return (top2[:, 0] - top2[:, 1]) < NEAR_GAP


def half_argmax_labels(lg64, g):
    """Every other row the fp64 argmax, the rest random classes (test_gpu_cnn_head.py)."""
    n = lg64.shape[0]
    rnd = torch.randint(0, NC, (n,), generator=g)
    return torch.where(torch.arange(n) % 2 == 1, lg64.argmax(1), rnd).to(torch.int32)


@functools.lru_cache(maxsize=None)
def train_case(B, bfull, wscale=1.0):
    """The B selected rows, W, b, labels and both references of one case; computed once on the
    CPU, shared by the tests and never modified."""
    g = torch.Generator().manual_seed(1000 * B + bfull + (500 if wscale != 1.0 else 0))
    X = torch.randint(0, 256, (B, K), generator=g, dtype=torch.uint8)
    W = torch.randn(NC, K, generator=g) * (0.05 * wscale)
    b = torch.randn(NC, generator=g) * 0.1
    y = half_argmax_labels(F.linear(x64(X), W.double(), b.double()), g)
    r64, r32 = reference(X, y, W, b, D), reference(X, y, W, b, F32)
    assert all(torch.isfinite(r64[q]).all() for q in ("dW", "db", "loss"))
    near = near_rows(r64["logits"])
    return dict(B=B, bfull=bfull, X=X, W=W, b=b, y=y, r64=r64, r32=r32, near=int(near.sum()),
                near_blk=blocked(near.double(), ROWS).sum(1))


MODES = ("flat", "half0", "half1", "gather")


def buffers(B, bfull, X, y, mode):
    """The device inputs of one row mode with X / y at the rows the step selects and different
    images everywhere else -> (images, labels, idx | None, counter, spe)."""
    g = torch.Generator().manual_seed(17 * B + bfull + MODES.index(mode))
    fill = lambda n: (torch.randint(0, 256, (n, K), generator=g, dtype=torch.uint8),
                      torch.randint(0, NC, (n,), generator=g).to(torch.int32))
    if mode == "gather":                          # images[idx[c * bfull + i]]
        nrow, c = 3 * bfull, 1
        images, labels = fill(nrow + 17)
        idx = torch.randperm(nrow + 17, generator=g)[:nrow].to(torch.int32)
        rows = idx[c * bfull: c * bfull + B].long()
        images[rows], labels[rows] = X, y
        return images, labels, idx, c, 0
    if mode == "flat":                            # one buffer, row c * bfull + i
        nrow, c, spe = 3 * bfull, 1, 0
    else:                                         # two epoch halves of 3 steps: 2 bfull + B rows
        half, spe = 2 * bfull + B, 3
        nrow, c = 2 * half, {"half1": 4, "half0": 7}[mode]      # epochs 1 and 2, step 1 of 3
        assert nrow % 2 == 0 and (spe - 1) * bfull < nrow // 2 <= spe * bfull   # bind.cpp step_rows
    rows = [step_row(bfull, spe, nrow, c, i) for i in range(B)]
    assert rows == list(range(rows[0], rows[0] + B)) and rows[0] > 0 and rows[-1] < nrow - 1
    if spe:
        assert (rows[0] >= nrow // 2) == (mode == "half1")
        assert (rows[-1] < nrow // 2) == (mode == "half0")
    images, labels = fill(nrow)
    images[rows[0]:rows[0] + B], labels[rows[0]:rows[0] + B] = X, y
    return images, labels, None, c, spe


def launch_train(C, dev, case, mode, B=None, slab=None):
    """One lin_train launch into a NaN slab of ceil(bfull / ROWS) blocks plus guard (or into
    `slab` as it stands).  Checks everything that does not depend on the values; returns the
    slab [blocks, SLAB] on the CPU and the device buffer."""
    bfull = case["bfull"]
    B = B or case["B"]
    images, labels, idx, c, spe = buffers(case["B"], bfull, case["X"], case["y"], mode)
    nfull = -(-bfull // ROWS)
    if slab is None:
        slab = nanbuf(nfull * SLAB, dev)
    metrics = preset(dev)
    c1 = torch.tensor([C1_0], dtype=torch.int64, device=dev)
    ctr = torch.tensor([c, SPARE], dtype=torch.int64, device=dev)
    C.lin_train(images.to(dev), labels.to(dev), None if idx is None else idx.to(dev), ctr[0:1],
                bfull, B, case["W"].to(dev), case["b"].to(dev), slab[:nfull * SLAB], metrics, c1,
                spe=spe)
    torch.cuda.synchronize()
    out = read_guarded(slab, nfull * SLAB, "slab").view(nfull, SLAB)
    nblk = -(-B // ROWS)
    assert torch.isfinite(out[:nblk, :COL_PAD]).all(), "slab element not written"
    assert torch.isnan(out[:nblk, COL_PAD:]).all(), "slab padding written"
    # loss / correct travel in the slab; the sample count alone is added here
    assert metrics.cpu().tolist() == [M0[0], M0[1], M0[2] + B]
    assert c1.item() == C1_0 + 1 and ctr.cpu().tolist() == [c, SPARE]
    return out, slab


def parts(out, nblk):
    return dict(dW=out[:nblk, :NK].reshape(nblk, NC, K), db=out[:nblk, COL_DB:COL_LOSS],
                loss=out[:nblk, COL_LOSS], correct=out[:nblk, COL_OK])


def check_blocks(tag, out, case):
    nblk = -(-case["B"] // ROWS)
    got = parts(out, nblk)
    for q in ("dW", "db", "loss"):
        rule(tag, q, got[q], case["r64"][q], case["r32"][q])
    cor = got["correct"].double()
    assert torch.equal(cor, cor.round())
    off = (cor - case["r64"]["correct"]).abs()
    print(f"LIN {tag} correct: {int(cor.sum())}/{int(case['r64']['correct'].sum())} "
          f"blocks off {int((off > 0).sum())} near rows {case['near']}")
    assert (off <= case["near_blk"]).all(), (tag, off.nonzero()[:4, 0].tolist())
    assert torch.isnan(out[nblk:]).all(), "a block behind the batch was written"


# ------------------------------------------------------------------ 1. one-row blocks, exact
def test_normalize_reference_is_the_fp32_formula():
    """The table the exact test compares against: ((v / 255 - 0.1307) / 0.3081) in correctly
    rounded fp32 operations (numpy scalars), for all 256 bytes."""
    v = np.arange(256, dtype=np.float32)
    t = (v / np.float32(255.0) - np.float32(MNIST_MEAN)) / np.float32(MNIST_STD)
    assert t.dtype == np.float32
    ref = normalize_reference(torch.arange(256, dtype=torch.int32).to(torch.uint8))
    assert np.array_equal(t, ref.numpy())
    assert np.unique(t).size == 256


@functools.lru_cache(maxsize=None)
def exact_case(B):
    g = torch.Generator().manual_seed(40 + B)
    X = torch.randint(0, 256, (B, K), generator=g, dtype=torch.uint8)
    row = torch.cat([torch.arange(256), torch.randint(0, 256, (K - 256,), generator=g)])
    X[B - 1] = row[torch.randperm(K, generator=g)].to(torch.uint8)
    assert torch.unique(X[B - 1]).numel() == 256          # every table entry is read
    assert (X[B - 1, 1:] != X[B - 1, :-1]).float().mean() > 0.98   # a moved byte is another value
    W = torch.randn(NC, K, generator=g) * 0.05
    b = torch.randn(NC, generator=g) * 0.1
    y = torch.randint(0, NC, (B,), generator=g).to(torch.int32)
    return dict(B=B, bfull=8, X=X, W=W, b=b, y=y)


@pytest.mark.parametrize("mode", ["half1", "gather"])
@pytest.mark.parametrize("B", [1, 5])
def test_one_row_block_is_exact(gpu, B, mode):
    """B = 1 (mod 4): the last block has one valid row, so dW[n][k] = fl32(db[n] * x32[k]) and
    db[n] = dl[n] as values: all 256 table entries, put_pixels' byte order, and rows >= nrows
    adding exactly nothing."""
    C = _C()
    case = exact_case(B)
    out, _ = launch_train(C, gpu, case, mode)
    blk = (B - 1) // ROWS
    db = out[blk, COL_DB:COL_LOSS]
    dW = out[blk, :NK].view(NC, K)
    assert (db != 0).all() and torch.isfinite(db).all()
    x32 = normalize_reference(case["X"][B - 1])
    want = db[:, None] * x32[None, :]                      # one correctly rounded fp32 product
    bad = int((dW != want).sum())
    print(f"LIN exact B={B} {mode}: {bad} of {NK} elements differ from fl32(db * x32)")
    assert bad == 0, (bad, (dW != want).nonzero()[:4].tolist())
    # db is dl of the one row: the reference's, by the rule
    r64, r32 = (reference(case["X"], case["y"], case["W"], case["b"], dt) for dt in (D, F32))
    rule(f"exact B={B} {mode}", "db", db[None], r64["db"][blk:blk + 1], r32["db"][blk:blk + 1])


# ------------------------------------------------------------------ 2. lin_train, block by block
TRAIN_CASES = [(1, 8), (5, 8), (13, 32), (64, 64), (96, 256), (256, 256)]
STEEP = (13, 32, 40.0)


def run_modes(C, gpu, case, tag):
    outs = {}
    for mode in MODES:
        out, _ = launch_train(C, gpu, case, mode)
        check_blocks(f"{tag} {mode}", out, case)
        outs[mode] = out
    # the same rows from whichever buffer: the same bits
    nblk = -(-case["B"] // ROWS)
    for mode in MODES[1:]:
        assert torch.equal(outs[mode][:nblk, :COL_PAD].view(torch.int32),
                           outs["flat"][:nblk, :COL_PAD].view(torch.int32)), mode


@pytest.mark.parametrize("B,bfull", TRAIN_CASES)
def test_lin_train_blocks_vs_fp64(gpu, B, bfull):
    """Every block's dW, db, loss and correct on its own, in the four row modes (flat buffer,
    either half of the two-half buffer, sampler gather)."""
    case = train_case(B, bfull)
    assert case["near"] <= (0 if B <= 64 else B // 100), case["near"]     # from the reference alone
    run_modes(_C(), gpu, case, f"train B={B}/{bfull}")


def test_lin_train_steep_logits(gpu):
    """W scaled up until the largest |logit| is past 88.7, where expf overflows in fp32: without
    the max subtraction in row_xent the slab holds inf / NaN."""
    case = train_case(*STEEP)
    top = case["r64"]["logits"].abs().max().item()
    assert top > 88.7, top
    assert case["near"] == 0
    print(f"LIN steep: largest |logit| {top:.1f}")
    run_modes(_C(), gpu, case, "train steep B=13/32")


def tie_case(variant, label):
    """Two rows whose logits are exactly tied between classes 2 and 5, above every other."""
    g = torch.Generator().manual_seed(77)
    X = torch.randint(0, 256, (2, K), generator=g, dtype=torch.uint8)
    b = torch.zeros(NC)
    if variant == "zero_w":
        W = torch.zeros(NC, K)
        b[2] = b[5] = 0.3
    else:                                         # two identical rows of W, equal biases
        W = torch.randn(NC, K, generator=g) * 0.01
        W[2] = W[5] = torch.rand(K, generator=g) * 0.05
        b = torch.randn(NC, generator=g) * 0.1
        b[5] = b[2]
    y = torch.full((2,), label, dtype=torch.int32)
    lg = F.linear(x64(X), W.double(), b.double())
    lg[:, 5] = lg[:, 2]                           # the same products in the same order
    others = lg[:, [0, 1, 3, 4, 6, 7, 8, 9]].max(1).values
    assert (lg[:, 2] - others > 0.25).all()
    assert (lg.argmax(1) == 2).all()              # torch takes the first maximum
    loss64 = (torch.logsumexp(lg, 1) - lg[:, label]).sum().item()
    lg32 = F.linear(normalize_reference(X), W, b)
    loss32 = (torch.logsumexp(lg32, 1) - lg32[:, label]).sum().item()
    return dict(B=2, bfull=8, X=X, W=W, b=b, y=y), loss64, loss32


@pytest.mark.parametrize("label,correct", [(2, 2), (5, 0)])
@pytest.mark.parametrize("variant", ["zero_w", "twin_rows"])
def test_lin_train_tie_takes_first_maximum(gpu, variant, label, correct):
    """row_xent's argmax under an exact tie: the first maximal class, as torch.argmax (the rule
    test_head_argmax_takes_first_maximum pins for the CNN head)."""
    case, loss64, loss32 = tie_case(variant, label)
    out, _ = launch_train(_C(), gpu, case, "flat")
    assert out[0, COL_OK].item() == correct
    k, t = abs(out[0, COL_LOSS].item() - loss64) / loss64, abs(loss32 - loss64) / loss64
    assert k <= max(8 * t, FLOOR), (k, t)


@pytest.mark.parametrize("label,correct", [(2, 2), (5, 0)])
@pytest.mark.parametrize("variant", ["zero_w", "twin_rows"])
def test_lin_eval_tie_takes_first_maximum(gpu, variant, label, correct):
    case, loss64, loss32 = tie_case(variant, label)
    m = preset(gpu)
    _C().lin_eval(case["X"].to(gpu), case["y"].to(gpu), case["W"].to(gpu), case["b"].to(gpu), m)
    m = m.cpu()
    assert m[1].item() == M0[1] + correct and m[2].item() == M0[2] + 2
    k, t = abs(m[0].item() - M0[0] - loss64) / loss64, abs(loss32 - loss64) / loss64
    assert k <= max(8 * t, FLOOR), (k, t)


def test_lin_train_second_launch_into_the_same_slab(gpu):
    """B = 256, then B = 13 into the same slab without poisoning it again: the 4 blocks of the
    second launch are a fresh B = 13 launch's to the bit, blocks 4..63 keep the first launch's."""
    C = _C()
    case = train_case(256, 256)
    first, slab = launch_train(C, gpu, case, "half1")
    small = 13
    nblk = -(-small // ROWS)
    fresh, _ = launch_train(C, gpu, case, "half1", B=small)
    assert torch.isnan(fresh[nblk:]).all()
    # (launch_train's own "all finite" and "padding NaN" hold for blocks 0..3 of the reused slab)
    second, _ = launch_train(C, gpu, case, "half1", B=small, slab=slab)
    bits = lambda t: t.contiguous().view(torch.int32)
    assert torch.equal(bits(second[:nblk]), bits(fresh[:nblk]))
    assert torch.equal(bits(second[nblk:]), bits(first[nblk:]))
    # (1 / 13 in dl, not 1 / 256: the second launch did write)
    assert not torch.equal(bits(second[:nblk, :COL_PAD]), bits(first[:nblk, :COL_PAD]))
    # and the 13-row launch on its own against fp64, block by block
    X, y = case["X"][:small], case["y"][:small]
    r64, r32 = (reference(X, y, case["W"], case["b"], dt) for dt in (D, F32))
    got = parts(second, nblk)
    for q in ("dW", "db", "loss"):
        rule("second launch B=13/256", q, got[q], r64[q], r32[q])


# ------------------------------------------------------------------ 3. lin_reduce
def seq_sum(x):
    """Rows of x added one after the other, in ascending order, from 0, in fp32 (np.sum and
    torch.sum add pairwise)."""
    s = torch.zeros(x.shape[1], dtype=F32)
    for j in range(x.shape[0]):
        s = s + x[j]
    return s


@functools.lru_cache(maxsize=None)
def random_slabs(nblk):
    """nblk slabs as lin_train leaves them (loss >= 0, correct in 0..ROWS, padding NaN) with
    gradient values of mixed magnitude, and two NaN slabs behind them that no launch may read."""
    g = torch.Generator().manual_seed(300 + nblk)
    slab = torch.full((nblk + 2, SLAB), NAN)
    scale = torch.exp2(torch.randint(-6, 3, (nblk, COL_LOSS), generator=g).float())
    slab[:nblk, :COL_LOSS] = torch.randn(nblk, COL_LOSS, generator=g) * scale
    slab[:nblk, COL_LOSS] = torch.rand(nblk, generator=g) * 10
    slab[:nblk, COL_OK] = torch.randint(0, ROWS + 1, (nblk,), generator=g).float()
    want = seq_sum(slab[:nblk, :COL_LOSS])
    if nblk > 2:      # the test can tell the documented order from the reverse one
        assert (want != seq_sum(slab[:nblk, :COL_LOSS].flip(0))).float().mean() > 0.05
    return slab, want


def check_metrics(m, slab, nblk, tag):
    """metrics[0..1] advanced by the fp64 sums of the loss / correct columns: against math.fsum
    of the preset and the nblk column values, within nblk additions' worth of fp64 rounding."""
    for j, col in enumerate((COL_LOSS, COL_OK)):
        terms = [M0[j]] + slab[:nblk, col].double().tolist()
        want, scale = math.fsum(terms), math.fsum(abs(v) for v in terms)
        assert abs(m[j].item() - want) <= nblk * U53 * scale, (tag, j, m[j].item(), want)
    assert m[2].item() == M0[2]                   # the sample count is lin_train's


def slab_unchanged(sd, slab):
    """The launches only read the slab: every bit as uploaded, the NaN padding columns and the
    two NaN slabs behind the valid ones included."""
    return torch.equal(sd.cpu().view(torch.int32), slab.reshape(-1).view(torch.int32))


@pytest.mark.parametrize("short", [0, 3])
@pytest.mark.parametrize("nblk", [1, 7, 8, 9, 17, 64])
def test_lin_reduce_sums_in_ascending_order(gpu, nblk, short):
    """lin_reduce on random slabs: gW / gb are the sequential fp32 sum over the slabs in
    ascending order, as values; the metrics workgroup; metrics=None; the counter."""
    C = _C()
    B = ROWS * nblk - short
    slab, want = random_slabs(nblk)
    sd = slab.reshape(-1).to(gpu)
    c0 = torch.tensor([41], dtype=torch.int64, device=gpu)
    res = []
    for metrics in (preset(gpu), None):
        gW, gb = nanbuf(NK, gpu), nanbuf(NC, gpu)
        C.lin_reduce(sd, B, gW[:NK], gb[:NC], c0, None, metrics)
        torch.cuda.synchronize()
        got = torch.cat([read_guarded(gW, NK, "gW"), read_guarded(gb, NC, "gb")])
        bad = int((got != want).sum())             # NaN != anything: padding / later slabs show
        assert bad == 0, (metrics is not None, bad, (got != want).nonzero()[:4, 0].tolist())
        res.append(got)
    assert c0.item() == 43                          # one step per launch
    assert torch.equal(res[0].view(torch.int32), res[1].view(torch.int32))
    m = preset(gpu)
    C.lin_reduce(sd, B, nanbuf(NK, gpu)[:NK], nanbuf(NC, gpu)[:NC], None, None, m)
    check_metrics(m.cpu(), slab, nblk, f"lin_reduce nblk={nblk}")
    assert slab_unchanged(sd, slab)


# ------------------------------------------------------------------ 4. the fused optimizer
@pytest.mark.parametrize("nblk", [1, 13, 16, 17, 64])
@pytest.mark.parametrize("kind,h,step", KIND_HYPER)
def test_fused_optimizer_on_the_linear_geometry(gpu, kind, h, step, nblk):
    """optim_step with LinearStep._fused_segments' two slab segments on one shared slab, the
    metrics tuple (column 7850, stride LIN_SLAB) and bump."""
    C = _C()
    spec = get_spec("linear")
    ow, ob, total = spec.offset("fc.weight"), spec.offset("fc.bias"), spec.total
    assert ow + NK <= ob and ob + NC < total        # arena padding behind both segments
    slab, seq = random_slabs(nblk)
    sd = slab.reshape(-1).to(gpu)
    g = torch.Generator().manual_seed(900 + nblk)
    p0, g0, m0 = (torch.randn(total, generator=g) * s for s in (1.0, 1.0, 0.5))
    v0 = torch.randn(total, generator=g) ** 2
    sw, sb = slice(ow, ow + NK), slice(ob, ob + NC)
    g0[sw] = g0[sb] = NAN                           # the launch overwrites them with the sums
    P, G, M = (Guarded(t, gpu) for t in (p0, g0, m0))
    V = Guarded(v0, gpu) if kind == "adam" else None
    bump = torch.tensor([41], dtype=torch.int64, device=gpu)
    mets = preset(gpu)
    sl = lambda col: (sd, nblk, col, SLAB)
    segs = [(ow, NC, K, None, None, sl(0)), (ob, 1, NC, None, None, sl(COL_DB))]
    launch(C, gpu, kind, h, step, P.view, G.view, M.view, V.view if V else None, segs,
           bump=bump, metrics=(sd, nblk, COL_LOSS, SLAB, mets))
    assert bump.item() == 42
    got = {"p": P.read(), "g": G.read(), "m": M.read()}
    ins = {"p": p0, "g": g0, "m": m0}
    if V:
        got["v"], ins["v"] = V.read(), v0
    # the reduced gradient left in the arena: the documented order, as values
    two = slab[:nblk]
    gw, gbias = slab_sum(two, 0, NK), slab_sum(two, COL_DB, NC)
    assert int((got["g"][sw] != gw).sum()) == 0 and int((got["g"][sb] != gbias).sum()) == 0
    if nblk <= 16:                                  # one slab per group: the sequential sum
        assert int((got["g"][sw] != seq[:NK]).sum()) == 0
        assert int((got["g"][sb] != seq[COL_DB:COL_LOSS]).sum()) == 0
        gW, gb = nanbuf(NK, gpu), nanbuf(NC, gpu)
        C.lin_reduce(sd, ROWS * nblk, gW[:NK], gb[:NC])
        torch.cuda.synchronize()
        assert int((got["g"][sw] != read_guarded(gW, NK, "gW")).sum()) == 0
        assert int((got["g"][sb] != read_guarded(gb, NC, "gb")).sum()) == 0
    # parameters and moments from that gradient: test_gpu_optim.py's fp64 rule
    for name, s, gin in (("fc.weight", sw, gw), ("fc.bias", sb, gbias)):
        measure(f"linear-fused nblk={nblk} {name}", kind, h, step, p0[s], gin, m0[s], v0[s],
                {k: got[k][s] for k in ("p", "m", "v") if k in got})
    # nothing else moves: slab columns 7850 / 7851 (the float4 group of the bias' tail) and the
    # NaN padding reach no parameter, moment or gradient
    covered = torch.zeros(total, dtype=torch.bool)
    covered[sw] = covered[sb] = True
    for k in got:
        assert torch.equal(got[k][~covered].view(torch.int32), ins[k][~covered].view(torch.int32)), k
        assert torch.isfinite(got[k][covered]).all(), k
    check_metrics(mets.cpu(), slab, nblk, f"optim nblk={nblk}")
    assert slab_unchanged(sd, slab)


# ------------------------------------------------------------------ 5. lin_eval
EVAL_SEED = {1: 1, 15: 115, 16: 16, 17: 17, 33: 33, 1000: 1000}   # chosen on the CPU: the near-tie caps


@functools.lru_cache(maxsize=None)
def eval_case(N):
    g = torch.Generator().manual_seed(EVAL_SEED[N])
    X = torch.randint(0, 256, (N, K), generator=g, dtype=torch.uint8)
    W = torch.randn(NC, K, generator=g) * 0.05
    b = torch.randn(NC, generator=g) * 0.1
    y = half_argmax_labels(F.linear(x64(X), W.double(), b.double()), g)
    r64, r32 = reference(X, y, W, b, D), reference(X, y, W, b, F32)
    return dict(X=X, W=W, b=b, y=y, loss64=r64["rowloss"].sum().item(),
                loss32=r32["rowloss"].sum().item(), correct=int(r64["hit"].sum()),
                near=int(near_rows(r64["logits"]).sum()))


@pytest.mark.parametrize("N", [1, 15, 16, 17, 33, 1000])
def test_lin_eval_edges(gpu, N):
    """lin_eval around its 16-row blocks (N = 17 and 33 leave one valid row in the last block),
    from a preset: count exact, correct exact outside near ties, the loss sum by the 8 x rule;
    a second call adds the same again."""
    C = _C()
    case = eval_case(N)
    near = case["near"]
    assert near <= (0 if N <= 64 else N // 100), near                     # from the reference alone
    args = (case["X"].to(gpu), case["y"].to(gpu), case["W"].to(gpu), case["b"].to(gpu))
    m = preset(gpu)
    C.lin_eval(*args, m)
    m1 = m.cpu().clone()
    C.lin_eval(*args, m)
    m2 = m.cpu()
    loss, cor = m1[0].item() - M0[0], m1[1].item() - M0[1]
    k = abs(loss - case["loss64"]) / case["loss64"]
    t = abs(case["loss32"] - case["loss64"]) / case["loss64"]
    print(f"LIN eval N={N}: loss {k:.1e}|{t:.1e}  correct {cor:.0f}/{case['correct']} near {near}")
    assert m1[2].item() == M0[2] + N
    assert cor == int(cor) and abs(cor - case["correct"]) <= near
    assert k <= max(8 * t, FLOOR), (k, t)
    # the second call: the counts exactly; the loss within the roundings of the fp64 atomic adds
    # (one per block and call, each at most 2^-53 of the running sum, and the two differences)
    assert m2[1].item() - m1[1].item() == cor and m2[2].item() == M0[2] + 2 * N
    nblk = -(-N // EVAL_ROWS)
    assert abs((m2[0].item() - m1[0].item()) - loss) <= (2 * nblk + 2) * U53 * m2[0].item()
