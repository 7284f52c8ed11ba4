"""The bf16 program's kernels (csrc/kernels/cnn_fwd.hip, cnn_fwd_band.hip, fc1_fwd.hip,
fc1_bwd.hip, cnn_bwd.hip, cnn_bwd_band.hip) called one by one on synthetic tensors, every output
element by element against an fp64 reference computed on the CPU from the very operands the
kernel read.  The plan and the helpers are tests/test_gpu_cnn_f32_kernels.py's:

    cnn_fwd / cnn_fwd_band   row, data-step counter (flat and two-half buffer) and sampler-gather
                             modes; training (uint8 hand-off, a1 / x hand-off) and evaluation
    fc1_fwd                  every split on its own, 32-row and 128-row blocks
    fc1_bwd                  dX and the head-slab reduction (dW: test_gpu_fc1_update.py)
    cnn_bwd / cnn_bwd_band   every slab on its own, before any reduction
    conv_reduce              on random slabs, pinned to its summation order

Every output buffer is pre-filled with a sentinel (NaN, 0x55 bytes, the bf16 NaN 0x7fc1) and
allocated larger than the kernel's contract: inside the contract every element is written,
outside it the sentinel survives.

fp32 outputs (fc1 partials, conv slabs, reduced gradients): the fp32 file's measure.  For
y = sum_k a_k b_k the reference forms s = sum_k |a_k| |b_k|, e = max |got - ref| / s (s == 0:
exactly 0), the same arithmetic in fp32 torch gives e_ref, and e <= 8 e_ref, e <= K 2^-24 with K
the number of summed terms.

bf16 outputs (a1g, pool, dpool): the kernel stores the round-to-nearest-even bf16 of an fp32
accumulator.  With z the fp64 value before the rounding (and before ReLU / max-pool where the
kernel applies them to the accumulator), t = min(8 max(e_ref, 2^-24), K 2^-24) s per element,
lo = post(bf16(z - t)) and hi = post(bf16(z + t)) (post = the kernel's ReLU and window max; both
monotone, so they commute with the rounding), the stored bits must satisfy lo <= got <= hi in
the order of the bf16 values.  Where lo == hi, all but the values within t of a rounding
boundary, that is bit equality.  From the reference alone: at most 5 % of an output's elements
have lo != hi.  bf16(.) of an fp64 value is computed in fp64 (frexp / round / ldexp): torch's
conversion goes through fp32 and rounds twice.

Exact conv1 inputs ("grid").  Pixel bytes from the values whose normalised bf16 value is a
multiple of 2^-10 (asserted: every byte but 24..37), w1 = k / 16 (|k| <= 16), b1 = k / 16
(|k| <= 8): every partial sum of conv1 is a multiple of 2^-14 below 2^5, so conv1 is exact in
fp32 in any order and a1 = bf16(relu(fp64 conv1)) is the only value a kernel may produce
(grid_a1 asserts it: two fp32 orders equal fp64).  They are used wherever the kernel hides its
a1 (cnn_fwd with one workgroup per image, cnn_bwd); where a1 is handed out (the band forward)
general inputs are used and conv2 is referred to the a1 of the same launch.

conv1 gradients.  The kernels round dz1 = da1 relu'(a1) to bf16 as the conv1-wgrad MFMA operand.
The reference computes da1 in fp64 (K = 576), takes bf16(da1) as the operand and forms
dz1_lo / dz1_hi by the interval rule; the ambiguity D = |dz1_hi - dz1_lo| carried through the
same sums (conv2d_weight(|x|, D), sum D) is allowed on top of the fp32 measure with K = 676 per
image (the products of two bf16 values are exact in fp32; what da1's own error can change is
the rounding of dz1, which D holds).

The bias gradients db2 and db1 are sums of bare bf16 values (8 significant bits, a few binades
apart): most of their fp32 sums are exact in any order, so e_ref is 0, or one rounding of one
element, by chance, and a kernel that rounds once elsewhere (5.9e-9 against 0 was measured)
would miss 8 e_ref.  For these two outputs e_ref is taken as at least 2^-24, one fp32
rounding of the sum, the floor the interval rule uses as well.

Max-pool ties, the special image rows and the seam probe: the fp32 file's docstring.  The
probe's rows (pooled rows 2k - 1, 2k, 0, 11; a1 rows 0, 1, 24, 25, 4k - 2 .. 4k + 1) are every
pooled row and every a1 row but 22 and 23, and every x row lies under one of those a1 rows (no
byte normalises to 0 either): in the forward the probe is the full image, so every forward
case is one, each output row compared per element on both sides of every 4-, 8- and 12-row
seam.  The backward has its own probe cases (dpool and a1 confined as in the fp32 file).

fc1_fwd's contract has no padding rows: split s starts at part + s B 128, so a row >= B of one
split is a row of the next.  `part` gets one extra row block behind the last split, which must
keep its NaN; a store past row B - 1 of an earlier split lands in the next split's rows, which
are compared per element.

Measured on MI355X, e_kernel | e_ref, each the largest over the cases of its test, and the
largest ratio e_kernel / e_ref of any one case (the bound is 8; "=" marks outputs that were
bit-equal to the fp32 emulation of the kernel's documented order in every case):

    kernel                 output  e_kernel | e_ref    ratio   K
    fc1_fwd  S = 1         part    1.3e-07 | 2.6e-08   5.2     9216
             S = 4         part    1.1e-07 | 2.6e-08   4.3     2304
             S = 16 .. 96  part    1.3e-07 | 1.6e-07   2.0     576 .. 96
    fc1_bwd  head slabs    gwf2    8.9e-08 | 8.9e-08   =       hb = 8, 16, 40
                           gbf2    3.0e-08 | 3.0e-08   =
                           gbf1    7.0e-08 | 7.0e-08   =
    cnn_bwd                gw2     1.3e-07 | 8.6e-08   2.0     576 per image
                           gb2     1.3e-08 | 1.3e-08   5.9e-9 against 0 once (floor 2^-24)
                           gw1     3.3e-08 | 3.3e-08   1.5     676 per image
                           gb1     0       | 5.6e-09   0
    cnn_bwd_band           gw2     1.2e-07 | 1.3e-07   1.5     24 R
                           gb2     1.4e-08 | 1.4e-08   1.0     6 R
                           gw1     1.4e-08 | 4.9e-08   0.6     676
                           gb1     0       | 9.3e-09   0
    conv_reduce            all     1.5e-07 | 1.5e-07   =       nblk = 1, 2, 7, 300

bf16 outputs, all inside [lo, hi]; e_ref of the value before the rounding and the share of
elements with lo != hi (the cap is 5 %):

    cnn_fwd_band  a1g    e_ref 6.9e-08 .. 1.4e-07   0.00 % .. 0.14 %   (grid inputs: bit-equal)
    cnn_fwd*      pool   e_ref 4.9e-08 .. 8.6e-08   0.00 % .. 1.26 %
    fc1_bwd       dpool  e_ref 6.5e-08 .. 1.8e-07   1.03 % (B = 1), 1.40 % (33), 2.03 % (160)
    cnn_bwd*      dz1    (reference only)           0.29 % .. 0.42 %

After the rounding pool is within 5.8e-4 .. 1.2e-3 of relu(max z) / s, the scale the norm bounds
of test_gpu_cnn.py see.  Windows left out of the pmask comparison: 0 .. 3.3e-04 of all windows
(cap 1e-2); pooled values <= -DELTA: 52 % .. 93 %.  45 % .. 52 % of the exact-conv1 a1 values need
a genuine bf16 rounding.  In the conv1 gradients the dz1 ambiguity is on average 45 % .. 80 % of
an element's allowance and at most 1.5e-3 of s; before it is taken off, |got - ref| / s reaches
4.0e-05 (a dz1 that rounded the other way), after it the gw1 / gb1 rows above.  xg, xng, ylab,
the evaluation template's pool / ylab and every output of a second launch were bit-identical in
every case.  (The e_ref columns depend on the host's BLAS.)

Mutations, five in one scratch build (one per source file, arithmetic or in-bounds index only),
run once; "old" = the parent's kernel-level tests (test_gpu_cnn.py, test_gpu_cnn_bwd_exact.py,
test_gpu_fc1_update.py, test_gpu_cnn_head.py):

    cnn_fwd       pooled value rounded twice (16 significant bits, then bf16): 6 of the 9
                  bands = 1 cases fail, on 1 to 4 of 9216 B values, each one bf16 step off.  old:
                  test_cnn_forward_kernels (norms) passes; test_cnn_forward_band_split fails,
                  only because cnn_fwd_band did not carry the same mutation
    cnn_fwd_band  the evaluation template writes pmask: all 30 band cases fail.  old: passes
    fc1_fwd       partial stored to the mirrored split slot: every S > 1 case fails (e up to 1.1
                  against a cap of 5.7e-6).  old: test_fc1_fwd_split_k passes
    fc1_bwd       metrics overwritten instead of advanced: all 3 cases fail.  old:
                  test_fc1_bwd_exact passes (it starts from 0); two whole-epoch tests fail
    cnn_bwd       dz1 rounded twice: all 4 bands = 1 cases fail on gw1 (1.5e-5 .. 2.5e-4 of s left
                  after the allowance).  old: test_cnn_bwd_exact fails 3 of 4 bands = 1 cases

(test_cnn_step_gradients_match_autograd[300] also failed under the combined build; which
mutation it saw was not separated.)
"""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from pytorch_distributed_mnist_amd.data.mnist import normalize_reference
from pytorch_distributed_mnist_amd.runtime.cnn_step import a1_swizzled, frag_major
from test_gpu_cnn_f32_kernels import (BFULL, C1, C2, DELTA, FEAT, HID, M0, MARGIN, NROW, P1, SPE,
                                      U24, _C, check_pmask, elementwise, fc_w1, fwd_inputs, nan_f32,
                                      nchw_w2, nhwc, seam_rows, step_row, window_ties, windows,
                                      written)
from test_gpu_fc1_update import Fc1Bwd
from test_gpu_optim import BF, F32, Guarded, same_bits, sentinel, slab_sum

pytestmark = pytest.mark.gpu

I55 = 0x55555555
MAX_AMBIGUOUS = 0.05          # share of a bf16 output's elements with lo != hi


# ---------------------------------------------------------------- helpers
def bf(t):
    return t.to(BF).to(torch.float32)


def bf16_of(z):
    """fp64 -> the nearest bf16 (ties to even), one rounding."""
    m, e = torch.frexp(z)                                # z = m 2^e, 0.5 <= |m| < 1
    return torch.ldexp(torch.round(m * 256.0), e - 8).to(torch.float32).to(BF)


def key16(t):
    """bf16 -> int32 keys in the order of the values (-0 below +0)."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i >= 0, i, -(i & 0x7fff) - 1)


def relu16(v):
    """bf16 -> relu as the kernels take it on the bit patterns: -0 becomes +0."""
    return (torch.relu(v.float()) + 0.0).to(BF)


def poison16(n, dev):
    return torch.full((n,), 0x5555, dtype=torch.int16, device=dev).view(BF)


def e_of(x, ref, s):
    nz = s > 0
    return ((x.double() - ref).abs()[nz] / s[nz]).max().item() if nz.any() else 0.0


def interval(tag, z, s, emu, K, post=lambda v: v):
    """The module docstring's bounds of one bf16 output, from the reference alone: (lo, hi) as
    int32 keys.  z, s fp64, emu the same arithmetic in fp32 torch, all before the rounding."""
    e_r = e_of(emu, z, s)
    t = min(MARGIN * max(e_r, U24), K * U24) * s
    lo, hi = key16(post(bf16_of(z - t))), key16(post(bf16_of(z + t)))
    assert (lo <= hi).all(), tag
    share = (lo != hi).double().mean().item()
    print(f"bf16k {tag}: e_ref {e_r:.2e}, lo != hi for {share:.2%} of {lo.numel()} elements")
    assert share <= MAX_AMBIGUOUS, (tag, share)
    return lo, hi


def inside(tag, got, bounds):
    lo, hi = bounds
    k = key16(got).view(lo.shape)
    bad = (k < lo) | (k > hi)
    assert not bad.any(), (tag, int(bad.sum()), k[bad][:8].tolist(), lo[bad][:8].tolist(),
                           hi[bad][:8].tolist())
    return (lo != hi).double().mean().item()


# ---------------------------------------------------------------- exact conv1 inputs
@functools.lru_cache(maxsize=None)
def grid_bytes():
    """The byte values whose normalised bf16 value is a multiple of 2^-10."""
    v = bf(normalize_reference(torch.arange(256, dtype=torch.uint8).view(1, 256))).double().view(-1)
    ok = (v * 1024.0) == torch.round(v * 1024.0)
    assert (~ok).nonzero().view(-1).tolist() == list(range(24, 38))
    return torch.arange(256, dtype=torch.uint8)[ok]


def grid_conv1(gen):
    w1 = torch.randint(-16, 17, (C1, 9), generator=gen).float() / 16.0
    b1 = torch.randint(-8, 9, (C1,), generator=gen).float() / 16.0
    return w1, b1


def grid_pixels(gen, shape):
    ok = grid_bytes()
    return ok[torch.randint(0, ok.numel(), shape, generator=gen)]


def grid_a1(images, w1, b1):
    """bf16(relu(conv1)) [B, 32, 26, 26] of grid inputs, after asserting that conv1 is exact in
    fp32 whatever the order: the library's order and taps last to first, bias last, both equal
    fp64, every value a multiple of 2^-14 below 2^5."""
    B = images.shape[0]
    assert torch.isin(images, grid_bytes()).all()
    assert torch.equal(bf(w1), w1) and torch.equal(w1 * 16, torch.round(w1 * 16)) and w1.abs().max() <= 1
    assert torch.equal(b1 * 16, torch.round(b1 * 16)) and b1.abs().max() <= 0.5
    xn = bf(normalize_reference(images)).view(B, 1, 28, 28)
    z = F.conv2d(xn.double(), w1.view(C1, 1, 3, 3).double(), b1.double())
    a = F.conv2d(xn, w1.view(C1, 1, 3, 3), b1)
    b = torch.zeros(B, C1, 26, 26)
    for tap in reversed(range(9)):
        ky, kx = divmod(tap, 3)
        b = b + xn[:, :, ky:ky + 26, kx:kx + 26] * w1[:, tap].view(1, C1, 1, 1)
    b = b + b1.view(1, C1, 1, 1)
    assert torch.equal(a.double(), z) and torch.equal(b.double(), z), "conv1 is not exact in fp32"
    assert torch.equal(z * 2.0 ** 14, torch.round(z * 2.0 ** 14)) and z.abs().max() < 32
    a1 = bf16_of(torch.relu(z))
    rounded = (a1.double() != torch.relu(z)).double().mean().item()
    print(f"bf16k exact conv1: {rounded:.0%} of the a1 values need a genuine bf16 rounding")
    assert rounded > 0
    return a1.float()


# ---------------------------------------------------------------- 1. cnn_fwd, cnn_fwd_band
IDX_CTR = 2                   # sampler-gather mode: rows idx[2 * BFULL + i]
# (mode, B, arg): row offset / counter.  "flat": counter mode with spe = 0 (rows 4 c + i);
# "half": spe = 3, the fp32 file's step_row geometry; "idx": sampler gather
FWD_MODES = [("row", 1, 0), ("row", 3, 0), ("row", 3, 3), ("flat", 3, 4), ("flat", 1, 5),
             ("half", 3, 5), ("half", 3, 7), ("half", 1, 7), ("idx", 3, IDX_CTR)]
FWD_CASES = ([(m, B, a, bands, "grid") for (m, B, a) in FWD_MODES for bands in (1,)]
             + [(m, B, a, bands, "general") for (m, B, a) in FWD_MODES for bands in (2, 3, 6)]
             + [("row", 3, 0, bands, "grid") for bands in (2, 3, 6)])


@functools.lru_cache(maxsize=None)
def fwd_case_inputs(kind):
    """The fp32 file's 22-row buffer (special rows 1, 21: all 0; 3, 5: all 255; 2, 20: the ring)
    and weights, in the bf16 kernels' operand types.  general: w1 and w2 rounded to bf16; grid:
    exact conv1 inputs."""
    images, labels, w1, b1, w2, b2 = fwd_inputs()
    w1, w2 = bf(w1), w2.to(BF)
    if kind == "grid":
        g = torch.Generator().manual_seed(4321)
        images = grid_pixels(g, (NROW, 784))
        ring = torch.zeros(28, 28, dtype=torch.uint8)
        ring[0], ring[27], ring[:, 0], ring[:, 27] = 200, 255, 41, 129
        for r, v in ((1, 0), (21, 0), (3, 255), (5, 255)):
            images[r] = v
        images[2] = ring.view(-1)
        images[20] = ring.view(-1)
        w1, b1 = grid_conv1(g)
    return images.contiguous(), labels, w1, b1, w2, b2


@functools.lru_cache(maxsize=None)
def gather_idx():
    return torch.randperm(NROW, generator=torch.Generator().manual_seed(9)).to(torch.int32)


def fwd_rows(mode, B, arg):
    if mode == "row":
        return [arg + i for i in range(B)]
    if mode == "flat":
        return [step_row(BFULL, 0, NROW, arg, i) for i in range(B)]
    if mode == "half":
        return [step_row(BFULL, SPE, NROW, arg, i) for i in range(B)]
    return [int(gather_idx()[step_row(BFULL, 0, NROW, arg, i)]) for i in range(B)]


def launch_fwd(C, dev, kind, mode, B, arg, bands, tmpl):
    """tmpl: "xg" (training, uint8 hand-off), "a1" (training, a1 / x hand-off), "eval"."""
    images, labels, w1, b1, w2, b2 = fwd_case_inputs(kind)
    o = dict(pool=poison16((B + 1) * FEAT, dev),
             pmask=torch.full(((B + 1) * FEAT,), 0x55, dtype=torch.uint8, device=dev),
             ylab=torch.full((B + 1,), I55, dtype=torch.int32, device=dev))
    xg = a1g = xng = None
    if tmpl == "xg":
        o["xg"] = xg = torch.full(((B + 1) * 784,), 0x55, dtype=torch.uint8, device=dev)
    elif tmpl == "a1":
        o["a1g"] = a1g = poison16((B + 1) * P1 * C1, dev)
        o["xng"] = xng = poison16((B + 1) * 784, dev)
    idx = ctr = None
    im, lb, bfull, spe = images.to(dev), labels.to(dev), BFULL, 0
    if mode == "row":
        im, lb, bfull = images[arg:].to(dev), labels[arg:].to(dev), B
    else:
        ctr = torch.tensor([arg], dtype=torch.int64, device=dev)
        spe = SPE if mode == "half" else 0
        if mode == "idx":
            idx = gather_idx().to(dev)
    C.cnn_fwd(im, lb, idx, ctr, bfull, B, w1.reshape(-1).to(dev), b1.to(dev),
              frag_major(w2.view(C2, 288)).to(dev), b2.to(dev), o["pool"], o["pmask"], xg,
              o["ylab"], bands, a1g, xng, spe=spe)
    torch.cuda.synchronize()
    if ctr is not None:
        assert ctr.item() == arg                       # the forward does not advance it
    return {k: v.cpu() for k, v in o.items()}


def bits_written(buf, n, poison, name):
    """buf (CPU, poisoned before the launch): returns [0, n); the rest is still poison."""
    raw = buf.view(torch.int16) if buf.dtype == BF else buf
    assert buf.numel() > n and (raw[n:] == poison).all(), f"{name}: written past the contract"
    return buf[:n]


@pytest.mark.parametrize("mode,B,arg,bands,kind", FWD_CASES)
def test_cnn_fwd(gpu, mode, B, arg, bands, kind):
    """cnn_fwd (bands 1) / cnn_fwd_band: ylab, xg, xng bit for bit; a1g, pool by the interval
    rule (grid inputs: a1g bit-equal); pmask; the evaluation template writes no pmask and the
    same pool / ylab bits."""
    C = _C()
    images, labels, w1, b1, w2, b2 = fwd_case_inputs(kind)
    rows = fwd_rows(mode, B, arg)
    assert max(rows) < NROW
    tag = f"fwd {kind} {mode}{arg} B={B} bands={bands}"

    # ---- the reference, and every condition on it, before any output is looked at
    xn = bf(normalize_reference(images[rows]))
    x64 = xn.double().view(B, 1, 28, 28)
    w1n = w1.view(C1, 1, 3, 3)
    a1_bounds = None
    if kind == "grid":
        a1_op = grid_a1(images[rows], w1, b1)                       # [B, 32, 26, 26]
    else:
        z1 = F.conv2d(x64, w1n.double(), b1.double())
        s1 = F.conv2d(x64.abs(), w1n.double().abs(), b1.double().abs())
        a1_bounds = interval(f"{tag} a1", z1, s1, F.conv2d(xn.view(B, 1, 28, 28), w1n, b1), 10,
                             relu16)
        a1_op = None                                                # the launch's own hand-off

    tr = {"xg": launch_fwd(C, gpu, kind, mode, B, arg, bands, "xg")}
    if bands > 1:
        tr["a1"] = launch_fwd(C, gpu, kind, mode, B, arg, bands, "a1")
    ev = launch_fwd(C, gpu, kind, mode, B, arg, bands, "eval")

    # ---- exact outputs
    for name, o in list(tr.items()) + [("eval", ev)]:
        assert o["ylab"][:B].tolist() == labels[rows].tolist(), name
        assert (o["ylab"][B:] == I55).all(), name
    xg = bits_written(tr["xg"]["xg"], B * 784, 0x55, "xg").view(B, 784)
    assert torch.equal(xg, images[rows]), "xg is not the selected rows"
    if bands > 1:
        xng = bits_written(tr["a1"]["xng"], B * 784, 0x5555, "xng").view(B, 784)
        assert same_bits(xng, normalize_reference(images[rows]).to(BF)), "xng != bf16(normalize)"
        a1g = bits_written(tr["a1"]["a1g"], B * P1 * C1, 0x5555, "a1g")
        a1k = a1_swizzled(a1g.view(B, P1, C1)).view(B, 26, 26, C1).permute(0, 3, 1, 2).contiguous()
        assert (key16(a1k) >= 0).all()                              # no negative, no -0
        if kind == "grid":
            assert same_bits(a1k, a1_op.to(BF)), "a1g != bf16(relu(conv1)) of exact inputs"
        else:
            share = inside(f"{tag} a1", a1k, a1_bounds)
            print(f"bf16k {tag}: a1g inside its bounds ({share:.2%} ambiguous)")
            a1_op = a1k.float()

    # ---- conv2 + pool from the a1 the kernel read
    W64 = nchw_w2(w2.float().reshape(-1)).double()
    a64 = a1_op.double()
    z2 = F.conv2d(a64, W64, b2.double())
    s2 = F.conv2d(a64, W64.abs(), b2.double().abs())
    z2_emu = F.conv2d(a1_op, nchw_w2(w2.float().reshape(-1)), b2)
    m64, gap, want, tied = window_ties(a1_op, z2)
    near = (m64.abs() < DELTA) | (gap <= DELTA)
    share = near.double().mean().item()
    nonpos = (m64 <= -DELTA).double().mean().item()
    print(f"bf16k {tag}: windows within delta {share:.2e}, pooled <= -delta {nonpos:.2f}, "
          f"windows whose maximum has identical copies {tied.double().mean().item():.2f}")
    assert share <= 0.01, share
    assert 0.05 <= nonpos <= 0.95, nonpos

    def post(v):         # bf16 [B, 64, 24, 24] -> relu, window max, the kernels' [B][pp][co]
        return relu16(nhwc(windows(v.float()).max(-1).values))

    # the tolerance of a window is that of its own positions: s per position, max after
    pool_bounds = interval(f"{tag} pool", z2, s2, z2_emu, 289, post)

    first = tr["a1"] if bands > 1 else tr["xg"]
    pool = bits_written(first["pool"], B * FEAT, 0x5555, "pool").view(B, FEAT)
    assert (pool.view(torch.int16) != 0x5555).all(), "pool: unwritten inside the contract"
    inside(f"{tag} pool", pool, pool_bounds)
    e_k = e_of(pool.float(), nhwc(torch.relu(m64)), nhwc(windows(s2).max(-1).values))
    print(f"bf16k {tag}: pool after the rounding, max |got - relu(max z)| / s = {e_k:.2e}")
    pmask = bits_written(first["pmask"], B * FEAT, 0x55, "pmask").view(B, FEAT)
    check_pmask(pmask, pool.float(), nhwc(m64), nhwc(gap), nhwc(want))

    # ---- the other templates store the same bits; evaluation leaves pmask alone
    for name, o in list(tr.items()) + [("eval", ev)]:
        assert same_bits(bits_written(o["pool"], B * FEAT, 0x5555, name).view(B, FEAT), pool), name
        if name != "eval":
            assert torch.equal(bits_written(o["pmask"], B * FEAT, 0x55, name).view(B, FEAT), pmask)
    assert (ev["pmask"] == 0x55).all(), "the evaluation template wrote pmask"


# ---------------------------------------------------------------- 2. fc1_fwd
FC1_FWD = ([(B, S) for B in (1, 33) for S in (1, 32, 48, 96)]
           + [(2048, 1), (2048, 16), (2049, 4)])
# S = 1 is one fp32 accumulator chain over all 9216 features (288 MFMA steps of 32 products),
# where the host BLAS blocks K and sums short chains (the fp32 file's MARGIN_FC1_FWD_EXACT).  The
# bf16 kernel stays inside the common margin: 5.2 x at S = 1, 4.3 x at S = 4, <= 2 x from 16 on.


@pytest.mark.parametrize("B,S", FC1_FWD)
def test_fc1_fwd(gpu, B, S):
    """Every split's partial on its own against fp64 of its contiguous 9216 / S features (9-k-step
    batches for S | 32, 3-k-step batches for 48 / 96, 128-row blocks from B = 2048 on with a
    ragged last block of one row at B = 2049)."""
    C = _C()
    g = torch.Generator().manual_seed(100 * B + S)
    pool = torch.randn(B, FEAT, generator=g).to(BF)
    w1 = (fc_w1() * 0.05).to(BF)
    rb = 128 if B >= C.FC1_BIG_B else 32
    n = S * B * HID
    part = nan_f32(n + rb * HID, gpu)
    C.fc1_fwd(pool.to(gpu), frag_major(w1).to(gpu), part, B, S)
    torch.cuda.synchronize()
    got = written(part.cpu(), n, "part").view(S, B, HID)
    K = FEAT // S

    def mm(p, w):
        return torch.einsum("bsk,nsk->sbn", p.view(B, S, K), w.view(HID, S, K))

    p64, w64 = pool.double(), w1.double()
    elementwise(f"fc1_fwd B={B} S={S}", got, mm(p64, w64), mm(p64.abs(), w64.abs()),
                mm(pool.float(), w1.float()), K, False)


# ---------------------------------------------------------------- 3. fc1_bwd: dX, head slabs
def head_sum(slab):
    """fc1_bwd's head-slab order in fp32: group g adds slabs g, g + 4, ... in ascending order
    from 0, then ((g0 + g1) + g2) + g3."""
    acc = []
    for grp in range(4):
        a = torch.zeros(slab.shape[1], dtype=F32)
        for j in range(grp, slab.shape[0], 4):
            a = a + slab[j]
        acc.append(a)
    return ((acc[0] + acc[1]) + acc[2]) + acc[3]


def run_fc1_bwd(pr):
    """One launch of an Fc1Bwd problem without the fused update: dpool over-allocated by the
    padding rows of ldt and one more, metrics pre-set."""
    gpu, C = pr.gpu, pr.C
    o = dict(g=Guarded(sentinel(HID * FEAT, F32), gpu), wt=Guarded(pr.wt, gpu),
             gwf2=Guarded(sentinel(1280, F32), gpu), gbf2=Guarded(sentinel(10, F32), gpu),
             gbf1=Guarded(sentinel(HID, F32), gpu))
    dpool = sentinel((pr.ldt + 1) * FEAT, BF).to(gpu)
    metrics = torch.tensor(M0, dtype=torch.float64, device=gpu)
    C.fc1_bwd(pr.dev["dh"], pr.dev["dht"], pr.ldt, pr.dev["pool"], o["wt"].view, pr.B, o["g"].view,
              dpool, pr.dev["slab"], o["gwf2"].view, o["gbf2"].view, o["gbf1"].view, metrics)
    torch.cuda.synchronize()
    out = {k: v.read() for k, v in o.items()}
    out.update(dpool=dpool.cpu(), metrics=metrics.cpu())
    return out


@pytest.mark.parametrize("B", [1, 33, 160])
def test_fc1_bwd_dx_and_head_slabs(gpu, B):
    """B = 1 / 33: one ragged 32-row tile (ldt 32 / 64); B = 160: five dX row tiles beside two
    128-row dW chunks."""
    pr = Fc1Bwd(gpu, B, seed=300 + B)
    dh, w1 = pr.dh[:B], pr.p0.view(HID, FEAT).to(BF)
    d64, w64 = dh.double(), w1.double()
    tag = f"fc1_bwd B={B}"
    bounds = interval(f"{tag} dpool", d64 @ w64, d64.abs() @ w64.abs(), dh.float() @ w1.float(), HID)
    a = run_fc1_bwd(pr)
    b = run_fc1_bwd(pr)
    dpool = a["dpool"]
    assert same_bits(dpool[B * FEAT:], sentinel((pr.ldt + 1 - B) * FEAT, BF)), "dpool rows >= B written"
    inside(f"{tag} dpool", dpool[:B * FEAT].view(B, FEAT), bounds)
    # head-slab reduction
    hb = pr.head_slab.shape[0]
    assert hb == pr.C.cnn_head_nblk(pr.ldt)
    h64 = pr.head_slab.double()
    ref, s, emu = h64.sum(0), h64.abs().sum(0), head_sum(pr.head_slab)
    for name, c0, n in (("gwf2", 0, 1280), ("gbf2", 1280, 10), ("gbf1", 1290, HID)):
        elementwise(f"{tag} {name}", a[name], ref[c0:c0 + n], s[c0:c0 + n], emu[c0:c0 + n], hb, False)
        assert same_bits(a[name], emu[c0:c0 + n]), f"{name} != the documented summation order"
    for k in ("dpool", "gwf2", "gbf2", "gbf1", "g"):
        assert same_bits(a[k], b[k]), f"{k} differs between two launches"
    m = a["metrics"]
    assert torch.equal(m, b["metrics"])
    tol = (hb + 4) * 2.0 ** -52
    assert abs(m[0] - M0[0] - ref[1418]) <= tol * (s[1418] + M0[0])
    assert abs(m[1] - M0[1] - ref[1419]) <= tol * (s[1419] + M0[1])
    assert m[2] == M0[2] + B


# ---------------------------------------------------------------- 4. cnn_bwd, cnn_bwd_band
# (B, ipb, bands, kind, seam)
CONV_BWD = ([(B, ipb, bands, "grid" if bands == 1 else "general", False)
             for (B, ipb, bands) in ((1, 1, 1), (3, 1, 1), (5, 2, 1), (7, 3, 1), (3, 1, 2), (2, 1, 3),
                                     (2, 1, 6), (1, 1, 6))]
            + [(2, 1, 3, "grid", False)]
            + [(2, 1, bands, "general", True) for bands in (2, 3, 6)])


def conv_bwd_inputs(B, kind, seam):
    g = torch.Generator().manual_seed(70 + B + (1000 if seam else 0) + (500 if kind == "grid" else 0))
    if kind == "grid":
        xg = grid_pixels(g, (B, 784))
        w1, b1 = grid_conv1(g)
        a1 = grid_a1(xg, w1, b1).permute(0, 2, 3, 1).reshape(B, P1, C1).contiguous()
        xn = bf(normalize_reference(xg))
    else:
        xg = w1 = b1 = None
        a1 = bf(torch.relu(torch.randn(B, P1, C1, generator=g)))     # about half exact zeros
        xn = bf(torch.randn(B, 784, generator=g))
    dpool = bf(torch.randn(B, FEAT, generator=g))
    sidx = torch.randint(0, 4, (B, FEAT), generator=g)
    pos = torch.rand(B, FEAT, generator=g) < 0.7
    pmask = torch.where(pos, 0x80 | (1 << sidx), 0).to(torch.uint8)   # cnn_fwd's encoding
    w2 = bf(torch.randn(C2, 9, C1, generator=g) * (2.0 / 288) ** 0.5)
    if seam:
        prow, arow = seam_rows()
        keep = torch.zeros(12, dtype=torch.bool)
        keep[prow] = True
        dpool = (dpool.view(B, 12, 12, C2) * keep.view(1, 12, 1, 1)).reshape(B, FEAT).contiguous()
        keep = torch.zeros(26, dtype=torch.bool)
        keep[arow] = True
        a1 = (a1.view(B, 26, 26, C1) * keep.view(1, 26, 1, 1)).reshape(B, P1, C1).contiguous()
    return xg, w1, b1, a1, xn, dpool, pmask, w2


def allowed(got, ref, allow):
    """got moved towards ref by the allowance: what is left is judged by the fp32 measure."""
    d = got.double() - ref
    return ref + d.sign() * (d.abs() - allow).clamp_min(0.0)


@pytest.mark.parametrize("B,ipb,bands,kind,seam", CONV_BWD)
def test_cnn_bwd_slabs(gpu, B, ipb, bands, kind, seam):
    """cnn_bwd (bands 1: slab g = images [g ipb, (g + 1) ipb); ipb = 1 is the path where the
    wgrad waves take the last dgrad pass) and cnn_bwd_band (slab (image, band): dW2 / db2 of the
    band's own dz2 rows; an image's slabs together: its dW1 / db1), every slab before any
    reduction."""
    C = _C()
    xg, w1, b1, a1, xn, dpool, pmask, w2 = conv_bwd_inputs(B, kind, seam)
    nblk = C.cnn_bwd_nblk(B, ipb, bands)
    assert nblk == (B * bands if bands > 1 else -(-B // ipb))
    SL = C.CNN_CONV_SLAB
    tag = f"cnn_bwd {kind} B={B} ipb={ipb} bands={bands}" + (" seam" if seam else "")

    # ---- reference
    dp = dpool.view(B, 12, 12, C2)
    mk = pmask.view(B, 12, 12, C2).long()
    dz2 = torch.zeros(B, 24, 24, C2)
    for sidx in range(4):
        dz2[:, (sidx >> 1)::2, (sidx & 1)::2, :] = dp * (mk == (0x80 | (1 << sidx)))
    a1n = a1.view(B, 26, 26, C1).permute(0, 3, 1, 2).contiguous()
    dzn = dz2.permute(0, 3, 1, 2).contiguous()
    W = nchw_w2(w2.reshape(-1))
    x = xn.view(B, 1, 28, 28)
    act = (a1n > 0).double()
    shp_w, shp_a = (C2, C1, 3, 3), (B, C1, 26, 26)
    # conv1 gradients: da1 in fp64, the bf16 operand and its rounding ambiguity (docstring)
    da1 = conv2d_input(shp_a, W.double(), dzn.double())
    s_da1 = conv2d_input(shp_a, W.double().abs(), dzn.double().abs())
    e_da1 = e_of(conv2d_input(shp_a, W, dzn), da1, s_da1)
    t = min(MARGIN * max(e_da1, U24), 576 * U24) * s_da1
    dz1 = bf16_of(da1).double() * act
    amb = (bf16_of(da1 + t).double() - bf16_of(da1 - t).double()).abs() * act
    print(f"bf16k {tag}: da1 e_ref {e_da1:.2e}, dz1 lo != hi for {(amb != 0).double().mean().item():.2%}")
    assert (amb != 0).double().mean().item() <= MAX_AMBIGUOUS

    def cotapci(t):      # [co][ci][ky][kx] -> the slab's [co][tap][ci]
        return t.permute(0, 2, 3, 1).reshape(C2, 9, C1)

    def conv2_part(sel, rows):
        """dW2 / db2 of images sel, dz2 rows [rows): ref, s, emu of each."""
        z = torch.zeros_like(dzn[sel])
        z[:, :, rows[0]:rows[1]] = dzn[sel][:, :, rows[0]:rows[1]]
        a, shp = a1n[sel], (C2, C1, 3, 3)
        return ((cotapci(conv2d_weight(a.double(), shp, z.double())),
                 cotapci(conv2d_weight(a.double(), shp, z.double().abs())),
                 cotapci(conv2d_weight(a, shp, z))),
                (z.double().sum((0, 2, 3)), z.double().abs().sum((0, 2, 3)), z.sum((0, 2, 3))))

    def conv1_part(sel):
        """dW1 / db1 of images sel: (ref, s, emu, allowance) of each."""
        xx, zz, dd = x[sel].double(), dz1[sel], amb[sel]
        shp = (C1, 1, 3, 3)
        return ((conv2d_weight(xx, shp, zz).reshape(C1, 9), conv2d_weight(xx.abs(), shp, zz.abs()).reshape(C1, 9),
                 conv2d_weight(x[sel], shp, zz.float()).reshape(C1, 9),
                 conv2d_weight(xx.abs(), shp, dd).reshape(C1, 9)),
                (zz.sum((0, 2, 3)), zz.abs().sum((0, 2, 3)), zz.float().sum((0, 2, 3)), dd.sum((0, 2, 3))))

    # ---- launch
    slab = nan_f32((nblk + 1) * SL, gpu)
    w2t = w2.to(BF).reshape(C2, 288).t().contiguous()                  # [tap * 32 + ci][co]
    if bands > 1:
        z8 = torch.zeros(B, 784, dtype=torch.uint8, device=gpu)
        zw, zb = torch.zeros(288, device=gpu), torch.zeros(32, device=gpu)
        C.cnn_bwd(z8, zw, zb, dpool.to(BF).to(gpu), pmask.to(gpu), w2t.to(gpu), B, ipb, slab, None,
                  bands, a1_swizzled(a1.to(BF)).to(gpu), xn.to(BF).reshape(-1).to(gpu))
    else:
        C.cnn_bwd(xg.to(gpu), w1.reshape(-1).to(gpu), b1.to(gpu), dpool.to(BF).to(gpu), pmask.to(gpu),
                  w2t.to(gpu), B, ipb, slab)
    torch.cuda.synchronize()
    sl = written(slab.cpu(), nblk * SL, "conv slab").view(nblk, SL).double()
    DB2, DW1, DB1 = C.CNN_CONV_SLAB_DB2, C.CNN_CONV_SLAB_DW1, C.CNN_CONV_SLAB_DB1

    def conv1_check(name, got, sel):
        (rw, sw, ew, aw), (rb, sb, eb, ab) = conv1_part(sel)
        n = len(sel)
        print(f"bf16k {tag} {name}: the dz1 ambiguity is on average "
              f"{(aw / (aw + MARGIN * U24 * sw).clamp_min(1e-300)).mean().item():.0%} of gw1's allowance "
              f"(allowance / s <= {(aw / sw.clamp_min(1e-300)).max().item():.1e}); before it, "
              f"|got - ref| / s <= {e_of(got[DW1:DB1].view(C1, 9), rw, sw):.2e}")
        elementwise(f"{tag} {name} gw1", allowed(got[DW1:DB1].view(C1, 9), rw, aw), rw, sw, ew, P1 * n, False)
        elementwise(f"{tag} {name} gb1", allowed(got[DB1:], rb, ab), rb, sb, eb, P1 * n, False, floor=U24)

    if bands == 1:
        for gi in range(nblk):
            sel = list(range(gi * ipb, min(B, (gi + 1) * ipb)))
            (rw, sw, ew), (rb, sb, eb) = conv2_part(sel, (0, 24))
            elementwise(f"{tag} slab{gi} gw2", sl[gi, :DB2].view(C2, 9, C1), rw, sw, ew, 576 * len(sel), False)
            elementwise(f"{tag} slab{gi} gb2", sl[gi, DB2:DW1], rb, sb, eb, 144 * len(sel), False, floor=U24)
            conv1_check(f"slab{gi}", sl[gi], sel)
    else:
        R = 24 // bands
        for img in range(B):
            for band in range(bands):
                gi = img * bands + band
                (rw, sw, ew), (rb, sb, eb) = conv2_part([img], (band * R, band * R + R))
                elementwise(f"{tag} slab{gi} gw2", sl[gi, :DB2].view(C2, 9, C1), rw, sw, ew, 24 * R, False)
                elementwise(f"{tag} slab{gi} gb2", sl[gi, DB2:DW1], rb, sb, eb, 6 * R, False, floor=U24)
            conv1_check(f"img{img}", sl[img * bands:(img + 1) * bands].sum(0), [img])


@pytest.mark.parametrize("nblk", [1, 2, 7, 300])
def test_conv_reduce(gpu, nblk):
    """conv_reduce on random slabs: per element against the fp64 column sum (K = nblk), bit-equal
    to its documented order (group rg adds slabs rg, rg + 16, ... from 0, the 16 group sums are
    added in order from 0: test_gpu_optim.slab_sum) and between two launches; guards survive."""
    C = _C()
    SL = C.CNN_CONV_SLAB
    slab = torch.randn(nblk, SL, generator=torch.Generator().manual_seed(nblk))
    dev = torch.cat((slab.reshape(-1), torch.full((SL,), float("nan")))).to(gpu)   # never read
    sizes = (C2 * 288, C2, 288, C1)
    runs = []
    for _ in range(2):
        outs = [Guarded(sentinel(n, F32), gpu) for n in sizes]
        C.conv_reduce(dev, nblk, *(o.view for o in outs))
        torch.cuda.synchronize()
        runs.append(torch.cat([o.read() for o in outs]))
    got = runs[0]
    assert same_bits(got, runs[1]), "conv_reduce differs between two launches"
    s64 = slab.double()
    emu = slab_sum(slab, 0, SL)
    elementwise(f"conv_reduce nblk={nblk}", got, s64.sum(0), s64.abs().sum(0), emu, nblk, False)
    assert same_bits(got, emu), "conv_reduce != the documented summation order"
