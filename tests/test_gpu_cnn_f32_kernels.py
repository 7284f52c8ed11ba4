"""The fp32 program's kernels (csrc/kernels/cnn_f32x3.hip, cnn_f32_exact.hip) called one by one on synthetic tensors,
every output element by element against an fp64 reference computed on the CPU from the very
operands the kernel read, in both product modes (x3 = split-bf16 on the bf16 MFMA, exact = the
fp32 MFMA):

    f32_fwd      row / data-step counter mode, training and evaluation templates
    f32_fc1_fwd  every split on its own
    f32_fc1_bwd  dW1, dX and the head-slab reduction
    f32_conv_bwd (+ conv_reduce) at full / partial image groups and (image, band) unit runs

Every output buffer is pre-filled with a sentinel (NaN, or 0x55 bytes) and allocated larger than
the kernel's contract: inside the contract every element must be written and finite, outside it
the sentinel must survive.

Measure.  For an output y = sum_k a_k b_k the reference also forms s = sum_k |a_k| |b_k|, and
e = max |got - ref| / s over all elements (elements with s == 0 must be exactly 0).  The same
arithmetic is emulated in fp32 torch on the CPU (x3: hi.lo + lo.hi + hi.hi of the split
operands, small terms first) and gives e_ref; the kernel must satisfy

    e_kernel <= 8 e_ref                          (another, legitimate, summation tree)
                                                 (32 for the exact f32_fc1_fwd: MARGIN_FC1_FWD_EXACT)
    e_kernel <= K 2^-24 (+ 2^-15 in x3 mode)     (K roundings of a term; 2^-15 per split product)

K is the number of summed terms of an element; for the conv1 gradients, a sum (over B 676 pixels)
of dgrad values that are sums (over 576 (co, tap) terms) themselves, it is the depth of the nested
sum, 576 + 676 B: the roundings one term passes through.

Max-pool ties.  pmask is compared with the fp64 argmax only in windows whose two largest fp64
values differ by more than DELTA = 1e-4, its sign only where |pooled| >= DELTA; the share of
windows left out this way is asserted to be <= 1 % from the reference alone.  The constant images
(all 0, all 255) and the ring image make windows in which several positions see bit-identical
3x3x32 a1 patches: their conv2 values are the same arithmetic on the same numbers, so they tie
exactly in the kernel, which must take the first of them ("first position holding the max").
There the expected bit is the first copy of the fp64 maximum and the lead is measured over the
positions that are not copies; such windows are checked exactly and do not count as left out.

Seam probe.  Inputs confined to the rows next to a 4-row band seam: pooled rows 2k - 1 and 2k
(k = 1 .. 5), 0 and 11; a1 rows 0, 1, 24, 25 and 4k - 2 .. 4k + 1.  With 4-row bands that is
every pooled row and every a1 row but 22 and 23: each term crosses a band halo.

Measured on MI355X, e_kernel | e_ref, each the largest over the shapes of its test, and the
largest ratio e_kernel / e_ref of any one shape (the bound is 8):

    kernel        output   exact                     x3
    f32_fwd       a1       1.7e-07|2.2e-07   0.9     7.5e-06|7.5e-06   1.0
    f32_fwd       pool     1.6e-07|1.2e-07   1.4     1.3e-06|1.3e-06   1.0
    f32_fc1_fwd   part     2.9e-07|2.8e-07   9.3 *   2.2e-06|2.2e-06   1.1
    f32_fc1_bwd   gwf1     3.3e-07|3.3e-07   1.0     1.5e-05|1.5e-05   1.0
    f32_fc1_bwd   dpool    3.9e-07|3.9e-07   1.0     2.1e-06|2.1e-06   1.0
    f32_conv_bwd  gw2      9.7e-08|1.6e-07   1.0     3.5e-06|3.5e-06   1.0
    f32_conv_bwd  gb2      2.2e-08|3.5e-08   1.3     5.3e-08|3.5e-08   2.9
    f32_conv_bwd  gw1      7.4e-09|8.5e-09   0.9     1.1e-07|1.1e-07   1.1
    f32_conv_bwd  gb1      4.0e-09|1.9e-09   2.3     9.4e-08|9.3e-08   1.1

* the exact f32_fc1_fwd at S = 1 (B = 40): 1.75e-07 against 1.89e-08; see MARGIN_FC1_FWD_EXACT.
xng, ylab, w2x and the a1 / W2^T layouts were bit-identical, the evaluation template's pool and
ylab bit-identical to the training template's, in every case.  Windows left out of the pmask
comparison (within DELTA): 3.6e-05 .. 3.3e-04 of all windows, against the cap of 1e-2; 30 .. 53 of
the 21632 B a1 values were bf16 half-way cases.  (The e_ref column depends on the host's BLAS.)
"""
import functools

import pytest
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from pytorch_distributed_mnist_amd.data.mnist import normalize_reference
from pytorch_distributed_mnist_amd.runtime.cnn_f32_step import conv_ipb
from pytorch_distributed_mnist_amd.runtime.structure import StepStructure

pytestmark = pytest.mark.gpu

D = torch.float64
FEAT, HID, P1, C1, C2 = 9216, 128, 676, 32, 64
U24, X3_PRODUCT = 2.0 ** -24, 2.0 ** -15     # fp32 rounding; split-bf16 product (above split8)
MARGIN = 8.0
# The exact f32_fc1_fwd alone: one fp32 accumulator chain over all 9216 / S features of a split
# (2304 MFMA steps at S = 1), where the host BLAS blocks K and sums short chains.  Its error is
# the same 1.6e-7 .. 2.9e-7 at every S while fp32 torch's falls to 1.9e-8 at S = 1: measured
# 9.3 x (S = 1), 7.2 x (S = 2), 4.5 x (S = 4), <= 3.1 x from S = 16 on.  32 = the largest measured
# ratio with a margin of 3.4; the K 2^-24 cap holds unchanged.
MARGIN_FC1_FWD_EXACT = 32.0
DELTA = 1e-4
I55 = 0x55555555
M0 = (5.0, 3.0, 11.0)                        # metrics pre-set


def _C():
    from pytorch_distributed_mnist_amd.ops import _ext
    return _ext.require()


# ---------------------------------------------------------------- helpers
def _split(t):
    """tests/test_split_bf16.py: hi = bf16(t), lo = bf16(t - hi), both as fp32."""
    hi = t.to(torch.bfloat16).to(torch.float32)
    lo = (t - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _bits16(t):
    """fp32 values that are exact bf16 -> their 16 bits."""
    return t.to(torch.bfloat16).view(torch.int16)


def _a1_swizzle(pl):
    """[..., 26 x, 4 chunks, 8] <-> the same with the 16-B chunk c of pixel (y, x) at
    c ^ (x & 3); an involution."""
    x = torch.arange(26).view(26, 1, 1)
    p = torch.arange(4).view(1, 4, 1)
    return pl.gather(pl.dim() - 2, (p ^ (x & 3)).expand(pl.shape)).contiguous()


def a1_layout(hi, lo):
    """hi / lo fp32 [B][676][32] (exact bf16 values) -> int16 [B][hi | lo][26][26][4][8]."""
    B = hi.shape[0]
    return _a1_swizzle(_bits16(torch.stack((hi, lo), 1)).view(B, 2, 26, 26, 4, 8))


def a1_planes(a1):
    """fp32 [B][676][32] -> the split-bf16 hand-off as int16 [B][hi | lo][26][26][4][8]."""
    return a1_layout(*_split(a1))


def a1_unplanes(raw):
    """Inverse of a1_planes: int16 [B][2][26][26][4][8] -> (hi, lo) fp32 [B][676][32]."""
    B = raw.shape[0]
    v = _a1_swizzle(raw.view(B, 2, 26, 26, 4, 8)).view(torch.bfloat16).float().view(B, 2, P1, C1)
    return v[:, 0], v[:, 1]


def w2t_planes(w2):
    """fp32 [co][tap][ci] -> the W2^T hand-off as int16 [hi | lo][tap][ci][8 chunks][8 co],
    chunk c (co 8 c .. 8 c + 7) at c ^ (ci & 7)."""
    hi, lo = _split(w2.view(C2, 9, C1))
    t = _bits16(torch.stack((hi, lo)).permute(0, 2, 3, 1).contiguous()).view(2, 9, C1, 8, 8)
    ci = torch.arange(C1).view(C1, 1, 1)
    p = torch.arange(8).view(1, 8, 1)
    return t.gather(3, (p ^ (ci & 7)).expand(t.shape)).contiguous()


def as_f32(i16):
    return i16.reshape(-1).view(torch.float32)


def nan_f32(n, dev):
    return torch.full((n,), float("nan"), dtype=torch.float32, device=dev)


def i55_f32(n, dev):
    return torch.full((n,), I55, dtype=torch.int32, device=dev).view(torch.float32)


def written(buf, n, name):
    """buf (CPU fp32, NaN-filled before the launch): [0, n) finite, the rest still NaN."""
    assert torch.isfinite(buf[:n]).all(), f"{name}: unwritten or non-finite inside the contract"
    assert buf.numel() > n and torch.isnan(buf[n:]).all(), f"{name}: written past the contract"
    return buf[:n]


def elementwise(tag, got, ref, s, emu, K, x3, margin=MARGIN, floor=0.0):
    """The module docstring's check of one output.  floor: the least e_ref the comparison
    uses (tests/test_gpu_cnn_bf16_kernels.py: sums of bare bf16 values)."""
    got, emu = got.double(), emu.double()
    assert got.shape == ref.shape == s.shape == emu.shape, tag
    zero = s == 0
    assert (ref[zero] == 0).all() and (got[zero] == 0).all(), f"{tag}: s == 0 but not 0"
    cap = K * U24 + (X3_PRODUCT if x3 else 0.0)
    if zero.all():
        print(f"f32k {tag}: all elements exactly 0")
        return
    nz = ~zero
    e_k = ((got - ref).abs()[nz] / s[nz]).max().item()
    e_r = ((emu - ref).abs()[nz] / s[nz]).max().item()
    print(f"f32k {tag}: e_kernel {e_k:.2e} e_ref {e_r:.2e} cap {cap:.2e}")
    assert e_k <= cap, (tag, e_k, cap)
    assert e_k <= margin * max(e_r, floor), (tag, e_k, e_r)


def nchw_w2(w2):
    """[co][tap][ci] -> [co][ci][ky][kx]."""
    return w2.view(C2, 3, 3, C1).permute(0, 3, 1, 2).contiguous()


def windows(z):
    """[B, C, 24, 24] -> [B, C, 12, 12, 4], window position s = 2 dy + dx."""
    B = z.shape[0]
    return z.view(B, -1, 12, 2, 12, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, -1, 12, 12, 4)


def nhwc(t):
    """[B, 64, 12, 12] -> the kernels' [B][pp][co]."""
    return t.permute(0, 2, 3, 1).reshape(t.shape[0], FEAT)


def window_ties(a1n, z2):
    """The module docstring's max-pool tie rule.  a1n [B, 32, 26, 26]: the a1 conv2 read; z2
    [B, 64, 24, 24]: its fp64 conv2.  Returns, per window [B, 64, 12, 12]: the fp64 maximum, its
    lead over the positions that are not copies of it, the expected argmax position (the first
    copy of the maximum) and whether the maximum has copies."""
    B = a1n.shape[0]
    win = windows(z2)
    m64, arg64 = win.max(-1)
    # window positions whose 3x3x32 a1 patches are bit-identical hold the same conv2 value in
    # the kernel (the same arithmetic on the same numbers): the first of them stands for all
    patches = windows(F.unfold(a1n, 3).view(B, 288, 24, 24))
    eq = (patches.unsqueeze(-1) == patches.unsqueeze(-2)).all(1)        # [B, 12, 12, 4 i, 4 j]
    pos4 = torch.arange(4).view(4, 1)
    first = torch.where(eq, pos4, 4).min(-2).values                     # [B, 12, 12, 4 j]
    eq_c = eq.unsqueeze(1).expand(B, C2, 12, 12, 4, 4)
    like = eq_c.gather(4, arg64[..., None, None].expand(B, C2, 12, 12, 1, 4)).squeeze(4)
    want = first.unsqueeze(1).expand(B, C2, 12, 12, 4).gather(4, arg64.unsqueeze(-1)).squeeze(-1)
    # the fp64 maximum's lead over the positions that are not copies of it
    gap = m64 - win.masked_fill(like, float("-inf")).max(-1).values
    return m64, gap, want, like.sum(-1) > 1


def check_pmask(pmask, pool, m_k, gap_k, want_k):
    """pmask [B, 9216] against window_ties' maximum, lead and expected position (all in the
    kernels' [B][pp][co] order) and against the pooled values of the same launch."""
    mk = pmask.long()
    low = mk & 0x7f
    ok = (mk == 0) | (((mk & 0x80) != 0) & (low != 0) & (low < 16) & ((low & (low - 1)) == 0))
    assert ok.all(), mk[~ok][:8].tolist()
    assert (mk[m_k <= -DELTA] == 0).all()
    assert (mk[m_k >= DELTA] != 0).all()
    assert ((mk != 0) == (pool > 0)).all()                              # mask and pool agree
    sel = (mk != 0) & (gap_k > DELTA)
    bad = sel & (low != (1 << want_k))
    assert not bad.any(), ("argmax bit", int(bad.sum()), low[bad][:8].tolist(), want_k[bad][:8].tolist())


# ---------------------------------------------------------------- 1. f32_fwd
BFULL, SPE, NROW = 4, 3, 22
FWD_CASES = [("row", 1, 0), ("row", 3, 0), ("row", 3, 3), ("ctr", 3, 5), ("ctr", 3, 7)]


def step_row(bfull, spe, nrow, c, img):
    """csrc/kernels.h step_row."""
    if spe <= 0:
        return c * bfull + img
    e = c // spe
    return (e & 1) * (nrow >> 1) + (c - e * spe) * bfull + img


def test_step_row_geometry():
    """A 22-row buffer of two 11-row epoch halves, 3 steps of 4 / 4 / 3 rows: counter 5 is the
    partial last step of the second half, counter 7 is back in the first."""
    assert [step_row(BFULL, SPE, NROW, 5, i) for i in range(3)] == [19, 20, 21]
    assert [step_row(BFULL, SPE, NROW, 7, i) for i in range(3)] == [4, 5, 6]
    assert [step_row(BFULL, 0, NROW, 2, i) for i in range(2)] == [8, 9]


@functools.lru_cache(maxsize=None)
def fwd_inputs():
    g = torch.Generator().manual_seed(1234)
    images = torch.randint(0, 256, (NROW, 784), generator=g, dtype=torch.uint8)
    ring = torch.zeros(28, 28, dtype=torch.uint8)
    ring[0], ring[27], ring[:, 0], ring[:, 27] = 200, 255, 31, 129
    for r, v in ((1, 0), (21, 0), (3, 255), (5, 255)):
        images[r] = v
    images[2] = ring.view(-1)
    images[20] = ring.view(-1)
    labels = torch.randint(0, 10, (NROW,), generator=g, dtype=torch.int32)
    w1 = torch.randn(C1, 9, generator=g) * (2.0 / 9) ** 0.5
    b1 = torch.randn(C1, generator=g) * 0.1
    w2 = torch.randn(C2, 9, C1, generator=g) * (2.0 / 288) ** 0.5
    # shifted down: a visible share of the pooled values is non-positive (pmask == 0 branch)
    b2 = torch.randn(C2, generator=g) * 0.5 - 1.5
    return images, labels, w1, b1, w2, b2


def launch_fwd(C, dev, mode, B, arg, x3, train):
    images, labels, w1, b1, w2, b2 = fwd_inputs()
    wh, wl = _split(w2)
    w2s = torch.cat((wh.reshape(-1), wl.reshape(-1))).to(torch.bfloat16).to(dev)
    pool = nan_f32((B + 1) * FEAT, dev)
    ylab = torch.full((B + 1,), I55, dtype=torch.int32, device=dev)
    pmask = a1g = xng = w2x = None
    if train:
        pmask = torch.full(((B + 1) * FEAT,), 0x55, dtype=torch.uint8, device=dev)
        a1g = (i55_f32 if x3 else nan_f32)((B + 1) * P1 * C1, dev)
        xng = nan_f32((B + 1) * 784, dev)
        w2x = i55_f32(2 * 9 * C1 * 128 // 4 + 64, dev)
    if mode == "row":
        im, lb, ctr, bfull, spe = images[arg:].to(dev), labels[arg:].to(dev), None, B, 0
    else:
        im, lb, bfull, spe = images.to(dev), labels.to(dev), BFULL, SPE
        ctr = torch.tensor([arg], dtype=torch.int64, device=dev)
    C.f32_fwd(im, lb, ctr, bfull, B, w1.reshape(-1).to(dev), b1.to(dev), w2.reshape(-1).to(dev),
              b2.to(dev), pool, pmask, a1g, xng, ylab, spe=spe, x3=x3, w2x=w2x, w2s=w2s)
    torch.cuda.synchronize()
    out = dict(pool=pool.cpu(), ylab=ylab.cpu())
    if ctr is not None:
        assert ctr.item() == arg                       # the forward does not advance it
    if train:
        out.update(pmask=pmask.cpu(), a1g=a1g.cpu(), xng=xng.cpu(), w2x=w2x.cpu())
    return out


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("mode,B,arg", FWD_CASES)
def test_f32_fwd(gpu, mode, B, arg, x3):
    """f32_fwd / f32x3_fwd, training and evaluation templates: ylab, xng, the a1 hand-off (and
    the layout helpers against it, bit for bit), w2x, pool, pmask.  The two templates differ
    only in what they store: pool and ylab are bit-identical."""
    C = _C()
    images, labels, w1, b1, w2, b2 = fwd_inputs()
    rows = ([arg + i for i in range(B)] if mode == "row"
            else [step_row(BFULL, SPE, NROW, arg, i) for i in range(B)])
    assert max(rows) < NROW
    tag = f"fwd {'x3' if x3 else 'exact'} {mode}{arg} B={B}"
    tr = launch_fwd(C, gpu, mode, B, arg, x3, True)
    ev = launch_fwd(C, gpu, mode, B, arg, x3, False)

    # ylab, xng
    assert tr["ylab"][:B].tolist() == labels[rows].tolist()
    assert (tr["ylab"][B:] == I55).all()
    xn = normalize_reference(images[rows])
    xng = written(tr["xng"], B * 784, "xng").view(B, 784)
    assert torch.equal(xng.view(torch.int32), xn.view(torch.int32)), \
        ("xng is not torchvision's arithmetic", (xng - xn).abs().max().item())

    # a1 hand-off
    x64 = xn.double().view(B, 1, 28, 28)
    w1n = w1.view(C1, 1, 3, 3)
    a1_ref = torch.relu(F.conv2d(x64, w1n.double(), b1.double()))
    s1 = F.conv2d(x64.abs(), w1n.double().abs(), b1.double().abs())
    a1_emu = torch.relu(F.conv2d(xn.view(B, 1, 28, 28), w1n, b1))
    if x3:
        raw = tr["a1g"].view(torch.int16)
        assert (raw[B * 2 * P1 * C1:] == 0x5555).all(), "a1 planes written past the contract"
        raw = raw[:B * 2 * P1 * C1].view(B, 2, 26, 26, 4, 8)
        hi, lo = a1_unplanes(raw)
        a1k = hi + lo                                                   # exact in fp32
        # a well-formed split: lo is the bf16 of what hi left, at most half an ulp of hi
        assert torch.equal(_bits16(a1k - hi), _bits16(lo)), "a1 lo plane is not bf16(a1 - hi)"
        assert (lo.abs() <= hi.abs() * 2.0 ** -8).all(), "a1 lo plane exceeds half an ulp of hi"
        # the layout helpers reproduce the kernel's bytes (conv_bwd's test rests on them).
        # hi + lo drops what lo's rounding left: where it lands exactly half-way between two
        # bf16 values (low 16 bits 0x8000) splitting it again may round hi the other way
        assert torch.equal(a1_layout(hi, lo), raw), "a1_layout != the forward's hand-off"
        tie = (a1k.view(torch.int32) & 0xffff) == 0x8000
        # lo keeps 8 bits of a remainder below half an ulp of hi: about 2^-9 of the values
        assert tie.double().mean().item() <= 2.0 ** -7
        print(f"f32k {tag}: {int(tie.sum())} of {tie.numel()} a1 values are bf16 half-way cases")
        zero = torch.zeros(())
        assert torch.equal(a1_planes(torch.where(tie, hi, a1k)),
                           a1_layout(hi, torch.where(tie, zero, lo))), \
            "a1_planes != the forward's hand-off"
        eh, el = _split(a1_emu)
        a1_emu = eh + el
        want = w2t_planes(w2).reshape(-1)
        got = tr["w2x"].view(torch.int16)
        assert torch.equal(got[:want.numel()], want), "w2x != w2t_planes(w2)"
        assert (got[want.numel():] == 0x5555).all(), "w2x written past the contract"
    else:
        a1k = written(tr["a1g"], B * P1 * C1, "a1g").view(B, P1, C1)
    assert (a1k >= 0).all()
    a1k_n = a1k.view(B, 26, 26, C1).permute(0, 3, 1, 2).contiguous()
    elementwise(f"{tag} a1", a1k_n, a1_ref, s1, a1_emu, 9, x3)

    # pool from the a1 the kernel handed off
    wh, wl = _split(w2)
    w2op = (wh + wl) if x3 else w2
    W64 = nchw_w2(w2op).double()
    a64 = a1k_n.double()
    z2 = F.conv2d(a64, W64, b2.double())
    s2 = F.conv2d(a64, W64.abs(), b2.double().abs())
    if x3:
        ah, al = _split(a1k_n)
        z2_emu = (F.conv2d(al, nchw_w2(wh), b2) + F.conv2d(ah, nchw_w2(wl))) + F.conv2d(ah, nchw_w2(wh))
    else:
        z2_emu = F.conv2d(a1k_n, nchw_w2(w2), b2)

    m64, gap, want, tied = window_ties(a1k_n, z2)
    # left out of the pmask comparison, from the reference alone
    near = (m64.abs() < DELTA) | (gap <= DELTA)
    share = near.double().mean().item()
    nonpos = (m64 <= -DELTA).double().mean().item()
    print(f"f32k {tag}: windows within delta {share:.2e}, pooled <= -delta {nonpos:.2f}, "
          f"windows whose maximum has identical copies {tied.double().mean().item():.2f}")
    assert share <= 0.01, share
    assert 0.05 <= nonpos <= 0.95, nonpos

    pool = written(tr["pool"], B * FEAT, "pool").view(B, FEAT)
    elementwise(f"{tag} pool", pool, nhwc(torch.relu(m64)), nhwc(windows(s2).max(-1).values),
                nhwc(torch.relu(windows(z2_emu).max(-1).values)), 288, x3)

    # pmask
    assert (tr["pmask"][B * FEAT:] == 0x55).all(), "pmask written past the contract"
    check_pmask(tr["pmask"][:B * FEAT].view(B, FEAT), pool, nhwc(m64), nhwc(gap), nhwc(want))

    # evaluation template
    assert torch.equal(ev["ylab"], tr["ylab"])
    assert torch.equal(written(ev["pool"], B * FEAT, "eval pool").view(torch.int32),
                       tr["pool"][:B * FEAT].view(torch.int32))


# ---------------------------------------------------------------- 2. f32_fc1_fwd
FC1_FWD = ([(B, S, x3) for x3 in (False, True)
            for (B, S) in ((1, 32), (33, 32), (31, 16), (64, 4), (40, 1), (5, 2))]
           + [(5, 288, False), (5, 96, True)])


@functools.lru_cache(maxsize=None)
def fc_w1():
    return torch.randn(HID, FEAT, generator=torch.Generator().manual_seed(77))


@pytest.mark.parametrize("B,S,x3", FC1_FWD)
def test_f32_fc1_fwd(gpu, B, S, x3):
    """Every split's partial on its own against fp64 of its contiguous 9216 / S features."""
    C = _C()
    g = torch.Generator().manual_seed(100 * B + S)
    pool = torch.randn(B, FEAT, generator=g)
    w1 = fc_w1()
    part = nan_f32((S + 1) * B * HID, gpu)
    C.f32_fc1_fwd(pool.reshape(-1).to(gpu), w1.reshape(-1).to(gpu), part, B, S, x3=x3)
    torch.cuda.synchronize()
    got = written(part.cpu(), S * B * HID, "part").view(S, B, HID)
    K = FEAT // S
    if x3:
        ph, pl = _split(pool)
        wh, wl = _split(w1)
        p_op, w_op = ph + pl, wh + wl
    else:
        p_op, w_op = pool, w1

    def mm(p, w):
        return torch.einsum("bsk,nsk->sbn", p.view(B, S, K), w.view(HID, S, K))

    ref = mm(p_op.double(), w_op.double())
    s = mm(p_op.double().abs(), w_op.double().abs())
    emu = (mm(pl, wh) + mm(ph, wl)) + mm(ph, wh) if x3 else mm(pool, w1)
    elementwise(f"fc1_fwd {'x3' if x3 else 'exact'} B={B} S={S}", got, ref, s, emu, K, x3,
                MARGIN if x3 else MARGIN_FC1_FWD_EXACT)


@pytest.mark.parametrize("S,x3", [(5, False), (5, True), (9, True)])
def test_f32_fc1_fwd_rejects_split(gpu, S, x3):
    """Splits that do not divide 288 (or, split-bf16, 96) are refused by the host, no launch."""
    C = _C()
    part = nan_f32(S * 2 * HID, gpu)
    with pytest.raises(RuntimeError):
        C.f32_fc1_fwd(torch.zeros(2 * FEAT, device=gpu), torch.zeros(HID * FEAT, device=gpu),
                      part, 2, S, x3=x3)
    torch.cuda.synchronize()
    assert torch.isnan(part).all()


# ---------------------------------------------------------------- 3. f32_fc1_bwd
def rel(a, b):
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.mark.parametrize("x3", [False, True])
@pytest.mark.parametrize("B", [1, 33, 40, 64])
def test_f32_fc1_bwd(gpu, B, x3):
    """dW1 (K = B), dX (K = 128; rows >= B untouched) and the head-slab reduction."""
    C = _C()
    g = torch.Generator().manual_seed(B)
    ldt = -(-B // 32) * 32
    dh = torch.zeros(ldt, HID)
    dh[:B] = torch.randn(B, HID, generator=g)          # cnn_head's contract: rows >= B are zero
    pool = torch.randn(B, FEAT, generator=g)
    w1 = fc_w1()
    hb = C.cnn_head_nblk(ldt)
    SLAB = C.CNN_HEAD_SLAB
    head_slab = torch.randn(hb, SLAB, generator=g)
    G = 256
    gwf1 = nan_f32(HID * FEAT + G, gpu)
    dpool = nan_f32((ldt + 1) * FEAT, gpu)
    gwf2, gbf2, gbf1 = nan_f32(1280 + G, gpu), nan_f32(10 + G, gpu), nan_f32(HID + G, gpu)
    metrics = torch.tensor(M0, dtype=torch.float64, device=gpu)
    C.f32_fc1_bwd(dh.reshape(-1).to(gpu), ldt, pool.reshape(-1).to(gpu), w1.reshape(-1).to(gpu), B,
                  gwf1[:HID * FEAT], dpool, head_slab.reshape(-1).to(gpu), gwf2[:1280], gbf2[:10],
                  gbf1[:HID], metrics, x3=x3)
    torch.cuda.synchronize()
    tag = f"fc1_bwd {'x3' if x3 else 'exact'} B={B}"
    if x3:
        dhh, dhl = _split(dh[:B])
        ph, pl = _split(pool)
        wh, wl = _split(w1)
        d_op, p_op, w_op = dhh + dhl, ph + pl, wh + wl
    else:
        d_op, p_op, w_op = dh[:B], pool, w1
    d64, p64, w64 = d_op.double(), p_op.double(), w_op.double()
    got = written(gwf1.cpu(), HID * FEAT, "gwf1").view(HID, FEAT)
    emu = (dhl.t() @ ph + dhh.t() @ pl) + dhh.t() @ ph if x3 else dh[:B].t() @ pool
    elementwise(f"{tag} gwf1", got, d64.t() @ p64, d64.abs().t() @ p64.abs(), emu, B, x3)
    got = written(dpool.cpu(), B * FEAT, "dpool").view(B, FEAT)
    emu = (dhl @ wh + dhh @ wl) + dhh @ wh if x3 else dh[:B] @ w1
    elementwise(f"{tag} dpool", got, d64 @ w64, d64.abs() @ w64.abs(), emu, HID, x3)
    # head-slab reduction: test_gpu_cnn_bwd_exact.py::test_fc1_bwd_exact's bounds
    hs = head_slab.double().sum(0)
    assert rel(written(gwf2.cpu(), 1280, "gwf2").double(), hs[:1280]) < 1e-6
    assert rel(written(gbf2.cpu(), 10, "gbf2").double(), hs[1280:1290]) < 1e-6
    assert rel(written(gbf1.cpu(), HID, "gbf1").double(), hs[1290:1418]) < 1e-6
    m = metrics.cpu()
    assert abs(m[0] - M0[0] - hs[1418]) < 1e-3 and abs(m[1] - M0[1] - hs[1419]) < 1e-3
    assert m[2] == M0[2] + B


# ---------------------------------------------------------------- 4. f32_conv_bwd + conv_reduce
CONV_BWD = ([(B, per, False) for (B, per) in ((1, 1), (3, 1), (5, 2), (7, 3))]
            + [(B, per, True) for (B, per) in ((1, 1), (1, 6), (3, 4), (5, 7), (2, 12), (3, 100))])


def seam_rows():
    """The seam probe's pooled rows and a1 rows (module docstring)."""
    prow = sorted({0, 11} | {2 * k - 1 for k in range(1, 6)} | {2 * k for k in range(1, 6)})
    arow = sorted({0, 1, 24, 25} | {4 * k + d for k in range(1, 6) for d in (-2, -1, 0, 1)})
    return prow, arow


def conv_bwd_inputs(B, seam):
    g = torch.Generator().manual_seed(50 + B + (1000 if seam else 0))
    a1 = torch.relu(torch.randn(B, P1, C1, generator=g))      # about half exact zeros
    xn = torch.randn(B, 784, generator=g)
    dpool = torch.randn(B, FEAT, generator=g)
    sidx = torch.randint(0, 4, (B, FEAT), generator=g)
    pos = torch.rand(B, FEAT, generator=g) < 0.7
    pmask = torch.where(pos, 0x80 | (1 << sidx), 0).to(torch.uint8)
    w2 = torch.randn(C2, 9, C1, generator=g) * (2.0 / 288) ** 0.5
    if seam:
        prow, arow = seam_rows()
        keep = torch.zeros(12, dtype=torch.bool)
        keep[prow] = True
        dpool = dpool.view(B, 12, 12, C2) * keep.view(1, 12, 1, 1)
        dpool = dpool.reshape(B, FEAT).contiguous()
        keep = torch.zeros(26, dtype=torch.bool)
        keep[arow] = True
        a1 = (a1.view(B, 26, 26, C1) * keep.view(1, 26, 1, 1)).reshape(B, P1, C1).contiguous()
    return a1, xn, dpool, pmask, w2


def conv_bwd_grads(a1n, x, dzn, W, x3, dt, emulate):
    """(gw2, gb2, gw1, gb1) of the conv backward from dz2.  dt = float64: the reference (and,
    with absolute operands, the magnitudes s); emulate: the kernels' arithmetic in fp32 torch
    (x3: every conv2 product from split operands, small terms first)."""
    B = a1n.shape[0]
    shp_w, shp_a = (C2, C1, 3, 3), (B, C1, 26, 26)
    if emulate and x3:
        ah, al = _split(a1n)
        zh, zl = _split(dzn)
        wh, wl = _split(W)
        gw2 = (conv2d_weight(ah, shp_w, zl) + conv2d_weight(al, shp_w, zh)) + conv2d_weight(ah, shp_w, zh)
        da1 = (conv2d_input(shp_a, wh, zl) + conv2d_input(shp_a, wl, zh)) + conv2d_input(shp_a, wh, zh)
    else:
        a1n, dzn, W = a1n.to(dt), dzn.to(dt), W.to(dt)
        gw2 = conv2d_weight(a1n, shp_w, dzn)
        da1 = conv2d_input(shp_a, W, dzn)
    return gw2, dzn.to(dt).sum((0, 2, 3)), da1


def check_conv_bwd(C, dev, B, per, x3, seam):
    a1, xn, dpool, pmask, w2 = conv_bwd_inputs(B, seam)
    nblk = C.f32_conv_bwd_nblk(B, per, x3)
    assert nblk == (-(-B * 6 // per) if x3 else -(-B // per) * 6)      # f32_conv_bwd_blocks
    SL = C.CNN_CONV_SLAB
    slab = nan_f32((nblk + 1) * SL, dev)
    if x3:
        a1g = as_f32(a1_planes(a1)).to(dev)
        w2x = as_f32(w2t_planes(w2)).to(dev)
    else:
        a1g, w2x = a1.reshape(-1).to(dev), None
    C.f32_conv_bwd(a1g, xn.reshape(-1).to(dev), dpool.reshape(-1).to(dev), pmask.reshape(-1).to(dev),
                   w2.reshape(-1).to(dev), B, slab, per, x3=x3, w2x=w2x)
    G = 256
    outs = [nan_f32(n + G, dev) for n in (C2 * 288, C2, 288, C1)]
    C.conv_reduce(slab, nblk, *(o[:o.numel() - G] for o in outs))
    torch.cuda.synchronize()
    slab_c = written(slab.cpu(), nblk * SL, "conv slab").view(nblk, SL)
    gw2, gb2, gw1, gb1 = (written(o.cpu(), o.numel() - G, "conv grad") for o in outs)
    # conv_reduce is the fixed-order sum of the slabs
    assert rel(torch.cat((gw2, gb2, gw1, gb1)).double(), slab_c.double().sum(0)) < 1e-6

    # operands as the kernel read them; dz2 is split inside the kernel
    if x3:
        a1_op, w2_op = sum(_split(a1)), sum(_split(w2))
    else:
        a1_op, w2_op = a1, w2
    dp = dpool.view(B, 12, 12, C2)
    mk = pmask.view(B, 12, 12, C2).long()
    dz2 = torch.zeros(B, 24, 24, C2)
    for sidx in range(4):
        dz2[:, (sidx >> 1)::2, (sidx & 1)::2, :] = dp * (mk == (0x80 | (1 << sidx)))
    a1n = a1_op.view(B, 26, 26, C1).permute(0, 3, 1, 2).contiguous()
    dzn = dz2.permute(0, 3, 1, 2).contiguous()
    W = nchw_w2(w2_op)
    x = xn.view(B, 1, 28, 28)
    act = a1n > 0

    def conv1_grads(da1, xx, dt):
        dz1 = da1 * act.to(dt)
        return conv2d_weight(xx.to(dt), (C1, 1, 3, 3), dz1).reshape(C1, 9), dz1.sum((0, 2, 3))

    r_gw2, r_gb2, r_da1 = conv_bwd_grads(a1n, x, dzn, W, x3, D, False)
    s_gw2, s_gb2, s_da1 = conv_bwd_grads(a1n.abs(), x, dzn.abs(), W.abs(), x3, D, False)
    e_gw2, e_gb2, e_da1 = conv_bwd_grads(a1n, x, dzn, W, x3, torch.float32, True)
    r_gw1, r_gb1 = conv1_grads(r_da1, x, D)
    s_gw1, s_gb1 = conv1_grads(s_da1, x.abs(), D)
    e_gw1, e_gb1 = conv1_grads(e_da1, x, torch.float32)
    tag = (f"conv_bwd {'x3' if x3 else 'exact'} B={B} {'upw' if x3 else 'ipb'}={per}"
           + (" seam" if seam else ""))

    def cotapci(t):      # [co][ci][ky][kx] -> the slab's [co][tap][ci]
        return t.permute(0, 2, 3, 1).reshape(C2, 9, C1)

    elementwise(f"{tag} gw2", gw2.view(C2, 9, C1), cotapci(r_gw2), cotapci(s_gw2), cotapci(e_gw2),
                B * 576, x3)
    elementwise(f"{tag} gb2", gb2, r_gb2, s_gb2, e_gb2, B * 144, x3)
    depth = 576 + B * P1
    elementwise(f"{tag} gw1", gw1.view(C1, 9), r_gw1, s_gw1, e_gw1, depth, x3)
    elementwise(f"{tag} gb1", gb1, r_gb1, s_gb1, e_gb1, depth, x3)


@pytest.mark.parametrize("B,per,x3", CONV_BWD)
def test_f32_conv_bwd(gpu, B, per, x3):
    """Exact: `per` images per workgroup (full and partial last groups).  x3: `per` (image,
    band) units per workgroup (one unit; one image; image changes mid-way; image and band
    changes with a partial last workgroup; two whole images; more than all units)."""
    check_conv_bwd(_C(), gpu, B, per, x3, False)


@pytest.mark.parametrize("x3", [False, True])
def test_f32_conv_bwd_seam_probe(gpu, x3):
    """B = 2 at the program's own work split, inputs confined to the rows next to the band
    seams (module docstring)."""
    check_conv_bwd(_C(), gpu, 2, conv_ipb(2, x3, StepStructure()), x3, True)
