"""The fc1-weight SGD update outside the optimizer kernel, against fp64.

The formula of ``optim_common.h update<OPT_SGD>`` runs in three kernels: ``optim_kernel``'s
transposed-shadow tile (tests/test_gpu_optim.py), ``fc1_bwd``'s dW epilogue (``fc_update``,
fc1_bwd.hip) and the extra workgroups of the forward launch (``fc_carry``, fc_carry.h).
test_gpu_comm.py shows them bit-identical to each other inside whole steps; here each is
pinned on its own to ``ref_update`` (test_gpu_optim.py: fp64 on the fp32 inputs the kernel
read, condition-scaled error, within 8 x ``FlatSGD.step_cpu`` and within R * 2^-23), its bf16
copies bit for bit to its own returned weights, and then the three to each other.

``fc1_bwd``'s stored gradient is compared element by element with the fp64 ``dh^T . pool`` of
its bf16 operands: e = max |g - ref| / sum_b |dh||pool|, within 8 x the same product in fp32
torch and within B * 2^-24 (B - 1 fp32 additions of exact bf16 x bf16 products).  The fused
update is then checked against ``ref_update`` of *that stored gradient* (the value the epilogue
holds in registers).

Measured on MI355X (max over the cases; "differ" = share of p elements not bit-equal to
``step_cpu``):

    path                    out  e(kernel)  e(cpu32)  ratio   R  e/(R 2^-23)  differ
    fc1_bwd fused update    p    2.07e-07   1.50e-07  1.72    7  0.33         22 % .. 43 %
                            m    1.18e-07   1.18e-07  1.40    4  0.32
    carried (cnn_fwd, band) p    1.71e-07   1.34e-07  1.47    7  0.27         8 % .. 11 %
                            m    1.17e-07   1.17e-07  1.07    4  0.32
    fc1_bwd stored dW       B = 1: exact (both);  B = 40: 1.00e-07 against 1.46e-07 in fp32
                            torch (cap 2.4e-06);  B = 160: 1.07e-07 against 1.45e-07 (cap 9.5e-06)

"differ" comes from ATen's CPU ``add(alpha=...)`` contracting to an FMA (test_gpu_optim.py); the
three kernels themselves are bit-identical to each other (test_one_formula_three_kernels).

Mutations tried on scratch builds (each fails tests of this file; "old" = the parent's suite):
h.first forced to 0 and the nesterov branch dropped (old: both pass), fcc_tpos swizzle
dropped on the read side (old: test_gpu_comm.py's whole-step comparisons fail), the fused
update reading fmv of the neighbouring nt (old: test_gpu_comm.py's world-size-1 carry fails).
"""
import math

import pytest
import torch

from pytorch_distributed_mnist_amd.runtime.cnn_step import frag_major, frag_major_t
from test_gpu_optim import (BF, F32, F64, Guarded, _C, err, launch, measure, same_bits, sentinel,
                            sgd)

pytestmark = pytest.mark.gpu

HID, FEAT = 128, 9216
N = HID * FEAT
HYPERS = {"mom_wd": sgd(lr=0.05, mom=0.9, wd=1e-4),
          "nesterov": sgd(lr=0.05, mom=0.9, nesterov=True, damp=0.1, gs=0.5)}


def _state(seed):
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(N, generator=gen) * 0.05, torch.randn(N, generator=gen) * 0.01)


def _update_tuple(C, gpu, h, step, p, g, m, sh, sht_next, store_grad=None):
    """As CnnStep._fc_update builds it: 17 entries, or 18 with store_grad."""
    lr = torch.tensor([h["lr"]], dtype=F64, device=gpu)
    st = torch.tensor([step], dtype=torch.int64, device=gpu)
    t = (C.OPT_SGD, p, g, m, None, sh, lr, st, 0.0, 0.0, 0.0, float(h["wd"]), float(h["mom"]),
         float(h["damp"]), bool(h["nesterov"]), float(h["gs"]), sht_next)
    return t if store_grad is None else t + (store_grad,)


class Fc1Bwd:
    """One fc1_bwd problem: inputs on the device, fresh poisoned outputs for every run."""

    def __init__(self, gpu, B, seed):
        self.C, self.gpu, self.B = _C(), gpu, B
        gen = torch.Generator().manual_seed(seed)
        self.ldt = ldt = -(-B // 32) * 32
        dh = torch.zeros(ldt, HID)
        dh[:B] = torch.randn(B, HID, generator=gen)
        self.dh = dh.to(BF)
        self.pool = torch.randn(B, FEAT, generator=gen).to(BF)
        self.p0, self.m0 = _state(seed + 1)
        self.wt = frag_major_t(self.p0.view(HID, FEAT).to(BF))       # the W1^T being read
        hb = self.C.cnn_head_nblk(ldt)
        self.head_slab = torch.randn(hb, self.C.CNN_HEAD_SLAB, generator=gen)
        self.dev = dict(dh=frag_major(self.dh).to(gpu), dht=frag_major(self.dh.t().contiguous()).to(gpu),
                        pool=self.pool.to(gpu), slab=self.head_slab.to(gpu))

    def run(self, h=None, step=1, store_grad=None, with_t=True):
        """h None: no fc_update.  Returns every output as CPU tensors (guards checked)."""
        gpu, C = self.gpu, self.C
        o = dict(p=Guarded(self.p0, gpu), m=Guarded(self.m0, gpu), g=Guarded(sentinel(N, F32), gpu),
                 sh=Guarded(sentinel(N, BF), gpu), sht=Guarded(sentinel(N, BF), gpu),
                 wt=Guarded(self.wt, gpu), dpool=Guarded(sentinel(self.B * FEAT, BF), gpu),
                 gwf2=Guarded(sentinel(1280, F32), gpu), gbf2=Guarded(sentinel(10, F32), gpu),
                 gbf1=Guarded(sentinel(HID, F32), gpu))
        metrics = torch.zeros(3, dtype=F64, device=gpu)
        fcu = None
        if h is not None:
            fcu = _update_tuple(C, gpu, h, step, o["p"].view, o["g"].view, o["m"].view, o["sh"].view,
                                o["sht"].view if with_t else None, store_grad)
            assert len(fcu) == (17 if store_grad is None else 18)
        C.fc1_bwd(self.dev["dh"], self.dev["dht"], self.ldt, self.dev["pool"], o["wt"].view, self.B,
                  o["g"].view, o["dpool"].view, self.dev["slab"], o["gwf2"].view, o["gbf2"].view,
                  o["gbf1"].view, metrics, fcu)
        torch.cuda.synchronize()
        out = {k: v.read() for k, v in o.items()}
        out["metrics"] = metrics.cpu()
        assert same_bits(out["wt"], self.wt), "the W1^T being read was written"
        return out


def check_copies(out, with_t=True):
    pb = out["p"].view(HID, FEAT).to(BF)
    assert same_bits(out["sh"], frag_major(pb)), "shadow != frag_major(bf16(p))"
    if with_t:
        assert same_bits(out["sht"], frag_major_t(pb)), "shadow_t_next != frag_major_t(bf16(p))"
    else:
        assert same_bits(out["sht"], sentinel(N, BF))


@pytest.mark.parametrize("hname", list(HYPERS))
@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("B", [1, 40, 160])
def test_fc1_bwd_fused_update(gpu, B, step, hname):
    """B = 1 / 40: one ragged 32-row block (ldt 32 / 64); B = 160: two 128-row chunks."""
    h = HYPERS[hname]
    pr = Fc1Bwd(gpu, B, seed=B)
    a = pr.run(h, step, store_grad=True)
    # the stored gradient against fp64 of the bf16 operands
    dh, pool = pr.dh[:B], pr.pool
    ref = dh.to(F64).t() @ pool.to(F64)
    scale = dh.to(F64).abs().t() @ pool.to(F64).abs()
    ek = err(a["g"].view(HID, FEAT), ref, scale)
    ec = err(dh.to(F32).t() @ pool.to(F32), ref, scale)
    print(f"DW B={B}: e(kernel)={ek:.3e} e(torch32)={ec:.3e} cap={B * 2.0 ** -24:.3e}")
    assert ek <= 8 * ec, (ek, ec)
    assert ek <= B * 2.0 ** -24, ek                  # B - 1 additions of exact products
    # the update of that gradient; R (test_gpu_optim.roundings): p 6 / 8, m 2 / 4 on a later
    # step (mom_wd / nesterov), the first step 2 less
    measure(f"fused-{hname}/B{B}", "sgd", h, step, pr.p0, a["g"], pr.m0, None,
            {"p": a["p"], "m": a["m"]})
    check_copies(a)
    # store_grad off: the same update, the gradient buffer untouched
    b = pr.run(h, step, store_grad=False)
    for k in ("p", "m", "sh", "sht", "dpool", "gwf2", "gbf2", "gbf1", "metrics"):
        assert same_bits(a[k], b[k]) if k != "metrics" else torch.equal(a[k], b[k]), k
    assert same_bits(b["g"], sentinel(N, F32)), "store_grad=False wrote the gradient"
    # 17 entries without a W1^T copy to write
    c = pr.run(h, step, with_t=False)
    for k in ("p", "m", "sh", "g"):
        assert same_bits(a[k], c[k]), k
    check_copies(c, with_t=False)
    # without fc_update: dX, the head-slab sums and the gradient do not change
    d = pr.run(None)
    for k in ("dpool", "gwf2", "gbf2", "gbf1", "g"):
        assert same_bits(a[k], d[k]), k
    assert torch.equal(a["metrics"], d["metrics"])
    assert same_bits(d["p"], pr.p0) and same_bits(d["m"], pr.m0)
    assert same_bits(d["sh"], sentinel(N, BF)) and same_bits(d["sht"], sentinel(N, BF))


class Fwd:
    """A B = 1 training launch of cnn_fwd, optionally carrying an fc1 update."""

    def __init__(self, gpu, bands, seed=3):
        self.C, self.gpu, self.bands = _C(), gpu, bands
        gen = torch.Generator().manual_seed(seed)
        self.images = torch.randint(0, 256, (1, 784), generator=gen, dtype=torch.uint8).to(gpu)
        self.labels = torch.tensor([7], dtype=torch.int32, device=gpu)
        self.w1 = (torch.randn(288, generator=gen) * 0.3).to(gpu)
        self.b1 = (torch.randn(32, generator=gen) * 0.1).to(gpu)
        self.w2 = (torch.randn(64 * 288, generator=gen) * 0.1).to(BF).to(gpu)
        self.b2 = (torch.randn(64, generator=gen) * 0.1).to(gpu)

    def run(self, h=None, step=1, p0=None, m0=None, g=None):
        gpu, C = self.gpu, self.C
        o = dict(pool=Guarded(sentinel(FEAT, BF), gpu))
        pmask = torch.full((FEAT + 128,), 0x55, dtype=torch.uint8, device=gpu)
        ylab = torch.full((1,), -1, dtype=torch.int32, device=gpu)
        band = self.bands > 1
        xg = None if band else torch.zeros(784, dtype=torch.uint8, device=gpu)
        a1g = torch.zeros(676 * 32, dtype=BF, device=gpu) if band else None
        xng = torch.zeros(784, dtype=BF, device=gpu) if band else None
        fcc = None
        if h is not None:
            o.update(p=Guarded(p0, gpu), m=Guarded(m0, gpu), g=Guarded(g, gpu),
                     sh=Guarded(sentinel(N, BF), gpu), sht=Guarded(sentinel(N, BF), gpu))
            fcc = _update_tuple(C, gpu, h, step, o["p"].view, o["g"].view, o["m"].view, o["sh"].view,
                                o["sht"].view)
        C.cnn_fwd(self.images, self.labels, None, None, 1, 1, self.w1, self.b1, self.w2, self.b2,
                  o["pool"].view, pmask[:FEAT], xg, ylab, self.bands, a1g, xng, fc_carry=fcc)
        torch.cuda.synchronize()
        out = {k: v.read() for k, v in o.items()}
        out["pmask"], out["ylab"] = pmask.cpu(), ylab.cpu()
        assert (out["pmask"][FEAT:] == 0x55).all(), "pmask written past the batch"
        return out


@pytest.mark.parametrize("hname,step", [("mom_wd", 1), ("mom_wd", 2), ("nesterov", 2)])
@pytest.mark.parametrize("bands", [1, 6])
def test_carried_update(gpu, bands, hname, step):
    """fc_carry on cnn_fwd (bands 1) and cnn_fwd_band (bands 6) over a seeded gradient: the
    update against ref_update, both copies from the returned weights, the gradient read only,
    and the forward's own outputs bit-identical to the launch without fc_carry."""
    h = HYPERS[hname]
    p0, m0 = _state(5)
    g = torch.randn(N, generator=torch.Generator().manual_seed(6)) * 0.1
    g[::16] = 0.0
    fw = Fwd(gpu, bands)
    a = fw.run(h, step, p0, m0, g)
    assert same_bits(a["g"], g)
    # R (test_gpu_optim.roundings): p 6 / 8, m 2 / 4 on a later step, the first step 2 less
    measure(f"carried-{hname}/bands{bands}", "sgd", h, step, p0, g, m0, None, {"p": a["p"], "m": a["m"]})
    check_copies(a)
    b = fw.run()
    for k in ("pool", "pmask", "ylab"):
        assert torch.equal(a[k].view(torch.uint8), b[k].view(torch.uint8)), k
    assert (b["ylab"] == 7).all() and not same_bits(b["pool"], sentinel(FEAT, BF))


@pytest.mark.parametrize("hname,step", [("mom_wd", 2), ("nesterov", 1)])
def test_one_formula_three_kernels(gpu, hname, step):
    """The same p0, m0, gradient, hyper-parameters and step through optim_kernel's fc1
    segment, fc1_bwd's fused update and the carried update: torch.equal p, m, W1 and W1^T
    (all three call update<OPT_SGD> with contraction off on identical fp32 inputs)."""
    h = HYPERS[hname]
    B = 40
    pr = Fc1Bwd(gpu, B, seed=77)
    fused = pr.run(h, step, store_grad=True)
    g = fused["g"]
    carried = Fwd(gpu, 1).run(h, step, pr.p0, pr.m0, g)
    off, total = 8, N + 16
    pad = lambda t: torch.cat([torch.zeros(off), t, torch.zeros(total - off - N)])
    P, G, M = (Guarded(pad(t), gpu) for t in (pr.p0, g, pr.m0))
    sh, sht = Guarded(sentinel(N, BF), gpu), Guarded(sentinel(N, BF), gpu)
    launch(_C(), gpu, "sgd", h, step, P.view, G.view, M.view, None,
           [(off, HID, FEAT, sh.view, sht.view, None, False, True, True)])
    opt = dict(p=P.read()[off:off + N], m=M.read()[off:off + N], sh=sh.read(), sht=sht.read())
    for k in ("p", "m", "sh", "sht"):
        assert same_bits(opt[k], fused[k]), f"optimizer vs fused: {k}"
        assert same_bits(opt[k], carried[k]), f"optimizer vs carried: {k}"
