"""MLP GPU step program (``--arch mlp``): 784 -> fc1 128 -> ReLU -> fc2 10, fp32 semantics.

  mlp_fwd   split-K fc1 GEMM on the raw uint8 rows of the epoch buffer -> fp32 partials, ylab
  cnn_head  fc1 reduce + bias + ReLU, fc2, CE, head backward (dh in fp32), counters -- the CNN
            programs' head and its smoothing / dropout / mixup twins (launch_head_train)
  mlp_bwd   dW1 tiles | head-slab reduction                         -> the one bucket complete
  world size 1: optimizer;  world size > 1: all-reduce -> optimizer

The image operand of both GEMMs is exact in bf16; fc1's weight goes in as hi / lo bf16 planes
that the optimizer keeps current (``csrc/kernels/mlp.hip``, docs/kernels.md "MLP").

Evaluation and prediction are GpuStepBase's (gpu_step.py): per chunk of EVAL_CHUNK images,
_eval_forward below -- mlp_fwd -- then cnn_head or cnn_predict_head.  With an int8 weight set
(weight_set_int8: predict(quantize="int8")) the chunk's fc1 is mlp_fwd_i8 on the integer MFMA
instead (``csrc/kernels/mlp_i8.hip``, docs/kernels.md "int8 evaluation"), with an MXFP4 one
(weight_set_mxfp4: predict(quantize="mxfp4")) mlp_fwd_mx4 on the block-scaled MFMA
(``csrc/kernels/mlp_mx4.hip``, docs/kernels.md "MXFP4 evaluation"), with a 2:4-pruned one
(weight_set_sparse24: predict(quantize="sparse24")) mlp_fwd_sp24 on the structured-sparsity MFMA
(``csrc/kernels/mlp_sp24.hip``, docs/kernels.md "2:4 sparse evaluation"); the head is the same.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from .cpu_step import check_attack
from .gpu_step import EVAL_CHUNK, GpuStepBase, split_bf16

NAMES = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")


def mlp_splitk(b: int) -> int:
    """Split-K of mlp_fwd for b rows: the 25 k-steps over 25, 5 or 1 workgroups per 16-row
    m-tile, the most that keeps the launch within two rounds of the 256 CUs."""
    mt = -(-b // 16)
    for s in (25, 5):
        if mt * s <= 512:
            return s
    return 1


def mlp_i8_splitk(b: int) -> int:
    """Split-K of mlp_fwd_i8 for b rows: the 13 k-steps of 64 over 13 workgroups per 16-row
    m-tile while that keeps the launch within two rounds of the 256 CUs (b <= 624), else 1."""
    return 13 if -(-b // 16) * 13 <= 512 else 1


# rows of mlp_fwd_i8's partials for any chunk of up to EVAL_CHUNK rows
I8_PART_ROWS = max(mlp_i8_splitk(b) * b for b in range(1, EVAL_CHUNK + 1))


class Int8Fc1(NamedTuple):
    """fc1 of an int8 weight set, in the place of the hi / lo planes: q1 int8 [128 x 832] (rows
    zero-padded), c1 fp32 [128] = alpha s1, and the partials buffer mlp_fwd_i8 writes (sized for
    any chunk of up to EVAL_CHUNK rows; the training step's own is sized for its splits)."""
    q1: torch.Tensor
    c1: torch.Tensor
    part: torch.Tensor


def mlp_mx4_splitk(b: int) -> int:
    """Split-K of mlp_fwd_mx4 for b rows: the 7 k-steps of 128 over 7 workgroups per 16-row
    m-tile while that keeps the launch within two rounds of the 256 CUs (b <= 1168), else 1."""
    return 7 if -(-b // 16) * 7 <= 512 else 1


# rows of mlp_fwd_mx4's partials for any chunk of up to EVAL_CHUNK rows
MX4_PART_ROWS = max(mlp_mx4_splitk(b) * b for b in range(1, EVAL_CHUNK + 1))


class Mx4Fc1(NamedTuple):
    """fc1 of an MXFP4 weight set, in the place of the hi / lo planes: codes uint8 [128 x 448]
    (two E2M1 codes per byte, rows zero-padded to 896 columns), scales uint8 [128 x 28] (one E8M0
    byte per 32 columns), and the partials buffer mlp_fwd_mx4 writes (sized as Int8Fc1's)."""
    codes: torch.Tensor
    scales: torch.Tensor
    part: torch.Tensor


def mlp_sp24_splitk(b: int) -> int:
    """Split-K of mlp_fwd_sp24 for b rows: mlp_i8_splitk's rule, the 13 k-steps of 64 dense
    columns over 13 workgroups per 16-row m-tile while the launch stays within 512 workgroups (b
    <= 624), else 1."""
    return 13 if -(-b // 16) * 13 <= 512 else 1


class Sp24Fc1(NamedTuple):
    """fc1 of a 2:4-pruned weight set, in the place of the hi / lo planes: whi / wlo bf16 [128 x
    416] (the two survivors of every 4 columns, hi = bf16(w), lo = bf16(w - hi), rows zero-padded
    to 832 dense columns), index int32 [128 x 28] (their 2-bit positions, a word per two k-steps
    of a lane group), and the partials buffer mlp_fwd_sp24 writes (sized as Int8Fc1's)."""
    whi: torch.Tensor
    wlo: torch.Tensor
    index: torch.Tensor
    part: torch.Tensor


class MlpStep(GpuStepBase):
    names = NAMES

    def __init__(self, prog, use_graphs):
        super().__init__(prog, use_graphs)
        C, dev, B = self.C, self.device, self.bfull
        f32 = torch.float32
        self.ldt = -(-B // 32) * 32
        cap = max(B, EVAL_CHUNK)
        self.ylab = torch.empty(cap, dtype=torch.int32, device=dev)
        part_n = max(max(mlp_splitk(b) * b for b in range(1, B + 1)),
                     mlp_splitk(EVAL_CHUNK) * EVAL_CHUNK) * 128
        self.part = torch.empty(part_n, dtype=f32, device=dev)
        self.dh32 = torch.zeros(self.ldt * 128, dtype=f32, device=dev)
        self.head_slab = torch.empty(C.cnn_head_nblk(self.ldt) * C.CNN_HEAD_SLAB, dtype=f32,
                                     device=dev)
        a = self.arena
        self.P = {n: a.param(n) for n in self.names}
        self.G = {n: a.grad(n) for n in self.names}
        # fc1.weight as split-bf16 planes [hi | lo], each [128][784] row-major
        self.w1split = torch.empty(2 * 128 * 784, dtype=torch.bfloat16, device=dev)
        self.refresh_shadows()

    @torch.no_grad()
    def refresh_shadows(self) -> None:
        """Re-derive fc1.weight's hi / lo planes (hi = bf16(w), lo = bf16(w - hi)) from the fp32
        master: the optimizer keeps them current after every update, this covers any other
        change (construction, a re-broadcast)."""
        split_bf16(self.arena.param("fc1.weight"), self.w1split)

    @torch.no_grad()
    def weight_set(self, arena):
        """(name views, fc1.weight's hi / lo planes) of `arena`; fresh tensors, the training
        copy is not touched."""
        return ({n: arena.param(n) for n in self.names},
                split_bf16(arena.param("fc1.weight"), torch.empty_like(self.w1split)))

    @torch.no_grad()
    def weight_set_int8(self, arena):
        """The int8 weight set of `arena` (the training weights or the averaged ones), built by
        one mlp_quant_w1 launch: (name views with fc1.bias replaced by d1, Int8Fc1).  Fresh
        tensors, outside any capture; nothing of `arena` or of the training step is touched."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("weight_set_int8() allocates: call it outside a graph capture")
        dev, f32 = self.device, torch.float32
        q1 = torch.empty(128 * self.C.MLP_I8_KPAD, dtype=torch.int8, device=dev)
        s1, c1, d1 = (torch.empty(128, dtype=f32, device=dev) for _ in range(3))
        r1 = torch.empty(128, dtype=torch.int32, device=dev)
        self.C.mlp_quant_w1(arena.param("fc1.weight"), arena.param("fc1.bias"), q1, s1, r1, c1, d1)
        P = {n: arena.param(n) for n in self.names}
        P["fc1.bias"] = d1
        return P, Int8Fc1(q1, c1, torch.empty(I8_PART_ROWS * 128, dtype=f32, device=dev))

    @torch.no_grad()
    def weight_set_mxfp4(self, arena):
        """The MXFP4 weight set of `arena`, built by one mlp_quant_mx4 launch: (name views with
        fc1.bias replaced by d1, Mx4Fc1).  As weight_set_int8: fresh tensors, outside any
        capture, nothing of `arena` or of the training step is touched."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("weight_set_mxfp4() allocates: call it outside a graph capture")
        dev, kpad = self.device, self.C.MLP_MX4_KPAD
        codes = torch.empty(128 * kpad // 2, dtype=torch.uint8, device=dev)
        scales = torch.empty(128 * kpad // 32, dtype=torch.uint8, device=dev)
        d1 = torch.empty(128, dtype=torch.float32, device=dev)
        self.C.mlp_quant_mx4(arena.param("fc1.weight"), arena.param("fc1.bias"), codes, scales, d1)
        P = {n: arena.param(n) for n in self.names}
        P["fc1.bias"] = d1
        return P, Mx4Fc1(codes, scales,
                         torch.empty(MX4_PART_ROWS * 128, dtype=torch.float32, device=dev))

    @torch.no_grad()
    def weight_set_sparse24(self, arena):
        """The 2:4-pruned weight set of `arena`, built by one mlp_prune_24 launch: (name views
        with fc1.bias replaced by d1, Sp24Fc1).  As weight_set_int8: fresh tensors, outside any
        capture, nothing of `arena` or of the training step is touched."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("weight_set_sparse24() allocates: call it outside a graph capture")
        dev, half = self.device, self.C.MLP_SP24_KPAD // 2
        whi, wlo = (torch.empty(128 * half, dtype=torch.bfloat16, device=dev) for _ in range(2))
        index = torch.empty(128 * 28, dtype=torch.int32, device=dev)
        d1 = torch.empty(128, dtype=torch.float32, device=dev)
        self.C.mlp_prune_24(arena.param("fc1.weight"), arena.param("fc1.bias"), whi, wlo, index, d1)
        P = {n: arena.param(n) for n in self.names}
        P["fc1.bias"] = d1
        return P, Sp24Fc1(whi, wlo, index,
                          torch.empty(I8_PART_ROWS * 128, dtype=torch.float32, device=dev))

    def optimizer_segments(self):
        segs = []
        for p in self.arena.spec.params:
            off = self.arena.spec.offset(p.name)
            if p.name == "fc1.weight":
                n = p.numel
                segs.append((off, 1, n, self.w1split[:n], None, None, None, None, None,
                             self.w1split[n:]))
            else:
                segs.append((off, 1, p.numel, None, None))
        return segs

    def _fwd(self, images, labels, ctr, bfull, b, w1split, spe=0) -> int:
        s = mlp_splitk(b)
        n = 128 * 784
        self.C.mlp_fwd(images, labels, ctr, bfull, b, w1split[:n], w1split[n:], self.part,
                       self.ylab, s, spe=spe)
        return s

    def _train_impl(self, B: int) -> None:
        C, P, G = self.C, self.P, self.G
        ldt = -(-B // 32) * 32
        images = self.ep_images.view(-1, 784)
        s = self._fwd(images, self.ep_labels, self.ctr[0:1], self.bfull, B, self.w1split,
                      spe=self.spe)
        self.launch_head_train(self.part, s, B, P["fc1.bias"], P["fc2.weight"], P["fc2.bias"],
                               self.ylab, None, None, ldt, self.head_slab,
                               self.metrics.train_view(), self.ctr[0:1], self.opt._step_dev, None,
                               self.dh32)
        # the head has advanced the data-step counter: the backward reads the rows of counter - 1
        C.mlp_bwd(images, self.ctr[0:1], self.bfull, B, self.dh32, ldt, G["fc1.weight"],
                  self.head_slab, G["fc2.weight"], G["fc2.bias"], G["fc1.bias"],
                  self.metrics.train_view(), spe=self.spe, ctr_advanced=True)
        self._update_one_bucket()

    def _eval_fc1(self, images, labels, b, w1):
        """fc1's partials and ylab of b <= EVAL_CHUNK rows for evaluation: (part, splitk); w1 is
        the hi / lo planes, or the Int8Fc1 / Mx4Fc1 / Sp24Fc1 of a quantised or pruned weight
        set."""
        if isinstance(w1, Sp24Fc1):
            s = mlp_sp24_splitk(b)
            self.C.mlp_fwd_sp24(images, labels, b, w1.whi, w1.wlo, w1.index, w1.part, self.ylab, s)
            return w1.part, s
        if isinstance(w1, Mx4Fc1):
            s = mlp_mx4_splitk(b)
            self.C.mlp_fwd_mx4(images, labels, b, w1.codes, w1.scales, w1.part, self.ylab, s)
            return w1.part, s
        if isinstance(w1, Int8Fc1):
            s = mlp_i8_splitk(b)
            self.C.mlp_fwd_i8(images, labels, b, w1.q1, w1.c1, w1.part, self.ylab, s)
            return w1.part, s
        return self.part, self._fwd(images, labels, None, b, b, w1)

    def _eval_forward(self, images, labels, b, ws):
        P, w1 = (self.P, self.w1split) if ws is None else ws
        part, se = self._eval_fc1(images, labels, b, w1)
        return part, se, P["fc1.bias"], P["fc2.weight"], P["fc2.bias"]

    @torch.no_grad()
    def attack(self, images_u8: torch.Tensor, labels, eps: int, steps: int, alpha: int, ws=None,
               chunk=None) -> torch.Tensor:
        """The FGSM / PGD images of uint8 [N >= 1, 784] under the plain NLL of `labels`: uint8
        [N, 784] on the device, within `eps` grey levels of the input, after `steps` steps of
        `alpha` grey levels from the images themselves (csrc/kernels/mlp_attack.hip; docs/kernels.md
        "Adversarial evaluation").  Per chunk of `chunk` rows (default and at most EVAL_CHUNK) and
        step: mlp_fwd on the iterate, then mlp_attack, the iterates in two ping-pong buffers.
        ws: the weight set attacked (None: the training weights).  Allocates, so not inside a
        graph capture; nothing of the training step is touched."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("attack() allocates its buffers: call it outside a graph capture")
        eps, steps, alpha = check_attack(eps, steps, alpha)
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 2 or images_u8.shape[1] != 784 \
                or images_u8.shape[0] < 1:
            raise ValueError("attack() takes uint8 images [N >= 1, 784], got "
                             f"{images_u8.dtype} {tuple(images_u8.shape)}")
        dev = self.device
        images = images_u8.to(dev).contiguous()
        n = images.shape[0]
        if labels is None or labels.numel() != n:
            raise ValueError(f"attack() needs one label per image ({n})")
        lab = labels.to(device=dev, dtype=torch.int32).contiguous()
        chunk = EVAL_CHUNK if chunk is None else int(chunk)
        if not 1 <= chunk <= EVAL_CHUNK:
            raise ValueError(f"chunk must be in 1..{EVAL_CHUNK}, got {chunk}")
        P, w1split = (self.P, self.w1split) if ws is None else ws
        nw = 128 * 784
        out = torch.empty_like(images)
        pp = [torch.empty(min(chunk, n), 784, dtype=torch.uint8, device=dev) for _ in range(2)]
        for s in range(0, n, chunk):
            b = min(chunk, n - s)
            x0 = cur = images[s:s + b]
            for k in range(steps):
                dst = out[s:s + b] if k == steps - 1 else pp[k & 1][:b]
                se = self._fwd(cur, lab[s:s + b], None, b, b, w1split)
                self.C.mlp_attack(self.part, se, b, self.ylab, P["fc1.bias"], P["fc2.weight"],
                                  P["fc2.bias"], w1split[:nw], w1split[nw:], x0, cur, dst, eps,
                                  alpha)
                cur = dst
        return out

