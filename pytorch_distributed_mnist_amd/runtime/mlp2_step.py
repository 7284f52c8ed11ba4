"""Two-hidden-layer MLP GPU step program (``--arch mlp2``): 784 -> fc1 128 -> ReLU -> fc2 128 ->
ReLU -> fc3 10, fp32 semantics.

  mlp_fwd      split-K fc1 GEMM on the raw uint8 rows of the epoch buffer -> part1, ylab (MlpStep's)
  mlp_hid_fwd  h1 = relu(fc1.bias + sum of part1) kept for the backward; pre2 = h1 . fc2.weight^T
               as a one-split partial
  cnn_head     its "fc1 bias" is fc2.bias, its "fc2" is fc3: bias + ReLU (+ dropout), fc3, CE,
               head backward -> dh2 in fp32, head slabs (launch_head_train: every twin applies)
  mlp_hid_bwd  dh1 = [h1 > 0] dh2 . fc2.weight | the fc2.weight gradient
  mlp_bwd      dW1 from dh1, and fc1's bias gradient (dh1's column sums) | head-slab reduction
               -> fc3.weight, fc3.bias, fc2.bias gradients              -> the one bucket complete
  world size 1: optimizer;  world size > 1: all-reduce -> optimizer

The hidden layer runs on the fp32 MFMA from the fp32 master weight (``csrc/kernels/mlp_hid.hip``,
docs/kernels.md "MLP, two hidden layers"): no shadow planes beyond fc1.weight's.

Evaluation and prediction are GpuStepBase's (gpu_step.py): per chunk of EVAL_CHUNK images,
_eval_forward below -- mlp_fwd -> mlp_hid_fwd, h1 not kept -- then cnn_head or cnn_predict_head
on pre2.
"""
from __future__ import annotations

import torch

from .gpu_step import EVAL_CHUNK
from .mlp_step import MlpStep

NAMES = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")


def hid_groups(b: int) -> int:
    """Workgroups of mlp_hid_fwd per 16-row m-tile (each recomputes the h1 tile for its 128 /
    groups output units): 2 while they fit the 256 CUs in one round -- half the MFMA chain per
    wave, measured 6.3 against 7.7 us at B = 256 -- else 1 (5.3 against 5.6 us at B = 4096)."""
    return 2 if 2 * -(-b // 16) <= 256 else 1


class Mlp2Step(MlpStep):
    names = NAMES

    def __init__(self, prog, use_graphs):
        super().__init__(prog, use_graphs)
        f32, dev = torch.float32, self.device
        cap = max(self.bfull, EVAL_CHUNK)
        self.h1 = torch.zeros(self.ldt * 128, dtype=f32, device=dev)
        self.dh1 = torch.zeros(self.ldt * 128, dtype=f32, device=dev)
        self.pre2 = torch.empty(cap * 128, dtype=f32, device=dev)

    def _fwd2(self, images, labels, ctr, bfull, b, ws, h1, spe=0) -> None:
        """Both hidden layers of b rows: pre2 [1][b][128] and ylab for the head that follows."""
        P, w1split = ws
        s = self._fwd(images, labels, ctr, bfull, b, w1split, spe=spe)
        self.C.mlp_hid_fwd(self.part, s, b, P["fc1.bias"], P["fc2.weight"], h1, self.pre2,
                           ngroups=hid_groups(b))

    def _train_impl(self, B: int) -> None:
        C, P, G = self.C, self.P, self.G
        ldt = -(-B // 32) * 32
        images = self.ep_images.view(-1, 784)
        self._fwd2(images, self.ep_labels, self.ctr[0:1], self.bfull, B, (P, self.w1split), self.h1,
                   spe=self.spe)
        self.launch_head_train(self.pre2, 1, B, P["fc2.bias"], P["fc3.weight"], P["fc3.bias"],
                               self.ylab, None, None, ldt, self.head_slab,
                               self.metrics.train_view(), self.ctr[0:1], self.opt._step_dev, None,
                               self.dh32)
        C.mlp_hid_bwd(self.dh32, self.h1, P["fc2.weight"], B, self.dh1, G["fc2.weight"])
        # the head has advanced the data-step counter: the backward reads the rows of counter - 1
        C.mlp_bwd(images, self.ctr[0:1], self.bfull, B, self.dh1, ldt, G["fc1.weight"],
                  self.head_slab, G["fc3.weight"], G["fc3.bias"], G["fc2.bias"],
                  self.metrics.train_view(), spe=self.spe, ctr_advanced=True,
                  dh_colsum=G["fc1.bias"])
        self._update_one_bucket()

    def _eval_forward(self, images, labels, b, ws):
        P, w1 = (self.P, self.w1split) if ws is None else ws
        # (a quantised or pruned weight set: mlp_fwd_i8's, mlp_fwd_mx4's or mlp_fwd_sp24's partials,
        # and d1 in fc1.bias's place)
        part, s = self._eval_fc1(images, labels, b, w1)
        self.C.mlp_hid_fwd(part, s, b, P["fc1.bias"], P["fc2.weight"], None, self.pre2,
                           ngroups=hid_groups(b))
        return self.pre2, 1, P["fc2.bias"], P["fc3.weight"], P["fc3.bias"]
