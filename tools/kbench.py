"""Per-kernel timing of the CNN step kernels at several batch sizes (CUDA events);
`kbench.py mlp [B ...]`: the MLP's two kernels and its step; `kbench.py mlp2 [B ...]`: the
two-hidden-layer MLP's hidden kernels (mlp_hid_fwd at both workgroup splits) and its step;
`kbench.py mlp_attack [B ...]`: mlp_attack at both workgroup splits beside its mlp_fwd;
`kbench.py mlp_i8 [B ...]`: mlp_fwd_i8 at both splits beside mlp_fwd, and mlp_quant_w1;
`kbench.py mlp_mx4 [B ...]`: mlp_fwd_mx4 at both splits beside mlp_fwd_i8 and mlp_fwd, and
mlp_quant_mx4; `kbench.py mlp_sp24 [B ...]`: mlp_fwd_sp24 at both splits beside those three, and
mlp_prune_24."""
import sys
import torch
sys.path.insert(0, ".")
from pytorch_distributed_mnist_amd.data.dropout import tag_labels
from pytorch_distributed_mnist_amd.data.mixup import MixupSpec
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.runtime.program import build_local_program
from pytorch_distributed_mnist_amd.runtime.cnn_step import choose_bands, choose_ipb
from pytorch_distributed_mnist_amd.runtime.mlp_step import mlp_splitk

train = synthetic_split(60000, True)
test = synthetic_split(512, False)


def timeit(fn, iters=50):
    """GPU time per call: `iters` back-to-back calls captured into one hipGraph and replayed
    (eager launches through the bindings would measure host overhead for small kernels)."""
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        fn()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for _ in range(iters):
                fn()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(3):
        g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / (3 * iters) * 1e3


def mlp(sizes):
    """mlp_fwd / mlp_bwd (csrc/kernels/mlp.hip) and the whole MLP step at each batch size."""
    for B in sizes:
        p = build_local_program("mlp", "fp32", "cuda", B, train, test, optimizer="sgd", lr=0.01,
                                use_graphs=False)
        p.optimizer.sync_hyperparams()
        p.set_train_indices(distributed_indices(len(train), 1, 0, 0))
        st = p.gpu
        C, G = st.C, st.G
        ldt = -(-B // 32) * 32
        st.train_step(B)
        torch.cuda.synchronize()
        z = torch.zeros(1, dtype=torch.int64, device="cuda")
        images = st.ep_images.view(-1, 784)
        fwd = lambda: st._fwd(images, st.ep_labels, z, B, B, st.w1split, spe=st.spe)
        bwd = lambda: C.mlp_bwd(images, z, B, B, st.dh32, ldt, G["fc1.weight"], st.head_slab,
                                G["fc2.weight"], G["fc2.bias"], G["fc1.bias"],
                                st.metrics.train_view(), spe=st.spe)
        t = [(timeit(fwd), timeit(bwd)) for _ in range(3)]
        st.ctr.zero_()
        step = timeit(lambda: st._train_impl(B), 8)
        print(f"mlp B={B:5d} S={fwd()} mlp_fwd|mlp_bwd x3: " +
              " ".join(f"{a:.2f}|{b:.2f}" for a, b in t) +
              f" | step={step:.1f}us -> {B / step:.2f}M img/s", flush=True)


def mlp2(sizes):
    """mlp_hid_fwd (1 and 2 workgroups per m-tile) / mlp_hid_bwd (csrc/kernels/mlp_hid.hip) and
    the whole mlp2 step at each batch size."""
    for B in sizes:
        p = build_local_program("mlp2", "fp32", "cuda", B, train, test, optimizer="sgd", lr=0.01,
                                use_graphs=False)
        p.optimizer.sync_hyperparams()
        p.set_train_indices(distributed_indices(len(train), 1, 0, 0))
        st = p.gpu
        C, P, G = st.C, st.P, st.G
        st.train_step(B)
        torch.cuda.synchronize()
        S = mlp_splitk(B)
        fwd = lambda g: C.mlp_hid_fwd(st.part, S, B, P["fc1.bias"], P["fc2.weight"], st.h1,
                                      st.pre2, ngroups=g)
        bwd = lambda: C.mlp_hid_bwd(st.dh32, st.h1, P["fc2.weight"], B, st.dh1, G["fc2.weight"])
        t = [(timeit(lambda: fwd(1)), timeit(lambda: fwd(2)), timeit(bwd)) for _ in range(3)]
        st.ctr.zero_()
        step = timeit(lambda: st._train_impl(B), 8)
        print(f"mlp2 B={B:5d} S={S} mlp_hid_fwd g=1|g=2|mlp_hid_bwd x3: " +
              " ".join(f"{a:.2f}|{b:.2f}|{c:.2f}" for a, b, c in t) +
              f" | step={step:.1f}us -> {B / step:.2f}M img/s", flush=True)


def mlp_attack(sizes):
    """mlp_attack (csrc/kernels/mlp_attack.hip) with seven workgroups per m-tile and with one,
    beside the mlp_fwd launch that feeds it, at each batch size."""
    for B in sizes:
        p = build_local_program("mlp", "fp32", "cuda", B, train, test, optimizer="sgd", lr=0.01,
                                use_graphs=False)
        st = p.gpu
        C, P = st.C, st.P
        x0 = train.images[:B].cuda()
        y = train.labels[:B].to(torch.int32).cuda()
        out = torch.empty_like(x0)
        n = 128 * 784
        fwd = lambda: st._fwd(x0, y, None, B, B, st.w1split)
        S = fwd()
        atk = lambda pb: C.mlp_attack(st.part, S, B, st.ylab, P["fc1.bias"], P["fc2.weight"],
                                      P["fc2.bias"], st.w1split[:n], st.w1split[n:], x0, x0, out,
                                      25, 6, None, pb)
        t = [(timeit(fwd), timeit(lambda: atk(7)), timeit(lambda: atk(1))) for _ in range(3)]
        print(f"mlp_attack B={B:5d} S={S} mlp_fwd|px_blocks=7|px_blocks=1 x3: " +
              " ".join(f"{a:.2f}|{b:.2f}|{c:.2f}" for a, b, c in t), flush=True)


def mlp_i8(sizes):
    """mlp_fwd_i8 at both splits beside mlp_fwd (at its own split) on the same rows, interleaved,
    at each batch size, and the one-off mlp_quant_w1 (csrc/kernels/mlp_i8.hip)."""
    from pytorch_distributed_mnist_amd.runtime.mlp_step import mlp_i8_splitk
    p = build_local_program("mlp", "fp32", "cuda", 1, train, test, optimizer="sgd", lr=0.01,
                            use_graphs=False)
    st = p.gpu
    _, w = st.weight_set_int8(p.arena)
    q1, s1, c1, d1 = (torch.empty_like(t) for t in (w.q1, w.c1, w.c1, w.c1))
    r1 = torch.empty(128, dtype=torch.int32, device="cuda")
    qk = lambda: st.C.mlp_quant_w1(p.arena.param("fc1.weight"), p.arena.param("fc1.bias"), q1, s1,
                                   r1, c1, d1)
    print("mlp_quant_w1 x3: " + " ".join(f"{timeit(qk):.2f}" for _ in range(3)), flush=True)
    n = 128 * 784
    for B in sizes:
        x = train.images[:B].cuda()
        y = train.labels[:B].to(torch.int32).cuda()
        part = torch.empty(25 * B * 128, device="cuda")
        S = mlp_splitk(B)
        f32 = lambda: st.C.mlp_fwd(x, y, None, B, B, st.w1split[:n], st.w1split[n:], part, st.ylab, S)
        i8 = lambda s: st.C.mlp_fwd_i8(x, y, B, w.q1, w.c1, part, st.ylab, s)
        t = [(timeit(f32), timeit(lambda: i8(13)), timeit(lambda: i8(1))) for _ in range(3)]
        print(f"mlp_i8 B={B:5d} mlp_fwd S={S}|mlp_fwd_i8 S=13|S=1 (rule: {mlp_i8_splitk(B)}) x3: " +
              " ".join(f"{a:.2f}|{b:.2f}|{c:.2f}" for a, b, c in t), flush=True)


def mlp_mx4(sizes):
    """mlp_fwd_mx4 at both splits beside mlp_fwd_i8 and mlp_fwd (each at its own rule's split) on
    the same rows, interleaved, at each batch size, and the one-off mlp_quant_mx4
    (csrc/kernels/mlp_mx4.hip)."""
    from pytorch_distributed_mnist_amd.runtime.mlp_step import mlp_i8_splitk, mlp_mx4_splitk
    p = build_local_program("mlp", "fp32", "cuda", 1, train, test, optimizer="sgd", lr=0.01,
                            use_graphs=False)
    st = p.gpu
    _, w8 = st.weight_set_int8(p.arena)
    _, w4 = st.weight_set_mxfp4(p.arena)
    codes, scales, d1 = torch.empty_like(w4.codes), torch.empty_like(w4.scales), torch.empty_like(w8.c1)
    qk = lambda: st.C.mlp_quant_mx4(p.arena.param("fc1.weight"), p.arena.param("fc1.bias"), codes,
                                    scales, d1)
    print("mlp_quant_mx4 x3: " + " ".join(f"{timeit(qk):.2f}" for _ in range(3)), flush=True)
    n = 128 * 784
    for B in sizes:
        x = train.images[:B].cuda()
        y = train.labels[:B].to(torch.int32).cuda()
        part = torch.empty(25 * B * 128, device="cuda")
        S, S8 = mlp_splitk(B), mlp_i8_splitk(B)
        f32 = lambda: st.C.mlp_fwd(x, y, None, B, B, st.w1split[:n], st.w1split[n:], part, st.ylab, S)
        i8 = lambda: st.C.mlp_fwd_i8(x, y, B, w8.q1, w8.c1, part, st.ylab, S8)
        mx = lambda s: st.C.mlp_fwd_mx4(x, y, B, w4.codes, w4.scales, part, st.ylab, s)
        t = [(timeit(f32), timeit(i8), timeit(lambda: mx(7)), timeit(lambda: mx(1))) for _ in range(3)]
        print(f"mlp_mx4 B={B:5d} mlp_fwd S={S}|mlp_fwd_i8 S={S8}|mlp_fwd_mx4 S=7|S=1 "
              f"(rule: {mlp_mx4_splitk(B)}) x3: " +
              " ".join(f"{a:.2f}|{b:.2f}|{c:.2f}|{d:.2f}" for a, b, c, d in t), flush=True)


def mlp_sp24(sizes):
    """mlp_fwd_sp24 at both splits beside mlp_fwd, mlp_fwd_i8 and mlp_fwd_mx4 (each at its own
    rule's split) on the same rows, interleaved, at each batch size, and the one-off mlp_prune_24
    (csrc/kernels/mlp_sp24.hip)."""
    from pytorch_distributed_mnist_amd.runtime.mlp_step import (mlp_i8_splitk, mlp_mx4_splitk,
                                                                mlp_sp24_splitk)
    p = build_local_program("mlp", "fp32", "cuda", 1, train, test, optimizer="sgd", lr=0.01,
                            use_graphs=False)
    st = p.gpu
    (_, w8), (_, w4), (_, ws) = (f(p.arena) for f in (st.weight_set_int8, st.weight_set_mxfp4,
                                                      st.weight_set_sparse24))
    whi, wlo, index, d1 = (torch.empty_like(t) for t in (ws.whi, ws.wlo, ws.index, w8.c1))
    pk = lambda: st.C.mlp_prune_24(p.arena.param("fc1.weight"), p.arena.param("fc1.bias"), whi, wlo,
                                   index, d1)
    print("mlp_prune_24 x3: " + " ".join(f"{timeit(pk):.2f}" for _ in range(3)), flush=True)
    n = 128 * 784
    for B in sizes:
        x = train.images[:B].cuda()
        y = train.labels[:B].to(torch.int32).cuda()
        part = torch.empty(25 * B * 128, device="cuda")
        S, S8, S4 = mlp_splitk(B), mlp_i8_splitk(B), mlp_mx4_splitk(B)
        f32 = lambda: st.C.mlp_fwd(x, y, None, B, B, st.w1split[:n], st.w1split[n:], part, st.ylab, S)
        i8 = lambda: st.C.mlp_fwd_i8(x, y, B, w8.q1, w8.c1, part, st.ylab, S8)
        mx = lambda: st.C.mlp_fwd_mx4(x, y, B, w4.codes, w4.scales, part, st.ylab, S4)
        sp = lambda s: st.C.mlp_fwd_sp24(x, y, B, ws.whi, ws.wlo, ws.index, part, st.ylab, s)
        t = [(timeit(f32), timeit(i8), timeit(mx), timeit(lambda: sp(13)), timeit(lambda: sp(1)))
             for _ in range(3)]
        print(f"mlp_sp24 B={B:5d} mlp_fwd S={S}|mlp_fwd_i8 S={S8}|mlp_fwd_mx4 S={S4}|mlp_fwd_sp24 "
              f"S=13|S=1 (rule: {mlp_sp24_splitk(B)}) x3: " +
              " ".join("|".join(f"{v:.2f}" for v in r) for r in t), flush=True)


def main():
  if sys.argv[1:2] == ["mlp_sp24"]:
      return mlp_sp24([int(b) for b in (sys.argv[2:] or ["32", "256", "624", "625", "2048"])])
  if sys.argv[1:2] == ["mlp_mx4"]:
      return mlp_mx4([int(b) for b in (sys.argv[2:] or ["32", "256", "1168", "1169", "2048"])])
  if sys.argv[1:2] == ["mlp_i8"]:
      return mlp_i8([int(b) for b in (sys.argv[2:] or ["32", "256", "624", "625", "2048"])])
  if sys.argv[1:2] == ["mlp_attack"]:
      return mlp_attack([int(b) for b in (sys.argv[2:] or ["32", "256", "2048"])])
  if sys.argv[1:2] == ["mlp"]:
      return mlp([int(b) for b in (sys.argv[2:] or ["32", "256", "4096"])])
  if sys.argv[1:2] == ["mlp2"]:
      return mlp2([int(b) for b in (sys.argv[2:] or ["32", "256", "4096"])])
  for B in [int(b) for b in (sys.argv[1:] or ["256", "1024", "4096"])]:
      p = build_local_program("cnn", "bf16", "cuda", B, train, test, optimizer="sgd", lr=0.01,
                              use_graphs=False)
      p.optimizer.sync_hyperparams()
      p.set_train_indices(distributed_indices(len(train), 1, 0, 0))
      st = p.gpu
      C, P, G = st.C, st.P, st.G
      ldt = -(-B // 32) * 32
      S = st.splitk_train
      bands = choose_bands(B)
      ipb = choose_ipb(B) if bands == 1 else 1
      nblk = C.cnn_bwd_nblk(B, ipb, bands)
      st.train_step(B)
      torch.cuda.synchronize()
      z = torch.zeros(1, dtype=torch.int64, device="cuda")
      epoch_word = torch.zeros(1, dtype=torch.int32, device="cuda")
      # the head with a learning-rate schedule on (kernels.h LrSched), beside the same head
      # advancing the step counter alone: scratch words, a table longer than the calls timed
      c1 = torch.zeros(1, dtype=torch.int64, device="cuda")
      sched = (torch.full((4096,), 0.01, dtype=torch.float64, device="cuda"),
               torch.zeros(1, dtype=torch.int64, device="cuda"),
               torch.zeros(1, dtype=torch.float64, device="cuda"))
      head = lambda **kw: C.cnn_head(st.part, S, B, P["fc1.bias"], P["fc2.weight"], P["fc2.bias"],
                                     st.ylab, True, st.dh, st.dht, ldt, st.head_slab,
                                     st.metrics.train_view(), None, c1, **kw)
      # the weight average's launch (ema.hip) over the arena into a scratch average, with plain
      # and with nontemporal accesses of the average
      avg = torch.zeros_like(p.arena.params)
      ema = lambda nt: C.ema_update(p.arena.params, avg, p.arena.spec.total, 0.0009765625, False,
                                    0.9990234375, c1, 0, nt=nt)
      tagged = tag_labels(train.labels).cuda()
      qt = torch.from_numpy(MixupSpec(0.4).table().copy()).cuda()
      ks = {
          "ema": lambda: ema(False),
          "ema_nt": lambda: ema(True),
          "cnn_fwd": lambda: C.cnn_fwd(st.ep_images.view(-1, 784), st.ep_labels, None, z, B, B,
                                       P["conv1.weight"], P["conv1.bias"], st.w2, P["conv2.bias"],
                                       st.pool, st.pmask, *st.fwd_outputs(B)),
          "fc1_fwd": lambda: C.fc1_fwd(st.pool, st.wf1, st.part, B, S),
          "cnn_head": lambda: C.cnn_head(st.part, S, B, P["fc1.bias"], P["fc2.weight"], P["fc2.bias"],
                                         st.ylab, True, st.dh, st.dht, ldt, st.head_slab,
                                         st.metrics.train_view(), None, None),
          # the head's masking variant at p = 0.5 (untagged labels: every row draws sample 0's
          # mask, the same work)
          "cnn_head_dropout": lambda: C.cnn_head_dropout(st.part, S, B, P["fc1.bias"],
                                                         P["fc2.weight"], P["fc2.bias"], st.ylab,
                                                         st.dh, st.dht, ldt, st.head_slab,
                                                         st.metrics.train_view(), None, None, None,
                                                         None, epoch_word, 1, 32768, 2.0),
          # the head with smoothed targets (E = 0.1)
          "cnn_head_smooth": lambda: C.cnn_head_smooth(st.part, S, B, P["fc1.bias"],
                                                       P["fc2.weight"], P["fc2.bias"], st.ylab,
                                                       st.dh, st.dht, ldt, st.head_slab,
                                                       st.metrics.train_view(), None, None, None,
                                                       None, 0.1),
          # the masking head's two-class variant (--mixup 0.4, p = 0.5): the row's pair is drawn
          # from the label word (untagged: sample 0's pair in every row, the same work), the
          # partner's label read from the tagged training labels
          "cnn_head_mixup": lambda: C.cnn_head_mixup(st.part, S, B, P["fc1.bias"], P["fc2.weight"],
                                                     P["fc2.bias"], st.ylab, st.dh, st.dht, ldt,
                                                     st.head_slab, st.metrics.train_view(), None,
                                                     None, None, None, epoch_word, 1, 32768, 2.0,
                                                     tagged, tagged.numel(), qt, 1),
          "cnn_head_step": lambda: head(),
          "cnn_head_sched": lambda: head(lr_sched=sched),
          "fc1_bwd": lambda: C.fc1_bwd(st.dh, st.dht, ldt, st.pool, st.current_wf1t(), B, G["fc1.weight"],
                                       st.dpool, st.head_slab, G["fc2.weight"], G["fc2.bias"],
                                       G["fc1.bias"], st.metrics.train_view(),
                                       st._fc_update() if st.fuse_fc1 else None),
          "cnn_bwd": lambda: C.cnn_bwd(st.xg, P["conv1.weight"], P["conv1.bias"], st.dpool, st.pmask,
                                       st.w2t, B, ipb, st.conv_slab, None, bands, st.a1g, st.xng),
          "conv_reduce": lambda: C.conv_reduce(st.conv_slab, nblk, G["conv2.weight"],
                                               G["conv2.bias"], G["conv1.weight"], G["conv1.bias"]),
          # the training step's update: the slab-fused launch at world size 1
          "optim": (lambda: st.launch_optimizer(st._fused_segments(nblk)))
                   if st.fuse_conv_reduce else (lambda: st.launch_optimizer()),
      }
      tot = 0.0
      line = []
      for name, fn in ks.items():
          us = timeit(fn)
          if name not in ("cnn_head_dropout", "cnn_head_smooth", "cnn_head_mixup", "cnn_head_step",
                          "cnn_head_sched", "ema", "ema_nt"):            # variants, opt-in launches
              tot += us
          line.append(f"{name}={us:.1f}")
      # the mixup head against the head it extends, interleaved
      pairs = [(timeit(ks["cnn_head_dropout"]), timeit(ks["cnn_head_mixup"])) for _ in range(4)]
      line.append("dropout|mixup x4: " + " ".join(f"{a:.2f}|{b:.2f}" for a, b in pairs))
      st.ctr.zero_()   # each step advances the data counter (rows are clamped past the epoch)
      step = timeit(lambda: st._train_impl(B), 8)
      print(f"B={B:5d} S={S} ipb={ipb} bands={bands} " + " ".join(line) + f" | sum={tot:.1f}us step={step:.1f}us "
            f"-> {B / step * 1e6 / 1e6:.2f}M img/s", flush=True)


if __name__ == "__main__":
    main()
