"""GPU time of the epoch gathers at one rank's epoch (n = 60,000 by default): gather_epoch
(data.hip), gather_epoch_augment, gather_epoch_elastic and gather_epoch_mixup (augment.hip), on
an otherwise idle GPU.

    python tools/gather_bench.py [n]

Each kernel is captured 20 times back to back into one hipGraph and the graph replayed
(device events around three replays); the order is read from device memory, as a capture
needs, and every output is checked against the other path before it is timed.  The augmenting
gather hides in half an epoch of steps; the shortest is Linear at B = 256 on one rank
(235 steps x 12.4 us / 2 = 1.4 ms), printed beside the times.
"""
import sys

import torch

sys.path.insert(0, ".")
from pytorch_distributed_mnist_amd.data.augment import AugmentSpec, augment_batch
from pytorch_distributed_mnist_amd.data.mixup import MixupSpec, mix_batch
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.ops import _ext


def timeit(fn, iters=20):
    fn()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        fn()
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 60000
    C = _ext.require()
    train = synthetic_split(n, True)
    images = train.images.cuda()
    labels = train.labels.to(device="cuda", dtype=torch.int32)
    order = distributed_indices(n, 1, 0, 0).to(torch.int32)
    idx = order.cuda()
    out_i = torch.empty(n, 784, dtype=torch.uint8, device="cuda")
    out_l = torch.empty(n, dtype=torch.int32, device="cuda")
    print(f"n = {n}: half of the shortest epoch (Linear, B = 256) = "
          f"{-(-n // 256) * 12.4 / 2:.0f} us")
    us = timeit(lambda: C.gather_epoch(images, labels, idx, out_i, out_l, None, None, 0, 0))
    assert torch.equal(out_i, images[idx.long()])
    print(f"gather_epoch                               {us:8.1f} us  "
          f"({2 * n * 784 / us / 1e3:.0f} GB/s read + written)")
    for name, spec in (("identity (0, 0, 0)", AugmentSpec(0, 0.0, 0.0)),
                       ("shift 2", AugmentSpec(2, 0.0, 0.0, 1)),
                       ("shift 2, rotate 10, zoom 0.1", AugmentSpec(2, 10.0, 0.1, 1)),
                       ("shift 8, rotate 45, zoom 0.5", AugmentSpec(8, 45.0, 0.5, 1))):
        cosq, sinq, invz = (torch.from_numpy(t).cuda() for t in spec.tables())
        fn = lambda: C.gather_epoch_augment(images, labels, idx, out_i, out_l, None, None, 0, 0,
                                            cosq, sinq, invz, spec.shift, 1, spec.seed)
        us = timeit(fn)
        k = min(n, 2048)                       # the oracle on the first rows
        want = augment_batch(train.images[order[:k].long()], order[:k].long(), 1, spec)
        assert torch.equal(out_i[:k].cpu(), want), name
        print(f"gather_epoch_augment {name:30s} {us:8.1f} us")
    for name, spec in (("elastic 2", AugmentSpec(0, 0.0, 0.0, 1, 2.0)),
                       ("shift 2, rotate 10, zoom 0.1, el. 2", AugmentSpec(2, 10.0, 0.1, 1, 2.0))):
        cosq, sinq, invz = (torch.from_numpy(t).cuda() for t in spec.tables())
        fn = lambda: C.gather_epoch_elastic(images, labels, idx, out_i, out_l, None, None, 0, 0,
                                            cosq, sinq, invz, spec.shift, 1, spec.seed,
                                            spec.elastic_q)
        us = timeit(fn)
        k = min(n, 2048)
        want = augment_batch(train.images[order[:k].long()], order[:k].long(), 1, spec)
        assert torch.equal(out_i[:k].cpu(), want), name
        print(f"gather_epoch_elastic {name:30s} {us:8.1f} us")
    mix = MixupSpec(0.4, 1)
    qt = torch.from_numpy(mix.table().copy()).cuda()
    for name, spec in (("mixup 0.4 alone", AugmentSpec(0, 0.0, 0.0, 1)),
                       ("mixup 0.4, elastic 2", AugmentSpec(0, 0.0, 0.0, 1, 2.0)),
                       ("mixup 0.4, s 2, r 10, z 0.1, el. 2", AugmentSpec(2, 10.0, 0.1, 1, 2.0))):
        cosq, sinq, invz = (torch.from_numpy(t).cuda() for t in spec.tables())
        fn = lambda: C.gather_epoch_mixup(images, labels, idx, out_i, out_l, None, None, 0, 0,
                                          cosq, sinq, invz, spec.shift, 1, spec.seed,
                                          spec.elastic_q, qt, n, mix.seed)
        us = timeit(fn)
        k = min(n, 2048)
        sel = order[:k].long()
        want = augment_batch(mix_batch(train.images, sel, 1, mix)[0], sel, 1, spec)
        assert torch.equal(out_i[:k].cpu(), want), name
        print(f"gather_epoch_mixup   {name:30s} {us:8.1f} us")


if __name__ == "__main__":
    main()
