"""GPU time of test-time augmentation (--tta V) on an otherwise idle GPU, by device events,
warm, medians with min-max over the repeats:

    python tools/tta_bench.py [n]

* tta_reduce alone (csrc/kernels/tta.hip) at n rows (10,000 by default) for V = 4, 8, 32, with
  labels, confusion and metrics: 100 back-to-back launches between two events, 30 repeats;
* the view gathers alone at n rows (affine ranges), the same way;
* the device part of predict() on an n-image test split at V = 1 (the plain path: the same-run
  baseline), 4 and 8, for the bf16 CNN and for Linear: events around one call, 30 repeats.
"""
import statistics
import sys

import torch

sys.path.insert(0, ".")
from pytorch_distributed_mnist_amd.data.augment import AugmentSpec
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.ops import _ext
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

SPEC = AugmentSpec(2, 10.0, 0.1, seed=7)


def events(fn, inner, repeats=30):
    """Microseconds per call of fn: `inner` calls between two device events, `repeats` times."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner * 1e3)
    return out


def show(name, us):
    print("{:<44s} {:10.2f} us ({:.2f}-{:.2f})".format(name, statistics.median(us), min(us),
                                                      max(us)), flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    C = _ext.require()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(0)
    y = torch.randint(0, 10, (n,), generator=g).to(device=dev, dtype=torch.int32)
    logp = torch.empty(n, 10, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    conf = torch.zeros(10, 10, dtype=torch.int64, device=dev)
    met = torch.zeros(3, dtype=torch.float64, device=dev)
    for V in (4, 8, 32):
        lv = torch.log_softmax(torch.randn(V, n, 10, generator=g) * 3.0, dim=-1).to(dev)
        show(f"tta_reduce n={n} V={V} labels+confusion+metrics",
             events(lambda: C.tta_reduce(lv, y, logp, pred, conf, met), 100))
        show(f"tta_reduce n={n} V={V} no labels",
             events(lambda: C.tta_reduce(lv, None, logp, pred), 100))

    train, test = synthetic_split(256, True), synthetic_split(n, False)
    for arch, dtype in (("cnn", "bf16"), ("linear", "fp32")):
        prog = build_local_program(arch, dtype, dev, 256, train, test, optimizer="sgd",
                                   use_graphs=False, augment=SPEC)
        step = prog.gpu
        if arch == "cnn":
            b = min(n, step.TTA_CHUNK)
            show(f"view gather (affine) {b} rows",
                 events(lambda: step.tta_view(step.test_images, 0, b, 1, SPEC), 20))
        for V in (1, 4, 8):
            if V == 1:
                fn = lambda: step.predict(step.test_images, step.test_labels)
            else:
                fn = lambda: step.predict_tta(step.test_images, step.test_labels, None, SPEC, V)
            show(f"predict() device time {arch} {dtype} n={n} V={V}", events(fn, 1))


if __name__ == "__main__":
    main()
