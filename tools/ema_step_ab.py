"""bf16 CNN step time through the graphs with and without the weight average, interleaved."""
import sys
import torch
sys.path.insert(0, ".")
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.optim.ema import EmaSpec
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

train = synthetic_split(60000, True)
test = synthetic_split(512, False)


def make(B, ema):
    p = build_local_program("cnn", "bf16", "cuda", B, train, test, optimizer="sgd", lr=0.01,
                            ema=ema)
    p.optimizer.sync_hyperparams()
    p.set_train_indices(distributed_indices(len(train), 1, 0, 0).to(torch.int32), epoch=0)
    p.gpu.begin_epoch()
    p.gpu.prepare(B)
    p.gpu.train_steps(B, 32)
    torch.cuda.synchronize()
    return p


def timed(p, B, n=64):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    p.gpu.train_steps(B, n)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


for B in (256, 32):
    progs = {"off": make(B, None), "ema": make(B, EmaSpec(0.999)),
             "ema+warmup": make(B, EmaSpec(0.999, True))}
    print(f"B={B} carry off/ema: {progs['off'].gpu.carries_across_graphs(B)} "
          f"{progs['ema'].gpu.carries_across_graphs(B)}", flush=True)
    for r in range(3):
        print(f"B={B} round {r}: " + "  ".join(f"{k}={timed(p, B):.2f}us" for k, p in progs.items()),
              flush=True)
