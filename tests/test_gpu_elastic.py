"""The elastic epoch gather (csrc/kernels/augment.hip gather_epoch_elastic_kernel) against its
NumPy oracle (data/augment.py augment_batch), bit for bit: the kernel alone, against the
augmenting gather at elastic_q = 0, through the training program's double-buffered epoch
gathers, and through the CLI."""
import pytest
import torch

from pytorch_distributed_mnist_amd.data.augment import AugmentSpec, augment_batch
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_gpu_app import EPOCH_RE, cli

pytestmark = pytest.mark.gpu

NIMG = 3000
SETTINGS = {"elastic": AugmentSpec(0, 0.0, 0.0, seed=31, elastic=2.0),
            "all": AugmentSpec(2, 10.0, 0.1, seed=(9 << 32) + 32, elastic=1.5),
            "max": AugmentSpec(8, 0.0, 0.0, seed=33, elastic=3.0)}
EPOCHS = (0, 3)


@pytest.fixture(scope="module")
def source():
    """3000 random source images and labels, and the oracle's transform of every one of them
    per (setting, epoch): computed once, shared by the shapes below (a gathered row is the
    transform of its dataset row, wherever it lands)."""
    g = torch.Generator().manual_seed(0)
    images = torch.randint(0, 256, (NIMG, 784), dtype=torch.uint8, generator=g)
    labels = torch.randint(0, 10, (NIMG,), dtype=torch.int32, generator=g)
    every = torch.arange(NIMG)
    expect = {(name, ep): augment_batch(images, every, ep, spec)
              for name, spec in SETTINGS.items() for ep in EPOCHS}
    return images, labels, expect


def _tables(spec):
    return [torch.from_numpy(t).cuda() for t in spec.tables()]


@pytest.mark.parametrize("n,max_wgs,host", [(1, 0, False), (63, 0, False), (64, 0, True),
                                            (1000 + 37, 0, True), (5000, 7, False)])
def test_gather_epoch_elastic_matches_oracle(gpu, source, n, max_wgs, host):
    """gather_epoch_elastic equals augment_batch bit for bit (images) and plain indexing
    (labels), at the gather's edge shapes: less than one 64-row pass, exactly one, a ragged
    last pass, a capped grid that strides; the order read from device memory or a pinned host
    buffer, with duplicates; elastic only (A = 2), all four ranges (A = 1.5, a seed with a
    non-zero high word) and A = 3 with shift 8; epochs 0 and 3.  Nothing is written past row
    n and the counters are reset."""
    from pytorch_distributed_mnist_amd.ops import _ext
    C = _ext.require()
    images, labels, expect = source
    d_images, d_labels = images.cuda(), labels.cuda()
    idx = torch.randint(0, NIMG, (n,), dtype=torch.int32,
                        generator=torch.Generator().manual_seed(n))
    il = idx.long()
    assert n < 1000 or il.unique().numel() < n        # duplicates
    d_idx = idx.pin_memory() if host else idx.cuda()
    for name, spec in SETTINGS.items():
        cosq, sinq, invz = _tables(spec)
        for ep in EPOCHS:
            out_i = torch.full((n + 3, 784), 7, dtype=torch.uint8, device="cuda")
            out_l = torch.full((n + 3,), -1, dtype=torch.int32, device="cuda")
            ctr = torch.full((4,), 9, dtype=torch.int64, device="cuda")
            step = torch.full((1,), 5, dtype=torch.int64, device="cuda")
            C.gather_epoch_elastic(d_images, d_labels, d_idx, out_i, out_l, ctr, step, 11, max_wgs,
                                   cosq, sinq, invz, spec.shift, ep, spec.seed, spec.elastic_q)
            torch.cuda.synchronize()
            got = out_i[:n].cpu()
            want = expect[(name, ep)][il]
            assert torch.equal(got, want), \
                (name, ep, int((got != want).any(1).sum()), "rows differ")
            assert torch.equal(out_l[:n].cpu(), labels[il])
            assert bool((out_i[n:] == 7).all()) and bool((out_l[n:] == -1).all())
            assert int(ctr.abs().sum()) == 0 and int(step.item()) == 11
    # the settings and epochs do differ (the comparison above is not vacuous)
    assert not torch.equal(expect[("all", 0)], expect[("all", 3)])
    assert not torch.equal(expect[("elastic", 0)], expect[("elastic", 3)])
    assert not torch.equal(expect[("elastic", 0)], images)
    assert not torch.equal(expect[("elastic", 0)], expect[("max", 0)])
    assert not torch.equal(expect[("all", 0)],
                           augment_batch(images, torch.arange(NIMG), 0,
                                         AugmentSpec(2, 10.0, 0.1, seed=(9 << 32) + 32)))


@pytest.mark.parametrize("n,max_wgs", [(1000 + 37, 0), (5000, 7)])
def test_zero_elastic_equals_augmenting_gather(gpu, n, max_wgs):
    """elastic_q = 0 through the elastic kernel: gather_epoch_augment's output, bit for bit,
    at (2, 10 degrees, 0.1)."""
    from pytorch_distributed_mnist_amd.ops import _ext
    C = _ext.require()
    g = torch.Generator().manual_seed(1)
    d_images = torch.randint(0, 256, (NIMG, 784), dtype=torch.uint8, generator=g).cuda()
    d_labels = torch.randint(0, 10, (NIMG,), dtype=torch.int32, generator=g).cuda()
    idx = torch.randint(0, NIMG, (n,), dtype=torch.int32,
                        generator=torch.Generator().manual_seed(n)).cuda()
    spec = AugmentSpec(2, 10.0, 0.1, seed=23)
    cosq, sinq, invz = _tables(spec)
    outs = []
    for elastic in (False, True):
        out_i = torch.full((n + 3, 784), 7, dtype=torch.uint8, device="cuda")
        out_l = torch.full((n + 3,), -1, dtype=torch.int32, device="cuda")
        if elastic:
            C.gather_epoch_elastic(d_images, d_labels, idx, out_i, out_l, None, None, 0, max_wgs,
                                   cosq, sinq, invz, spec.shift, 2, spec.seed, 0)
        else:
            C.gather_epoch_augment(d_images, d_labels, idx, out_i, out_l, None, None, 0, max_wgs,
                                   cosq, sinq, invz, spec.shift, 2, spec.seed)
        torch.cuda.synchronize()
        outs.append((out_i, out_l))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0][:n], d_images[idx.long()])
    with pytest.raises(RuntimeError, match="elastic_q"):
        C.gather_epoch_elastic(d_images, d_labels, idx, out_i, out_l, None, None, 0, max_wgs,
                               cosq, sinq, invz, spec.shift, 2, spec.seed, 769)


def test_epoch_plumbing_through_the_program(gpu):
    """Linear model, 1000 samples, B = 64, epochs 0..3 (graphs, a ragged tail, both halves of
    the epoch buffer twice), as test_gpu_augment's: after epoch e, half e & 1 of the epoch
    buffer holds augment_batch(images[idx_e], idx_e, e) with the elastic field on; with the next
    order handed over, the other half holds epoch e + 1's once the ahead gather's event has
    completed.  Gathering every epoch at its boundary instead gives the same parameters bit
    for bit."""
    train = synthetic_split(1000, True)
    test = synthetic_split(128, False)
    spec = AugmentSpec(2, 0.0, 0.0, seed=17, elastic=2.0)
    n = len(train)
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(5)]
    want = [augment_batch(train.images[o.long()], o.long(), e, spec) for e, o in enumerate(order)]
    plain = AugmentSpec(2, 0.0, 0.0, seed=17)
    assert not torch.equal(want[0], augment_batch(train.images[order[0].long()],
                                                  order[0].long(), 0, plain))
    params = []
    for ahead in (True, False):
        p = build_local_program("linear", "fp32", "cuda", 64, train, test, optimizer="adam",
                                lr=1e-3, seed=7, use_graphs=True, augment=spec)
        p.optimizer.sync_hyperparams()
        with pytest.raises(ValueError, match="epoch"):
            p.set_train_indices(order[0])
        for e in range(4):
            p.set_train_indices(order[e], order[e + 1] if ahead else None, epoch=e)
            p.train_epoch()
            torch.cuda.synchronize()
            buf = p.gpu.ep_images.view(2, n, 784)
            assert torch.equal(buf[e & 1].cpu(), want[e]), (ahead, e)
            assert torch.equal(p.gpu.ep_labels.view(2, n)[e & 1].cpu().long(),
                               train.labels[order[e].long()])
            if ahead:
                pend = p.gpu._pending
                assert pend is not None and pend[2] is not None and pend[3] == e + 1
                pend[2].synchronize()
                assert torch.equal(buf[1 - (e & 1)].cpu(), want[e + 1]), (ahead, e)
        torch.cuda.synchronize()
        params.append(p.arena.params.clone())
    assert torch.equal(params[0], params[1])


def test_linear_cli_gpu_matches_cpu_with_elastic(gpu, tmp_path):
    """test_linear_cli_gpu_matches_cpu with --aug-elastic 2 --aug-shift 2: the GPU path (elastic
    gather) and the CPU path (augment_batch per batch) train on bit-identical inputs, so that
    test's tolerances carry over."""
    d1, d2 = tmp_path / "gpu", tmp_path / "cpu"
    d1.mkdir()
    d2.mkdir()
    common = ["--synthetic-size", "4096", "--epochs", "2", "--seed", "2",
              "--aug-elastic", "2", "--aug-shift", "2"]
    g = [l for l in cli(common, d1) if l.startswith("Epoch:")]
    c = [l for l in cli(common, d2, device="cpu", backend="gloo") if l.startswith("Epoch:")]
    assert len(g) == len(c) == 2
    for lg, lc in zip(g, c):
        mg, mc = EPOCH_RE.match(lg), EPOCH_RE.match(lc)
        for i in (3, 5):
            assert abs(float(mg.group(i)) - float(mc.group(i))) < 2e-5, (lg, lc)
        for i in (4, 6):
            assert abs(float(mg.group(i)) - float(mc.group(i))) <= 0.05, (lg, lc)


def test_cnn_cli_with_elastic_is_deterministic(gpu, tmp_path):
    """The bf16 CNN through the CLI with --aug-elastic: two well-formed epoch lines, and a
    second identical run prints the same lines."""
    runs = []
    for name in ("a", "b"):
        d = tmp_path / name
        d.mkdir()
        out = cli(["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.05", "--synthetic-size",
                   "8192", "--epochs", "2", "--seed", "1", "--aug-elastic", "2"], d)
        ep = [l for l in out if l.startswith("Epoch:")]
        assert len(ep) == 2 and all(EPOCH_RE.match(l) for l in ep), out
        runs.append(ep)
    assert runs[0] == runs[1]
