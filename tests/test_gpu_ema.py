"""The exponential moving average of the weights on the GPU (csrc/kernels/ema.hip, optim/ema.py):
the kernel against a float32 NumPy oracle; TrainProgram with the average on, through the graphs,
against a host-driven oracle (the same program without the average, one step at a time, the test
applying the NumPy update to the whole weights after every step); graphs against eager; the
world-size > 1 chains composed on one GPU against the local chain; evaluation of the average; and
the CLI against the CPU path.

Everything here is compared bit for bit but the CLI test, whose tolerances are
tests/test_gpu_label_smoothing.py's for the same comparison."""
import functools

import numpy as np
import pytest
import torch

from pytorch_distributed_mnist_amd.data.dropout import DropoutSpec
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.optim.ema import EmaSpec, ema_weight
from pytorch_distributed_mnist_amd.optim.schedule import ScheduleSpec
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_gpu_app import EPOCH_RE, cli

pytestmark = pytest.mark.gpu

GUARD = 4096
SIZES = [1, 3, 4, 5, 2047, 2048, 2049, 7850, 1199882]


def _C():
    from pytorch_distributed_mnist_amd.ops import _ext
    return _ext.require()


def numpy_weight(D, k, warmup):
    """w = float32(1 - d_k), d_k in fp64 (the issue's definition, not optim/ema.py's code)."""
    d = np.float64(D)
    if warmup:
        d = np.minimum(d, (np.float64(1.0) + np.float64(k)) / (np.float64(10.0) + np.float64(k)))
    return np.float32(np.float64(1.0) - d)


def numpy_ema(e, p, w):
    """e + w (p - e): three float32 roundings."""
    d = (p - e).astype(np.float32)
    s = (np.float32(w) * d).astype(np.float32)
    return (e + s).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(n):
    """(p, e) float32 [n + GUARD]: normal-distributed, with lanes of p == e, +-0 and 1e-30 among
    the first n (as many as fit), and a guard of a fixed pattern behind."""
    g = np.random.default_rng(n)
    p = g.standard_normal(n + GUARD).astype(np.float32)
    e = g.standard_normal(n + GUARD).astype(np.float32)
    special = [(0.25, 0.25), (0.0, -0.0), (-0.0, 0.0), (0.0, 0.0), (-0.0, -0.0), (1e-30, 0.5),
               (0.5, 1e-30), (1e-30, -1e-30), (1e-30, 1e-30), (0.0, 1e-30), (-1.5, -0.0)]
    for i, (pv, ev) in enumerate(special):
        for at in (i, n - 1 - i):                   # at the front, and in the scalar tail
            if 0 <= at < n and n > len(special):
                p[at], e[at] = pv, ev
    if n <= len(special):                           # the tiny sizes: p == e, -0 and 1e-30 lanes
        for i, (pv, ev) in zip(range(n), [(0.25, 0.25), (0.0, -0.0), (1e-30, 0.5), (0.5, 1e-30),
                                          (-0.0, 0.0)]):
            p[i], e[i] = pv, ev
    return p, e


def _bits(a):
    return np.asarray(a).view(np.int32)


def _check_kernel(gpu, n, D, warmup, word, offset, nt):
    C = _C()
    p_np, e_np = _inputs(n)
    p = torch.from_numpy(p_np).to(gpu)
    e = torch.from_numpy(e_np.copy()).to(gpu)
    step = torch.tensor([word], dtype=torch.int64, device=gpu)
    C.ema_update(p, e, n, ema_weight(D), warmup, D, step, offset, nt=nt)
    torch.cuda.synchronize()
    want = e_np.copy()
    want[:n] = numpy_ema(e_np[:n], p_np[:n], numpy_weight(D, word + offset, warmup))
    got = e.cpu().numpy()
    assert np.array_equal(_bits(got[:n]), _bits(want[:n])), \
        (n, D, warmup, word, int((_bits(got[:n]) != _bits(want[:n])).sum()))
    assert np.array_equal(_bits(got[n:]), _bits(e_np[n:])), "guard behind ema"
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(p_np)), "params (and their guard)"
    assert step.item() == word


@pytest.mark.parametrize("nt", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_numpy(gpu, n, nt):
    """ema_update against the NumPy oracle, bit for bit, in both store variants: without warmup
    D = 0.5, 0.999, 1 - 2^-20 (the step word and the offset are then not used: any value);
    with warmup D = 0.999 at update index word + offset = 1 + 0 (the first), 5 + 3 and
    10,000 - 7 (past the first k with d_k = D, 8990).  The 4,096 floats behind both buffers,
    the parameters and the step word keep their bits."""
    for D in (0.5, 0.999, 1.0 - 2.0 ** -20):
        _check_kernel(gpu, n, D, False, 123, -45, nt)
    for word, offset in ((1, 0), (5, 3), (10000, -7)):
        _check_kernel(gpu, n, 0.999, True, word, offset, nt)
    assert numpy_weight(0.999, 1, True) > numpy_weight(0.999, 8, True) > \
        numpy_weight(0.999, 9993, True) == numpy_weight(0.999, 1, False)


def test_kernel_argument_checks(gpu):
    C = _C()
    p = torch.zeros(64, device=gpu)
    e = torch.ones(64, device=gpu)
    step = torch.ones(1, dtype=torch.int64, device=gpu)
    w = ema_weight(0.9)
    for bad in (lambda: C.ema_update(p, e, 65, w, False, 0.9, step, 0),
                lambda: C.ema_update(p, e, 0, w, False, 0.9, step, 0),
                lambda: C.ema_update(p, p, 64, w, False, 0.9, step, 0),
                lambda: C.ema_update(p, p[16:], 48, w, False, 0.9, step, 0),
                lambda: C.ema_update(p[1:], e, 8, w, False, 0.9, step, 0),
                lambda: C.ema_update(p, e.double(), 64, w, False, 0.9, step, 0),
                lambda: C.ema_update(p, e, 64, w, False, 1.0, step, 0),
                lambda: C.ema_update(p, e, 64, 0.1, False, 0.9, step, 0),     # not a float32 value
                lambda: C.ema_update(p, e, 64, w, True, 0.9, step.int(), 0),
                lambda: C.ema_update(p.cpu(), e, 64, w, False, 0.9, step, 0)):
        with pytest.raises(RuntimeError):
            bad()
    torch.cuda.synchronize()
    assert torch.equal(e, torch.ones(64, device=gpu))         # nothing ran


# ---------------------------------------------------------------------------- program level
EPOCHS = 2
SPEC = EmaSpec(0.9, warmup=True)


def _program(arch, dtype, opt, B, n, ema, graphs, **kw):
    train, test = synthetic_split(n, True), synthetic_split(64, False)
    p = build_local_program(arch, dtype, "cuda", B, train, test, optimizer=opt,
                            lr=1e-3 if opt == "adam" else 0.05, momentum=0.9, seed=4,
                            use_graphs=graphs, ema=ema, **kw)
    p.optimizer.sync_hyperparams()
    return p


def _state(p):
    torch.cuda.synchronize()
    p.reducer.check()
    p.gpu.check_device()
    return [p.arena.params.clone()] + [v.clone() for v in p.optimizer.state_buffers().values()]


def _run_epochs(p, n, epochs=EPOCHS, between=None):
    """`epochs` epochs as the app runs them (the next epoch's order handed over for the ahead
    gather); between(epoch) runs after each."""
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(epochs + 1)]
    for e in range(epochs):
        p.set_train_indices(order[e], order[e + 1] if e + 1 < epochs else None, epoch=e)
        p.train_epoch()
        if between is not None:
            between(e)
    return _state(p)


def _run_oracle(p, n, spec):
    """The same program without the average, one train_steps(B, 1) at a time (each updates in
    place, so the weights are whole afterwards), the float32 NumPy average applied on the host
    after every step."""
    assert p.ema is None and p.gpu.ema is None
    B = p.batch_size
    full, tail = divmod(n, B)
    e = p.arena.params.cpu().numpy().copy()
    k = 0
    for ep in range(EPOCHS):
        p.set_train_indices(distributed_indices(n, 1, 0, ep).to(torch.int32), epoch=ep)
        p.gpu.begin_epoch()
        for i in range(full + (1 if tail else 0)):
            p.gpu.train_steps(B if i < full else tail, 1)
            torch.cuda.synchronize()
            k += 1
            e = numpy_ema(e, p.arena.params.cpu().numpy(), numpy_weight(spec.decay, k, spec.warmup))
    return _state(p), e, k


CONFIGS = {
    # name: (arch, dtype, optimizer, B, samples per epoch: three full steps and a ragged tail)
    "cnn-bf16-256": ("cnn", "bf16", "sgd", 256, 864),     # the batch of the carried fc1 update
    "cnn-bf16-bands": ("cnn", "bf16", "sgd", 32, 32 * 3 + 12),
    "cnn-bf16-5": ("cnn", "bf16", "sgd", 5, 5 * 3 + 3),
    "cnn-fp32": ("cnn", "fp32", "sgd", 32, 32 * 3 + 12),
    "linear-adam": ("linear", "fp32", "adam", 256, 864),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_program_average_matches_the_host_oracle(gpu, name):
    """--ema-decay 0.9 --ema-warmup over two epochs through the graphs: the training weights,
    the optimizer state and the average have the bits of the host-driven oracle -- so every
    step's whole weights entered the average once, in order, and turning the average on left
    training untouched.  At B = 256 the program without the average carries its fc1 update
    into the next forward launch; the one with it does not."""
    arch, dtype, opt, B, n = CONFIGS[name]
    p = _program(arch, dtype, opt, B, n, SPEC, True)
    q = _program(arch, dtype, opt, B, n, None, False)
    if name == "cnn-bf16-256":
        assert not p.gpu.carries_across_graphs(B) and not p.gpu._local_carry(B)
        assert _program(arch, dtype, opt, B, n, None, True).gpu.carries_across_graphs(B)
    assert torch.equal(p.ema.params, p.arena.params) and p.ema.updates == 0
    got = _run_epochs(p, n)
    assert p.gpu.graphs
    want, e, k = _run_oracle(q, n, SPEC)
    assert p.ema.updates == k == EPOCHS * 4
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (name, i, (a - b).abs().max().item())
    avg = p.ema.params.cpu().numpy()
    assert np.array_equal(_bits(avg), _bits(e)), (name, int((_bits(avg) != _bits(e)).sum()))
    assert not np.array_equal(avg, got[0].cpu().numpy())


def test_graphs_equal_eager_with_dropout_and_a_schedule(gpu):
    """Two epochs with --dropout and --lr-schedule cosine on: graph replays and eager launches
    leave the same bits in the weights, the momentum and the average."""
    B, n = 32, 32 * 3 + 12
    res = {}
    for graphs in (False, True):
        sched = ScheduleSpec("cosine", 0.05, EPOCHS, 4, warmup=2, lr_min=0.1)
        p = _program("cnn", "bf16", "sgd", B, n, SPEC, graphs, dropout=DropoutSpec(0.5, seed=77),
                     schedule=sched)
        res[graphs] = _run_epochs(p, n) + [p.ema.params.clone()]
        assert bool(p.gpu.graphs) == graphs and p.ema.updates == 8
    for i, (a, b) in enumerate(zip(res[False], res[True])):
        assert torch.equal(a, b), i
    assert not torch.equal(res[True][0], res[True][-1])


def test_resume_offsets_the_update_index(gpu):
    """A program whose average and count were restored (a resume: the optimizer-step word starts
    where the optimizer's state says, the update index where the checkpoint says) continues as
    the uninterrupted program: the offset between the two is the launch's argument."""
    arch, dtype, opt, B, n = CONFIGS["linear-adam"]
    p = _program(arch, dtype, opt, B, n, SPEC, True)
    straight = _run_epochs(p, n) + [p.ema.params.clone()]
    a = _program(arch, dtype, opt, B, n, SPEC, True)
    _run_epochs(a, n, epochs=1)
    b = _program(arch, dtype, opt, B, n, SPEC, True)
    b.arena.load_state_dict(a.arena.state_dict())
    b.optimizer.load_state_dict(a.optimizer.state_dict())
    b.ema.load_state_dict(a.ema.state_dict(), a.ema.updates)
    b.set_train_indices(distributed_indices(n, 1, 0, 1).to(torch.int32), epoch=1)
    b.train_epoch()
    assert b.gpu._ema_off == 0 and b.ema.updates == 8
    for i, (x, y) in enumerate(zip(straight, _state(b) + [b.ema.params.clone()])):
        assert torch.equal(x, y), i
    # the same leg with the count restored as 0 (a checkpoint without an average): another
    # offset, other warmup weights, another average
    c = _program(arch, dtype, opt, B, n, SPEC, True)
    c.arena.load_state_dict(a.arena.state_dict())
    c.optimizer.load_state_dict(a.optimizer.state_dict())
    c.ema.load_state_dict(a.ema.state_dict(), 0)
    c.set_train_indices(distributed_indices(n, 1, 0, 1).to(torch.int32), epoch=1)
    c.gpu.begin_epoch()
    c.gpu.prepare(B, sizes=(3,))           # graphs captured ahead of the first step, as the
    assert c.gpu.graphs                    # start-up check and the benchmark do
    c.train_epoch()
    torch.cuda.synchronize()
    assert c.gpu._ema_off == -4 and c.ema.updates == 4
    assert not torch.equal(c.ema.params, straight[-1])


# ---------------------------------------------------------------------------- structures
def _structure_run(gpu, B, mode, capsys=None):
    n = B * 3 + 12
    comm = None
    kw = dict(transport="rccl")
    if mode != "local":
        from pytorch_distributed_mnist_amd.parallel.comm import RcclComm
        comm = RcclComm(0, 1, gpu)
        kw = dict(comm=comm, force_comm=True, transport="rccl")
    p = _program("cnn", "bf16", "sgd", B, n, SPEC, True, **kw)
    if comm is not None:
        assert p.reducer.kind == "rccl" and p.reducer.active
        p.gpu.set_rccl_mode(mode)
        if mode == "carry":
            # not offered with the average: nocarry, one notice line (asked twice, said once)
            p.gpu.set_rccl_mode("side")
            assert not p.gpu.fc_carry and not p.gpu.fc_side and not p.gpu.fc_early
            assert not p.gpu.shard_fc and "--ema-decay" in p.shard_unsupported_reason()
            out = capsys.readouterr().out
            assert out.count("notice: --ema-decay") == 1 and "'nocarry'" in out
        else:
            assert p.gpu.fc_early == (mode == "early") and not p.gpu.fc_carry
        assert not p.gpu._fwd_carry_on(B)
    state = _run_epochs(p, n)
    out = state + [p.gpu.wf1.clone(), p.gpu.current_wf1t().clone(), p.ema.params.clone()]
    if comm is not None:
        p.reducer.close()
        comm.close()
    return out


@functools.lru_cache(maxsize=None)
def _local(gpu, B):
    return _structure_run(gpu, B, "local")


@pytest.mark.parametrize("mode,B", [("nocarry", 32), ("nocarry", 256), ("early", 32),
                                    ("carry", 256)])
def test_structures_with_the_average_match_local(gpu, mode, B, capsys):
    """The RCCL chains of world size > 1 through a forced 1-rank communicator
    (tests/test_gpu_comm.py's composition), the average on, two epochs of graph replays with a
    ragged tail: the local chain's weights, momentum, bf16 W1 / W1^T and average, bit for bit.
    Asking for carry runs nocarry."""
    want = _local(gpu, B)
    got = _structure_run(gpu, B, mode, capsys)
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), (mode, i)


# ---------------------------------------------------------------------------- evaluation
@pytest.mark.parametrize("name", ["cnn-bf16-256", "cnn-fp32", "linear-adam"])
def test_evaluation_reads_the_average_and_leaves_training_alone(gpu, name):
    """Train an epoch, evaluate and predict (the average, then the training weights), train one
    more: the bits of a run that never evaluated, in the weights, the optimizer state, the
    average and the bf16 copies.  evaluate() with the average is evaluate() of a fresh program
    whose training weights were loaded from ema_state_dict.  (bf16 CNN: three steps per epoch,
    so the evaluation falls on the odd step phase of the W1^T double buffer.)"""
    arch, dtype, opt, B, _ = CONFIGS[name]
    n = B * 2 + 40
    seen = {}

    def look(e):
        if e == 0:
            seen["avg"] = p.evaluate()
            seen["raw"] = p.evaluate(average=False)
            seen["pred"] = p.predict()
            seen["pred_raw"] = p.predict(average=False)
            seen["sd"] = p.ema.state_dict()

    def copies(prog):
        g = prog.gpu
        if name != "cnn-bf16-256":
            return []
        return [g.wf1.clone(), g.current_wf1t().clone(), g.w2.clone(), g.w2t.clone()]

    p = _program(arch, dtype, opt, B, n, SPEC, True)
    got = _run_epochs(p, n, between=look) + [p.ema.params.clone()] + copies(p)
    if name == "cnn-bf16-256":
        assert p.gpu.phase_period == 2
    q = _program(arch, dtype, opt, B, n, SPEC, True)
    want = _run_epochs(q, n) + [q.ema.params.clone()] + copies(q)
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (name, i)

    fresh = _program(arch, dtype, opt, B, n, None, True)
    fresh.arena.load_state_dict(seen["sd"])
    if hasattr(fresh.gpu, "refresh_shadows"):
        fresh.gpu.refresh_shadows()
    loss, acc = fresh.evaluate()
    assert (loss.average, acc.accuracy) == (seen["avg"][0].average, seen["avg"][1].accuracy)
    assert loss.average != seen["raw"][0].average
    assert torch.equal(fresh.predict().log_probs, seen["pred"].log_probs)
    assert not torch.equal(seen["pred_raw"].log_probs, seen["pred"].log_probs)


# ---------------------------------------------------------------------------- CLI
@pytest.mark.parametrize("conv,loss_tol,acc_tol", [("exact", 5e-5, 0.1), ("x3", 2e-3, 0.5)])
def test_cnn_fp32_cli_gpu_matches_cpu_with_the_average(gpu, tmp_path, monkeypatch, conv, loss_tol,
                                                       acc_tol):
    """tests/test_gpu_label_smoothing.py's GPU-vs-CPU CLI comparison with --ema-decay 0.99: its
    epochs and tolerances (exact products: both epochs; split-bf16: the first).  The test
    figures come from the averaged weights on both paths; the checkpoints hold the average and
    its count."""
    monkeypatch.setenv("PDM_F32_CONV", conv)
    d1, d2 = tmp_path / "gpu", tmp_path / "cpu"
    d1.mkdir()
    d2.mkdir()
    epochs = 2 if conv == "exact" else 1
    common = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.05", "--dtype", "fp32",
              "--synthetic-size", "1024", "--epochs", str(epochs), "--seed", "4",
              "--ema-decay", "0.99"]
    g = [l for l in cli(common, d1) if l.startswith("Epoch:")]
    c = [l for l in cli(common, d2, device="cpu", backend="gloo") if l.startswith("Epoch:")]
    assert len(g) == len(c) == epochs
    for lg, lc in zip(g, c):
        print(lg, "|", lc)
        mg, mc = EPOCH_RE.match(lg), EPOCH_RE.match(lc)
        for i in (3, 5):
            assert abs(float(mg.group(i)) - float(mc.group(i))) < loss_tol, (lg, lc)
        for i in (4, 6):
            assert abs(float(mg.group(i)) - float(mc.group(i))) <= acc_tol, (lg, lc)
    for d in (d1, d2):
        ck = torch.load(d / "checkpoints" / f"checkpoint_{epochs - 1}.pth.tar", weights_only=True)
        assert ck["ema_updates"] == 4 * epochs
        assert list(ck["ema_state_dict"]) == list(ck["state_dict"])
    # the GPU's own evaluation of its checkpoint's average reproduces the epoch's test figures
    ck = str(d1 / "checkpoints" / f"checkpoint_{epochs - 1}.pth.tar")
    ev = [l for l in cli(["--arch", "cnn", "--optimizer", "sgd", "--dtype", "fp32", "--evaluate",
                          "--resume", ck, "--ema-decay", "0.99"], d1) if l.startswith("test loss:")]
    m = EPOCH_RE.match(g[-1])
    assert ev == ["test loss: {}, test acc: {}%.".format(m.group(5), m.group(6))]
