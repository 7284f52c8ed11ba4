"""The device-resident learning-rate schedule (csrc/kernels.h LrSched, optim/schedule.py) on the
GPU: the launches that advance the optimizer-step counter -- cnn_head, cnn_head_dropout,
lin_train -- called directly with a schedule (the rate word takes the table's entries, the cursor
moves on, every other output keeps its bits); TrainProgram with a schedule, eager and through
the graphs, against a host-driven oracle (the same program without a schedule, one step at a
time, the test writing each step's rate); every multi-GPU step structure composed on one GPU
against the local chain; and the CLI against the CPU path.

Everything here is compared bit for bit but the CLI test, whose tolerances are
tests/test_gpu_dropout.py's for the same comparison.  No test drives the cursor past the table
on the device: the over-run is the host's error, raised before anything is queued."""
import functools

import pytest
import torch

from pytorch_distributed_mnist_amd.data.dropout import DropoutSpec
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.optim.schedule import ScheduleSpec
from pytorch_distributed_mnist_amd.runtime.program import build_local_program

from test_gpu_app import EPOCH_RE, cli
from test_gpu_cnn_head import GUARD, HID, M0, SLAB, _C, _ldt, bits, make_inputs, nanbuf

pytestmark = pytest.mark.gpu

TABLE = [0.125, 0.3, 1e-3, 0.07, 2.5e-4]      # 5 entries; the cursor starts at 2
START = 2


def _sched(dev):
    return (torch.tensor(TABLE, dtype=torch.float64, device=dev),
            torch.tensor([START], dtype=torch.int64, device=dev),
            torch.tensor([-1.0], dtype=torch.float64, device=dev))


def _head_call(C, dev, inp, bf16_mode, dropout, sched):
    """One training-head launch into NaN-filled buffers -> every output, on the CPU."""
    part, bf1, wf2, bf2, y = inp
    S, B = part.shape[0], part.shape[1]
    ldt = _ldt(B)
    nblk = C.cnn_head_nblk(ldt)
    slab = nanbuf(nblk * SLAB, torch.float32, dev)
    metrics = torch.tensor(M0, dtype=torch.float64, device=dev)
    c0 = torch.tensor([41], dtype=torch.int64, device=dev)
    c1 = torch.tensor([7], dtype=torch.int64, device=dev)
    dh = dht = dh32 = None
    if bf16_mode:
        dh, dht = nanbuf(ldt * HID, torch.bfloat16, dev), nanbuf(ldt * HID, torch.bfloat16, dev)
    else:
        dh32 = nanbuf(ldt * HID, torch.float32, dev)
    args = (part.reshape(-1).to(dev), S, B, bf1.to(dev), wf2.reshape(-1).to(dev), bf2.to(dev))
    kw = {} if sched is None else {"lr_sched": sched}
    if dropout is None:
        C.cnn_head(*args, y.to(dev), True, dh, dht, ldt, slab, metrics, c0, c1, None, dh32, **kw)
    else:
        word = (y.long() | (torch.arange(B) * 977 << 4)).to(torch.int32)
        C.cnn_head_dropout(*args, word.to(dev), dh, dht, ldt, slab, metrics, c0, c1, None, dh32,
                           torch.tensor([3], dtype=torch.int32, device=dev), dropout.seed,
                           dropout.T, dropout.scale, **kw)
    torch.cuda.synchronize()
    out = dict(slab=slab.cpu(), metrics=metrics.cpu(), c0=c0.cpu(), c1=c1.cpu())
    for k, t in (("dh", dh), ("dht", dht), ("dh32", dh32)):
        if t is not None:
            out[k] = t.cpu()
    return out


def _same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if x.dtype in (torch.float32, torch.bfloat16):
            x, y = bits(x), bits(y)
        elif x.dtype == torch.float64:
            x, y = x.view(torch.int64), y.view(torch.int64)
        assert torch.equal(x, y), k


# test_gpu_cnn_head.py's smallest edge shapes: one valid row; a last row group with one valid row
@pytest.mark.parametrize("B,S", [(1, 32), (37, 32)])
@pytest.mark.parametrize("head", ["cnn_head", "cnn_head_dropout"])
@pytest.mark.parametrize("bf16_mode", [False, True])
def test_head_advances_the_schedule(gpu, B, S, head, bf16_mode):
    """Three launches with a 5-entry table and the cursor at 2: the rate word takes table[2],
    table[3], table[4] exactly and the cursor ends at 5; every other output (slab, dh / dht or
    dh32, the metrics, both counters, the NaN guards behind the buffers) has the bits of the
    same launch without the schedule."""
    C = _C()
    inp = make_inputs(B, S, 1, 1000 * B + S)
    drop = DropoutSpec(0.5, seed=(9 << 32) + 41) if head == "cnn_head_dropout" else None
    plain = _head_call(C, gpu, inp, bf16_mode, drop, None)
    assert (int(plain["c0"]), int(plain["c1"])) == (42, 8)
    for k in ("slab", "dh", "dht", "dh32"):
        if k in plain:
            assert torch.isnan(plain[k][-GUARD:].float()).all(), k
    table, cursor, lr = sched = _sched(gpu)
    for call in range(3):
        got = _head_call(C, gpu, inp, bf16_mode, drop, sched)
        assert lr.item() == TABLE[START + call], (call, lr.item())
        assert cursor.item() == START + call + 1
        _same_bits(got, plain)
    assert cursor.item() == len(TABLE)
    assert table.cpu().tolist() == TABLE                     # the table is only read


def test_head_schedule_argument_checks(gpu):
    """An evaluation head, or a head that does not advance the optimizer-step counter, takes no
    schedule; the table and the words are checked before the launch."""
    C = _C()
    part, bf1, wf2, bf2, y = (t.to(gpu) for t in make_inputs(4, 1, 1, 5))
    metrics = torch.zeros(3, dtype=torch.float64, device=gpu)
    c1 = torch.zeros(1, dtype=torch.int64, device=gpu)
    table, cursor, lr = _sched(gpu)
    args = (part.reshape(-1), 1, 4, bf1, wf2.reshape(-1), bf2, y)
    slab = torch.zeros(C.cnn_head_nblk(32) * SLAB, device=gpu)
    dh32 = torch.zeros(32 * HID, device=gpu)
    with pytest.raises(RuntimeError, match="training head"):
        C.cnn_head(*args, False, None, None, 32, None, metrics, None, None, None, None,
                   lr_sched=(table, cursor, lr))
    for bad in ((table, cursor, lr, lr), (table.float(), cursor, lr), (table, cursor.int(), lr),
                (table[:0], cursor, lr), (table, cursor, torch.zeros(2, dtype=torch.float64, device=gpu)),
                (table.cpu(), cursor, lr)):
        with pytest.raises(RuntimeError, match="lr_sched"):
            C.cnn_head(*args, True, None, None, 32, slab, metrics, None, c1, None, dh32, lr_sched=bad)
    with pytest.raises(RuntimeError, match="c1 is None"):
        C.cnn_head(*args, True, None, None, 32, slab, metrics, None, None, None, dh32,
                   lr_sched=(table, cursor, lr))
    torch.cuda.synchronize()
    assert cursor.item() == START and lr.item() == -1.0 and c1.item() == 0     # nothing ran


# test_gpu_linear.py's smallest edge shapes: one valid row; a last row group of one row
@pytest.mark.parametrize("B,bfull", [(1, 8), (13, 32)])
def test_lin_train_advances_the_schedule(gpu, B, bfull):
    """lin_train, the Linear chain's launch that advances the optimizer-step counter (in every
    world-size variant: lin_reduce and the optimizer launch advance the data step): the same
    three launches."""
    C = _C()
    g = torch.Generator().manual_seed(B)
    N = 4 * bfull
    images = torch.randint(0, 256, (N, 784), dtype=torch.uint8, generator=g).to(gpu)
    labels = torch.randint(0, 10, (N,), generator=g).to(gpu, torch.int32)
    W = (torch.randn(10, 784, generator=g) * 0.05).to(gpu)
    b = (torch.randn(10, generator=g) * 0.1).to(gpu)
    nblk = (bfull + C.LIN_ROWS - 1) // C.LIN_ROWS

    def call(sched):
        slab = torch.full((nblk * C.LIN_SLAB,), float("nan"), device=gpu)
        ctr = torch.tensor([2, 0], dtype=torch.int64, device=gpu)
        ostep = torch.tensor([7], dtype=torch.int64, device=gpu)
        metrics = torch.tensor(M0, dtype=torch.float64, device=gpu)
        kw = {} if sched is None else {"lr_sched": sched}
        C.lin_train(images, labels, None, ctr[0:1], bfull, B, W, b, slab, metrics, ostep, **kw)
        torch.cuda.synchronize()
        return dict(slab=slab.cpu(), ctr=ctr.cpu(), ostep=ostep.cpu(), metrics=metrics.cpu())

    plain = call(None)
    assert int(plain["ostep"]) == 8 and plain["ctr"].tolist() == [2, 0]
    table, cursor, lr = sched = _sched(gpu)
    for i in range(3):
        _same_bits(call(sched), plain)
        assert lr.item() == TABLE[START + i] and cursor.item() == START + i + 1
    with pytest.raises(RuntimeError, match="c1 is None"):
        C.lin_train(images, labels, None, torch.zeros(1, dtype=torch.int64, device=gpu), bfull, B,
                    W, b, torch.zeros(nblk * C.LIN_SLAB, device=gpu), None, None, lr_sched=sched)


# ---------------------------------------------------------------------------- program level
EPOCHS = 2


def _spec(lr0, spe):
    return ScheduleSpec("cosine", lr0, EPOCHS, spe, warmup=3, lr_min=0.1)


def _program(arch, dtype, opt, B, n, schedule, graphs, dropout=None, lr=0.05, **kw):
    train, test = synthetic_split(n, True), synthetic_split(64, False)
    p = build_local_program(arch, dtype, "cuda", B, train, test, optimizer=opt, lr=lr,
                            momentum=0.9, seed=4, use_graphs=graphs, dropout=dropout,
                            schedule=schedule, **kw)
    p.optimizer.sync_hyperparams()
    return p


def _state(p):
    torch.cuda.synchronize()
    p.reducer.check()
    p.gpu.check_device()
    out = [p.arena.params.clone()] + [v.clone() for v in p.optimizer.state_buffers().values()]
    out.append(p.optimizer._lr_dev.clone())
    return out


def _run_scheduled(p, n, spec):
    """EPOCHS epochs as the app runs them (the next epoch's order handed over for the ahead
    gather), checking the host's view of the rate after each."""
    table = spec.table()
    order = [distributed_indices(n, 1, 0, e).to(torch.int32) for e in range(EPOCHS + 1)]
    for e in range(EPOCHS):
        p.set_train_indices(order[e], order[e + 1] if e + 1 < EPOCHS else None, epoch=e)
        p.train_epoch()
        last = float(table[(e + 1) * spec.spe - 1])
        assert p.optimizer.param_groups[0]["lr"] == last
        assert p.optimizer._lr_dev.item() == last
        assert p.gpu._sched_cursor.item() == (e + 1) * spec.spe
    return _state(p)


def _run_oracle(p, n, spec):
    """The same program without a schedule, one train_steps(B, 1) at a time, the rate of global
    step g written into the optimizer's lr (host word, then the device word) before it."""
    assert p.schedule is None and p.gpu.schedule is None
    table = spec.table()
    B = p.batch_size
    full, tail = divmod(n, B)
    for e in range(EPOCHS):
        p.set_train_indices(distributed_indices(n, 1, 0, e).to(torch.int32), epoch=e)
        p.gpu.begin_epoch()
        for i in range(spec.spe):
            p.optimizer.param_groups[0]["lr"] = float(table[e * spec.spe + i])
            p.optimizer.sync_hyperparams()
            p.gpu.train_steps(B if i < full else tail, 1)
    return _state(p)


CONFIGS = {
    # name: (arch, dtype, optimizer, B, samples per epoch (a ragged tail), dropout)
    "linear-adam": ("linear", "fp32", "adam", 32, 32 * 5 + 20, None),
    "cnn-bf16-bands": ("cnn", "bf16", "sgd", 32, 32 * 5 + 20, None),
    # 18 steps per epoch: 17 full batches = a 16-step graph and its 1-step remainder, the
    # fc1 update carried from one into the other (B > 128: fc1_carry_local), then the tail
    "cnn-bf16-carry": ("cnn", "bf16", "sgd", 144, 144 * 17 + 40, None),
    "cnn-fp32": ("cnn", "fp32", "sgd", 32, 32 * 5 + 20, None),
    "cnn-bf16-dropout": ("cnn", "bf16", "sgd", 32, 32 * 5 + 20, DropoutSpec(0.5, seed=77)),
}


@pytest.mark.parametrize("name", list(CONFIGS))
def test_program_schedule_eager_graphs_and_oracle(gpu, name):
    """cosine, warmup 3, --lr-min 0.1 over two epochs with a ragged tail: the eager run, the
    graph run and the host-driven oracle end with the same bits in the parameters, the optimizer
    state and the rate word; the host's lr follows; a step past the run raises before anything
    is queued; removing the schedule drops the graphs."""
    arch, dtype, opt, B, n, drop = CONFIGS[name]
    lr0 = 1e-3 if opt == "adam" else 0.05
    spec = _spec(lr0, -(-n // B))
    if name == "cnn-bf16-carry":
        assert spec.spe == 18
    res = {}
    for mode, graphs in (("eager", False), ("graphs", True)):
        p = _program(arch, dtype, opt, B, n, spec, graphs, drop, lr=lr0)
        if name == "cnn-bf16-carry":
            assert p.gpu.carries_across_graphs(B) and not p.gpu.carries_across_graphs(40)
        res[mode] = _run_scheduled(p, n, spec)
        assert bool(p.gpu.graphs) == graphs
        if graphs:
            # past the table: the host refuses, nothing reaches the device
            with pytest.raises(RuntimeError, match="schedule"):
                p.gpu.train_steps(B, 1)
            torch.cuda.synchronize()
            assert p.gpu._sched_cursor.item() == spec.total
            assert all(torch.equal(a, b) for a, b in zip(_state(p), res[mode]))
            p.set_schedule(None)
            assert not p.gpu.graphs and p.gpu.lr_sched() is None
    res["oracle"] = _run_oracle(_program(arch, dtype, opt, B, n, None, False, drop, lr=lr0), n, spec)
    for mode in ("graphs", "oracle"):
        for i, (a, b) in enumerate(zip(res["eager"], res[mode])):
            assert torch.equal(a, b), (mode, i, (a - b).abs().max().item())
    # the schedule matters: a constant rate ends elsewhere
    flat = _program(arch, dtype, opt, B, n, None, False, drop, lr=lr0)
    flat_state = _run_oracle(flat, n, ScheduleSpec("constant", lr0, EPOCHS, spec.spe))
    assert not torch.equal(flat_state[0], res["eager"][0])


def test_resume_positions_the_cursor(gpu):
    """A program started at epoch 1 (a resume) puts the cursor at spe before its first step: its
    rates are the second half of the table, not the first."""
    arch, dtype, opt, B, n, _ = CONFIGS["linear-adam"]
    spec = _spec(1e-3, -(-n // B))
    p = _program(arch, dtype, opt, B, n, spec, True, lr=1e-3)
    assert p.gpu._sched_cursor.item() == 0
    p.set_train_indices(distributed_indices(n, 1, 0, 1).to(torch.int32), epoch=1)
    p.train_epoch()
    torch.cuda.synchronize()
    assert p.gpu._sched_cursor.item() == 2 * spec.spe
    assert p.optimizer._lr_dev.item() == float(spec.table()[-1]) == p.optimizer.param_groups[0]["lr"]
    with pytest.raises(ValueError, match="epoch"):
        p.set_train_indices(distributed_indices(n, 1, 0, 0).to(torch.int32))


# ---------------------------------------------------------------------------- structures
def _comm(gpu):
    from pytorch_distributed_mnist_amd.parallel.comm import RcclComm
    return RcclComm(0, 1, gpu)


# test_gpu_comm.py::test_calibration_candidates_as_composed_match_local's structures (RCCL carry
# at B >= 256, early below, as there), and with them the RCCL side-stream and sharded (zero) ones
STRUCTURES = {
    "xgmi": ("xgmi", "carry", True), "xgmi-noxchg": ("xgmi", "carry", False),
    "rccl-nocarry": ("rccl", "nocarry", True), "rccl-carry": ("rccl", "carry", True),
    "rccl-early": ("rccl", "early", True), "rccl-side": ("rccl", "side", True),
    "rccl-zero": ("rccl", "zero", True),
}


def _structure_run(gpu, B, name):
    n = B * 19 + 40
    spec = _spec(0.05, -(-n // B))
    comm = None
    kw = dict(transport="rccl")
    if name != "local":
        transport, mode, xchg = STRUCTURES[name]
        comm = _comm(gpu)
        kw = dict(comm=comm, force_comm=True, transport=transport)
    p = _program("cnn", "bf16", "sgd", B, n, spec, True, **kw)
    if comm is not None:
        assert p.reducer.kind == transport
        p.gpu.set_rccl_mode(mode, invalidate=False)
        p.gpu.xgmi_exchange = xchg and p.structure.xgmi_exchange
        p.gpu.invalidate_graphs()
        if transport == "xgmi":
            assert p.gpu._xchg() == xchg
        if mode == "zero":
            assert p.gpu.shard_fc
    state = _run_scheduled(p, n, spec)
    p.sync_master()
    torch.cuda.synchronize()
    out = state[:2] + [p.gpu.wf1.clone(), p.gpu.current_wf1t().clone(), state[-1]]
    if comm is not None:
        p.reducer.close()
        comm.close()
    return out


@functools.lru_cache(maxsize=None)
def _local(gpu, B):
    return _structure_run(gpu, B, "local")


@pytest.mark.parametrize("name,B", [("xgmi", 32), ("xgmi", 256), ("xgmi-noxchg", 32),
                                    ("xgmi-noxchg", 256), ("rccl-nocarry", 32),
                                    ("rccl-nocarry", 256), ("rccl-carry", 256), ("rccl-early", 32),
                                    ("rccl-side", 32), ("rccl-zero", 256)])
def test_structures_with_a_schedule_match_local(gpu, name, B):
    """Each multi-GPU step structure through a forced 1-rank communicator, the schedule on, over
    two epochs of graph replays with the ragged tail: the local chain's weights, momentum, bf16
    W1 / W1^T and rate word bit for bit.  Every consumer of step k's rate -- the optimizer
    launches, the carried fc1 update in step k + 1's forward, the fc update deferred past it or
    on the side stream, the sharded update -- runs between head k and head k + 1
    (docs/kernels.md "Device-resident learning-rate schedule")."""
    want = _local(gpu, B)
    got = _structure_run(gpu, B, name)
    for i, (a, b) in enumerate(zip(want, got)):
        assert torch.equal(a, b), (name, i)


# ---------------------------------------------------------------------------- CLI
def test_cnn_fp32_cli_gpu_matches_cpu_with_a_schedule(gpu, tmp_path, monkeypatch):
    """tests/test_gpu_dropout.py's GPU-vs-CPU CLI comparison with --lr-schedule cosine
    --lr-warmup 4, at that test's tolerances for the exact fp32 products (loss 5e-5, accuracy
    0.1, both epochs): both paths read the same table, and their checkpoints hold its entry of
    the epoch's last step.  2000 samples (7 full batches and a tail of 208): one sample is 0.05
    points of accuracy, so a near-tie row that the two devices classify differently stays
    inside the accuracy tolerance instead of sitting exactly on it."""
    monkeypatch.setenv("PDM_F32_CONV", "exact")
    d1, d2 = tmp_path / "gpu", tmp_path / "cpu"
    d1.mkdir()
    d2.mkdir()
    common = ["--arch", "cnn", "--optimizer", "sgd", "--lr", "0.05", "--dtype", "fp32",
              "--synthetic-size", "2000", "--epochs", "2", "--seed", "4",
              "--lr-schedule", "cosine", "--lr-warmup", "4"]
    g = [l for l in cli(common, d1) if l.startswith("Epoch:")]
    c = [l for l in cli(common, d2, device="cpu", backend="gloo") if l.startswith("Epoch:")]
    assert len(g) == len(c) == 2
    for lg, lc in zip(g, c):
        print(lg, "|", lc)
        mg, mc = EPOCH_RE.match(lg), EPOCH_RE.match(lc)
        for i in (3, 5):
            assert abs(float(mg.group(i)) - float(mc.group(i))) < 5e-5, (lg, lc)
        for i in (4, 6):
            assert abs(float(mg.group(i)) - float(mc.group(i))) <= 0.1, (lg, lc)
    table = ScheduleSpec("cosine", 0.05, 2, 8, warmup=4).table()           # 2000 / 256: 7 + a tail
    for d in (d1, d2):
        for e in range(2):
            ck = torch.load(d / "checkpoints" / f"checkpoint_{e}.pth.tar", weights_only=True)
            assert ck["optimizer"]["param_groups"][0]["lr"] == table[(e + 1) * 8 - 1], (d, e)
