"""Per-rank job driver and process launch (reference ``run``/``main``).

Mirrors reference ``multi_proc_single_gpu.py:163-359``: process-group init,
per-rank batch split, model + DDP-style parameter broadcast, optimizer, resume,
device-resident loaders, the epoch loop (set_epoch -> adjust_lr -> train ->
evaluate -> print -> rank-0 checkpoint), and spawn / launch entrypoints.

Deliberate, output-format-invisible fixes: launch mode is
auto-detected (no source edit), ``--local-rank`` is accepted, the device is
selected with set_device, ``--seed`` is applied inside every rank, the
``world_size == device_count`` assert is relaxed to ``world_size <=
device_count`` and skipped for CPU/gloo, checkpoints are written atomically,
metrics are read once per epoch, and the process group is torn down on exit.
"""
from __future__ import annotations

import os
import random
import warnings

import torch

from . import parallel
from .config import parse_args, usage_error
from .data import sampler
from .data.augment import spec_from_args
from .data.dropout import spec_from_args as dropout_from_args
from .data.mixup import spec_from_args as mixup_from_args
from .data.mnist import load_split
from .engine import Trainer
from .models.reference import MODULES
from .models.specs import get_spec
from .optim.flat import adjust_learning_rate, build_optimizer
from .optim.ema import WeightEma, spec_from_args as ema_from_args
from .optim.schedule import spec_from_args as schedule_from_args
from .runtime.arena import FlatArena
from .runtime.program import TrainProgram
from .utils import trace
from .utils.checkpoint import load_checkpoint, make_state, save_checkpoint

best_acc = 0


def _printer(rank, prefix):
    """print() semantics (space-joined args), but each line reaches stdout in ONE write, so
    the lines of concurrently printing ranks never interleave mid-line."""
    import sys

    def p(*a, sep=" ", end="\n"):
        line = sep.join(str(x) for x in a)
        if prefix:
            line = "[rank {}] ".format(rank) + line
        sys.stdout.write(line + end)
        sys.stdout.flush()
    return p


def resolve_dtype(dtype: str, arch: str, device: torch.device) -> str:
    """--dtype auto: bf16 for the CNN on GPU (its HIP kernels), fp32 otherwise."""
    if dtype != "auto":
        return dtype
    return "bf16" if (arch == "cnn" and device.type == "cuda") else "fp32"


def _seed_everything(seed: int) -> None:
    random.seed(seed)
    torch.manual_seed(seed)


def build_rank_state(args, rank: int, world_size: int, local_rank: int, init_pg: bool = True):
    """Everything one rank needs before its epoch loop (shared by app, bench and tests)."""
    device = parallel.pick_device(local_rank, args.device)
    if device.type == "cuda" and args.backend == "nccl":
        ngpus = torch.cuda.device_count()
        if world_size > ngpus:
            raise RuntimeError(f"--world-size {world_size} needs one GPU per rank, "
                               f"but only {ngpus} are visible")
    init_method = args.init_method
    if "MASTER_ADDR" in os.environ and getattr(args, "_launched", False) and \
            not getattr(args, "_init_method_explicit", False):
        init_method = "env://"
    elif getattr(args, "_launched", False) and init_method.startswith("tcp://") and \
            os.environ.get("TORCHELASTIC_USE_AGENT_STORE", "").lower() == "true":
        # torchrun workers connect to the agent's store as clients for ANY tcp:// init
        # method; an explicit -i naming another endpoint must be hosted by rank 0 instead
        # (the reference's launch-mode semantics), or every rank would wait for a server.
        hostport = init_method[len("tcp://"):].split("?")[0]
        master = "{}:{}".format(os.environ.get("MASTER_ADDR"), os.environ.get("MASTER_PORT"))
        if hostport != master:
            os.environ["TORCHELASTIC_USE_AGENT_STORE"] = "False"
    ctx = parallel.init_distributed(args.backend, init_method, world_size, rank, local_rank, device,
                                    timeout_s=args.timeout, init_pg=init_pg)
    return ctx


def structure_candidates(args, program, comm, world_size):
    """[(name, apply, abortable)] in preference order for the start-up check
    (parallel/startup.py); empty when there is nothing to choose or the check is off.
    GPU with the direct xGMI transport: xgmi (conv bucket exchanged in the optimizer launch),
    xgmi-noxchg (the exchange off), rccl-nocarry (plain RCCL collectives, built on demand).
    abortable: a host deadline may abort the RCCL communicator (the xgmi kernels' waits are
    bounded on the device: they end by themselves and report through the error word)."""
    mode = getattr(args, "structure_check", "auto")
    if mode == "off" or world_size < 2:
        return []
    red = program.reducer
    spec = program.arena.spec
    made = {}

    def rebuilt(transport, **kw):
        def apply():
            if transport not in made:
                made[transport] = parallel.GradReducer(comm, program.arena.grads,
                                                       spec.bucket_bounds(), transport=transport,
                                                       channels=spec.channel_bounds())
            program.use_structure(made[transport], **kw)
        return apply

    cands = []
    if red.kind == "xgmi":
        cands.append(("xgmi", lambda: program.use_structure(red, xgmi_exchange=True), False))
        if program.gpu is not None and hasattr(program.gpu, "xgmi_exchange") and \
                program.structure.xgmi_exchange and red.exchange_ok(1):
            cands.append(("xgmi-noxchg",
                          lambda: program.use_structure(red, xgmi_exchange=False), False))
        if isinstance(comm, parallel.RcclComm):
            # (with the weight average on, the only RCCL mode offered: CnnStep.rccl_mode_offered)
            cands.append(("rccl-nocarry", rebuilt("rccl", rccl_mode="nocarry"), True))
        elif mode == "on":
            # the one-GPU rehearsal (xgmi over a gloo control plane): the gloo reducer
            cands.append(("torch", rebuilt(None), True))
    elif mode == "on":
        # one structure: the check still runs when asked (the protocol's CPU / gloo
        # rehearsal), with the same reducer rebuilt as the fallback
        cands.append((red.kind, lambda: program.use_structure(red), True))
        cands.append((f"{red.kind}-rebuilt", rebuilt(red.kind if red.kind != "torch" else None),
                      True))
    return cands if len(cands) > 1 else []


def run(args):
    global best_acc
    launched = getattr(args, "_launched", False)
    rank = args.rank
    world_size = args.world_size
    local_rank = args.local_rank if launched else rank
    ctx = build_rank_state(args, rank, world_size, local_rank)
    device = ctx.device
    out = _printer(rank, args.rank_prefix)
    if getattr(args, "trace", False):
        trace.enable(True)

    # Reference splits the node batch by the GPU count (:170-175); the GPU count
    # equals world_size under its assert, and world_size is what we divide by.
    ngpus = world_size
    args.batch_size = int(args.batch_size / ngpus)
    args.workers = int((args.workers + ngpus - 1) / ngpus)
    dev_count = torch.cuda.device_count() if device.type == "cuda" else ngpus
    out("rank: {}, device count: {}, workers:{}".format(rank, dev_count, args.workers))

    if args.seed is not None:
        _seed_everything(args.seed)

    # Model: torch default init on this rank, then rank 0's weights are
    # broadcast (DDP construction semantics).
    spec = get_spec(args.arch)
    arena = FlatArena(spec, device)
    arena.load_module(MODULES[args.arch]())
    # DDP construction: every rank must hold the same model before rank 0's weights are
    # broadcast (reference :188-189, DDP's _verify_param_shape_across_processes)
    parallel.verify_params_across_ranks(spec, rank, world_size)
    comm = parallel.make_comm(ctx)
    comm.broadcast_(arena.params, 0)

    optimizer = build_optimizer(args.optimizer, arena, args)

    # exponential moving average of the weights (--ema-decay / --ema-warmup, optim/ema.py):
    # every rank's own copy, started at the broadcast weights.  With --evaluate the flag only
    # selects which of the checkpoint's weights are evaluated, and nothing is averaged.
    ema_spec = ema_from_args(args)
    ema = None if ema_spec is None or args.evaluate else WeightEma(ema_spec, arena)

    if args.resume:
        if os.path.isfile(args.resume):
            out("=> loading checkpoint '{}'".format(args.resume))
            checkpoint = load_checkpoint(args.resume, map_location="cpu")
            args.start_epoch = checkpoint['epoch']
            best_acc = checkpoint['best_acc']
            out("best_acc: {}".format(best_acc))
            if ema_spec is not None and args.evaluate:
                if 'ema_state_dict' not in checkpoint:
                    raise SystemExit("error: --evaluate --ema-decay: checkpoint '{}' holds no "
                                     "averaged weights (no ema_state_dict); evaluate it without "
                                     "--ema-decay".format(args.resume))
                arena.load_state_dict(checkpoint['ema_state_dict'])
            else:
                arena.load_state_dict(checkpoint['state_dict'])
            optimizer.load_state_dict(checkpoint['optimizer'])
            if ema is not None and 'ema_state_dict' in checkpoint:
                ema.load_state_dict(checkpoint['ema_state_dict'], checkpoint['ema_updates'])
            elif ema is not None:
                ema.reset(arena)
                out("notice: checkpoint '{}' holds no averaged weights: the average starts at "
                    "its weights".format(args.resume))
            out("=> loaded checkpoint '{}' (epoch {})".format(args.resume, checkpoint['epoch']))
        else:
            out("=> no checkpoint found at '{}'".format(args.resume))

    train_split = load_split(args.root, True, synthetic=args.synthetic,
                             synthetic_size=args.synthetic_size)
    test_split = load_split(args.root, False, synthetic=args.synthetic)
    reducer = parallel.GradReducer(comm, arena.grads, spec.bucket_bounds(),
                                   transport=getattr(args, "comm", None),
                                   channels=spec.channel_bounds())
    dtype = resolve_dtype(args.dtype, args.arch, device)
    reducer0 = reducer
    # train-time augmentation (--aug-*): training epochs only; --evaluate ignores the flags
    augment = None if args.evaluate else spec_from_args(args)
    # test-time augmentation (--tta V): every test pass classifies V views per image, drawn with
    # the --aug-* ranges and --aug-seed -- the one place where --evaluate reads those flags (as
    # the ranges of the views only: nothing trains there)
    tta = getattr(args, "tta", 1)
    tta_augment = spec_from_args(args) if tta > 1 else None
    if tta > 1 and rank == 0:
        out("notice: test-time augmentation: every test pass averages {} views per image "
            "(the image and {} drawn within the --aug-* ranges)".format(tta, tta - 1))
    # dropout on the CNN's hidden units (--dropout): likewise
    dropout = None if args.evaluate else dropout_from_args(args)
    # mixup (--mixup): likewise
    mixup = None if args.evaluate else mixup_from_args(args)
    # per-step learning-rate schedule (--lr-schedule / --lr-warmup / --lr-min): likewise; None
    # with the defaults, and then the host's per-epoch adjust_learning_rate below is all there is
    schedule = None
    if not args.evaluate:
        spe = -(-sampler.num_samples_per_rank(len(train_split), world_size) // args.batch_size)
        try:
            schedule = schedule_from_args(args, spe)
        except ValueError as e:
            usage_error(str(e))
    # label smoothing of the training loss (--label-smoothing): likewise
    smoothing = 0.0 if args.evaluate else getattr(args, "label_smoothing", 0.0)
    program = TrainProgram(args.arch, dtype, arena, optimizer, reducer, train_split, test_split,
                           args.batch_size, use_graphs=args.graphs, augment=augment,
                           dropout=dropout, schedule=schedule, label_smoothing=smoothing,
                           ema=ema, mixup=mixup, tta=tta, tta_augment=tta_augment)
    if device.type == "cuda":
        # every host sync of the epoch loop waits at most --timeout for the device (and the
        # collectives it is queued behind), then aborts the communicator and raises
        program.sync_fn = lambda what: parallel.bounded_sync(device, args.timeout, comm, what)
    if getattr(args, "shard_fc", False) and world_size > 1:
        why = program.shard_unsupported_reason()
        if why is None:
            program.set_shard_fc(True)
        elif rank == 0:
            out("warning: --shard-fc: {}; running unsharded".format(why))
    trainer = Trainer(program)

    try:
        if not args.evaluate:
            cands = structure_candidates(args, program, comm, world_size)
            if cands:
                from .parallel.startup import check_structures
                idx = sampler.distributed_indices(len(train_split), world_size, rank,
                                                  args.start_epoch)
                if program.gpu is not None:
                    idx = idx.to(torch.int32)

                def check_sync(what, abortable):
                    if device.type == "cuda":
                        parallel.bounded_sync(device, args.timeout, comm, what, abort=abortable)
                check_structures(program, cands, idx, rank, world_size, check_sync,
                                 epoch=args.start_epoch)
        reducer = program.reducer          # (the start-up check may have switched it)
        if args.evaluate:
            test_loss, test_acc = trainer.evaluate()
            out('test loss: {}, test acc: {}.'.format(test_loss, test_acc))
            predict_out = getattr(args, "predict_out", None)
            if predict_out:
                # every rank runs the (unsharded) pass, as it runs the evaluation; rank 0 writes
                # the file and prints the per-class lines
                from .predict import class_lines, save_predictions
                pred = program.predict()
                if rank == 0:
                    save_predictions(predict_out, pred, test_split.labels)
                    for line in class_lines(pred.confusion):
                        out(line)
            return

        # epoch e+1's sample order is computed on a host thread while epoch e trains
        prefetch = sampler.EpochIndexPrefetcher(len(train_split), world_size, rank,
                                                int32=program.gpu is not None)
        for epoch in range(args.start_epoch, args.epochs):
            with trace.range("epoch {}".format(epoch)):
                if schedule is None:    # (else the program sets every step's rate)
                    adjust_learning_rate(optimizer, epoch, args)

                nxt = prefetch.peek(epoch + 1) if program.gpu is not None and \
                    epoch + 1 < args.epochs else None
                train_loss, train_acc = trainer.train(prefetch.get(epoch), nxt, epoch)
                reducer.check()             # xgmi: raise if a peer never arrived
                test_loss, test_acc = trainer.evaluate()

                out('Epoch: {}/{},'.format(epoch, args.epochs),
                    'train loss: {}, train acc: {},'.format(train_loss, train_acc),
                    'test loss: {}, test acc: {}.'.format(test_loss, test_acc))
                if args.perf:
                    # node images/sec over the slowest rank's train time (BASELINE.md
                    # protocol); every rank joins the max (control plane, gloo)
                    t_train = trainer.last_train_seconds
                    if world_size > 1 and parallel.distributed_is_initialized():
                        t = torch.tensor([t_train], dtype=torch.float64)
                        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
                        t_train = float(t.item())
                    if rank == 0:
                        n = train_loss.count * world_size
                        out("perf: epoch {} train {:.1f} img/s (node, {} samples in {:.4f}s on the "
                            "slowest rank), eval {:.4f}s".format(
                                epoch, n / max(t_train, 1e-12), n, t_train,
                                trainer.last_eval_seconds))

                is_best = test_acc.accuracy > best_acc
                best_acc = max(test_acc.accuracy, best_acc)
                program.sync_master()       # sharded state: every rank gathers the full state
                if rank == 0:
                    with trace.range("checkpoint"):
                        save_checkpoint(make_state(epoch + 1, arena, best_acc, optimizer, ema),
                                        is_best, epoch, directory=args.checkpoint_dir)
    finally:
        if 'prefetch' in locals():
            prefetch.close()
        if device.type == "cuda":
            import sys
            pending = sys.exc_info()[1] is not None
            try:
                parallel.bounded_sync(device, args.timeout, comm, "teardown")
            except RuntimeError:
                if not pending:       # do not mask the error that is already propagating
                    raise
        program.reducer.close()
        if program.reducer is not reducer0:
            reducer0.close()
        comm.close()
        parallel.shutdown()


def run_spawn(proc_id, args):
    """Spawn entry: rank = process index (reference :273-276)."""
    args.rank = proc_id
    args._launched = False
    run(args)


def run_dist_launch(args):
    """Launcher entry: rank from the launcher (reference :278-281, env-aware)."""
    rank, ws, local_rank = parallel.launched_rank(args)
    args.rank, args.world_size, args.local_rank = rank, ws, local_rank
    args._launched = True
    run(args)


def main(argv=None):
    args = parse_args(argv)
    argv_list = list(argv) if argv is not None else None
    import sys
    raw = argv_list if argv_list is not None else sys.argv[1:]
    print(args)
    args._init_method_explicit = any(a in ("-i", "--init-method") or a.startswith("--init-method=")
                                     for a in raw)
    if args.seed is not None:
        warnings.warn('You have chosen to seed training. The seed is applied inside every rank '
                      'before model initialisation.')
    if parallel.is_launched(args):
        run_dist_launch(args)
        return
    if args.world_size == 1:
        run_spawn(0, args)      # one rank: run in-process (no extra interpreter)
    else:
        parallel.spawn(run_spawn, args.world_size, args)
