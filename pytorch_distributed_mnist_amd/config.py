"""Command-line surface.

Every reference flag is kept with its default (reference
``multi_proc_single_gpu.py:289-334``).  ``--local_rank`` also
accepts the ``--local-rank`` spelling torch>=2's launcher passes.

Additions are opt-in and default to the reference's behaviour:
``--arch {linear,cnn}``, ``--optimizer {adam,sgd}`` (sgd finally consumes
``--momentum``/``--wd`` as the commented-out reference code would,
:192-194), ``--dtype {fp32,bf16}``, ``--synthetic``/``--synthetic-size``,
``--device``, ``--no-graphs``, ``--checkpoint-dir``, ``--timeout``, ``--perf``,
``--rank-prefix``, ``--predict-out`` (with ``--evaluate``) and the train-time augmentation
``--aug-shift`` / ``--aug-rotate`` / ``--aug-zoom`` / ``--aug-elastic`` / ``--aug-seed``,
dropout on the CNN's hidden layer, ``--dropout`` / ``--dropout-seed``, the per-step learning-rate schedule
``--lr-schedule`` / ``--lr-warmup`` / ``--lr-min``, label smoothing of the training loss,
``--label-smoothing``, mixup, ``--mixup`` / ``--mixup-seed``, the exponential moving average of the weights, ``--ema-decay`` /
``--ema-warmup``, and test-time augmentation, ``--tta``.
"""
from __future__ import annotations

import argparse
import sys


class _LocalRankAction(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, int(values))
        setattr(namespace, "local_rank_given", True)


def _ranged(kind, lo, hi):
    """argparse type: a `kind` (int or float) in [lo, hi]; anything else is a usage error."""
    def parse(text):
        try:
            v = kind(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"invalid {kind.__name__} value: {text!r}")
        if not lo <= v <= hi:                        # (also rejects nan)
            raise argparse.ArgumentTypeError(f"{text} is outside {lo}..{hi}")
        return v
    return parse


def _ema_decay(text):
    """argparse type of --ema-decay: 0 (off) or a float in the open interval (0, 1)."""
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"invalid float value: {text!r}")
    if not 0.0 <= v < 1.0:                           # (also rejects nan)
        raise argparse.ArgumentTypeError(f"{text} is outside 0 < D < 1 (0 = off)")
    return v


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        description="MI355X-native distributed MNIST training (DDP over RCCL/xGMI)")
    parser.add_argument('--root', type=str, default='data')
    parser.add_argument('-j', '--workers', default=4, type=int, metavar='N',
                        help='number of data loading workers (default: 4); kept for CLI '
                             'parity — data is device-resident, no worker processes run')
    parser.add_argument('--epochs', type=int, default=20)
    parser.add_argument('--start-epoch', default=0, type=int, metavar='N',
                        help='manual epoch number (useful on restarts)')
    parser.add_argument('--batch-size', type=int, default=256,
                        help='mini-batch size(default: 256), this is the total batch size of '
                             'all GPUs on the current node when use Distributed Data Parallel')
    parser.add_argument('--lr', '--learning-rate', default=1e-3, type=float,
                        metavar='LR', help='initial learning rate', dest='lr')
    parser.add_argument('--momentum', default=0.9, type=float, metavar='M', help='momentum')
    parser.add_argument('--wd', '--weight-decay', default=1e-4, type=float,
                        metavar='W', help='weight decay (default: 1e-4)', dest='weight_decay')
    parser.add_argument('--resume', default='', type=str, metavar='PATH',
                        help='path to latest checkpoint (default: none)')
    parser.add_argument('-e', '--evaluate', dest='evaluate', action='store_true',
                        help='evaluate model on validation set')
    parser.add_argument('--backend', type=str, default='nccl',
                        help='Name of the backend to use (nccl = RCCL on ROCm, or gloo).')
    parser.add_argument('--local_rank', '--local-rank', type=int, default=0, dest='local_rank',
                        action=_LocalRankAction)
    parser.add_argument('-i', '--init-method', type=str, default='tcp://127.0.0.1:23456',
                        help='URL specifying how to initialize the package.')
    parser.add_argument('-s', '--world-size', type=int, default=1,
                        help='Number of processes participating in the job.')
    parser.add_argument('-r', '--rank', type=int, default=0, help='Rank of the current process.')
    parser.add_argument('--seed', default=None, type=int,
                        help='seed for initializing training (applied inside every rank).')
    # ---- additions (opt-in; defaults reproduce the reference) ----
    g = parser.add_argument_group("MI355X framework options")
    g.add_argument('--arch', choices=['linear', 'cnn'], default='linear',
                   help="linear = reference Net (Linear 784->10); cnn = north-star CNN")
    g.add_argument('--optimizer', choices=['adam', 'sgd'], default='adam')
    g.add_argument('--dtype', choices=['auto', 'fp32', 'bf16'], default='auto',
                   help='compute dtype of activations / GEMM inputs (master weights stay fp32); '
                        'auto = bf16 for the CNN on GPU, fp32 otherwise (the reference Linear '
                        'model and every CPU run)')
    g.add_argument('--synthetic', action='store_true',
                   help='use deterministic synthetic MNIST-shaped data even if MNIST is on disk')
    g.add_argument('--synthetic-size', type=int, default=None,
                   help='number of synthetic training samples (default 60000)')
    g.add_argument('--device', choices=['auto', 'cuda', 'cpu'], default='auto')
    g.add_argument('--no-graphs', dest='graphs', action='store_false',
                   help='launch kernels eagerly instead of replaying captured hipGraphs')
    g.add_argument('--comm', choices=['auto', 'xgmi', 'rccl'], default=None,
                   help='gradient all-reduce transport on GPU with --backend nccl: xgmi = direct '
                        'peer-to-peer pushes over xGMI (hipIpc), rccl = ncclAllReduce; auto '
                        '(default, or $PDM_COMM) = xgmi when every rank passes its self-check')
    g.add_argument('--shard-fc', action='store_true',
                   help='bf16 CNN, world size > 1 over rccl (or gloo): shard the fc1 weight\'s '
                        'optimizer update over the ranks (reduce-scatter of its gradient, each '
                        'rank updates 128 / world_size rows, all-gather of the bf16 rows); '
                        'checkpoints gather the full state first and keep the reference format')
    g.add_argument('--structure-check', choices=['auto', 'on', 'off'], default='auto',
                   help='world size > 1: before the first epoch, run a few steps of each step '
                        'structure in preference order and keep the first that passes on every '
                        'rank, restoring the training state afterwards (auto: on the GPU when '
                        'there is a fallback structure; on: also with a single structure, e.g. '
                        'on CPU/gloo, where the fallback is the same reducer rebuilt)')
    g.add_argument('--checkpoint-dir', default='checkpoints')
    g.add_argument('--timeout', type=float, default=1800.0,
                   help='deadline in seconds for the rendezvous, RCCL communicator init and every '
                        'host sync on the device (a missing peer raises instead of hanging)')
    g.add_argument('--perf', action='store_true',
                   help='print an extra per-epoch throughput line on rank 0')
    g.add_argument('--trace', action='store_true',
                   help='emit roctx ranges (epoch/train/evaluate/checkpoint) for rocprofv3 '
                        '--marker-trace')
    g.add_argument('--rank-prefix', action='store_true',
                   help="prefix every per-rank line with '[rank r] '")
    # (no default: the attribute exists only when the flag is given, so the Namespace line the
    # app prints is unchanged without it)
    g.add_argument('--predict-out', metavar='PATH', default=argparse.SUPPRESS,
                   help='with --evaluate: after the test line, rank 0 writes PATH, a NumPy .npz '
                        'with per-sample log_probs [N, 10], pred [N], labels [N] and the confusion '
                        'matrix [10, 10] of the test set, and prints one accuracy line per class')
    # train-time augmentation (data/augment.py; no defaults either, for the same reason)
    g.add_argument('--aug-shift', metavar='N', type=_ranged(int, 0, 8), default=argparse.SUPPRESS,
                   help='train-time augmentation: random shift of up to N pixels (0..8) per '
                        'sample and epoch, applied while the epoch is gathered')
    g.add_argument('--aug-rotate', metavar='DEG', type=_ranged(float, 0.0, 45.0),
                   default=argparse.SUPPRESS,
                   help='train-time augmentation: random rotation of up to DEG degrees (0..45)')
    g.add_argument('--aug-zoom', metavar='F', type=_ranged(float, 0.0, 0.5),
                   default=argparse.SUPPRESS,
                   help='train-time augmentation: random zoom by a factor in 1 -/+ F (0..0.5)')
    g.add_argument('--aug-elastic', metavar='A', type=_ranged(float, 0.0, 3.0),
                   default=argparse.SUPPRESS,
                   help='train-time augmentation: elastic distortion, a smooth random '
                        'displacement field per sample and epoch whose control points move by '
                        'up to A pixels (0..3)')
    g.add_argument('--aug-seed', metavar='N', type=_ranged(int, 0, 2 ** 64 - 1),
                   default=argparse.SUPPRESS,
                   help='seed of the augmentation draws (default: --seed if given, else 0); a '
                        "sample's transform depends on (seed, epoch, dataset index) only. Like "
                        '--lr, the --aug-* flags are given again on --resume; --evaluate ignores '
                        'them unless --tta asks for views')
    # dropout on the CNN's hidden units (data/dropout.py; no defaults, as above: absent = 0 = off)
    g.add_argument('--dropout', metavar='P', type=_ranged(float, 0.0, 0.9),
                   default=argparse.SUPPRESS,
                   help='--arch cnn: drop each of the 128 hidden units in front of fc2 with '
                        'probability P (0..0.9, default 0 = off) in training steps, kept units '
                        'scaled by 1 / (1 - P); evaluation never drops')
    g.add_argument('--dropout-seed', metavar='N', type=_ranged(int, 0, 2 ** 64 - 1),
                   default=argparse.SUPPRESS,
                   help='seed of the dropout draws (default: --seed if given, else 0); a unit\'s '
                        'draw depends on (seed, epoch, dataset index, unit) only. Like --lr, '
                        '--dropout is given again on --resume; --evaluate ignores it')
    # per-step learning-rate schedule (optim/schedule.py; no defaults, as above: absent = the
    # reference's per-epoch step decay, set by the host)
    g.add_argument('--lr-schedule', choices=['step', 'constant', 'linear', 'cosine'],
                   default=argparse.SUPPRESS,
                   help='learning rate per optimizer step: step (default) = the reference\'s '
                        'decay by 10 every 10 epochs, constant = --lr, linear / cosine = an '
                        'anneal from --lr to --lr-min * --lr over the run\'s steps (--epochs x '
                        'steps per epoch, counted from epoch 0). Like --lr, the --lr-* flags are '
                        'given again on --resume; --evaluate ignores them')
    g.add_argument('--lr-warmup', metavar='N', type=_ranged(int, 0, 2 ** 31 - 1),
                   default=argparse.SUPPRESS,
                   help='the first N optimizer steps of the run ramp linearly up to the '
                        'scheduled rate (default 0; fewer than the run\'s steps)')
    g.add_argument('--lr-min', metavar='F', type=_ranged(float, 0.0, 1.0),
                   default=argparse.SUPPRESS,
                   help='--lr-schedule linear / cosine: the final learning rate as a fraction '
                        'of --lr (0..1, default 0)')
    # label smoothing of the training heads (no default, as above: absent = 0 = off)
    g.add_argument('--label-smoothing', metavar='E', type=_ranged(float, 0.0, 1.0),
                   default=argparse.SUPPRESS,
                   help='training steps use the targets (1 - E) * onehot + E / 10 (0..1, default '
                        '0 = off), as torch\'s cross_entropy(label_smoothing=E); the printed train '
                        'loss is the smoothed loss, the test loss stays the plain NLL. Like --lr, '
                        'it is given again on --resume; --evaluate ignores it')
    # mixup (data/mixup.py; no defaults, as above: absent = 0 = off)
    g.add_argument('--mixup', metavar='A', type=_ranged(float, 0.0, 10.0),
                   default=argparse.SUPPRESS,
                   help='--arch cnn: mixup (Zhang et al. 2018) in training steps: every sample is '
                        'blended with a partner drawn from the whole training set, image and '
                        'target alike, with weight lambda ~ Beta(A, A) folded to >= 1/2 (0 < A '
                        '<= 10, default 0 = off); the printed train loss is the mixed loss, '
                        'train acc counts the primary sample\'s label; evaluation is never mixed')
    g.add_argument('--mixup-seed', metavar='N', type=_ranged(int, 0, 2 ** 64 - 1),
                   default=argparse.SUPPRESS,
                   help='seed of the mixup draws (default: --seed if given, else 0); a sample\'s '
                        'partner and weight depend on (seed, epoch, dataset index) only. Like '
                        '--lr, --mixup is given again on --resume; --evaluate ignores it')
    # exponential moving average of the weights (optim/ema.py; no defaults, as above: absent = off)
    g.add_argument('--ema-decay', metavar='D', type=_ema_decay, default=argparse.SUPPRESS,
                   help='keep an exponential moving average of the weights, e += (1 - D) (p - e) '
                        'after every optimizer step (0 < D < 1; default 0 = off): each epoch\'s '
                        'test line, the model_best choice and the checkpoint\'s ema_state_dict '
                        'come from it, training is unchanged. Like --lr, it is given again on '
                        '--resume; with --evaluate it selects the checkpoint\'s averaged weights')
    g.add_argument('--ema-warmup', action='store_true', default=argparse.SUPPRESS,
                   help='with --ema-decay: the k-th update uses min(D, (1 + k) / (10 + k)), so '
                        'the early average follows the weights')
    # test-time augmentation (no default, as above: absent = 1 = off)
    g.add_argument('--tta', metavar='V', type=_ranged(int, 1, 32), default=argparse.SUPPRESS,
                   help='test-time augmentation: every test pass of the run (each epoch\'s test '
                        'line and so the model_best choice, --evaluate, --predict-out) classifies '
                        'each image together with V - 1 views of it distorted within the --aug-* '
                        'ranges and reports the log of the mean probability (1..32, default 1 = '
                        'off; V > 1 needs an --aug-* range). Training is unchanged. Like --lr, it '
                        'is given again on --resume and --evaluate, which then reads the --aug-* '
                        'flags as the ranges of the views')
    parser.set_defaults(local_rank_given=False)
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(sys.argv[1:] if argv is None else argv)
    if hasattr(args, "predict_out") and not args.evaluate:
        parser.error("--predict-out is only valid with --evaluate (it writes the predictions of "
                     "the evaluation pass)")
    if getattr(args, "dropout", 0.0) > 0.0 and args.arch == "linear":
        parser.error("argument --dropout: --arch linear has no hidden layer to drop "
                     "(use --arch cnn)")
    if getattr(args, "mixup", 0.0) > 0.0 and args.arch == "linear":
        parser.error("argument --mixup: only the CNN's training head mixes targets "
                     "(use --arch cnn)")
    if hasattr(args, "lr_min") and getattr(args, "lr_schedule", "step") in ("step", "constant"):
        parser.error("argument --lr-min: --lr-schedule {} has no final rate (use --lr-schedule "
                     "linear or cosine)".format(getattr(args, "lr_schedule", "step")))
    if getattr(args, "tta", 1) > 1 and not (getattr(args, "aug_shift", 0) > 0 or
                                            getattr(args, "aug_rotate", 0.0) > 0.0 or
                                            getattr(args, "aug_zoom", 0.0) > 0.0 or
                                            getattr(args, "aug_elastic", 0.0) > 0.0):
        parser.error("argument --tta: {} views need a range to be drawn from (give --aug-shift, "
                     "--aug-rotate, --aug-zoom or --aug-elastic): without one every view is the "
                     "same image".format(args.tta))
    if hasattr(args, "ema_warmup") and not getattr(args, "ema_decay", 0.0):
        parser.error("argument --ema-warmup: there is no average to warm up (give --ema-decay D)")
    return args


def usage_error(message: str) -> None:
    """Exit as argparse does for a bad flag (usage, ``error: message``, status 2): for flags
    that can only be checked once the run's geometry is known (--lr-warmup against the run's
    steps)."""
    build_parser().error(message)
