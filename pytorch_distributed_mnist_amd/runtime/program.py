"""Per-rank training program: device-resident data + step kernels + graphs.

What replaces the reference's DataLoader/Trainer machinery
(``multi_proc_single_gpu.py:77-161``):

* the uint8 train/test sets are uploaded to the device once (47 + 8 MB);
* each epoch the rank's DistributedSampler-identical index vector is uploaded
  (int32, <=240 KB) and a device step counter is reset;
* a train step is a fixed chain of HIP kernels that read the batch indices via
  that counter, so the step has no host inputs at all and is captured once per
  batch size into a hipGraph (``torch.cuda.CUDAGraph`` on ROCm) — the
  full-batch graph and the ragged-tail graph;
* loss/accuracy accumulate on the device; the host reads them once per epoch.

On the CPU (gloo path) the same program runs the torch reference step.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from ..data.augment import AugmentSpec, augment_batch, check_tta, tta_view
from ..data.dropout import DropoutSpec
from ..data.mixup import MixupSpec, mix_batch
from ..data.mnist import image_rows, label_vector
from ..data.sampler import batch_bounds
from ..optim.ema import EmaSpec, WeightEma
from ..optim.schedule import ScheduleSpec
from ..utils.metrics import DeviceMetrics
from .cpu_step import eval_step_cpu, predict_step_cpu, train_step_cpu, tta_reduce_cpu
from .structure import StepStructure


# rows per CPU forward of predict(): a constant, not the program's batch size, so that the same
# weights give the same bits whichever program (trainer or load_predictor) holds them
PREDICT_BATCH_CPU = 256


@dataclass
class Prediction:
    """What ``TrainProgram.predict`` returns, on the host: log_probs fp32 [N, 10] (log-softmax
    of the logits), pred int64 [N] (argmax, first maximum) and, with labels, confusion int64
    [10, 10] (confusion[y][p] = rows of class y predicted as p), else None."""
    log_probs: torch.Tensor
    pred: torch.Tensor
    confusion: Optional[torch.Tensor]


class TrainProgram:
    def __init__(self, model: str, dtype: str, arena, optimizer, reducer, train_split, test_split,
                 batch_size: int, eval_batch: Optional[int] = None, use_graphs: bool = True,
                 structure: Optional[StepStructure] = None,
                 augment: Optional[AugmentSpec] = None,
                 dropout: Optional[DropoutSpec] = None,
                 schedule: Optional[ScheduleSpec] = None, label_smoothing: float = 0.0,
                 ema: Optional[WeightEma] = None, mixup: Optional[MixupSpec] = None,
                 tta: int = 1, tta_augment: Optional[AugmentSpec] = None):
        self.model = model
        # test-time augmentation (--tta V): evaluate() and predict() classify every image
        # together with V - 1 distorted views of it and combine the V log-softmax rows into the
        # log of the mean probability (docs/kernels.md "Test-time augmentation").  The views'
        # ranges are `tta_augment` (None: `augment`, the training ranges).  1: off, and both
        # run exactly what they run without it.  Training never sees any of this.
        self.set_tta(tta, tta_augment if tta_augment is not None else augment)
        # mixup (data/mixup.py): training steps only -- every sample is blended with a partner
        # of the whole training set, on the GPU inside the epoch gather (image) and the head
        # kernel (target), on the CPU per batch.  None or alpha = 0: off, and nothing changes.
        self.mixup = mixup if mixup is not None and mixup.enabled else None
        if self.mixup is not None and model != "cnn":
            raise ValueError(f"mixup is built into the CNN's training head: the {model} model "
                             "has no such head")
        self._mix_table = self.mixup.table() if self.mixup is not None else None
        # exponential moving average of the weights (optim/ema.py): a second flat buffer that
        # takes in every step's whole weights after the step's update -- on the GPU the last
        # launch of the step, inside the graphs, on the CPU after optimizer.step().  Training
        # never reads it; evaluate() and predict() use it by default when it is on.  None: off,
        # and nothing changes.
        self.ema = ema
        # label smoothing (--label-smoothing E in 0..1): the training steps' targets are
        # (1 - E) onehot + E / 10, as torch's F.cross_entropy(..., label_smoothing=E) -- on the
        # GPU inside the head kernels, on the CPU in the criterion.  The training loss is the
        # smoothed one; evaluation and prediction always use the plain NLL.  0: off.
        self.label_smoothing = float(label_smoothing)
        if not 0.0 <= self.label_smoothing <= 1.0:
            raise ValueError(f"label_smoothing must be in 0..1, got {label_smoothing}")
        # per-step learning-rate schedule (optim/schedule.py): the rate of optimizer step
        # epoch * spe + i is the run's table entry -- on the GPU copied into the optimizer's lr
        # word by the launch that advances the step counter, on the CPU set before each step.
        # None: off, and the optimizer's lr is whatever the host sets (adjust_learning_rate).
        self.schedule = schedule
        # dropout on the CNN's hidden units (data/dropout.py): training steps only -- on the GPU
        # inside the head kernel, on the CPU a multiplier after fc1's ReLU.  None or p = 0: off,
        # and nothing changes.
        self.dropout = dropout if dropout is not None and dropout.enabled else None
        if self.dropout is not None and model != "cnn":
            raise ValueError(f"dropout needs a hidden layer: the {model} model has none")
        # train-time augmentation (data/augment.py): applied to the training batches only --
        # on the GPU inside the epoch gather, on the CPU per batch.  None or a spec with every
        # range 0: off, and nothing changes.
        self.augment = augment if augment is not None and augment.enabled else None
        self._aug_tables = self.augment.tables() if self.augment is not None else None
        self._epoch = None
        # how the step is laid out (fusions, band splits, collective placement): read from
        # the PDM_* knobs once, here, unless the caller passes one
        self.structure = structure if structure is not None else StepStructure.from_env()
        self.dtype = dtype
        self.arena = arena
        self.optimizer = optimizer
        self.reducer = reducer
        self.device = arena.device
        self.batch_size = int(batch_size)
        if self.batch_size < 1:
            raise ValueError("per-rank batch size must be >= 1")
        self.eval_batch = int(eval_batch or self.batch_size)
        self.use_graphs = bool(use_graphs)
        self.metrics = DeviceMetrics(self.device)
        self.is_gpu = self.device.type == "cuda"
        self.train_split = train_split
        self.test_split = test_split
        self.train_idx_cpu: Optional[torch.Tensor] = None
        self._bounds = []
        self._n_train = 0
        # host sync before the once-per-epoch metric read: set by the app to a bounded
        # wait (parallel.bounded_sync) so a hung collective raises after --timeout
        self.sync_fn = None
        if self.is_gpu:
            from .gpu_step import make_gpu_step
            self.gpu = make_gpu_step(self, use_graphs=use_graphs)
        else:
            if dtype != "fp32":
                raise ValueError("the CPU path computes in fp32 only (--dtype fp32)")
            self.gpu = None

    # -- epochs ---------------------------------------------------------------
    def set_train_indices(self, indices: torch.Tensor, next_indices=None, epoch=None) -> None:
        """Install this rank's sample order for the coming epoch (and, on the GPU, start
        materialising the next epoch's, ``next_indices``, beside this one's first steps).

        GPU: the pinned int32 order the prefetcher hands over is read by the gather kernel in
        place; the batch bounds are arithmetic (full batches, then one ragged tail, as the
        DataLoader).  ``epoch``: the epoch number, which the augmentation's and the dropout's
        draws depend on (``next_indices`` is epoch + 1's order); required with either on,
        unused otherwise."""
        if self.augment is not None and epoch is None:
            raise ValueError("augmentation is on: set_train_indices needs the epoch number "
                             "(the transforms are drawn per (seed, epoch, sample))")
        if self.dropout is not None and epoch is None:
            raise ValueError("dropout is on: set_train_indices needs the epoch number "
                             "(the masks are drawn per (seed, epoch, sample, unit))")
        if self.mixup is not None and epoch is None:
            raise ValueError("mixup is on: set_train_indices needs the epoch number "
                             "(the pairs are drawn per (seed, epoch, sample))")
        if self.schedule is not None:
            if epoch is None:
                raise ValueError("a learning-rate schedule is on: set_train_indices needs the "
                                 "epoch number (the rate follows (epoch, step in epoch))")
            spe = -(-len(indices) // self.batch_size)
            if spe != self.schedule.spe or not 0 <= int(epoch) < self.schedule.epochs:
                raise ValueError(f"the learning-rate schedule covers {self.schedule.epochs} "
                                 f"epochs of {self.schedule.spe} steps: epoch {epoch} of {spe} "
                                 "steps is not one of them")
        self._n_train = len(indices)
        self._epoch = None if epoch is None else int(epoch)
        if self.gpu is not None:
            self.gpu.set_train_indices(indices, next_indices, epoch)
            return
        self.train_idx_cpu = indices.to(torch.int64)
        self._bounds = batch_bounds(len(indices), self.batch_size)

    @property
    def steps_per_epoch(self) -> int:
        return -(-self._n_train // self.batch_size)

    def train_epoch(self):
        self.metrics.reset(DeviceMetrics.TRAIN)
        self.optimizer.sync_hyperparams()
        if self.gpu is not None:
            self.gpu.begin_epoch()
            full, tail = divmod(self._n_train, self.batch_size)
            self.gpu.train_steps(self.batch_size, full)      # full batches come first
            if tail:
                self.gpu.train_step(tail)                     # ragged tail
            if self.sync_fn is not None:
                self.sync_fn("training epoch")
            self.gpu.check_device()
            lr = self.gpu.scheduled_lr()
            if lr is not None:
                # the rate of the last step run, as the reference keeps the last rate it set
                # (checkpoints); the device word already holds it
                self.optimizer.param_groups[0]["lr"] = lr
                self.optimizer._lr_synced = lr
        else:
            buf = self.metrics.buf[0:3]
            table = None if self.schedule is None else self.schedule.table()
            g0 = 0 if table is None else self._epoch * self.schedule.spe
            for i, (start, size) in enumerate(self._bounds):
                idx = self.train_idx_cpu[start:start + size]
                images, mix = self.train_batch_cpu(idx)
                train_step_cpu(self.model, self.arena, images,
                               self.train_split.labels[idx], self.reducer, self.optimizer, buf,
                               dropout=self.dropout, dataset_index=idx, epoch=self._epoch,
                               lr=None if table is None else float(table[g0 + i]),
                               label_smoothing=self.label_smoothing, ema=self.ema, mixup=mix)
        return self.metrics.read(DeviceMetrics.TRAIN)

    def set_tta(self, views: int, spec: Optional[AugmentSpec]) -> None:
        """Install the test-time augmentation: `views` views per image (1..32; 1 = off) drawn
        with the ranges and the seed of `spec`, which more than one view needs enabled."""
        spec = spec if spec is not None and spec.enabled else None
        self.tta = check_tta(views, spec)
        self.tta_augment = spec
        self._tta_tables = spec.tables() if spec is not None else None

    def set_schedule(self, schedule: Optional[ScheduleSpec]) -> None:
        """Install (or with None remove) the learning-rate schedule; on the GPU the graphs are
        re-captured on next use."""
        self.schedule = schedule
        if self.gpu is not None:
            self.gpu.set_schedule(schedule)

    def train_images_cpu(self, idx: torch.Tensor) -> torch.Tensor:
        """The CPU path's training batch of the samples `idx` (uint8 [len(idx), 784]), mixed and
        augmented for the installed epoch when mixup / augmentation are on."""
        return self.train_batch_cpu(idx)[0]

    def train_batch_cpu(self, idx: torch.Tensor):
        """(images, mix): train_images_cpu's batch and, with mixup on, what the criterion needs
        of the pairs, (partner labels int64 [n], lambda fp32 [n]); else None.  The images are
        mixed as uint8 first and transformed second, with the primary sample's parameters."""
        mix = None
        if self.mixup is None:
            images = self.train_split.images[idx]
        else:
            images, j, q = mix_batch(self.train_split.images, idx, self._epoch, self.mixup,
                                     self._mix_table)
            mix = (self.train_split.labels[torch.from_numpy(j)].to(torch.int64),
                   torch.from_numpy(q).to(torch.float32) / 256.0)
        if self.augment is not None:
            images = augment_batch(images, idx, self._epoch, self.augment, self._aug_tables)
        return images, mix

    # -- fc1 optimizer-state sharding (CNN, world size > 1) ------------------------------------
    def shard_supported(self) -> bool:
        return self.shard_unsupported_reason() is None

    def shard_unsupported_reason(self):
        """None when the fc1 update can be sharded here, else why not (for the user)."""
        if self.ema is not None:
            return ("the weight average (--ema-decay) takes in every step's whole weights on "
                    "every rank")
        if self.model != "cnn":
            return f"the {self.model} model has no fc1 layer to shard"
        if self.gpu is not None:
            if not hasattr(self.gpu, "shard_unsupported_reason"):
                return (f"the {self.dtype} CNN program has no sharded update "
                        "(only the bf16 CNN program does)")
            return self.gpu.shard_unsupported_reason()
        ws = self.reducer.comm.world_size
        if not self.reducer.can_shard:
            return f"the {self.reducer.kind} gradient transport has no reduce-scatter"
        if 128 % ws:
            return f"world size {ws} does not split fc1's 128 rows evenly"
        return None

    def set_shard_fc(self, on: bool = True) -> None:
        """Shard the fc1 weight's optimizer update over the ranks: its gradient is
        reduce-scattered (GPU; the gloo CPU path all-reduces it), each rank updates its
        128 / world_size rows and the updated rows are all-gathered (bf16 rows on the GPU,
        fp32 rows on the CPU).  Optimizer state of the other rows is not kept current:
        ``sync_master`` gathers it (checkpoints)."""
        if self.gpu is not None:
            self.gpu.set_shard_fc(on)
            return
        if not on:
            self.sync_master()
            self.reducer.clear_shard()
            return
        ws = self.reducer.comm.world_size
        self.reducer.set_shard(0, self.arena.spec.offset("fc1.weight"), 128 // ws * 9216)

    def sync_master(self) -> None:
        """Make the fp32 master weights and optimizer state whole on every rank (a no-op
        unless an update is sharded; collective then: every rank calls it)."""
        if self.gpu is not None:
            if hasattr(self.gpu, "sync_master"):
                self.gpu.sync_master()
            return
        sh = getattr(self.reducer, "shard", None)
        if sh is not None:
            _, start, count = sh
            n = count * self.reducer.comm.world_size
            for buf in self.optimizer.state_buffers().values():
                self.reducer.gather(buf[start:start + n])

    def use_structure(self, reducer, rccl_mode: Optional[str] = None,
                      xgmi_exchange: Optional[bool] = None) -> None:
        """Switch the step to another gradient reducer and step structure (the start-up
        check's fallbacks, parallel/startup.py; bench.py's calibration candidates): graphs
        are re-captured on next use."""
        self.reducer = reducer
        g = self.gpu
        if g is None:
            return
        if getattr(g, "shard_fc", False):
            g.set_shard_fc(False)            # (gathers the sharded state on the old reducer)
        g.reducer = reducer
        g.use_graphs = self.use_graphs and reducer.capturable
        if rccl_mode is not None and hasattr(g, "set_rccl_mode"):
            g.set_rccl_mode(rccl_mode, invalidate=False)
        if xgmi_exchange is not None and hasattr(g, "xgmi_exchange"):
            g.xgmi_exchange = bool(xgmi_exchange) and self.structure.xgmi_exchange
        g.invalidate_graphs()

    def run_steps(self, n: int, bsz: Optional[int] = None) -> None:
        """Run ``n`` full steps from the current counter (bench helper; GPU only)."""
        self.gpu.train_steps(bsz or self.batch_size, n)

    def _eval_arena(self, average: Optional[bool]):
        """The arena evaluate() / predict() read: the averaged weights when `average` (None:
        whenever the average is on), else the training weights."""
        if average is None:
            average = self.ema is not None
        if not average:
            return self.arena
        if self.ema is None:
            raise ValueError("this program keeps no weight average (ema=None)")
        return self.ema.arena

    @torch.no_grad()
    def evaluate(self, average: Optional[bool] = None):
        """Full, unsharded test-set pass on every rank (reference :99-116, :142-149).  With the
        weight average on it evaluates the averaged weights (average=False: the training
        weights); neither the training weights nor any state of the step is touched."""
        self.metrics.reset(DeviceMetrics.EVAL)
        n = len(self.test_split)
        arena = self._eval_arena(average)
        if self.tta > 1:
            # test-time augmentation: the combined rows' sums, sum of -log_probs[y], correct
            # and rows, in fp64 -- on the GPU added by tta_reduce, chunk by chunk
            if self.gpu is not None:
                self.gpu.predict_tta(self.gpu.test_images, self.gpu.test_labels,
                                     None if arena is self.arena else self.gpu.weight_set(arena),
                                     self.tta_augment, self.tta,
                                     metrics=self.metrics.eval_view())
                if self.sync_fn is not None:
                    self.sync_fn("evaluation")
            else:
                y = self.test_split.labels.to(torch.int64)
                logp, pred, _ = self._predict_tta_cpu(arena, self.test_split.images, None,
                                                      self.tta)
                buf = self.metrics.buf[3:6]
                buf[0] += -logp.gather(1, y[:, None]).to(torch.float64).sum()
                buf[1] += int(pred.eq(y).sum())
                buf[2] += n
        elif self.gpu is not None:
            self.gpu.evaluate(None if arena is self.arena else self.gpu.weight_set(arena))
            if self.sync_fn is not None:
                self.sync_fn("evaluation")
        else:
            buf = self.metrics.buf[3:6]
            for start, size in batch_bounds(n, self.eval_batch):
                eval_step_cpu(self.model, arena, self.test_split.images[start:start + size],
                              self.test_split.labels[start:start + size], buf)
        return self.metrics.read(DeviceMetrics.EVAL)

    @torch.no_grad()
    def predict(self, images=None, labels=None, average: Optional[bool] = None,
                tta: Optional[int] = None) -> Prediction:
        """Per-sample predictions of the current weights: for ``images`` (uint8 [N, 28, 28] or
        [N, 784], torch or NumPy, any N >= 1; ``labels`` optional), or with no arguments for the
        test split and its labels.  Runs evaluate()'s forward; the metric accumulators are not
        touched.  ``average``: as evaluate()'s.  ``tta``: the number of test-time views per
        image (None: the program's; 1: none); with more than one, log_probs is the log of the
        views' mean probability, and view v of row r is drawn for r's position in ``images``."""
        arena = self._eval_arena(average)
        views = self.tta if tta is None else check_tta(tta, self.tta_augment)
        if images is None:
            if labels is not None:
                raise ValueError("labels without images")
            if self.gpu is not None:       # the device-resident copy of the test split
                images, labels = self.gpu.test_images, self.gpu.test_labels
            else:
                images, labels = self.test_split.images, self.test_split.labels
        else:
            images = image_rows(images)
            if labels is not None:
                labels = label_vector(labels, images.shape[0])
        if self.gpu is not None:
            ws = None if arena is self.arena else self.gpu.weight_set(arena)
            if views > 1:
                logp, pred, conf = self.gpu.predict_tta(images, labels, ws, self.tta_augment,
                                                        views)
            else:
                logp, pred, conf = self.gpu.predict(images, labels, ws)
            if self.sync_fn is not None:
                self.sync_fn("prediction")
            return Prediction(logp.cpu(), pred.cpu().to(torch.int64),
                              None if conf is None else conf.cpu())
        if views > 1:
            return Prediction(*self._predict_tta_cpu(arena, images, labels, views))
        outs = [predict_step_cpu(self.model, arena, images[start:start + size],
                                 None if labels is None else labels[start:start + size])
                for start, size in batch_bounds(images.shape[0], PREDICT_BATCH_CPU)]
        return Prediction(torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]),
                          None if labels is None else sum(o[2] for o in outs))

    def _predict_tta_cpu(self, arena, images, labels, views: int):
        """The CPU path's predict() with `views` > 1 test-time views: per batch of rows, every
        view (data/augment.py tta_view) through predict_step_cpu, combined by tta_reduce_cpu."""
        spec, tables = self.tta_augment, self._tta_tables
        outs = []
        for start, size in batch_bounds(images.shape[0], PREDICT_BATCH_CPU):
            lv = torch.stack([predict_step_cpu(self.model, arena,
                                               tta_view(images, start, size, v, spec, tables))[0]
                              for v in range(views)])
            outs.append(tta_reduce_cpu(lv, None if labels is None else
                                       labels[start:start + size]))
        return (torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]),
                None if labels is None else sum(o[2] for o in outs))


def build_local_program(arch: str, dtype: str, device, batch_size: int, train_split, test_split,
                        optimizer: str = "adam", lr: float = 1e-3, momentum: float = 0.9,
                        weight_decay: float = 1e-4, seed: int = 0, use_graphs: bool = True,
                        comm=None, force_comm: bool = False, transport: str | None = None,
                        augment: Optional[AugmentSpec] = None,
                        dropout: Optional[DropoutSpec] = None,
                        schedule: Optional[ScheduleSpec] = None, label_smoothing: float = 0.0,
                        ema: Optional[EmaSpec] = None, mixup: Optional[MixupSpec] = None,
                        tta: int = 1, tta_augment: Optional[AugmentSpec] = None):
    """Single-rank program without a process group (tests, bench at N=1, smoke)."""
    from types import SimpleNamespace

    from ..models.reference import MODULES
    from ..models.specs import get_spec
    from ..optim.flat import build_optimizer
    from ..parallel.comm import LocalComm
    from ..parallel.reducer import GradReducer
    from .arena import FlatArena

    torch.manual_seed(seed)
    spec = get_spec(arch)
    arena = FlatArena(spec, torch.device(device))
    arena.load_module(MODULES[arch]())
    opt = build_optimizer(optimizer, arena, SimpleNamespace(lr=lr, momentum=momentum,
                                                            weight_decay=weight_decay))
    comm = comm or LocalComm()
    reducer = GradReducer(comm, arena.grads, spec.bucket_bounds(), channels=spec.channel_bounds(),
                          force=force_comm,
                          transport=transport)
    return TrainProgram(arch, dtype, arena, opt, reducer, train_split, test_split, batch_size,
                        use_graphs=use_graphs, augment=augment, dropout=dropout,
                        schedule=schedule, label_smoothing=label_smoothing,
                        ema=None if ema is None else WeightEma(ema, arena), mixup=mixup,
                        tta=tta, tta_augment=tta_augment)
