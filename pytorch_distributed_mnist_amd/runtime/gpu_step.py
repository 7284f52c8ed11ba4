"""GPU step programs: the fixed kernel chains of one training step, and graphs.

Each model family has a ``_train_impl(B)`` that enqueues, on the current HIP
stream, every kernel of one step plus the bucket all-reduces; it has no host
inputs (batch indices come from a device step counter), so it is captured once
per batch size into a ``torch.cuda.CUDAGraph`` (hipGraph) and replayed.

Counter protocol (kernels of one step must not race on a counter): the first
kernel reads the data-step counter and only a later kernel advances it; the
optimizer-step counter is advanced before the optimizer kernel reads it (t >= 1).
CNN: ``cnn_head`` advances both.  Linear: ``lin_train`` advances the optimizer
step, ``lin_reduce`` (or, at world size 1, the optimizer launch) the data step.
With a learning-rate schedule installed (optim/schedule.py), the launch that advances
the optimizer-step counter also copies the step's rate from the run's table into the
optimizer's lr word: lr and the step count travel together, to the same readers.

With the weight average on (optim/ema.py) every chain below ends in one more launch,
ema_update, which only reads the optimizer-step counter.

Linear (reference Net, fp32):  lin_train -> [lin_reduce -> all-reduce] -> optim
CNN (bf16):  cnn_fwd -> fc1_fwd -> cnn_head -> fc1_bwd -> [all-reduce bucket 0]
             -> cnn_bwd -> conv_reduce -> [all-reduce bucket 1] -> optim
"""
from __future__ import annotations

import gc
import os

import torch

from ..ops import _ext
from ..optim.ema import ema_weight
from .. import knobs


_GRAPH_STEPS = int(knobs.get("PDM_GRAPH_STEPS", "16"))  # steps per full graph
if _GRAPH_STEPS <= 0:
    raise ValueError(f"PDM_GRAPH_STEPS must be positive, got {_GRAPH_STEPS}")


def make_gpu_step(prog, use_graphs: bool = True):
    if prog.model == "linear":
        if prog.dtype != "fp32":
            raise ValueError("the reference Linear model runs in fp32 (--dtype fp32)")
        return LinearStep(prog, use_graphs)
    if prog.model == "cnn":
        if prog.dtype == "fp32":                 # the reference's precision, fp32 MFMA
            from .cnn_f32_step import CnnStepF32
            return CnnStepF32(prog, use_graphs)
        if prog.dtype != "bf16":
            raise ValueError(f"unsupported CNN dtype {prog.dtype!r} (bf16 or fp32)")
        from .cnn_step import CnnStep
        return CnnStep(prog, use_graphs)
    raise ValueError(prog.model)


class GpuStepBase:
    def check_device(self) -> None:
        """Raise if a kernel of this step recorded an error it could not raise itself (the
        default: none can)."""

    def __init__(self, prog, use_graphs: bool):
        self.C = _ext.require()
        self.prog = prog
        dev = prog.device
        self.device = dev
        self.arena = prog.arena
        self.opt = prog.optimizer
        self.reducer = prog.reducer
        self.train_images = prog.train_split.images.to(dev).contiguous()
        self.train_labels = prog.train_split.labels.to(device=dev, dtype=torch.int32).contiguous()
        self.test_images = prog.test_split.images.to(dev).contiguous()
        self.test_labels = prog.test_split.labels.to(device=dev, dtype=torch.int32).contiguous()
        # [train data step, (spare)]
        self.ctr = torch.zeros(2, dtype=torch.int64, device=dev)
        # the samples of two consecutive epochs in sampler order (set_train_indices): epoch e
        # in half e & 1 of the epoch buffer, located by the running data-step counter
        # (kernels.h StepRows: spe steps per epoch)
        self.ep_images = torch.empty(0, dtype=torch.uint8, device=dev)
        self.ep_labels = torch.empty(0, dtype=torch.int32, device=dev)
        self.spe = 0
        self._n_epoch = 0
        self._ctr_host = 0               # the data-step counter's value once the queue drains
        self._dev_step = None            # the optimizer-step count the device holds (host view)
        # [order, half, event | None, epoch | None]: the next epoch's gather
        self._pending = None
        # train-time augmentation (data/augment.py): the epoch gather transforms each image;
        # its Q14 tables are uploaded once, here, never during a capture
        self.augment = getattr(prog, "augment", None)
        self._aug_tables = None
        if self.augment is not None:
            self._aug_tables = tuple(torch.from_numpy(t).to(dev) for t in self.augment.tables())
        # dropout on the CNN's hidden units (data/dropout.py): the head draws a row's mask from
        # its dataset index, which travels in the label word -- the training labels are uploaded
        # tagged, label | (index << 4), once, here (the gathers and the forward kernels copy
        # label words verbatim; test labels are never tagged) -- and from the epoch, a device
        # word that set_train_indices fills in stream order (as the optimizer's lr: the graphs
        # read the pointer, so one set of graphs serves every epoch)
        self.dropout = getattr(prog, "dropout", None)
        self._epoch_dev = None
        if self.dropout is not None:
            from ..data.dropout import tag_labels
            self.train_labels = tag_labels(prog.train_split.labels).to(dev).contiguous()
            self._epoch_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        # mixup (data/mixup.py): the epoch gather blends every image with its partner's and the
        # head mixes the targets, both from the same (seed, epoch, dataset index) draw.  The head
        # learns a row's dataset index and the epoch as the dropout head does, so the tagged
        # training labels and the epoch word are there with mixup on, dropout or not; the
        # quantile table (and, without augmentation, the identity transform's tables) are
        # uploaded once, here, never during a capture
        self.mixup = getattr(prog, "mixup", None)
        self._mix_table = None
        if self.mixup is not None:
            from ..data.dropout import tag_labels
            if self.dropout is None:
                self.train_labels = tag_labels(prog.train_split.labels).to(dev).contiguous()
                self._epoch_dev = torch.zeros(1, dtype=torch.int32, device=dev)
            self._mix_table = torch.from_numpy(self.mixup.table().copy()).to(dev)
            if self._aug_tables is None:
                from ..data.augment import AugmentSpec
                self._aug_tables = tuple(torch.from_numpy(t).to(dev)
                                         for t in AugmentSpec().tables())
        # label smoothing of the training heads (--label-smoothing E): a per-run constant, passed
        # to the head launch as a kernel argument and baked into the graphs; 0: off, and the
        # step launches the plain heads
        self.label_smoothing = float(getattr(prog, "label_smoothing", 0.0))
        # per-step learning-rate schedule (optim/schedule.py): the run's table is uploaded once,
        # here; its pointer, length and the cursor word are baked into the graphs, so one set
        # of graphs serves every epoch.  The cursor is the global index of the next optimizer
        # step; begin_epoch puts it at epoch * spe when the device holds something else
        # (_sched_dev is the host's view of the device word, as _dev_step)
        self._install_schedule(getattr(prog, "schedule", None))
        # exponential moving average of the weights (optim/ema.py): ema_update is the last
        # launch of every step (launch_ema).  With the warmup on it computes the update's
        # index from the optimizer-step word plus _ema_off, the host's count of updates minus
        # the word's value (both move on by one per step, so the offset holds until either is
        # set anew: a resume, the start-up check's restore); the offset is a kernel argument,
        # baked into the graphs, which are re-captured when it changes (_ema_sync)
        self.ema = getattr(prog, "ema", None)
        self._ema_off = None
        # test-time augmentation (predict_tta): the views' Q14 tables on the device, per spec
        self._tta_table_cache = {}
        self._epoch_start = 0
        self._gather_stream = None       # stream of the ahead-of-time gathers
        self._ring = None                # pinned staging buffers of the epoch orders
        self._ring_i = 0
        self.use_graphs = bool(use_graphs) and self.reducer.capturable
        self.graphs = {}
        self.bfull = prog.batch_size
        self.structure = prog.structure
        self.metrics = prog.metrics
        self._opt_segments = None
        # step phase for double-buffered operands (CnnStep's W1^T): a step reads the buffers of
        # phase p and leaves the next step phase (p + 1) % phase_period.  A graph bakes in the
        # phase it was captured at, so graphs are keyed by it as well.
        self.phase = 0
        self.phase_period = 1

    # -- data ----------------------------------------------------------------

    def _stage(self, idx: torch.Tensor) -> list:
        """Copy an epoch order into the next pinned staging buffer of a ring of three ([buffer,
        event]); the gather kernel reads it in place (zero-copy).  The buffers are allocated
        once, on this thread and never during a graph capture (a host-memory allocation from
        any thread would invalidate a capture), and one is reused only after the event behind
        its previous reader has completed (at most two are in flight: this epoch's and the
        next's)."""
        n = idx.numel()
        if self._ring is None or self._ring[0][0].numel() != n:
            for old in self._ring or ():
                if old[1] is not None:   # a queued gather still reads this pinned buffer
                    old[1].synchronize()
            self._ring = [[torch.empty(n, dtype=torch.int32, pin_memory=True), None]
                          for _ in range(3)]
            self._ring_i = 0
        buf = self._ring[self._ring_i]
        self._ring_i = (self._ring_i + 1) % 3
        if buf[1] is not None:
            buf[1].synchronize()
        buf[0].copy_(idx)
        return buf

    def _gather(self, idx: torch.Tensor, half: int, stream, epoch=None) -> torch.cuda.Event:
        """Queue the gather of an epoch order into half `half` of the epoch buffer on `stream`;
        returns the event behind it.  With augmentation on, the augmenting gather draws the
        transforms of epoch `epoch`."""
        n = self._n_epoch
        buf = self._stage(idx)
        with torch.cuda.stream(stream):
            if self.mixup is not None:
                # --mixup: always the mixup twin of the elastic gather; without augmentation
                # its ranges are zero (the identity tables), which is the plain mixed gather
                a = self.augment
                cosq, sinq, invz = self._aug_tables
                self.C.gather_epoch_mixup(self.train_images, self.train_labels, buf[0],
                                          self.ep_images.view(-1, 784)[half * n:(half + 1) * n],
                                          self.ep_labels[half * n:(half + 1) * n],
                                          max_wgs=0, cosq=cosq, sinq=sinq, invz=invz,
                                          shift=0 if a is None else a.shift, epoch=int(epoch),
                                          seed=0 if a is None else a.seed,
                                          elastic_q=0 if a is None else a.elastic_q,
                                          qt=self._mix_table,
                                          ntrain=self.train_images.shape[0],
                                          mixup_seed=self.mixup.seed)
            elif self.augment is None:
                self.C.gather_epoch(self.train_images, self.train_labels, buf[0],
                                    self.ep_images.view(-1, 784)[half * n:(half + 1) * n],
                                    self.ep_labels[half * n:(half + 1) * n],
                                    # one workgroup per 64 rows (grid-striding ones taking
                                    # fewer CUs beside the steps measured no better)
                                    max_wgs=0)
            elif self.augment.elastic > 0.0:
                # --aug-elastic: the elastic twin of the augmenting gather (the same contract,
                # plus the control displacements' range)
                cosq, sinq, invz = self._aug_tables
                self.C.gather_epoch_elastic(self.train_images, self.train_labels, buf[0],
                                            self.ep_images.view(-1, 784)[half * n:(half + 1) * n],
                                            self.ep_labels[half * n:(half + 1) * n],
                                            max_wgs=0, cosq=cosq, sinq=sinq, invz=invz,
                                            shift=self.augment.shift, epoch=int(epoch),
                                            seed=self.augment.seed,
                                            elastic_q=self.augment.elastic_q)
            else:
                cosq, sinq, invz = self._aug_tables
                self.C.gather_epoch_augment(self.train_images, self.train_labels, buf[0],
                                            self.ep_images.view(-1, 784)[half * n:(half + 1) * n],
                                            self.ep_labels[half * n:(half + 1) * n],
                                            max_wgs=0, cosq=cosq, sinq=sinq, invz=invz,
                                            shift=self.augment.shift, epoch=int(epoch),
                                            seed=self.augment.seed)
            ev = torch.cuda.Event()
            ev.record(stream)
        buf[1] = ev
        return ev

    def set_train_indices(self, idx_cpu: torch.Tensor, next_idx=None, epoch=None) -> None:
        """Install this epoch's sample order; optionally start materialising the next one's.

        ``gather_epoch`` copies an epoch's samples contiguously into one half of the epoch
        buffer (the step kernels read their rows behind one counter load), reading the order
        in place from a pinned staging buffer (``EpochIndexPrefetcher`` computes it on its
        worker thread; only this thread touches pinned memory).  The data-step counter is
        never reset: epoch e = counter / spe lives in half e & 1 (kernels.h StepRows), so the
        step graphs stay valid across epochs.  With ``next_idx`` given, the next epoch's
        gather is queued on a side stream into the other half once this epoch is half-way
        through (``_issue_ahead``), behind an event after the steps queued so far (the other
        half's last reader, the previous epoch, is among them), and runs beside this epoch's
        steps.  At the next boundary that gather has long completed (the host checks its
        event) and the compute stream does not even wait for it: in steady state an epoch
        boundary enqueues nothing.  The host never waits for queued steps.

        ``epoch`` is the epoch number of ``idx_cpu`` (``next_idx`` is epoch + 1's order): with
        augmentation on, the gathers transform each image by its (seed, epoch, sample) draw,
        so the number is required; with dropout on, the head draws its masks from it (the
        epoch word is filled here, in stream order: behind every step of the previous epoch
        queued so far, ahead of this epoch's); with mixup on, the gather and the head both
        draw the pairs from it; without any of them, it is not used.
        """
        if self.schedule is not None:
            if epoch is None:
                raise ValueError("a learning-rate schedule is on: set_train_indices needs the "
                                 "epoch number")
            self._sched_epoch = int(epoch)
        if self.augment is None and self.dropout is None and self.mixup is None:
            epoch = None
        elif epoch is None:
            raise ValueError(("augmentation" if self.augment is not None else
                              "dropout" if self.dropout is not None else "mixup") +
                             " is on: set_train_indices needs the epoch number")
        else:
            epoch = int(epoch)
            if self._epoch_dev is not None and not 0 <= epoch < 2 ** 31:
                raise ValueError(f"epoch {epoch} does not fit the device epoch word")
        n = idx_cpu.numel()
        cur = torch.cuda.current_stream(self.device)
        if self._n_epoch != n:
            p = self._pending
            if p is not None and p[2] is not None:
                # an ahead gather still writes the old epoch buffer and reads a pinned buffer
                # of the ring about to be replaced: drain it before either is freed
                p[2].synchronize()
            self.ep_images = torch.empty(2 * n * 784, dtype=torch.uint8, device=self.device)
            self.ep_labels = torch.empty(2 * n, dtype=torch.int32, device=self.device)
            self._n_epoch = n
            self.spe = -(-n // self.bfull)
            self.graphs.clear()          # graphs captured the old buffer and geometry
            self._pending = None
        if self.schedule is not None and self.spe != self.schedule.spe:
            raise ValueError(f"the learning-rate schedule was built for {self.schedule.spe} "
                             f"steps per epoch; this epoch has {self.spe}")
        # this epoch starts at the next multiple of spe (a partial epoch before it -- tests,
        # tools -- moves the counter on)
        start = -(-self._ctr_host // self.spe) * self.spe
        if start != self._ctr_host:
            self.ctr[0:1].fill_(start)
            self._ctr_host = start
        half = (start // self.spe) & 1
        p, self._pending = self._pending, None
        if p is not None and p[0] is idx_cpu and p[1] == half and p[2] is not None and \
                p[3] == epoch:
            if not p[2].query():         # gathered ahead on the side stream: still running
                cur.wait_event(p[2])
        else:
            if p is not None and p[2] is not None:
                cur.wait_event(p[2])     # an unused ahead gather still writes a half
            self._gather(idx_cpu, half, cur, epoch)
        if self._epoch_dev is not None:
            self._epoch_dev.fill_(epoch)     # on the compute stream, never inside a capture
        self._epoch_start = start
        if next_idx is not None and next_idx.numel() == n:
            if self._gather_stream is None:
                # created and used once here, not inside a timed run: HIP sets up a stream's
                # hardware queue at its first launch (~5 ms of host time)
                self._gather_stream = torch.cuda.Stream(self.device)
                with torch.cuda.stream(self._gather_stream):
                    torch.zeros(1, device=self.device)
            self._pending = [next_idx, 1 - half, None, None if epoch is None else epoch + 1]

    def _issue_ahead(self) -> None:
        """Queue the next epoch's gather on the side stream once this epoch is half-way
        through (train_steps calls this between replays): the copy then runs beside steps in
        the middle of an epoch rather than beside the first steps after a boundary."""
        p = self._pending
        if p is None or p[2] is not None or \
                self._ctr_host - self._epoch_start < max(1, self.spe // 2):
            return
        # the side stream waits for everything queued on the compute stream so far; the other
        # half's last reader, the previous epoch, is among it
        free = torch.cuda.Event()
        free.record(torch.cuda.current_stream(self.device))
        self._gather_stream.wait_event(free)
        p[2] = self._gather(p[0], p[1], self._gather_stream, p[3])

    def skip_steps(self, k: int) -> None:
        """Move the data-step counter k steps on within the epoch (bench.py positions its
        timed window; every step is the same kernel chain on a different batch)."""
        self.ctr[0:1].add_(k)
        self._ctr_host += k
        if self.schedule is not None:    # the schedule follows (epoch, step in epoch)
            self._sched_cursor.add_(k)
            self._sched_dev += k
        self._issue_ahead()              # as the skipped steps would have

    def begin_epoch(self) -> None:
        self.opt.sync_hyperparams()
        if self._dev_step != self.opt.step_count:
            self.opt.sync_step()
            self._dev_step = self.opt.step_count
        if self.schedule is not None and self._sched_epoch is not None:
            # the epoch's first step is global step epoch * spe: written in stream order (never
            # inside a capture) when the device holds something else -- at the start, on a
            # resume, after a partial epoch; in steady state the cursor is already there
            want = self._sched_epoch * self.schedule.spe
            if self._sched_dev != want:
                self._sched_cursor.fill_(want)
                self._sched_dev = want

    def _install_schedule(self, schedule) -> None:
        self.schedule = schedule
        self._sched_table = self._sched_cursor = None
        if schedule is not None:
            self._sched_table = torch.from_numpy(schedule.table().copy()).to(self.device)
            self._sched_cursor = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._sched_dev = 0
        self._sched_epoch = None

    def set_schedule(self, schedule) -> None:
        """Install (or with None remove) the per-step learning-rate schedule; the graphs bake
        its table in, so they are re-captured."""
        if schedule is None and self.schedule is None:
            return
        self._install_schedule(schedule)
        self.invalidate_graphs()

    def lr_sched(self):
        """The lr_sched argument of the launch that advances the optimizer-step counter (None
        without a schedule): (table, cursor, the optimizer's lr word)."""
        if self.schedule is None:
            return None
        return (self._sched_table, self._sched_cursor, self.opt._lr_dev)

    def scheduled_lr(self):
        """The rate of the last step queued (None without a schedule, or before any step)."""
        if self.schedule is None or self._sched_dev < 1:
            return None
        return float(self.schedule.table()[self._sched_dev - 1])

    # -- step ------------------------------------------------------------------
    # One hipGraph replay costs ~10-16 us of host time (MI355X_MICROARCH.md price
    # list, graph-replay-floor) — more than a whole small step's GPU time — so
    # steps are captured GRAPH_STEPS at a time (identical steps: the batch comes
    # from the device counter) and a run of n steps replays n // GRAPH_STEPS
    # multi-step graphs plus one graph of the remainder.
    GRAPH_STEPS = _GRAPH_STEPS
    GRAPH_SIZES = tuple(range(_GRAPH_STEPS, 0, -1))

    def carries_across_graphs(self, B: int) -> bool:
        """Whether a step of batch B leaves work to the next one (CnnStep: the carried fc1 update), so
        consecutive graph replays of one train_steps call hand it over: the graphs then come
        in variants by (carry in, carry out)."""
        return False

    def _graph(self, B: int, nsteps: int, phase=None, cin: bool = False, cout: bool = False):
        phase = self.phase if phase is None else phase
        key = (B, nsteps, phase, bool(cin), bool(cout))
        g = self.graphs.get(key)
        if g is None:
            g = torch.cuda.CUDAGraph()
            saved = self.phase
            self.phase = phase
            # no garbage collection inside the capture: a GC pass there may tear down native
            # objects of earlier programs (RCCL finalize, stream syncs, frees), which is
            # prohibited while capturing and aborts the process (torch.cuda.graph collects
            # once before the capture begins)
            gc_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(g):          # captured on a side stream
                    # the persistent collective stays out of the graph when it is launched
                    # per train_steps call (collective_outside): no cross-queue edges
                    self._train_seq(B, nsteps, collective=not self.collective_outside(),
                                    cin=cin, cout=cout)
            finally:
                if gc_on:
                    gc.enable()
                self.phase = saved              # capturing runs nothing
            self.graphs[key] = g
        return g

    def _replay(self, B: int, nsteps: int, cin: bool = False, cout: bool = False) -> None:
        self._graph(B, nsteps, cin=cin, cout=cout).replay()
        self.phase = (self.phase + nsteps) % self.phase_period

    def _carry_flags(self, B: int, nreplays: int):
        """(carry in, carry out) of each of `nreplays` consecutive replays of one call."""
        if not self.carries_across_graphs(B):
            return [(False, False)] * nreplays
        return [(i > 0, i < nreplays - 1) for i in range(nreplays)]

    def _plan(self, B: int, n: int):
        """The replays of ``train_steps(B, n)``: [(steps, carry in, carry out)] -- n // GRAPH_STEPS
        full graphs, then one graph of the remainder (each graph boundary leaves the queue
        idle for ≈ 9 us: profiles/r6/window/)."""
        k = self.GRAPH_STEPS
        r = n % k
        sizes = [k] * (n // k) + ([r] if r else [])
        return [(s, ci, co) for s, (ci, co) in zip(sizes, self._carry_flags(B, len(sizes)))]

    def _variants(self, B: int, sizes):
        """Every (steps, phase, carry in, carry out) graph some ``_plan(B, n)`` replays, for the
        given graph sizes.  A graph smaller than GRAPH_STEPS only stands for the remainder,
        which is always a call's last replay, so it never carries out."""
        flags = ((False, False), (False, True), (True, True), (True, False)) \
            if self.carries_across_graphs(B) else ((False, False),)
        return [(n, ph, ci, co) for n in sizes for ph in range(self.phase_period)
                for ci, co in flags if not (co and n < self.GRAPH_STEPS)]

    def prepare(self, B: int, sizes=None) -> None:
        """Capture and upload every graph ``train_steps(B, n)`` replays (GRAPH_SIZES, or
        `sizes`, in every step phase), so no capture or first-launch upload lands inside a
        timed run.  Capturing enqueues nothing; the graphs' steps read the device counters
        when replayed."""
        if not self.use_graphs:
            return
        self._ema_sync()                 # (the graphs bake the EMA launch's offset in)
        for n, ph, ci, co in self._variants(B, sizes or self.GRAPH_SIZES):
            g = self._graph(B, n, ph, ci, co)
            try:
                exe = g.raw_cuda_graph_exec()
            except (AttributeError, RuntimeError):
                continue
            dev = self.device.index if self.device.index is not None else \
                torch.cuda.current_device()
            self.C.graph_upload(int(exe), dev)
        torch.cuda.synchronize(self.device)

    def train_steps(self, B: int, n: int) -> None:
        """Enqueue n consecutive training steps of batch size B."""
        if n <= 0:
            return
        if self.schedule is not None and self._sched_dev + n > self.schedule.total:
            # (the kernel's clamp to the last entry is only a backstop)
            raise RuntimeError(f"{n} steps from global step {self._sched_dev} run past the "
                               f"learning-rate schedule's {self.schedule.total} steps "
                               f"({self.schedule.epochs} epochs of {self.schedule.spe})")
        self._ema_sync()
        if self.use_graphs:
            plan = self._plan(B, n)
            if self.collective_outside():
                # one persistent collective for all n steps, launched eagerly on its own
                # stream beside the graph replays: the steps hand it their buckets through
                # device words, and the last optimizer waits for its last bucket, so
                # nothing has to join it back (a graph fork / join edge between two queues
                # costs 5-10 us on MI355X, every replay).  Every graph is captured first: a
                # capture synchronizes the device, which would wait for a running
                # collective that waits for steps not yet launched.
                ph = self.phase
                for size, ci, co in plan:
                    self._graph(B, size, ph, ci, co)
                    ph = (ph + size) % self.phase_period
                self.reducer.begin(n, self.collective_channels(), self.collective_wide(B))
            for size, ci, co in plan:
                self._issue_ahead()
                self._replay(B, size, ci, co)
                self._ctr_host += size
        else:
            self._issue_ahead()
            self._train_seq(B, n)
            self._ctr_host += n
        self._issue_ahead()
        self.opt.step_count += n
        if self._dev_step is not None:
            self._dev_step += n
        if self.schedule is not None:
            self._sched_dev += n
        if self.ema is not None:
            self.ema.updates += n

    def _ema_sync(self) -> None:
        """Before steps are queued: make the offset the EMA launch adds to the optimizer-step
        word current (never inside a capture)."""
        if self.ema is None:
            return
        if self._dev_step is None:       # nobody has put the host's step count on the device
            self.opt.sync_step()
            self._dev_step = self.opt.step_count
        off = self.ema.updates - self._dev_step
        if off != self._ema_off:
            self._ema_off = off
            if self.ema.spec.warmup:     # (without it the kernel does not read the offset)
                self.graphs.clear()

    def launch_ema(self) -> None:
        """The step's last launch with the weight average on: ema += w (params - ema) over the
        whole arena, behind the launch that completed the step's weight update."""
        ema = self.ema
        if ema is None:
            return
        sp = ema.spec
        self.C.ema_update(self.arena.params, ema.params, self.arena.spec.total,
                          ema_weight(sp.decay), sp.warmup, sp.decay, self.opt._step_dev,
                          self._ema_off)

    def weight_set(self, arena):
        """What evaluate() / predict() read of a weight arena other than the training one (the
        averaged weights): the name views and whatever compute copies the forward kernels
        take, derived here, outside any capture.  The training weights, their copies and the
        step phase are not involved."""
        raise NotImplementedError

    def train_step(self, B: int) -> None:
        self.train_steps(B, 1)

    def collective_outside(self) -> bool:
        """Streamed xgmi: the persistent collective is launched per train_steps call outside
        the step graphs (StepStructure.xgmi_outside) instead of inside every graph."""
        return bool(self.reducer.streamed and self.structure.xgmi_outside)

    def collective_channels(self):
        """Buckets the persistent collective carries (None: all)."""
        return None

    def collective_wide(self, B: int) -> bool:
        """Whether the wide persistent collective fits beside this step's kernels at B."""
        return False

    def _train_seq(self, B: int, n: int, collective: bool = True, cin: bool = False,
                   cout: bool = False) -> None:
        """n consecutive steps (captured together into one graph, or eager); `collective`:
        launch (and join) the persistent collective for them here; cin / cout: work carried
        in from the previous sequence / out to the next (carries_across_graphs)."""
        streamed = self.reducer.streamed and collective
        if streamed:
            # one launch for the n steps
            self.reducer.begin(n, self.collective_channels(), self.collective_wide(B))
        for _ in range(n):
            self._train_impl(B)
            self.launch_ema()
            self.phase = (self.phase + 1) % self.phase_period
        if streamed:
            self.reducer.end()

    def _train_impl(self, B: int) -> None:
        raise NotImplementedError

    def launch_head_train(self, part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab, metrics,
                          c0, c1, xg=None, dh32=None) -> None:
        """The CNN programs' training head: cnn_head, or with dropout on its masking twin
        (cnn_head_drop.hip), which reads the dataset index from the tagged label word and the
        epoch from the device epoch word; with label smoothing on, cnn_head_smooth, or the
        masking twin with the smoothing passed on; with mixup on, cnn_head_mixup, which takes
        dropout and smoothing along."""
        d, e, m = self.dropout, self.label_smoothing, self.mixup
        if m is not None:
            # --mixup: the two-class twin of the masking head (cnn_head_mix.hip) whatever else
            # is on; it recomputes the gather's pairs and reads the partners' labels
            drop = dict(seed=d.seed, T=d.T, scale=d.scale) if d is not None else {}
            self.C.cnn_head_mixup(part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab,
                                  metrics, c0, c1, xg, dh32, epoch=self._epoch_dev,
                                  train_labels=self.train_labels,
                                  ntrain=self.train_labels.numel(), qt=self._mix_table,
                                  mixup_seed=m.seed, lr_sched=self.lr_sched(),
                                  label_smoothing=e, **drop)
        elif d is not None:
            smooth = dict(label_smoothing=e) if e > 0.0 else {}
            self.C.cnn_head_dropout(part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab,
                                    metrics, c0, c1, xg, dh32, self._epoch_dev, d.seed, d.T,
                                    d.scale, lr_sched=self.lr_sched(), **smooth)
        elif e > 0.0:
            self.C.cnn_head_smooth(part, splitk, B, bf1, wf2, bf2, ylab, dh, dht, ldt, slab,
                                   metrics, c0, c1, xg, dh32, e, lr_sched=self.lr_sched())
        else:
            self.C.cnn_head(part, splitk, B, bf1, wf2, bf2, ylab, True, dh, dht, ldt, slab,
                            metrics, c0, c1, xg, dh32, lr_sched=self.lr_sched())

    # -- optimizer ---------------------------------------------------------------
    def optimizer_segments(self):
        """[(offset, rows, cols, shadow|None, shadow_t|None)] covering the arena."""
        return [(0, 1, self.arena.spec.total, None, None)]

    def launch_optimizer(self, segments=None, signal_ch: int = -1, bump=None,
                         metrics=None, exchange: bool = False) -> None:
        """One fused optimizer launch over `segments` (default: every parameter).

        xgmi streamed mode: bucket `signal_ch` (>= 0) is published to the persistent
        collective and the update waits for the buckets its segments belong to, by a
        one-workgroup wait kernel in front of it (every optimizer workgroup waiting for its
        own segment's bucket parked the whole grid on the GPU meanwhile; that variant was
        measured slower and removed in round 6).
        """
        if self._opt_segments is None:
            self._opt_segments = self.optimizer_segments()
        segs = self._opt_segments if segments is None else segments
        red = self.reducer
        xg = {}
        if exchange:
            # xgmi streamed, in-launch exchange of bucket 1 (the conv slabs): its workgroups
            # all-reduce their sums themselves; every other workgroup waits for its bucket
            # from the persistent collective (long done by now: it ran beside cnn_bwd)
            xg = dict(xg=red.sync, signal_ch=-1, waits=red.waits_for(segs, exchanged=(1,)),
                      timeout_s=red.timeout_s, xchg=red._native,
                      xchg_bucket=red.channels_of(1)[0])
        elif red.streamed:
            waits = red.waits_for(segs)
            uniq = []
            for i in range(0, len(waits), 2):
                if waits[i] not in uniq[0::2]:
                    uniq += waits[i:i + 2]
            self.C.xgmi_wait(red.sync, signal_ch, uniq, red.timeout_s)
        o = self.opt
        g = o.param_groups[0]
        grads = self.reducer.out_grads       # the xgmi transport's result arena, or in place
        if o.kind == "adam":
            b1, b2 = g["betas"]
            self.C.optim_step(self.C.OPT_ADAM, self.arena.params, grads, o.exp_avg,
                              o.exp_avg_sq, o._lr_dev, o._step_dev, float(b1), float(b2),
                              float(g["eps"]), float(g["weight_decay"]), 0.0, 0.0, False,
                              float(self.reducer.grad_scale), segs, bump=bump, metrics=metrics,
                              **xg)
        else:
            self.C.optim_step(self.C.OPT_SGD, self.arena.params, grads,
                              o.momentum_buffer, None, o._lr_dev, o._step_dev, 0.0, 0.0, 0.0,
                              float(g["weight_decay"]), float(g["momentum"]),
                              float(g["dampening"]), bool(g["nesterov"]),
                              float(self.reducer.grad_scale), segs, bump=bump, metrics=metrics,
                              **xg)

    def invalidate_graphs(self) -> None:
        self.graphs.clear()
        self._opt_segments = None

    # -- prediction --------------------------------------------------------------
    def _predict_io(self, images_u8: torch.Tensor, labels):
        """Device inputs and fresh outputs of ``predict``: (images uint8 [N, 784], labels int32
        [N] or None, log_probs fp32 [N, 10], pred int32 [N], confusion int64 [10, 10] or None).
        The outputs are allocated here, so this must not run inside a graph capture."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("predict() allocates its outputs: call it outside a graph capture")
        dev = self.device
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 2 or images_u8.shape[1] != 784 \
                or images_u8.shape[0] < 1:
            raise ValueError("predict() takes uint8 images [N >= 1, 784], got "
                             f"{images_u8.dtype} {tuple(images_u8.shape)}")
        images = images_u8.to(dev).contiguous()
        n = images.shape[0]
        lab = None
        if labels is not None:
            if labels.numel() != n:
                raise ValueError(f"{labels.numel()} labels for {n} images")
            lab = labels.to(device=dev, dtype=torch.int32).contiguous()
        logp = torch.empty(n, 10, dtype=torch.float32, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev)
        conf = None if lab is None else torch.zeros(10, 10, dtype=torch.int64, device=dev)
        return images, lab, logp, pred, conf

    def predict(self, images_u8: torch.Tensor, labels=None):
        """(log_probs, pred, confusion | None) of any N >= 1 images, on the device; enqueued on
        the current stream (the caller synchronises before reading)."""
        raise NotImplementedError

    # -- test-time augmentation ----------------------------------------------------
    # rows per view gather and reduce launch: the whole 10,000-image test split in one (the
    # gathers take a workgroup per 64 rows, so 2048 rows would occupy 32 of the CUs; the CNN
    # programs' predict() walks its own 2048-row chunks inside); 13 MB of view rows at V = 32
    TTA_CHUNK = 16384

    def _tta_tables(self, spec):
        """The Q14 tables of `spec` on the device, uploaded once per spec (never in a capture)."""
        t = self._tta_table_cache.get(spec)
        if t is None:
            t = tuple(torch.from_numpy(a).to(self.device) for a in spec.tables())
            self._tta_table_cache[spec] = t
        return t

    def tta_view(self, images: torch.Tensor, start: int, b: int, v: int, spec, out=None,
                 scratch=None) -> torch.Tensor:
        """View `v` of the rows start .. start + b of the device images (uint8 [N, 784]): uint8
        [b, 784] on the device, data/augment.py's tta_view bit for bit.  View 0 is the rows
        themselves; the others come from the augmenting epoch gathers, asked for the rows
        `start + arange(b)` in epoch TTA_EPOCH + v, so a row's draw is that of its position in
        `images`.  out (uint8 [>= b * 784]) and scratch ((labels int32 [N], out_labels int32
        [>= b]): the gathers copy a label per row) are allocated here unless given."""
        from ..data.augment import MAX_TTA, TTA_EPOCH
        if not 0 <= v < MAX_TTA:
            raise ValueError(f"view {v} is outside 0..{MAX_TTA - 1}")
        n = images.shape[0]
        if not (0 <= start and b >= 1 and start + b <= n):
            raise ValueError(f"rows {start}..{start + b} are not rows of {n} images")
        if v == 0:
            return images[start:start + b]
        dev = self.device
        if out is None:
            out = torch.empty(b * 784, dtype=torch.uint8, device=dev)
        if scratch is None:
            scratch = (torch.zeros(n, dtype=torch.int32, device=dev),
                       torch.empty(b, dtype=torch.int32, device=dev))
        idx = torch.arange(start, start + b, dtype=torch.int32, device=dev)
        cosq, sinq, invz = self._tta_tables(spec)
        kw = dict(max_wgs=0, cosq=cosq, sinq=sinq, invz=invz, shift=spec.shift,
                  epoch=TTA_EPOCH + v, seed=spec.seed)
        if spec.elastic > 0.0:
            self.C.gather_epoch_elastic(images, scratch[0], idx, out, scratch[1],
                                        elastic_q=spec.elastic_q, **kw)
        else:
            self.C.gather_epoch_augment(images, scratch[0], idx, out, scratch[1], **kw)
        return out[:b * 784].view(b, 784)

    def predict_tta(self, images_u8: torch.Tensor, labels, ws, spec, views: int, chunk=None,
                    metrics=None):
        """predict() with test-time augmentation: (log_probs, pred, confusion | None) of any
        N >= 1 images, combined over `views` views per image (data/augment.py check_tta: 1..32,
        and an enabled `spec` for more than one).  Per chunk of `chunk` rows (default
        TTA_CHUNK) every view goes through this step's own predict() with the weight set `ws`
        (None: the training weights) and one tta_reduce launch (csrc/kernels/tta.hip) writes
        the chunk's slices of the outputs; with `metrics` (fp64 [3], needs labels) it also adds
        the evaluation sums (sum of -log_probs[y], correct, rows).  Allocates, so not inside a
        graph capture; nothing of the training step is touched."""
        from ..data.augment import check_tta
        views = check_tta(views, spec)
        chunk = self.TTA_CHUNK if chunk is None else int(chunk)
        if chunk < 1:
            raise ValueError(f"chunk must be >= 1, got {chunk}")
        images, lab, logp, pred, conf = self._predict_io(images_u8, labels)
        if metrics is not None and lab is None:
            raise ValueError("metrics need labels")
        n = images.shape[0]
        dev = self.device
        chunk = min(chunk, n)
        stack = torch.empty(views * chunk * 10, dtype=torch.float32, device=dev)
        out = torch.empty(chunk * 784, dtype=torch.uint8, device=dev)
        scratch = (torch.zeros(n, dtype=torch.int32, device=dev),
                   torch.empty(chunk, dtype=torch.int32, device=dev))
        for s in range(0, n, chunk):
            b = min(chunk, n - s)
            st = stack[:views * b * 10].view(views, b, 10)
            for v in range(views):
                x = self.tta_view(images, s, b, v, spec, out, scratch)
                st[v].copy_(self.predict(x, None, ws)[0])
            self.C.tta_reduce(st, None if lab is None else lab[s:s + b], logp[s:s + b],
                              pred[s:s + b], conf, metrics)
        return logp, pred, conf


class LinearStep(GpuStepBase):
    """Reference Net step.  world size 1: lin_train -> optim (the optimizer sums the
    per-workgroup gradient slabs itself and advances the data-step counter);
    world size > 1: lin_train -> lin_reduce -> [all-reduce] -> optim."""

    def __init__(self, prog, use_graphs):
        super().__init__(prog, use_graphs)
        nblk = (self.bfull + self.C.LIN_ROWS - 1) // self.C.LIN_ROWS
        self.slab = torch.zeros(nblk * self.C.LIN_SLAB, dtype=torch.float32, device=self.device)
        self.W = self.arena.param("fc.weight")
        self.b = self.arena.param("fc.bias")
        self.gW = self.arena.grad("fc.weight")
        self.gb = self.arena.grad("fc.bias")
        # world size 1 (no all-reduce between backward and update): the slab reduction runs
        # inside the optimizer launch (PDM_FUSE_LIN_REDUCE=0 disables)
        self.fuse_reduce = not self.reducer.active and self.structure.fuse_lin_reduce
        self._fused = {}

    def invalidate_graphs(self) -> None:
        super().invalidate_graphs()
        self._fused = {}

    def _fused_segments(self, nblk: int):
        segs = self._fused.get(nblk)
        if segs is None:
            C, spec = self.C, self.arena.spec
            sl = lambda col: (self.slab, nblk, col, C.LIN_SLAB)
            segs = [(spec.offset("fc.weight"), 10, 784, None, None, sl(0)),
                    (spec.offset("fc.bias"), 1, 10, None, None, sl(7840))]
            self._fused[nblk] = segs
        return segs

    def _train_impl(self, B: int) -> None:
        C = self.C
        C.lin_train(self.ep_images.view(-1, 784), self.ep_labels, None, self.ctr[0:1], self.bfull,
                    B, self.W, self.b, self.slab, self.metrics.train_view(), self.opt._step_dev,
                    spe=self.spe, lr_sched=self.lr_sched(), label_smoothing=self.label_smoothing)
        red = self.reducer
        # the step's train loss / correct partials sit in the slabs (columns 7850, 7851): the
        # launch that sums the gradient slabs adds them to the fp64 metrics in a fixed order
        nblk = (B + C.LIN_ROWS - 1) // C.LIN_ROWS
        mets = (self.slab, nblk, 10 * 784 + 10, C.LIN_SLAB, self.metrics.train_view())
        if self.fuse_reduce:
            self.launch_optimizer(self._fused_segments(nblk), bump=self.ctr[0:1], metrics=mets)
            return
        C.lin_reduce(self.slab, B, self.gW, self.gb, self.ctr[0:1],
                     red.sync if red.streamed else None, self.metrics.train_view())
        if red.streamed:
            # the optimizer publishes the bucket and waits for the persistent collective
            self.launch_optimizer(signal_ch=0)
            return
        red.bucket_ready(0)
        red.finalize()
        self.launch_optimizer()

    def weight_set(self, arena):
        return arena.param("fc.weight"), arena.param("fc.bias")

    def evaluate(self, ws=None) -> None:
        W, b = (self.W, self.b) if ws is None else ws
        self.C.lin_eval(self.test_images, self.test_labels, W, b, self.metrics.eval_view())

    def predict(self, images_u8, labels=None, ws=None):
        W, b = (self.W, self.b) if ws is None else ws
        images, lab, logp, pred, conf = self._predict_io(images_u8, labels)
        self.C.lin_predict(images, lab, W, b, logp, pred, conf)
        return logp, pred, conf
