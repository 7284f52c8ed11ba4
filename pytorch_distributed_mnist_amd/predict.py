"""Inference from a saved checkpoint: per-sample log-probabilities, predicted classes and,
with labels, the confusion matrix.

    from pytorch_distributed_mnist_amd.predict import load_predictor
    p = load_predictor("checkpoints/model_best.pth.tar", "cnn")
    out = p.predict(images_u8, labels)        # uint8 [N, 28, 28] or [N, 784], torch or NumPy
    out.log_probs, out.pred, out.confusion

Only the checkpoint's ``state_dict`` (with ``ema=True``: its ``ema_state_dict``) is read (the reference's ``module.``-prefixed format,
``utils/checkpoint.py``): no optimizer state, no process group and no dataset are needed.  On
the GPU the images go through the evaluation forward and the prediction head kernels
(``csrc/kernels/predict.hip``), on the CPU through the torch reference forward.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import numpy as np
import torch

from .app import resolve_dtype
from .data.augment import AugmentSpec, check_tta
from .data.mnist import IMAGE_PIXELS, MnistSplit, NUM_CLASSES
from .models.specs import get_spec
from .optim.flat import build_optimizer
from .parallel.comm import LocalComm
from .parallel.dist import pick_device
from .parallel.reducer import GradReducer
from .runtime.arena import FlatArena
from .runtime.program import Prediction, TrainProgram
from .utils.checkpoint import load_checkpoint


class Predictor:
    """A model loaded for inference; ``predict`` may be called any number of times."""

    def __init__(self, program: TrainProgram):
        self.program = program
        self.arch, self.dtype, self.device = program.model, program.dtype, program.device

    def predict(self, images, labels=None) -> Prediction:
        """images: uint8 [N, 28, 28] or [N, 784] (raw pixels; normalisation happens inside), as
        a torch tensor or a NumPy array, N >= 1; labels: N class indices, optional.  Returns
        log_probs fp32 [N, 10], pred int64 [N] and confusion int64 [10, 10] (None without
        labels), on the host.  With test-time augmentation on (``load_predictor(tta=V,
        augment=spec)``) log_probs is the log of the mean probability over the V views."""
        return self.program.predict(images, labels)


def load_predictor(checkpoint_path: str, arch: str, device: str = "auto",
                   dtype: str = "auto", ema: bool = False, tta: int = 1,
                   augment: Optional[AugmentSpec] = None) -> Predictor:
    """Build ``arch`` ("linear" or "cnn") on ``device`` ("auto", "cuda" or "cpu") and load the
    checkpoint's weights -- with ``ema=True`` its averaged weights (``ema_state_dict``, written
    by runs with ``--ema-decay``; a checkpoint without them raises KeyError).  A checkpoint of
    another architecture raises the arena's ``load_state_dict`` error.

    ``tta`` (1..32) and ``augment`` (an ``AugmentSpec``): test-time augmentation, as ``--tta V``
    with the run's ``--aug-*`` flags -- ``predict`` combines ``tta`` views per image, view 0 the
    image itself and the others drawn with ``augment``'s ranges and seed for the row's position
    in ``images``.  ``tta > 1`` without an enabled spec raises ValueError."""
    tta = check_tta(tta, augment)
    dev = pick_device(0, device)
    spec = get_spec(arch)
    arena = FlatArena(spec, dev)
    checkpoint = load_checkpoint(checkpoint_path, map_location="cpu")
    if ema and "ema_state_dict" not in checkpoint:
        raise KeyError(f"checkpoint {checkpoint_path!r} holds no averaged weights "
                       "(no ema_state_dict): it was written without --ema-decay")
    arena.load_state_dict(checkpoint["ema_state_dict" if ema else "state_dict"])
    # the program wants an optimizer, a reducer and two splits: a stateless SGD, the
    # one-rank reducer and empty splits (nothing here trains or reads a dataset)
    opt = build_optimizer("sgd", arena, SimpleNamespace(lr=0.0, momentum=0.0, weight_decay=0.0))
    reducer = GradReducer(LocalComm(), arena.grads, spec.bucket_bounds(),
                          channels=spec.channel_bounds())
    empty = MnistSplit(torch.empty(0, IMAGE_PIXELS, dtype=torch.uint8),
                       torch.empty(0, dtype=torch.int64), "none")
    program = TrainProgram(arch, resolve_dtype(dtype, arch, dev), arena, opt, reducer, empty, empty,
                           batch_size=1, use_graphs=False, tta=tta, tta_augment=augment)
    if dev.type == "cuda":
        program.sync_fn = lambda what: torch.cuda.synchronize(dev)
    return Predictor(program)


def save_predictions(path: str, prediction: Prediction, labels) -> None:
    """Write ``path`` (a NumPy .npz with log_probs, pred, labels, confusion) atomically:
    temporary file in the same directory, then ``os.replace``, as checkpoints are."""
    import os
    import tempfile
    d = os.path.dirname(path) or "."
    os.makedirs(d, exist_ok=True)
    fd, tmp = tempfile.mkstemp(prefix=".tmp_pred_", dir=d)
    try:
        with os.fdopen(fd, "wb") as f:
            np.savez(f, log_probs=prediction.log_probs.numpy(), pred=prediction.pred.numpy(),
                     labels=torch.as_tensor(labels).to(torch.int64).cpu().numpy(),
                     confusion=prediction.confusion.numpy())
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def class_lines(confusion: torch.Tensor):
    """One line per class from a confusion matrix: ``class c: correct/count (pct%)``."""
    out = []
    for c in range(NUM_CLASSES):
        correct, count = int(confusion[c, c]), int(confusion[c].sum())
        out.append("class {}: {}/{} ({:.2f}%)".format(c, correct, count,
                                                     100.0 * correct / count if count else 0.0))
    return out
