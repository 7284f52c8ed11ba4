"""Train-time augmentation on the host (data/augment.py): the Philox generator, the integer
transform against slicing and against an independent float64 bilinear reference, its
dependence on (seed, epoch, dataset index) alone, the --aug-* flags, and the CLI on CPU/gloo
(world-size invariance, resume)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import REPO, free_port

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.augment import (AugmentSpec, augment_batch, draw,
                                                        philox4x32_10)
from pytorch_distributed_mnist_amd.data.mnist import synthetic_split
from pytorch_distributed_mnist_amd.data.sampler import distributed_indices
from pytorch_distributed_mnist_amd.runtime.program import build_local_program


def _words(s):
    return [int(w, 16) for w in s.split()]


@pytest.mark.parametrize("counter,key,expected", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff",
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0",
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, expected):
    """Random123's Philox4x32-10 known-answer vectors."""
    out = philox4x32_10(np.array(_words(counter), dtype=np.uint64),
                        np.array(_words(key), dtype=np.uint64))
    assert out.dtype == np.uint32 and out.tolist() == _words(expected)


def test_philox_vectorised_matches_single():
    g = np.random.default_rng(0)
    ctr = g.integers(0, 2 ** 32, (50, 4), dtype=np.uint64)
    key = g.integers(0, 2 ** 32, (2,), dtype=np.uint64)
    out = philox4x32_10(ctr, key)
    for i in (0, 17, 49):
        assert out[i].tolist() == philox4x32_10(ctr[i], key).tolist()


def _noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 784), dtype=np.uint8)


def test_identity_when_all_ranges_zero():
    """S = R = Z = 0: A = 16384, B = 0, fx = fy = 0 -- the map is exactly the identity."""
    spec = AugmentSpec(0, 0.0, 0.0, seed=5)
    assert not spec.enabled
    img = _noise(256, 1)
    idx = np.random.default_rng(2).integers(0, 60000, 256)
    assert np.array_equal(augment_batch(img, idx, 3, spec), img)


def test_pure_shift_equals_slicing():
    """S = 3, R = Z = 0: every output is the zero-filled integer shift of its source by the
    sample's (dx, dy), built here by slicing."""
    spec = AugmentSpec(3, 0.0, 0.0, seed=11)
    n = 300
    img = _noise(n, 3)
    idx = np.random.default_rng(4).integers(0, 60000, n)
    out = augment_batch(img, idx, 2, spec).reshape(n, 28, 28)
    _, _, dx, dy = draw(idx, 2, spec)
    assert set(dx.tolist()) == set(range(-3, 4)) and set(dy.tolist()) == set(range(-3, 4))
    src = img.reshape(n, 28, 28)
    for i in range(n):
        ex = np.zeros((28, 28), dtype=np.uint8)
        a, b = int(dx[i]), int(dy[i])       # out[y, x] = src[y - dy, x - dx]
        ex[max(b, 0):28 + min(b, 0), max(a, 0):28 + min(a, 0)] = \
            src[i, max(-b, 0):28 + min(-b, 0), max(-a, 0):28 + min(-a, 0)]
        assert np.array_equal(out[i], ex), (i, a, b)


def _float_reference(img, idx, epoch, spec):
    """Independent float64 bilinear reference: the same theta_k, z_j, dx, dy, rotation about
    (13.5, 13.5), zero outside the image.  Returns unrounded float64 [N, 28, 28]."""
    n = img.shape[0]
    k, j, dx, dy = draw(idx, epoch, spec)
    theta = np.radians(spec.rotate * (2.0 * k - 1023.0) / 1023.0)
    z = 1.0 + spec.zoom * (2.0 * j - 63.0) / 63.0
    c, s = (np.cos(theta) / z)[:, None, None], (np.sin(theta) / z)[:, None, None]
    yy, xx = np.meshgrid(np.arange(28.0), np.arange(28.0), indexing="ij")
    cx, cy = (xx - 13.5)[None], (yy - 13.5)[None]
    sx = c * cx + s * cy + 13.5 - dx[:, None, None]
    sy = -s * cx + c * cy + 13.5 - dy[:, None, None]
    x0, y0 = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0, sy - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    pad = np.zeros((n, 30, 30), dtype=np.float64)      # one zero pixel all round
    pad[:, 1:29, 1:29] = img.reshape(n, 28, 28)
    rows = np.arange(n)[:, None, None]

    def p(ax, ay):
        return pad[rows, np.clip(ay + 1, 0, 29), np.clip(ax + 1, 0, 29)]

    return ((1 - fx) * (1 - fy) * p(x0, y0) + fx * (1 - fy) * p(x0 + 1, y0)
            + (1 - fx) * fy * p(x0, y0 + 1) + fx * fy * p(x0 + 1, y0 + 1))


@pytest.mark.parametrize("shift,rotate,zoom", [(0, 15.0, 0.0), (2, 15.0, 0.15), (4, 30.0, 0.25)])
def test_geometry_against_float64_bilinear(shift, rotate, zoom):
    """4000 white-noise images (the worst case for interpolation) against the float64
    reference: at most 3 grey levels apart.  The bound is the spec's: the source coordinate is
    off by <= 1/512 px (1/256-px rounding) + <= 0.002 px (Q14 matrix) per axis, times 255 per
    pixel of gradient on two axes, plus 0.5 for the final rounding: about 2.5."""
    spec = AugmentSpec(shift, rotate, zoom, seed=123)
    n = 4000
    img = _noise(n, 7)
    idx = np.random.default_rng(8).integers(0, 60000, n)
    out = augment_batch(img, idx, 1, spec)
    assert out.dtype == np.uint8 and out.shape == (n, 784)
    ref = _float_reference(img, idx, 1, spec).reshape(n, 784)
    err = np.abs(out.astype(np.float64) - ref).max()
    print(f"augment ({shift}, {rotate}, {zoom}): max |integer - float64| = {err:.3f}")
    assert err <= 3.0, err
    assert not np.array_equal(out, img)


def test_depends_on_seed_epoch_index_only():
    """The same (seed, epoch, index) gives the same bytes wherever the sample sits in the
    batch; changing any one of the three changes most samples."""
    spec = AugmentSpec(2, 10.0, 0.1, seed=9)
    n = 200
    img = _noise(n, 5)
    idx = np.random.default_rng(6).permutation(60000)[:n]
    base = augment_batch(img, idx, 4, spec)
    perm = np.random.default_rng(7).permutation(n)
    assert np.array_equal(augment_batch(img[perm], idx[perm], 4, spec), base[perm])
    assert np.array_equal(augment_batch(img[:7], idx[:7], 4, spec), base[:7])
    # torch in, torch out, the same bytes
    t = augment_batch(torch.from_numpy(img), torch.from_numpy(idx), 4, spec)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), base)
    for other in (augment_batch(img, idx, 5, spec),
                  augment_batch(img, idx, 4, AugmentSpec(2, 10.0, 0.1, seed=10)),
                  augment_batch(img, idx, 4, AugmentSpec(2, 10.0, 0.1, seed=9 + (1 << 32))),
                  augment_batch(img, idx + 1, 4, spec)):
        same = (other == base).all(axis=1).mean()
        assert same < 0.05, same


def test_tables_and_spec_validation():
    cosq, sinq, invz = AugmentSpec(0, 0.0, 0.0).tables()
    assert cosq.dtype == sinq.dtype == invz.dtype == np.int32
    assert cosq.shape == sinq.shape == (1024,) and invz.shape == (64,)
    assert (cosq == 16384).all() and (sinq == 0).all() and (invz == 16384).all()
    cosq, sinq, invz = AugmentSpec(0, 45.0, 0.5).tables()
    assert sinq[0] == -sinq[1023] == -round(np.sin(np.pi / 4) * 16384)
    assert invz[0] == 32768 and invz[63] == round(16384 / 1.5)
    for bad in (dict(shift=9), dict(shift=-1), dict(rotate=45.5), dict(rotate=-1.0),
                dict(zoom=0.6), dict(zoom=float("nan"))):
        with pytest.raises(ValueError):
            AugmentSpec(**bad)


def test_cli_flags(capsys):
    a = parse_args(["--aug-shift", "2", "--aug-rotate", "10", "--aug-zoom", "0.1",
                    "--aug-seed", "77"])
    assert (a.aug_shift, a.aug_rotate, a.aug_zoom, a.aug_seed) == (2, 10.0, 0.1, 77)
    a = parse_args(["--aug-shift", "8", "--aug-rotate", "45", "--aug-zoom", "0.5"])
    assert (a.aug_shift, a.aug_rotate, a.aug_zoom) == (8, 45.0, 0.5) and not hasattr(a, "aug_seed")
    a = parse_args([])
    for name in ("aug_shift", "aug_rotate", "aug_zoom", "aug_seed"):
        assert not hasattr(a, name)
    assert "aug" not in repr(a)
    for bad in (["--aug-shift", "9"], ["--aug-shift", "-1"], ["--aug-shift", "1.5"],
                ["--aug-rotate", "46"], ["--aug-rotate", "-0.5"], ["--aug-zoom", "0.51"],
                ["--aug-zoom", "-0.1"], ["--aug-zoom", "nan"], ["--aug-seed", "-1"],
                ["--aug-seed", str(2 ** 64)]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert "error: argument --aug-" in capsys.readouterr().err, bad


def test_aug_seed_defaults_to_seed():
    from pytorch_distributed_mnist_amd.data.augment import spec_from_args
    assert spec_from_args(parse_args([])) is None
    assert spec_from_args(parse_args(["--aug-seed", "4"])) is None       # no range: off
    assert spec_from_args(parse_args(["--aug-shift", "1"])).seed == 0
    assert spec_from_args(parse_args(["--aug-shift", "1", "--seed", "6"])).seed == 6
    s = spec_from_args(parse_args(["--aug-zoom", "0.2", "--seed", "6", "--aug-seed", "8"]))
    assert s == AugmentSpec(0, 0.0, 0.2, 8)


def test_set_train_indices_needs_the_epoch():
    """With a spec enabled the epoch number is required: the augmentation is never dropped
    silently.  With it, the CPU program trains on augment_batch's images."""
    train, test = synthetic_split(256, True), synthetic_split(64, False)
    spec = AugmentSpec(2, 10.0, 0.1, seed=1)
    p = build_local_program("linear", "fp32", "cpu", 64, train, test, augment=spec)
    idx = distributed_indices(len(train), 1, 0, 0)
    with pytest.raises(ValueError, match="epoch"):
        p.set_train_indices(idx)
    p.set_train_indices(idx, epoch=2)
    sel = idx[:64].to(torch.int64)
    assert torch.equal(p.train_images_cpu(sel), augment_batch(train.images[sel], sel, 2, spec))
    assert not torch.equal(p.train_images_cpu(sel), train.images[sel])
    p.train_epoch()
    # a spec with every range 0 is off: no epoch needed, the images pass through
    q = build_local_program("linear", "fp32", "cpu", 64, train, test,
                            augment=AugmentSpec(0, 0.0, 0.0, seed=1))
    q.set_train_indices(idx)
    assert q.augment is None and torch.equal(q.train_images_cpu(sel), train.images[sel])


def test_augmentation_changes_training_but_not_evaluation():
    train, test = synthetic_split(512, True), synthetic_split(128, False)
    idx = distributed_indices(len(train), 1, 0, 0)
    res = []
    for spec in (None, AugmentSpec(2, 10.0, 0.1, seed=1)):
        p = build_local_program("linear", "fp32", "cpu", 64, train, test, seed=3, augment=spec)
        res.append(p.evaluate()[0].average)
        p.set_train_indices(idx, epoch=0)
        p.train_epoch()
        res.append(p.arena.params.clone())
    assert res[0] == res[2]                         # same weights, same test pass
    assert not torch.equal(res[1], res[3])          # different training images


AUG = ["--aug-shift", "2", "--aug-rotate", "10", "--aug-zoom", "0.1"]


def _run_cli(args, cwd, timeout=300):
    env = dict(os.environ)
    env["PYTHONPATH"] = REPO + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(REPO, "multi_proc_single_gpu.py"), "--device", "cpu",
           "--backend", "gloo", "-i", f"tcp://127.0.0.1:{free_port()}", "--synthetic"] + args
    r = subprocess.run(cmd, cwd=cwd, env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.slow
def test_cli_world_size_invariance_with_augmentation(tmp_path):
    """World size 1 and 2 with the same --aug-* flags train on the same transformed samples:
    the same weights (tests/test_app_cpu.py's comparison), and not those of a run without."""
    dirs = [tmp_path / n for n in ("ws1", "ws2", "plain")]
    for d in dirs:
        d.mkdir()
    common = ["--epochs", "1", "--synthetic-size", "2048", "--seed", "11", "--arch", "linear"]
    _run_cli(common + AUG + ["--world-size", "1"], dirs[0])
    _run_cli(common + AUG + ["--world-size", "2"], dirs[1])
    _run_cli(common + ["--world-size", "1"], dirs[2])
    a, b, c = (torch.load(d / "checkpoints" / "checkpoint_0.pth.tar",
                          weights_only=True)["state_dict"] for d in dirs)
    for k in a:
        assert torch.allclose(a[k], b[k], atol=1e-6, rtol=0), (k, (a[k] - b[k]).abs().max())
    assert not torch.allclose(a["module.fc.weight"], c["module.fc.weight"], atol=1e-6, rtol=0)


def test_cli_resume_reproduces_uninterrupted_run(tmp_path):
    """Two epochs straight equal one epoch plus --resume for the second (the flags given
    again): the transforms depend on the epoch number, not on the process that draws them."""
    d1, d2 = tmp_path / "straight", tmp_path / "resumed"
    d1.mkdir()
    d2.mkdir()
    common = ["--synthetic-size", "2048", "--seed", "3"] + AUG
    straight = _run_cli(common + ["--epochs", "2"], d1)
    assert "aug_shift=2" in straight                # the Namespace line shows the given flags
    _run_cli(common + ["--epochs", "1"], d2)
    out = _run_cli(common + ["--epochs", "2", "--resume",
                             str(d2 / "checkpoints" / "checkpoint_0.pth.tar")], d2)
    ep = [l for l in out.splitlines() if l.startswith("Epoch:")]
    assert len(ep) == 1 and ep[0].startswith("Epoch: 1/2,")
    a = torch.load(d1 / "checkpoints" / "checkpoint_1.pth.tar", weights_only=True)
    b = torch.load(d2 / "checkpoints" / "checkpoint_1.pth.tar", weights_only=True)
    assert a["epoch"] == b["epoch"] == 2 and a["best_acc"] == b["best_acc"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(b["optimizer"]["state"][i][name])), \
                (i, name)
    # --evaluate ignores the flags
    ev = _run_cli(["--evaluate", "--resume", str(d1 / "checkpoints" / "checkpoint_1.pth.tar")]
                  + AUG, d1)
    line = [l for l in ev.splitlines() if l.startswith("test loss:")]
    ep1 = [l for l in straight.splitlines() if l.startswith("Epoch: 1/2")][0]
    assert len(line) == 1 and line[0].split("test loss: ")[1] == ep1.split("test loss: ")[1]
