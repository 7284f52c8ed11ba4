"""Elastic distortion on the host (data/augment.py, --aug-elastic): the spline weights, the
control draws and the field against a scalar re-implementation of the spec, its bounds (no
fold), an independent float64 reference, that elastic = 0 changes nothing, the dependence on
(seed, epoch, dataset index) alone, the CLI on CPU/gloo, and the built kernel's resources."""
import glob
import os

import numpy as np
import pytest
import torch

from conftest import REPO

from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.augment import (AugmentSpec, augment_batch, draw,
                                                        elastic_controls, elastic_field,
                                                        philox4x32_10, spec_from_args)

from test_augment_cpu import _noise, _run_cli


def _q(e):
    """The spec field that gives E = e exactly."""
    return e / 256.0


# ---------------------------------------------------------------- the spec, element by element

def _weights(f):
    return [(16 - f) ** 2, 256 + 32 * f - 2 * f * f, f * f]


def _scalar_controls(index, epoch, seed, e):
    """Section 1 of the spec for one sample, one Philox call per control point."""
    gx, gy = [], []
    for q in range(36):
        r = philox4x32_10(np.array([index & 0xFFFFFFFF, epoch, 2, q], dtype=np.uint64),
                          np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64))
        gx.append(((int(r[0]) >> 16) * (2 * e + 1) >> 16) - e)
        gy.append(((int(r[1]) >> 16) * (2 * e + 1) >> 16) - e)
    return gx, gy


def _scalar_field(g):
    """ex (or ey) of one sample's 36 control values, pixel by pixel: a list of 784 ints."""
    out = []
    for y in range(28):
        hy = 2 * y + 1
        cy0, wy = hy >> 4, _weights(hy & 15)
        for x in range(28):
            hx = 2 * x + 1
            cx0, wx = hx >> 4, _weights(hx & 15)
            s = 0
            for b in range(3):
                for a in range(3):
                    s += wy[b] * wx[a] * g[6 * (cy0 + b) + cx0 + a]
            assert abs(s) < 2 ** 31
            out.append((s + (1 << 17)) >> 18)         # Python's >> floors, as the spec's
    return out


def test_spline_weights_partition_unity():
    """The weights sum to 512 and are never negative, so a constant control field reproduces
    itself exactly, for every constant in -768..768."""
    for f in range(16):
        w = _weights(f)
        assert sum(w) == 512 and min(w) >= 0, (f, w)
    for c in range(-768, 769):
        for f in (1, 7, 15):                          # f is odd: 2 (x & 7) + 1
            for g in (1, 9, 15):
                s = sum(wy * wx * c for wy in _weights(g) for wx in _weights(f))
                assert (s + (1 << 17)) >> 18 == c, (c, f, g)
    # and at every pixel of the image
    assert _scalar_field([-768] * 36) == [-768] * 784
    assert _scalar_field([5] * 36) == [5] * 784


@pytest.mark.parametrize("e", [1, 256, 768])
def test_field_matches_scalar_spec(e):
    """elastic_controls and the (ex, ey) that augment_batch adds equal the scalar loops above
    for 50 samples; the output of augment_batch is the bilinear blend at the displaced
    coordinates (no affine part), pixel by pixel."""
    seed = (7 << 32) + 41
    spec = AugmentSpec(0, 0.0, 0.0, seed, _q(e))
    assert spec.elastic_q == e
    n = 50
    idx = np.random.default_rng(e).integers(0, 60000, n)
    gx, gy = elastic_controls(idx, 5, spec)
    ex, ey = elastic_field(idx, 5, spec)
    assert gx.shape == gy.shape == (n, 6, 6) and gx.dtype == gy.dtype == np.int64
    assert ex.shape == ey.shape == (n, 784)
    img = _noise(n, 11)
    out = augment_batch(img, idx, 5, spec)
    for i in range(n):
        sgx, sgy = _scalar_controls(int(idx[i]), 5, seed, e)
        assert gx[i].reshape(-1).tolist() == sgx and gy[i].reshape(-1).tolist() == sgy, i
        sex, sey = _scalar_field(sgx), _scalar_field(sgy)
        assert ex[i].tolist() == sex and ey[i].tolist() == sey, i
        if i < 5:
            for pix in range(784):
                sx = 256 * (pix % 28) + sex[pix]      # the identity map is 256 x exactly
                sy = 256 * (pix // 28) + sey[pix]
                x0, fx, y0, fy = sx >> 8, sx & 255, sy >> 8, sy & 255

                def p(xx, yy):
                    return int(img[i, yy * 28 + xx]) if 0 <= xx < 28 and 0 <= yy < 28 else 0

                o = ((256 - fx) * (256 - fy) * p(x0, y0) + fx * (256 - fy) * p(x0 + 1, y0)
                     + (256 - fx) * fy * p(x0, y0 + 1) + fx * fy * p(x0 + 1, y0 + 1) + 32768) >> 16
                assert int(out[i, pix]) == o, (i, pix)


@pytest.mark.parametrize("e", [2, 768])
def test_control_draws(e):
    """36 x 20,000 draws: every one in [-E, E], both ends drawn at E = 2, the mean within
    5 sigma of 0 (a uniform integer on [-E, E] has variance ((2E+1)^2 - 1) / 12)."""
    spec = AugmentSpec(0, 0.0, 0.0, 99, _q(e))
    gx, gy = elastic_controls(np.arange(20000), 1, spec)
    count = 36 * 20000
    for g in (gx, gy):
        assert g.size == count
        assert g.min() >= -e and g.max() <= e
        if e == 2:
            assert g.min() == -2 and g.max() == 2
            assert sorted(np.unique(g).tolist()) == [-2, -1, 0, 1, 2]
        sigma = np.sqrt(((2 * e + 1) ** 2 - 1) / 12.0 / count)
        assert abs(g.mean()) <= 5 * sigma, (g.mean(), sigma)
    assert not np.array_equal(gx, gy)


def test_bounds_and_no_fold():
    """E = 768, 4000 samples: |ex| <= E, neighbouring pixels differ by at most E/4 + 1 in x and
    in y, hence 256 + difference >= 63 > 0: the map never folds."""
    e = 768
    spec = AugmentSpec(0, 0.0, 0.0, 5, 3.0)
    idx = np.random.default_rng(1).integers(0, 60000, 4000)
    worst = 0
    for f in elastic_field(idx, 2, spec):
        f = f.reshape(-1, 28, 28)
        assert np.abs(f).max() <= e
        dx = np.abs(np.diff(f, axis=2)).max()
        dy = np.abs(np.diff(f, axis=1)).max()
        assert dx <= e // 4 + 1 and dy <= e // 4 + 1, (dx, dy)
        worst = max(worst, int(dx), int(dy))
        assert 256 + np.diff(f, axis=2).min() >= 63 and 256 + np.diff(f, axis=1).min() >= 63
    print(f"elastic E = 768: largest neighbour difference {worst} (bound {e // 4 + 1})")
    sd = np.concatenate([f.reshape(-1) for f in elastic_field(idx, 2, spec)]).std() / 256.0
    print(f"elastic A = 3: displacement standard deviation {sd:.3f} px")
    assert 0.8 < sd < 1.1


# ---------------------------------------------------------------- float64 reference

def _float_reference(img, idx, epoch, spec):
    """Independent float64 reference: test_augment_cpu's float inverse map (theta_k, z_j, dx,
    dy, rotation about (13.5, 13.5)), plus the float quadratic B-spline of the same control
    points (knots every 8 pixels, cell coordinate t = (x + 0.5) / 8), float bilinear sampling,
    zero outside the image.  Returns unrounded float64 [N, 28, 28]."""
    n = img.shape[0]
    k, j, dx, dy = draw(idx, epoch, spec)
    theta = np.radians(spec.rotate * (2.0 * k - 1023.0) / 1023.0)
    z = 1.0 + spec.zoom * (2.0 * j - 63.0) / 63.0
    c, s = (np.cos(theta) / z)[:, None, None], (np.sin(theta) / z)[:, None, None]
    yy, xx = np.meshgrid(np.arange(28.0), np.arange(28.0), indexing="ij")
    cx, cy = (xx - 13.5)[None], (yy - 13.5)[None]
    sx = c * cx + s * cy + 13.5 - dx[:, None, None]
    sy = -s * cx + c * cy + 13.5 - dy[:, None, None]

    gx, gy = (g.astype(np.float64) / 256.0 for g in elastic_controls(idx, epoch, spec))
    t = (np.arange(28.0) + 0.5) / 8.0
    cell = np.floor(t).astype(np.int64)
    u = t - cell
    basis = np.zeros((28, 6))                          # basis[x, control column]
    for a, w in enumerate(((1 - u) ** 2 / 2, (1 + 2 * u - 2 * u * u) / 2, u * u / 2)):
        basis[np.arange(28), cell + a] = w
    assert np.allclose(basis.sum(1), 1.0)
    sx = sx + np.einsum("yb,nba,xa->nyx", basis, gx, basis)
    sy = sy + np.einsum("yb,nba,xa->nyx", basis, gy, basis)

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


@pytest.mark.parametrize("shift,rotate,zoom,elastic", [(0, 0.0, 0.0, 2.0), (2, 15.0, 0.15, 3.0)])
def test_geometry_against_float64_reference(shift, rotate, zoom, elastic):
    """4000 white-noise images against the float64 reference: at most 4 grey levels apart --
    the affine test's bound of 3, plus 1: ex and ey are each within 0.5/256 px of the float
    spline, and white noise has a slope of at most 255 per pixel (2 x 255 x 0.5/256 < 1).
    Measured: 1.196 at (0, 0, 0, A = 2), 1.822 at (2, 15, 0.15, A = 3)."""
    spec = AugmentSpec(shift, rotate, zoom, 123, elastic)
    n = 4000
    img = _noise(n, 7)
    idx = np.random.default_rng(8).integers(0, 60000, n)
    out = augment_batch(img, idx, 1, spec)
    assert out.dtype == np.uint8 and out.shape == (n, 784)
    ref = _float_reference(img, idx, 1, spec).reshape(n, 784)
    err = np.abs(out.astype(np.float64) - ref).max()
    print(f"elastic ({shift}, {rotate}, {zoom}, {elastic}): max |integer - float64| = {err:.3f}")
    assert err <= 4.0, err
    # the spline itself: within 0.5/256 px of the float spline
    ex, _ = elastic_field(idx[:200], 1, spec)
    off = AugmentSpec(shift, rotate, zoom, 123)
    assert not np.array_equal(out, augment_batch(img, idx, 1, off))
    gx = elastic_controls(idx[:200], 1, spec)[0].astype(np.float64)
    t = (np.arange(28.0) + 0.5) / 8.0
    cell = np.floor(t).astype(np.int64)
    u = t - cell
    basis = np.zeros((28, 6))
    for a, w in enumerate(((1 - u) ** 2 / 2, (1 + 2 * u - 2 * u * u) / 2, u * u / 2)):
        basis[np.arange(28), cell + a] = w
    fl = np.einsum("yb,nba,xa->nyx", basis, gx, basis).reshape(200, 784)
    assert np.abs(ex - fl).max() <= 0.5 + 1e-9


# ---------------------------------------------------------------- off, and what a draw depends on

def test_elastic_zero_changes_nothing():
    """For test_gpu_augment's three settings, elastic = 0 gives the bits of a spec built
    without the field; the positional construction still works; elastic alone enables the
    spec; the range is validated."""
    img = _noise(300, 3)
    idx = np.random.default_rng(4).integers(0, 60000, 300)
    for args, seed in (((3, 0.0, 0.0), 21), ((0, 20.0, 0.0), (5 << 32) + 22),
                       ((2, 10.0, 0.1), 23)):
        old = AugmentSpec(*args, seed=seed)
        new = AugmentSpec(*args, seed=seed, elastic=0.0)
        assert old == new and old.elastic == 0.0 and old.elastic_q == 0
        for ep in (0, 3):
            assert np.array_equal(augment_batch(img, idx, ep, old), augment_batch(img, idx, ep, new))
    s = AugmentSpec(2, 10.0, 0.1, 23)
    assert (s.shift, s.rotate, s.zoom, s.seed, s.elastic) == (2, 10.0, 0.1, 23, 0.0)
    assert AugmentSpec(2, 10.0, 0.1, 23, 1.5).elastic == 1.5
    assert AugmentSpec(elastic=1.0).enabled and not AugmentSpec(elastic=0.0).enabled
    assert AugmentSpec(elastic=1.0).elastic_q == 256 and AugmentSpec(elastic=3.0).elastic_q == 768
    assert AugmentSpec(elastic=2).elastic == 2.0
    for bad in (3.5, -1.0, -0.001, float("nan")):
        with pytest.raises(ValueError):
            AugmentSpec(elastic=bad)
    # elastic = 0 with every other range 0 is the identity
    assert np.array_equal(augment_batch(img, idx, 1, AugmentSpec(0, 0.0, 0.0, 5, 0.0)), img)


def test_depends_on_seed_epoch_index_only():
    """A permuted batch gives the permuted output; another epoch or seed (either key word)
    gives different output; the affine draws do not move when elastic is turned on."""
    spec = AugmentSpec(2, 10.0, 0.1, 9, 2.0)
    n = 200
    img = _noise(n, 5)
    idx = np.random.default_rng(6).permutation(60000)[:n]
    base = augment_batch(img, idx, 4, spec)
    perm = np.random.default_rng(7).permutation(n)
    assert np.array_equal(augment_batch(img[perm], idx[perm], 4, spec), base[perm])
    assert np.array_equal(augment_batch(img[:7], idx[:7], 4, spec), base[:7])
    t = augment_batch(torch.from_numpy(img), torch.from_numpy(idx), 4, spec)
    assert isinstance(t, torch.Tensor) and np.array_equal(t.numpy(), base)
    for other in (augment_batch(img, idx, 5, spec),
                  augment_batch(img, idx, 4, AugmentSpec(2, 10.0, 0.1, 10, 2.0)),
                  augment_batch(img, idx, 4, AugmentSpec(2, 10.0, 0.1, 9 + (1 << 32), 2.0)),
                  augment_batch(img, idx + 1, 4, spec),
                  augment_batch(img, idx, 4, AugmentSpec(2, 10.0, 0.1, 9))):
        same = (other == base).all(axis=1).mean()
        assert same < 0.05, same
    # the control draws alone move with the epoch, the index and both key words
    g0 = elastic_controls(idx, 4, spec)[0]
    assert not np.array_equal(g0, elastic_controls(idx, 5, spec)[0])
    assert not np.array_equal(g0, elastic_controls(idx + 1, 4, spec)[0])
    assert not np.array_equal(g0, elastic_controls(idx, 4, AugmentSpec(seed=9 + (1 << 32),
                                                                       elastic=2.0))[0])
    # counter word 2 keeps the streams apart: the affine draws are the same with and without
    plain = AugmentSpec(2, 10.0, 0.1, 9)
    for a, b in zip(draw(idx, 4, spec), draw(idx, 4, plain)):
        assert np.array_equal(a, b)
    assert len(draw(idx, 4, spec)) == 4


# ---------------------------------------------------------------- the flag

def test_cli_flag(capsys):
    a = parse_args(["--aug-elastic", "2"])
    assert a.aug_elastic == 2.0 and not hasattr(a, "aug_shift")
    assert parse_args(["--aug-elastic", "3"]).aug_elastic == 3.0
    assert parse_args(["--aug-elastic", "0"]).aug_elastic == 0.0
    a = parse_args([])
    assert not hasattr(a, "aug_elastic") and "aug" not in repr(a)
    for bad in (["--aug-elastic", "3.5"], ["--aug-elastic", "-1"], ["--aug-elastic", "nan"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2, bad
        assert "error: argument --aug-elastic" in capsys.readouterr().err, bad


def test_spec_from_args():
    """--aug-elastic enables the augmentation on its own; --aug-seed defaults to --seed."""
    assert spec_from_args(parse_args(["--aug-elastic", "0"])) is None
    assert spec_from_args(parse_args(["--aug-elastic", "0", "--aug-seed", "4"])) is None
    assert spec_from_args(parse_args(["--aug-elastic", "1"])) == AugmentSpec(elastic=1.0)
    assert spec_from_args(parse_args(["--aug-elastic", "1", "--seed", "6"])).seed == 6
    s = spec_from_args(parse_args(["--aug-elastic", "2.5", "--aug-shift", "1", "--seed", "6",
                                   "--aug-seed", "8"]))
    assert s == AugmentSpec(1, 0.0, 0.0, 8, 2.5)
    assert spec_from_args(parse_args(["--aug-shift", "1"])) == AugmentSpec(1, 0.0, 0.0, 0)


COMMON = ["--synthetic-size", "2048", "--seed", "3"]
EL = ["--aug-elastic", "2"]


def _epochs(out):
    return [l for l in out.splitlines() if l.startswith("Epoch:")]


def _ckpt(d, i):
    return torch.load(d / "checkpoints" / f"checkpoint_{i}.pth.tar", weights_only=True)


def _same_checkpoint(a, b):
    assert a["epoch"] == b["epoch"] and a["best_acc"] == b["best_acc"]
    for k, v in a["state_dict"].items():
        assert torch.equal(v, b["state_dict"][k]), k
    for i, st in a["optimizer"]["state"].items():
        for name, v in st.items():
            assert torch.equal(torch.as_tensor(v),
                               torch.as_tensor(b["optimizer"]["state"][i][name])), (i, name)


@pytest.fixture(scope="module")
def cli_runs(tmp_path_factory):
    """The CPU/gloo runs the tests below share (test_augment_cpu's sizes): one epoch without
    the flag, with --aug-elastic 0 and with --aug-elastic 2, and two epochs with it."""
    root = tmp_path_factory.mktemp("elastic_cli")
    runs = {}
    for name, args in (("plain", ["--epochs", "1"]),
                       ("zero", ["--epochs", "1", "--aug-elastic", "0"]),
                       ("one", ["--epochs", "1"] + EL),
                       ("two", ["--epochs", "2"] + EL)):
        d = root / name
        d.mkdir()
        runs[name] = (d, _run_cli(COMMON + args, d))
    return runs


def test_cli_zero_equals_no_flag(cli_runs):
    """--aug-elastic 0 prints and checkpoints what the run without the flag does: every line
    of the output, but for the flag itself (and the rendezvous port) in the Namespace line."""
    import re
    (dp, plain), (dz, zero) = cli_runs["plain"], cli_runs["zero"]
    assert "aug_elastic=0.0" in zero and "aug_elastic" not in plain
    assert len(_epochs(plain)) == 1

    def norm(out):
        out = re.sub(r"init_method='[^']*'", "init_method=''", out)
        return re.sub(r", aug_elastic=0\.0", "", out).splitlines()

    assert norm(plain) == norm(zero)
    assert any(l.startswith("Namespace(") for l in norm(plain))
    _same_checkpoint(_ckpt(dp, 0), _ckpt(dz, 0))


def test_cli_elastic_changes_training_not_evaluation(cli_runs):
    (dp, plain), (d2, two) = cli_runs["plain"], cli_runs["two"]
    assert "aug_elastic=2.0" in two
    ep = _epochs(two)
    assert len(ep) == 2
    loss = lambda l: l.split("train loss: ")[1].split(",")[0]
    assert loss(ep[0]) != loss(_epochs(plain)[0])
    assert not torch.equal(_ckpt(dp, 0)["state_dict"]["module.fc.weight"],
                           _ckpt(d2, 0)["state_dict"]["module.fc.weight"])
    # --evaluate ignores the flag: the same test line with and without it, and it is the
    # training run's own test loss of that epoch
    ck = str(d2 / "checkpoints" / "checkpoint_1.pth.tar")
    lines = []
    for extra in (EL, []):
        out = _run_cli(["--evaluate", "--resume", ck] + extra, d2)
        line = [l for l in out.splitlines() if l.startswith("test loss:")]
        assert len(line) == 1
        lines.append(line[0])
    assert lines[0] == lines[1]
    assert lines[0].split("test loss: ")[1] == ep[1].split("test loss: ")[1]


def test_cli_resume_reproduces_uninterrupted_run(cli_runs):
    """Two epochs straight equal one epoch plus --resume for the second, the flag given again."""
    (d1, _), (d2, _) = cli_runs["one"], cli_runs["two"]
    _same_checkpoint(_ckpt(d1, 0), _ckpt(d2, 0))
    out = _run_cli(COMMON + EL + ["--epochs", "2", "--resume",
                                  str(d1 / "checkpoints" / "checkpoint_0.pth.tar")], d1)
    ep = _epochs(out)
    assert len(ep) == 1 and ep[0].startswith("Epoch: 1/2,")
    assert ep[0] == _epochs(cli_runs["two"][1])[1]
    _same_checkpoint(_ckpt(d1, 1), _ckpt(d2, 1))


@pytest.mark.slow
def test_cli_world_size_invariance(cli_runs, tmp_path):
    """World size 1 and 2 with --aug-elastic 2 train on the same distorted samples: the same
    weights, under test_augment_cpu's comparison."""
    _run_cli(COMMON + EL + ["--epochs", "1", "--world-size", "2"], tmp_path)
    a = _ckpt(cli_runs["one"][0], 0)["state_dict"]
    b = _ckpt(tmp_path, 0)["state_dict"]
    for k in a:
        assert torch.allclose(a[k], b[k], atol=1e-6, rtol=0), (k, (a[k] - b[k]).abs().max())
    c = _ckpt(cli_runs["plain"][0], 0)["state_dict"]
    assert not torch.allclose(a["module.fc.weight"], c["module.fc.weight"], atol=1e-6, rtol=0)


# ---------------------------------------------------------------- the built kernel

SO = sorted(glob.glob(os.path.join(REPO, "pytorch_distributed_mnist_amd", "_C*.so")))


@pytest.mark.skipif(not SO or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"),
                    reason="extension not built or ROCm llvm tools absent")
def test_kernel_resources():
    """The elastic gather runs beside cnn_bwd as the augmenting gather does: no LDS, no
    scratch.  The augmenting gather is still there, with no LDS either."""
    import sys
    sys.path.insert(0, os.path.join(REPO, "tools"))
    from kernel_resources import kernels as read
    ks = read(SO[0])
    el = {k: v for k, v in ks.items() if "gather_epoch_elastic_kernel" in k}
    au = {k: v for k, v in ks.items() if "gather_epoch_augment_kernel" in k}
    assert len(el) == 1 and len(au) == 1, (list(el), list(au))
    for v in el.values():
        assert v["group_segment_fixed_size"] == 0
        assert v.get("private_segment_fixed_size", 0) == 0
        assert v["vgpr_count"] + v.get("agpr_count", 0) <= 256    # two waves per SIMD
    for v in au.values():
        assert v["group_segment_fixed_size"] == 0
