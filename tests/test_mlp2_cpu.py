"""--arch mlp2 off the GPU: the layout spec, the flags, the CPU / gloo path and the predictor."""
from types import SimpleNamespace

import pytest
import torch

from test_dropout_cpu import _run_cli, _weights
from pytorch_distributed_mnist_amd.config import parse_args
from pytorch_distributed_mnist_amd.data.mnist import normalize_reference, synthetic_split
from pytorch_distributed_mnist_amd.models.reference import MODULES
from pytorch_distributed_mnist_amd.models.specs import get_spec
from pytorch_distributed_mnist_amd.optim.flat import build_optimizer
from pytorch_distributed_mnist_amd.predict import load_predictor
from pytorch_distributed_mnist_amd.runtime.arena import FlatArena
from pytorch_distributed_mnist_amd.utils.checkpoint import make_state, save_checkpoint

MLP2 = ["--arch", "mlp2", "--optimizer", "sgd", "--lr", "0.05", "--batch-size", "64",
        "--synthetic-size", "256", "--dropout", "0.2", "--seed", "11"]
KEYS = ["module.fc%d.%s" % (i, k) for i in (1, 2, 3) for k in ("weight", "bias")]
HYPER = SimpleNamespace(lr=1e-3, momentum=0.9, weight_decay=0.0)


def test_layout_roundtrip_with_optimizer_state():
    """torch -> arena -> torch for the weights and the Adam state; one bucket in backward-ready
    order (fc1.weight last), 256-B aligned, torch's own layouts."""
    torch.manual_seed(0)
    m, spec = MODULES["mlp2"](), get_spec("mlp2")
    assert [p.name for p in spec.params] == ["fc3.weight", "fc3.bias", "fc2.bias", "fc2.weight",
                                             "fc1.bias", "fc1.weight"]
    assert spec.bucket_bounds() == [(0, spec.total)] and all(o % 64 == 0 for o in spec.offsets)
    arena = FlatArena(spec, "cpu")
    arena.load_module(m)
    sd = arena.state_dict()
    assert list(sd) == KEYS == ["module." + k for k in m.state_dict()]
    assert all(torch.equal(sd["module." + k], v) for k, v in m.state_dict().items())
    assert torch.equal(arena.param("fc2.weight"), m.fc2.weight.detach())
    opt = build_optimizer("adam", arena, HYPER)
    arena.grads.copy_(torch.randn(spec.total))
    opt.step_cpu()
    other = build_optimizer("adam", FlatArena(spec, "cpu"), HYPER)
    other.load_state_dict(opt.state_dict())
    for name in ("fc1.weight", "fc2.weight", "fc3.bias"):
        assert torch.equal(other.arena.view_of(other.exp_avg, name), arena.view_of(opt.exp_avg, name))
        assert arena.view_of(opt.exp_avg, name).abs().sum() > 0


def test_flags(capsys):
    a = parse_args(["--arch", "mlp2", "--dropout", "0.2", "--mixup", "0.4", "--dtype", "fp32"])
    assert a.arch == "mlp2" and a.dropout == 0.2 and a.mixup == 0.4
    for bad in (["--arch", "mlp2", "--dtype", "bf16"], ["--arch", "linear", "--dropout", "0.2"],
                ["--arch", "linear", "--mixup", "0.4"]):
        with pytest.raises(SystemExit) as e:
            parse_args(bad)
        assert e.value.code == 2 and "error: argument " + bad[2] in capsys.readouterr().err


@pytest.mark.slow
def test_two_epochs_world_sizes_and_resume(tmp_path):
    """Two CPU epochs with dropout: world size 2 trains world size 1's weights, one epoch +
    --resume equals the uninterrupted run bit for bit; the six tensors load into the module."""
    dirs = [tmp_path / n for n in ("ws1", "ws2", "resumed")]
    for d in dirs:
        d.mkdir()
    out = _run_cli(MLP2 + ["--epochs", "2", "--world-size", "1"], dirs[0])
    assert sum(l.startswith("Epoch:") for l in out.splitlines()) == 2
    _run_cli(MLP2 + ["--epochs", "2", "--world-size", "2"], dirs[1])
    _run_cli(MLP2 + ["--epochs", "1"], dirs[2])
    _run_cli(MLP2 + ["--epochs", "2", "--resume",
                     str(dirs[2] / "checkpoints" / "checkpoint_0.pth.tar")], dirs[2])
    a, b, c = (_weights(d, "checkpoint_1.pth.tar")["state_dict"] for d in dirs)
    assert list(a) == KEYS and tuple(a["module.fc2.weight"].shape) == (128, 128)
    for k in a:
        assert torch.allclose(a[k], b[k], atol=1e-6, rtol=0), (k, (a[k] - b[k]).abs().max())
        assert torch.equal(a[k], c[k]), k
    MODULES["mlp2"]().load_state_dict({k[len("module."):]: v for k, v in a.items()})


def test_load_predictor_equals_the_module(tmp_path):
    torch.manual_seed(3)
    m, arena = MODULES["mlp2"](), FlatArena(get_spec("mlp2"), "cpu")
    arena.load_module(m)
    save_checkpoint(make_state(1, arena, 0.0, build_optimizer("sgd", arena, HYPER)), False, 0,
                    directory=str(tmp_path))
    test = synthetic_split(37, False)
    out = load_predictor(str(tmp_path / "checkpoint_0.pth.tar"), "mlp2", device="cpu").predict(
        test.images, test.labels)
    with torch.no_grad():
        ref = torch.log_softmax(m(normalize_reference(test.images)), 1)
    assert torch.allclose(out.log_probs, ref, atol=1e-6, rtol=0)
    assert torch.equal(out.pred, ref.argmax(1)) and out.confusion.sum() == 37
