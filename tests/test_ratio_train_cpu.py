"""CPU side of the ratio estimators' training pass: the new C exports and their bindings, the float64 restatement
(tests/ratio_ref64.py) against torch's own BatchNorm / max-pool, the two losses against closed forms, and the
train_ratio CLI's arguments, pair construction and checkpoint format."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from helpers import make_module
from ratio_ref64 import ENCODERS, forward64, kind_of, params64
from ratio_guided_multimodal_fm_amd import _lib, train_ratio
from ratio_guided_multimodal_fm_amd.utils.losses import DiscriminatorLoss, RuLSIFLoss, get_ratio_loss
from ratio_guided_multimodal_fm_amd.utils.trainer import RatioTrainer

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
EXPORTS = ("rgfm_ratio_train_workspace_bytes", "rgfm_ratio_forward_train", "rgfm_ratio_backward",
           "rgfm_ratio_pool_choice", "rgfm_ratio_dropout_mask", "rgfm_ratio_update_params")
SHAPES = {"ratio_ms": ((1, 32, 32), (3, 32, 32)), "ratio28": ((1, 28, 28), (1, 28, 28))}


def test_exports_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    L = _lib.lib()
    for name in EXPORTS:
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.rgfm_abi_version() == 3


def test_exports_reject_null_arguments():
    L = _lib.lib()
    n = ctypes.c_size_t()
    assert L.rgfm_ratio_train_workspace_bytes(None, 4, ctypes.byref(n)) == -1
    assert L.rgfm_ratio_forward_train(None, None, None, None, 4, 1, 0.0, 0, None, None, 0, None) == -1
    assert L.rgfm_ratio_backward(None, None, None, None, None, 4, None, 0, None) == -1
    assert L.rgfm_ratio_pool_choice(None, None, 0, 0, 4, None) == -1
    assert L.rgfm_ratio_dropout_mask(None, 0, 0, 0.1, 4, None) == -1
    assert L.rgfm_ratio_update_params(None, None, 0, None) == -1


def _inputs(tag, B, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, *SHAPES[tag][0], generator=g), torch.randn(B, *SHAPES[tag][1], generator=g)


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
@pytest.mark.parametrize("training", [True, False])
def test_restatement_uses_every_parameter(tag, training):
    m = make_module(tag)
    sd = params64(m)
    x, y = _inputs(tag, 3)
    s = forward64(kind_of(m), sd, x, y, training)
    assert s.shape == (3,) and s.dtype == torch.float64
    s.square().sum().backward()
    for k, _ in m.named_parameters():
        assert sd[k].grad is not None, k


class _TorchEncoder(nn.Module):
    """An encoder of ENCODERS as plain torch.nn layers (nn.BatchNorm2d / GroupNorm, F.max_pool2d)."""

    def __init__(self, kind, e, in_ch, sd):
        super().__init__()
        self.prefix, self.layers = ENCODERS[kind][e]
        self.mods = nn.ModuleDict()
        for conv, norm, _ in self.layers:
            w = sd[f"{self.prefix}.{conv}.weight"]
            self.mods[conv] = nn.Conv2d(w.shape[1], w.shape[0], 3, padding=1)
            self.mods[norm] = nn.BatchNorm2d(w.shape[0]) if kind == "mnist_svhn" else nn.GroupNorm(8, w.shape[0])
        w = sd[f"{self.prefix}.fc.weight"]
        self.mods["fc"] = nn.Linear(w.shape[1], w.shape[0])
        self.double()
        self.mods.load_state_dict({k[len(self.prefix) + 1:]: v.detach() for k, v in sd.items() if k.startswith(self.prefix + ".")})

    def forward(self, h):
        for conv, norm, pool in self.layers:
            h = F.silu(self.mods[norm](self.mods[conv](h)))
            if pool:
                h = F.max_pool2d(h, 2)
        return self.mods["fc"](h.mean((2, 3)))


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
@pytest.mark.parametrize("training", [True, False])
def test_restatement_equals_torch_layers_with_true_argmax(tag, training):
    m = make_module(tag)
    kind = kind_of(m)
    sd = params64(m, requires_grad=False)
    x, y = _inputs(tag, 5, seed=1)
    encs = [_TorchEncoder(kind, e, img.shape[1], sd).train(training) for e, img in enumerate((x, y))]
    score_net = make_module(tag).score_net.double().eval()  # (dropout off: masks=None below)
    with torch.no_grad():
        feats = torch.cat([enc(img.double()) for enc, img in zip(encs, (x, y))], dim=1)
        want = score_net(feats).squeeze(-1)
        out = {}
        got = forward64(kind, sd, x, y, training, out=out)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))
    if kind == "mnist_svhn" and training:  # the buffers nn.BatchNorm2d itself left behind
        for enc in encs:
            for k, v in enc.mods.state_dict().items():
                if "running" in k or "num_batches" in k:
                    r = out["buffers"][f"{enc.prefix}.{k}"]
                    assert float((v.double() - r.double()).abs().max()) <= 1e-12, k
    else:
        assert out["buffers"] == {}


def test_losses_against_closed_forms():
    sr, sf = torch.tensor([0.0, math.log(3.0)]), torch.tensor([0.0, -math.log(3.0), math.log(3.0)])
    loss, met = DiscriminatorLoss()(sr, sf)
    # -log sigmoid: log 2 and log(4/3); -log(1 - sigmoid): log 2, log(4/3), log 4
    want = (math.log(2) + math.log(4 / 3)) / 2 + (math.log(2) + math.log(4 / 3) + math.log(4)) / 3
    assert float(loss) == pytest.approx(want, rel=1e-6)
    assert set(met) == {"loss", "acc_real", "acc_fake"}
    assert met["acc_real"] == pytest.approx(0.5) and met["acc_fake"] == pytest.approx(1 / 3)
    # RuLSIF with w = softplus(T): T = log(e^w - 1)
    inv = lambda w: math.log(math.expm1(w))  # noqa: E731
    sr, sf = torch.tensor([inv(2.0), inv(1.0)]), torch.tensor([inv(0.5), inv(0.5)])
    fn = RuLSIFLoss(alpha=0.2, lambda_penalty=0.1)
    loss, met = fn(sr, sf)
    mix = [2.0, 1.0, 0.5, 0.5]
    want = 0.5 * np.mean(np.square(mix)) - 1.5 + 0.1 * (np.mean(mix) - 1.0) ** 2
    assert float(loss) == pytest.approx(want, rel=1e-6)
    assert set(met) == {"loss", "mean_w_real", "mean_w_fake", "constraint_term"}
    assert met["mean_w_real"] == pytest.approx(1.5) and met["mean_w_fake"] == pytest.approx(0.5)
    assert met["constraint_term"] == pytest.approx(0.1 * 0.0, abs=1e-7)
    assert isinstance(get_ratio_loss("disc"), DiscriminatorLoss)
    r = get_ratio_loss("rulsif", alpha=0.3, lambda_penalty=0.5)
    assert (r.alpha, r.lambda_penalty) == (0.3, 0.5)
    assert (RuLSIFLoss().alpha, RuLSIFLoss().lambda_penalty) == (0.2, 0.1)
    with pytest.raises(ValueError):
        get_ratio_loss("kl")
    # differentiable in the scores
    s = torch.zeros(4, requires_grad=True)
    DiscriminatorLoss()(s[:2], s[2:])[0].backward()
    assert torch.allclose(s.grad, torch.tensor([-0.25, -0.25, 0.25, 0.25]))


def test_cli_arguments_and_defaults(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)  # (checkpoint_path creates ./checkpoints, as the reference's get_checkpoint_path does)
    a = train_ratio.parse_args(["--kind", "mnist_svhn", "--data", "d.npz"])
    assert (a.loss_type, a.epochs, a.batch_size, a.lr, a.real_fake_ratio, a.seed) == ("disc", 30, 128, 1e-4, 0.5, 42)
    assert (a.rulsif_alpha, a.lambda_penalty, a.transform_type, a.device) == (0.2, 0.1, "rotate90", "cuda")
    assert (train_ratio.PATIENCE, train_ratio.SAVE_EVERY) == (5, 10)
    with pytest.raises(SystemExit):
        train_ratio.parse_args(["--kind", "cifar", "--data", "d.npz"])
    with pytest.raises(SystemExit):
        train_ratio.parse_args(["--kind", "mnist28", "--data", "d.npz", "--loss_type", "kl"])
    a = train_ratio.parse_args(["--kind", "mnist28", "--data", "d.npz", "--loss_type", "rulsif", "--transform_type", "flip"])
    assert train_ratio.checkpoint_path(a, "best").replace(os.sep, "/").endswith("checkpoints/ratio_rulsif_flip_best.pth")


def test_pair_construction():
    label = torch.arange(4000) % 10
    for ratio in (0.5, 0.2):
        is_real, y_idx = train_ratio.make_pairs(label, ratio, torch.Generator().manual_seed(3))
        n = label.numel()
        assert abs(float(is_real.float().mean()) - ratio) <= 5 * math.sqrt(ratio * (1 - ratio) / n)
        same = label[y_idx] == label
        assert torch.equal(same, is_real.bool())  # real pairs share the label, fake pairs never do
    x = torch.arange(10.0).view(10, 1, 1, 1)
    label = torch.arange(10) % 2
    seen = torch.cat([b["x"] for b in train_ratio.batches(x, x.clone(), label, 4, 0.5, torch.Generator().manual_seed(0))])
    assert sorted(seen.view(-1).tolist()) == list(range(10))


def test_data_file_and_checkpoint_round_trip(tmp_path, monkeypatch):
    x, y = np.zeros((4, 1, 28, 28), np.float32), np.ones((4, 1, 28, 28), np.float32)
    np.savez(tmp_path / "ok.npz", x=x, y=y, label=np.array([0, 1, 0, 1]))
    torch.save({"x": torch.zeros(4, 1, 32, 32), "y": torch.zeros(4, 3, 32, 32), "label": torch.tensor([0, 1, 2, 3])}, tmp_path / "ok.pt")
    gx, gy, gl = train_ratio.load_pairs(str(tmp_path / "ok.npz"), (1, 28, 28), (1, 28, 28))
    assert gx.shape == (4, 1, 28, 28) and gy.dtype == torch.float32 and gl.dtype == torch.int64
    assert train_ratio.load_pairs(str(tmp_path / "ok.pt"), (1, 32, 32), (3, 32, 32))[1].shape == (4, 3, 32, 32)
    with pytest.raises(ValueError):
        train_ratio.load_pairs(str(tmp_path / "ok.npz"), (1, 32, 32), (3, 32, 32))
    np.savez(tmp_path / "one.npz", x=x, y=y, label=np.zeros(4, np.int64))
    with pytest.raises(ValueError):
        train_ratio.load_pairs(str(tmp_path / "one.npz"), (1, 28, 28), (1, 28, 28))
    # a plain state_dict under the reference's name, as sample.py / evaluate.py load it
    monkeypatch.chdir(tmp_path)
    m = make_module("ratio28")
    a = train_ratio.parse_args(["--kind", "mnist28", "--data", "ok.npz"])
    path = train_ratio.checkpoint_path(a, "best")
    assert path.replace(os.sep, "/") == "checkpoints/ratio_disc_rotate90_best.pth"
    torch.save(m.state_dict(), path)
    from ratio_guided_multimodal_fm_amd.models import RatioEstimator
    from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
    fresh = RatioEstimator()
    assert load_checkpoint(fresh, path) == {}
    assert all(torch.equal(v, fresh.state_dict()[k]) for k, v in m.state_dict().items())
    a = train_ratio.parse_args(["--kind", "mnist_svhn", "--data", "ok.pt", "--loss_type", "rulsif"])
    assert train_ratio.checkpoint_path(a, "epoch10") == "checkpoints/ratio_rulsif_mnist_svhn_epoch10.pth"


def test_dropout_p_and_trainer_interface():
    m = make_module("ratio_ms")
    assert m.dropout_p() == pytest.approx(0.1)
    m.score_net[3].p = 0.2
    with pytest.raises(ValueError):
        m.dropout_p()
    assert make_module("ratio28").dropout_p() == pytest.approx(0.1)

    class Tiny(nn.Module):  # a model without forward_train goes through __call__
        def __init__(self):
            super().__init__()
            self.w = nn.Parameter(torch.tensor(0.0))

        def forward(self, x, y):
            return self.w * (x - y).flatten(1).sum(1)

    t = Tiny()
    tr = RatioTrainer(t, DiscriminatorLoss(), torch.optim.SGD(t.parameters(), lr=0.1), "cpu")
    batch = {"x": torch.tensor([[1.0], [0.0]]), "y": torch.tensor([[0.0], [1.0]]), "is_real": torch.tensor([1, 0])}
    met = tr.train_epoch([batch])
    assert met["loss"] == pytest.approx(2 * math.log(2)) and float(t.w.detach()) > 0
    assert tr.evaluate([batch])["loss"] < met["loss"]
