"""CPU side of the training pass: the new C exports and their bindings, CFMSchedule.add_noise, the float64
restatement against the module's parameter layout, the dropout hook's geometry, and the train_flow CLI's arguments
and checkpoint format."""
import ctypes
import os

import numpy as np
import pytest
import torch

from helpers import GENERIC_UNETS, make_generic_unet, make_module
from unet_ref64 import cfg_of, forward64, params64
from ratio_guided_multimodal_fm_amd import _lib, train_flow
from ratio_guided_multimodal_fm_amd.utils.flow_utils import CFMSchedule

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TRAIN_EXPORTS = ("rgfm_unet_train_workspace_bytes", "rgfm_unet_forward_train", "rgfm_unet_backward",
                 "rgfm_unet_dropout_mask", "rgfm_unet_update_params")


def test_training_exports_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    L = _lib.lib()
    for name in TRAIN_EXPORTS:
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.rgfm_abi_version() == 3


def test_training_exports_reject_bad_arguments():
    L = _lib.lib()
    n = ctypes.c_size_t()
    assert L.rgfm_unet_train_workspace_bytes(None, 4, ctypes.byref(n)) == -1
    assert L.rgfm_unet_forward_train(None, None, None, 1, None, 4, 0.0, 0, None, 0, None) == -1
    assert L.rgfm_unet_backward(None, None, None, None, 4, None, 0, None) == -1
    assert L.rgfm_unet_dropout_mask(None, 0, 0, 0.1, 4, None) == -1
    assert L.rgfm_unet_update_params(None, None, 0, None) == -1


def test_add_noise_semantics():
    torch.manual_seed(0)
    x1 = torch.randn(6, 3, 8, 8)
    t = torch.rand(6)
    torch.manual_seed(1)
    xt, u = CFMSchedule().add_noise(x1, t)
    torch.manual_seed(1)
    x0 = torch.randn_like(x1)  # the one draw add_noise makes
    tt = t.view(6, 1, 1, 1)
    assert torch.equal(xt, (1 - tt) * x0 + tt * x1)
    assert torch.equal(u, x1 - x0)
    xt0, u0 = CFMSchedule().add_noise(x1, torch.zeros(6))
    assert torch.allclose(xt0 + u0, x1, atol=1e-6)  # x_t + (1 - t) u = x_1


@pytest.mark.parametrize("tag", ["unet28", "mnist32", "svhn"] + list(GENERIC_UNETS))
def test_float64_restatement_uses_every_parameter(tag):
    m = make_generic_unet(tag)[0] if tag in GENERIC_UNETS else make_module(tag)
    sd = params64(m)
    S, C = m.img_size, m.in_channels
    v = forward64(cfg_of(m), sd, torch.randn(1, C, S, S), torch.tensor([0.3]))
    assert v.shape == (1, C, S, S) and v.dtype == torch.float64
    v.square().sum().backward()
    assert all(p.grad is not None for p in sd.values())


def test_resblock_geometry_and_dropout_p():
    m = make_module("svhn")
    geo = m.resblock_geometry()
    assert len(geo) == len(m._resblocks()) == 6 + 2 + 9
    assert geo[0] == (32, 64) and geo[6] == (8, 128) and geo[-1] == (32, 64)
    assert m.dropout_p() == pytest.approx(0.1)
    m.middle_block1.dropout.p = 0.2
    with pytest.raises(ValueError):
        m.dropout_p()


def test_cli_arguments_and_defaults():
    a = train_flow.parse_args(["--preset", "svhn", "--data", "d.npy"])
    assert (a.epochs, a.batch_size, a.lr, a.seed, a.patience, a.save_every, a.resume) == (50, 128, 1e-4, 42, 10, 10, None)
    assert a.out_dir == "checkpoints"
    with pytest.raises(SystemExit):
        train_flow.parse_args(["--preset", "cifar", "--data", "d.npy"])
    assert {k: v[2] for k, v in train_flow.PRESETS.items()}["mnist32"] == "flow_mnist32"
    assert train_flow.PRESETS["svhn"][2] == "flow_svhn"


def test_cli_data_and_checkpoint_format(tmp_path):
    np.save(tmp_path / "ok.npy", np.zeros((3, 1, 32, 32), np.float32))
    torch.save(torch.zeros(3, 3, 32, 32), tmp_path / "ok.pt")
    assert train_flow.load_data(str(tmp_path / "ok.npy"), (1, 32, 32)).shape == (3, 1, 32, 32)
    assert train_flow.load_data(str(tmp_path / "ok.pt"), (3, 32, 32)).dtype == torch.float32
    with pytest.raises(ValueError):
        train_flow.load_data(str(tmp_path / "ok.npy"), (3, 32, 32))
    data = torch.arange(10.0).view(10, 1, 1, 1)
    seen = torch.cat([b["x"] for b in train_flow.batches(data, 4, torch.Generator().manual_seed(0))])
    assert sorted(seen.view(-1).tolist()) == list(range(10))
    m = make_module("mnist32")
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    ck = train_flow.checkpoint(3, m, opt, 0.25)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "best_loss"}
    torch.save(ck, tmp_path / "c.pth")
    from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
    fresh = make_module("mnist32")
    assert load_checkpoint(fresh, str(tmp_path / "c.pth")) == {"epoch": 3, "best_loss": 0.25}
