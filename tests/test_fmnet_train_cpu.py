"""CPU side of FlowMatchingModel's training pass: the float64 restatement (tests/fmnet_ref64.py) against the
reference's autograd fixture, the new C exports and their bindings, and the train_flow CLI's `original` preset and
checkpoint names."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fmnet_ref64 import forward64, params64
from helpers import golden, make_module
from ratio_guided_multimodal_fm_amd import _lib, train_flow

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TOL_GRAD = 1e-4  # max |g - g_ref| <= TOL_GRAD * max |g_ref| per tensor (the project's training tolerance)
FMNET_TRAIN_EXPORTS = ("rgfm_fmnet_train_workspace_bytes", "rgfm_fmnet_forward_train", "rgfm_fmnet_backward",
                       "rgfm_fmnet_update_params")


def train_case(F_dim, T_dim, batch):  # must match tests/golden/make_fmnet_train_golden.py
    g = torch.Generator().manual_seed(900 + F_dim + T_dim + batch)
    return (torch.randn(batch, 1, 28, 28, generator=g), torch.rand(batch, generator=g),
            torch.randn(batch, 1, 28, 28, generator=g))


def test_float64_restatement_matches_reference_autograd():
    gold = golden("fmnet_train_grad")
    m = make_module("fm_original")
    x, t, target = train_case(256, 128, 2)
    sd = params64(m)
    x64 = x.double().requires_grad_(True)
    loss = F.mse_loss(forward64(sd, x64, t), target.double())
    loss.backward()
    assert abs(loss.item() - float(gold["loss"])) <= 1e-5 * abs(float(gold["loss"]))
    r = gold["dx"]
    assert np.abs(x64.grad.numpy() - r).max() <= TOL_GRAD * np.abs(r).max()
    names = [k for k, _ in m.named_parameters()]
    assert names == list(m.state_dict())  # no buffers: the gradient blob follows state_dict order
    for i, k in enumerate(names):
        gf = sd[k].grad.reshape(-1)
        idx = torch.randint(0, gf.numel(), (64,), generator=torch.Generator().manual_seed(7000 + i))
        amax = float(gold[f"amax_{i}"])
        assert abs(float(gf.abs().max()) - amax) <= TOL_GRAD * amax, k
        assert np.abs(gf[idx].numpy() - gold[f"probe_{i}"]).max() <= TOL_GRAD * amax, k


def test_reference_fp32_error_leaves_room_for_the_tolerance():
    """The GPU tests bound every gradient tensor by TOL_GRAD * max|g64|; the reference's own fp32 autograd must sit
    within a third of that for their cases, or the bound would have to come from 3 x ref32_err instead."""
    gold = golden("fmnet_train_grad")
    assert float(gold["ref32_err"]) == float(gold["ref32_err_cases"].max())
    assert float(gold["ref32_err"]) <= TOL_GRAD / 3


def test_float64_restatement_uses_every_parameter():
    m = make_module("fm_original")
    sd = params64(m)
    v = forward64(sd, torch.randn(1, 1, 28, 28), torch.tensor([0.3]))
    assert v.shape == (1, 1, 28, 28) and v.dtype == torch.float64
    v.square().sum().backward()
    assert all(p.grad is not None for p in sd.values())


def test_training_exports_declared_bound_and_built():
    hdr = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    L = _lib.lib()
    for name in FMNET_TRAIN_EXPORTS:
        assert name + "(" in hdr, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(L, name), name
    assert L.rgfm_abi_version() == 3


def test_training_exports_reject_bad_arguments():
    L = _lib.lib()
    n = ctypes.c_size_t()
    assert L.rgfm_fmnet_train_workspace_bytes(None, 4, ctypes.byref(n)) == -1
    assert L.rgfm_fmnet_forward_train(None, None, None, 1, None, 4, None, 0, None) == -1
    assert L.rgfm_fmnet_backward(None, None, None, None, 4, None, 0, None) == -1
    assert L.rgfm_fmnet_update_params(None, None, 0, None) == -1


def test_module_and_engine_offer_the_training_path():
    m = make_module("fm_original")
    assert callable(m.forward_train)
    assert callable(m._engine._fn("update_params"))  # (an optimizer step repacks the same handle)
    with pytest.raises(_lib.RgfmError, match="HIP device"):
        m.forward_train(torch.zeros(2, 1, 28, 28), torch.zeros(2))


def stems(*argv):
    return train_flow.parse_args([*argv, "--data", "d.npy"]).stem


def test_cli_original_preset_and_checkpoint_stems():
    assert train_flow.PRESETS["original"][1] == (1, 28, 28)
    assert stems("--preset", "original", "--modality", "x") == "flow_x"
    assert stems("--preset", "original", "--modality", "y") == "flow_y_rotate90"
    assert stems("--preset", "original", "--modality", "y", "--transform_type", "flip") == "flow_y_flip"
    assert stems("--preset", "original", "--modality", "x", "--transform_type", "flip") == "flow_x"
    # unet28: the same names with --modality, its own stem without
    assert stems("--preset", "unet28", "--modality", "x") == "flow_x"
    assert stems("--preset", "unet28", "--modality", "y") == "flow_y_rotate90"
    assert stems("--preset", "unet28") == "flow_unet28"
    assert stems("--preset", "mnist32") == "flow_mnist32"
    assert stems("--preset", "svhn") == "flow_svhn"
    a = train_flow.parse_args(["--preset", "original", "--modality", "x", "--data", "d.npy"])
    assert (a.epochs, a.batch_size, a.lr, a.transform_type) == (50, 128, 1e-4, "rotate90")
    with pytest.raises(SystemExit):
        train_flow.parse_args(["--preset", "original", "--data", "d.npy"])
    with pytest.raises(SystemExit):
        train_flow.parse_args(["--preset", "svhn", "--modality", "x", "--data", "d.npy"])
    with pytest.raises(SystemExit):
        train_flow.parse_args(["--preset", "original", "--modality", "z", "--data", "d.npy"])
