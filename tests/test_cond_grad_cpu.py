"""Conditional sampling with gradient log-ratio guidance, the parts that need no GPU: the library exports the new entry
points, the float64 restatement's factorised one-sided gradient IS the target half of the two-sided autograd gradient,
the sampler cases show the guidance term in float64 alone, and sample_conditional refuses an unknown guidance_method
before touching the device."""
import ctypes
import os

import pytest
import torch

import cond_grad_ref64 as CG
from helpers import make_module
from ratio_guided_multimodal_fm_amd import _lib
from ratio_guided_multimodal_fm_amd import models as M
from ratio_guided_multimodal_fm_amd.synth import load_synth
from ratio_guided_multimodal_fm_amd.utils.flow_utils import sample_conditional

NEW = ("rgfm_ratio_cond_prepare_workspace_bytes", "rgfm_ratio_cond_prepare", "rgfm_ratio_grad_cond_workspace_bytes",
       "rgfm_ratio_grad_log_ratio_cond", "rgfm_sample_cond_grad_workspace_bytes", "rgfm_sample_cond_grad")
TOL_SAMPLER = 1e-4


def test_library_exports_the_new_entry_points():
    """Every new symbol is in the _lib table, resolves in the built library, and the ABI version did not move."""
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    assert _lib.SIGNATURES["rgfm_ratio_cond_prepare"][1] == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert len(_lib.SIGNATURES["rgfm_ratio_grad_log_ratio_cond"][1]) == 10
    assert len(_lib.SIGNATURES["rgfm_sample_cond_grad"][1]) == 13
    assert os.path.exists(_lib.LIB_PATH), "build the library first (__graft_entry__.build())"
    h = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(h, name), name
    h.rgfm_abi_version.restype = ctypes.c_int
    assert h.rgfm_abi_version() == 3 == _lib.ABI_VERSION
    with open(os.path.join(os.path.dirname(_lib.LIB_PATH), "..", "..", "include", "rgfm.h")) as f:
        header = f.read()
    for name in NEW:
        assert f"int {name}(" in header, name


def _case(tag):
    if tag == "flexible":
        m = load_synth(M.FlexibleRatioEstimator(2, 3, 64, 128), 31).eval()
        g = torch.Generator().manual_seed(71)
        return m, torch.randn(3, 2, 12, 12, generator=g), torch.randn(3, 3, 20, 20, generator=g)
    m = make_module(tag)
    g = torch.Generator().manual_seed(72)
    sx, sy = ((1, 32, 32), (3, 32, 32)) if tag == "ratio_ms" else ((1, 28, 28), (1, 28, 28))
    return m, torch.randn(2, *sx, generator=g), torch.randn(2, *sy, generator=g)


@pytest.mark.parametrize("loss_type", ["disc", "rulsif"])
@pytest.mark.parametrize("tag", ["flexible", "ratio_ms", "ratio28"])
def test_factorised_one_sided_gradient_is_the_target_half(tag, loss_type):
    m, x, y = _case(tag)
    kind, sd = CG.kind_of(m), CG.params64(m)
    gx, gy, lr = CG.grad_both64(kind, sd, x, y, loss_type)
    for given, cond, target, want in (("x", x, y, gy), ("y", y, x, gx)):
        g, l = CG.grad_factorised64(kind, sd, cond, target, given, loss_type)
        a, la = CG.grad_given64(kind, sd, cond, target, given, loss_type)
        scale = float(want.abs().max())
        e1, e2 = float((g - want).abs().max()), float((a - want).abs().max())
        print(f"{tag} {loss_type} given={given}: factorised {e1:.2e} autograd-one-sided {e2:.2e} scale {scale:.2e}")
        assert e1 <= 1e-12 and e2 <= 1e-12, (e1, e2)
        assert float((l - lr).abs().max()) <= 1e-12 and float((la - lr).abs().max()) <= 1e-12
    # the context is what the header defines: W1[:, slice] f + b1
    ctx = CG.context64(kind, sd, x.double(), "x")
    F_ = m.feature_dim
    want = CG.features64(kind, sd, x.double(), 0) @ sd["score_net.0.weight"][:, :F_].T + sd["score_net.0.bias"]
    assert ctx.shape == (x.shape[0], m.hidden_dim) and float((ctx - want).abs().max()) <= 1e-12


@pytest.mark.parametrize("given", ["x", "y"])
def test_sampler_cases_show_the_guidance_term_in_float64(given):
    """The GPU test asks that the guided loop ends farther than 100 x TOL_SAMPLER from the unguided one: the float64
    loops of the chosen seeds are that far apart on their own (with TOL_SAMPLER to spare on each side)."""
    a, b = CG.sampler_loop64(given, CG.GAMMA_S), CG.sampler_loop64(given, 0.0)
    dist = float((a - b).abs().max())
    print(f"given={given}: float64 |guided - unguided| {dist:.3e}")
    assert dist > 100 * TOL_SAMPLER + 2 * TOL_SAMPLER, dist
    assert a.shape == CG.sampler_case(given)[3].shape and torch.isfinite(a).all()


def test_unknown_guidance_method_is_refused_before_the_device():
    """No tensor is moved and no library call is made: plain CPU tensors and modules are enough to get the error."""
    net, rr = make_module("unet28"), make_module("ratio28")
    cond = torch.zeros(2, 1, 28, 28)
    for bad in ("none", "mc", "grad", None):
        with pytest.raises(ValueError, match="guidance_method"):
            sample_conditional(net, rr, cond, "x", 2, 0.5, 3, guidance_method=bad)
    with pytest.raises(_lib.RgfmError, match="U-Net"):  # a FlowMatchingModel target is still refused, in either method
        sample_conditional(make_module("fm_original"), rr, cond, "x", 2, 0.5, 3, guidance_method="grad_log_ratio")
