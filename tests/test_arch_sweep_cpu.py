"""CPU pins of the float64 yardstick the architecture sweep (tests/test_gpu_arch_sweep.py) measures against: its output
against the reference-generated fixtures, its layer trace against the oracle's (same order, same shapes), and the oracle
and the library planning every descriptor of helpers.ARCH_SWEEP, the deepest one included."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from helpers import ARCH_SWEEP, GENERIC_UNETS, golden, make_generic_unet, make_module, make_sweep_unet, maxdiff
from unet_ref64 import cfg_of, forward64, params64
from ratio_guided_multimodal_fm_amd import _lib

TOL_EVAL = 1e-5
SHAPES = {"unet28": (1, 28, 28), "mnist32": (1, 32, 32), "svhn": (3, 32, 32)}


def _f64(m, x, t, trace=False):
    with torch.no_grad():
        return forward64(cfg_of(m), params64(m, requires_grad=False), x, t, trace=trace)


@pytest.mark.parametrize("tag", list(GENERIC_UNETS))
def test_float64_matches_reference_generic(tag):
    m, x, t = make_generic_unet(tag)
    assert maxdiff(_f64(m, x, t).numpy(), golden("unet_generic")[f"{tag}_out"]) < TOL_EVAL


@pytest.mark.parametrize("tag", ["unet28", "mnist32", "svhn"])
def test_float64_matches_reference_presets(tag):
    m = make_module(tag)
    g = golden(f"unet_layers_{tag}")
    x = torch.randn(2, *SHAPES[tag], generator=torch.Generator().manual_seed(77))
    for ti, tval in enumerate((0.0, 0.37)):
        v = _f64(m, x, torch.full((2,), tval))
        assert maxdiff(v.numpy(), g[f"t{ti}_output"]) < TOL_EVAL, (tag, ti)


@pytest.mark.parametrize("tag", ["a4", "a12"])
def test_float64_trace_matches_oracle_trace(tag):
    m, x, t = make_sweep_unet(tag, 3)
    v, acts = _f64(m, x, t, trace=True)
    ro, racts = O.unet_forward(O.desc_of(m), O.blob_of(m), x.numpy(), t.numpy(), trace=True)
    assert len(acts) == len(racts) == O.lib().ro_unet_num_activations(ctypes.byref(O.desc_of(m)))
    for i, (a, r) in enumerate(zip(acts, racts)):
        assert tuple(a.shape) == r.shape, (tag, i)
        d = maxdiff(a.numpy(), r)
        assert d < TOL_EVAL * max(1.0, float(np.abs(r).max())), (tag, i, d)
    assert acts[-1] is v
    assert maxdiff(v.numpy(), ro) < TOL_EVAL


@pytest.mark.parametrize("tag", list(ARCH_SWEEP))
def test_sweep_descriptors_are_accepted_and_counted(tag):
    m, _, _ = make_sweep_unet(tag, 1)
    n = ctypes.c_size_t()
    assert _lib.lib().rgfm_unet_param_floats(ctypes.byref(m._engine.desc()), ctypes.byref(n)) == 0
    assert n.value == sum(v.numel() for v in m.state_dict().values())
    assert O.unet_param_floats(O.desc_of(m)) == n.value


def test_oracle_plans_the_deepest_descriptor():
    """4 levels x 8 ResBlocks: 32 encoder and 36 decoder blocks, the most check_desc accepts."""
    m, x, t = make_sweep_unet("deep", 2)
    assert len(m.decoder_blocks) == 36 and len(m.encoder_blocks) == 32
    assert O.unet_param_floats(O.desc_of(m)) == sum(v.numel() for v in m.state_dict().values())
    ro = O.unet_forward(O.desc_of(m), O.blob_of(m), x.numpy(), t.numpy())
    assert maxdiff(ro, _f64(m, x, t).numpy()) < TOL_EVAL


def test_oracle_refuses_descriptors_beyond_the_limits():
    for kw in (dict(num_res_blocks=9), dict(num_levels=5), dict(num_res_blocks=0), dict(model_channels=288)):
        d = O.unet_desc(1, 32, 32, (1, 1, 1, 1), 2)
        for k, v in kw.items():
            setattr(d, k, v)
        assert O.unet_param_floats(d) == 0, kw
        assert O.lib().ro_unet_num_activations(ctypes.byref(d)) == 0, kw
