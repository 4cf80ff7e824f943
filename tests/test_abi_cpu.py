"""CPU-only checks of the boundary: the C-ABI library loads and exports exactly
the symbols include/rgfm.h declares; descriptor-only entry points (no GPU work)
agree with the oracle's parameter counts; the product path fails loudly without
a HIP device."""
import ctypes
import os
import re

import pytest
import torch

from oracle import oracle as O
from helpers import make_module
from ratio_guided_multimodal_fm_amd import _lib

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_header_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    declared = set(re.findall(r"\b(rgfm_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.SIGNATURES)


def test_conv_kernel_table_follows_the_route_numbers():
    """CONV_KERNELS (csrc/rgfm_kernels.h) is indexed by RGFM_ROUTE_*: its names are include/rgfm.h's route names in
    index order -- the strings of _lib.ROUTES -- and every route has its own init and launch function."""
    hdr = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    routes = sorted((int(i), n.lower()) for n, i in re.findall(r"#define RGFM_ROUTE_(\w+) (\d+)", hdr) if n not in ("COUNT", "T2", "SLOTS"))
    assert tuple(n for _, n in routes) == _lib.ROUTES and [i for i, _ in routes] == list(range(len(_lib.ROUTES)))
    src = open(os.path.join(ROOT, "ratio_guided_multimodal_fm_amd", "csrc", "rgfm_kernels.h")).read()
    table = src[src.index("CONV_KERNELS[RGFM_ROUTE_COUNT] = {"):]
    rows = re.findall(r'\{"(\w+)", (conv_\w+_init), (launch_conv_\w+)\},\s*// RGFM_ROUTE_(\w+)', table[:table.index("};")])
    assert tuple(r[0] for r in rows) == _lib.ROUTES
    assert all(r[0] == r[3].lower() for r in rows)
    assert len({r[1] for r in rows}) == len({r[2] for r in rows}) == len(_lib.ROUTES)


def test_library_exports_every_symbol():
    L = _lib.lib()
    for name in _lib.SIGNATURES:
        assert hasattr(L, name), name
    assert L.rgfm_abi_version() == _lib.ABI_VERSION


@pytest.mark.parametrize("tag", ["unet28", "mnist32", "svhn"])
def test_unet_param_count(tag):
    m = make_module(tag)
    d = m._engine.desc()
    n = ctypes.c_size_t()
    assert _lib.lib().rgfm_unet_param_floats(ctypes.byref(d), ctypes.byref(n)) == 0
    assert n.value == sum(v.numel() for v in m.state_dict().values())
    assert n.value == O.unet_param_floats(O.desc_of(m))


@pytest.mark.parametrize("tag", ["ratio_ms", "ratio28"])
def test_ratio_param_count(tag):
    m = make_module(tag)
    d = m._engine.desc()
    n = ctypes.c_size_t()
    assert _lib.lib().rgfm_ratio_param_floats(ctypes.byref(d), ctypes.byref(n)) == 0
    assert n.value == sum(v.numel() for v in m.state_dict().values())


def test_bad_descriptor_is_an_error_code():
    d = _lib.UNetDesc()
    d.in_channels, d.img_size, d.model_channels, d.num_levels, d.num_res_blocks = 2, 32, 32, 2, 2
    n = ctypes.c_size_t()
    rc = _lib.lib().rgfm_unet_param_floats(ctypes.byref(d), ctypes.byref(n))
    assert rc == -1 and b"in_channels" in _lib.lib().rgfm_last_error()


def test_no_cpu_fallback():
    m = make_module("mnist32")
    with pytest.raises(_lib.RgfmError, match="no CPU path|HIP device"):
        m(torch.zeros(1, 1, 32, 32), torch.zeros(1))
    from ratio_guided_multimodal_fm_amd import CFMSchedule
    with pytest.raises(RuntimeError, match="no CPU path"):
        CFMSchedule().sample(m, 2, 2, device="cpu")


def test_state_dict_keys_match_reference_layout():
    """Key order/shape ABI: counts pinned by the reference import in make_golden.py."""
    assert len(make_module("mnist32").state_dict()) == 148
    assert len(make_module("svhn").state_dict()) == 208
    assert len(make_module("ratio_ms").state_dict()) == 102
    sd = make_module("svhn").state_dict()
    assert list(sd)[:6] == ["time_embed.0.weight", "time_embed.0.bias", "time_embed.2.weight",
                            "time_embed.2.bias", "input_conv.weight", "input_conv.bias"]
    assert "decoder_blocks.8.skip.weight" in sd and "upsamplers.1.conv.bias" in sd
