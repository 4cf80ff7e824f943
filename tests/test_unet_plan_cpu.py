"""The U-Net plan (csrc/unet_plan.h: plan_unet, the one place in csrc/ that knows FlexibleUNet's topology) on the CPU:
the header alone compiled with the host compiler and -fsanitize=address,undefined into a stand-alone program
(tests/unet_plan_main.cpp), run once over every descriptor of the three presets, helpers.GENERIC_UNETS and
helpers.ARCH_SWEEP, and its printout compared with the CPU module and the float64 restatement (tests/unet_ref64.py):

  offsets    every parameter's blob offset and element count against the cumulative positions of state_dict(); the total
             against rgfm_unet_param_floats and the oracle's count;
  trace      the (C, S) table of the trace hooks against the shapes of forward64(..., trace=True) at batch 1;
  data flow  a small interpreter of the printed op list, built on unet_ref64's _gn / _conv / _linear, returns forward64's
             float64 output EXACTLY -- in0 / in1 / out, and with them the skip pairing, are what the forward computes;
  row FLOPs  the exact sum 2 * H_out * W_out * numel(weight) over the module's convs (integer-valued doubles).

The interpreter runs on every descriptor: the slowest float64 forward pairs at batch 1 (a256, a64, a48) take 0.2 - 0.4 s
on the CPU, so none needs a shape-only form of the check.
"""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from oracle import oracle as O
from helpers import ARCH_SWEEP, GENERIC_UNETS, make_generic_unet, make_module, make_sweep_unet
from ratio_guided_multimodal_fm_amd import _lib
from unet_ref64 import _conv, _gn, _linear, cfg_of, forward64, params64, timestep_embedding64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ratio_guided_multimodal_fm_amd", "csrc")
PRESETS = ("unet28", "mnist32", "svhn")
TAGS = PRESETS + tuple(GENERIC_UNETS) + tuple(ARCH_SWEEP)


def module_of(tag):
    if tag in PRESETS:
        return make_module(tag)
    return make_generic_unet(tag)[0] if tag in GENERIC_UNETS else make_sweep_unet(tag, 1)[0]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{tag: {"total", "flops", "tensors": [(C, S)], "ops": [dict], "params": [(op, name, offset, count)], "trace"}}"""
    cxx = shutil.which("g++")
    assert cxx, "the plan check needs the host g++"
    exe = str(tmp_path_factory.mktemp("plan") / "unet_plan")
    # (both sanitizer runtimes linked statically: the program does not depend on what the environment preloads)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC,
                           os.path.join(ROOT, "tests", "unet_plan_main.cpp"), "-o", exe])
    args = []
    for tag in TAGS:
        c = cfg_of(module_of(tag))
        mult = tuple(c["channel_mult"])
        args += [c["in_channels"], c["img_size"], c["model_channels"], len(mult), *(mult + (0,) * (4 - len(mult))),
                 c["num_res_blocks"]]
    out = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True, text=True)
    assert out.stderr == "", out.stderr
    table = {tag: dict(tensors=[], ops=[], params=[], trace=[]) for tag in TAGS}
    for line in out.stdout.splitlines():
        f = line.split()
        p, what, f = table[TAGS[int(f[0])]], f[1], f[2:]
        if what == "total":
            p["total"] = int(f[0])
        elif what == "flops":
            p["flops"] = float.fromhex(f[0])
        elif what == "tensor":
            assert int(f[0]) == len(p["tensors"])
            p["tensors"].append((int(f[1]), int(f[2])))
        elif what == "trace":
            p["trace"].append((int(f[0]), int(f[1])))
        elif what == "param":
            p["params"].append((int(f[0]), f[1], int(f[2]), int(f[3])))
        else:
            assert what == "op" and int(f[0]) == len(p["ops"])
            p["ops"].append(dict(zip(("idx", "in0", "in1", "out", "S", "block"), map(int, f[2:])), kind=f[1]))
    return table


def module_name(cfg, op):
    """state_dict prefix of the module an op runs ('' for the input conv and the output head, printed by full key)"""
    n_enc = len(cfg["channel_mult"]) * cfg["num_res_blocks"]
    k = op["block"]
    if op["kind"] == "RES":
        if k < n_enc:
            return f"encoder_blocks.{k}."
        return f"middle_block{k - n_enc + 1}." if k < n_enc + 2 else f"decoder_blocks.{k - n_enc - 2}."
    return {"DOWN": f"downsamplers.{op['idx']}.", "UP": f"upsamplers.{op['idx']}."}.get(op["kind"], "")


@pytest.mark.parametrize("tag", TAGS)
def test_offsets_are_the_state_dict_positions(plans, tag):
    m, p = module_of(tag), plans[tag]
    cfg = cfg_of(m)
    want, off = {}, 0
    for name, v in m.state_dict().items():
        want[name] = (off, v.numel())
        off += v.numel()
    got = {}
    for op, name, o, n in p["params"]:
        key = (module_name(cfg, p["ops"][op]) if op >= 0 else "") + name
        assert key not in got, key
        got[key] = (o, n)
    assert got == want
    n = ctypes.c_size_t()
    assert _lib.lib().rgfm_unet_param_floats(ctypes.byref(m._engine.desc()), ctypes.byref(n)) == 0
    assert p["total"] == off == n.value == O.unet_param_floats(O.desc_of(m))
    res = [o for o in p["ops"] if o["kind"] == "RES"]
    assert [o["block"] for o in res] == [o["idx"] for o in res] == list(range(len(res)))
    assert [o["kind"] for o in p["ops"]][::len(p["ops"]) - 1] == ["IN", "OUT"]


def interpret(p, cfg, sd, x, t):
    """The printed op list run in float64: each op reads tensors in0 (+ in1, concatenated behind it) and writes out."""
    emb = timestep_embedding64(t.to(torch.float64).reshape(-1).expand(x.shape[0]), cfg["model_channels"])
    emb = F.silu(_linear(F.silu(_linear(emb, sd, "time_embed.0")), sd, "time_embed.2"))
    T, v = {}, None
    for op in p["ops"]:
        kind, name = op["kind"], module_name(cfg, op)
        if kind == "IN":
            h = x.to(torch.float64)
        else:
            h = T[op["in0"]] if op["in1"] < 0 else torch.cat([T[op["in0"]], T[op["in1"]]], dim=1)
            assert op["in1"] < 0 or kind == "RES"
        assert h.shape[-1] == h.shape[-2] == op["S"]
        if kind == "IN":
            o = _conv(h, sd, "input_conv")
        elif kind == "DOWN":
            o = _conv(h, sd, name + "conv", stride=2)
        elif kind == "UP":
            o = _conv(F.interpolate(h, scale_factor=2, mode="nearest"), sd, name + "conv")
        elif kind == "RES":
            a = _conv(F.silu(_gn(h, sd, name + "norm1")), sd, name + "conv1")
            a = a + _linear(emb, sd, name + "time_mlp.1")[:, :, None, None]
            a = _conv(F.silu(_gn(a, sd, name + "norm2")), sd, name + "conv2")
            o = a + (_conv(h, sd, name + "skip") if name + "skip.weight" in sd else h)
        else:
            assert kind == "OUT" and op["out"] == -1 and v is None
            v = _conv(F.silu(_gn(h, sd, "out_norm")), sd, "out_conv")
            continue
        assert op["out"] not in T and tuple(o.shape[1:]) == (p["tensors"][op["out"]][0],) + (p["tensors"][op["out"]][1],) * 2
        T[op["out"]] = o
    assert len(T) == len(p["tensors"])
    return v


@pytest.mark.parametrize("tag", TAGS)
def test_trace_table_and_data_flow_are_the_float64_forwards(plans, tag):
    m, p = module_of(tag), plans[tag]
    cfg, sd = cfg_of(m), params64(m, requires_grad=False)
    x = torch.randn(1, cfg["in_channels"], cfg["img_size"], cfg["img_size"], generator=torch.Generator().manual_seed(5))
    t = torch.tensor([0.37])
    with torch.no_grad():
        v, acts = forward64(cfg, sd, x, t, trace=True)
        got = interpret(p, cfg, sd, x, t)
    assert p["trace"] == [(a.shape[1], a.shape[2]) for a in acts] and all(a.shape[2] == a.shape[3] for a in acts)
    assert len(p["trace"]) == O.lib().ro_unet_num_activations(ctypes.byref(O.desc_of(m)))
    assert got.dtype == torch.float64 and torch.equal(got, v)


@pytest.mark.parametrize("tag", TAGS)
def test_row_flops_are_the_convs_of_the_module(plans, tag):
    m = module_of(tag)
    cfg = cfg_of(m)
    levels, nrb, img = len(cfg["channel_mult"]), cfg["num_res_blocks"], cfg["img_size"]

    def out_size(name):  # of the conv `name`: the level of its module, from the module's index alone
        mod, _, k = name.partition(".")
        k = int(k.split(".")[0]) if k[:1].isdigit() else 0
        level = {"encoder_blocks": k // nrb, "decoder_blocks": levels - 1 - k // (nrb + 1), "downsamplers": k + 1,
                 "upsamplers": levels - 2 - k, "middle_block1": levels - 1, "middle_block2": levels - 1,
                 "input_conv": 0, "out_conv": 0}[mod]
        return img >> level

    want = sum(2 * out_size(k) ** 2 * v.numel() for k, v in m.state_dict().items() if v.dim() == 4)
    assert want < 2 ** 53 and plans[tag]["flops"] == float(want)
