"""Cases that put ONE stretch of a net's raw-staged tensors outside the window of the default two-plane fp16 conv
arithmetic (raw-staged values below 2048, every producer wave block's maximum at least 2^-8,
GroupNorm parameters inside norm_params_ok) while the rest of the net stays ordinary, and the float64 side of the tests
that run them (tests/test_range_cases_cpu.py, tests/test_gpu_range_guard.py).

The edit is a SCALE PAIR.  The producer of a residual-stream tensor -- a ResBlock's conv2 (and its 1x1 skip conv), a
Downsample / Upsample conv or input_conv -- is multiplied by f (weight and bias), and the weights of every conv that
reads that tensor raw by 1 / f: the next block's 1x1 skip (its input-channel slice), the Downsample / Upsample behind
it, and the slice of a decoder block's skip that reads a stored encoder copy.  A block with an identity skip passes a
large stream on (its output is targeted too: a chain) and swallows a small one (h + conv2(...) is ordinary again).
Readers behind a GroupNorm are scale-free up to the norm's eps.  f is a power of two except in the just-inside /
just-outside cases, whose windows are narrower than a factor of two.

Nothing is drawn at run time: seeds and factors are fixed below.  They were chosen on the CPU from the float64 trace
of the unedited nets (`python tests/range_cases.py` prints the table they were read from); tests/test_range_cases_cpu.py
checks every case's trace against the magnitudes its test relies on."""
import functools
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))  # (run as a script: print_table)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

from helpers import ARCH_SWEEP, make_sweep_unet  # noqa: E402
from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.synth import load_synth  # noqa: E402
from unet_ref64 import cfg_of, forward64, params64  # noqa: E402

HIGH, LOW = 1, 2  # the range flag's bits: a staged value too large / a producer's wave block too small

# descriptors of this file's own, as small as ARCH_SWEEP's: tag -> (FlexibleUNet kwargs, weight seed, data seed)
OWN_UNETS = {
    # 16 -> 8: Downsample on hx2s, Upsample 8 -> 16 as parity classes; the 8x8 level (64 channels) on hx2c with the
    # P-format hand-over to hx2d, its first block (32 -> 64) with the fused 1x1 skip on hx2d
    "r16": (dict(in_channels=1, img_size=16, model_channels=32, channel_mult=(1, 2), num_res_blocks=1), 131, 531),
    # 32 -> 16, three input channels: Downsample on hx2s; the 32-px level on hx2p over four full 8-row tiles per sample
    "r32": (dict(in_channels=3, img_size=32, model_channels=32, channel_mult=(1, 2), num_res_blocks=1), 132, 532),
    # 28 -> 14: ragged tiles (the !FULL scans of hx2p), skip blocks at both levels
    "r28": (dict(in_channels=1, img_size=28, model_channels=32, channel_mult=(1, 2), num_res_blocks=1), 133, 533),
}


def make_unet(tag, batch, device=None):
    """(module, x, t): ARCH_SWEEP[tag] as helpers.make_sweep_unet builds it, or OWN_UNETS[tag] the same way."""
    if tag in ARCH_SWEEP:
        return make_sweep_unet(tag, batch, device)
    cfg, wseed, dseed = OWN_UNETS[tag]
    m = load_synth(M.FlexibleUNet(**cfg), wseed).eval()
    x = torch.randn(batch, cfg["in_channels"], cfg["img_size"], cfg["img_size"], generator=torch.Generator().manual_seed(dseed))
    t = torch.linspace(0.0, 0.99, batch) if batch > 1 else torch.tensor([0.99])
    return (m.to(device) if device is not None else m), x, t


# ------------------------------------------------------------------ the scale pair
def topology(m):
    """The forward of a FlexibleUNet as [(module name, kind, streams read, stream written, trace index of the output)]:
    kind 'in' | 'res' | 'down' | 'up'; a decoder block reads (h, stored encoder copy) in the order of its concat.  The
    trace indices are forward64(..., trace=True)'s / UNetEngine.forward_trace's."""
    nrb, levels = m.num_res_blocks, len(m.channel_mult)
    ops, state = [("input_conv", "in", (), 0, 0)], dict(act=1, nxt=1)

    def op(name, kind, ins):
        state["act"] += 2 if kind == "res" else 1
        ops.append((name, kind, tuple(ins), state["nxt"], state["act"] - 1))
        state["nxt"] += 1
        return state["nxt"] - 1

    h, hs, bi = 0, [0], 0
    for level in range(levels):
        for _ in range(nrb):
            h = op(f"encoder_blocks.{bi}", "res", [h])
            hs.append(h)
            bi += 1
        if level < levels - 1:
            h = op(f"downsamplers.{level}", "down", [h])
            hs.append(h)
    h = op("middle_block1", "res", [h])
    h = op("middle_block2", "res", [h])
    bi = ui = 0
    for level in reversed(range(levels)):
        for _ in range(nrb + 1):
            h = op(f"decoder_blocks.{bi}", "res", [h, hs.pop()])
            bi += 1
        if level > 0:
            h = op(f"upsamplers.{ui}", "up", [h])
            ui += 1
    return ops


def _out_channels(mod, kind):
    return mod.out_channels if kind in ("in", "res") else mod.conv.out_channels


def scale_pair(m, producer, f):
    """Applies the scale pair in place (module on the CPU or a device): `producer`'s output times f, its raw readers'
    weights times 1 / f.  Returns (targeted, readers): the trace indices of the tensors that carry the factor and the
    names of the modules that read them raw (a ResBlock name = its fused 1x1 skip)."""
    f = float(f)
    scaled, chans, targeted, readers = set(), {}, [], []
    with torch.no_grad():
        for name, kind, ins, out, act in topology(m):
            mod = m.get_submodule(name)
            chans[out] = _out_channels(mod, kind)
            has_skip = kind == "res" and isinstance(mod.skip, nn.Conv2d)
            if name == producer:
                assert not any(i in scaled for i in ins)
                if kind == "res" and not has_skip and f < 1:
                    raise ValueError(f"{name} has an identity skip: its output cannot be made small (h is added back)")
                convs = [mod] if kind == "in" else [mod.conv] if kind != "res" else [mod.conv2] + ([mod.skip] if has_skip else [])
                for c in convs:
                    c.weight.mul_(f)
                    c.bias.mul_(f)
                scaled.add(out)
                targeted.append(act)
                continue
            if not any(i in scaled for i in ins):
                continue
            readers.append(name)
            if kind != "res":
                mod.conv.weight.mul_(1.0 / f)
            elif has_skip:
                off = 0
                for i in ins:
                    if i in scaled:
                        mod.skip.weight[:, off:off + chans[i]].mul_(1.0 / f)
                    off += chans[i]
            elif f > 1:  # identity skip: the large stream is passed on
                scaled.add(out)
                targeted.append(act)
    assert targeted, f"no such producer: {producer}"
    return targeted, readers


def block_maxima(a):
    """max |a| per (sample, 32-channel block) of an activation [B, C, H, W] (numpy): [B, ceil(C / 32)]."""
    a = np.abs(np.asarray(a, np.float64))
    return np.stack([a[:, c:c + 32].reshape(a.shape[0], -1).max(axis=1) for c in range(0, a.shape[1], 32)], axis=1)


def trace64(m, x, t):
    """(v, activations) of the module in float64 on its own (edited) weights, as numpy."""
    with torch.no_grad():
        v, acts = forward64(cfg_of(m), params64(m, requires_grad=False), x, t, trace=True)
    return v.numpy(), [a.numpy() for a in acts]


# ------------------------------------------------------------------ parts A and B: one stretch of one U-Net forward
# Route census of the UNEDITED nets in the default mode (one forward, 3 rows): the launches per route that each case's
# census is compared with, as EXPECT in tests/test_gpu_arch_sweep.py (whose entries for a96 and a224 are repeated).
# A key that is missing is not compared.  r16: the five ResBlocks of the 8x8 level (32 -> 64, two identity blocks,
# 128 -> 64, 96 -> 64) run conv1 on hx2c and conv2 behind the P-format hand-over on hx2d; r32: the same five at 16x16
# with 64 channels run conv1 on hx2p (the P-format producer there) and conv2 on hx2d.  hx2p: two convs per ResBlock and
# the Upsample, less the launches named on the other routes.
ROUTES = {
    "a96": dict(hx2p=25, hx2w=0, hx2s=0, hx2c=0, hx2d=0, hx2q=0, hx2=1, t2=0, bx3=0, f32=0),
    "a224": dict(hx2p=25, hx2w=0, hx2s=0, hx2c=0, hx2d=0, hx2q=0, hx2=1, t2=0, bx3=0, f32=0),
    "r16": dict(hx2p=7, hx2w=0, hx2s=1, hx2c=5, hx2d=5, hx2q=0, hx2=0, t2=1, bx3=0, f32=0),
    "r32": dict(hx2p=12, hx2w=0, hx2s=1, hx2c=0, hx2d=5, hx2q=0, hx2=0, t2=1, bx3=0, f32=0),
    "r28": dict(hx2p=17, hx2w=0, hx2s=0, hx2c=0, hx2d=0, hx2q=0, hx2=1, t2=1, bx3=0, f32=0),
}
# r32 at 256 rows: 1024 tiles at 32 px, so the six stride-1 launches of that level (encoder_blocks.0, decoder_blocks.2
# and .3: conv1 and conv2 each) move from hx2p to hx2q.  conv_hx2q_supported takes a fused 1x1 skip only with
# Cout % 64 != 0 at 32 px -- a64's 32-px level has 64 channels, its skip launches stay on hx2p at any batch.
ROUTES_R32_256 = dict(hx2w=0, hx2s=1, hx2c=0, hx2d=5, hx2q=6, hx2p=6, hx2=0, t2=1, bx3=0, f32=0)

LG_HIGH, LG_LOW = 12, -15  # the unedited streams of every net below have block maxima in [2, 10] (print_table)


def _case(net, producer, lg, route, rows=3, env=None, f=None, routes=None, **extra):
    return dict(net=net, producer=producer, f=float(f) if f is not None else 2.0 ** lg, bit=HIGH if (f or 2.0 ** lg) > 1 else LOW,
                route=route, rows=rows, env=env or {}, routes=routes, **extra)


# name -> case.  `route`: the route of the launch whose check must raise the bit -- high side: the launch that STAGES the
# targeted tensor raw; low side: the launch that PRODUCES it.  `isolated`: False where a launch of another route stages
# the same tensor (high side only: every Downsample input and every encoder tensor is also a stored encoder copy that a
# decoder block's fused skip reads on hx2p); tests/test_gpu_range_guard.py lists those in its docstring.
A_CASES = {
    # ---- high side
    "hi-skip-hx2p": _case("a96", "decoder_blocks.3", LG_HIGH, "hx2p"),              # 20 px, read by decoder_blocks.4 only
    "hi-skip-hx2d": _case("r16", "middle_block2", LG_HIGH, "hx2d"),                 # 8x8, read by decoder_blocks.0 only
    "hi-skip-hx2q": _case("r32", "decoder_blocks.2", LG_HIGH, "hx2q", rows=256, routes=ROUTES_R32_256),  # read by decoder_blocks.3 only
    "hi-down-hx2": _case("a224", "encoder_blocks.1", LG_HIGH, "hx2", isolated=False),   # 10 -> 5 (+ decoder_blocks.4)
    "hi-down-hx2s": _case("r16", "encoder_blocks.0", LG_HIGH, "hx2s", isolated=False),  # 16 -> 8 (+ decoder_blocks.2)
    "hi-up-nine": _case("a224", "decoder_blocks.2", LG_HIGH, "hx2p"),               # 5 -> 10 in nine taps
    "hi-up-t2": _case("r16", "decoder_blocks.1", LG_HIGH, "t2"),                    # 8 -> 16 as parity classes
    # ---- low side
    "lo-conv2-hx2p-full": _case("r32", "decoder_blocks.2", LG_LOW, "hx2p"),         # 32 px: four full 8-row tiles
    "lo-conv2-hx2p-ragged": _case("r28", "decoder_blocks.2", LG_LOW, "hx2p"),       # 28 px: the last tile is ragged
    "lo-conv2-hx2d": _case("r16", "decoder_blocks.0", LG_LOW, "hx2d"),              # 8x8 behind the P-format hand-over
    "lo-conv2-hx2q": _case("r32", "decoder_blocks.2", LG_LOW, "hx2q", rows=256, routes=ROUTES_R32_256),
    "lo-down-hx2": _case("a224", "downsamplers.0", LG_LOW, "hx2"),
    "lo-down-hx2s": _case("r16", "downsamplers.0", LG_LOW, "hx2s"),
    "lo-up-nine": _case("a224", "upsamplers.0", LG_LOW, "hx2p"),
    "lo-up-t2": _case("r16", "upsamplers.0", LG_LOW, "t2"),
    "lo-input-1ch": _case("r16", "input_conv", LG_LOW, None),
    "lo-input-3ch": _case("r32", "input_conv", LG_LOW, None),
    # weights x 2^-45: outside the fp16 path's weight window, so the producer runs on bx3 from create on; so does the
    # reader, whose skip slice is x 2^45 (routes: only what must hold is compared)
    "lo-conv2-bx3": _case("r28", "decoder_blocks.2", -45, "bx3", routes=dict(hx2w=0, hx2s=0, hx2c=0, hx2d=0, hx2q=0, hx2=1, t2=1, f32=0)),
}

# Part B: the same producers with the factor that puts the targeted tensor's float64 maximum at 1280 (inside: below
# 2048 by 1.6) and at 3584 (outside by 1.75).  "hx2c" of the issue is the 8x8 level here: conv_mfma_hx2c.hip never
# stages a raw tensor in the default dispatch (conv_hx2c_supported leaves the fused-skip launches to hx2p / hx2d).
B_HIGH = {
    "hx2p": ("a96", "decoder_blocks.3", 154.1, 431.5),
    "hx2d-8x8": ("r16", "middle_block2", 463.9, 1300.0),
    "hx2s": ("r16", "encoder_blocks.0", 443.4, 1241.0),
}
B_CASES = {}
for _k, (_net, _prod, _fin, _fout) in B_HIGH.items():
    B_CASES[f"inside-hi-{_k}"] = _case(_net, _prod, None, None, f=_fin, window=(1024.0, 1536.0), falls_back=False)
    B_CASES[f"outside-hi-{_k}"] = _case(_net, _prod, None, None, f=_fout, window=(3072.0, 4096.0), falls_back=True)
# just inside, low: every block maximum of the targeted tensor in [2^-7, 2^-5] (unedited: 6.5 .. 7.4)
B_CASES["inside-lo-hx2p"] = _case("r32", "decoder_blocks.2", -8, None, window=(2.0 ** -7, 2.0 ** -5), falls_back=None)


@functools.lru_cache(maxsize=None)
def unet_case(name):
    """(CPU module with the case's edit, x, t, targeted trace indices, readers, float64 v, float64 activations) --
    computed once, shared, never modified.  A 256-row case keeps the rows ROWS_256 on the float64 side."""
    c = {**A_CASES, **B_CASES}[name]
    m, x, t = make_unet(c["net"], c["rows"])
    targeted, readers = scale_pair(m, c["producer"], c["f"])
    idx = ROWS_256 if c["rows"] == 256 else list(range(c["rows"]))
    v, acts = trace64(m, x[idx], t[idx])
    return m, x, t, targeted, readers, v, acts


ROWS_256 = [0, 128, 255]  # eval-mode rows are independent: float64 runs these rows of a 256-row batch only


# ---- part B: one row of a batch out of range.  input_conv's bias is zeroed, so the first-level stream of a row is its
# input's scale times an ordinary one; nothing downstream is compensated (the GroupNorms renormalise the row).
ROW_CASES = {
    # name -> (net, batch, row, log2 of the row's input scale)
    "hi-row-r32-B5": ("r32", 5, 3, 12),
    "lo-row-r32-B5": ("r32", 5, 3, -16),
    "hi-row-a4-B66": ("a4", 66, 37, 12),   # 2x2 and 4x4 maps: several samples per wave block
    "lo-row-a4-B66": ("a4", 66, 37, -16),
}


@functools.lru_cache(maxsize=None)
def row_case(name):
    """(CPU module, x, t, row, float64 v, float64 input_conv output)."""
    net, batch, row, lg = ROW_CASES[name]
    m, x, t = make_unet(net, batch)
    with torch.no_grad():
        m.input_conv.bias.zero_()
    x = x.clone()
    x[row] *= 2.0 ** lg
    v, acts = trace64(m, x, t)
    return m, x, t, row, v, acts[0]


# ------------------------------------------------------------------ part C: the GroupNorm gate of a U-Net conv
# norm2 of r28's decoder_blocks.2 set to constants (gamma, beta); norm_params_ok wants hi = 8 max|gamma| + max|beta| <
# 1024 and lo = max(max|gamma|, max|beta|) >= 2^-6.  conv2's weights take `wscale` so that the block's output stays
# ordinary (the activation behind the norm is ~ beta): the gate is the only thing the case moves.
NORM_NET, NORM_BLOCK = "r28", "decoder_blocks.2"
NORM_CASES = {
    # name -> (gamma, beta, conv2 weight scale, inside the gate?)
    "hi-inside": (100.0, 223.9, 2.0 ** -8, True),    # hi = 1023.9
    "hi-outside": (100.0, 224.1, 2.0 ** -8, False),  # hi = 1024.1
    "lo-inside": (2.0 ** -6, 2.0 ** -6, 2.0 ** 6, True),
    "lo-outside": (2.0 ** -7, 2.0 ** -7, 2.0 ** 6, False),
}


def apply_norm_edit(m, name):
    """The NORM_CASES edit, in place on a module anywhere (a live handle sees it through update_params)."""
    gamma, beta, wscale, _ = NORM_CASES[name]
    blk = m.get_submodule(NORM_BLOCK)
    with torch.no_grad():
        blk.norm2.weight.fill_(gamma)
        blk.norm2.bias.fill_(beta)
        blk.conv2.weight.mul_(wscale)


@functools.lru_cache(maxsize=None)
def norm_case(name):
    """(CPU module with the edit, x, t, float64 v, float64 activations)."""
    m, x, t = make_unet(NORM_NET, 3)
    apply_norm_edit(m, name)
    v, acts = trace64(m, x, t)
    return m, x, t, v, acts


# ---- part A, the Winograd cell: a conv whose input is normalised stages S_A silu(gamma xhat + beta); the Winograd
# input transform adds up to four staged values, so conv_mfma_hx2w.hip tests 4 max against the fp16 limit where the
# direct kernels test max.  norm1 of a64's decoder_blocks.2 (16 px, 256 -> 128: a long-K layer RGFM_WINO=1 moves to
# hx2w) set to constants just under norm_params_ok's ceiling (hi = 8 * 60 + 520 = 1000 < 1024): the staged values are
# 16 (520 + 60 xhat) -- 4 max crosses 32760 from xhat = -0.14 on, max itself only at xhat = 25.  conv1's weights take
# 2^-8 so that its output stays ordinary.
WINO_NET, WINO_BLOCK = "a64", "decoder_blocks.2"
WINO_GAMMA, WINO_BETA, WINO_WSCALE = 60.0, 520.0, 2.0 ** -8


@functools.lru_cache(maxsize=None)
def wino_case():
    """(CPU module with the edit, x, t, float64 v, float64 activations, float64 silu(norm1(.)) of the edited block)."""
    import torch.nn.functional as F
    m, x, t = make_unet(WINO_NET, 3)
    blk = m.get_submodule(WINO_BLOCK)
    with torch.no_grad():
        blk.norm1.weight.fill_(WINO_GAMMA)
        blk.norm1.bias.fill_(WINO_BETA)
        blk.conv1.weight.mul_(WINO_WSCALE)
    v, acts = trace64(m, x, t)
    ops = topology(m)
    act_of = {out: act for _, _, _, out, act in ops}
    ins = next(i for name, _, i, _, _ in ops if name == WINO_BLOCK)
    cat = torch.cat([torch.from_numpy(acts[act_of[i]]) for i in ins], dim=1)
    with torch.no_grad():
        staged = F.silu(F.group_norm(cat, 8, blk.norm1.weight.double(), blk.norm1.bias.double(), eps=1e-5)).numpy()
    return m, x, t, v, acts, staged


# ------------------------------------------------------------------ part D: the guarded entry points
# The nets of tests/test_gpu_ode.py: g16 (1x16x16; ode_ref64.g16_case) as the x net and the target, g24 (3x24x24) as
# the y net.  g16 is the edited one: decoder_blocks.13 (16 px, 128 -> 64, read raw by decoder_blocks.14 alone) times
# 2^12 (bit 1) or 2^-15 (bit 2).  Start states: test_gpu_ode.py's seeds.
D_STEPS, D_GAMMA, D_B = 4, 0.7, 3
D_PRODUCER = "decoder_blocks.13"
D_LG = {HIGH: 12, LOW: -15}
D_TRACE_T = (0.0, 0.5, 0.875)  # where tests/test_range_cases_cpu.py looks at the edited net's trace
# the scale per stage of the 'pair-gs' entry: stage 1 (Euler) / stages 2 and 5 (midpoint) run unguided
D_STAGE_SCALE = {"euler": (1.0, 0.0, 0.5, 1.0), "midpoint": (1.0, 1.0, 0.0, 0.5, 1.0, 0.0, 0.5, 1.0)}
D_GAMMA_ROWS = (0.3, 0.7, 1.1)
# entry -> solvers.  The FlowMatchingModel loops and the graph replay (one case is asked for) are Euler only.
D_ENTRIES = {
    "single": ("euler", "midpoint"), "two": ("euler", "midpoint"), "two-same": ("euler", "midpoint"),
    "pair": ("euler", "midpoint"), "pair-mc": ("euler", "midpoint"), "pair-cross": ("euler", "midpoint"),
    "pair-gs": ("euler", "midpoint"), "pair-diag": ("euler", "midpoint"), "pair-graph": ("euler",),
    "pair-grad": ("euler", "midpoint"), "cond": ("euler", "midpoint"), "cond-grad": ("euler", "midpoint"),
}


@functools.lru_cache(maxsize=None)
def d_net(which):
    """CPU module: 'x' the unedited g16, 'y' g24, HIGH / LOW the edited g16.  Shared: deep-copy before moving it."""
    from helpers import make_generic_unet
    if which == "y":
        return make_generic_unet("g24")[0]
    m = make_generic_unet("g16")[0]
    if which in (HIGH, LOW):
        scale_pair(m, D_PRODUCER, 2.0 ** D_LG[which])
    return m


@functools.lru_cache(maxsize=None)
def d_flex():
    """FlexibleRatioEstimator for x = 1x16x16, y = 3x24x24 (tests/test_gpu_ode.py: flex)."""
    import cond_grad_ref64 as CG
    return load_synth(M.FlexibleRatioEstimator(1, 3, CG.FEAT, CG.HID), CG.W_SEED).eval()


@functools.lru_cache(maxsize=None)
def d_inputs():
    """Every input of the part D loops, fp32 on the CPU: shared, never modified."""
    import cond_grad_ref64 as CG
    g = torch.Generator().manual_seed(8100)
    d = dict(x0=torch.randn(D_B, 1, 16, 16, generator=torch.Generator().manual_seed(7130)),   # test_gpu_ode.start("g16", 3)
             y0=torch.randn(D_B, 3, 24, 24, generator=torch.Generator().manual_seed(7130)),   # ... start("g24", 3)
             x1=torch.randn(D_B, 1, 16, 16, generator=g))
    for n in (7, 5):
        d[f"mx{n}"], d[f"my{n}"] = 0.5 * torch.randn(n, 1, 16, 16, generator=g), 0.5 * torch.randn(n, 3, 24, 24, generator=g)
    d["r7"] = torch.exp(0.5 * torch.randn(7, generator=g))
    d["R5"] = torch.exp(0.5 * torch.randn(5, 5, generator=g))
    d["Rc"] = torch.exp(0.5 * torch.randn(D_B, 7, generator=g))
    d["rows"] = torch.tensor(D_GAMMA_ROWS)
    _, _, d["cond"], d["s0"] = CG.sampler_case("x")
    return d


def _f64(t):
    return t.numpy().astype(np.float64)


@functools.lru_cache(maxsize=None)
def d_want(entry, bit, solver):
    """float64 end state (tuple, in the order the entry returns its states) of a part D loop on the edited weights."""
    import cond_grad_ref64 as CG
    import guidance_cross_ref64 as XR
    import ode_ref64 as O
    import strength_ref64 as ST
    i = d_inputs()
    vx, vy = O.velocity_of(d_net(bit)), O.velocity_of(d_net("y"))
    run = lambda F, state: O.integrate64(F, tuple(_f64(s) for s in state), D_STEPS, solver)
    mx, my, r = _f64(i["mx7"]).reshape(7, -1), _f64(i["my7"]).reshape(7, -1), _f64(i["r7"])
    if entry == "single":
        out = run(O.F_single(vx), (i["x0"],))
    elif entry == "two":  # (fm_x = g24 unedited on y0, fm_y = the edited g16 on x0)
        out = run(O.F_single(vy), (i["y0"],)) + run(O.F_single(vx), (i["x0"],))
    elif entry == "two-same":
        out = run(O.F_single(vx), (i["x0"],)) + run(O.F_single(vx), (i["x1"],))
    elif entry == "pair":
        out = run(O.F_pair_mc(vx, vy, None, None, None, 0.0), (i["x0"], i["y0"]))
    elif entry in ("pair-mc", "pair-diag", "pair-graph"):
        out = run(O.F_pair_mc(vx, vy, mx, my, r, D_GAMMA), (i["x0"], i["y0"]))
    elif entry == "pair-cross":
        mx5, my5, R = _f64(i["mx5"]).reshape(5, -1), _f64(i["my5"]).reshape(5, -1), _f64(i["R5"])

        def F(s, t):  # (tests/test_gpu_guidance_cross.py: loop64)
            x, y = s
            ax, ay = np.asarray(vx(x, t), np.float64), np.asarray(vy(y, t), np.float64)
            if O.guided_after_eps(t):
                gx, gy = XR.cross64(x.reshape(D_B, -1), y.reshape(D_B, -1), ax.reshape(D_B, -1), ay.reshape(D_B, -1), mx5, my5, R, t, D_GAMMA)[:2]
                ax, ay = gx.reshape(x.shape), gy.reshape(y.shape)
            return ax, ay
        out = run(F, (i["x0"], i["y0"]))
    elif entry == "pair-gs":
        out = ST.integrate_rows64(*ST.pair_mc(vx, vy, mx, my, r), (_f64(i["x0"]), _f64(i["y0"])), D_GAMMA_ROWS, D_STEPS, solver,
                                  schedule=list(D_STAGE_SCALE[solver]))
    elif entry == "pair-grad":
        out = run(O.F_pair_grad(vx, vy, d_flex(), D_GAMMA), (i["x0"], i["y0"]))
    elif entry == "cond":
        out = run(O.F_cond_mc(vx, mx, _f64(i["Rc"]), D_GAMMA), (i["x0"],))
    elif entry == "cond-grad":
        out = run(O.F_cond_grad(vx, CG.sampler_case("x")[0], i["cond"], "x", D_GAMMA), (i["s0"],))
    else:
        raise KeyError(entry)
    for a in out:
        a.setflags(write=False)
    return out


# ---- FlowMatchingModel (parts D and F): decoder.fc1 times 2^lg; deconv1 stages its 7x7 output raw.  Unedited, the
# (sample, 32-channel block) maxima of that map are 2.0 .. 3.1 (seed 41, the rows below).
FM_SEED, FM_SEED_Y, FM_DATA_SEED = 41, 20, 8
FM_LG = {HIGH: 13, LOW: -16}
FM_T = (0.1, 0.5, 0.9)


@functools.lru_cache(maxsize=None)
def fm_net(which):
    """CPU FlowMatchingModel: HIGH / LOW the edited net (seed 41), 'x' the same unedited, 'y' the unedited partner."""
    m = load_synth(M.FlowMatchingModel(), FM_SEED_Y if which == "y" else FM_SEED).eval()
    if which in (HIGH, LOW):
        with torch.no_grad():
            m.decoder.fc1.weight.mul_(2.0 ** FM_LG[which])
            m.decoder.fc1.bias.mul_(2.0 ** FM_LG[which])
    return m


@functools.lru_cache(maxsize=None)
def fm_inputs():
    g = torch.Generator().manual_seed(FM_DATA_SEED)
    d = dict(x=torch.randn(3, 1, 28, 28, generator=g), t=torch.tensor(FM_T))
    d["y"] = torch.randn(3, 1, 28, 28, generator=g)
    d["mx"], d["my"] = 0.5 * torch.randn(7, 1, 28, 28, generator=g), 0.5 * torch.randn(7, 1, 28, 28, generator=g)
    d["r"] = torch.exp(0.5 * torch.randn(7, generator=g))
    return d


def fm_map64(m, x, t):
    """float64 output of decoder.fc1 as [B, 256, 7, 7] (fmnet_ref64.forward64 up to that Linear)."""
    import torch.nn.functional as F
    import fmnet_ref64 as FM
    sd = FM.params64(m, requires_grad=False)
    with torch.no_grad():
        h = x.double()
        for k, stride in enumerate(FM.ENCODER_STRIDES, 1):
            h = F.conv2d(h, sd[f"encoder.conv{k}.weight"], sd[f"encoder.conv{k}.bias"], stride=stride, padding=1)
            h = FM._gn_silu(h, sd, f"encoder.gn{k}")
        feat = F.linear(h.reshape(h.shape[0], -1), sd["encoder.fc.weight"], sd["encoder.fc.bias"])
        T_dim = sd["decoder.fc1.weight"].shape[1] - feat.shape[1]
        comb = torch.cat([feat, FM.time_embedding64(t.double().reshape(-1), T_dim)], dim=1)
        return F.linear(comb, sd["decoder.fc1.weight"], sd["decoder.fc1.bias"]).reshape(-1, 256, 7, 7).numpy()


@functools.lru_cache(maxsize=None)
def fm_want(what, bit):
    """float64: 'forward' v(x, t); 'single' / 'pair' the 4-step Euler loops (tuple of end states)."""
    import fmnet_ref64 as FM
    i = fm_inputs()
    sd, sdy = FM.params64(fm_net(bit), requires_grad=False), FM.params64(fm_net("y"), requires_grad=False)
    with torch.no_grad():
        if what == "forward":
            out = (FM.forward64(sd, i["x"], i["t"]).numpy(),)
        elif what == "single":
            out = (FM.euler64(sd, i["x"], D_STEPS).numpy(),)
        else:
            out = tuple(a.numpy() for a in FM.pair64(sd, sdy, i["x"], i["y"], i["mx"], i["my"], i["r"], D_STEPS, D_GAMMA))
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------ part E: the estimator inside the gradient loops
# BatchNorm kind (RatioEstimatorMNISTSVHN, "ms_64"): the BatchNorm behind encoder_svhn.conv2a times f (weight and bias),
# the weights of conv2b, which stages silu(that layer) raw inside the loops, times 1 / f.  NOT "an encoder's second
# conv", as first planned: both encoders' second convs sit in front of a max-pool, where the high edit saturates SiLU
# (every window of negative pre-activations ties at -0) and no data seed can meet the seed rule of
# tests/ratio_sweep_seeds.py; conv2a is the first layer whose reader is a conv and that no pool follows.  The edit changes
# the function (silu(f z) / f is not silu(z)), so the pools behind it route differently and the rows were searched again
# on the EDITED modules among the candidates 3100 .. 4099 of the "ms_" entries, one row at a time (eval-mode rows are
# independent): gap / dev 6.7 and 6.05 (high), 5.38 (low; the only candidate that reaches the rule's floor of 5).
E_MS_EDIT = ("encoder_svhn", "bn2a", "conv2b")
E_LG = {HIGH: 12, LOW: -16}
E_MS_SEEDS = {HIGH: (3416, 3294), LOW: (3493,)}
# GroupNorm kinds (their loops run the exact fp32 convs): the same edit on the last encoder layer, gn4 times f and the
# encoder's Linear times 1 / f -- the one layer behind every pool, so that the committed seeds keep their margins.
E_GN_EDIT = {"r28": ("encoder_x", "gn4", "fc"), "flex": ("encoder_y", "gn4", "fc")}


def _edit_estimator(rr, where, lg):
    enc = getattr(rr, where[0])
    with torch.no_grad():
        getattr(enc, where[1]).weight.mul_(2.0 ** lg)
        getattr(enc, where[1]).bias.mul_(2.0 ** lg)
        getattr(enc, where[2]).weight.mul_(2.0 ** -lg)
    return rr


def e_ms_inputs(bit):
    from helpers import sweep_ratio_inputs
    rows = [sweep_ratio_inputs("ms_64", 1, s)[:2] for s in E_MS_SEEDS[bit]]
    return torch.cat([r[0] for r in rows]), torch.cat([r[1] for r in rows])


@functools.lru_cache(maxsize=None)
def e_case(kind, loop, bit):
    """A case dict as grad_loop_ref64.pair_case / cond_case build it, on an edited estimator.  kind 'ms' | 'r28' | 'flex';
    loop 'pair' | 'cond' (given = 'x': the target is the y side; 'flex' has the cond loop of cond_grad_ref64 only)."""
    import cond_grad_ref64 as CG
    import grad_loop_ref64 as GL
    lg = E_LG[bit]
    if kind == "flex":
        assert loop == "cond"
        rr, net, cond, s0 = CG.sampler_case("x")
        rr = _edit_estimator(rr, E_GN_EDIT["flex"], lg)
        rkind, keys, nets, x, y = "flexible", ("g16",), (net,), cond, s0
    else:
        tag = "ms_64" if kind == "ms" else "r28_512"
        rkind = "mnist_svhn" if kind == "ms" else "mnist28"
        rr = _edit_estimator(GL.estimator(tag, "disc", 0), E_MS_EDIT if kind == "ms" else E_GN_EDIT["r28"], lg)
        x, y = e_ms_inputs(bit) if kind == "ms" else GL._inputs(tag, 5)
        keys = GL.UNETS[rkind] if loop == "pair" else GL.UNETS[rkind][1:]
        nets = tuple(GL.unet(k) for k in keys)
    sd = CG.params64(rr)
    if loop == "pair":
        s0s = (x, y)
        g64 = CG.grad_both64(rkind, sd, x, y, "disc")[:2]
        extra = {}
    else:
        s0s = (y,)
        g64 = (CG.grad_given64(rkind, sd, x, y, "x", "disc")[0],)
        extra = dict(cond=x, given="x")
    v64 = tuple(GL.velocity64(k, n, s) for k, n, s in zip(keys, nets, s0s))
    gamma = tuple(GL.gamma_of(float(g.abs().max())) for g in g64)
    rho = tuple(GL.rho_of(s, v, g, gm) for s, v, g, gm in zip(s0s, v64, g64, gamma))
    return dict(rr=rr, nets=nets, s0=s0s, g64=tuple(g64), v64=v64, gamma=gamma, rho=rho, **extra)


E_CASES = [("ms", "pair", HIGH), ("ms", "pair", LOW), ("ms", "cond", HIGH), ("ms", "cond", LOW),
           ("r28", "pair", HIGH), ("r28", "pair", LOW), ("flex", "cond", HIGH), ("flex", "cond", LOW)]


def e_staged64(bit):
    """float64 BatchNorm output of encoder_svhn.conv2a on the edited 'ms' estimator at its rows: what conv2b stages as
    S_A silu(.) inside the loops."""
    import torch.nn.functional as F
    import ratio_ref64 as RR
    import ratio_sweep_seeds as S
    rr = e_case("ms", "pair", bit)["rr"]
    sd = S.state(rr, torch.float64)
    _, y = e_ms_inputs(bit)
    h = y.double()
    with torch.no_grad():
        for conv, norm, pool in RR.ENCODERS["mnist_svhn"][1][1]:
            z = F.conv2d(h, sd[f"encoder_svhn.{conv}.weight"], sd[f"encoder_svhn.{conv}.bias"], padding=1)
            rm, rv = sd[f"encoder_svhn.{norm}.running_mean"], sd[f"encoder_svhn.{norm}.running_var"]
            z = (z - rm[None, :, None, None]) / torch.sqrt(rv[None, :, None, None] + S.EPS)
            z = z * sd[f"encoder_svhn.{norm}.weight"][None, :, None, None] + sd[f"encoder_svhn.{norm}.bias"][None, :, None, None]
            if norm == E_MS_EDIT[1]:
                return z.numpy()
            h = F.silu(z)
            if pool:
                h = RR.windows(h).max(-1).values
    raise AssertionError("layer not found")


def print_table():
    """The float64 magnitudes the factors above were read from: every stream of every net used, unedited."""
    for tag in ("r16", "r32", "r28", "a96", "a224", "a64", "a4"):
        m, x, t = make_unet(tag, 3)
        _, acts = trace64(m, x, t)
        print(f"== {tag}")
        for name, kind, ins, out, act in topology(m):
            bm = block_maxima(acts[act])
            print(f"  {name:20s} {kind:4s} reads {ins} trace {act:2d} {acts[act].shape[1:]} block maxima [{bm.min():.3g}, {bm.max():.3g}]")


if __name__ == "__main__":
    print_table()
