"""float64 torch.nn.functional restatement of FlexibleUNet (reference src/models/unet_flexible.py:39-261), written
from the architecture: the yardstick of the training-pass tests.  Takes the module's state_dict (any dtype / device;
evaluated in float64 on the CPU) and optionally the dropout keep masks the library reports (rgfm_unet_dropout_mask),
one per ResBlock in forward order."""
import math

import torch
import torch.nn.functional as F


def _gn(x, sd, name):
    return F.group_norm(x, min(8, x.shape[1]), sd[name + ".weight"], sd[name + ".bias"], eps=1e-5)


def _conv(x, sd, name, stride=1):
    w = sd[name + ".weight"]
    return F.conv2d(x, w, sd[name + ".bias"], stride=stride, padding=w.shape[-1] // 2)


def _linear(x, sd, name):
    return F.linear(x, sd[name + ".weight"], sd[name + ".bias"])


def timestep_embedding64(t, dim):
    half = dim // 2
    freqs = torch.exp(-math.log(10000) * torch.arange(half, dtype=torch.float64) / half)
    args = t[:, None] * freqs[None, :]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


def params64(module, requires_grad=True):
    """{name: float64 CPU leaf tensor} of the module's state_dict."""
    return {k: v.detach().to("cpu", torch.float64).clone().requires_grad_(requires_grad)
            for k, v in module.state_dict().items()}


def forward64(cfg, sd, x, t, masks=None, p_drop=0.0, trace=False):
    """v = FlexibleUNet(**cfg)(x, t) in float64; masks: list of keep masks (1 / 0) per ResBlock, or None.
    trace=True: (v, activations) with the activations in the order and shapes of UNetEngine.forward_trace and
    oracle.unet_forward(..., trace=True): input_conv, then per ResBlock conv1 + time term (before norm2) and the block's
    output, each Downsample / Upsample output, and v last."""
    x = x.to(torch.float64)
    t = t.to(torch.float64).reshape(-1)
    if t.numel() == 1:
        t = t.expand(x.shape[0])
    mc, mult, nrb = cfg["model_channels"], tuple(cfg["channel_mult"]), cfg["num_res_blocks"]
    blk = [0]
    acts = []

    def res(h, name, emb):
        a = _conv(F.silu(_gn(h, sd, name + ".norm1")), sd, name + ".conv1")
        a = a + _linear(F.silu(emb), sd, name + ".time_mlp.1")[:, :, None, None]
        acts.append(a)
        a = F.silu(_gn(a, sd, name + ".norm2"))
        if masks is not None:
            a = a * masks[blk[0]].to(torch.float64) / (1.0 - p_drop)
        blk[0] += 1
        a = _conv(a, sd, name + ".conv2")
        a = a + (_conv(h, sd, name + ".skip") if name + ".skip.weight" in sd else h)
        acts.append(a)
        return a

    emb = timestep_embedding64(t, mc)
    emb = _linear(F.silu(_linear(emb, sd, "time_embed.0")), sd, "time_embed.2")
    h = _conv(x, sd, "input_conv")
    acts.append(h)
    hs = [h]
    bi = 0
    for level in range(len(mult)):
        for _ in range(nrb):
            h = res(h, f"encoder_blocks.{bi}", emb)
            hs.append(h)
            bi += 1
        if level < len(mult) - 1:
            h = _conv(h, sd, f"downsamplers.{level}.conv", stride=2)
            acts.append(h)
            hs.append(h)
    h = res(h, "middle_block1", emb)
    h = res(h, "middle_block2", emb)
    bi = ui = 0
    for level in reversed(range(len(mult))):
        for _ in range(nrb + 1):
            h = res(torch.cat([h, hs.pop()], dim=1), f"decoder_blocks.{bi}", emb)
            bi += 1
        if level > 0:
            h = _conv(F.interpolate(h, scale_factor=2, mode="nearest"), sd, f"upsamplers.{ui}.conv")
            acts.append(h)
            ui += 1
    v = _conv(F.silu(_gn(h, sd, "out_norm")), sd, "out_conv")
    return (v, acts + [v]) if trace else v


def cfg_of(module):
    return dict(in_channels=module.in_channels, img_size=module.img_size, model_channels=module.model_channels,
                channel_mult=tuple(module.channel_mult), num_res_blocks=module.num_res_blocks)
