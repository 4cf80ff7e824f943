"""float64 yardstick of class-conditional U-Nets and classifier-free guidance (tests/test_cfg_cpu.py, tests/test_gpu_cfg.py).

Nothing new is restated here: everything is COMPOSED from the pinned float64 pieces.

* The labelled net.  emb = time_embed(timestep_embedding(t)) + E[y] and time_embed ends in a Linear, so for rows that
  share a label c the labelled net is the unlabelled `unet_ref64.forward64` with E[c] added to ``time_embed.2.bias`` in a
  copy of the parameter dict.  A mixed batch is evaluated per class group and the rows are put back in place; the
  gradient of ``label_emb.weight`` comes from autograd through that sum.  y = None is the null label K in every row.
* CFG loops are `ode_ref64.integrate64` with F = v_u + w (v_c - v_u), v_c at the rows' labels, v_u at the null label.

`direct64` restates the labelled forward in ten lines ON ONE TINY NET SHAPE (one level, one ResBlock per stage, no
Downsample / Upsample): tests/test_cfg_cpu.py pins the composition against it.
"""
import numpy as np
import torch
import torch.nn.functional as F

import ode_ref64 as O
import unet_ref64 as U

EMB = "label_emb.weight"


def forward_labels64(cfg, sd, x, t, y=None, masks=None, p_drop=0.0):
    """v = FlexibleUNet(**cfg, num_classes=K)(x, t, y) in float64; sd: the float64 parameter dict with `EMB` [K + 1, temb]
    (leaf tensors: gradients flow to every entry, EMB included).  y: integer labels [B] in 0..K, or None (all K)."""
    E = sd[EMB]
    K = E.shape[0] - 1
    x = x.to(torch.float64)
    B = x.shape[0]
    t = t.to(torch.float64).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    y = torch.full((B,), K, dtype=torch.long) if y is None else torch.as_tensor(y).long().reshape(-1).cpu()
    assert y.shape[0] == B and int(y.min()) >= 0 and int(y.max()) <= K
    base = {k: v for k, v in sd.items() if k != EMB}
    out = [None] * B
    for c in sorted(set(y.tolist())):
        rows = torch.nonzero(y == c).reshape(-1)
        sdc = dict(base)
        sdc["time_embed.2.bias"] = base["time_embed.2.bias"] + E[c]
        m = None if masks is None else [mk[rows] for mk in masks]
        v = U.forward64(cfg, sdc, x[rows], t[rows], m, p_drop)
        for j, r in enumerate(rows.tolist()):
            out[r] = v[j]
    return torch.stack(out)


def params64(module, requires_grad=True):
    return U.params64(module, requires_grad)


def velocity_labels_of(net, y):
    """v(x [B, C, H, W] float64 numpy, t) of a class-conditional module at the labels y (None: the null label)."""
    cfg, sd = U.cfg_of(net), U.params64(net, requires_grad=False)
    return lambda x, t: forward_labels64(cfg, sd, torch.from_numpy(np.ascontiguousarray(x)), torch.tensor([t]), y).numpy()


def F_cfg(net, y, w):
    """The guided velocity of one net: v_u + w (v_c - v_u).  w = 1 / w = 0 evaluate one branch, as the library does."""
    vc, vu = velocity_labels_of(net, y), velocity_labels_of(net, None)

    def F(s, t):
        if w == 1.0:
            return (vc(s[0], t),)
        if w == 0.0:
            return (vu(s[0], t),)
        c, u = vc(s[0], t), vu(s[0], t)
        return (u + w * (c - u),)
    return F


def sample_cfg64(net, x0, y, w, num_steps, solver="euler", step_begin=0, step_end=None):
    return O.integrate64(F_cfg(net, y, w), (x0,), num_steps, solver, step_begin, step_end)[0]


def direct64(sd, x, t, y):
    """The labelled forward of FlexibleUNet(channel_mult=(1,), num_res_blocks=1) written out directly: four ResBlocks
    (encoder, two middle, two decoder) around one skip list, emb = time_embed(..) + E[y] in every time_mlp."""
    x, t = x.to(torch.float64), t.to(torch.float64).reshape(-1).expand(x.shape[0])
    mc = sd["time_embed.0.weight"].shape[1]
    gn = lambda h, n: F.group_norm(h, min(8, h.shape[1]), sd[n + ".weight"], sd[n + ".bias"], eps=1e-5)
    conv = lambda h, n: F.conv2d(h, sd[n + ".weight"], sd[n + ".bias"], padding=sd[n + ".weight"].shape[-1] // 2)
    lin = lambda h, n: F.linear(h, sd[n + ".weight"], sd[n + ".bias"])
    emb = lin(F.silu(lin(U.timestep_embedding64(t, mc), "time_embed.0")), "time_embed.2") + sd[EMB][torch.as_tensor(y).long()]

    def res(h, n):
        a = conv(F.silu(gn(h, n + ".norm1")), n + ".conv1") + lin(F.silu(emb), n + ".time_mlp.1")[:, :, None, None]
        a = conv(F.silu(gn(a, n + ".norm2")), n + ".conv2")
        return a + (conv(h, n + ".skip") if n + ".skip.weight" in sd else h)
    h0 = conv(x, "input_conv")
    h1 = res(h0, "encoder_blocks.0")
    h = res(res(h1, "middle_block1"), "middle_block2")
    h = res(torch.cat([h, h1], 1), "decoder_blocks.0")
    h = res(torch.cat([h, h0], 1), "decoder_blocks.1")
    return conv(F.silu(gn(h, "out_norm")), "out_conv")
