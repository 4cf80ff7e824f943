#!/usr/bin/env python3
"""Training throughput of the velocity U-Net: one full CFM step (forward, backward, Adam) at batch 128.

    python tools/bench_train.py [--presets mnist32 svhn] [--batch 128] [--steps 20] [--warmup 5]

For each preset it times (a) the HIP step (FlexibleUNet.forward_train + the library's backward) and (b) the same
step on a plain torch.nn.functional fp32 restatement of the net on the same GPU (MIOpen convs, PyTorch autograd),
both with Dropout(0.1) active, and prints one JSON line per preset: samples/s of both and their ratio, plus the
weight-gradient convs' algorithmic FLOPs per step (2 * Cout * Cin * taps * B * H_out * W_out summed over every conv),
the number a `rocprofv3 --kernel-trace --stats` time of ug_igemm_kernel<2> divides into TFLOP/s (against 157.3
nominal fp32 matrix TFLOP/s).
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.models.unet_flexible import timestep_embedding  # noqa: E402
from ratio_guided_multimodal_fm_amd.utils.flow_utils import CFMSchedule, train_flow_matching_epoch  # noqa: E402

PRESETS = {"mnist32": lambda: M.FlowMatchingUNetMNIST(32), "svhn": M.FlowMatchingUNetSVHN}


def functional_forward(m, sd, x, t, p_drop):
    """FlexibleUNet.forward as torch.nn.functional calls over the module's parameters (MIOpen baseline)."""
    def gn(h, n):
        return F.group_norm(h, min(8, h.shape[1]), sd[n + ".weight"], sd[n + ".bias"])

    def conv(h, n, stride=1):
        w = sd[n + ".weight"]
        return F.conv2d(h, w, sd[n + ".bias"], stride=stride, padding=w.shape[-1] // 2)

    def res(h, n, emb):
        a = conv(F.silu(gn(h, n + ".norm1")), n + ".conv1")
        a = a + F.linear(F.silu(emb), sd[n + ".time_mlp.1.weight"], sd[n + ".time_mlp.1.bias"])[:, :, None, None]
        a = F.dropout(F.silu(gn(a, n + ".norm2")), p_drop, training=True)
        return conv(a, n + ".conv2") + (conv(h, n + ".skip") if n + ".skip.weight" in sd else h)

    emb = timestep_embedding(t, m.model_channels)
    emb = F.linear(F.silu(F.linear(emb, sd["time_embed.0.weight"], sd["time_embed.0.bias"])),
                   sd["time_embed.2.weight"], sd["time_embed.2.bias"])
    h = conv(x, "input_conv")
    hs = [h]
    bi = 0
    last = len(m.channel_mult) - 1
    for level in range(last + 1):
        for _ in range(m.num_res_blocks):
            h = res(h, f"encoder_blocks.{bi}", emb)
            hs.append(h)
            bi += 1
        if level < last:
            h = conv(h, f"downsamplers.{level}.conv", 2)
            hs.append(h)
    h = res(res(h, "middle_block1", emb), "middle_block2", emb)
    bi = ui = 0
    for level in range(last, -1, -1):
        for _ in range(m.num_res_blocks + 1):
            h = res(torch.cat([h, hs.pop()], 1), f"decoder_blocks.{bi}", emb)
            bi += 1
        if level > 0:
            h = conv(F.interpolate(h, scale_factor=2, mode="nearest"), f"upsamplers.{ui}.conv")
            ui += 1
    return conv(F.silu(gn(h, "out_norm")), "out_conv")


def wgrad_flops(m, B):
    """Algorithmic FLOPs of every conv weight gradient of one backward (output raster x Cout x Cin x taps x 2),
    over the net's conv list in the order functional_forward runs it."""
    flops = 0
    S = m.img_size
    mc, last = m.model_channels, len(m.channel_mult) - 1

    def c(cout, cin, taps, So):
        return 2 * B * So * So * cout * cin * taps

    flops += c(mc, m.in_channels, 9, S)
    blocks = m._resblocks()
    bi = 0
    for level in range(last + 1):
        for _ in range(m.num_res_blocks):
            r = blocks[bi]
            flops += c(r.out_channels, r.in_channels, 9, S) + c(r.out_channels, r.out_channels, 9, S)
            flops += c(r.out_channels, r.in_channels, 1, S) if r.in_channels != r.out_channels else 0
            bi += 1
        if level < last:
            ch = blocks[bi - 1].out_channels
            S //= 2
            flops += c(ch, ch, 9, S)
    for _ in range(2):
        r = blocks[bi]
        flops += c(r.out_channels, r.in_channels, 9, S) + c(r.out_channels, r.out_channels, 9, S)
        bi += 1
    for level in range(last, -1, -1):
        for _ in range(m.num_res_blocks + 1):
            r = blocks[bi]
            flops += c(r.out_channels, r.in_channels, 9, S) + c(r.out_channels, r.out_channels, 9, S)
            flops += c(r.out_channels, r.in_channels, 1, S) if r.in_channels != r.out_channels else 0
            bi += 1
        if level > 0:
            S *= 2
            ch = blocks[bi - 1].out_channels
            flops += c(ch, ch, 9, S)
    flops += c(m.in_channels, blocks[-1].out_channels, 9, S)
    return flops


def time_steps(step, steps, warmup):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        step()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--presets", nargs="+", default=["mnist32", "svhn"])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["hip", "miopen"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    for name in args.presets:
        m = PRESETS[name]().to(dev)
        B, S, C = args.batch, m.img_size, m.in_channels
        data = torch.rand(B, C, S, S, device=dev) * 2 - 1
        res = {"preset": name, "batch": B, "steps": args.steps}
        if args.only != "miopen":
            opt = torch.optim.Adam(m.parameters(), lr=1e-4)
            sched = CFMSchedule()
            ms = time_steps(lambda: train_flow_matching_epoch(m, [{"x": data}], opt, sched, dev), args.steps,
                            args.warmup)
            res.update(hip_ms=round(ms, 3), hip_samples_per_s=round(B / ms * 1e3, 1))
        if args.only != "hip":
            ref = PRESETS[name]().to(dev)
            params = dict(ref.named_parameters())
            opt2 = torch.optim.Adam(ref.parameters(), lr=1e-4)

            def step_ref():
                t = torch.rand(B, device=dev)
                x_t, u = CFMSchedule().add_noise(data, t)
                loss = F.mse_loss(functional_forward(ref, params, x_t, t, 0.1), u)
                opt2.zero_grad()
                loss.backward()
                opt2.step()
                loss.item()
            ms2 = time_steps(step_ref, args.steps, args.warmup)
            res.update(miopen_ms=round(ms2, 3), miopen_samples_per_s=round(B / ms2 * 1e3, 1))
        if "hip_ms" in res and "miopen_ms" in res:
            res["hip_over_miopen"] = round(res["miopen_ms"] / res["hip_ms"], 3)
        res["wgrad_gflop_per_step"] = round(wgrad_flops(m, B) / 1e9, 3)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
