#!/usr/bin/env python3
"""Training throughput of FlowMatchingModel ("--model original"): one full CFM step (forward, backward, Adam) at
batch 128.

    python tools/bench_train_fmnet.py [--batch 128] [--steps 20] [--warmup 5] [--only hip|miopen]

Times (a) the HIP step (FlowMatchingModel.forward_train + the library's backward, then the repack of the handle the
next step's forward triggers) and (b) the same step on a plain torch.nn.functional fp32 restatement of the net on the
same GPU (MIOpen convs / transposed convs, rocBLAS Linears, PyTorch autograd), in the same process, and prints one
JSON line: samples/s of both and their ratio.  `--only hip` is the form to put behind
`rocprofv3 --kernel-trace --stats --` for the per-kernel table.
"""
import argparse
import json
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

from ratio_guided_multimodal_fm_amd import models as M  # noqa: E402
from ratio_guided_multimodal_fm_amd.utils.flow_utils import CFMSchedule, train_flow_matching_epoch  # noqa: E402


def functional_forward(sd, x, t, T_dim):
    """FlowMatchingModel.forward as torch.nn.functional calls over the module's parameters (MIOpen baseline)."""
    def gn_silu(h, n):
        return F.silu(F.group_norm(h, 8, sd[n + ".weight"], sd[n + ".bias"]))

    h = x
    for i, stride in enumerate((1, 2, 2, 1), 1):
        h = gn_silu(F.conv2d(h, sd[f"encoder.conv{i}.weight"], sd[f"encoder.conv{i}.bias"], stride=stride, padding=1),
                    f"encoder.gn{i}")
    feat = F.linear(h.flatten(1), sd["encoder.fc.weight"], sd["encoder.fc.bias"])
    half = T_dim // 2
    freqs = torch.exp(torch.arange(half, device=x.device) * -(math.log(10000) / (half - 1)))
    args = t[:, None] * freqs[None, :]
    comb = torch.cat([feat, args.sin(), args.cos()], dim=1)
    h = F.linear(comb, sd["decoder.fc1.weight"], sd["decoder.fc1.bias"]).view(-1, 256, 7, 7)
    for i in (1, 2):
        h = gn_silu(F.conv_transpose2d(h, sd[f"decoder.deconv{i}.weight"], sd[f"decoder.deconv{i}.bias"], stride=2,
                                       padding=1), f"decoder.gn{i}")
    h = gn_silu(F.conv2d(h, sd["decoder.conv3.weight"], sd["decoder.conv3.bias"], padding=1), "decoder.gn3")
    return F.conv2d(h, sd["decoder.conv_out.weight"], sd["decoder.conv_out.bias"], padding=1)


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
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["hip", "miopen"], default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    B = args.batch
    data = torch.rand(B, 1, 28, 28, device=dev) * 2 - 1
    res = {"model": "original", "batch": B, "steps": args.steps}
    if args.only != "miopen":
        m = M.FlowMatchingModel().to(dev)
        opt = torch.optim.Adam(m.parameters(), lr=1e-4)
        sched = CFMSchedule()
        ms = time_steps(lambda: train_flow_matching_epoch(m, [{"x": data}], opt, sched, dev), args.steps, args.warmup)
        res.update(hip_ms=round(ms, 3), hip_samples_per_s=round(B / ms * 1e3, 1))
    if args.only != "hip":
        ref = M.FlowMatchingModel().to(dev)
        params = dict(ref.named_parameters())
        opt2 = torch.optim.Adam(ref.parameters(), lr=1e-4)

        def step_ref():
            t = torch.rand(B, device=dev)
            x_t, u = CFMSchedule().add_noise(data, t)
            loss = F.mse_loss(functional_forward(params, x_t, t, ref.time_emb_dim), u)
            opt2.zero_grad()
            loss.backward()
            opt2.step()
            loss.item()
        ms2 = time_steps(step_ref, args.steps, args.warmup)
        res.update(miopen_ms=round(ms2, 3), miopen_samples_per_s=round(B / ms2 * 1e3, 1))
    if "hip_ms" in res and "miopen_ms" in res:
        res["hip_over_miopen"] = round(res["miopen_ms"] / res["hip_ms"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
