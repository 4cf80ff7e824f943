#!/usr/bin/env python3
"""Bits and workspace sizes of everything that reads the U-Net handle's plan (csrc/unet_plan.h), for a same-box A/B of
two trees: one line per case -- name, the byte counts, then SHA-256s.  Only the package's public functions, raw size
queries and the case builders of tests/helpers.py, so the same file runs unchanged in a worktree of an earlier commit:

    python3 tools/unet_bits.py > new.txt
    (cd ../parent && python3 tools/unet_bits.py) > parent.txt
    diff parent.txt new.txt

Run it as one process per environment (default, RGFM_CONV=bx3, RGFM_CONV=f32, RGFM_GN=table, RGFM_FUSE_FIN=0,
RGFM_HX2D=0, RGFM_UP_T2=0, RGFM_WINO=1).

Cases: the three presets, helpers.GENERIC_UNETS and helpers.ARCH_SWEEP at batch 3, a4 and a224 also at batch 1.  Line
"<tag>/B<n>": rgfm_unet_workspace_bytes, rgfm_unet_train_workspace_bytes; the forward output; every forward_trace
activation (their number, then one hash over all of them in order); the conv_routes dict and the P-handover count of
the plain forward; forward_train's v, dx and the parameter-gradient blob (state_dict order) through autograd.
On g16 and a96 once more with dropout 0.1 under a fixed seed ("<tag>/B3/p0.1": v, dx, the blob, then one hash over the
dropout_mask of every block).  On g16 and g24 the likelihood path ("<tag>/B3/logp": linearize().v and .vjp; divergence
with 2 probes -- its workspace bytes, v, div; log_prob at 3 steps, Euler then midpoint -- workspace bytes, logp, z).
"""
import ctypes
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from helpers import ARCH_SWEEP, GENERIC_UNETS, make_generic_unet, make_module, make_sweep_unet  # noqa: E402
from ratio_guided_multimodal_fm_amd import _lib  # noqa: E402

SEED, B = 99, 3
PRESETS = {"unet28": (1, 28), "mnist32": (1, 32), "svhn": (3, 32)}


def sha(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def query(fn, *args):
    nb = ctypes.c_size_t()
    _lib.check(getattr(_lib.lib(), fn)(*args, ctypes.byref(nb)))
    return nb.value


def case(tag, batch, dev):
    """(module on the device, x, t) of a tag at `batch` rows"""
    if tag in PRESETS:
        c, s = PRESETS[tag]
        g = torch.Generator().manual_seed(500 + list(PRESETS).index(tag))
        m, x = make_module(tag, dev), torch.randn(batch, c, s, s, generator=g)
        t = torch.linspace(0.0, 0.99, batch) if batch > 1 else torch.tensor([0.99])
    elif tag in GENERIC_UNETS:
        m, x, t = make_generic_unet(tag, dev)
        x, t = x[:batch], t[:batch]
    else:
        m, x, t = make_sweep_unet(tag, batch, dev)
    return m, x.to(dev), t.to(dev)


def train_pass(m, x, t):
    for p in m.parameters():
        p.grad = None
    xg = x.clone().requires_grad_(True)
    torch.cuda.manual_seed(SEED)
    v = m.forward_train(xg, t)
    g = torch.Generator().manual_seed(SEED)
    (v * torch.randn(v.shape, generator=g).to(v.device)).sum().backward()
    return sha(v), sha(xg.grad), sha(*[p.grad for p in m.parameters()])


def plain(tag, batch, dev):
    m, x, t = case(tag, batch, dev)
    E, h = m._engine, m._engine.handle(dev)
    sizes = query("rgfm_unet_workspace_bytes", h, batch), query("rgfm_unet_train_workspace_bytes", h, batch)
    with torch.no_grad():
        out = sha(m(x, t))
        routes = ",".join(f"{k}={v}" for k, v in E.conv_routes(dev).items())
        n = ctypes.c_int()
        _lib.check(_lib.lib().rgfm_unet_p_handovers(h, ctypes.byref(n)))
        acts = E.forward_trace(x, t)[1]
    print(f"{tag}/B{batch}", *sizes, out, len(acts), sha(*acts), routes, f"p={n.value}", *train_pass(m, x, t), flush=True)


def dropout(tag, dev):
    m, x, t = case(tag, B, dev)
    blocks = m._resblocks()
    for b in blocks:
        b.dropout.p = 0.1
    m.train()
    torch.cuda.manual_seed(SEED)  # the seed forward_train will draw
    seed = int(torch.randint(0, 2 ** 62, (1,), device=dev).item())
    masks = [m._engine.dropout_mask(k, seed, 0.1, B, dev) for k in range(len(blocks))]
    print(f"{tag}/B{B}/p0.1", *train_pass(m, x, t), sha(*masks), flush=True)


def likelihood(tag, dev):
    m, x, t = case(tag, B, dev)
    E, h = m._engine, m._engine.handle(dev)
    g = torch.Generator().manual_seed(SEED + 1)
    eps = torch.randn(2, *x.shape, generator=g).to(dev)
    lin = E.linearize(x, t)
    out = [sha(lin.v), sha(lin.vjp(eps[0]))]
    out += [query("rgfm_unet_divergence_workspace_bytes", h, B), *map(sha, E.divergence(x, t, eps))]
    for sid, solver in enumerate(("euler", "midpoint")):
        out += [query("rgfm_unet_log_prob_workspace_bytes", h, B, sid, 2), *map(sha, E.log_prob(x, eps, 3, solver))]
    print(f"{tag}/B{B}/logp", *out, flush=True)


def main():
    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    _lib.lib()
    for tag in list(PRESETS) + list(GENERIC_UNETS) + list(ARCH_SWEEP):
        plain(tag, B, dev)
    for tag in ("a4", "a224"):
        plain(tag, 1, dev)
    for tag in ("g16", "a96"):
        dropout(tag, dev)
    for tag in ("g16", "g24"):
        likelihood(tag, dev)
    return 0


if __name__ == "__main__":
    sys.exit(main())
