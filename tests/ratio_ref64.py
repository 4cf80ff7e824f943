"""float64 torch restatement of the two ratio estimators (reference src/models/ratio_flexible.py:185-364 and
src/models/ratio_estimator.py:34-135), written from the architecture over the module's own state_dict: the yardstick
of the ratio training tests.

It has a training / eval switch (BatchNorm on batch or running statistics), takes the dropout keep masks the library
reports, and takes the max-pools' CHOICES (window element 0..3, row-major) so that a pool is a gather, not a max: a
near-tie inside a 2x2 window flips the routing between fp32 and float64, which is a discontinuity of the function and
not an arithmetic error.  With choices=None the pools take the true float64 argmax."""
import torch
import torch.nn.functional as F

ENCODERS = {
    # kind: ((prefix, [(conv, norm, pool_after)]) for x, then for y)
    "mnist_svhn": (("encoder_mnist", [("conv1", "bn1", 1), ("conv2", "bn2", 1), ("conv3", "bn3", 1), ("conv4", "bn4", 0)]),
                   ("encoder_svhn", [("conv1a", "bn1a", 0), ("conv1b", "bn1b", 1), ("conv2a", "bn2a", 0), ("conv2b", "bn2b", 1),
                                     ("conv3a", "bn3a", 0), ("conv3b", "bn3b", 1), ("conv4a", "bn4a", 0), ("conv4b", "bn4b", 1)])),
    "mnist28": (("encoder_x", [("conv1", "gn1", 1), ("conv2", "gn2", 1), ("conv3", "gn3", 1), ("conv4", "gn4", 0)]),
                ("encoder_y", [("conv1", "gn1", 1), ("conv2", "gn2", 1), ("conv3", "gn3", 1), ("conv4", "gn4", 0)])),
}
MOMENTUM, EPS = 0.1, 1e-5


def kind_of(module):
    return "mnist_svhn" if hasattr(module, "encoder_mnist") else "mnist28"


def params64(module, requires_grad=True):
    """{name: float64 CPU tensor} of the module's state_dict; floating entries that are parameters become leaves."""
    names = {k for k, _ in module.named_parameters()}
    return {k: v.detach().to("cpu", torch.float64).clone().requires_grad_(requires_grad and k in names)
            for k, v in module.state_dict().items()}


def windows(a):
    """[B, C, Ho, Wo, 4]: the 2x2 windows of a max-pool (floor division of odd rasters), row-major inside a window."""
    B, C, H, W = a.shape
    Ho, Wo = H // 2, W // 2
    return a[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)


def forward64(kind, sd, x, y, training, choices=None, masks=None, p_drop=0.0, out=None):
    """scores [B] in float64.  choices: per encoder a list of integer tensors [B, C, Ho, Wo], or None; masks: the keep
    masks (1 / 0) of the two Dropout layers, or None.  `out` (a dict) receives 'buffers' -- the BatchNorm buffers after
    this call ({name: tensor}; training mode updates them) -- and 'windows', per encoder the pre-pool windows."""
    imgs = (x.to(torch.float64), y.to(torch.float64))
    feats, new_buffers, wins = [], {}, ([], [])
    for e, (prefix, layers) in enumerate(ENCODERS[kind]):
        h, pool_i = imgs[e], 0
        for conv, norm, pool in layers:
            z = F.conv2d(h, sd[f"{prefix}.{conv}.weight"], sd[f"{prefix}.{conv}.bias"], padding=1)
            g, b = sd[f"{prefix}.{norm}.weight"], sd[f"{prefix}.{norm}.bias"]
            if kind == "mnist28":
                zn = F.group_norm(z, 8, g, b, eps=EPS)
            else:
                rm, rv = sd[f"{prefix}.{norm}.running_mean"], sd[f"{prefix}.{norm}.running_var"]
                if training:
                    mean, var = z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=False)
                    n = z.numel() // z.shape[1]
                    new_buffers[f"{prefix}.{norm}.running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
                    new_buffers[f"{prefix}.{norm}.running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)).detach()
                    new_buffers[f"{prefix}.{norm}.num_batches_tracked"] = sd[f"{prefix}.{norm}.num_batches_tracked"] + 1
                else:
                    mean, var = rm, rv
                zn = (z - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
                zn = zn * g[None, :, None, None] + b[None, :, None, None]
            h = F.silu(zn)
            if pool:
                w = windows(h)
                wins[e].append(w.detach())
                k = w.argmax(-1) if choices is None else choices[e][pool_i].to("cpu", torch.int64)
                h = w.gather(-1, k[..., None])[..., 0]
                pool_i += 1
        feats.append(F.linear(h.mean((2, 3)), sd[f"{prefix}.fc.weight"], sd[f"{prefix}.fc.bias"]))
    h = torch.cat(feats, dim=1)
    linears = sorted(int(k.split(".")[1]) for k, v in sd.items() if k.startswith("score_net.") and k.endswith(".weight") and v.dim() == 2)
    for li, idx in enumerate(linears[:-1]):
        h = F.linear(h, sd[f"score_net.{idx}.weight"], sd[f"score_net.{idx}.bias"])
        h = F.silu(F.layer_norm(h, h.shape[1:], sd[f"score_net.{idx + 1}.weight"], sd[f"score_net.{idx + 1}.bias"], eps=EPS))
        if li < 2 and masks is not None:  # both estimators: Dropout behind the first two hidden layers
            h = h * masks[li].to("cpu", torch.float64) / (1.0 - p_drop)
    if out is not None:
        out["buffers"], out["windows"] = new_buffers, wins
    last = linears[-1]
    return F.linear(h, sd[f"score_net.{last}.weight"], sd[f"score_net.{last}.bias"]).squeeze(-1)
