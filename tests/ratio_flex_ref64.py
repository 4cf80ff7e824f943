"""float64 torch.nn.functional restatement of FlexibleRatioEstimator (reference src/models/ratio_flexible.py:13-154),
written from the architecture over the module's own state_dict: the yardstick of the flexible-estimator tests.

Any channel counts and any image sizes (the two sizes independent): two encoders of four 3x3 convs (32, 64, 128, 128
channels), each followed by GroupNorm(8) and SiLU, a floor 2x2 max-pool behind the first three, a global average pool
and a Linear; then the score MLP (Linear, LayerNorm, SiLU, Dropout, twice; Linear to one score).

As tests/ratio_ref64.py does for the fixed kinds, the training forward takes the dropout keep masks the library reports
and the max-pools' CHOICES (window element 0..3, row-major), so that a pool is a gather and not a max: a near-tie in a
2x2 window flips the routing between fp32 and float64, which is a discontinuity of the function, not an arithmetic
error.  With choices=None the pools take the true float64 argmax."""
import torch
import torch.nn.functional as F

EPS = 1e-5
ENCODERS = ("encoder_x", "encoder_y")


def params64(module_or_sd, requires_grad=True):
    """{name: float64 CPU tensor}; every entry is a parameter of this architecture and becomes a leaf."""
    sd = module_or_sd.state_dict() if hasattr(module_or_sd, "state_dict") else module_or_sd
    return {k: torch.as_tensor(v).detach().to("cpu", torch.float64).clone().requires_grad_(requires_grad)
            for k, v in sd.items()}


def windows(a):
    """[B, C, Ho, Wo, 4]: the 2x2 windows of a floor max-pool, row-major inside a window; the last row / column of an
    odd raster is in no window."""
    B, C, H, W = a.shape
    Ho, Wo = H // 2, W // 2
    return a[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)


def forward64(sd, x, y, choices=None, masks=None, p_drop=0.0, out=None):
    """scores [B] in float64.  choices: per encoder a list of three integer tensors [B, C, Ho, Wo], or None; masks: the
    keep masks (1 / 0) of the two Dropout layers, or None (eval mode).  `out` (a dict) receives 'windows', per encoder
    the pre-pool windows, and 'pooled_in', per encoder the activated maps in front of the pools (leaves of nothing:
    retain_grad() is called on them so that a test can read the gradient of a dropped row / column)."""
    imgs = (x.to(torch.float64), y.to(torch.float64))
    feats, wins, pre = [], ([], []), ([], [])
    for e, prefix in enumerate(ENCODERS):
        h = imgs[e]
        for i in range(1, 5):
            z = F.conv2d(h, sd[f"{prefix}.conv{i}.weight"], sd[f"{prefix}.conv{i}.bias"], padding=1)
            h = F.silu(F.group_norm(z, 8, sd[f"{prefix}.gn{i}.weight"], sd[f"{prefix}.gn{i}.bias"], eps=EPS))
            if i < 4:
                if h.requires_grad:
                    h.retain_grad()
                pre[e].append(h)
                w = windows(h)
                wins[e].append(w.detach())
                k = w.argmax(-1) if choices is None else choices[e][i - 1].to("cpu", torch.int64)
                h = w.gather(-1, k[..., None])[..., 0]
        feats.append(F.linear(h.mean((2, 3)), sd[f"{prefix}.fc.weight"], sd[f"{prefix}.fc.bias"]))
    h = torch.cat(feats, dim=1)
    for li, idx in enumerate((0, 4)):
        h = F.linear(h, sd[f"score_net.{idx}.weight"], sd[f"score_net.{idx}.bias"])
        h = F.silu(F.layer_norm(h, h.shape[1:], sd[f"score_net.{idx + 1}.weight"], sd[f"score_net.{idx + 1}.bias"], eps=EPS))
        if masks is not None:
            h = h * masks[li].to("cpu", torch.float64) / (1.0 - p_drop)
    if out is not None:
        out["windows"], out["pooled_in"] = wins, pre
    return F.linear(h, sd["score_net.8.weight"], sd["score_net.8.bias"]).squeeze(-1)


def log_ratio64(sd, x, y, loss_type, **kw):
    """log r(x, y) (reference :135-154)."""
    s = forward64(sd, x, y, **kw)
    if loss_type == "disc":
        return F.logsigmoid(s) - F.logsigmoid(-s)
    if loss_type == "rulsif":
        return torch.log(F.softplus(s) + 1e-8)
    raise ValueError(f"Unknown loss_type: {loss_type}")
