"""float64 torch restatement of the three evaluation classifiers (reference src/models/classifier.py:9-52 and
src/models/svhn_classifier.py:11-116), written from the architecture over the module's own state_dict: the yardstick
of the classifier training tests.

It has a training / eval switch (BatchNorm on batch or running statistics) and takes, each optionally, the max-pools'
CHOICES (window element 0..3, row-major), the ReLU GATES (1 / 0) and the dropout keep MASK of another run, so that a
pool is a gather and a ReLU a multiplication: a near-tie inside a 2x2 window or a pre-activation next to zero flips the
decision between fp32 and float64, which is a discontinuity of the function and not an arithmetic error.  With None it
takes its own float64 decisions (the first maximal window element, value > 0: torch's).

A conv block's gate lives on the block's OUTPUT raster: behind a pool it is the gate of the element taken, so the block
computes gate * y[choice] -- which is max_pool2d(relu(y)) when both decisions are its own."""
import torch
import torch.nn.functional as F

NETS = {
    # kind: (image shape, [(conv, norm or None, pool_after)])
    "mnist28": ((1, 28, 28), [("conv1", None, 1), ("conv2", None, 1)]),
    "mnist32": ((1, 32, 32), [("conv1", None, 1), ("conv2", None, 1), ("conv3", None, 0)]),
    "svhn": ((3, 32, 32), [("conv1", "bn1", 1), ("conv2", "bn2", 1), ("conv3", "bn3", 0), ("conv4", "bn4", 0)]),
}
MOMENTUM, EPS = 0.1, 1e-5


def kind_of(module):
    return {"MNISTClassifier": "mnist28", "MNISTClassifier32": "mnist32", "SVHNClassifier": "svhn"}[type(module).__name__]


def params64(module, requires_grad=True):
    """{name: float64 CPU tensor} of the module's state_dict; floating entries that are parameters become leaves."""
    names = {k for k, _ in module.named_parameters()}
    return {k: v.detach().to("cpu", torch.float64).clone().requires_grad_(requires_grad and k in names)
            for k, v in module.state_dict().items()}


def windows(a):
    """[B, C, Ho, Wo, 4]: the 2x2 windows of a max-pool, row-major inside a window."""
    B, C, H, W = a.shape
    Ho, Wo = H // 2, W // 2
    return a[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)


def first_argmax(w):
    """Index of the first maximal element along the last axis."""
    idx = torch.arange(w.shape[-1]).expand_as(w)
    return torch.where(w == w.max(-1, keepdim=True).values, idx, w.shape[-1]).min(-1).values


def forward64(kind, sd, x, training, choices=None, gates=None, mask=None, p_drop=0.0, out=None):
    """logits [B, 10] in float64.  choices: per conv block an integer tensor [B, C, Ho, Wo] or None (blocks without a
    pool), or None; gates: per conv block, then fc1, a 1 / 0 tensor on the layer's output, or None; mask: the keep mask
    (1 / 0) [B, hidden] of the Dropout layer, or None.  `out` (a dict) receives 'buffers' -- the BatchNorm buffers after
    this call ({name: tensor}; training mode updates them) --, 'pre' -- per layer the pre-activation the decisions were
    taken on: the windows [B, C, Ho, Wo, 4] of y in front of a pool, else y --, and this run's own 'choices' / 'gates'
    in the format of the arguments."""
    h = x.to(torch.float64)
    new_buffers, pre, own_c, own_g = {}, [], [], []
    for i, (conv, norm, pool) in enumerate(NETS[kind][1]):
        y = F.conv2d(h, sd[f"{conv}.weight"], sd[f"{conv}.bias"], padding=1)
        if norm:
            rm, rv = sd[f"{norm}.running_mean"], sd[f"{norm}.running_var"]
            if training:
                mean, var = y.mean((0, 2, 3)), y.var((0, 2, 3), unbiased=False)
                n = y.numel() // y.shape[1]
                new_buffers[f"{norm}.running_mean"] = ((1 - MOMENTUM) * rm + MOMENTUM * mean).detach()
                new_buffers[f"{norm}.running_var"] = ((1 - MOMENTUM) * rv + MOMENTUM * var * n / (n - 1)).detach()
                new_buffers[f"{norm}.num_batches_tracked"] = sd[f"{norm}.num_batches_tracked"] + 1
            else:
                mean, var = rm, rv
            y = (y - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS)
            y = y * sd[f"{norm}.weight"][None, :, None, None] + sd[f"{norm}.bias"][None, :, None, None]
        if pool:
            w = windows(y)
            pre.append(w.detach())
            k0 = first_argmax(F.relu(w.detach()))
            own_c.append(k0)
            k = k0 if choices is None else choices[i].to("cpu", torch.int64)
            y = w.gather(-1, k[..., None])[..., 0]
        else:
            pre.append(y.detach())
            own_c.append(None)
        g0 = (y.detach() > 0).to(torch.float64)
        own_g.append(g0)
        h = y * (g0 if gates is None else gates[i].to("cpu", torch.float64))
    u = F.linear(h.flatten(1), sd["fc1.weight"], sd["fc1.bias"])
    pre.append(u.detach())
    g0 = (u.detach() > 0).to(torch.float64)
    own_g.append(g0)
    h = u * (g0 if gates is None else gates[-1].to("cpu", torch.float64))
    if mask is not None:
        h = h * mask.to("cpu", torch.float64) / (1.0 - p_drop)
    if out is not None:
        out["buffers"], out["pre"], out["choices"], out["gates"] = new_buffers, pre, own_c, own_g
    return F.linear(h, sd["fc2.weight"], sd["fc2.bias"])
