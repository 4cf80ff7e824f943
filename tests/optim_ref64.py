"""Float64 restatement of the optimizer step (ratio_guided_multimodal_fm_amd/utils/optim.py, csrc/optim.hip) in plain
torch: clip_grad_norm_'s coefficient from the global norm of all gradients, coupled (Adam) or decoupled (AdamW) weight
decay, torch.optim.Adam's update with per-tensor step counts, and the weight EMA.  Every tensor is float64 on the CPU.

    ref = RefAdam64([dict(params=[...], lr=1e-3, weight_decay=0.0, decoupled=False)], max_grad_norm=1.0, ema_decay=0.99)
    norm = ref.step([[g0, g1, None, ...]])     # per group, per parameter: a gradient or None (skipped)

ref.params / ref.exp_avg / ref.exp_avg_sq / ref.ema / ref.steps are flat lists over all groups' parameters.
"""
import torch


class RefAdam64:
    def __init__(self, groups, max_grad_norm=None, ema_decay=None):
        self.groups = []
        self.params = []
        for g in groups:
            g = dict(g)
            g.setdefault("lr", 1e-3), g.setdefault("betas", (0.9, 0.999)), g.setdefault("eps", 1e-8)
            g.setdefault("weight_decay", 0.0), g.setdefault("decoupled", False)
            g["params"] = [p.detach().to("cpu", torch.float64).clone() for p in g["params"]]
            g["first"] = len(self.params)
            self.params += g["params"]
            self.groups.append(g)
        self.max_grad_norm, self.ema_decay = max_grad_norm, ema_decay
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.ema = [p.clone() for p in self.params] if ema_decay is not None else None
        self.steps = [0] * len(self.params)
        self.grad_norm = None

    def step(self, grads):
        grads = [[None if g is None else g.detach().to("cpu", torch.float64) for g in gs] for gs in grads]
        coef = 1.0
        if self.max_grad_norm is not None:
            total = sum((g * g).sum() for gs in grads for g in gs if g is not None)
            self.grad_norm = float(torch.as_tensor(total, dtype=torch.float64).sqrt())
            coef = min(1.0, self.max_grad_norm / (self.grad_norm + 1e-6))
        for group, gs in zip(self.groups, grads):
            lr, (b1, b2), eps, wd = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            for k, g in enumerate(gs):
                if g is None:
                    continue
                i = group["first"] + k
                p, m, v = self.params[i], self.exp_avg[i], self.exp_avg_sq[i]
                self.steps[i] += 1
                t = self.steps[i]
                g = coef * g.reshape(p.shape)
                if wd != 0.0:
                    if group["decoupled"]:
                        p.mul_(1.0 - lr * wd)
                    else:
                        g = g + wd * p
                m.mul_(b1).add_(g, alpha=1.0 - b1)
                v.mul_(b2).add_(g * g, alpha=1.0 - b2)
                bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
                p.sub_((lr / bc1) * m / (v.sqrt() / bc2 ** 0.5 + eps))
                if self.ema is not None:
                    self.ema[i].mul_(self.ema_decay).add_(p, alpha=1.0 - self.ema_decay)
        return self.grad_norm
