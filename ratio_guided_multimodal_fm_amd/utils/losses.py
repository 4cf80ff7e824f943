"""Density-ratio losses on the score vector T(x, y) (interface of the reference ``src/utils/losses.py``).

Each loss maps (scores of real pairs, scores of fake pairs) to ``(loss, metrics)``.  They run in torch on the [B] score
vector that ``forward_train`` returns: B floats, whose gradient enters the HIP backward as ``dscore``.

``cross_entropy`` is the classifiers' loss: the fused softmax cross-entropy kernel (``rgfm_clf_xent``).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F


class DensityRatioLoss(nn.Module):
    def forward(self, scores_real, scores_fake):
        raise NotImplementedError


class DiscriminatorLoss(DensityRatioLoss):
    """Logistic regression of real against fake: -E_q[log sigmoid(T)] - E_p[log(1 - sigmoid(T))].

    At the optimum sigmoid(T) / (1 - sigmoid(T)) = q / p, so log r = logsigmoid(T) - logsigmoid(-T)."""

    def forward(self, scores_real, scores_fake):
        loss = F.softplus(-scores_real).mean() + F.softplus(scores_fake).mean()
        with torch.no_grad():
            metrics = {'loss': loss.item(),
                       'acc_real': (scores_real > 0).float().mean().item(),
                       'acc_fake': (scores_fake < 0).float().mean().item()}
        return loss, metrics


class RuLSIFLoss(DensityRatioLoss):
    """Relative unconstrained least-squares importance fitting with w = softplus(T):
    0.5 E_mix[w^2] - E_q[w] + lambda (E_mix[w] - 1)^2, the mixture being the batch's real and fake pairs together."""

    def __init__(self, alpha=0.2, lambda_penalty=0.1):
        super().__init__()
        self.alpha = alpha
        self.lambda_penalty = lambda_penalty

    def forward(self, scores_real, scores_fake):
        w_real, w_fake = F.softplus(scores_real), F.softplus(scores_fake)
        w_mix = torch.cat([w_real, w_fake])
        constraint = self.lambda_penalty * (w_mix.mean() - 1.0) ** 2
        loss = 0.5 * (w_mix ** 2).mean() - w_real.mean() + constraint
        with torch.no_grad():
            metrics = {'loss': loss.item(), 'mean_w_real': w_real.mean().item(), 'mean_w_fake': w_fake.mean().item(),
                       'constraint_term': constraint.item()}
        return loss, metrics


def cross_entropy(logits, labels):
    """``(loss, pred)``: the mean softmax cross-entropy of logits [B, classes <= 32] against integer labels [B], and
    the predicted classes [B] (argmax, the first index on a tie), from one launch of the fused HIP kernel.  The loss
    is differentiable w.r.t. the logits: the kernel computes (softmax - onehot) / B with it.  HIP tensors only."""
    from .._engine import cross_entropy as fused
    loss, pred, _ = fused(logits, labels)
    return loss, pred


def get_ratio_loss(loss_type='disc', **kwargs):
    if loss_type == 'disc':
        return DiscriminatorLoss()
    if loss_type == 'rulsif':
        return RuLSIFLoss(alpha=kwargs.get('alpha', 0.2), lambda_penalty=kwargs.get('lambda_penalty', 0.1))
    raise ValueError(f"Unknown loss type: {loss_type}")
