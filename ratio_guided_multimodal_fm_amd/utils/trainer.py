"""Training loop of a ratio estimator (interface of the reference ``src/utils/trainer.py``).

Batches are dicts ``{'x', 'y', 'is_real'}``.  A model with ``forward_train`` (this package's estimators: HIP forward and
backward) is trained through it; any other module through its ``__call__``.
"""
import numpy as np
import torch


def _mean_metrics(metrics_list):
    return {k: float(np.mean([m[k] for m in metrics_list])) for k in metrics_list[0]}


class RatioTrainer:
    def __init__(self, model, loss_fn, optimizer, device='cuda'):
        self.model = model
        self.loss_fn = loss_fn
        self.optimizer = optimizer
        self.device = device

    def _scores(self, batch):
        x, y = batch['x'].to(self.device), batch['y'].to(self.device)
        is_real = batch['is_real'].to(self.device)
        fwd = getattr(self.model, 'forward_train', None) or self.model
        scores = fwd(x, y)
        return scores[is_real == 1], scores[is_real == 0]

    def train_step(self, batch):
        loss, metrics = self.loss_fn(*self._scores(batch))
        self.optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(self.model.parameters(), max_norm=1.0)
        self.optimizer.step()
        return metrics

    def train_epoch(self, dataloader):
        self.model.train()
        return _mean_metrics([self.train_step(batch) for batch in dataloader])

    def evaluate(self, dataloader):
        self.model.eval()
        with torch.no_grad():
            return _mean_metrics([self.loss_fn(*self._scores(batch))[1] for batch in dataloader])
