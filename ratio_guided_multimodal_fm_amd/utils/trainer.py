"""Training loop of a ratio estimator (interface of the reference ``src/utils/trainer.py``).

Batches are dicts ``{'x', 'y', 'is_real'}``.  A model with ``forward_train`` (this package's estimators: HIP forward and
backward) is trained through it; any other module through its ``__call__``.

``ClassifierTrainer`` is the loop of the reference's classifier trainers (``src/train_classifier.py:22-68``,
``src/train_classifiers_mnist_svhn.py:63-113``) on ``forward_train`` and the fused cross-entropy kernel; its batches
are ``(images, labels)`` pairs.
"""
import numpy as np
import torch

from .losses import cross_entropy


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
        if getattr(self.optimizer, 'max_grad_norm', None) is None:  # (utils.optim.Adam clips inside its step)
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


class ClassifierTrainer:
    def __init__(self, model, optimizer, device='cuda'):
        self.model = model
        self.optimizer = optimizer
        self.device = device

    def train_step(self, x, labels):
        """One optimizer step in the module's current mode; returns (loss, number of correct predictions) as device
        scalars: the step reads nothing back itself (forward_train's draw of the dropout seed does, once)."""
        x, labels = x.to(self.device), labels.to(self.device)
        loss, pred = cross_entropy(self.model.forward_train(x), labels)
        self.optimizer.zero_grad()
        loss.backward()
        self.optimizer.step()
        return loss.detach(), (pred == labels).sum()

    def train_epoch(self, dataloader):
        """(mean loss over the batches, accuracy over the items), as the reference's train_epoch."""
        self.model.train()
        losses, correct, total = [], [], 0
        for x, labels in dataloader:
            loss, ok = self.train_step(x, labels)
            losses.append(loss), correct.append(ok)
            total += labels.shape[0]
        return float(torch.stack(losses).mean().item()), int(torch.stack(correct).sum().item()) / total

    def evaluate(self, dataloader):
        """Accuracy in eval mode, the predictions taken from the cross-entropy kernel."""
        self.model.eval()
        correct, total = [], 0
        with torch.no_grad():
            for x, labels in dataloader:
                x, labels = x.to(self.device), labels.to(self.device)
                _, pred = cross_entropy(self.model.forward_train(x), labels)
                correct.append((pred == labels).sum())
                total += labels.shape[0]
        return int(torch.stack(correct).sum().item()) / total
