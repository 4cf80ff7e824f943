"""``MNISTClassifier`` of the 28x28 evaluation harness (reference ``src/models/classifier.py:9-52``).

Runs once on the final samples, so ``forward`` is an ordinary PyTorch module executed by PyTorch-ROCm (same
policy as ``svhn_classifier.py``); ``state_dict`` keys/shapes match the reference's checkpoint
``checkpoints/mnist_classifier.pth``.  ``forward_train`` is the differentiable forward that trains it: exact fp32 on
the matrix cores with a hand-written HIP backward (``rgfm_clf_forward_train`` / ``rgfm_clf_backward``).
"""
import torch.nn as nn
import torch.nn.functional as F

from .._engine import ClassifierEngine, engine_property


class MNISTClassifier(nn.Module):
    """1x28x28 -> 10 logits: conv-ReLU-pool, conv-ReLU-pool, Linear(3136,128)-ReLU-Dropout-Linear(128,10)."""

    _engine = engine_property(lambda m: ClassifierEngine(m, kind="mnist28"))

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(1, 32, 3, padding=1)
        self.conv2 = nn.Conv2d(32, 64, 3, padding=1)
        self.fc1 = nn.Linear(64 * 7 * 7, 128)
        self.fc2 = nn.Linear(128, 10)
        self.dropout = nn.Dropout(0.25)

    def forward(self, x):
        x = F.max_pool2d(F.relu(self.conv1(x)), 2)
        x = F.max_pool2d(F.relu(self.conv2(x)), 2)
        x = F.relu(self.fc1(x.flatten(1)))
        return self.fc2(self.dropout(x))

    def forward_train(self, x):
        """Logits [B, 10] in the module's current mode with autograd through the HIP backward: ``loss.backward()``
        fills ``p.grad`` of every parameter (and ``x.grad`` if requested).  While ``self.training``: dropout seeded
        from the CUDA generator (and, in the BatchNorm net, batch statistics with the buffers updated)."""
        return self._engine.forward_train(x)

    def dropout_p(self):
        """The dropout probability behind fc1."""
        return float(self.dropout.p)
