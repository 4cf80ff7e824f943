"""Density-ratio estimators of the reference's ``src/models/ratio_flexible.py``, host side.

API mirrors of ``FlexibleRatioEstimator`` with its presets (reference ``:69-182``; GroupNorm ``ImageEncoder``
``:13-66``) and of ``RatioEstimatorMNISTSVHN`` (``:305-385``; BatchNorm encoders ``:185-302``): parameter
containers with the reference's ``state_dict`` keys; ``forward`` / ``log_ratio`` run in the HIP library
(eval-mode semantics: BatchNorm uses running statistics, Dropout is the identity).
"""
import torch.nn as nn

from .._engine import FlexibleRatioEngine, RatioEngine, engine_property
from .ratio_estimator import ImageEncoder, RatioEstimator


class FlexibleRatioEstimator(nn.Module):
    """Ratio estimator for any pair of square images: x [B, x_channels, Sx, Sx], y [B, y_channels, Sy, Sy] with 1..4
    channels and sizes 8..64 (reference ``:69-154``).  The parameters do not depend on the image sizes (the encoders
    end in a global average pool); the sizes are read from the inputs of each call and the engine keeps one device
    handle per (Sx, Sy) pair seen.  ``forward`` / ``forward_train`` / ``log_ratio`` / ``grad_log_ratio`` /
    ``grad_log_ratio_given`` / ``forward_cross`` / ``cross_log_ratio`` / ``dropout_p`` as for ``RatioEstimator``, whose architecture at 1x28x28 + 1x28x28 this is."""
    _engine = engine_property(lambda m: FlexibleRatioEngine(m))

    def __init__(self, x_channels=1, y_channels=1, feature_dim=256, hidden_dim=512, loss_type='disc'):
        super().__init__()
        self.x_channels = x_channels
        self.y_channels = y_channels
        self.feature_dim = feature_dim
        self.hidden_dim = hidden_dim
        self.loss_type = loss_type
        self.encoder_x = ImageEncoder(in_channels=x_channels, feature_dim=feature_dim)
        self.encoder_y = ImageEncoder(in_channels=y_channels, feature_dim=feature_dim)
        h = hidden_dim
        self.score_net = nn.Sequential(
            nn.Linear(feature_dim * 2, h), nn.LayerNorm(h), nn.SiLU(), nn.Dropout(0.1),
            nn.Linear(h, h // 2), nn.LayerNorm(h // 2), nn.SiLU(), nn.Dropout(0.1),
            nn.Linear(h // 2, 1))

    # the same surface as RatioEstimator (the engine is what differs)
    forward = RatioEstimator.forward
    forward_train = RatioEstimator.forward_train
    dropout_p = RatioEstimator.dropout_p
    log_ratio = RatioEstimator.log_ratio
    grad_log_ratio = RatioEstimator.grad_log_ratio
    grad_log_ratio_given = RatioEstimator.grad_log_ratio_given
    forward_cross = RatioEstimator.forward_cross
    cross_log_ratio = RatioEstimator.cross_log_ratio


class RatioEstimatorMNIST(FlexibleRatioEstimator):
    """Ratio estimator for MNIST transforms (both x and y are 1x28x28; reference ``:159-169``)."""

    def __init__(self, loss_type='disc'):
        super().__init__(x_channels=1, y_channels=1, feature_dim=256, hidden_dim=512, loss_type=loss_type)


class RatioEstimatorMNISTSVHN_old(FlexibleRatioEstimator):
    """Ratio estimator for MNIST-SVHN (x 1x32x32, y 3x32x32), the reference's old ~944K-parameter version
    (``:172-182``)."""

    def __init__(self, loss_type='disc'):
        super().__init__(x_channels=1, y_channels=3, feature_dim=256, hidden_dim=512, loss_type=loss_type)


class _BNEncoderParams(nn.Module):
    def __init__(self, plan, feature_dim):
        super().__init__()
        for name, cin, cout in plan:
            setattr(self, "conv" + name, nn.Conv2d(cin, cout, 3, padding=1))
            setattr(self, "bn" + name, nn.BatchNorm2d(cout))
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.fc = nn.Linear(plan[-1][2], feature_dim)


class MNISTEncoder(_BNEncoderParams):
    """1x32x32 -> feature_dim (reference :185-232)."""

    def __init__(self, feature_dim=256):
        super().__init__([("1", 1, 32), ("2", 32, 64), ("3", 64, 128), ("4", 128, 128)], feature_dim)


class SVHNEncoder(_BNEncoderParams):
    """3x32x32 -> feature_dim (reference :235-302)."""

    def __init__(self, feature_dim=256):
        super().__init__([("1a", 3, 64), ("1b", 64, 64), ("2a", 64, 128), ("2b", 128, 128),
                          ("3a", 128, 256), ("3b", 256, 256), ("4a", 256, 256), ("4b", 256, 256)],
                         feature_dim)


class RatioEstimatorMNISTSVHN(nn.Module):
    _engine = engine_property(lambda m: RatioEngine(m, kind="mnist_svhn"))

    def __init__(self, feature_dim=256, hidden_dim=512, loss_type='disc'):
        super().__init__()
        self.feature_dim = feature_dim
        self.hidden_dim = hidden_dim
        self.loss_type = loss_type
        self.encoder_mnist = MNISTEncoder(feature_dim)
        self.encoder_svhn = SVHNEncoder(feature_dim)
        h = hidden_dim
        self.score_net = nn.Sequential(
            nn.Linear(feature_dim * 2, h), nn.LayerNorm(h), nn.SiLU(), nn.Dropout(0.1),
            nn.Linear(h, h), nn.LayerNorm(h), nn.SiLU(), nn.Dropout(0.1),
            nn.Linear(h, h // 2), nn.LayerNorm(h // 2), nn.SiLU(),
            nn.Linear(h // 2, 1))

    def forward(self, x, y):
        """Scores T(x, y): x [B,1,32,32], y [B,3,32,32] -> [B]."""
        return self._engine.eval(x, y, "score")

    def forward_train(self, x, y):
        """Scores [B] in the module's current mode with autograd through the HIP backward: ``loss.backward()`` fills
        ``p.grad`` of every parameter (and ``x.grad`` / ``y.grad`` if requested).  While ``self.training``: batch
        statistics (BatchNorm buffers updated with momentum 0.1), dropout seeded from the CUDA generator."""
        return self._engine.forward_train(x, y)

    def dropout_p(self):
        """The one dropout probability of the score MLP (the device pass takes one p)."""
        ps = {l.p for l in self.score_net if isinstance(l, nn.Dropout)}
        if len(ps) != 1:
            raise ValueError(f"the Dropout layers of score_net must share one p, got {sorted(ps)}")
        return ps.pop()

    def log_ratio(self, x, y):
        """log r(x, y); raises ValueError for an unknown loss_type (reference :384-385)."""
        if self.loss_type not in ("disc", "rulsif"):
            raise ValueError(f"Unknown loss_type: {self.loss_type}")
        return self._engine.eval(x, y, "log_ratio")

    def forward_cross(self, x, y):
        """Scores of every pair: x [nx,1,32,32], y [ny,3,32,32] -> [nx, ny] with entry (i, j) = forward(x_i, y_j).
        Each encoder runs once per image, not once per pair (``rgfm_ratio_eval_cross``); eval mode only."""
        return self._engine.eval_cross(x, y, "score")

    def cross_log_ratio(self, x, y):
        """log r(x_i, y_j) of every pair -> [nx, ny]: the matrix conditional sampling weighs its MC set with."""
        if self.loss_type not in ("disc", "rulsif"):
            raise ValueError(f"Unknown loss_type: {self.loss_type}")
        return self._engine.eval_cross(x, y, "log_ratio")

    def grad_log_ratio(self, x, y):
        """(d log_ratio/dx, d log_ratio/dy): what ``torch.autograd.grad(self.log_ratio(x, y).sum(), (x, y))``
        returns for the reference module in eval mode -- the quantity of the reference README's "Gradient
        Log-Ratio" guidance (``README.md:159-164``), which the reference itself never computes.  Hand-written
        reverse pass on the device (``csrc/ratio_grad.hip``); the parameters themselves get no gradient."""
        if self.loss_type not in ("disc", "rulsif"):
            raise ValueError(f"Unknown loss_type: {self.loss_type}")
        gx, gy, _ = self._engine.grad_log_ratio(x, y)
        return gx, gy

    # (one side observed: the same surface as RatioEstimator)
    grad_log_ratio_given = RatioEstimator.grad_log_ratio_given
