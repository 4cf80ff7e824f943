"""Train a density-ratio estimator r(x, y) = q(x, y) / p_ind(x, y) on the HIP backward.

    python -m ratio_guided_multimodal_fm_amd.train_ratio --kind mnist_svhn --data pairs.npz
    python -m ratio_guided_multimodal_fm_amd.train_ratio --kind flexible --x_channels 3 --y_channels 3 --data pairs.npz

Mirrors the reference trainers (src/train_ratio_mnist_svhn.py for --kind mnist_svhn, src/train_ratio.py for --kind
mnist28): same arguments and defaults, Adam, plain state_dict checkpoints under the reference's names (best / every 10
epochs), early stopping with patience 5.  The data is one .npz / .pt with `x` [N, ...], `y` [N, ...] and `label` [N],
already in the reference's value range (no dataset download here): a real pair takes y from an item of the same
label, a fake pair from another label, drawn per item with probability real_fake_ratio.

--kind flexible trains a FlexibleRatioEstimator (the reference has no trainer for it; the mnist28 trainer's epoch is
used): the channel counts come from --x_channels / --y_channels, the (square) image sizes from the data file.  Its
checkpoints, checkpoints/ratio_<loss>_flexible_<tag>.pth, are the dict format load_checkpoint reads --
{'model_state_dict', 'epoch', 'best_loss'} -- with the constructor arguments beside them ('x_channels', 'y_channels',
'feature_dim', 'hidden_dim', 'loss_type'), since unlike the fixed kinds the file name does not determine the module.
"""
import argparse
import os

import numpy as np
import torch
import torch.nn.functional as F

from .models.ratio_estimator import RatioEstimator
from .models.ratio_flexible import FlexibleRatioEstimator, RatioEstimatorMNISTSVHN
from .utils import set_seed
from .utils.losses import get_ratio_loss
from .utils.optim import add_optimizer_args, build_optimizer, check_optimizer_args, ema_path
from .utils.path_utils import get_checkpoint_path
from .utils.trainer import RatioTrainer

KINDS = {
    # kind: (constructor, x shape, y shape)
    'mnist_svhn': (RatioEstimatorMNISTSVHN, (1, 32, 32), (3, 32, 32)),
    'mnist28': (RatioEstimator, (1, 28, 28), (1, 28, 28)),
    'flexible': (FlexibleRatioEstimator, None, None),  # (channels from the arguments, sizes from the data)
}
PATIENCE, SAVE_EVERY = 5, 10


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--kind', choices=sorted(KINDS), required=True)
    p.add_argument('--data', required=True, help=".npz / .pt with 'x' [N,...], 'y' [N,...], 'label' [N]")
    p.add_argument('--loss_type', type=str, default='disc', choices=['disc', 'rulsif'])
    p.add_argument('--transform_type', type=str, default='rotate90', help='names the mnist28 checkpoint')
    p.add_argument('--x_channels', type=int, default=1, help='--kind flexible: channels of x (1..4)')
    p.add_argument('--y_channels', type=int, default=1, help='--kind flexible: channels of y (1..4)')
    p.add_argument('--epochs', type=int, default=30)
    p.add_argument('--batch_size', type=int, default=128)
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--real_fake_ratio', type=float, default=0.5, help='Proportion of real pairs')
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--rulsif_alpha', type=float, default=0.2)
    p.add_argument('--lambda_penalty', type=float, default=0.1)
    p.add_argument('--seed', type=int, default=42)
    add_optimizer_args(p)
    args = p.parse_args(argv)
    check_optimizer_args(p, args)
    return args


def load_pairs(path, shape_x, shape_y):
    """(x, y, label) tensors of the data file.  A shape's size entries may be None (--kind flexible): any square
    image of that many channels."""
    d = torch.load(path, map_location='cpu') if path.endswith('.pt') else np.load(path)
    x = torch.as_tensor(np.asarray(d['x']), dtype=torch.float32).contiguous()
    y = torch.as_tensor(np.asarray(d['y']), dtype=torch.float32).contiguous()
    label = torch.as_tensor(np.asarray(d['label'])).long().reshape(-1)
    def fits(t, shape):
        if shape[1] is None:
            return t.dim() == 4 and t.shape[1] == shape[0] and t.shape[2] == t.shape[3]
        return tuple(t.shape[1:]) == shape
    if not fits(x, shape_x) or not fits(y, shape_y):
        raise ValueError(f"{path}: expected x [N, {shape_x}] and y [N, {shape_y}], got {tuple(x.shape)} and {tuple(y.shape)}")
    if not (x.shape[0] == y.shape[0] == label.shape[0]):
        raise ValueError(f"{path}: x, y and label must have the same length")
    if label.unique().numel() < 2:
        raise ValueError(f"{path}: fake pairs need at least two labels")
    return x, y, label


def make_pairs(label, real_fake_ratio, gen):
    """Per item i: is_real[i] ~ Bernoulli(real_fake_ratio) and the index of its y -- an item of the same label
    (real) or of another label (fake), uniform among those."""
    n = label.shape[0]
    is_real = (torch.rand(n, generator=gen) < real_fake_ratio).long()
    by_label = {int(k): torch.nonzero(label == k).reshape(-1) for k in label.unique()}
    others = {k: torch.nonzero(label != k).reshape(-1) for k in by_label}
    u = torch.rand(n, generator=gen)
    y_idx = torch.empty(n, dtype=torch.long)
    for i in range(n):
        pool = by_label[int(label[i])] if is_real[i] else others[int(label[i])]
        y_idx[i] = pool[min(int(u[i] * pool.numel()), pool.numel() - 1)]
    return is_real, y_idx


def batches(x, y, label, batch_size, real_fake_ratio, gen):
    """One epoch in the reference loaders' shuffle=True, drop_last=False order, pairs redrawn every epoch."""
    is_real, y_idx = make_pairs(label, real_fake_ratio, gen)
    perm = torch.randperm(x.shape[0], generator=gen)
    for i in range(0, x.shape[0], batch_size):
        j = perm[i:i + batch_size]
        yield {'x': x[j], 'y': y[y_idx[j]], 'is_real': is_real[j]}


def train_epoch_mnist_svhn(model, loader, loss_fn, optimizer, device):
    """The MNIST-SVHN trainer's epoch: BCE on the one class present when a batch is all real or all fake, no
    gradient clipping; metrics {'loss', 'accuracy'}."""
    model.train()
    total_loss, correct, total, num_batches = 0.0, 0, 0, 0
    for batch in loader:
        x, y = batch['x'].to(device), batch['y'].to(device)
        is_real = batch['is_real'].to(device).float()
        scores = model.forward_train(x, y)
        scores_real, scores_fake = scores[is_real == 1], scores[is_real == 0]
        if len(scores_real) > 0 and len(scores_fake) > 0:
            loss, _ = loss_fn(scores_real, scores_fake)
        elif len(scores_real) > 0:
            loss = F.binary_cross_entropy_with_logits(scores_real, torch.ones_like(scores_real))
        else:
            loss = F.binary_cross_entropy_with_logits(scores_fake, torch.zeros_like(scores_fake))
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        preds = (scores.detach() > 0).float()
        correct += (preds == is_real).sum().item()
        total += len(is_real)
        total_loss += loss.item()
        num_batches += 1
    return {'loss': total_loss / num_batches, 'accuracy': correct / total}


def checkpoint_path(args, tag):
    if args.kind == 'mnist_svhn':
        os.makedirs('checkpoints', exist_ok=True)
        return f'checkpoints/ratio_{args.loss_type}_mnist_svhn_{tag}.pth'
    if args.kind == 'flexible':
        os.makedirs('checkpoints', exist_ok=True)
        return f'checkpoints/ratio_{args.loss_type}_flexible_{tag}.pth'
    return get_checkpoint_path('ratio', args.loss_type, args.transform_type, tag)


def save_checkpoint(model, args, path, epoch, best_loss, optimizer=None):
    """Plain state_dict for the fixed kinds (as the reference trainers write); the flexible kind adds what rebuilds it.
    With an optimizer that keeps an EMA of the weights, the averaged weights go to the sibling <name>_ema.pth as a
    plain state_dict."""
    if getattr(optimizer, 'ema_decay', None) is not None:
        torch.save(optimizer.ema_state_dict(model), ema_path(path))
    if args.kind != 'flexible':
        torch.save(model.state_dict(), path)
        return
    torch.save({'model_state_dict': model.state_dict(), 'epoch': epoch, 'best_loss': best_loss,
                'x_channels': model.x_channels, 'y_channels': model.y_channels, 'feature_dim': model.feature_dim,
                'hidden_dim': model.hidden_dim, 'loss_type': model.loss_type}, path)


def main(argv=None):
    args = parse_args(argv)
    set_seed(args.seed)
    ctor, shape_x, shape_y = KINDS[args.kind]
    device = torch.device(args.device)
    if args.kind == 'flexible':
        shape_x, shape_y = (args.x_channels, None, None), (args.y_channels, None, None)
    x, y, label = load_pairs(args.data, shape_x, shape_y)
    if args.kind == 'flexible':
        print(f"x: {tuple(x.shape[1:])}, y: {tuple(y.shape[1:])}")
        model = ctor(x_channels=args.x_channels, y_channels=args.y_channels, loss_type=args.loss_type).to(device)
    else:
        model = ctor(loss_type=args.loss_type).to(device)
    print(f"Model parameters: {sum(p.numel() for p in model.parameters()):,}")
    if args.kind == 'mnist_svhn':
        loss_fn = get_ratio_loss(loss_type=args.loss_type)
    else:
        loss_fn = get_ratio_loss(loss_type=args.loss_type, alpha=args.rulsif_alpha, lambda_penalty=args.lambda_penalty)
    # (--optimizer hip clips at the reference's max_norm = 1.0 by default, inside the step; RatioTrainer then skips its own)
    optimizer = build_optimizer(args, model.parameters(), default_max_grad_norm=1.0)
    trainer = RatioTrainer(model, loss_fn, optimizer, device)
    gen = torch.Generator().manual_seed(args.seed)
    best_loss, patience_counter = float('inf'), 0
    for epoch in range(args.epochs):
        loader = batches(x, y, label, args.batch_size, args.real_fake_ratio, gen)
        if args.kind == 'mnist_svhn':
            metrics = train_epoch_mnist_svhn(model, loader, loss_fn, optimizer, device)
        else:
            metrics = trainer.train_epoch(loader)
        print(f"Epoch {epoch + 1}/{args.epochs} - " + ' - '.join(f"{k}: {v:.4f}" for k, v in metrics.items()))
        if metrics['loss'] < best_loss:
            best_loss, patience_counter = metrics['loss'], 0
            path = checkpoint_path(args, 'best')
            save_checkpoint(model, args, path, epoch + 1, best_loss, optimizer)
            print(f"  -> Saved best model: {path}")
        else:
            patience_counter += 1
        if (epoch + 1) % SAVE_EVERY == 0:
            path = checkpoint_path(args, f'epoch{epoch + 1}')
            save_checkpoint(model, args, path, epoch + 1, best_loss, optimizer)
            print(f"  -> Saved checkpoint: {path}")
        if patience_counter >= PATIENCE:
            print(f"\nEarly stopping after {epoch + 1} epochs (patience={PATIENCE})")
            break
    print(f"\nTraining complete! Best loss: {best_loss:.4f}")
    return best_loss


if __name__ == '__main__':
    main()
