"""Train an evaluation classifier (the coherence metric's digit classifiers) on the HIP backward.

    python -m ratio_guided_multimodal_fm_amd.train_classifier --kind mnist28 --data mnist28.npz --test_data mnist28_test.npz
    python -m ratio_guided_multimodal_fm_amd.train_classifier --kind svhn --data svhn.npz

Mirrors the reference trainers (src/train_classifier.py for --kind mnist28, src/train_classifiers_mnist_svhn.py for
--kind mnist32 and --kind svhn): same arguments and defaults (3 epochs for mnist28, 10 for the other two; batch 128,
lr 1e-3, Adam), cross-entropy, plain state_dict checkpoints under the reference's names --
checkpoints/mnist_classifier.pth whenever the test accuracy improves, checkpoints/mnist32_classifier.pth and
checkpoints/svhn_classifier.pth after the last epoch -- which evaluate.py and evaluate_mnist_svhn.py load.  The data is
one .npz / .pt with `x` [N, C, S, S] already in [-1, 1] and `label` [N] (no dataset download here); without
--test_data the last 10 % of the file is held out.
"""
import argparse
import os

import numpy as np
import torch

from .models.classifier import MNISTClassifier
from .models.svhn_classifier import MNISTClassifier32, SVHNClassifier
from .utils import set_seed
from .utils.optim import add_optimizer_args, build_optimizer, check_optimizer_args, ema_path
from .utils.trainer import ClassifierTrainer

KINDS = {
    # kind: (constructor, image shape, default epochs, checkpoint, saved on every improvement of the test accuracy)
    'mnist28': (MNISTClassifier, (1, 28, 28), 3, 'checkpoints/mnist_classifier.pth', True),
    'mnist32': (MNISTClassifier32, (1, 32, 32), 10, 'checkpoints/mnist32_classifier.pth', False),
    'svhn': (SVHNClassifier, (3, 32, 32), 10, 'checkpoints/svhn_classifier.pth', False),
}
HOLD_OUT = 0.1


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--kind', choices=sorted(KINDS), required=True)
    p.add_argument('--data', required=True, help=".npz / .pt with 'x' [N,C,S,S] in [-1, 1] and 'label' [N]")
    p.add_argument('--test_data', default=None, help='same format; default: the last 10 %% of --data is held out')
    p.add_argument('--epochs', type=int, default=None, help='default: 3 (mnist28) or 10 (mnist32, svhn)')
    p.add_argument('--batch_size', type=int, default=128)
    p.add_argument('--lr', type=float, default=1e-3)
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--seed', type=int, default=42)
    add_optimizer_args(p)
    args = p.parse_args(argv)
    check_optimizer_args(p, args)
    if args.epochs is None:
        args.epochs = KINDS[args.kind][2]
    return args


def load_images(path, shape):
    """(x, label) tensors of the data file."""
    d = torch.load(path, map_location='cpu') if path.endswith('.pt') else np.load(path)
    for key in ('x', 'label'):
        if key not in d:
            raise ValueError(f"{path}: no '{key}' entry")
    x = torch.as_tensor(np.asarray(d['x']), dtype=torch.float32).contiguous()
    label = torch.as_tensor(np.asarray(d['label'])).long().reshape(-1)
    if x.dim() != 4 or tuple(x.shape[1:]) != shape:
        raise ValueError(f"{path}: expected x [N, {shape[0]}, {shape[1]}, {shape[2]}], got {tuple(x.shape)}")
    if x.shape[0] != label.shape[0] or x.shape[0] == 0:
        raise ValueError(f"{path}: x and label must have the same, non-zero length")
    if int(label.min()) < 0 or int(label.max()) > 9:
        raise ValueError(f"{path}: labels must be in 0..9")
    return x, label


def split_data(x, label):
    """(train, test): the last 10 % of the file held out (at least one item on either side)."""
    n = x.shape[0]
    k = min(max(1, int(round(n * HOLD_OUT))), n - 1)
    if k < 1:
        raise ValueError("holding out 10 % needs at least two items")
    return (x[:n - k], label[:n - k]), (x[n - k:], label[n - k:])


def batches(x, label, batch_size, gen=None):
    """One pass; gen: shuffled with it (the reference loaders' shuffle=True, drop_last=False order)."""
    n = x.shape[0]
    order = torch.randperm(n, generator=gen) if gen is not None else torch.arange(n)
    for i in range(0, n, batch_size):
        j = order[i:i + batch_size]
        yield x[j], label[j]


def checkpoint_path(kind):
    return KINDS[kind][3]


def save_checkpoint(model, kind, optimizer=None):
    """The plain state_dict; with an optimizer that keeps an EMA of the weights also the sibling <name>_ema.pth."""
    path = checkpoint_path(kind)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    torch.save(model.state_dict(), path)
    if getattr(optimizer, 'ema_decay', None) is not None:
        torch.save(optimizer.ema_state_dict(model), ema_path(path))
    return path


def main(argv=None):
    args = parse_args(argv)
    set_seed(args.seed)
    ctor, shape, _, _, save_best = KINDS[args.kind]
    device = torch.device(args.device)
    x, label = load_images(args.data, shape)
    if args.test_data:
        train, test = (x, label), load_images(args.test_data, shape)
    else:
        train, test = split_data(x, label)
    print(f"train: {train[0].shape[0]} images, test: {test[0].shape[0]} images")
    model = ctor().to(device)
    print(f"Model parameters: {sum(p.numel() for p in model.parameters()):,}")
    optimizer = build_optimizer(args, model.parameters())
    trainer = ClassifierTrainer(model, optimizer, device)
    gen = torch.Generator().manual_seed(args.seed)
    best_acc = 0.0
    for epoch in range(args.epochs):
        train_loss, train_acc = trainer.train_epoch(batches(*train, args.batch_size, gen))
        test_acc = trainer.evaluate(batches(*test, args.batch_size))
        print(f"Epoch {epoch + 1}/{args.epochs} - Train Loss: {train_loss:.4f}, Train Acc: {train_acc:.4f}, "
              f"Test Acc: {test_acc:.4f}")
        if test_acc > best_acc:
            best_acc = test_acc
            if save_best:
                print(f"  -> Saved best model: {save_checkpoint(model, args.kind, optimizer)} (test_acc={test_acc:.4f})")
    if not save_best:
        print(f"Saved classifier: {save_checkpoint(model, args.kind, optimizer)} (best acc: {best_acc:.4f})")
    print(f"\nTraining complete! Best test accuracy: {best_acc:.4f}")
    return best_acc


if __name__ == '__main__':
    main()
