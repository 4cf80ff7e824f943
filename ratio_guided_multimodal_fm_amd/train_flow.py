"""Train a velocity U-Net with conditional flow matching on the HIP backward.

    python -m ratio_guided_multimodal_fm_amd.train_flow --preset svhn --data svhn_train.npy

Mirrors the reference trainers (src/train_flow_svhn.py, src/train_flow_mnist32.py, src/train_flow.py): same
arguments and defaults, Adam, best / every-N checkpoints {'epoch', 'model_state_dict', 'optimizer_state_dict',
'best_loss'} under the reference's names, early stopping.  The data is one tensor [N, C, H, W] in a .npy or .pt
file, already in the reference's value range (no dataset download here).
"""
import argparse
import os

import numpy as np
import torch

from .models import FlowMatchingUNet, FlowMatchingUNetMNIST, FlowMatchingUNetSVHN
from .utils import set_seed
from .utils.flow_utils import CFMSchedule, train_flow_matching_epoch

PRESETS = {
    # preset: (constructor, image shape, checkpoint stem) -- the stems sample_mnist_svhn.py / sample.py load
    'mnist32': (lambda: FlowMatchingUNetMNIST(32), (1, 32, 32), 'flow_mnist32'),
    'svhn': (FlowMatchingUNetSVHN, (3, 32, 32), 'flow_svhn'),
    'unet28': (FlowMatchingUNet, (1, 28, 28), 'flow_unet28'),
}


def parse_args(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    p.add_argument('--preset', choices=sorted(PRESETS), required=True)
    p.add_argument('--data', required=True, help='.npy / .pt tensor [N, C, H, W]')
    p.add_argument('--epochs', type=int, default=50)
    p.add_argument('--batch_size', type=int, default=128)
    p.add_argument('--lr', type=float, default=1e-4)
    p.add_argument('--device', type=str, default='cuda')
    p.add_argument('--save_every', type=int, default=10, help='Save checkpoint every N epochs')
    p.add_argument('--patience', type=int, default=10, help='Early stopping patience')
    p.add_argument('--seed', type=int, default=42)
    p.add_argument('--resume', type=str, default=None, help='checkpoint to resume from')
    p.add_argument('--out_dir', type=str, default='checkpoints')
    return p.parse_args(argv)


def load_data(path, shape):
    data = torch.load(path, map_location='cpu') if path.endswith('.pt') else torch.from_numpy(np.load(path))
    data = torch.as_tensor(data, dtype=torch.float32).contiguous()
    if data.dim() != 4 or tuple(data.shape[1:]) != shape:
        raise ValueError(f"{path}: expected a tensor [N, {shape[0]}, {shape[1]}, {shape[2]}], got {tuple(data.shape)}")
    return data


def batches(data, batch_size, gen):
    """The reference loaders' shuffle=True, drop_last=False epoch order."""
    perm = torch.randperm(data.shape[0], generator=gen)
    for i in range(0, data.shape[0], batch_size):
        yield {'x': data[perm[i:i + batch_size]]}


def checkpoint(epoch, model, optimizer, best_loss):
    return {'epoch': epoch, 'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(),
            'best_loss': best_loss}


def main(argv=None):
    args = parse_args(argv)
    set_seed(args.seed)
    ctor, shape, stem = PRESETS[args.preset]
    device = torch.device(args.device)
    data = load_data(args.data, shape)
    model = ctor().to(device)
    optimizer = torch.optim.Adam(model.parameters(), lr=args.lr)
    schedule = CFMSchedule()
    start_epoch, best_loss = 0, float('inf')
    if args.resume:
        ckpt = torch.load(args.resume, map_location=device)
        if isinstance(ckpt, dict) and 'model_state_dict' in ckpt:
            model.load_state_dict(ckpt['model_state_dict'])
            if 'optimizer_state_dict' in ckpt:
                optimizer.load_state_dict(ckpt['optimizer_state_dict'])
            start_epoch = ckpt.get('epoch', 0)
            best_loss = ckpt.get('best_loss', best_loss)
        else:
            model.load_state_dict(ckpt)
        print(f"Resumed from {args.resume}: epoch {start_epoch}, best_loss={best_loss:.4f}")
    os.makedirs(args.out_dir, exist_ok=True)
    gen = torch.Generator().manual_seed(args.seed)
    patience_counter = 0
    for epoch in range(start_epoch, args.epochs):
        avg_loss = train_flow_matching_epoch(model, batches(data, args.batch_size, gen), optimizer, schedule, device)
        print(f"Epoch {epoch + 1}/{args.epochs} - Loss: {avg_loss:.4f}")
        if avg_loss < best_loss:
            best_loss, patience_counter = avg_loss, 0
            path = os.path.join(args.out_dir, f'{stem}_best.pth')
            torch.save(checkpoint(epoch + 1, model, optimizer, best_loss), path)
            print(f"  -> Saved best model: {path}")
        else:
            patience_counter += 1
        if (epoch + 1) % args.save_every == 0:
            path = os.path.join(args.out_dir, f'{stem}_epoch{epoch + 1}.pth')
            torch.save(checkpoint(epoch + 1, model, optimizer, best_loss), path)
            print(f"  -> Saved checkpoint: {path}")
        if patience_counter >= args.patience:
            print(f"\nEarly stopping after {epoch + 1} epochs")
            break
    print(f"\nTraining complete! Best loss: {best_loss:.4f}")
    return best_loss


if __name__ == '__main__':
    main()
