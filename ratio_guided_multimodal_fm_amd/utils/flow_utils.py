"""Samplers of the 28x28 experiments and CFM training (reference ``src/utils/flow_utils.py``).

``CFMSchedule.sample`` (``:69-100``) and ``sample_bimodal_guided``
(``:178-375``) keep the reference signatures and return values; the Euler
loops, the U-Net evaluations, the ratio estimator and the MC guidance all run
inside librgfm_hip.so (one C-ABI call per phase).  ``sample_conditional`` (new: the reference
has no conditional sampler) integrates one net given images of the other modality.  ``CFMSchedule.add_noise``
(``:40-67``) and ``train_flow_matching_epoch`` (``:103-156``) train a
``FlexibleUNet`` through its HIP backward (``FlexibleUNet.forward_train``).
"""
import torch
import torch.nn.functional as F

from .. import _engine
from .._lib import solver_id as _solver_id


def _device(device):
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError(
            f"device '{device}' requested: the MI355X sampler has no CPU path; pass a HIP device "
            "('cuda' / 'cuda:N').")
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


class CFMSchedule:
    """Rectified-flow schedule; only the sampler is on the accelerated path."""

    def __init__(self, sigma=0.0):
        self.sigma = sigma

    def compute_mu_t(self, x_0, x_1, t):
        t = t.view(-1, 1, 1, 1)
        return (1 - t) * x_0 + t * x_1

    def compute_sigma_t(self, t):
        return self.sigma

    def add_noise(self, x_1, t):
        """(x_t, u_t): x_0 ~ N(0, I) like x_1, x_t = (1 - t) x_0 + t x_1, u_t = x_1 - x_0 (reference :40-67)."""
        x_0 = torch.randn_like(x_1)
        t = t.view(x_1.shape[0], *([1] * (x_1.dim() - 1)))
        return (1 - t) * x_0 + t * x_1, x_1 - x_0

    def sample(self, model, num_samples, num_steps=100, device='cuda', solver='euler'):
        """x0 ~ N(0, I) [n,1,28,28]; num_steps explicit Euler steps (reference :69-100), or midpoint steps with
        solver='midpoint' (two network evaluations each, second order; U-Net nets)."""
        _engine._solver(solver, model)
        model.eval()
        dev = _device(device)
        x_t = torch.randn(num_samples, 1, 28, 28, device=dev)
        return _engine.sample_single(model, x_t, num_steps, solver=solver)


def _velocity_train(model, x_t, t):
    """model(x_t, t) with training semantics: FlexibleUNet trains through its HIP backward."""
    fwd = getattr(model, 'forward_train', None)
    if fwd is None:
        raise TypeError(f"{type(model).__name__} has no HIP training path (FlexibleUNet and its presets have one)")
    return fwd(x_t, t)


def train_flow_matching_epoch(model, dataloader, optimizer, schedule, device, modality='x'):
    """One CFM epoch (reference :103-156): per batch t ~ U(0, 1), (x_t, u_t) = schedule.add_noise(x_1, t),
    MSE(model(x_t, t), u_t), backward, optimizer step.  Batches are dicts (``batch[modality]``) as the reference's
    loaders yield, or plain tensors.  Returns the mean batch loss."""
    model.train()
    dev = _device(device)
    total_loss = 0.0
    num_batches = 0
    for batch in dataloader:
        x_1 = (batch[modality] if isinstance(batch, dict) else batch).to(dev)
        t = torch.rand(x_1.shape[0], device=dev)
        x_t, u_t_target = schedule.add_noise(x_1, t)
        v_t = _velocity_train(model, x_t, t)
        loss = F.mse_loss(v_t, u_t_target)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        total_loss += loss.item()
        num_batches += 1
    return total_loss / num_batches


def paired_sampler(fm_x, fm_y, ratio_estimator, guidance_method, guidance_strength, num_samples,
                   num_steps, device, mc_batch_size, shape_x, shape_y, noise=None, verbose=True, solver='euler'):
    """Shared body of both paired samplers.

    `noise` = (x0, y0, mc_x0, mc_y0) overrides the generator draws (parity
    tests upload CPU-generated noise); tensors are copied, never modified.

    `solver` = 'euler' | 'midpoint' integrates EVERY loop of the call (the MC pre-phase and the main loop) with that
    solver, `num_steps` steps each; the noise draws and their order do not depend on it.  'midpoint' needs U-Net nets.
    """
    _engine._solver(solver, fm_x, fm_y)
    fm_x.eval()
    fm_y.eval()
    if ratio_estimator is not None:
        ratio_estimator.eval()
    dev = _device(device)
    guided = guidance_method == 'mc_feng' and ratio_estimator is not None
    grad_guided = guidance_method == 'grad_log_ratio' and ratio_estimator is not None

    if noise is None:
        x_t = torch.randn(num_samples, *shape_x, device=dev)
        y_t = torch.randn(num_samples, *shape_y, device=dev)
    else:
        x_t, y_t = noise[0].to(dev, copy=True).contiguous(), noise[1].to(dev, copy=True).contiguous()

    mc_x1 = mc_y1 = mc_ratios = None
    if guided:
        if verbose:
            print(f"  Generating {mc_batch_size} independent MC samples from flows...")
        # noise in the reference's draw order (x0, y0, mc_x0, mc_y0), then the two independent
        # pre-phase integrations run concurrently on two HIP streams (the N_mc-row launches are too
        # small to fill 256 CUs one net at a time)
        if noise is None:
            mc_x1 = torch.randn(mc_batch_size, *shape_x, device=dev)
            mc_y1 = torch.randn(mc_batch_size, *shape_y, device=dev)
        else:
            mc_x1 = noise[2].to(dev, copy=True).contiguous()
            mc_y1 = noise[3].to(dev, copy=True).contiguous()
        _engine.sample_two_streams(fm_x, mc_x1, fm_y, mc_y1, num_steps, solver=solver)
        if verbose:
            print(f"  Generated MC samples: x shape={mc_x1.shape}, y shape={mc_y1.shape}")
        if ratio_estimator.loss_type not in ("disc", "rulsif"):
            raise ValueError(f"Unknown loss_type: {ratio_estimator.loss_type}")
        mc_ratios = ratio_estimator._engine.eval(mc_x1, mc_y1, "ratio")
        if verbose:
            print(f"  MC ratios: min={mc_ratios.min():.4f}, max={mc_ratios.max():.4f}, "
                  f"mean={mc_ratios.mean():.4f}")

    if grad_guided:
        # "Gradient Log-Ratio" of the reference README (:159-164): v + gamma * grad log r(x_t, y_t) every step.  The
        # reference accepts only 'none' / 'mc_feng' and has no code for this mode; see rgfm_sample_pair_grad.
        if ratio_estimator.loss_type not in ("disc", "rulsif"):
            raise ValueError(f"Unknown loss_type: {ratio_estimator.loss_type}")
        _engine.sample_pair_grad(fm_x, fm_y, ratio_estimator, x_t, y_t, num_steps, guidance_strength, solver=solver)
        return x_t, y_t
    _engine.sample_pair(fm_x, fm_y, x_t, y_t, mc_x1, mc_y1, mc_ratios, num_steps, guidance_strength, solver=solver)
    return x_t, y_t


def sample_conditional(fm_target, ratio_estimator, condition, given='x', num_steps=100, guidance_strength=1.0,
                       mc_batch_size=256, mc_samples=None, device=None, guidance_method='mc_feng', solver='euler'):
    """Partners for `condition` in the other modality: one sample of `fm_target`'s modality per condition image.

    ``given='x'``: `condition` is the estimator's x argument and the target is its y; ``given='y'`` the other way
    round.  Only the target net is integrated.

    ``guidance_method='mc_feng'`` (default): the MC guidance of the paired sampler (reference
    ``src/sample_mnist_svhn.py:124-171``) with one side observed: the MC set is `fm_target`'s own unguided samples,
    sample b weighs MC sample j by r(condition_b, mc_j) times its own Gaussian factor (``rgfm_sample_cond``).
    Draw order (global generator of the device): the MC noise ``[mc_batch_size, C, H, W]`` first, then the start
    noise ``[len(condition), C, H, W]``.  With `mc_samples` (terminal MC samples of an earlier call) no MC noise is
    drawn and no pre-phase runs.

    ``guidance_method='grad_log_ratio'``: the one-sided reading of the paired gradient log-ratio sampler, every step
    ``s += (v(s, t) + guidance_strength * d log r / d s) dt`` (``rgfm_sample_cond_grad``).  Only the start noise
    ``[len(condition), C, H, W]`` is drawn; there is no MC set and no pre-phase (`mc_batch_size` and `mc_samples` are
    ignored).  The condition's encoder and its half of the first score Linear run once, before the loop
    (``rgfm_ratio_cond_prepare``); each step runs the target's encoder alone, forward and reverse.

    ``solver='midpoint'`` integrates every loop of the call (the MC pre-phase too) with the explicit midpoint rule
    (``rgfm_sample_*_ode``); the draws and their order are those of ``'euler'``.

    Returns the samples ``[len(condition), C, H, W]`` on the device.  U-Net targets only; ``--sharded`` launches have
    no conditional form yet.
    """
    from .._lib import RgfmError
    _solver_id(solver)
    if given not in ('x', 'y'):
        raise ValueError(f"given must be 'x' or 'y', got {given!r}")
    if guidance_method not in ('mc_feng', 'grad_log_ratio'):
        raise ValueError(f"guidance_method must be 'mc_feng' or 'grad_log_ratio', got {guidance_method!r}")
    if not isinstance(fm_target._engine, _engine.UNetEngine):
        raise RgfmError(f"sample_conditional needs a U-Net target (FlexibleUNet and its presets); "
                        f"{type(fm_target).__name__} has no conditional sampler")
    fm_target.eval()
    ratio_estimator.eval()
    if ratio_estimator.loss_type not in ("disc", "rulsif"):
        raise ValueError(f"Unknown loss_type: {ratio_estimator.loss_type}")
    dev = _device(condition.device if device is None else device)
    condition = condition.to(dev, torch.float32).contiguous()
    shape = (fm_target.in_channels, fm_target.img_size, fm_target.img_size)
    if guidance_method == 'grad_log_ratio':
        s_t = torch.randn(condition.shape[0], *shape, device=dev)
        ctx = ratio_estimator._engine.cond_prepare(condition, given, shape)
        return _engine.sample_cond_grad(fm_target, ratio_estimator, s_t, ctx, given, num_steps, guidance_strength, solver=solver)
    if mc_samples is None:
        mc = torch.randn(mc_batch_size, *shape, device=dev)
        _engine.sample_single(fm_target, mc, num_steps, solver=solver)
    else:
        mc = mc_samples.to(dev, torch.float32).contiguous()
    s_t = torch.randn(condition.shape[0], *shape, device=dev)
    if given == 'x':
        ratios = ratio_estimator.cross_log_ratio(condition, mc).exp()
    else:
        ratios = ratio_estimator.cross_log_ratio(mc, condition).exp().T.contiguous()
    return _engine.sample_cond(fm_target, s_t, mc, ratios, num_steps, guidance_strength, solver=solver)


def sample_bimodal_guided(fm_x, fm_y, ratio_estimator=None, guidance_method='none',
                          guidance_strength=0.0, num_samples=16, num_steps=100, device='cuda',
                          mc_batch_size=64, solver='euler'):
    """Pairs of 1x28x28 images, optional mc_feng guidance (reference :178-375).

    Returns ``(samples_x [n,1,28,28], samples_y [n,1,28,28])`` on `device`.
    Guidance is silently off when `ratio_estimator` is None, skipped on step 0
    (t > 1e-3 test), and `guidance_strength` is not clamped -- all as in the
    reference.  The reference's one-shot diagnostics print (:349-363) is not
    reproduced.
    """
    return paired_sampler(fm_x, fm_y, ratio_estimator, guidance_method, guidance_strength,
                          num_samples, num_steps, device, mc_batch_size, (1, 28, 28), (1, 28, 28), solver=solver)
