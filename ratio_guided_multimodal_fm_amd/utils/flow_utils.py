"""Samplers of the 28x28 experiments and CFM training (reference ``src/utils/flow_utils.py``).

``CFMSchedule.sample`` (``:69-100``) and ``sample_bimodal_guided``
(``:178-375``) keep the reference signatures and return values; the Euler
loops, the U-Net evaluations, the ratio estimator and the MC guidance all run
inside librgfm_hip.so (one C-ABI call per phase).  ``sample_conditional`` (new: the reference
has no conditional sampler) integrates one net given images of the other modality.  ``CFMSchedule.add_noise``
(``:40-67``) and ``train_flow_matching_epoch`` (``:103-156``) train a
``FlexibleUNet`` through its HIP backward (``FlexibleUNet.forward_train``).  ``CFMSchedule.log_prob`` / ``encode``,
``bits_per_dim`` and ``joint_log_prob`` (new: the reference has no likelihood) integrate the flow backwards with the
divergence of v accumulated along the path (``rgfm_unet_log_prob``).
"""
import math

import torch
import torch.nn.functional as F

from .. import _engine
from .._lib import solver_id as _solver_id
from .diagnostics import check as _check_diagnostics
from .guidance_schedule import resolve as _resolve_strength


def _sde_kwargs(eta, sde_seed):
    """Keywords of the main loop's _engine call for a stochastic sampler: `eta` is what _engine.check_sde returned at the
    head of the call; 0: {} -- the call goes out as it always did.  Called AFTER every other draw of the call: a seed
    that is None is drawn here (one 62-bit integer from torch's CPU default generator), so the start noise and the MC
    set are those of the sde_eta = 0 call and torch.manual_seed fixes the whole call."""
    if eta == 0.0:
        return {}
    return {'sde_eta': eta, 'sde_seed': _engine.draw_sde_seed() if sde_seed is None else int(sde_seed)}


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

    def sample(self, model, num_samples, num_steps=100, device='cuda', solver='euler', sde_eta=0.0, sde_seed=None,
               labels=None, cfg_scale=1.0):
        """x0 ~ N(0, I) [n,1,28,28]; num_steps explicit Euler steps (reference :69-100), or midpoint steps with
        solver='midpoint' (two network evaluations each, second order; U-Net nets).  `sde_eta` > 0: Euler-Maruyama
        steps of the SDE with the same marginals (``paired_sampler``; U-Net nets, solver='euler'), the noise seeded by
        `sde_seed` (None: drawn from torch's CPU generator after the start noise).
        `labels` (an integer tensor [num_samples], values 0..K of a net built with ``num_classes=K``; K is the null
        label) and `cfg_scale` = w: classifier-free guidance, every stage advances by ``v_u + w (v_c - v_u)``
        (``rgfm_sample_single_cfg``; w = 1: the conditional net alone, one evaluation per stage; w = 0: the
        unconditional branch, the bits of the call without labels).  The start noise then has the net's own image shape;
        the draws are those of the call without labels.  Neither (default): the call is what it was."""
        _engine._solver(solver, model)
        eta = _engine.check_sde(sde_eta, solver, (model,))
        cfg = _engine.check_cfg(labels, cfg_scale, num_samples, model)
        model.eval()
        dev = _device(device)
        if cfg is None:
            x_t = torch.randn(num_samples, 1, 28, 28, device=dev)
            return _engine.sample_single(model, x_t, num_steps, solver=solver, **_sde_kwargs(eta, sde_seed))
        x_t = torch.randn(num_samples, model.in_channels, model.img_size, model.img_size, device=dev)
        return _engine.sample_single(model, x_t, num_steps, solver=solver, labels=labels, cfg_scale=cfg[1],
                                     **_sde_kwargs(eta, sde_seed))


    def log_prob(self, model, x, num_steps=100, solver='midpoint', n_probes=1, generator=None, batch_size=128, labels=None):
        """``(logp [B], z [B, C, H, W])``: the log-density of the images `x` under the flow of `model`, and their
        latents.  `x` (data, t = 1) is integrated backwards to ``z = x(0)`` in `num_steps` steps of `solver` while the
        divergence of v is accumulated: ``logp = log N(z; 0, I) - int_0^1 div v dt`` (``rgfm_unet_log_prob``; exact
        fp32 arithmetic, no dropout whatever the module's mode).  The divergence is Hutchinson's estimate over
        `n_probes` Rademacher probes per image, drawn ONCE for the whole of `x` from `generator` (default: the
        device's torch generator) and fixed along the path; the images are then processed in chunks of `batch_size`,
        so the result does not depend on `batch_size`.  U-Net nets only.  There is no labelled likelihood: `labels`
        other than None raises ``RgfmError``; a class-conditional net is scored as its unconditional branch."""
        _check_likelihood_args(model, x, num_steps, solver, batch_size)
        model._engine.no_labels(labels, "log_prob")
        if not isinstance(n_probes, int) or n_probes < 1:
            raise ValueError(f"n_probes must be an integer >= 1, got {n_probes!r} (encode() integrates without probes)")
        dev = _device(x.device)
        x = x.to(dev, torch.float32).contiguous()
        gdev = dev if generator is None else generator.device
        eps = torch.randint(0, 2, (n_probes, *x.shape), generator=generator, device=gdev).to(dev, torch.float32) * 2 - 1
        logp, z = torch.empty(x.shape[0], device=dev), torch.empty_like(x)
        for b in range(0, x.shape[0], batch_size):
            e = min(b + batch_size, x.shape[0])
            logp[b:e], z[b:e] = model._engine.log_prob(x[b:e], eps[:, b:e].contiguous(), num_steps, solver)
        return logp, z

    def encode(self, model, x, num_steps=100, solver='midpoint', batch_size=128):
        """The latents ``z = x(0)`` of the images `x`: the backward integration of ``log_prob`` without probes (the
        same bits as its `z`)."""
        _check_likelihood_args(model, x, num_steps, solver, batch_size)
        dev = _device(x.device)
        x = x.to(dev, torch.float32).contiguous()
        z = torch.empty_like(x)
        for b in range(0, x.shape[0], batch_size):
            e = min(b + batch_size, x.shape[0])
            z[b:e] = model._engine.log_prob(x[b:e], None, num_steps, solver)[1]
        return z


def _check_likelihood_args(model, x, num_steps, solver, batch_size):
    """Argument checks of log_prob / encode; all of them run before any device call."""
    from .._lib import RgfmError
    sid = _solver_id(solver)
    cap = 2048 if sid else 4096
    if not isinstance(num_steps, int) or not 1 <= num_steps <= cap:
        raise ValueError(f"num_steps must be an integer in [1, {cap}] for solver={solver!r}, got {num_steps!r}")
    if not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"batch_size must be an integer >= 1, got {batch_size!r}")
    if not isinstance(model._engine, _engine.UNetEngine):
        raise RgfmError(f"the likelihood needs a U-Net velocity net (FlexibleUNet and its presets); "
                        f"{type(model).__name__} has no HIP reverse walk to x alone")
    shape = (model.in_channels, model.img_size, model.img_size)
    if x.dim() != 4 or tuple(x.shape[1:]) != shape:
        raise ValueError(f"x of shape [B,{','.join(map(str, shape))}] expected, got {tuple(x.shape)}")


def bits_per_dim(logp, dims, data_range=2.0, levels=256):
    """Bits per dimension of log-densities `logp` (nats, of data scaled to an interval of length `data_range` and
    quantised to `levels` levels): ``-logp / (dims ln 2) + log2(levels / data_range)`` -- the change of variables back
    to the integer grid; +7 bits for 8-bit images scaled to [-1, 1].  `logp`: tensor or number."""
    if dims < 1 or data_range <= 0 or levels < 1:
        raise ValueError(f"dims >= 1, data_range > 0 and levels >= 1 expected, got {dims!r}, {data_range!r}, {levels!r}")
    return -logp / (dims * math.log(2.0)) + math.log2(levels / data_range)


def joint_log_prob(fm_x, fm_y, ratio_estimator, x, y, num_steps=100, solver='midpoint', n_probes=1, generator=None,
                   batch_size=128):
    """``(joint, logp_x, logp_y, log_r)``, each ``[B]``: the log-density of the pairs ``(x_b, y_b)`` under the
    ratio-corrected joint model ``p(x) p(y) r(x, y)``, ``joint = logp_x + logp_y + log_r`` with the marginal terms from
    ``CFMSchedule.log_prob`` (x first, then y, both drawing from `generator`) and
    ``log_r = ratio_estimator.log_ratio(x, y)``.  The ratio estimator is not normalised, so neither is the joint."""
    if x.shape[0] != y.shape[0]:
        raise ValueError(f"x and y must pair up: {x.shape[0]} and {y.shape[0]} images")
    sched = CFMSchedule()
    logp_x = sched.log_prob(fm_x, x, num_steps, solver, n_probes, generator, batch_size)[0]
    logp_y = sched.log_prob(fm_y, y, num_steps, solver, n_probes, generator, batch_size)[0]
    ratio_estimator.eval()
    log_r = ratio_estimator.log_ratio(x.to(logp_x.device, torch.float32).contiguous(),
                                      y.to(logp_x.device, torch.float32).contiguous()).reshape(-1)
    return logp_x + logp_y + log_r, logp_x, logp_y, log_r


def _velocity_train(model, x_t, t):
    """model(x_t, t) with training semantics: FlexibleUNet trains through its HIP backward."""
    fwd = getattr(model, 'forward_train', None)
    if fwd is None:
        raise TypeError(f"{type(model).__name__} has no HIP training path (FlexibleUNet and its presets have one)")
    return fwd(x_t, t)


def drop_labels(labels, num_classes, p_uncond, generator=None):
    """Label dropout of classifier-free training: each label becomes the null label `num_classes` with probability
    `p_uncond`, the decisions drawn as ``torch.rand(len(labels))`` on the labels' device (`generator`: default that
    device's).  ``p_uncond=0`` draws all the same, so the stream of random numbers does not depend on the value."""
    if not 0.0 <= float(p_uncond) <= 1.0:
        raise ValueError(f"p_uncond must be a probability, got {p_uncond!r}")
    u = torch.rand(labels.shape[0], device=labels.device, generator=generator)
    return torch.where(u < float(p_uncond), torch.full_like(labels, int(num_classes)), labels)


def train_flow_matching_epoch(model, dataloader, optimizer, schedule, device, modality='x', p_uncond=0.1):
    """One CFM epoch (reference :103-156): per batch t ~ U(0, 1), (x_t, u_t) = schedule.add_noise(x_1, t),
    MSE(model(x_t, t), u_t), backward, optimizer step.  Batches are dicts (``batch[modality]``) as the reference's
    loaders yield, or plain tensors.  Returns the mean batch loss.
    Labelled batches -- ``(x, label)`` tuples / lists, or (for a net with classes) dicts with a ``'label'`` entry --
    train a net built with ``num_classes=K`` class-conditionally: each label is replaced by the null label K with probability `p_uncond`
    (``drop_labels``, drawn from the device's generator AFTER the batch's t and noise draws).  Without labels nothing
    is drawn for them: the epoch's draws are what they were."""
    model.train()
    dev = _device(device)
    total_loss = 0.0
    num_batches = 0
    for batch in dataloader:
        labels = None
        if isinstance(batch, (tuple, list)):
            batch, labels = batch
        elif isinstance(batch, dict) and getattr(model, 'num_classes', None):
            labels = batch.get('label')
        x_1 = (batch[modality] if isinstance(batch, dict) else batch).to(dev)
        t = torch.rand(x_1.shape[0], device=dev)
        x_t, u_t_target = schedule.add_noise(x_1, t)
        if labels is not None:
            K = getattr(model, 'num_classes', None)
            if not K:
                raise TypeError(f"labelled batches need a net built with num_classes; {type(model).__name__} has none")
            labels = drop_labels(torch.as_tensor(labels).to(dev).reshape(-1).long(), K, p_uncond)
            v_t = model.forward_train(x_t, t, labels)
        else:
            v_t = _velocity_train(model, x_t, t)
        loss = F.mse_loss(v_t, u_t_target)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        total_loss += loss.item()
        num_batches += 1
    return total_loss / num_batches


PAIRINGS = ('paired', 'cross')


def check_pairing(mc_pairing, guidance_method='mc_feng'):
    """'paired' | 'cross' (anything else: ValueError); 'cross' is a pairing of the MC guidance and goes with
    guidance_method='mc_feng' only.  Raised before any device work."""
    if not isinstance(mc_pairing, str) or mc_pairing not in PAIRINGS:
        raise ValueError(f"mc_pairing must be 'paired' or 'cross', got {mc_pairing!r}")
    if mc_pairing == 'cross' and guidance_method != 'mc_feng':
        raise ValueError(f"mc_pairing='cross' pairs up the MC set of guidance_method='mc_feng'; got guidance_method={guidance_method!r}")
    return mc_pairing


def add_pairing_arg(p):
    """--mc_pairing of the command-line tools."""
    p.add_argument('--mc_pairing', type=str, default='paired', choices=list(PAIRINGS),
                   help="MC guidance (mc_feng): 'paired' uses the mc_batch_size pairs (x1_i, y1_i) of the MC set; 'cross' "
                        "all mc_batch_size^2 pairs (x1_i, y1_j) of the same set (U-Net nets, mc_batch_size <= 1024; not "
                        "with --sharded)")


def add_sde_args(p):
    """--sde_eta / --sde_seed of the command-line tools."""
    p.add_argument('--sde_eta', type=float, default=0.0,
                   help="stochastic sampler: Euler-Maruyama steps of the SDE with the ODE's marginals in the main loop, "
                        "noise strength eta (0 = the ODE; U-Net nets, --solver euler; not with --sharded)")
    p.add_argument('--sde_seed', type=int, default=None,
                   help='seed of the per-step noise of --sde_eta (default: drawn from the generator that --seed seeds)')


def sde_from_cli(args, sharded=False):
    """Sampler keywords of --sde_eta / --sde_seed: {} without them, so that the call goes out as it always did."""
    from .._lib import RgfmError
    if not args.sde_eta:
        return {}
    if sharded:
        raise RgfmError("--sde_eta has no --sharded form: run the stochastic sampler on one device")
    return {'sde_eta': args.sde_eta, 'sde_seed': args.sde_seed}


def add_label_args(p):
    """--num_classes / --labels / --cfg_scale of the command-line tools (class-conditional nets)."""
    p.add_argument('--num_classes', type=int, default=None,
                   help='the flow checkpoints are class-conditional nets with this many classes (train_flow --num_classes); '
                        'without --labels they run as their unconditional branch')
    p.add_argument('--labels', type=str, default=None, metavar='{c,random,cycle}',
                   help="labels of the samples (needs --num_classes, --guidance_method none, U-Net nets; not with --sharded): "
                        "an integer c for every sample, 'random' (uniform over the classes, from the generator that --seed "
                        "seeds) or 'cycle' (0, 1, ..., K-1, 0, ...); both nets of a pair take the same labels")
    p.add_argument('--cfg_scale', type=float, default=1.0,
                   help='classifier-free guidance scale w of --labels: v_u + w (v_c - v_u); 1 = the conditional net alone')


def labels_from_cli(args, num_samples, sharded=False, guided=False, unet=True):
    """Sampler keywords of --labels / --cfg_scale: {} without --labels, so that the call goes out as it always did."""
    from .._lib import RgfmError
    spec = getattr(args, 'labels', None)
    if spec is None:
        if getattr(args, 'cfg_scale', 1.0) != 1.0:
            raise RgfmError("--cfg_scale needs --labels")
        return {}
    K = getattr(args, 'num_classes', None)
    if not K:
        raise RgfmError("--labels needs --num_classes (the checkpoints must be class-conditional nets)")
    if sharded:
        raise RgfmError("--labels has no --sharded form: run the labelled sampler on one device")
    if guided:
        raise RgfmError("--labels goes with --guidance_method none: a label-conditioned guided loop is not defined here")
    if not unet:
        raise RgfmError("--labels needs U-Net velocity nets (not --model original)")
    if spec == 'random':
        labels = torch.randint(0, K, (num_samples,))
    elif spec == 'cycle':
        labels = torch.arange(num_samples) % K
    else:
        try:
            c = int(spec)
        except ValueError:
            raise RgfmError(f"--labels: an integer, 'random' or 'cycle' expected, got {spec!r}") from None
        if not 0 <= c <= K:
            raise RgfmError(f"--labels {c}: labels lie in 0..{K} ({K} is the null label)")
        labels = torch.full((num_samples,), c, dtype=torch.long)
    return {'labels': labels, 'cfg_scale': float(args.cfg_scale)}


def add_ess_arg(p):
    """--ess_floor of the command-line tools."""
    p.add_argument('--ess_floor', type=float, default=None,
                   help="MC guidance (mc_feng): hold every row's importance weights to this effective sample size by "
                        "tempering them with an exponent tau <= 1 of the row's own (1 <= ess_floor <= mc_batch_size; "
                        "U-Net nets, --mc_pairing paired; not with --sharded).  Default: the plain weights")


def ess_from_cli(args, sharded=False):
    """Sampler keywords of --ess_floor: {} without it, so that the call goes out as it always did."""
    from .._lib import RgfmError
    if getattr(args, 'ess_floor', None) is None:
        return {}
    if sharded:
        raise RgfmError("--ess_floor has no --sharded form: run the tempered sampler on one device")
    return {'ess_floor': args.ess_floor}


def _ess_kwargs(ess_floor, guidance_method, guided, n_mc, models, cross, diagnostics, diag):
    """Keywords of the MC loop's _engine call for an effective-sample-size floor; every check runs here or in
    _engine.check_ess, before any device work.  None gives {}: the call goes out as it always did.  With records
    (`diag`, what diagnostics._begin returned) the object's `tau` [n_stages, B] is allocated and handed to the loop."""
    from .._lib import RgfmError
    if ess_floor is None:
        return {}
    if guidance_method != 'mc_feng':
        raise RgfmError(f"ess_floor holds the importance weights of guidance_method='mc_feng' to a floor; "
                        f"{guidance_method!r} has no weights to temper")
    floor = _engine.check_ess(ess_floor, n_mc, models, cross)
    if not guided:  # (mc_feng without a ratio estimator runs unguided, as in the reference: nothing to temper)
        return {}
    kw = {'ess_floor': floor}
    if diag is not None:
        kw['tau'] = diagnostics._begin_tau()
    return kw


def _strength_kwargs(guidance_strength, guidance_schedule, rows, num_steps, solver, dev_of, models, what='num_samples'):
    """(gamma, keywords) of the main loop's _engine call for a strength that may be a vector and a schedule that may be
    given: all checks run here, before any device work.  A scalar strength without a schedule gives (the strength as
    passed, {}): the call goes out as it always did.  `dev_of()`: the device, asked for only when a vector goes there."""
    from .._lib import RgfmError
    gamma, vec, scale = _resolve_strength(guidance_strength, guidance_schedule, rows, num_steps, solver, what)
    if vec is None and scale is None:
        return gamma, {}
    for m in models:
        if not isinstance(m._engine, _engine.UNetEngine):
            raise RgfmError("a guidance strength per sample and a guidance_schedule need U-Net velocity nets (FlexibleUNet "
                            f"and its presets); {type(m).__name__} takes a scalar strength only")
    kw = {}
    if vec is not None:
        kw['gamma_rows'] = vec.to(dev_of()).contiguous()
    if scale is not None:
        kw['stage_scale'] = scale
    return gamma, kw


def _pair_cfg(labels, cfg_scale, num_samples, fm_x, fm_y, guidance_method, diagnostics, eta):
    """The labels and scales of a paired call, checked before any draw and any device work: None without them (the call
    is then today's), else ((labels_x, w_x), (labels_y, w_y))."""
    from .._lib import RgfmError
    lx, ly = labels if isinstance(labels, (tuple, list)) else (labels, labels)
    wx, wy = cfg_scale if isinstance(cfg_scale, (tuple, list)) else (cfg_scale, cfg_scale)
    cx = _engine.check_cfg(lx, wx, num_samples, fm_x)
    cy = _engine.check_cfg(ly, wy, num_samples, fm_y)
    if cx is None and cy is None:
        return None
    if guidance_method != 'none':
        raise RgfmError(f"labels go with guidance_method='none' (the supervised pair), got {guidance_method!r}: a "
                        "label-conditioned guided loop is not defined here; without labels the nets run unconditionally")
    if diagnostics is not None or eta != 0.0:
        raise RgfmError("the labelled pair takes no diagnostics and no sde_eta (CFMSchedule.sample has the stochastic "
                        "labelled loop for one net)")
    return cx or (None, 1.0), cy or (None, 1.0)


def _stats(name, t):
    return f"{name}: min={t.min():.4f}, max={t.max():.4f}, mean={t.mean():.4f}"


def paired_sampler(fm_x, fm_y, ratio_estimator, guidance_method, guidance_strength, num_samples,
                   num_steps, device, mc_batch_size, shape_x, shape_y, noise=None, verbose=True, solver='euler',
                   diagnostics=None, mc_pairing='paired', guidance_schedule=None, sde_eta=0.0, sde_seed=None,
                   ess_floor=None, labels=None, cfg_scale=1.0):
    """Shared body of both paired samplers.

    `labels` (``guidance_method='none'``, nets built with ``num_classes``): one integer tensor [num_samples] used for
    BOTH nets -- the supervised coherent pair, the baseline ratio guidance is measured against -- or a pair
    ``(labels_x, labels_y)``, either of which may be None.  `cfg_scale`: a float, or a pair ``(w_x, w_y)``; each net's
    stages advance by ``v_u + w (v_c - v_u)`` (``rgfm_sample_two_cfg``; ``CFMSchedule.sample``).  The noise draws are
    those of the call without labels.  Labels together with a guided method, `diagnostics`, `sde_eta` or sharded
    launches raise ``RgfmError``: what the MC set of a label-conditioned guided loop should be is a research question,
    not plumbing.  In those calls a class-conditional net runs without labels, as its unconditional branch.

    `ess_floor` (None, or a float with 1 <= ess_floor <= mc_batch_size): adaptive tempering of the MC importance
    weights (``guidance_method='mc_feng'``, ``rgfm_sample_pair_ess``).  At every guided stage a
    row whose effective sample size is below the floor has its weights flattened by an exponent tau <= 1 of its own,
    found by bisection so that the effective sample size reaches the floor; rows at or above it keep their bits.  With
    `diagnostics` the object gains ``tau`` [n_stages, B] (1: untouched, 0: the stage ran unguided) and its ess / w_max /
    w_min are those of the tempered weights.  Tempering biases the estimator toward the flatter posterior mean.  Both
    solvers, strength rows and schedules, `sde_eta`; not with ``mc_pairing='cross'``, the gradient method,
    ``FlowMatchingModel`` nets or sharded launches (``RgfmError``).  None (default): the call is what it was.

    `sde_eta` > 0: the main loop takes Euler-Maruyama steps of ``dx = [F + eta (t F - x)] dt + sqrt(2 eta (1 - t)) dW``,
    the SDE that shares the marginals of the ODE ``dx = F dt`` on the path ``x_t = (1 - t) x_0 + t x_1`` (F: the loop's
    whole guided velocity; ``rgfm_sample_*_sde``, DESIGN.md "Stochastic sampling").  The per-step noise is generated on
    the device from `sde_seed` (counter-based: a function of seed, modality, step and element).  ``sde_seed=None``
    draws the seed from torch's CPU default generator after every other draw of the call, so the start noise and the
    MC set are those of the ``sde_eta=0`` call and ``torch.manual_seed`` fixes the whole call.  The MC pre-phase stays
    deterministic.  Both guidance methods, both pairings, with `diagnostics`, strength rows and schedules; U-Net nets
    and ``solver='euler'`` only (``RgfmError`` otherwise).  ``sde_eta=0`` (default): the call is what it was.

    `guidance_strength`: a float, or a 1-D tensor / sequence of `num_samples` strengths (one per pair).
    `guidance_schedule` = None | ``utils.guidance_schedule.GuidanceSchedule`` | callable s(t) | sequence of per-stage
    values: scales the strength per stage of the main loop; a stage whose scale is 0 runs unguided and skips the
    guidance work (``GuidanceSchedule.window``).  Row b, stage k: ``float64(strength_b) * s_k``.  Both guidance
    methods, both solvers, both pairings, with and without `diagnostics`; U-Net nets.  With a float strength and no
    schedule the call is what it was.

    `noise` = (x0, y0, mc_x0, mc_y0) overrides the generator draws (parity
    tests upload CPU-generated noise); tensors are copied, never modified.

    `solver` = 'euler' | 'midpoint' integrates EVERY loop of the call (the MC pre-phase and the main loop) with that
    solver, `num_steps` steps each; the noise draws and their order do not depend on it.  'midpoint' needs U-Net nets.

    `diagnostics` = a ``utils.diagnostics.GuidanceDiagnostics``: the main loop fills it with per-stage, per-sample
    records (effective sample size, weight range, Z_bar, velocity and guidance norms), written on the device with no
    host synchronisation.  The returned samples keep their bits.  Sharded launches (``distributed.py``) take none.

    `mc_pairing` = 'paired' (default) guides with the `mc_batch_size` pairs ``(mc_x1[i], mc_y1[i])``.  'cross'
    (``guidance_method='mc_feng'``, U-Net nets, ``mc_batch_size <= 1024``) guides with all ``mc_batch_size ** 2`` pairs
    ``(mc_x1[i], mc_y1[j])``: every one of them is a draw from the product of the marginals, so the same pre-phase
    yields that many importance pairs.  The noise draws and the pre-phase are unchanged; the ratios are the matrix
    ``ratio_estimator._engine.eval_cross(mc_x1, mc_y1, "ratio")`` and the loop is ``rgfm_sample_pair_cross``.  With
    `diagnostics` the effective sample size is the joint one (1 .. mc_batch_size ** 2; utils/diagnostics.py).
    """
    _check_diagnostics(diagnostics)
    check_pairing(mc_pairing, guidance_method)
    if mc_pairing == 'cross' and ratio_estimator is not None:
        _engine._check_cross((mc_batch_size, mc_batch_size), mc_batch_size, mc_batch_size, fm_x, fm_y)
    _engine._solver(solver, fm_x, fm_y)
    eta = _engine.check_sde(sde_eta, solver, (fm_x, fm_y))
    cfg = _pair_cfg(labels, cfg_scale, num_samples, fm_x, fm_y, guidance_method, diagnostics, eta)
    guidance_strength, gs_kw = _strength_kwargs(guidance_strength, guidance_schedule, num_samples, num_steps, solver,
                                                lambda: _device(device), (fm_x, fm_y))
    _ess_kwargs(ess_floor, guidance_method, False, mc_batch_size, (fm_x, fm_y), mc_pairing == 'cross', None, None)
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
        if mc_pairing == 'cross':
            mc_ratios = ratio_estimator._engine.eval_cross(mc_x1, mc_y1, "ratio")
            if verbose:
                print("  " + _stats(f"MC ratio matrix [{mc_batch_size} x {mc_batch_size}]", mc_ratios))
                print("  " + _stats("  its diagonal (the paired ratios)", mc_ratios.diagonal()))
        else:
            mc_ratios = ratio_estimator._engine.eval(mc_x1, mc_y1, "ratio")
            if verbose:
                print(f"  MC ratios: min={mc_ratios.min():.4f}, max={mc_ratios.max():.4f}, "
                      f"mean={mc_ratios.mean():.4f}")

    if cfg is not None:
        (lx, wx), (ly, wy) = cfg
        _engine.sample_two_cfg(fm_x, x_t, fm_y, y_t, num_steps, solver=solver, labels_x=lx, labels_y=ly, cfg_scale_x=wx,
                               cfg_scale_y=wy)
        return x_t, y_t
    if grad_guided:
        # "Gradient Log-Ratio" of the reference README (:159-164): v + gamma * grad log r(x_t, y_t) every step.  The
        # reference accepts only 'none' / 'mc_feng' and has no code for this mode; see rgfm_sample_pair_grad.
        if ratio_estimator.loss_type not in ("disc", "rulsif"):
            raise ValueError(f"Unknown loss_type: {ratio_estimator.loss_type}")
        diag = None
        if diagnostics is not None and num_samples:
            diag = diagnostics._begin('grad_log_ratio', solver, num_steps, num_samples, dev, stage_scale=gs_kw.get('stage_scale'))
        _engine.sample_pair_grad(fm_x, fm_y, ratio_estimator, x_t, y_t, num_steps, guidance_strength, solver=solver, diag=diag,
                                 **gs_kw, **_sde_kwargs(eta, sde_seed))
        return x_t, y_t
    diag = None
    if diagnostics is not None and num_samples:
        diag = diagnostics._begin('mc_feng' if guided else 'none', solver, num_steps, num_samples, dev, stage_scale=gs_kw.get('stage_scale'))
    ess_kw = _ess_kwargs(ess_floor, guidance_method, guided and num_samples > 0, mc_batch_size, (fm_x, fm_y), False,
                         diagnostics, diag)
    _engine.sample_pair(fm_x, fm_y, x_t, y_t, mc_x1, mc_y1, mc_ratios, num_steps, guidance_strength, solver=solver, diag=diag,
                        **gs_kw, **_sde_kwargs(eta, sde_seed), **ess_kw)
    return x_t, y_t


def shared_mc_sweep(fm_x, fm_y, ratio_estimator, guidance_method, strengths, num_samples, num_steps, device,
                    mc_batch_size, shape_x, shape_y, solver='euler', diagnostics=None, mc_pairing='paired',
                    guidance_schedule=None, sde_eta=0.0, sde_seed=None, ess_floor=None):
    """All `strengths` of one guided method as ONE ``paired_sampler`` call of ``len(strengths) * num_samples`` rows: row
    block j carries ``strengths[j]`` (a strength per row), over one MC set, one pre-phase and one start-noise set
    ``[num_samples]`` repeated per block (common random numbers: the blocks differ by the strength alone).  The noise is
    drawn once, in the order of one ordinary call (x0, y0, then mc_x0, mc_y0 for 'mc_feng').  Rows do not depend on the
    batch they run in, so block j has the bits of a call with that strength on the same noise and MC set.
    Returns ``[(samples_x, samples_y), ...]``, one pair ``[num_samples, ...]`` per strength; `diagnostics` (optional)
    holds the records of all rows, block after block.
    `sde_eta` > 0 (``paired_sampler``): one noise seed for the whole call (`sde_seed`; None: drawn after the noise above).
    The per-step noise is a function of the element's place in the batch, so the blocks then share the start noise and
    the MC set but not the path noise.  `ess_floor`: ``paired_sampler``'s, for every block."""
    if guidance_method not in ('mc_feng', 'grad_log_ratio') or ratio_estimator is None:
        raise ValueError(f"a shared-MC sweep runs a guided method with its ratio estimator, got {guidance_method!r}")
    strengths = [float(g) for g in strengths]
    if not strengths:
        return []
    eta = _engine.check_sde(sde_eta, solver, (fm_x, fm_y))
    _ess_kwargs(ess_floor, guidance_method, False, mc_batch_size, (fm_x, fm_y), mc_pairing == 'cross', None, None)
    dev = _device(device)
    x0 = torch.randn(num_samples, *shape_x, device=dev)
    y0 = torch.randn(num_samples, *shape_y, device=dev)
    mc_x0 = mc_y0 = None
    if guidance_method == 'mc_feng':
        mc_x0 = torch.randn(mc_batch_size, *shape_x, device=dev)
        mc_y0 = torch.randn(mc_batch_size, *shape_y, device=dev)
    k = len(strengths)
    rows = torch.tensor(strengths, dtype=torch.float32).repeat_interleave(num_samples)
    noise = (x0.repeat(k, 1, 1, 1), y0.repeat(k, 1, 1, 1), mc_x0, mc_y0)
    xs, ys = paired_sampler(fm_x, fm_y, ratio_estimator, guidance_method, rows, k * num_samples, num_steps, dev,
                            mc_batch_size, shape_x, shape_y, noise=noise, verbose=False, solver=solver,
                            diagnostics=diagnostics, mc_pairing=mc_pairing, guidance_schedule=guidance_schedule,
                            ess_floor=ess_floor, **_sde_kwargs(eta, sde_seed))
    return [(xs[j * num_samples:(j + 1) * num_samples], ys[j * num_samples:(j + 1) * num_samples]) for j in range(k)]


def sample_conditional(fm_target, ratio_estimator, condition, given='x', num_steps=100, guidance_strength=1.0,
                       mc_batch_size=256, mc_samples=None, device=None, guidance_method='mc_feng', solver='euler',
                       diagnostics=None, guidance_schedule=None, sde_eta=0.0, sde_seed=None, ess_floor=None, labels=None):
    """Partners for `condition` in the other modality: one sample of `fm_target`'s modality per condition image.
    (`labels` other than None raises ``RgfmError``: conditional sampling has no labelled form; a class-conditional
    target runs as its unconditional branch.)

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

    `diagnostics` = a ``utils.diagnostics.GuidanceDiagnostics``: filled by the guided loop (the target's fields in the
    ``_x`` entries, the ``_y`` entries 0); the samples keep their bits.

    `guidance_strength` may be a 1-D tensor / sequence of ``len(condition)`` strengths and `guidance_schedule` scales
    it per stage, as in ``paired_sampler``.

    `sde_eta` > 0: Euler-Maruyama steps in the guided loop, as in ``paired_sampler`` (``rgfm_sample_cond_sde`` /
    ``rgfm_sample_cond_grad_sde``; ``solver='euler'``).  The MC pre-phase stays deterministic; ``sde_seed=None`` is
    drawn from torch's CPU generator after the draws above.

    `ess_floor`: the effective-sample-size floor of ``paired_sampler`` on each row's one-sided weights
    (``guidance_method='mc_feng'``, ``rgfm_sample_cond_ess``; ``1 <= ess_floor <=`` the size of the MC set).

    Returns the samples ``[len(condition), C, H, W]`` on the device.  U-Net targets only; ``--sharded`` launches have
    no conditional form yet.
    """
    from .._lib import RgfmError
    _check_diagnostics(diagnostics)
    _solver_id(solver)
    if given not in ('x', 'y'):
        raise ValueError(f"given must be 'x' or 'y', got {given!r}")
    if guidance_method not in ('mc_feng', 'grad_log_ratio'):
        raise ValueError(f"guidance_method must be 'mc_feng' or 'grad_log_ratio', got {guidance_method!r}")
    if labels is not None:
        raise RgfmError("sample_conditional has no labelled form; without labels a class-conditional target runs as its "
                        "unconditional branch")
    if not isinstance(fm_target._engine, _engine.UNetEngine):
        raise RgfmError(f"sample_conditional needs a U-Net target (FlexibleUNet and its presets); "
                        f"{type(fm_target).__name__} has no conditional sampler")
    fm_target.eval()
    ratio_estimator.eval()
    if ratio_estimator.loss_type not in ("disc", "rulsif"):
        raise ValueError(f"Unknown loss_type: {ratio_estimator.loss_type}")
    eta = _engine.check_sde(sde_eta, solver, (fm_target,))
    n_mc = mc_batch_size if mc_samples is None else len(mc_samples)
    _ess_kwargs(ess_floor, guidance_method, False, n_mc, (fm_target,), False, None, None)
    guidance_strength, gs_kw = _strength_kwargs(guidance_strength, guidance_schedule, len(condition), num_steps, solver,
                                                lambda: _device(condition.device if device is None else device),
                                                (fm_target,), what='len(condition)')
    dev = _device(condition.device if device is None else device)
    condition = condition.to(dev, torch.float32).contiguous()
    shape = (fm_target.in_channels, fm_target.img_size, fm_target.img_size)
    if guidance_method == 'grad_log_ratio':
        s_t = torch.randn(condition.shape[0], *shape, device=dev)
        ctx = ratio_estimator._engine.cond_prepare(condition, given, shape)
        diag = None
        if diagnostics is not None and s_t.shape[0]:
            diag = diagnostics._begin('grad_log_ratio', solver, num_steps, s_t.shape[0], dev, stage_scale=gs_kw.get('stage_scale'))
        return _engine.sample_cond_grad(fm_target, ratio_estimator, s_t, ctx, given, num_steps, guidance_strength, solver=solver,
                                        diag=diag, **gs_kw, **_sde_kwargs(eta, sde_seed))
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
    diag = None
    if diagnostics is not None and s_t.shape[0]:
        diag = diagnostics._begin('mc_feng', solver, num_steps, s_t.shape[0], dev, stage_scale=gs_kw.get('stage_scale'))
    ess_kw = _ess_kwargs(ess_floor, guidance_method, s_t.shape[0] > 0, n_mc, (fm_target,), False, diagnostics, diag)
    return _engine.sample_cond(fm_target, s_t, mc, ratios, num_steps, guidance_strength, solver=solver, diag=diag, **gs_kw,
                               **_sde_kwargs(eta, sde_seed), **ess_kw)


def sample_bimodal_guided(fm_x, fm_y, ratio_estimator=None, guidance_method='none',
                          guidance_strength=0.0, num_samples=16, num_steps=100, device='cuda',
                          mc_batch_size=64, solver='euler', diagnostics=None, mc_pairing='paired', guidance_schedule=None,
                          sde_eta=0.0, sde_seed=None, ess_floor=None, labels=None, cfg_scale=1.0):
    """Pairs of 1x28x28 images, optional mc_feng guidance (reference :178-375).
    `labels`, `cfg_scale` (``guidance_method='none'``): the class-conditional pair (``paired_sampler``).

    Returns ``(samples_x [n,1,28,28], samples_y [n,1,28,28])`` on `device`.
    Guidance is silently off when `ratio_estimator` is None, skipped on step 0
    (t > 1e-3 test), and `guidance_strength` is not clamped -- all as in the
    reference.  The reference's one-shot diagnostics print (:349-363) is
    available through `diagnostics`: pass a ``utils.diagnostics.GuidanceDiagnostics`` and read its
    ``reference_block(int(0.3 * num_steps))`` (the same text) or its per-sample, per-stage records.
    ``mc_pairing='cross'``: the guidance over all ``mc_batch_size ** 2`` pairs of the MC set (``paired_sampler``).
    `guidance_strength` may also hold one strength per sample and `guidance_schedule` scales it per stage
    (``paired_sampler``, ``utils/guidance_schedule.py``).  `sde_eta`, `sde_seed`: the stochastic sampler
    (``paired_sampler``).  `ess_floor`: the effective-sample-size floor of the importance weights (``paired_sampler``).
    """
    return paired_sampler(fm_x, fm_y, ratio_estimator, guidance_method, guidance_strength,
                          num_samples, num_steps, device, mc_batch_size, (1, 28, 28), (1, 28, 28), solver=solver,
                          diagnostics=diagnostics, mc_pairing=mc_pairing, guidance_schedule=guidance_schedule,
                          sde_eta=sde_eta, sde_seed=sde_seed, ess_floor=ess_floor, labels=labels, cfg_scale=cfg_scale)
