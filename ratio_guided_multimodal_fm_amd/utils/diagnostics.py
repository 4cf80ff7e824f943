"""Guidance diagnostics: what the reference prints once per run (``src/utils/flow_utils.py:349-363``: ``sigma_t``,
``||v||``, ``||g||``, the weight range, ``Z_bar``) as per-sample, per-stage curves, plus the effective sample size of
the importance weights.

Pass a ``GuidanceDiagnostics()`` as ``diagnostics=`` to ``paired_sampler``, ``sample_bimodal_guided``,
``sample_bimodal_guided_mnist_svhn`` or ``sample_conditional`` (either guidance method, either solver).  The sampler's
return value and its bits do not change; after the call the object holds

    records   device tensor [n_stages, B, 8] (include/rgfm.h, RGFM_DIAG_*), written by the loop's own kernels with no
              host synchronisation: n_stages = num_steps for 'euler', 2 num_steps for 'midpoint' (stage 1, stage 2 of
              each step)
    t, sigma_t   float64 CPU tensors [n_stages]: each stage's time by the loops' own formulas and 1 - t + 1e-3
    guided    bool CPU tensor [n_stages]: the stage ran with guidance ('mc_feng': t > 1e-3 and an MC set; the first
              stage of a run never is, and its records are all zero)
    tau       with ``ess_floor=`` only (else None): device tensor [n_stages, B], the exponent each row's importance
              weights were tempered by at the stage -- 1: the row was at or above the floor and kept its weights,
              0: the stage ran unguided.  ess / w_max / w_min are then those of the tempered weights, z_bar stays the
              untempered value

MC guidance fills every field; an effective sample size near 1 means one MC sample carries the row ("copy the nearest
MC sample").  Gradient log-ratio guidance fills the four norms (``g`` is ``grad log r`` before gamma) and leaves
ess / w_max / w_min / z_bar at 0.  One-sided (conditional) sampling leaves the ``_y`` fields at 0.

Cross pairing (``mc_pairing='cross'``: the guidance over all N x N pairs of the MC set, N = mc_batch_size): the records
describe the N^2 joint weights w_ij through what the loop forms of them.  ``ess`` is the JOINT effective sample size
(sum_ij w_ij)^2 / sum_ij w_ij^2, 1 .. N^2 (compare it with N^2, not N); ``w_max`` / ``w_min`` are the max and min over
the 2N marginal weights wx_i = sum_j w_ij, wy_j = sum_i w_ij (each marginal sums to 1, as a paired row does);
``z_bar`` is mean_ij R_ij a_i b_j + 1e-10; the four norms are as before, g formed from the marginal weights.
``reference_block`` and ``row_metrics`` read such records unchanged.

Sharded launches (``distributed.py``) are out of scope: they take no ``diagnostics=``.
"""
import torch

FIELDS = ("ess", "w_max", "w_min", "z_bar", "v_norm_x", "v_norm_y", "g_norm_x", "g_norm_y")
DIAG_FLOATS = len(FIELDS)  # RGFM_DIAG_FLOATS
EPS = 1e-3
METHODS = ("none", "mc_feng", "grad_log_ratio")


def stage_times(num_steps, solver="euler", step_begin=0, step_end=None):
    """Times of the stages of steps [step_begin, step_end) as Python doubles, in the loops' stage order and by their
    formulas (csrc/sampler_stages.h): Euler ``t = step * (1.0 / num_steps)``; midpoint ``t1`` as Euler, then
    ``t2 = (step + 0.5) * (1.0 / num_steps)``."""
    if solver not in ("euler", "midpoint"):
        raise ValueError(f"solver must be 'euler' or 'midpoint', got {solver!r}")
    if not isinstance(num_steps, int) or num_steps < 1:
        raise ValueError(f"num_steps must be an integer >= 1, got {num_steps!r}")
    step_end = num_steps if step_end is None else step_end
    if not 0 <= step_begin <= step_end <= num_steps:
        raise ValueError(f"bad step range [{step_begin},{step_end}) of {num_steps}")
    dtd = 1.0 / float(num_steps)
    out = []
    for step in range(step_begin, step_end):
        out.append(float(step) * dtd)
        if solver == "midpoint":
            out.append((float(step) + 0.5) * dtd)
    return out


def check(diagnostics):
    """None or a GuidanceDiagnostics; anything else is a TypeError (raised before any device work)."""
    if diagnostics is not None and not isinstance(diagnostics, GuidanceDiagnostics):
        raise TypeError(f"diagnostics must be a GuidanceDiagnostics or None, got {type(diagnostics).__name__}")
    return diagnostics


class GuidanceDiagnostics:
    """Per-sample, per-stage guidance diagnostics of one sampler call (module docstring)."""

    def __init__(self):
        self.records = self.t = self.sigma_t = self.guided = None
        self.tau = None  # with ess_floor=: the rows' tempering exponents [n_stages, B] (1: untouched, 0: unguided stage)
        self.method = self.solver = None
        self.num_steps = self.step_begin = None

    # ---- filled by the samplers
    def _schedule(self, method, solver, num_steps, step_begin=0, step_end=None, has_mc=True):
        if method not in METHODS:
            raise ValueError(f"guidance method must be one of {METHODS}, got {method!r}")
        ts = stage_times(num_steps, solver, step_begin, step_end)
        self.method, self.solver, self.num_steps, self.step_begin = method, solver, num_steps, step_begin
        self.t = torch.tensor(ts, dtype=torch.float64)
        self.sigma_t = torch.tensor([1 - t + EPS for t in ts], dtype=torch.float64)
        if method == "mc_feng":
            self.guided = torch.tensor([bool(has_mc) and t > EPS for t in ts], dtype=torch.bool)
        else:
            self.guided = torch.full((len(ts),), method == "grad_log_ratio", dtype=torch.bool)
        return len(ts)

    def _begin(self, method, solver, num_steps, batch, device, step_begin=0, step_end=None, has_mc=True, stage_scale=None):
        """Sets the schedule and returns a fresh records tensor [n_stages, batch, 8] on `device` for the loop.
        `stage_scale` (a guidance schedule's per-stage values): a stage whose scale is 0 runs unguided."""
        n = self._schedule(method, solver, num_steps, step_begin, step_end, has_mc)
        if stage_scale is not None:
            self.guided = self.guided & torch.tensor([float(v) != 0.0 for v in stage_scale], dtype=torch.bool)
        self.records = torch.zeros(n, batch, DIAG_FLOATS, dtype=torch.float32, device=device)
        self.tau = None
        return self.records

    def _begin_tau(self):
        """A fresh exponents tensor [n_stages, batch] beside the records of _begin, for a loop with an ess_floor."""
        self.tau = torch.zeros(self.records.shape[:2], dtype=torch.float32, device=self.records.device)
        return self.tau

    @classmethod
    def from_records(cls, records, method, solver, num_steps, step_begin=0, step_end=None, has_mc=True):
        """A filled object around existing records [n_stages, B, 8] (any device): saved arrays, tests."""
        d = cls()
        n = d._schedule(method, solver, num_steps, step_begin, step_end, has_mc)
        records = torch.as_tensor(records)
        if records.dim() != 3 or records.shape[0] != n or records.shape[2] != DIAG_FLOATS:
            raise ValueError(f"records of shape [{n},B,{DIAG_FLOATS}] expected, got {tuple(records.shape)}")
        d.records = records
        return d

    # ---- reading
    def _field(self, name):
        if self.records is None:
            raise RuntimeError("no records yet: pass this object as diagnostics= to a sampler first")
        return self.records[..., FIELDS.index(name)]

    def ess(self):
        """Effective sample size (sum w)^2 / sum w^2 of each row's importance weights [n_stages, B]; 0: not MC-guided."""
        return self._field("ess")

    def w_max(self):
        return self._field("w_max")

    def w_min(self):
        return self._field("w_min")

    def z_bar(self):
        return self._field("z_bar")

    def v_norm_x(self):
        return self._field("v_norm_x")

    def v_norm_y(self):
        return self._field("v_norm_y")

    def g_norm_x(self):
        return self._field("g_norm_x")

    def g_norm_y(self):
        return self._field("g_norm_y")

    def stage_of_step(self, step):
        """Index of the (first) stage of step `step` of the run."""
        per = 2 if self.solver == "midpoint" else 1
        i = (int(step) - self.step_begin) * per
        if self.records is None or not 0 <= i < self.records.shape[0]:
            raise IndexError(f"step {step} is not among the recorded steps")
        return i

    def summary(self, stage):
        """Plain numbers of one stage: means over the rows; the weight range as the reference prints it (min and max
        over all rows' weights); ess also at its minimum over the rows.  Synchronises with the device."""
        if self.records is None:
            raise RuntimeError("no records yet: pass this object as diagnostics= to a sampler first")
        r = self.records[stage].double().cpu()
        mean = lambda name: float(r[:, FIELDS.index(name)].mean())
        out = {"stage": int(stage), "t": float(self.t[stage]), "sigma_t": float(self.sigma_t[stage]),
               "guided": bool(self.guided[stage]), "ess_mean": mean("ess"), "ess_min": float(r[:, 0].min()),
               "w_max": float(r[:, 1].max()), "w_min": float(r[:, 2].min()), "z_bar": mean("z_bar")}
        for name in FIELDS[4:]:
            out[name] = mean(name)
        return out

    def reference_block(self, step):
        """The text of the reference's diagnostics print (``src/utils/flow_utils.py:357-362``) for step `step` of the
        run, in its format (midpoint: the step's first stage).  MC guidance only; '' when that stage ran unguided
        (the reference prints from inside its guided branch)."""
        if self.method != "mc_feng":
            raise ValueError("the reference prints this block for mc_feng guidance only; use summary() for "
                             f"{self.method!r}")
        s = self.summary(self.stage_of_step(step))
        if not s["guided"]:
            return ""
        return (f"\n[MC Guidance Diagnostics at t={s['t']:.2f}]\n"
                f"  sigma_t={s['sigma_t']:.4f}\n"
                f"  ||v_x||={s['v_norm_x']:.4f}, ||v_y||={s['v_norm_y']:.4f}\n"
                f"  ||g_x||={s['g_norm_x']:.4f}, ||g_y||={s['g_norm_y']:.4f}\n"
                f"  weights: min={s['w_min']:.6f}, max={s['w_max']:.6f}\n"
                f"  Z_bar: {s['z_bar']:.4f}")

    def save(self, path):
        """records, t and sigma_t (and the guided mask) as a .npz file."""
        import numpy as np
        np.savez(path, records=self.records.cpu().numpy(), t=self.t.numpy(), sigma_t=self.sigma_t.numpy(),
                 guided=self.guided.numpy())


# ---- the command-line tools
def add_cli_args(p, sampling=True):
    """--diagnostics (and, for the sampling tools, --diagnostics_out) of the command-line tools."""
    if not sampling:
        p.add_argument('--diagnostics', action='store_true',
                       help='add ess_mean, ess_min and w_max of the importance weights at step int(0.3 * num_steps) to '
                            'each result row (utils/diagnostics.py); not with --sharded')
        return
    p.add_argument('--diagnostics', action='store_true',
                   help="guidance diagnostics (utils/diagnostics.py): print the reference's diagnostics block "
                        "(sigma_t, ||v||, ||g||, weight range, Z_bar) at step int(0.3 * num_steps), plus the effective "
                        "sample size of the importance weights there; not with --sharded")
    p.add_argument('--diagnostics_out', type=str, default=None, metavar='FILE.npz',
                   help='save the per-stage, per-sample diagnostics records [n_stages, B, 8] with t and sigma_t per stage')


def report_diagnostics(diag, num_steps, show, out_path):
    """--diagnostics / --diagnostics_out of the sampling tools: the reference's block at its step (with the effective
    sample size under it), and the .npz."""
    if diag is None or diag.records is None:
        return
    if show:
        step = int(0.3 * num_steps)
        s = diag.summary(diag.stage_of_step(step))
        if diag.method == 'mc_feng':
            print(diag.reference_block(step) or f"\n[MC Guidance Diagnostics: step {step} ran unguided]")
            print(f"  ESS: mean={s['ess_mean']:.2f}, min={s['ess_min']:.2f}")
        else:
            print(f"\n[Guidance Diagnostics at t={s['t']:.2f}]\n  ||v_x||={s['v_norm_x']:.4f}, ||v_y||={s['v_norm_y']:.4f}\n"
                  f"  ||g_x||={s['g_norm_x']:.4f}, ||g_y||={s['g_norm_y']:.4f}")
    if out_path:
        diag.save(out_path)
        print(f"Saved diagnostics: {out_path}")


def row_metrics(diag, num_steps):
    """ess_mean, ess_min and w_max at step int(0.3 * num_steps): what --diagnostics adds to an evaluation row."""
    s = diag.summary(diag.stage_of_step(int(0.3 * num_steps)))
    return {k: s[k] for k in ('ess_mean', 'ess_min', 'w_max')}
