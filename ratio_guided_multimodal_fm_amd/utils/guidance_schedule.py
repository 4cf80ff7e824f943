"""Guidance strength as data: a scale per stage (``GuidanceSchedule``) and a strength per sample.

Every guided sampler takes ``guidance_strength`` (a float, or a 1-D tensor / sequence with one strength per sample)
and ``guidance_schedule`` (None, a ``GuidanceSchedule``, a callable ``s(t)`` or a sequence of per-stage values).  For
row b and stage k of the main loop the effective strength is ``float64(gamma_b) * s_k`` (include/rgfm.h, "Guidance
strength per sample and per stage").  A stage with ``s_k == 0`` runs unguided: no guidance block, no ratio-estimator
pass.  ``window(t_lo, t_hi)`` guides inside a time window only (the usual remedy against the late collapse of the
importance weights that ``utils/diagnostics.py`` shows), ``linear`` / ``cosine`` let the strength decay with t.

The stage times are those of ``utils.diagnostics.stage_times``: the one statement of them on the Python side.
"""
import math

import torch

from .diagnostics import stage_times

KINDS = ("constant", "linear", "cosine")


class GuidanceSchedule:
    """A per-stage scale s(t) of the guidance strength.  Build one with the constructors below."""

    def __init__(self, kind, fn=None, values=None, text=None):
        self.kind, self._fn, self._values, self._text = kind, fn, values, text or kind

    def __repr__(self):
        return f"GuidanceSchedule.{self._text}"

    @classmethod
    def constant(cls):
        """s = 1 at every stage: the strength itself."""
        return cls("constant", lambda t: 1.0, text="constant()")

    @classmethod
    def window(cls, t_lo, t_hi):
        """1 where t_lo <= t <= t_hi (both edges inclusive), else 0."""
        t_lo, t_hi = float(t_lo), float(t_hi)
        if not (math.isfinite(t_lo) and math.isfinite(t_hi) and t_lo <= t_hi):
            raise ValueError(f"window needs finite t_lo <= t_hi, got {t_lo!r}, {t_hi!r}")
        return cls("window", lambda t: 1.0 if t_lo <= t <= t_hi else 0.0, text=f"window({t_lo!r}, {t_hi!r})")

    @classmethod
    def linear(cls, start=1.0, end=0.0):
        """start + (end - start) t."""
        start, end = float(start), float(end)
        return cls("linear", lambda t: start + (end - start) * t, text=f"linear({start!r}, {end!r})")

    @classmethod
    def cosine(cls, start=1.0, end=0.0):
        """end + (start - end) (1 + cos(pi t)) / 2: `start` at t = 0, `end` at t = 1, flat at both ends."""
        start, end = float(start), float(end)
        return cls("cosine", lambda t: end + (start - end) * 0.5 * (1.0 + math.cos(math.pi * t)),
                   text=f"cosine({start!r}, {end!r})")

    @classmethod
    def from_values(cls, seq):
        """Explicit per-stage values, one per stage of the call (its length is checked by ``stage_values``)."""
        vals = [float(v) for v in (seq.tolist() if isinstance(seq, torch.Tensor) else seq)]
        return cls("values", values=vals, text=f"from_values(<{len(vals)} values>)")

    @classmethod
    def from_callable(cls, fn):
        """s(t) = fn(t), t a Python float."""
        if not callable(fn):
            raise TypeError(f"from_callable needs a callable, got {type(fn).__name__}")
        return cls("callable", fn, text=f"from_callable({getattr(fn, '__name__', 'fn')})")

    def stage_values(self, num_steps, solver="euler", step_begin=0, step_end=None):
        """Python floats, one per stage of steps [step_begin, step_end), at the times of
        ``utils.diagnostics.stage_times`` (Euler: one stage per step; midpoint: two).  A ``from_values`` schedule of
        another length is a ValueError."""
        ts = stage_times(num_steps, solver, step_begin, step_end)
        if self._values is not None:
            if len(self._values) != len(ts):
                raise ValueError(f"the schedule holds {len(self._values)} values, the call has {len(ts)} stages "
                                 f"(solver={solver!r}, steps [{step_begin},{num_steps if step_end is None else step_end}))")
            return list(self._values)
        return [float(self._fn(t)) for t in ts]


def as_schedule(schedule):
    """None | GuidanceSchedule | callable | sequence -> None | GuidanceSchedule (anything else: TypeError)."""
    if schedule is None or isinstance(schedule, GuidanceSchedule):
        return schedule
    if callable(schedule):
        return GuidanceSchedule.from_callable(schedule)
    if isinstance(schedule, (list, tuple, torch.Tensor)):
        return GuidanceSchedule.from_values(schedule)
    raise TypeError(f"guidance_schedule must be None, a GuidanceSchedule, a callable or a sequence, got "
                    f"{type(schedule).__name__}")


def resolve_strength(guidance_strength, rows, what="num_samples"):
    """(gamma, gamma_rows): a scalar strength is (float, None) -- today's call; a 1-D tensor / sequence of length
    `rows` is (0.0, CPU fp32 tensor [rows]).  Wrong length, rank or dtype: ValueError.  No device work."""
    g = guidance_strength
    if isinstance(g, torch.Tensor):
        if g.dim() == 0:
            return float(g), None
        if g.dim() != 1:
            raise ValueError(f"guidance_strength: a number or a 1-D tensor of length {what} = {rows} expected, got shape "
                             f"{tuple(g.shape)}")
        if not (g.dtype.is_floating_point or g.dtype in (torch.int32, torch.int64)):
            raise ValueError(f"guidance_strength: a real tensor expected, got {g.dtype}")
        vec = g.detach().to(torch.float32)
    elif isinstance(g, (list, tuple)):
        try:
            vec = torch.tensor([float(v) for v in g], dtype=torch.float32)
        except TypeError:
            raise ValueError(f"guidance_strength: a number or a flat sequence of {rows} numbers expected") from None
    else:
        try:
            import numpy as np
            if isinstance(g, np.ndarray) and g.ndim:
                if g.ndim != 1:
                    raise ValueError(f"guidance_strength: a number or a 1-D array of length {what} = {rows} expected, got "
                                     f"shape {g.shape}")
                vec = torch.as_tensor(g).to(torch.float32)
            else:
                return g, None
        except ImportError:
            return g, None
    if vec.shape[0] != rows:
        raise ValueError(f"guidance_strength holds {vec.shape[0]} strengths, {what} = {rows}")
    return 0.0, vec


def resolve(guidance_strength, guidance_schedule, rows, num_steps, solver, what="num_samples"):
    """(gamma, gamma_rows, stage_scale) of a sampler call, all checks done and nothing on the device: the scalar (as
    given), the per-row vector or None, the per-stage Python floats or None."""
    gamma, vec = resolve_strength(guidance_strength, rows, what)
    sched = as_schedule(guidance_schedule)
    scale = None if sched is None else sched.stage_values(num_steps, solver)
    return gamma, vec, scale


# ---- the command-line tools
def add_cli_args(p):
    """--guidance_schedule / --guidance_window of the command-line tools."""
    p.add_argument('--guidance_schedule', type=str, default=None, choices=list(KINDS),
                   help="scale of the guidance strength over t (utils/guidance_schedule.py): 'constant' (1), 'linear' "
                        "(1 - t), 'cosine' ((1 + cos(pi t)) / 2); U-Net nets, not with --sharded")
    p.add_argument('--guidance_window', type=float, nargs=2, default=None, metavar=('T_LO', 'T_HI'),
                   help='guide only at stages with T_LO <= t <= T_HI (the other stages run unguided and skip the guidance '
                        'work); multiplies --guidance_schedule when both are given')


def from_cli(args):
    """The schedule the two flags describe, or None when neither is given."""
    kind, win = getattr(args, 'guidance_schedule', None), getattr(args, 'guidance_window', None)
    if kind is None and win is None:
        return None
    base = {None: GuidanceSchedule.constant, 'constant': GuidanceSchedule.constant, 'linear': GuidanceSchedule.linear,
            'cosine': GuidanceSchedule.cosine}[kind]()
    if win is None:
        return base
    w = GuidanceSchedule.window(win[0], win[1])
    if kind in (None, 'constant'):
        return w
    return GuidanceSchedule("callable", lambda t: base._fn(t) * w._fn(t), text=f"{base._text} * {w._text}")
