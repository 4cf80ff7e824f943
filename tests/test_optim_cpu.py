"""CPU-only checks of the optimizer step (utils/optim.py, csrc/optim.hip): the float64 restatement against
torch.optim.Adam itself, the three C exports, state_dict round trips through torch.optim.Adam, the trainers' new
arguments and load_checkpoint(ema=True)."""
import copy
import ctypes
import os
import re

import pytest
import torch

from optim_ref64 import RefAdam64
from ratio_guided_multimodal_fm_amd import _lib, train_classifier, train_flow, train_ratio
from ratio_guided_multimodal_fm_amd.utils import load_checkpoint
from ratio_guided_multimodal_fm_amd.utils.optim import Adam

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
SHAPES = [(1,), (3,), (5, 7), (64,), (257,), (4, 3, 3, 3)]


def make_params(seed, dtype=torch.float32, shapes=SHAPES):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g, dtype=torch.float64).to(dtype).requires_grad_(True) for s in shapes]


def make_grads(seed, step, params):
    g = torch.Generator().manual_seed(1000 * seed + step)
    return [torch.randn(p.shape, generator=g, dtype=torch.float64) for p in params]


# ---- 1. the restatement against torch.optim.Adam (float64, CPU) ------------------------------------------------------
@pytest.mark.parametrize("wd,decoupled", [(0.0, False), (0.05, False), (0.05, True)])
@pytest.mark.parametrize("max_norm", [None, 0.5, 1e3])
def test_restatement_matches_torch_adam(wd, decoupled, max_norm):
    """Same arithmetic in the same precision: 1e-12 relative only pins that the restatement is written down correctly."""
    decay, lr = 0.9, 3e-3
    params = make_params(1, torch.float64)
    ref = RefAdam64([dict(params=params, lr=lr, weight_decay=wd, decoupled=decoupled)], max_grad_norm=max_norm,
                    ema_decay=decay)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls(params, lr=lr, weight_decay=wd, foreach=False)
    ema = [p.detach().clone() for p in params]
    for step in range(5):
        grads = make_grads(1, step, params)
        for i, (p, g) in enumerate(zip(params, grads)):
            p.grad = None if (i == 2 and step in (1, 2)) else g.clone()  # a skipped parameter keeps its own step count
        norm = ref.step([[None if p.grad is None else p.grad for p in params]])
        if max_norm is not None:
            total = torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
            assert abs(float(total) - norm) <= 1e-12 * norm
        opt.step()
        with torch.no_grad():
            for e, p in zip(ema, params):
                if p.grad is not None:
                    e.lerp_(p, 1 - decay)
    assert ref.steps[2] == 3 and ref.steps[0] == 5
    for i, p in enumerate(params):
        st = opt.state[p]
        for name, got, want in (("p", ref.params[i], p.detach()), ("exp_avg", ref.exp_avg[i], st["exp_avg"]),
                                ("exp_avg_sq", ref.exp_avg_sq[i], st["exp_avg_sq"]), ("ema", ref.ema[i], ema[i])):
            err = float((got - want).abs().max())
            assert err <= 1e-12 * float(want.abs().max()), (i, name, err)


# ---- 2. the C ABI ----------------------------------------------------------------------------------------------------
def test_exports_and_abi_version():
    L = _lib.lib()
    for name in ("rgfm_adam_workspace_bytes", "rgfm_adam_grad_norm", "rgfm_adam_step"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert L.rgfm_abi_version() == 3 == _lib.ABI_VERSION
    hdr = open(os.path.join(ROOT, "include", "rgfm.h")).read()
    assert re.search(r"#define RGFM_ABI_VERSION 3\b", hdr)
    assert ctypes.sizeof(_lib.AdamEntry) == 48
    n = ctypes.c_size_t()
    assert L.rgfm_adam_workspace_bytes(ctypes.byref(n)) == 0 and n.value >= 8 and n.value % 16 == 0


def test_null_and_inconsistent_arguments_return_einval():
    L = _lib.lib()
    d = _lib.AdamDesc()
    d.lr, d.eps, d.weight_decay, d.max_grad_norm, d.ema_decay = 1e-3, 1e-8, 0.0, 0.0, -1.0
    d.betas[0], d.betas[1] = 0.9, 0.999
    fake = 0x1000  # (never dereferenced: every call below fails its argument checks first)
    assert L.rgfm_adam_workspace_bytes(None) == -1
    assert L.rgfm_adam_grad_norm(None, 1, 0, 4, fake, 1 << 20, None) == -1
    assert b"table" in L.rgfm_last_error()
    assert L.rgfm_adam_grad_norm(fake, 1, 0, 4, None, 0, None) == -1
    assert L.rgfm_adam_grad_norm(fake, 0, 0, 4, fake, 1 << 20, None) == -1
    assert L.rgfm_adam_grad_norm(fake, 1, 0, 6, fake, 1 << 20, None) == -1  # not whole quads
    assert L.rgfm_adam_step(None, fake, 1, 0, 4, fake, fake, None, None, None, 0, None) == -1
    assert L.rgfm_adam_step(ctypes.byref(d), None, 1, 0, 4, fake, fake, None, None, None, 0, None) == -1
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 0, 4, None, fake, None, None, None, 0, None) == -1
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 0, 4, fake, None, None, None, None, 0, None) == -1
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 4, 4, fake, fake, None, None, None, 0, None) == -1  # empty span
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 0, 4, fake + 4, fake, None, None, None, 0, None) == -1
    assert b"aligned" in L.rgfm_last_error()
    d.ema_decay = 0.99  # an EMA without its buffer
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 0, 4, fake, fake, None, None, None, 0, None) == -1
    d.ema_decay = -1.0  # a buffer without an EMA
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 0, 4, fake, fake, fake, None, None, 0, None) == -1
    d.max_grad_norm = 1.0  # a clip without the workspace of the norm
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 0, 4, fake, fake, None, None, None, 0, None) == -1
    d.max_grad_norm, d.betas[0] = 0.0, 1.0
    assert L.rgfm_adam_step(ctypes.byref(d), fake, 1, 0, 4, fake, fake, None, None, None, 0, None) == -1
    assert b"betas" in L.rgfm_last_error()


# ---- 3. state_dict ---------------------------------------------------------------------------------------------------
def fill_state(opt, seed):
    g = torch.Generator().manual_seed(seed)
    for k, buf in opt._flat.items():
        buf.copy_(torch.rand(buf.shape, generator=g))
    opt._steps[:] = torch.arange(len(opt._steps)).numpy() + 3


def test_state_dict_round_trip_through_torch_adam():
    params = make_params(2)
    a = Adam(params, lr=2e-3, ema_decay=0.9)
    fill_state(a, 7)
    sd = a.state_dict()
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "ema"}
    t = torch.optim.Adam(params, lr=1e-3, foreach=False)
    # the extra key is carried along, the moments and the step are what torch.optim.Adam uses (a deep copy: torch's
    # load_state_dict keeps the 'step' tensors it is given and its step() counts in them)
    t.load_state_dict(copy.deepcopy(sd))
    assert float(t.state[params[1]]["step"]) == 4.0 and t.param_groups[0]["lr"] == 2e-3
    assert torch.equal(t.state[params[1]]["exp_avg"], a.state[params[1]]["exp_avg"])
    for p in params:
        p.grad = torch.zeros_like(p)
    t.step()  # (loads into a working optimizer)
    t.load_state_dict(sd)
    b = Adam(make_params(2), lr=1e-3, ema_decay=0.9)
    b.load_state_dict(t.state_dict())
    assert b.param_groups[0]["lr"] == 2e-3
    assert (b._steps == a._steps).all()
    for k in ("exp_avg", "exp_avg_sq", "ema"):  # (the slots' padding is not state: compared per tensor)
        for pa, pb in zip(a._order, b._order):
            assert torch.equal(a.state[pa][k], b.state[pb][k]), k
    sd2 = b.state_dict()
    for i in sd["state"]:
        for k, v in sd["state"][i].items():
            assert torch.equal(v, sd2["state"][i][k]), (i, k)


def test_torch_written_state_loads_and_the_ema_starts_from_the_parameters():
    params = make_params(3)
    t = torch.optim.Adam(params, lr=1e-3, foreach=False)
    for step in range(2):
        for p, g in zip(params, make_grads(3, step, params)):
            p.grad = g.float()
        t.step()
    a = Adam(params, lr=5e-4, ema_decay=0.99)
    for p in params:
        a.state[p]["ema"].zero_()
    a.load_state_dict(t.state_dict())
    for i, p in enumerate(params):
        assert torch.equal(a.state[p]["ema"], p.detach())
        assert torch.equal(a.state[p]["exp_avg_sq"], t.state[p]["exp_avg_sq"])
        assert a._steps[i] == 2 and float(a.state_dict()["state"][i]["step"]) == 2.0
    assert a.param_groups[0]["lr"] == 1e-3


def test_loaded_state_still_aliases_the_flat_buffers():
    params = make_params(4)
    a, b = Adam(params, ema_decay=0.5), Adam(params, ema_decay=0.5)
    fill_state(a, 9)
    b.load_state_dict(a.state_dict())
    for k, buf in b._flat.items():
        lo, hi = buf.data_ptr(), buf.data_ptr() + 4 * buf.numel()
        for i, p in enumerate(params):
            v = b.state[p][k]
            assert lo <= v.data_ptr() and v.data_ptr() + 4 * v.numel() <= hi, (k, i)
            assert v.data_ptr() == lo + 4 * int(b._offset[i]) and int(b._offset[i]) % 4 == 0
            assert v.shape == p.shape
        buf.fill_(2.5)
        assert all(float(b.state[p][k].min()) == 2.5 for p in params)


# ---- 4. trainers' arguments, load_checkpoint ------------------------------------------------------------------------
CLIS = [(train_flow, ["--preset", "svhn", "--data", "d.npy"]), (train_ratio, ["--kind", "mnist28", "--data", "d.npz"]),
        (train_classifier, ["--kind", "svhn", "--data", "d.npz"])]


@pytest.mark.parametrize("mod,argv", CLIS, ids=["flow", "ratio", "classifier"])
def test_optimizer_arguments(mod, argv):
    a = mod.parse_args(argv)
    assert (a.optimizer, a.ema_decay, a.max_grad_norm, a.weight_decay) == ("torch", None, None, None)
    for flag in (["--ema_decay", "0.999"], ["--max_grad_norm", "1.0"], ["--weight_decay", "0.01"]):
        with pytest.raises(SystemExit):
            mod.parse_args(argv + flag)
        with pytest.raises(SystemExit):
            mod.parse_args(argv + ["--optimizer", "torch"] + flag)
    a = mod.parse_args(argv + ["--optimizer", "hip", "--ema_decay", "0.999", "--max_grad_norm", "2.0", "--weight_decay", "0.01"])
    assert (a.optimizer, a.ema_decay, a.max_grad_norm, a.weight_decay) == ("hip", 0.999, 2.0, 0.01)
    with pytest.raises(SystemExit):
        mod.parse_args(argv + ["--optimizer", "sgd"])


def test_defaults_leave_the_existing_arguments_alone():
    a = train_flow.parse_args(["--preset", "svhn", "--data", "d.npy"])
    assert (a.epochs, a.batch_size, a.lr, a.seed, a.patience, a.save_every, a.resume) == (50, 128, 1e-4, 42, 10, 10, None)
    a = train_ratio.parse_args(["--kind", "mnist28", "--data", "d.npz"])
    assert (a.epochs, a.batch_size, a.lr, a.real_fake_ratio, a.loss_type) == (30, 128, 1e-4, 0.5, "disc")
    a = train_classifier.parse_args(["--kind", "mnist28", "--data", "d.npz"])
    assert (a.epochs, a.batch_size, a.lr) == (3, 128, 1e-3)


def test_build_optimizer_follows_the_arguments():
    from ratio_guided_multimodal_fm_amd.utils.optim import build_optimizer, ema_path
    params = make_params(5)
    a = train_ratio.parse_args(["--kind", "mnist28", "--data", "d.npz"])
    assert type(build_optimizer(a, params, default_max_grad_norm=1.0)) is torch.optim.Adam
    a = train_ratio.parse_args(["--kind", "mnist28", "--data", "d.npz", "--optimizer", "hip"])
    o = build_optimizer(a, params, default_max_grad_norm=1.0)
    assert isinstance(o, Adam) and o.max_grad_norm == 1.0 and o.ema_decay is None and o.param_groups[0]["lr"] == 1e-4
    a = train_ratio.parse_args(["--kind", "mnist28", "--data", "d.npz", "--optimizer", "hip", "--max_grad_norm", "3", "--ema_decay", "0.5"])
    o = build_optimizer(a, params, default_max_grad_norm=1.0)
    assert o.max_grad_norm == 3.0 and o.ema_decay == 0.5
    assert ema_path("checkpoints/svhn_classifier.pth") == "checkpoints/svhn_classifier_ema.pth"


def test_load_checkpoint_ema(tmp_path):
    m = torch.nn.Linear(3, 2)
    avg = {k: v + 1 for k, v in m.state_dict().items()}
    torch.save({"epoch": 4, "model_state_dict": m.state_dict(), "ema_state_dict": avg, "best_loss": 0.5}, tmp_path / "c.pth")
    live, ema = torch.nn.Linear(3, 2), torch.nn.Linear(3, 2)
    assert load_checkpoint(live, str(tmp_path / "c.pth")) == {"epoch": 4, "best_loss": 0.5}
    assert load_checkpoint(ema, str(tmp_path / "c.pth"), ema=True) == {"epoch": 4, "best_loss": 0.5}
    assert torch.equal(live.weight, m.weight) and torch.equal(ema.weight, m.weight + 1) and torch.equal(ema.bias, m.bias + 1)
    torch.save({"epoch": 4, "model_state_dict": m.state_dict(), "best_loss": 0.5}, tmp_path / "plain.pth")
    torch.save(m.state_dict(), tmp_path / "raw.pth")
    for name in ("plain.pth", "raw.pth"):
        with pytest.raises(KeyError, match="ema_state_dict"):
            load_checkpoint(ema, str(tmp_path / name), ema=True)
        load_checkpoint(live, str(tmp_path / name))


def test_ema_state_dict_keys_and_buffers():
    m = torch.nn.Sequential(torch.nn.Linear(3, 3), torch.nn.BatchNorm1d(3))
    o = Adam(m.parameters(), ema_decay=0.9)
    m[1].running_mean.fill_(0.25)
    for p in m.parameters():
        o.state[p]["ema"].fill_(7.0)
    sd = o.ema_state_dict(m)
    assert list(sd) == list(m.state_dict())
    assert float(sd["0.weight"].min()) == 7.0 and float(sd["1.bias"].max()) == 7.0
    assert float(sd["1.running_mean"].min()) == 0.25 and int(sd["1.num_batches_tracked"]) == 0
    with pytest.raises(_lib.RgfmError, match="EMA"):
        Adam(m.parameters()).ema_state_dict(m)


def test_step_on_cpu_parameters_raises():
    params = make_params(6)
    o = Adam(params, lr=1e-3)
    for p in params:
        p.grad = torch.ones_like(p)
    before = [p.detach().clone() for p in params]
    with pytest.raises(_lib.RgfmError, match="HIP device"):
        o.step()
    assert all(torch.equal(a, b) for a, b in zip(before, params))


def test_ratio_trainer_leaves_the_clip_to_an_optimizer_that_has_one(monkeypatch):
    """RatioTrainer.train_step clips with torch as before, unless the optimizer carries a max_grad_norm of its own."""
    from types import SimpleNamespace
    from ratio_guided_multimodal_fm_amd.utils.losses import get_ratio_loss
    from ratio_guided_multimodal_fm_amd.utils.trainer import RatioTrainer

    class Scorer(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(8, 1)

        def forward(self, x, y):
            return self.lin(torch.cat([x, y], 1)).squeeze(1)

    calls = []
    real_clip = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda *a, **k: (calls.append(k.get("max_norm")), real_clip(*a, **k))[1])
    m = Scorer()
    batch = {"x": torch.randn(6, 4), "y": torch.randn(6, 4), "is_real": torch.tensor([1, 0, 1, 0, 1, 0])}
    RatioTrainer(m, get_ratio_loss("disc"), torch.optim.Adam(m.parameters(), lr=1e-3), "cpu").train_step(batch)
    assert calls == [1.0]
    stepped = []
    own_clip = SimpleNamespace(max_grad_norm=1.0, zero_grad=lambda: None, step=lambda: stepped.append(1))
    RatioTrainer(m, get_ratio_loss("disc"), own_clip, "cpu").train_step(batch)
    assert calls == [1.0] and stepped == [1]
    no_clip = SimpleNamespace(max_grad_norm=None, zero_grad=lambda: None, step=lambda: stepped.append(2))
    RatioTrainer(m, get_ratio_loss("disc"), no_clip, "cpu").train_step(batch)
    assert calls == [1.0, 1.0]


def test_raw_state_dict_trainers_write_a_sibling_ema_file(tmp_path, monkeypatch):
    from types import SimpleNamespace
    from helpers import make_module
    monkeypatch.chdir(tmp_path)
    clf = make_module("clf_mnist28")
    opt = Adam(clf.parameters(), ema_decay=0.5)
    for p in clf.parameters():
        opt.state[p]["ema"].fill_(3.0)
    path = train_classifier.save_checkpoint(clf, "mnist28", opt)
    assert path == "checkpoints/mnist_classifier.pth"
    raw, avg = torch.load(path), torch.load("checkpoints/mnist_classifier_ema.pth")
    assert list(raw) == list(avg) == list(clf.state_dict())
    assert all(float(v.min()) == 3.0 for v in avg.values()) and torch.equal(raw["fc2.bias"], clf.fc2.bias)
    train_classifier.save_checkpoint(clf, "mnist32", torch.optim.Adam(clf.parameters()))
    assert not os.path.exists("checkpoints/mnist32_classifier_ema.pth")
    ratio = make_module("ratio28")
    args = SimpleNamespace(kind="mnist_svhn", loss_type="disc", transform_type="rotate90")
    ropt = Adam(ratio.parameters(), ema_decay=0.5)
    train_ratio.save_checkpoint(ratio, args, train_ratio.checkpoint_path(args, "best"), 1, 0.5, ropt)
    avg = torch.load("checkpoints/ratio_disc_mnist_svhn_best_ema.pth")
    assert list(avg) == list(ratio.state_dict()) == list(torch.load("checkpoints/ratio_disc_mnist_svhn_best.pth"))
    train_ratio.save_checkpoint(ratio, args, train_ratio.checkpoint_path(args, "epoch10"), 10, 0.5)
    assert not os.path.exists("checkpoints/ratio_disc_mnist_svhn_epoch10_ema.pth")


def test_groups_are_fixed_at_construction():
    params = make_params(7)
    o = Adam([dict(params=params[:2], lr=1e-2), dict(params=params[2:])], lr=1e-3)
    assert [g["lr"] for g in o.param_groups] == [1e-2, 1e-3]
    with pytest.raises(_lib.RgfmError, match="after construction"):
        o.add_param_group(dict(params=make_params(8)))
    sched = torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5)  # (lr is read from the group at every step)
    assert o.param_groups[0]["initial_lr"] == 1e-2 and sched.get_last_lr() == [1e-2, 1e-3]
