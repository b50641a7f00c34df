"""CPU: the host side of the fused optimisers -- the learning-rate schedule equals torch's scheduler objects float for float, the
refused settings are refused before any GPU work, and the new C exports are bound."""
import ctypes
import warnings

import pytest
import torch

from splice_amd import _lib
from splice_amd.util import LrSchedule, fused_optimizer, get_optimizer, get_scheduler

DEFAULT = dict(lr=0.002, optimizer_beta1=0.0, optimizer_beta2=0.99, n_epochs=10000, scheduler_n_epochs_decay=8, scheduler_lr_decay_iters=300)


def _torch_lrs(cfg, steps):
    """lr of step k = the scheduler's lr after k scheduler.step() calls (train.py:79-80), with the arguments train.py passes."""
    w = [torch.nn.Parameter(torch.zeros(1))]
    opt = get_optimizer(dict(cfg, optimizer="sgd"), w)
    sch = get_scheduler(opt, cfg["scheduler_policy"], n_epochs=cfg["n_epochs"], n_epochs_decay=cfg["scheduler_n_epochs_decay"],
                        lr_decay_iters=cfg["scheduler_lr_decay_iters"])
    out = []
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for _ in range(steps):
            out.append(opt.param_groups[0]["lr"])
            opt.step()
            sch.step()
    return out


@pytest.mark.parametrize("policy", ["none", "linear", "step", "cosine"])
def test_schedule_equals_torch_default_config(policy):
    cfg = dict(DEFAULT, scheduler_policy=policy)
    ref = _torch_lrs(cfg, cfg["n_epochs"] + 5)   # past T_max: cosine's restart branch
    sch = LrSchedule(cfg)
    got = [sch.lr(k) for k in range(len(ref))]
    bad = [k for k in range(len(ref)) if got[k] != ref[k]]
    assert not bad, (policy, bad[:5], [(got[k], ref[k]) for k in bad[:3]])


@pytest.mark.parametrize("policy", ["none", "linear", "step", "cosine"])
@pytest.mark.parametrize("n_epochs,decay,iters", [(1, 0, 1), (3, 1, 2), (7, 2, 1), (12, 5, 4)])
def test_schedule_equals_torch_small_values(policy, n_epochs, decay, iters):
    cfg = dict(DEFAULT, lr=0.01, scheduler_policy=policy, n_epochs=n_epochs, scheduler_n_epochs_decay=decay, scheduler_lr_decay_iters=iters)
    ref = _torch_lrs(cfg, 4 * n_epochs + 6)
    sch = LrSchedule(cfg)
    assert [sch.lr(k) for k in range(len(ref))] == ref
    # random access (the recurrence restarts when asked for an earlier step)
    assert sch.lr(2) == ref[2] and sch.lr(len(ref) - 1) == ref[-1]


def test_schedule_values_move():
    """The schedules are not the constant: a check that the comparisons above compare something."""
    for policy in ("linear", "step", "cosine"):
        cfg = dict(DEFAULT, scheduler_policy=policy, n_epochs=10, scheduler_n_epochs_decay=3, scheduler_lr_decay_iters=2)
        lrs = [LrSchedule(cfg).lr(k) for k in range(8)]
        assert lrs[0] == 0.002 and len(set(lrs)) > 2, (policy, lrs)


def test_plateau_and_unknown_names_refused():
    with pytest.raises(NotImplementedError, match="no metric"):
        LrSchedule(dict(DEFAULT, scheduler_policy="plateau"))
    with pytest.raises(NotImplementedError):
        LrSchedule(dict(DEFAULT, scheduler_policy="warmup"))
    with pytest.raises(NotImplementedError):
        fused_optimizer(dict(DEFAULT, optimizer="lion"))
    assert fused_optimizer(dict(DEFAULT, optimizer="adam")) == (0, 0.0, 0.99, 1e-8)
    assert fused_optimizer(dict(DEFAULT, optimizer="rmsprop"))[:2] == (1, 0.99)
    assert fused_optimizer(dict(DEFAULT, optimizer="sgd"))[0] == 2


def test_engine_refuses_plateau_before_touching_the_gpu():
    """The engine checks the optimiser settings first: the refusal needs no GPU and names the reason."""
    from splice_amd.engine import MultiPairEngine
    with pytest.raises(NotImplementedError, match="plateau"):
        MultiPairEngine(dict(scheduler_policy="plateau"), None, [{}], (64, 64), device="cpu")
    with pytest.raises(NotImplementedError, match="adagrad"):
        MultiPairEngine(dict(optimizer="adagrad"), None, [{}], (64, 64), device="cpu")


def test_optimiser_exports_bound_and_present():
    names = ("splice_optim_step", "splice_optim_step_ex", "splice_step_set_optimizer", "splice_step_set_lr")
    assert set(names) <= set(_lib.exported_symbols())
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
