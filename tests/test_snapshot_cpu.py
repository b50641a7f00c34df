"""CPU: pair snapshots.  The three keys are off by default and checked on the host, ``restore`` refuses what does
not fit by name before anything touches a GPU, ``MultiScaleEngine`` refuses the feature, a retried batch item resumes, the checkpoint
file round-trips, and the exports are declared, built and bound."""
import ctypes
import os
import random

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, PAIR_KEYS, SNAPSHOT_FREE_KEYS, MultiPairEngine, MultiScaleEngine, checkpoint_rule, compact_rule, merge_pair_cfgs,
                               snapshot_cfg_mismatch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------------------------ the keys
def test_the_keys_are_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    for cfg in (DEFAULT_CFG, packaged):
        assert cfg["stop_compact"] is False and cfg["resume"] is False and cfg["checkpoint_every"] == 0 and isinstance(cfg["checkpoint_every"], int)
        assert compact_rule(cfg) is False and checkpoint_rule(cfg) == (0, False)
    assert compact_rule({}) is False and checkpoint_rule({}) == (0, False)
    assert compact_rule(dict(stop_compact=True, stop_window=4)) is True and checkpoint_rule(dict(checkpoint_every=5, resume=True)) == (5, True)
    assert not set(PAIR_KEYS) & {"stop_compact", "checkpoint_every", "resume"}


@pytest.mark.parametrize("key,bad", [("stop_compact", v) for v in (1, 0, "true", None, 1.0)] + [("resume", v) for v in (1, "yes", None)] +
                         [("checkpoint_every", v) for v in (-1, 1.5, "4", None, True)])
def test_bad_values_are_refused_on_the_host(key, bad):
    rule = compact_rule if key == "stop_compact" else checkpoint_rule
    with pytest.raises(ValueError, match=f"'{key}' must be"):
        rule({key: bad, "stop_window": 3})
    if key == "stop_compact":   # (no device is touched: the engine gets no further than the host checks)
        with pytest.raises(ValueError, match="'stop_compact' must be"):
            MultiPairEngine({key: bad, "stop_window": 3}, None, [{}] * 2, (64, 64), device="cpu")


def test_stop_compact_needs_the_stop_rule():
    for cfg in (dict(stop_compact=True), dict(stop_compact=True, stop_window=0)):
        with pytest.raises(ValueError, match="'stop_compact'.*'stop_window' > 0"):
            compact_rule(cfg)
        for slots in (1, 3):
            with pytest.raises(ValueError, match="'stop_compact'.*'stop_window' > 0"):
                MultiPairEngine(cfg, None, [{}] * slots, (64, 64), device="cpu")
    # the key passes its check; the next host check (the crop counts) is the one that refuses: nothing has touched a GPU
    with pytest.raises(ValueError, match="n_crops"):
        MultiPairEngine(dict(stop_compact=True, stop_window=3), None, [{}] * 2, (64, 64), (64, 64), device="cpu", n_crops=(9, 1))


def test_stop_compact_is_shared_by_the_slots_of_a_sweep():
    with pytest.raises(ValueError, match="'stop_compact' is shared"):
        merge_pair_cfgs(dict(stop_window=3), [{}, dict(stop_compact=True)])
    assert merge_pair_cfgs(dict(stop_window=3, stop_compact=True), [{}, dict(lr=0.1)])[1]["stop_compact"] is True


def test_multiscale_engine_refuses_all_three():
    with pytest.raises(NotImplementedError, match="stop_compact.*MultiScaleEngine"):
        MultiScaleEngine(dict(stop_compact=True, stop_window=3), None, {}, (64, 64), device="cpu")
    eng = MultiScaleEngine.__new__(MultiScaleEngine)     # (the refusals need no built engine)
    with pytest.raises(NotImplementedError, match="snapshot.*MultiScaleEngine"):
        eng.snapshot(0)
    with pytest.raises(NotImplementedError, match="restore.*MultiScaleEngine"):
        eng.restore([{}])


# ------------------------------------------------------------------------------------------------------------------ restore
class Fresh(MultiPairEngine):
    """The host side of a fresh engine of ``slots`` slots with every rule on: ``restore`` runs the product's own checks and raises
    before it would touch a tensor."""

    def __init__(self, slots, cfg=None, step_idx=-1):
        self.cfg = dict(DEFAULT_CFG, stop_window=3, **(cfg or {}))
        self.cfgs, self.P, self.P_in, self.live, self._parked = [self.cfg] * slots, slots, slots, list(range(slots)), {}
        self.step_idx, self.stop_rule, self.handle = step_idx, (3, 0.01, 2, 0), None
        self.n_crops_ab, self.crop_hw, self.entire_hw, self.plan_e = (1, 1), (64, 64), (64, 64), object()
        self.ema = self.best = self.best_ema = self.clip_dev = self.lr_state_dev = self.trace_dev = torch.zeros(1)   # (kept: the states must carry them)

    @property
    def gen(self):
        raise AssertionError("restore touched an arena before its host checks passed")


def _state(step_idx=4, **cfg):
    t = torch.zeros(1)
    return dict(format=1, step_idx=step_idx, cfg=dict(DEFAULT_CFG, stop_window=3, **cfg), n_crops=(1, 1), crop_hw=(64, 64), entire_hw=(64, 64), generator_calls=0,
                params=t, m=t, v=t, running=t, losses=t, ema=t, best=t, best_ema=t, best_rec=t, means=t, clip=t, lr_state=t, lr_cuts=t, trace=t,
                stop=(0.0, 0, 0, 0.0, 0, -1))


def test_restore_refuses_by_name_before_the_gpu():
    with pytest.raises(ValueError, match="another 'lr'"):
        Fresh(2).restore([_state(), _state(lr=0.5)])
    with pytest.raises(ValueError, match="another 'n_epochs'"):
        Fresh(1).restore([_state(n_epochs=7)])
    with pytest.raises(ValueError, match="another 'ema_decay'"):
        Fresh(1, dict(ema_decay=0.5)).restore([_state()])
    with pytest.raises(ValueError, match="disagree on 'step_idx'"):
        Fresh(2).restore([_state(4), _state(5)])
    with pytest.raises(ValueError, match="3 states for 2 slots"):
        Fresh(2).restore([_state()] * 3)
    with pytest.raises(ValueError, match="1 states for 2 slots"):
        Fresh(2).restore([_state()])
    with pytest.raises(ValueError, match="already stepped"):
        Fresh(2, step_idx=0).restore([_state(), _state()])
    with pytest.raises(ValueError, match="'format'"):
        Fresh(1).restore([dict(_state(), format=2)])
    with pytest.raises(ValueError, match="'crop_hw'"):
        Fresh(1).restore([dict(_state(), crop_hw=(72, 72))])
    with pytest.raises(ValueError, match="lacks 'trace'"):
        Fresh(1).restore([{k: v for k, v in _state().items() if k != "trace"}])
    with pytest.raises(AssertionError, match="touched an arena"):     # a state that fits gets past the checks (and the stub has no arenas)
        Fresh(2).restore([_state(), _state()])


def test_paths_and_logging_keys_do_not_bind_a_state():
    a = dict(DEFAULT_CFG, dataroot="/one", log_images_freq=3, stop_compact=True, checkpoint_every=4, resume=True)
    b = dict(DEFAULT_CFG, dataroot="/two", log_images_freq=10)
    assert snapshot_cfg_mismatch(a, b) is None and set(SNAPSHOT_FREE_KEYS) == {"dataroot", "log_images_freq", "stop_compact", "checkpoint_every", "resume"}
    assert snapshot_cfg_mismatch(dict(a, seed=1), dict(b, seed=2)) == "seed" and snapshot_cfg_mismatch(dict(a, cls_warmup=2), b) == "cls_warmup"
    assert snapshot_cfg_mismatch({"lr": 0.002}, dict(DEFAULT_CFG)) is None      # an absent key stands for its default
    Fresh(1, dict(dataroot="/elsewhere", log_images_freq=7))._check_states([_state()])


# ----------------------------------------------------------------------------------------------------------- the checkpoint
class Snapshots:
    """An engine as the loop's checkpoint code sees it: ``snapshot`` and ``restore``."""

    def __init__(self, slots):
        self.P_in, self.restored = slots, None

    def snapshot(self, pair, device=None):
        assert device == "cpu"
        return dict(format=1, step_idx=7, params=torch.full((3,), float(pair)))

    def restore(self, states):
        self.restored = states


class Feed:
    step = 7


def test_the_checkpoint_file_round_trips_and_is_replaced_atomically(tmp_path):
    from splice_amd.train import CHECKPOINT_NAME, load_checkpoint, save_checkpoint
    path = str(tmp_path / CHECKPOINT_NAME)
    random.seed(5)
    np.random.seed(5)
    torch.manual_seed(5)
    save_checkpoint(path, Snapshots(2), Feed(), 8)
    assert os.listdir(tmp_path) == [CHECKPOINT_NAME]                       # no temporary file stays behind
    want = (random.random(), np.random.rand(), torch.rand(1).item())
    random.seed(6), np.random.seed(6), torch.manual_seed(6)
    eng, feed = Snapshots(2), Feed()
    feed.step = -1
    assert load_checkpoint(path, eng, feed) == 8 and feed.step == 7
    assert [s["params"].tolist() for s in eng.restored] == [[0.0] * 3, [1.0] * 3]
    assert (random.random(), np.random.rand(), torch.rand(1).item()) == want  # the generators go on where the checkpoint left them
    torch.save({"format": 2}, path)
    with pytest.raises(ValueError, match="format 1"):
        load_checkpoint(path, eng, feed)


def test_a_retried_batch_item_resumes_where_checkpoints_are_written():
    from splice_amd.batch import retry_resumes
    assert retry_resumes(dict(checkpoint_every=50)) and not retry_resumes({}) and not retry_resumes(dict(checkpoint_every=0)) and not retry_resumes(None)
    assert not retry_resumes(dict(checkpoint_every=True))


# --------------------------------------------------------------------------------------------------------------- the exports
def test_exports_declared_bound_and_present():
    names = ("splice_step_restore", "splice_step_set_input_rows")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["splice_step_restore"][0]) == 4 and len(_lib._SIGNATURES["splice_step_set_input_rows"][0]) == 3
    assert len(_lib._SIGNATURES["splice_step_run"][0]) == 11 and len(_lib._SIGNATURES["splice_step_stop_state"][0]) == 3   # (as they were)
