"""CPU: keeping the best window's weights under the plateau stop rule is off by default, its setting is checked
on the host before anything touches a GPU, the NumPy restatement of rule, record and history gives the known answers on hand-written
sequences, and the exports are declared, built and bound."""
import ctypes
import os

import numpy as np
import pytest
import yaml

from splice_amd import _lib
from splice_amd.engine import DEFAULT_CFG, STOP_HISTORY, MultiPairEngine, MultiScaleEngine, best_rule, merge_pair_cfgs, np_plateau

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_option_is_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    assert DEFAULT_CFG["stop_keep_best"] is False and packaged["stop_keep_best"] is False
    assert best_rule({}) is False and best_rule(packaged) is False and best_rule(dict(stop_window=5)) is False


def test_best_rule_accepts_and_refuses():
    assert best_rule(dict(stop_keep_best=True, stop_window=5)) is True
    assert best_rule(dict(stop_keep_best=False, stop_window=0)) is False
    with pytest.raises(ValueError, match="'stop_keep_best' needs .*'stop_window' > 0"):
        best_rule(dict(stop_keep_best=True))
    for bad in (1, 0, "true", None, 1.0):
        with pytest.raises(ValueError, match="'stop_keep_best' must be true or false"):
            best_rule(dict(stop_keep_best=bad, stop_window=5))
    with pytest.raises(ValueError, match="'stop_rel'"):   # (the rule's own keys are checked on the way)
        best_rule(dict(stop_keep_best=True, stop_window=5, stop_rel=2))


def test_engines_refuse_before_the_gpu():
    with pytest.raises(ValueError, match="'stop_keep_best' needs"):
        MultiPairEngine(dict(stop_keep_best=True), None, [{}], (64, 64), device="cpu")
    with pytest.raises(ValueError, match="'stop_keep_best' must be"):
        MultiPairEngine(dict(stop_keep_best="yes", stop_window=5), None, [{}, {}], (64, 64), (64, 64), device="cpu")
    with pytest.raises(NotImplementedError, match="stop_keep_best"):
        MultiScaleEngine(dict(stop_keep_best=True, stop_window=10), None, {}, (64, 64), device="cpu")
    with pytest.raises(ValueError, match="'stop_keep_best' needs"):
        MultiScaleEngine(dict(stop_keep_best=True), None, {}, (64, 64), device="cpu")


def test_option_is_shared_by_the_slots_of_a_sweep():
    with pytest.raises(ValueError, match="'stop_keep_best' is shared"):
        merge_pair_cfgs(dict(stop_window=5), [{}, dict(stop_keep_best=True)])
    assert merge_pair_cfgs(dict(stop_window=5, stop_keep_best=True), [{}, dict(stop_keep_best=True, lr=0.1)])[1]["stop_keep_best"] is True


def _run(losses, counted=None, window=2, rel=0.1, patience=2, min_steps=0):
    return np_plateau(losses, counted or [True] * len(losses), window, rel, patience, min_steps)


def test_restatement_on_a_falling_then_flat_sequence():
    """W = 2, rel 0.1, patience 2.  Window means 3.5, 1.5, 1.45, 1.4, then 0.5: windows 0 and 1 move best (steps 1 and 3), windows
    2 and 3 do not beat 1.5 * 0.9 = 1.35, so the slot stops at step 7; the window of 0.5 closes behind the stop."""
    s = _run([4, 3, 2, 1, 1.5, 1.4, 1.4, 1.4, 0.5, 0.5, 9])
    assert (s["best_step"], s["best_window"], s["stop_step"], s["moves"]) == (3, 1, 7, 2)
    assert s["means"].dtype == np.float32 and s["means"].tobytes() == np.array([3.5, 1.5, f32(f32(1.5) + f32(1.4)) / f32(2), 1.4], dtype=f32).tobytes()
    # the state went on behind the stop: five windows closed, best moved to 0.5, one step sits in the open window
    assert (s["windows"], s["bad"], s["count"]) == (5, 0, 1) and s["best"] == f32(0.5) and s["sum"] == f32(9)
    assert s["means"][s["best_window"]] == f32(1.5) != s["best"]


def test_record_and_history_stand_still_after_a_stop_although_windows_moves():
    base = [4, 3, 2, 1, 1.5, 1.4, 1.4, 1.4]
    at_stop = _run(base)
    assert at_stop["stop_step"] == 7 and at_stop["windows"] == 4
    later = _run(base + [0.5, 0.5, 0.1, 0.1, 0.01, 0.01])
    assert later["windows"] == 7 and later["best"] == f32(0.01)
    for key in ("best_step", "best_window", "moves", "stop_step"):
        assert later[key] == at_stop[key], key
    assert later["means"].tobytes() == at_stop["means"].tobytes()


def test_the_stopping_window_itself_is_still_live():
    """min_steps holds the stop back: bad reaches patience at step 5, below min_steps, so the slot runs on; the windows behind it, one
    of them a new best, are recorded, and the slot stops where bad reaches patience again."""
    s = _run([2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1], patience=2, min_steps=9)
    # means 2 2 2 | 1 (best, step 7) | 1 (bad 1, step 9) | 1 (bad 2, step 11 >= 9: stop)
    assert (s["best_step"], s["best_window"], s["stop_step"], s["moves"]) == (7, 3, 11, 2)
    assert s["means"].tolist() == [2, 2, 2, 1, 1, 1]
    # a window that is both a new best and closes at the stop step is recorded: patience 1, the stop comes one window after it
    s = _run([2, 2, 1, 1, 1, 1], patience=1)
    assert (s["best_step"], s["best_window"], s["stop_step"]) == (3, 1, 5) and s["means"].tolist() == [2, 1, 1]


def test_uncounted_steps_and_the_first_window():
    """Steps that are not counted neither fill a window nor can they be a best step; the first window always sets best."""
    counted = [False, True, True, False, True, True, True]
    s = _run([100, 5, 7, 100, 9, 9, 1], counted, patience=5)
    assert (s["best_step"], s["best_window"], s["windows"], s["count"], s["stop_step"]) == (2, 0, 2, 1, -1)
    assert s["means"].tolist() == [6, 9]
    none = _run([1.0], window=2)
    assert (none["best_step"], none["best_window"], none["moves"]) == (-1, -1, 0) and none["means"].size == 0


def test_history_holds_the_first_windows_only():
    n = STOP_HISTORY + 6
    losses = [1.0 / (1 + k) for k in range(n)]                 # every window of one step is a new best: the slot never stops
    s = np_plateau(losses, [True] * n, 1, 0.001, 2, 0)
    assert s["stop_step"] == -1 and s["best_step"] == n - 1 and s["best_window"] == n - 1 and s["moves"] == n
    assert s["means"].size == STOP_HISTORY and s["means"].tobytes() == np.array(losses[:STOP_HISTORY], dtype=f32).tobytes()


def test_margins_are_collected():
    margins = []
    np_plateau([2, 2, 1, 1], [True] * 4, 2, 0.1, 2, 0, margins)
    assert len(margins) == 1 and abs(margins[0] - (1.8 - 1.0) / 1.8) < 1e-6


def test_best_exports_declared_bound_and_present():
    names = ("splice_plateau_update_best", "splice_optim_step_pairs_best", "splice_step_set_keep_best")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert ctypes.sizeof(_lib.BestState) == 8 and [f for f, _ in _lib.BestState._fields_] == ["best_step", "best_window"]
    assert "#define SPLICE_STOP_HISTORY 64" in hdr and STOP_HISTORY == 64 == _lib.STOP_HISTORY
