"""CPU: the plateau stop rule is off by default, its settings are checked on the host before anything touches a GPU, and its
exports are declared, built and bound."""
import ctypes
import os

import pytest
import yaml

from splice_amd import _lib
from splice_amd.engine import DEFAULT_CFG, MultiPairEngine, MultiScaleEngine, merge_pair_cfgs, stop_rule, stop_window_closes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULTS = dict(stop_window=0, stop_rel=0.01, stop_patience=2, stop_min_steps=0)


def test_rule_is_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    for key, val in DEFAULTS.items():
        assert DEFAULT_CFG[key] == val and packaged[key] == val, key
    assert stop_rule({}) == (0, 0.01, 2, 0) and stop_rule(packaged)[0] == 0
    assert not any(stop_window_closes(k, 0, 1, 5) for k in range(50))


def test_window_closes_matches_a_hand_count():
    """cls_warmup = 1, entire_A_every = 5, W = 3: step 0 is warm-up (and an entire-image step), 5 10 15 are entire-image steps; the
    counted steps are 1 2 3 | 4 6 7 | 8 9 11 | 12 13 14 | 16 17 18."""
    closes = [k for k in range(20) if stop_window_closes(k, 3, 1, 5)]
    assert closes == [3, 7, 11, 14, 18]
    # without the entire-image branch every step from the warm-up on counts: 1 2 3 | 4 5 6 | ...
    assert [k for k in range(11) if stop_window_closes(k, 3, 1, 0)] == [3, 6, 9]
    assert [k for k in range(7) if stop_window_closes(k, 2, 0, 0)] == [1, 3, 5]


@pytest.mark.parametrize("key,value", [("stop_window", -1), ("stop_window", 2.5), ("stop_rel", 0), ("stop_rel", 1), ("stop_rel", -0.1), ("stop_rel", "x"),
                                       ("stop_patience", 0), ("stop_min_steps", -3)])
def test_bad_values_refused_by_key_before_the_gpu(key, value):
    with pytest.raises(ValueError, match=f"'{key}'"):
        MultiPairEngine({key: value}, None, [{}], (64, 64), device="cpu")
    with pytest.raises(ValueError, match=f"'{key}'"):   # checked whether or not the rule is on
        MultiPairEngine({"stop_window": 5, key: value}, None, [{}, {}], (64, 64), (64, 64), device="cpu")


def test_multiscale_engine_refuses_the_rule():
    with pytest.raises(NotImplementedError, match="stop_window"):
        MultiScaleEngine(dict(stop_window=10), None, {}, (64, 64), device="cpu")
    with pytest.raises(ValueError, match="'stop_rel'"):
        MultiScaleEngine(dict(stop_window=10, stop_rel=2), None, {}, (64, 64), device="cpu")


@pytest.mark.parametrize("key,value", [("stop_window", 25), ("stop_rel", 0.05), ("stop_patience", 3), ("stop_min_steps", 100)])
def test_stop_keys_are_shared_by_the_slots_of_a_sweep(key, value):
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs({}, [{}, {key: value}])
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        MultiPairEngine({}, None, [{}, {}], (64, 64), (64, 64), device="cpu", pair_cfgs=[{}, {key: value}])
    assert merge_pair_cfgs({key: value}, [{}, {key: value, "lr": 0.1}])[1][key] == value   # the base value is accepted


def test_stop_exports_declared_bound_and_present():
    names = ("splice_step_set_stop_rule", "splice_step_stop_state", "splice_plateau_update")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert ctypes.sizeof(_lib.StopState) == 24 and [f for f, _ in _lib.StopState._fields_] == ["sum", "count", "windows", "best", "bad", "stop_step"]
