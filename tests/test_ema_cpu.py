"""CPU: the weight average is off by default, its settings are checked on the host before anything touches a GPU, and its exports are
declared, built and bound."""
import ctypes
import os

import numpy as np
import pytest
import yaml

from splice_amd import _lib
from splice_amd.engine import DEFAULT_CFG, PAIR_KEYS, MultiPairEngine, MultiScaleEngine, ema_rule, merge_pair_cfgs, np_ema

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_average_is_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    for key, val in dict(ema_decay=0.0, ema_start=0).items():
        assert DEFAULT_CFG[key] == val and packaged[key] == val, key
    assert ema_rule({}) == (0.0, 0) and ema_rule(packaged) == (0.0, 0)


def test_ema_rule_accepts():
    assert ema_rule(dict(ema_decay=0.999, ema_start=100)) == (0.999, 100)
    assert ema_rule(dict(ema_decay=0)) == (0.0, 0)
    assert ema_rule(dict(ema_decay=np.float32(0.5), ema_start=np.int64(3))) == (0.5, 3)


@pytest.mark.parametrize("key,value", [("ema_decay", True), ("ema_decay", 1.0), ("ema_decay", 1), ("ema_decay", -0.1), ("ema_decay", "0.9"), ("ema_decay", float("nan")),
                                       ("ema_start", 2.0), ("ema_start", -1), ("ema_start", True), ("ema_start", "3")])
def test_bad_values_refused_by_key_before_the_gpu(key, value):
    with pytest.raises(ValueError, match=f"'{key}'"):
        ema_rule({key: value})
    with pytest.raises(ValueError, match=f"'{key}'"):
        MultiPairEngine({key: value}, None, [{}], (64, 64), device="cpu")
    with pytest.raises(ValueError, match=f"'{key}'"):   # checked whether or not the average is on
        MultiPairEngine({"ema_decay": 0.9, key: value}, None, [{}, {}], (64, 64), (64, 64), device="cpu")
    with pytest.raises(ValueError, match=f"'{key}'"):
        MultiScaleEngine({key: value}, None, {}, (64, 64), device="cpu")


@pytest.mark.parametrize("key,value", [("ema_decay", 0.99), ("ema_start", 10)])
def test_ema_keys_are_shared_by_the_slots_of_a_sweep(key, value):
    assert key not in PAIR_KEYS
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs({}, [{}, {key: value}])
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        MultiPairEngine({}, None, [{}, {}], (64, 64), (64, 64), device="cpu", pair_cfgs=[{}, {key: value}])
    assert merge_pair_cfgs({key: value}, [{}, {key: value, "lr": 0.1}])[1][key] == value   # the base value is accepted


def test_ema_exports_declared_bound_and_present():
    names = ("splice_optim_step_ema", "splice_step_set_ema", "splice_optim_step_pairs_ema")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["splice_optim_step_ema"][0]) == 18 and len(_lib._SIGNATURES["splice_step_set_ema"][0]) == 4
    assert len(_lib._SIGNATURES["splice_optim_step_pairs_ema"][0]) == 20


def test_numpy_restatement_by_hand():
    """0.9 and 0.1 are not fp32 numbers: the rule multiplies by float32(0.9) and by float32(1) - float32(0.9), each product and the sum
    rounded to fp32."""
    f = np.float32
    e, p = np.array([1.0, 3.0], dtype=f), np.array([2.0, -1.0], dtype=f)
    assert np_ema(e, p, 2, 0.9, 2).tobytes() == p.tobytes()          # step <= start: the average copies the weights
    got = np_ema(e, p, 3, 0.9, 2)
    d = f(0.9)
    want = np.array([f(f(d * e[k]) + f(f(f(1) - d) * p[k])) for k in range(2)], dtype=f)
    assert got.dtype == f and got.tobytes() == want.tobytes()
    assert f(1) - d != f(0.1)                                        # (what makes "1 - d" part of the rule)
