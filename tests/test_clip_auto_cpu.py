"""CPU: clipping of every pair's gradient against its own running norm.  The three keys are off by default and
checked on the host, they are shared by the slots of a sweep, the NumPy restatement of the rule (engine.np_clip_auto) has the
properties the rule is built for, ``restore`` refuses a snapshot taken under another rule by the key's name, and the exports are
declared, built and bound."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, PAIR_KEYS, MultiPairEngine, MultiScaleEngine, clip_regime, grad_clip_auto_rule, merge_pair_cfgs, np_clip_auto,
                               snapshot_cfg_mismatch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
KEYS = ("grad_clip_auto", "grad_clip_auto_beta", "grad_clip_auto_warmup")


# ------------------------------------------------------------------------------------------------------------------ the keys
def test_the_keys_are_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    for cfg in (DEFAULT_CFG, packaged, {}):
        assert grad_clip_auto_rule(cfg) == (0.0, 0.98, 8)
    for cfg in (DEFAULT_CFG, packaged):
        assert cfg["grad_clip_auto"] == 0.0 and cfg["grad_clip_auto_beta"] == 0.98 and cfg["grad_clip_auto_warmup"] == 8
    assert grad_clip_auto_rule(dict(grad_clip_auto=2, grad_clip_auto_beta=0, grad_clip_auto_warmup=1)) == (2.0, 0.0, 1)
    assert grad_clip_auto_rule(dict(grad_clip_auto=np.float32(1.5), grad_clip_auto_warmup=np.int64(3))) == (1.5, 0.98, 3)
    assert grad_clip_auto_rule(dict(grad_clip_auto=1)) == (1.0, 0.98, 8) and grad_clip_auto_rule(dict(grad_clip_auto=1e30))[0] == 1e30


BAD = [("grad_clip_auto", v) for v in (0.5, 0.999, 1e-9, -1.0, -2, float("nan"), float("inf"), 1e39, "2", None, True)] + \
      [("grad_clip_auto_beta", v) for v in (-0.1, 1.0, 1.5, float("nan"), 0.99999999, "0.9", None, True)] + \
      [("grad_clip_auto_warmup", v) for v in (0, -1, 1.5, 8.0, "8", None, True)]


@pytest.mark.parametrize("key,value", BAD)
def test_bad_values_are_refused_on_the_host(key, value):
    """k in (0, 1), a non-finite k (1e39 is no finite float32), beta outside [0, 1) -- 0.99999999 rounds to 1.0f --, warmup < 1, and
    what is no number: refused by the key's name before an engine touches a device."""
    cfg = {"grad_clip_auto": 2.0, key: value}
    with pytest.raises(ValueError, match=f"'{key}'"):
        grad_clip_auto_rule(cfg)
    with pytest.raises(ValueError, match=f"'{key}'"):
        MultiPairEngine(cfg, None, [{}], (64, 64), device="cpu")
    with pytest.raises(ValueError, match=f"'{key}'"):
        MultiPairEngine(cfg, None, [{}, {}], (64, 64), (64, 64), device="cpu")
    with pytest.raises(ValueError, match=f"'{key}'"):
        MultiScaleEngine(cfg, None, {}, (64, 64), device="cpu")


def test_the_keys_are_shared_by_the_slots_of_a_sweep():
    for key, value in zip(KEYS, (2.0, 0.9, 4)):
        assert key not in PAIR_KEYS
        with pytest.raises(ValueError, match=f"'{key}' is shared by every slot of a sweep"):
            merge_pair_cfgs({}, [{}, {key: value}])
        with pytest.raises(ValueError, match=f"'{key}' is shared by every slot of a sweep"):
            MultiPairEngine({}, None, [{}, {}], (64, 64), (64, 64), device="cpu", pair_cfgs=[{}, {key: value}])
        assert merge_pair_cfgs({key: value}, [{}, {key: value, "lr": 0.1}])[1][key] == value   # the base value is accepted


def test_the_regime_of_a_step():
    assert [clip_regime(s, 2, s % 3 == 0) for s in range(7)] == [-1, -1, 0, 1, 0, 0, 1]
    assert clip_regime(0, 0, True) == 1 and clip_regime(0, 0, False) == 0 and clip_regime(0, 1, True) == -1


# -------------------------------------------------------------------------------------------------------- the restatement
def _run(norms, regimes, k, beta, warmup, max_norm=0.0):
    state, out = None, []
    for norm, r in zip(norms, regimes):
        new, coef, skip = np_clip_auto(state, F(norm), r, k, beta, warmup, max_norm)
        out.append(dict(before=state, after=new, coef=coef, skip=skip))
        state = new
    return out


def test_the_first_step_of_a_regime_sets_its_reference_and_warmup_holds_the_threshold_back():
    run = _run([4.0, 9.0, 2.0, 100.0, 100.0], [0, 1, 0, 0, 0], 2.0, 0.5, 3)
    assert run[0]["after"] == dict(ref=[F(4), F(0)], count=[1, 0], thr=F(np.inf), regime=0)
    assert run[1]["after"] == dict(ref=[F(4), F(9)], count=[1, 1], thr=F(np.inf), regime=1)
    assert run[2]["after"]["ref"] == [F(3), F(9)] and run[2]["after"]["count"] == [2, 1]
    # the third observation of regime 0 is still inside the warm-up: a spike passes and enters the reference whole
    assert run[3]["coef"] == 1 and run[3]["after"]["ref"][0] == F(51.5) and run[3]["after"]["thr"] == np.inf
    # the fourth is judged: thr = 2 * 51.5, x = min(100, 103)
    assert run[4]["after"]["thr"] == F(103) and run[4]["coef"] == 1 and run[4]["after"]["ref"][0] == F(75.75)
    assert all(type(x) is np.float32 for r in run for x in r["after"]["ref"] + [r["after"]["thr"], r["coef"]])


def test_a_k_whose_product_overflows_never_clips():
    rng = np.random.default_rng(3)
    norms = np.concatenate([[F(3e38), F(1e38)], rng.lognormal(0, 3, 60).astype(F) * F(1e30)]).astype(F)
    run = _run(norms, [s % 2 for s in range(len(norms))], 3e38, 0.5, 1)
    assert all(r["coef"] == 1 and r["skip"] == 0 for r in run)
    assert any(r["after"]["thr"] == np.inf and r["before"] is not None and r["before"]["count"][r["after"]["regime"]] >= 1 for r in run)   # k * ref = inf
    assert all(np.isfinite(x) for r in run for x in r["after"]["ref"])


def test_a_non_finite_norm_moves_neither_reference_nor_count():
    for bad in (np.nan, np.inf):
        for regime in (0, 1, -1):
            run = _run([1.0, 2.0, 1.0, 2.0, bad], [0, 1, 0, 1, regime], 2.0, 0.9, 1, max_norm=5.0)
            before, after = run[-1]["before"], run[-1]["after"]
            assert run[-1]["skip"] == 1 and run[-1]["coef"] == 0
            assert after["ref"] == before["ref"] and after["count"] == before["count"] and after["regime"] == regime
            want = F(5.0) if regime < 0 else np.minimum(F(5.0), F(2.0) * before["ref"][regime])
            assert after["thr"].tobytes() == F(want).tobytes()


def test_regime_minus_one_touches_nothing_but_the_last_threshold_and_the_guard():
    warm = _run([1.0, 2.0, 1.0, 2.0], [0, 1, 0, 1], 2.0, 0.9, 1)[-1]["after"]
    for max_norm, norm, coef in ((0.0, 50.0, F(1)), (5.0, 50.0, F(5.0) / (F(50.0) + F(1e-6))), (5.0, 1.0, F(1))):
        new, c, skip = np_clip_auto(warm, F(norm), -1, 2.0, 0.9, 1, max_norm)
        assert new["ref"] == warm["ref"] and new["count"] == warm["count"] and new["regime"] == -1 and skip == 0
        assert new["thr"] == (F(max_norm) if max_norm else np.inf) and c.tobytes() == F(coef).tobytes()
    new, c, skip = np_clip_auto(None, F(np.nan), -1, 2.0, 0.9, 1, 0.0)
    assert (new["ref"], new["count"], skip, c) == ([F(0), F(0)], [0, 0], 1, 0)
    assert np_clip_auto(warm, F(1.0), 0, 2.0, 0.9, 1, 0.0)[0] != warm and warm["count"] == [2, 2]   # (the state passed in is not written)


@pytest.mark.parametrize("k,beta", [(2.0, 0.9), (1.0, 0.0), (1.05, 0.5), (10.0, 0.98)])
def test_one_spike_raises_the_reference_by_at_most_the_factor_k(k, beta):
    rng = np.random.default_rng(11)
    norms = rng.lognormal(0, 0.1, 30).astype(F)
    state = _run(norms, [0] * 30, k, beta, 4)[-1]["after"]
    ref = state["ref"][0]
    for spike in (30.0, 1e3, 1e30, 3e38):                     # (the norms are about 1: each is beyond k times the reference)
        new, coef, skip = np_clip_auto(state, F(spike), 0, k, beta, 4, 0.0)
        bound = F(F(beta) * ref) + F(F(F(1) - F(beta)) * F(F(k) * ref))
        assert skip == 0 and coef < 1 and new["thr"] == F(k) * ref and ref <= new["ref"][0] <= bound, (spike, new["ref"][0], bound)
        assert (new["ref"][0] > ref) == (k > 1)               # (k = 1: the capped observation is the reference itself)
        assert new["ref"][1] == 0 and new["count"] == [31, 0]


def test_a_designed_run_clips_the_spike_behind_the_warmup_and_passes_the_one_inside_it():
    """200 norms falling from 1.0 to 0.5 with 10 % jitter, every 25th step an entire-image step at three times the level, spikes x 10
    at steps 50 (an entire-image step inside its regime's warm-up of 10) and 120, a NaN at step 80; k = 2, beta = 0.9."""
    rng = np.random.default_rng(2)
    steps = np.arange(200)
    regimes = [1 if s % 25 == 0 else 0 for s in steps]
    norms = (np.linspace(1.0, 0.5, 200) * rng.lognormal(0, 0.1, 200) * np.where(np.array(regimes) == 1, 3.0, 1.0)).astype(F)
    norms[50] *= F(10)
    norms[120] *= F(10)
    norms[80] = np.nan
    run = _run(norms, regimes, 2.0, 0.9, 10)
    assert [s for s in steps if run[s]["coef"] < 1 and not run[s]["skip"]] == [120]
    assert [s for s in steps if run[s]["skip"]] == [80] and run[80]["after"]["ref"] == run[80]["before"]["ref"]
    assert run[50]["coef"] == 1 and run[50]["after"]["thr"] == np.inf and run[50]["before"]["count"][1] == 2
    ref = run[-1]["after"]["ref"]
    assert 0.45 < ref[0] < 0.65 and run[-1]["after"]["count"] == [191, 8]
    # a tight rule on the same norms clips often: the threshold follows the norm down
    tight = _run(norms, regimes, 1.05, 0.5, 2)
    assert 40 <= sum(r["coef"] < 1 and not r["skip"] for r in tight) <= 110


# ------------------------------------------------------------------------------------------------------------------ restore
class Fresh(MultiPairEngine):   # (tests/test_snapshot_cpu.py::Fresh, with the records of both clipping rules)
    """The host side of a fresh engine: ``restore`` runs the product's own checks and raises before it would touch a tensor."""

    def __init__(self, slots, cfg=None, auto=True):
        self.cfg = dict(DEFAULT_CFG, **(cfg or {}))
        self.cfgs, self.P, self.P_in, self.live, self._parked = [self.cfg] * slots, slots, slots, list(range(slots)), {}
        self.step_idx, self.stop_rule, self.handle = -1, (0, 0.01, 2, 0), None
        self.n_crops_ab, self.crop_hw, self.entire_hw, self.plan_e = (1, 1), (64, 64), (64, 64), object()
        self.ema = self.best = self.best_ema = self.lr_state_dev = self.trace_dev = None
        self.clip_dev = torch.zeros(1)
        self.clip_auto_dev = torch.zeros(1) if auto else None

    @property
    def gen(self):
        raise AssertionError("restore touched an arena before its host checks passed")


def _state(auto=True, **cfg):
    t = torch.zeros(1)
    s = dict(format=1, step_idx=4, cfg=dict(DEFAULT_CFG, **cfg), n_crops=(1, 1), crop_hw=(64, 64), entire_hw=(64, 64), generator_calls=0,
             params=t, m=t, v=t, running=t, losses=t, clip=t)
    return dict(s, clip_auto=t) if auto else s


def test_restore_refuses_a_snapshot_taken_under_another_rule_by_the_keys_name():
    on = dict(grad_clip_auto=2.0)
    with pytest.raises(ValueError, match="another 'grad_clip_auto' \\(3.0, the slot has 2.0\\)"):
        Fresh(1, on).restore([_state(grad_clip_auto=3.0)])
    with pytest.raises(ValueError, match="another 'grad_clip_auto' "):
        Fresh(1, on).restore([_state(auto=False, grad_clip_norm=1.0)])          # (taken with the fixed rule alone)
    with pytest.raises(ValueError, match="another 'grad_clip_auto_beta'"):
        Fresh(1, on).restore([_state(grad_clip_auto=2.0, grad_clip_auto_beta=0.5)])
    with pytest.raises(ValueError, match="another 'grad_clip_auto_warmup'"):
        Fresh(2, on).restore([_state(grad_clip_auto=2.0), _state(grad_clip_auto=2.0, grad_clip_auto_warmup=2)])
    with pytest.raises(ValueError, match="lacks 'clip_auto'"):
        Fresh(1, on).restore([_state(auto=False, grad_clip_auto=2.0)])
    with pytest.raises(ValueError, match="carries 'clip_auto'"):
        Fresh(1, dict(grad_clip_norm=1.0), auto=False).restore([_state(grad_clip_norm=1.0)])
    with pytest.raises(AssertionError, match="touched an arena"):                # a state that fits gets past the checks
        Fresh(1, on).restore([_state(grad_clip_auto=2.0)])
    with pytest.raises(AssertionError, match="touched an arena"):                # ... and with the key off a state has today's keys
        Fresh(1, dict(grad_clip_norm=1.0), auto=False).restore([_state(auto=False, grad_clip_norm=1.0)])
    assert snapshot_cfg_mismatch(dict(DEFAULT_CFG), {k: v for k, v in DEFAULT_CFG.items() if k not in KEYS}) is None   # an older snapshot's config


# ------------------------------------------------------------------------------------------------------- result.json fields
class Ran:
    """An engine as ``train.clip_fields`` sees it."""
    grad_clip, step_idx, clip_dev = 0.5, 3, object()

    def __init__(self, auto):
        self.clip_auto, self.clip_auto_dev = (2.0 if auto else 0.0, 0.98, 8), (object() if auto else None)

    def clip_state(self, slot=None):
        return dict(clipped=2, skipped=1)

    def clip_auto_state(self, slot=None):
        return dict(ref=[F(0.25), F(1.5)], count=[3, 1], thr=F(0.5), regime=0)


def test_result_fields_are_todays_with_the_key_off():
    import json
    from splice_amd.train import clip_fields
    assert clip_fields(Ran(False)) == dict(grad_clip_norm=0.5, clipped_steps=2, skipped_steps=1)
    on = clip_fields(Ran(True))
    assert on == dict(grad_clip_norm=0.5, clipped_steps=2, skipped_steps=1, grad_clip_auto=2.0, clip_ref=[0.25, 1.5])
    assert json.loads(json.dumps(on)) == on
    fresh = Ran(True)
    fresh.step_idx = -1
    assert clip_fields(fresh) == dict(grad_clip_norm=0.5, clipped_steps=0, skipped_steps=0, grad_clip_auto=2.0, clip_ref=[0.0, 0.0])


# --------------------------------------------------------------------------------------------------------------- the exports
def test_exports_declared_bound_and_present():
    names = ("splice_grad_norm_pairs_auto", "splice_step_set_grad_clip_auto")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["splice_grad_norm_pairs_auto"][0]) == 16 and len(_lib._SIGNATURES["splice_step_set_grad_clip_auto"][0]) == 7
    assert len(_lib._SIGNATURES["splice_grad_norm_pairs"][0]) == 11 and len(_lib._SIGNATURES["splice_step_set_grad_clip"][0]) == 3   # (as they were)


def test_the_record_is_24_bytes_laid_out_as_the_header_says(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "splice_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(splice_clip_auto_state), offsetof(splice_clip_auto_state, ref), offsetof(splice_clip_auto_state, count),\n'
                   '           offsetof(splice_clip_auto_state, thr), offsetof(splice_clip_auto_state, regime), sizeof(splice_clip_state));\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    m = _lib.ClipAutoState
    assert out == [24, 0, 8, 16, 20, 24]
    assert [ctypes.sizeof(m), m.ref.offset, m.count.offset, m.thr.offset, m.regime.offset, ctypes.sizeof(_lib.ClipState)] == out
