"""CPU: the plateau lr rule is off by default, its settings are checked on the host before anything touches a GPU,
its NumPy restatement leaves the stop rule's state alone and cuts where torch's ReduceLROnPlateau cuts, the floor and the cap of 64 cuts
hold, the end of a run writes the effective lr and the result fields, and the exports are declared, built and bound."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, PAIR_KEYS, STOP_HISTORY, MultiPairEngine, MultiScaleEngine, lr_plateau_rule, merge_pair_cfgs,
                               np_lr_plateau, np_plateau, replay_lr_scales)
from splice_amd.train import _optimise, lr_fields

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ON = dict(stop_window=5, lr_plateau_factor=0.5)
STOP_FIELDS = ("sum", "count", "windows", "best", "bad", "stop_step")


# ------------------------------------------------------------------------------------------------------------------ the keys
def test_the_rule_is_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    for cfg in (DEFAULT_CFG, packaged):
        assert (cfg["lr_plateau_factor"], cfg["lr_plateau_patience"], cfg["lr_plateau_min_scale"]) == (0.0, 1, 0.0)
        assert isinstance(cfg["lr_plateau_patience"], int)
    assert lr_plateau_rule({}) == (0.0, 1, 0.0) and lr_plateau_rule(packaged) == (0.0, 1, 0.0)
    assert lr_plateau_rule(dict(ON, lr_plateau_patience=3, lr_plateau_min_scale=0.25)) == (0.5, 3, 0.25)
    assert not set(PAIR_KEYS) & {"lr_plateau_factor", "lr_plateau_patience", "lr_plateau_min_scale"}


BAD = [("lr_plateau_factor", v) for v in (-0.1, 1, 1.0, 1.5, "0.5", None, True, float("nan"), 1 - 1e-12)] + \
      [("lr_plateau_patience", v) for v in (0, -1, 1.5, 2.0, "2", None, True)] + \
      [("lr_plateau_min_scale", v) for v in (-0.1, 1, 1.0, 2, "0.1", None, False, float("nan"))]


@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("key,bad", BAD)
def test_every_bad_value_is_refused_on_the_host(key, bad, on):
    cfg = dict(ON if on else {}, **{key: bad})
    with pytest.raises(ValueError, match=f"'{key}' must be"):
        lr_plateau_rule(cfg)
    for slots in (1, 2):   # (no device is touched: the engines get no further than the host checks)
        with pytest.raises(ValueError, match=f"'{key}' must be"):
            MultiPairEngine(cfg, None, [{}] * slots, (64, 64), device="cpu")
    with pytest.raises(ValueError, match=f"'{key}' must be"):
        MultiScaleEngine(cfg, None, {}, (64, 64), device="cpu")


def test_a_factor_needs_the_windows_of_the_stop_rule():
    for cfg in (dict(lr_plateau_factor=0.5), dict(lr_plateau_factor=0.5, stop_window=0)):
        with pytest.raises(ValueError, match="'lr_plateau_factor'.*'stop_window' > 0"):
            lr_plateau_rule(cfg)
        with pytest.raises(ValueError, match="'lr_plateau_factor'.*'stop_window' > 0"):
            MultiPairEngine(cfg, None, [{}] * 2, (64, 64), device="cpu")
    assert lr_plateau_rule(dict(stop_window=0, lr_plateau_patience=4)) == (0.0, 4, 0.0)   # off: the other keys are only checked


def test_the_engine_takes_the_keys_before_the_gpu():
    # the keys pass their check; the next host check (the crop counts) is the one that refuses: nothing has touched a GPU
    with pytest.raises(ValueError, match="n_crops"):
        MultiPairEngine(dict(ON), None, [{}] * 2, (64, 64), (64, 64), device="cpu", n_crops=(9, 1))


def test_the_keys_are_shared_by_the_slots_of_a_sweep():
    for key, val in (("lr_plateau_factor", 0.25), ("lr_plateau_patience", 3), ("lr_plateau_min_scale", 0.5)):
        with pytest.raises(ValueError, match=f"'{key}' is shared"):
            merge_pair_cfgs(dict(ON), [{}, {key: val}])
    merged = merge_pair_cfgs(dict(ON, lr_plateau_patience=3), [{}, dict(lr_plateau_factor=0.5, lr_plateau_patience=3, lr=0.1)])
    assert merged[1]["lr_plateau_factor"] == 0.5 and merged[1]["lr"] == 0.1


def test_multiscale_engine_refuses_the_rule():
    with pytest.raises(NotImplementedError, match="lr_plateau_factor.*MultiScaleEngine"):
        MultiScaleEngine(dict(ON), None, {}, (64, 64), device="cpu")


def test_scheduler_policy_plateau_stays_refused_and_points_at_the_keys():
    from splice_amd.util import LrSchedule
    with pytest.raises(NotImplementedError, match="plateau.*lr_plateau_factor"):
        LrSchedule(dict(DEFAULT_CFG, scheduler_policy="plateau"))


def test_batch_set_parses_the_keys():
    from splice_amd import batch
    cfg = dict(stop_window=batch._parse_value("5"), lr_plateau_factor=batch._parse_value("0.5"), lr_plateau_patience=batch._parse_value("2"),
               lr_plateau_min_scale=batch._parse_value("0.1"))
    assert lr_plateau_rule(cfg) == (0.5, 2, 0.1)


# --------------------------------------------------------------------------------------------------------- the restatement
def sequences():
    """The three 200-step sequences of tests/test_stop_gpu.py::test_rule_alone_equals_numpy_restatement (falling then flat, flat, rising)
    and its mask of counted steps."""
    steps = 200
    rng = np.random.default_rng(11)
    t = np.arange(steps, dtype=np.float64)
    seqs = np.stack([2.0 * np.exp(-t / 25.0) + 0.1 + 1e-4 * rng.standard_normal(steps),
                     1.0 + 1e-3 * rng.standard_normal(steps),
                     0.5 + 0.01 * t + 1e-3 * rng.standard_normal(steps)]).astype(np.float32)
    return seqs, [(k >= 3 and k % 7 != 0) for k in range(steps)]


# (W, rel, stop_patience, min_steps, factor, lr_patience, min_scale)
PARAMS = [(5, 0.01, 2, 40, 0.5, 2, 0.1), (5, 0.01, 1000, 0, 0.5, 2, 0.1), (1, 0.01, 1000, 0, 0.9, 1, 0.0)]


@pytest.mark.parametrize("params", PARAMS)
def test_the_stop_fields_are_those_of_the_stop_rule(params):
    seqs, counted = sequences()
    for seq in seqs:
        want = np_plateau(seq, counted, *params[:4])
        got = np_lr_plateau(seq, counted, *params)
        for k in STOP_FIELDS:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (k, got[k], want[k])
        assert got["scales"].dtype == f32 and len(got["scales"]) == len(seq) and got["scales"][0] == 1
        lr = got["lr"]
        assert lr["cuts"] == len(lr["cut_steps"]) and lr["last_cut_step"] == (lr["cut_steps"][-1] if lr["cut_steps"] else -1)
        assert replay_lr_scales(lr["cut_steps"], len(seq), params[4], params[6]).tobytes() == got["scales"].tobytes()


def test_what_the_three_parameter_sets_cover():
    seqs, counted = sequences()
    falling, flat, rising = [[np_lr_plateau(seq, counted, *p) for p in PARAMS] for seq in seqs]
    # set 0: every slot stops, and the lr record stays what it was at the stop (no cut behind the stop step)
    for got in (falling[0], flat[0], rising[0]):
        assert 0 <= got["stop_step"] < 199 and all(t <= got["stop_step"] for t in got["lr"]["cut_steps"])
    assert flat[0]["lr"]["cuts"] < flat[1]["lr"]["cuts"]                       # (the same slot goes on cutting when it does not stop)
    # set 1: the falling sequence's better windows reset `bad`: its first cut comes late; the flat and rising ones reach the floor in four cuts
    assert falling[1]["lr"]["cut_steps"][0] > 100 and flat[1]["lr"]["cut_steps"][0] < 30
    for got in (flat[1], rising[1]):
        assert got["lr"]["cuts"] == 4 and got["lr"]["scale"] == f32(0.1) and got["scales"][-1] == f32(0.1)
        assert [float(x) for x in sorted(set(got["scales"]), reverse=True)] == [1.0, 0.5, 0.25, 0.125, float(f32(0.1))]
    # set 2: one cut per window until the cap
    got = rising[2]
    assert got["lr"]["cuts"] == STOP_HISTORY == 64 and got["windows"] > 64 + 1 and got["lr"]["bad"] == got["windows"] - 1 - 64
    scale = f32(1)
    for _ in range(64):
        scale = f32(scale * f32(0.9))
    assert got["lr"]["scale"].tobytes() == scale.tobytes()


def _window_means64(seq, counted, window):
    out, acc = [], []
    for t, (x, c) in enumerate(zip(seq, counted)):
        if c:
            acc.append(float(x))
            if len(acc) == window:
                out.append((t, sum(acc) / window))
                acc = []
    return out


@pytest.mark.parametrize("params", PARAMS[1:])
def test_cuts_fall_where_reduce_lr_on_plateau_cuts(params):
    """torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor, patience=lr_patience - 1, threshold=stop_rel, threshold_mode='rel',
    cooldown=0, min_lr=min_scale x lr) fed the float64 window means: the same windows, up to the cap of 64 cuts."""
    window, rel, patience, min_steps, factor, lr_patience, min_scale = params
    seqs, counted = sequences()
    for seq in seqs:
        margins = []
        got = np_lr_plateau(seq, counted, *params, margins=margins)
        assert margins and min(margins) > 1e-5, min(margins)        # no comparison sits at its threshold: float32 against float64 cannot decide one
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
        sch = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, mode="min", factor=factor, patience=lr_patience - 1, threshold=rel, threshold_mode="rel",
                                                         cooldown=0, min_lr=min_scale, eps=0.0)
        cuts = []
        for t, mean in _window_means64(seq, counted, window):
            before = opt.param_groups[0]["lr"]
            sch.step(mean)
            if opt.param_groups[0]["lr"] < before:
                cuts.append(t)
        assert got["lr"]["cut_steps"] == cuts[:STOP_HISTORY], (got["lr"]["cut_steps"], cuts)
        assert len(cuts) <= STOP_HISTORY or got["lr"]["cuts"] == STOP_HISTORY


def test_the_floor_is_reached_and_held():
    losses = [1.0] * 40
    got = np_lr_plateau(losses, [True] * 40, 2, 0.01, 1000, 0, 0.3, 1, 0.05)
    # 1 -> 0.3 -> 0.09 -> max(0.027, 0.05): three cuts at the windows 1, 2, 3 (the first window is better), none later
    assert got["lr"]["cut_steps"] == [3, 5, 7] and got["lr"]["scale"].tobytes() == f32(0.05).tobytes()
    assert got["scales"][8:].tobytes() == np.full(32, 0.05, dtype=f32).tobytes()
    assert got["lr"]["bad"] == 20 - 1 - 3                        # (at the floor nothing resets the count any more)
    got = np_lr_plateau(losses, [True] * 40, 2, 0.01, 1000, 0, 0.5, 3, 0.0)
    assert got["lr"]["cut_steps"] == [7, 13, 19, 25, 31, 37]      # patience 3: every third flat window
    assert got["lr"]["scale"] == f32(0.5) ** 6 and got["lr"]["bad"] == 1


def test_the_cap_of_64_cuts_holds():
    n = 80
    got = np_lr_plateau([1.0] * n, [True] * n, 1, 0.01, 1000, 0, 0.99, 1, 0.0)
    assert got["lr"]["cuts"] == 64 and got["lr"]["cut_steps"] == list(range(1, 65)) and got["lr"]["last_cut_step"] == 64
    assert got["scales"][65:].tobytes() == np.full(n - 65, got["lr"]["scale"], dtype=f32).tobytes()
    assert got["lr"]["bad"] == n - 65


def test_a_cut_neither_resets_the_stop_rule_nor_waits_for_min_steps():
    got = np_lr_plateau([1.0] * 12, [True] * 12, 2, 0.01, 3, 100, 0.5, 1, 0.0)
    assert got["lr"]["cut_steps"] == [3, 5, 7, 9, 11] and got["bad"] == 5 and got["stop_step"] == -1   # min_steps holds the stop back only
    got = np_lr_plateau([1.0] * 12, [True] * 12, 2, 0.01, 3, 0, 0.5, 1, 0.0)
    assert got["stop_step"] == 7 and got["lr"]["cut_steps"] == [3, 5, 7]        # the stopping step is still live; later windows do not cut


# ---------------------------------------------------------------------------------------------------------- the end of a run
class Engine(MultiPairEngine):
    """The host side of a real engine over fabricated device state (CPU tensors): ``loss_trace_columns``, ``lr_state`` and ``lr_scale``
    are the product's own code; nothing launches."""

    def __init__(self, slots, steps, cuts, rule=(0.5, 1, 0.1), cfg=None, single=False):
        self.cfg = dict(DEFAULT_CFG, **(cfg or {}))
        self.cfgs, self.P, self.single = [self.cfg] * slots, slots, single
        self.stop_rule, self.lr_rule = (3, 0.01, 1000, 0), rule
        self._pair_lr, self.plan_e, self.handle = False, None, None
        self._stopped, self._stop_dirty, self._lr_scale = [None] * slots, False, [1.0] * slots
        self.ema = self.best = self.best_ema = self.clip_dev = None
        self.grad_clip, self.ema_rule = 0.0, (0.0, 0)
        self.step_idx, self.lr, self.steps = -1, self.cfg["lr"], steps
        self.trace_dev = torch.arange(steps * slots * 8, dtype=torch.float32).reshape(steps, slots, 8)
        self.lr_state_dev = self.lr_cuts_dev = None
        if rule[0] > 0:
            scales = [replay_lr_scales(c, steps + 1, rule[0], rule[2])[-1] for c in cuts]
            self.lr_state_dev = torch.tensor([[int(np.float32(s).view(np.int32)), 0, len(c), c[-1] if c else -1] for s, c in zip(scales, cuts)], dtype=torch.int32)
            self.lr_cuts_dev = torch.tensor([c + [-1] * (STOP_HISTORY - len(c)) for c in cuts], dtype=torch.int32)

    def generate(self, img, pair=0, track_running_stats=False, ema=False, best=False):
        return ["image"]

    def step(self, a, b, entire):
        self.step_idx += 1

    def book_logged_forward(self):
        pass

    def window_closes(self, step_idx):
        return False

    def losses(self):
        return {"loss": 0.5} if self.single else [{"loss": 0.5}] * self.P

    def lr_state(self, pair=None):     # (single: what SpliceEngine hands out)
        return MultiPairEngine.lr_state(self, 0 if self.single else pair)

    @property
    def lr_scale(self):
        scales = MultiPairEngine.lr_scale.fget(self)
        return scales[0] if self.single else scales


class Writer:
    def __init__(self, d):
        self.dir = str(d)
        os.makedirs(self.dir)

    def submit(self, image, force=True, name="output.png"):
        pass

    def close(self):
        pass


def _loop(tmp_path, eng, progress=False, **cfg):
    writers = [Writer(tmp_path / f"slot{p}") for p in range(eng.P)]
    _optimise(dict(n_epochs=eng.steps, log_images_freq=100, **cfg), eng, lambda: ("a", "b", None), ["A"] * eng.P, writers, None, progress, single=eng.single)
    return writers


def _lr_column(path):
    lines = open(path).read().split("\n")[1:-1]
    return np.array([float(ln.split(",")[1]) for ln in lines], dtype=np.float64)


def test_losses_csv_holds_the_effective_lr(tmp_path):
    cuts = [[2, 5, 6, 9], [], [0]]
    eng = Engine(3, 12, cuts, cfg=dict(lr=0.002, scheduler_policy="cosine", n_epochs=12))
    writers = _loop(tmp_path, eng, loss_trace=True)
    from splice_amd.util import LrSchedule
    for p, w in enumerate(writers):
        sch = LrSchedule(eng.cfg)
        want, scale = [], f32(1)
        for s in range(12):
            want.append(f32(sch.lr(s)) * scale)                       # the scale in force at step s: cuts made at earlier steps
            if s in cuts[p]:
                scale = max(f32(scale * f32(0.5)), f32(0.1))
        got = _lr_column(os.path.join(w.dir, "losses.csv"))
        assert got.astype(f32).tobytes() == np.array(want, dtype=f32).tobytes(), (p, got, want)   # (%.9g: parses back to the bits)
    floored = _lr_column(os.path.join(writers[0].dir, "losses.csv"))[10]
    assert f32(floored) == f32(LrSchedule(eng.cfg).lr(10)) * f32(0.1)   # 0.0625 is floored


def test_result_fields(tmp_path):
    from splice_amd import batch
    eng = Engine(2, 12, [[2, 5], []])
    _loop(tmp_path, eng)
    assert lr_fields(eng, 0) == {"lr_plateau_factor": 0.5, "lr_cuts": 2, "lr_cut_steps": [2, 5], "lr_scale": 0.25}
    assert lr_fields(eng, 1) == {"lr_plateau_factor": 0.5, "lr_cuts": 0, "lr_cut_steps": [], "lr_scale": 1.0}
    fields = batch._slot_fields(eng, 0)
    assert fields["lr_cuts"] == 2 and fields["lr_cut_steps"] == [2, 5] and fields["lr_scale"] == 0.25 and fields["lr_plateau_factor"] == 0.5
    json.dumps(fields)                                                    # plain numbers and lists
    assert eng.lr_state(1) == dict(scale=f32(1), bad=0, cuts=0, last_cut_step=-1, cut_steps=[])
    one = Engine(1, 4, [[1]], single=True)
    _loop(tmp_path / "one", one)
    assert lr_fields(one) == {"lr_plateau_factor": 0.5, "lr_cuts": 1, "lr_cut_steps": [1], "lr_scale": 0.5} and one.lr_state()["cuts"] == 1
    off = Engine(2, 4, [[], []], rule=(0.0, 1, 0.0))
    assert lr_fields(off, 1) == {"lr_plateau_factor": 0.0, "lr_cuts": 0, "lr_cut_steps": [], "lr_scale": 1.0}
    with pytest.raises(RuntimeError, match="lr_plateau_factor"):
        off.lr_state()


def test_with_the_rule_off_the_file_and_the_progress_line_are_what_they_were(tmp_path, capsys):
    off = Engine(1, 3, [[]], rule=(0.0, 1, 0.0), single=True)
    w = _loop(tmp_path / "off", off, progress=True, loss_trace=True)
    assert capsys.readouterr().out == "Epoch 1: loss=0.5000 lr=0.002\n"
    assert _lr_column(os.path.join(w[0].dir, "losses.csv")).tolist() == [0.002] * 3
    assert open(os.path.join(w[0].dir, "losses.csv")).readline() == "step,lr,loss,loss_global_ssim,loss_entire_ssim,loss_entire_cls,loss_global_cls,loss_global_id_B\n"
    assert off.lr_scale == 1.0
    on = Engine(1, 3, [[0]], single=True)
    on._lr_scale = [0.5]                                                  # (the host's copy: what the last closed window left)
    _loop(tmp_path / "on", on, progress=True)
    assert capsys.readouterr().out == "Epoch 1: loss=0.5000 lr=0.002 lr_scale=0.5\n"
    many = Engine(2, 3, [[0], []])
    many._lr_scale = [0.5, 1.0]
    _loop(tmp_path / "many", many, progress=True)
    assert capsys.readouterr().out == "Epoch 1: loss=0.5000, 0.5000 lr=0.002 lr_scale=[0.5, 1.0]\n"


# --------------------------------------------------------------------------------------------------------------- the exports
def test_exports_declared_bound_and_present():
    names = ("splice_step_set_lr_plateau", "splice_plateau_update_lr")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["splice_step_set_lr_plateau"][0]) == 6 and len(_lib._SIGNATURES["splice_plateau_update_lr"][0]) == 18
    assert len(_lib._SIGNATURES["splice_plateau_update"][0]) == 10 and len(_lib._SIGNATURES["splice_total_loss_pairs_trace"][0]) == 26   # (as they were)
    assert ctypes.sizeof(_lib.LrState) == 16 and [f[0] for f in _lib.LrState._fields_] == ["scale", "bad", "cuts", "last_cut_step"]
    assert "typedef struct splice_lr_state {" in hdr and _lib.STOP_HISTORY == STOP_HISTORY == 64
