"""CPU: the per-step loss trace is off by default, its setting is checked on the host before anything touches a GPU,
losses.csv round-trips every float32, the train loop writes one file per slot exactly when the key is on, and the exports are declared,
built and bound."""
import ctypes
import os

import numpy as np
import pytest
import yaml

from splice_amd import _lib
from splice_amd.engine import DEFAULT_CFG, LOSS_KEYS, PAIR_KEYS, MultiPairEngine, MultiScaleEngine, active_terms, merge_pair_cfgs, trace_rule
from splice_amd.train import _optimise, trace_fields
from splice_amd.util import write_loss_trace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def test_option_is_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    assert DEFAULT_CFG["loss_trace"] is False and packaged["loss_trace"] is False
    assert trace_rule({}) is False and trace_rule(packaged) is False and trace_rule(dict(loss_trace=True)) is True
    assert "loss_trace" not in PAIR_KEYS


@pytest.mark.parametrize("bad", ["yes", 1.5, 2, 1, 0, None])
def test_trace_rule_refuses_what_is_no_bool(bad):
    with pytest.raises(ValueError, match="'loss_trace' must be true or false"):
        trace_rule(dict(loss_trace=bad))
    with pytest.raises(ValueError, match="'loss_trace' must be"):
        MultiPairEngine(dict(loss_trace=bad), None, [{}], (64, 64), device="cpu")
    with pytest.raises(ValueError, match="'loss_trace' must be"):
        MultiScaleEngine(dict(loss_trace=bad), None, {}, (64, 64), device="cpu")


def test_engine_takes_the_key_before_the_gpu():
    # the key passes its check; the next host check (the crop counts) is the one that refuses: nothing has touched a GPU
    with pytest.raises(ValueError, match="n_crops"):
        MultiPairEngine(dict(loss_trace=True), None, [{}] * 2, (64, 64), (64, 64), device="cpu", n_crops=(9, 1))


def test_multiscale_engine_refuses_the_key():
    with pytest.raises(NotImplementedError, match="loss_trace.*phase-mode"):
        MultiScaleEngine(dict(loss_trace=True), None, {}, (64, 64), device="cpu")


def test_option_is_shared_by_the_slots_of_a_sweep():
    with pytest.raises(ValueError, match="'loss_trace' is shared"):
        merge_pair_cfgs({}, [{}, dict(loss_trace=True)])
    assert merge_pair_cfgs(dict(loss_trace=True), [{}, dict(loss_trace=True, lr=0.1)])[1]["loss_trace"] is True


def test_batch_set_parses_the_key():
    from splice_amd import batch
    assert batch._parse_value("true") is True and trace_rule(dict(loss_trace=batch._parse_value("true"))) is True
    assert trace_rule(dict(loss_trace=batch._parse_value("false"))) is False


def test_active_terms_over_the_three_regimes():
    c = dict(DEFAULT_CFG, cls_warmup=2, entire_A_every=3)
    names = lambda s, ent=True, cfg=c: [k for k in LOSS_KEYS if active_terms(cfg, s, ent)[k]]
    assert names(0) == ["loss", "loss_entire_ssim", "loss_entire_cls", "loss_global_cls"]          # warm-up and an entire-image step
    assert names(1) == ["loss", "loss_global_cls"]                                                 # warm-up
    assert names(2) == ["loss", "loss_global_ssim", "loss_global_cls", "loss_global_id_B"]         # ordinary
    assert names(3) == LOSS_KEYS                                                                   # everything
    assert names(3, ent=False) == names(2)                                                         # an engine without the branch
    assert names(3, cfg=dict(c, lambda_global_identity=0, lambda_entire_cls=0)) == ["loss", "loss_global_ssim", "loss_entire_ssim", "loss_global_cls"]


# ------------------------------------------------------------------------------------------------------------- losses.csv
def _bits(x):
    return np.asarray(x, dtype=f32).view(np.uint32)


def _fabricated():
    """5 rows that hold the awkward float32 values: denormals (smallest and largest), the smallest normal, the largest finite, values
    with nine significant digits, a negative zero, an infinity and NaN."""
    special = np.array([1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x3DCCCCCD, 0x3F800001, 0x80000000, 0x7F800000], dtype=np.uint32).view(f32)
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((5, 8)).astype(f32)
    rows[3] = special                                                     # (step 3 computes every term)
    rows[1] = rng.integers(0, 0x7F800000, 8, dtype=np.uint32).view(f32)   # random finite bit patterns
    rows[2, :6] = rng.integers(0, 0x00800000, 6, dtype=np.uint32).view(f32)   # denormals
    rows[4, 6:] = np.nan
    return rows


def _read(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0].split(","), [ln.split(",") for ln in lines[1:-1]]


@pytest.mark.parametrize("clip", [False, True])
def test_write_loss_trace_round_trips_every_float(tmp_path, clip):
    rows = _fabricated()
    c = dict(DEFAULT_CFG, cls_warmup=2, entire_A_every=3)
    active = [active_terms(c, s, True) for s in range(5)]
    lrs = [0.002, 0.002 * (1 - 1 / 3), 1e-6, 0.0, 1.0]
    path = tmp_path / "out" / "losses.csv"
    write_loss_trace(path, rows, lrs, active, clip)
    header, body = _read(path)
    assert header == ["step", "lr"] + LOSS_KEYS + (["grad_norm", "clip_coef"] if clip else [])
    assert len(body) == 5 and [ln[0] for ln in body] == ["0", "1", "2", "3", "4"]
    for s, ln in enumerate(body):
        assert len(ln) == len(header)
        assert f32(float(ln[1])) == f32(lrs[s])
        for i, k in enumerate(LOSS_KEYS):
            if active[s][k]:
                assert _bits(float(ln[2 + i])) == _bits(rows[s, i]), (s, k, ln[2 + i], rows[s, i])
            else:
                assert ln[2 + i] == ""                                   # an inactive term is a blank field
        if clip:
            for i in (6, 7):
                got = f32(float(ln[2 + i]))
                assert (np.isnan(got) and np.isnan(rows[s, i])) or _bits(got) == _bits(rows[s, i])
    assert body[1][2 + LOSS_KEYS.index("loss_global_ssim")] == "" and body[1][2 + LOSS_KEYS.index("loss_global_cls")] != ""
    assert not os.path.exists(str(path) + ".tmp")


def test_write_loss_trace_holds_the_rows_it_is_given(tmp_path):
    # a slot that stopped at step 2 of 5: loss_trace() hands over 3 rows, the file has 3 lines
    rows = _fabricated()[:3]
    c = dict(DEFAULT_CFG)
    write_loss_trace(tmp_path / "losses.csv", rows, [0.002] * 3, [active_terms(c, s, False) for s in range(3)], False)
    _, body = _read(tmp_path / "losses.csv")
    assert [ln[0] for ln in body] == ["0", "1", "2"]
    write_loss_trace(tmp_path / "losses.csv", rows[:0], [], [], True)    # no step ran: the header alone
    header, body = _read(tmp_path / "losses.csv")
    assert body == [] and header[-2:] == ["grad_norm", "clip_coef"]


# ---------------------------------------------------------------------------------------------------------- the train loop
class Engine:
    """The stub of tests/test_train_loop_cpu.py with a trace: slot p ran ``ran[p]`` steps."""

    def __init__(self, slots, ran, trace, clip=0.0):
        self.slots, self.ran, self.step_idx, self.lr = slots, ran, -1, 0.002
        self.ema = self.best = self.best_ema = None
        self.grad_clip = clip
        self.trace_dev = "rows" if trace else None
        self.asked = 0

    def generate(self, img, pair=0, track_running_stats=False, ema=False, best=False):
        return ["image"]

    def step(self, a, b, entire):
        self.step_idx += 1

    def book_logged_forward(self):
        pass

    def window_closes(self, step_idx):
        return False

    def all_stopped(self):
        return False

    def loss_trace_columns(self):
        self.asked += 1
        assert self.trace_dev is not None
        c = dict(DEFAULT_CFG)
        out = []
        for p in range(self.slots):
            n = min(self.ran[p], self.step_idx + 1)
            rows = np.full((n, 8), p + 0.5, dtype=f32)
            out.append((rows, [0.002] * n, [active_terms(c, s, False) for s in range(n)]))
        return out


class Writer:
    def __init__(self, d):
        self.dir = d
        os.makedirs(d)
        self.closed = False

    def submit(self, image, force=True, name="output.png"):
        pass

    def close(self):
        self.closed = True


def _loop(tmp_path, slots, ran, on, n_epochs=4, clip=0.0):
    eng = Engine(slots, ran, on, clip)
    writers = [Writer(str(tmp_path / f"slot{p}")) for p in range(slots)]
    cfg = dict(n_epochs=n_epochs, log_images_freq=2)
    if on is not None:
        cfg["loss_trace"] = on
    _optimise(cfg, eng, lambda: ("a", "b", None), ["A"] * slots, writers, None, False, single=slots == 1)
    assert all(w.closed for w in writers)
    return eng, writers


@pytest.mark.parametrize("slots", [1, 3])
def test_the_loop_writes_one_file_per_slot_when_the_key_is_on(tmp_path, slots):
    ran = [4, 2, 4][:slots]
    eng, writers = _loop(tmp_path, slots, ran, True, clip=1.0 if slots == 3 else 0.0)
    assert eng.asked == 1                                                # one copy, at the end of the run
    for p, w in enumerate(writers):
        assert os.listdir(w.dir) == ["losses.csv"]
        header, body = _read(os.path.join(w.dir, "losses.csv"))
        assert len(body) == ran[p] and all(float(ln[2]) == p + 0.5 for ln in body)
        assert (header[-1] == "clip_coef") == (slots == 3)
    assert trace_fields(eng) == {"loss_trace": "losses.csv"} and trace_fields(eng, os.path.join("sweep", "2")) == {"loss_trace": os.path.join("sweep", "2", "losses.csv")}


@pytest.mark.parametrize("on", [False, None])
def test_the_loop_writes_nothing_when_the_key_is_off(tmp_path, on):
    eng, writers = _loop(tmp_path, 2, [4, 4], on)
    assert eng.asked == 0 and all(os.listdir(w.dir) == [] for w in writers)
    assert trace_fields(eng) == {}


def test_no_epochs_no_file(tmp_path):
    eng, writers = _loop(tmp_path, 1, [0], True, n_epochs=0)
    assert eng.asked == 0 and os.listdir(writers[0].dir) == [] and trace_fields(eng) == {}


# --------------------------------------------------------------------------------------------------------------- the exports
def test_trace_exports_declared_bound_and_present():
    names = ("splice_step_set_loss_trace", "splice_total_loss_pairs_trace")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["splice_step_set_loss_trace"][0]) == 3
    assert len(_lib._SIGNATURES["splice_total_loss_pairs_trace"][0]) == len(_lib._SIGNATURES["splice_total_loss_pairs"][0]) + 8
    assert len(_lib._SIGNATURES["splice_grad_norm_pairs"][0]) == 11      # (its signature is what it was)
