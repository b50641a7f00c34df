"""GPU: clipping of every pair's gradient against its own running norm inside the fused step.  Op level: the
AUTO instance of the second norm launch against the NumPy restatement of the rule (engine.np_clip_auto fed engine.np_grad_clip's norm)
over a designed sequence of steps, frozen slots, refusals.  Then the fused step: a factor nothing reaches changes no bit, a clipped run
equals the restatement fed its recorded norms, graph replay equals eager launches, a pair's bits do not depend on its neighbours or on
a neighbour's stop, snapshots and compaction carry the records, the several-scales engine, train_model.  Every comparison is exact."""
import ctypes as C
import csv
import json

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import (CLIP_CHUNK, MultiPairEngine, MultiScaleEngine, SpliceEngine, clip_auto_records, clip_records, clip_regime, np_clip_auto,
                               np_grad_clip)
from splice_amd.generator import optim_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
HUGE = 1e30
F = np.float32


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return _np(a).tobytes() == _np(b).tobytes()


def _table(P=1):
    return torch.zeros(P, 6, dtype=torch.int32, device=DEV)


def _partials(P, n, guard=8):   # (tests/test_clip_gpu.py::_partials)
    chunks = (n + CLIP_CHUNK - 1) // CLIP_CHUNK
    return torch.full((P * chunks + guard,), -7.0, device=DEV), P * chunks


def _norm_auto(g, g2, P, stride, n, c, rule, regime, part, state, auto, stop=None, step_dev=None):
    k, beta, warmup = rule
    return _lib.lib().splice_grad_norm_pairs_auto(_lib.ptr(g), _lib.ptr(g2), P, stride, n, c, k, beta, warmup, regime, _lib.ptr(part), _lib.ptr(state), _lib.ptr(auto),
                                                  _lib.ptr(stop), _lib.ptr(step_dev), _lib.current_stream())


class Restated:
    """One pair's two records as the NumPy restatement leaves them, step after step."""

    def __init__(self, rule, cap):
        self.rule, self.cap, self.auto, self.clipped, self.skipped, self.last = rule, cap, None, 0, 0, None

    def step(self, sumsq, norm, regime):
        before = self.auto
        self.auto, coef, skip = np_clip_auto(self.auto, norm, regime, *self.rule, self.cap)
        self.clipped += int(coef < 1 and not skip)
        self.skipped += skip
        self.last = dict(sumsq=F(sumsq), norm=F(norm), coef=coef, skip=skip, clipped=self.clipped, skipped=self.skipped)
        judged = regime >= 0 and before is not None and before["count"][regime] >= self.rule[2]
        return dict(coef=coef, skip=skip, judged=judged, thr=self.auto["thr"])

    def check(self, rec, auto, tag):
        for key in ("sumsq", "norm", "coef"):
            assert rec[key].tobytes() == self.last[key].tobytes(), (tag, key, rec[key], self.last[key])
        assert (rec["skip"], rec["clipped"], rec["skipped"]) == (self.last["skip"], self.last["clipped"], self.last["skipped"]), (tag, rec, self.last)
        assert [x.tobytes() for x in auto["ref"]] == [x.tobytes() for x in self.auto["ref"]], (tag, auto, self.auto)
        assert auto["count"] == self.auto["count"] and auto["regime"] == self.auto["regime"] and auto["thr"].tobytes() == self.auto["thr"].tobytes(), (tag, auto, self.auto)


# ------------------------------------------------------------------------------------------------------------------- op level
SEQ_STEPS, SEQ_RULE = 44, (2.0, 0.9, 4)
SEQ_LEVELS = (1.0, 3.0, 0.2)
SEQ_SPIKES = {(0, 23): 10.0, (1, 30): 10.0}     # (pair, step): regime 0 behind its warm-up; regime 1 behind its own (steps 5 .. 25 observed)
SEQ_NAN = (2, 17)                               # one NaN element in pair 2 alone


def _seq_regime(t):
    return -1 if t == 0 else 1 if t % 5 == 0 else 0


def _sequence():
    """s[p, t]: levels that fall from 1 to 0.5 with 10 % jitter, entire-image steps (every 5th) at three times the level, the spikes."""
    rng = np.random.default_rng(5)
    s = np.linspace(1.0, 0.5, SEQ_STEPS)[None] * rng.lognormal(0, 0.1, (3, SEQ_STEPS)) * np.array(SEQ_LEVELS)[:, None]
    s *= np.array([3.0 if _seq_regime(t) == 1 else 1.0 for t in range(SEQ_STEPS)])[None]
    for (p, t), x in SEQ_SPIKES.items():
        s[p, t] *= x
    return s.astype(F)


@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("n,stride,cap", [(1027, 1088, 0.0), (4100, 4160, 700.0)])
def test_both_records_equal_the_restatement_after_every_step(n, stride, cap, with_g2):
    """Three pairs over 44 designed steps: both regimes, a step before cls_warmup, a spike in each regime behind its warm-up, one NaN
    element in one pair.  The cap of 700 lies over every norm but the two spikes' (the largest other is about 3 * 3 * sqrt(4100) = 576
    times its jitter), under k times the entire-image reference of pair 1 (about 2 * 500) and over k times the ordinary reference of pair
    0 (about 2 * 50): pair 1's spike is clipped by the cap, pair 0's by its running norm."""
    P = 3
    gen = torch.Generator().manual_seed(n + with_g2)
    u, w = torch.randn(P, stride, generator=gen), torch.randn(P, stride, generator=gen) * 0.25    # (the padding holds values too: it is not read)
    s = _sequence()
    state, auto = _table(P), _table(P)
    part, used = _partials(P, n)
    ref = [Restated(SEQ_RULE, cap) for _ in range(P)]
    seen = []
    for t in range(SEQ_STEPS):
        g_h = u * torch.from_numpy(s[:, t])[:, None]
        g2_h = w * torch.from_numpy(s[:, t])[:, None] if with_g2 else None
        if t == SEQ_NAN[1]:
            g_h[SEQ_NAN[0], 5] = float("nan")
        g, g2 = g_h.to(DEV), (None if g2_h is None else g2_h.to(DEV))
        assert _norm_auto(g, g2, P, stride, n, cap, SEQ_RULE, _seq_regime(t), part, state, auto) == 0, _lib.lib().splice_last_error()
        recs, autos = clip_records(state), clip_auto_records(auto)
        for p in range(P):
            sumsq, norm, _, _ = np_grad_clip(_np(g_h[p, :n]), None if g2_h is None else _np(g2_h[p, :n]), HUGE)
            seen.append(dict(ref[p].step(sumsq, norm, _seq_regime(t)), pair=p, step=t))
            ref[p].check(recs[p], autos[p], (t, p))
    assert bool((part[used:] == -7.0).all())
    # the premises, on the restatement's own output: the case cannot pass vacuously
    clipped = [(d["pair"], d["step"]) for d in seen if d["coef"] < 1 and not d["skip"]]
    assert set(SEQ_SPIKES) <= set(clipped) and len(clipped) < 8, clipped
    assert sum(d["judged"] and d["coef"] == 1 and not d["skip"] for d in seen) >= 60
    assert [(d["pair"], d["step"]) for d in seen if d["skip"]] == [SEQ_NAN]
    assert all(min(r.auto["count"]) > SEQ_RULE[2] for r in ref) and [r.auto["count"] for r in ref] == [[35, 8], [35, 8], [34, 8]]
    if cap:
        thr = {(d["pair"], d["step"]): d["thr"] for d in seen}
        assert thr[(1, 30)] == F(cap) and thr[(0, 23)] < F(cap) and thr[(0, 0)] == F(cap) and clipped == sorted(SEQ_SPIKES)
    assert len({a["ref"][0].tobytes() for a in autos}) == 3                                       # every pair has its own reference


def _stop_records(P, stopped):   # (tests/test_ema_gpu.py::_stop_records)
    state = torch.zeros(P, 6, dtype=torch.int32)
    state[:, 5] = -1
    for slot, k in stopped.items():
        state[slot, 5] = k
    return state.to(DEV)


def test_a_frozen_slot_keeps_both_records():
    """Slot 1 of 3 stopped at step index 0: the launch of step 1 still writes its records, those of steps 2 to 4 leave both alone."""
    P, n, stride, rule = 3, 4100, 4160, (1.0, 0.0, 1)
    gen = torch.Generator().manual_seed(17)
    stop = _stop_records(P, {1: 0})
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    state, auto, part = _table(P), _table(P), _partials(P, n)[0]
    ref = [Restated(rule, 0.0) for _ in range(P)]
    frozen = None
    for t in (1, 2, 3, 4):
        step_dev.fill_(t)
        g_h = torch.randn(P, stride, generator=gen) * t
        assert _norm_auto(g_h.to(DEV), None, P, stride, n, 0.0, rule, 0, part, state, auto, stop, step_dev) == 0
        recs, autos = clip_records(state), clip_auto_records(auto)
        for p in (0, 2) + ((1,) if t == 1 else ()):
            sumsq, norm, _, _ = np_grad_clip(_np(g_h[p, :n]), None, HUGE)
            ref[p].step(sumsq, norm, 0)
            ref[p].check(recs[p], autos[p], (t, p))
        if t == 1:
            frozen = (state[1].clone(), auto[1].clone())
            assert autos[1]["count"] == [1, 0] and autos[1]["ref"][0] > 0
        else:
            assert _same(state[1], frozen[0]) and _same(auto[1], frozen[1]), t
    assert clip_records(state)[0]["clipped"] == 3 and clip_auto_records(auto)[2]["count"] == [4, 0]   # (the norms grow: k = 1 clips steps 2 to 4)


def test_invalid_arguments_are_refused():
    L = _lib.lib()
    g, part, state, auto = torch.zeros(4352, device=DEV), torch.zeros(8, device=DEV), _table(2), _table(2)
    ok = dict(c=0.0, k=2.0, beta=0.9, warmup=4, regime=0, P=1, stride=0, n=4, gp=g, pp=part, sp=state, ap=auto)

    def call(**over):
        a = dict(ok, **over)
        return _norm_auto(a["gp"], None, a["P"], a["stride"], a["n"], a["c"], (a["k"], a["beta"], a["warmup"]), a["regime"], a["pp"], a["sp"], a["ap"])
    assert call() == 0 and call(c=1.0) == 0 and call(regime=-1) == 0 and call(regime=1) == 0 and call(k=1.0, beta=0.0, warmup=1) == 0
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(c=bad) != 0 and b"max_norm" in L.splice_last_error(), bad
    for bad in (dict(k=0.5), dict(k=0.0), dict(k=float("nan")), dict(k=float("inf")), dict(beta=1.0), dict(beta=-0.1), dict(beta=float("nan")), dict(warmup=0),
                dict(regime=2), dict(regime=-2), dict(ap=None)):
        assert call(**bad) != 0 and b"running norm" in L.splice_last_error(), bad
    assert call(sp=None) != 0 and call(pp=None) != 0 and call(gp=None) != 0 and call(n=0) != 0 and call(P=0) != 0
    assert call(P=2, stride=2174, n=2170) != 0 and b"multiple of 4" in L.splice_last_error()
    assert call(P=2, stride=2176, n=2170) == 0
    stop = _stop_records(2, {})
    assert _norm_auto(g, None, 2, 2176, 2170, 0.0, (2.0, 0.9, 4), 0, part, state, auto, stop, None) != 0
    # the export without the rule keeps its own check: no cap is no rule there
    assert L.splice_grad_norm_pairs(_lib.ptr(g), None, 1, 0, 4, 0.0, _lib.ptr(part), _lib.ptr(state), None, None, _lib.current_stream()) != 0
    assert b"max_norm" in L.splice_last_error()
    torch.cuda.synchronize()
    assert clip_auto_records(auto)[1]["count"] == [1, 0]          # (only the accepted calls wrote: six of them saw pair 0, one pair 1)
    assert clip_auto_records(auto)[0]["count"] == [4, 1]


def test_optim_step_wrapper_clips_against_the_running_norm():
    n = 1027
    gen = torch.Generator().manual_seed(5)
    p0, g_h = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    p, m, v, state, auto = p0.to(DEV), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), _table(), _table()
    ref = Restated((1.0, 0.0, 1), 0.0)
    want = _np(p0)
    for t, scale in enumerate((1.0, 3.0)):                         # SGD: p -= lr * fl(g * coef); the second gradient is three times the first
        g = (g_h * scale).to(DEV)
        optim_step(2, p, g, m, v, 2e-3, 0.0, 0.0, 0.0, t + 1, clip_auto=(1.0, 0.0, 1), clip_regime=0, clip_state=state, clip_auto_state=auto)
        sumsq, norm, _, _ = np_grad_clip(_np(g_h * scale), None, HUGE)
        out = ref.step(sumsq, norm, 0)
        ref.check(clip_records(state)[0], clip_auto_records(auto)[0], t)
        want = (want - F(2e-3) * (_np(g_h * scale) * out["coef"]).astype(F)).astype(F)
        assert _np(p).tobytes() == want.tobytes(), t
    assert ref.clipped == 1 and F(0.33) < ref.last["coef"] < F(0.34)
    with pytest.raises(ValueError, match="clip_auto_state"):
        optim_step(2, p, g, m, v, 2e-3, 0.0, 0.0, 0.0, 3, clip_auto=(1.0, 0.0, 1), clip_state=state)


# ---------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):   # (tests/test_ema_gpu.py::_cfg)
    from splice_amd.engine import DEFAULT_CFG
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed, pair=0):
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _auto(k, beta=0.0, warmup=1):
    return dict(grad_clip_auto=k, grad_clip_auto_beta=beta, grad_clip_auto_warmup=warmup)


ONE = dict(cls_warmup=1, entire_A_every=4)
ONE_STEPS, ONE_EMA = 8, dict(ema_decay=0.5, ema_start=3)
TIGHT = _auto(1.0)                        # k = 1, beta = 0: the threshold is the regime's previous norm
_RUNS = {}


def _one_run(vit, rule=None, fixed=0.0, ema=False, graph=True, steps=ONE_STEPS, lr=2e-3, seed=61, trace=False):
    """``steps`` steps of one pair (cached per setting); per step the arenas, buffers, losses, the average and both records."""
    key = (None if rule is None else tuple(sorted(rule.items())), fixed, ema, graph, steps, lr, seed, trace)
    if key in _RUNS:
        return _RUNS[key]
    cfg = _cfg(**ONE, lr=lr, grad_clip_norm=fixed, n_epochs=steps, loss_trace=trace, **(rule or {}), **(ONE_EMA if ema else {}))
    eng = SpliceEngine(cfg, None, synth.generator_params(seed, 0.02), (64, 64), (64, 64), vit_engine=vit)
    if not graph:
        _lib.check(_lib.lib().splice_step_use_graph(eng.handle, 0), "use_graph")
    A, B = _pair(62)
    snaps = []
    for _ in range(steps):
        eng.step(A, B, A)
        snaps.append(dict(params=eng.params.clone(), m=eng.m.clone(), v=eng.v.clone(), running=eng.running.clone(), losses=eng.losses_dev.clone(),
                          ema=eng.pair_ema().clone() if ema else None, rec=None if eng.clip_dev is None else eng.clip_dev.clone(),
                          auto=None if eng.clip_auto_dev is None else eng.clip_auto_dev.clone()))
    torch.cuda.synchronize()
    _RUNS[key] = (eng, snaps)
    return _RUNS[key]


def _graphs(eng):
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    return stats[0] + stats[2]


@pytest.mark.parametrize("ema", [False, True])
def test_a_factor_nothing_reaches_changes_no_bit(vit, ema):
    """k = 1e30 with a warm-up of 1: from its second observation on a regime has a finite threshold (the entire-image steps see their
    first at step 4), and no norm comes near it."""
    eng, snaps = _one_run(vit, _auto(HUGE, 0.98, 1), ema=ema)
    assert _graphs(eng) >= 2                                           # graphs were in use (ordinary and entire-image variant)
    off, off_snaps = _one_run(vit, ema=ema)
    _, fixed_snaps = _one_run(vit, fixed=HUGE, ema=ema)
    assert off.clip_dev is None and off.clip_auto_dev is None
    with pytest.raises(RuntimeError, match="grad_clip_norm == 0"):
        off.clip_state()
    with pytest.raises(RuntimeError, match="grad_clip_auto == 0"):
        off.clip_auto_state()
    with pytest.raises(RuntimeError, match="grad_clip_auto == 0"):
        _one_run(vit, fixed=HUGE, ema=ema)[0].clip_auto_state()
    for k, (a, b, c) in enumerate(zip(snaps, off_snaps, fixed_snaps)):
        for key in ("params", "m", "v", "running", "losses") + (("ema",) if ema else ()):
            assert _same(a[key], b[key]), (k, key)
        assert _same(a["rec"], c["rec"]), k                            # sumsq, norm, coef 1, no skip, counts 0: the fixed rule's record
        auto = clip_auto_records(a["auto"])[0]
        assert auto["regime"] == clip_regime(k, 1, k % 4 == 0) and (np.isfinite(auto["thr"]) == (k in (2, 3, 5, 6, 7))), (k, auto)
    assert eng.clip_auto_state()["count"] == [6, 1] and eng.clip_state() == clip_records(snaps[-1]["rec"])[0]


# candidate settings of the clipped run, tried in this order: (lr, generator seed)
TIGHT_STEPS = 12
TIGHT_CANDIDATES = ((2e-3, 61), (5e-3, 61), (2e-2, 61), (2e-3, 62), (5e-2, 63))


def _tight_run(vit, **kw):
    """The first candidate whose run is clipped at some steps with a regime and not at all of them: (candidate, engine, snaps)."""
    tried = []
    for lr, seed in TIGHT_CANDIDATES:
        eng, snaps = _one_run(vit, TIGHT, steps=TIGHT_STEPS, lr=lr, seed=seed, **kw)
        clipped = clip_records(snaps[-1]["rec"])[0]["clipped"]
        tried.append((lr, seed, clipped))
        if 0 < clipped < TIGHT_STEPS - 1:                             # (steps 1 .. 11 have a regime)
            return (lr, seed), eng, snaps
    raise AssertionError(f"no candidate clips some steps and not all: {tried}")


def _check_against_restatement(snaps, rule, cap, cls_warmup, entire_every, tag):
    ref = Restated(rule, cap)
    for k, s in enumerate(snaps):
        rec = clip_records(s["rec"])[0]
        ref.step(rec["sumsq"], rec["norm"], clip_regime(k, cls_warmup, k % entire_every == 0))
        assert rec["norm"].tobytes() == np.sqrt(rec["sumsq"]).tobytes(), (tag, k)
        ref.check(rec, clip_auto_records(s["auto"])[0], (tag, k))
    return ref


def test_a_clipped_run_equals_the_restatement_fed_its_norms(vit):
    (lr, seed), eng, snaps = _tight_run(vit)
    print(f"clipped run: lr {lr}, generator seed {seed}, clipped {eng.clip_state()['clipped']} of {TIGHT_STEPS - 1} steps with a regime")
    ref = _check_against_restatement(snaps, (1.0, 0.0, 1), 0.0, 1, 4, "tight")
    assert 0 < ref.clipped < TIGHT_STEPS - 1 and ref.skipped == 0 and ref.auto["count"] == [9, 2]
    autos = [clip_auto_records(s["auto"])[0] for s in snaps]
    assert autos[0]["regime"] == -1 and autos[0]["thr"] == np.inf and autos[0]["count"] == [0, 0]          # step 0 lies before cls_warmup
    assert autos[4]["regime"] == 1 and autos[4]["thr"] == np.inf and autos[8]["thr"] == autos[4]["ref"][1]   # entire-image steps: a reference of their own
    _, off_snaps = _one_run(vit, steps=TIGHT_STEPS, lr=lr, seed=seed)
    first = min(k for k, s in enumerate(snaps) if clip_records(s["rec"])[0]["coef"] < 1)
    assert all(_same(snaps[k]["params"], off_snaps[k]["params"]) for k in range(first))
    assert not _same(snaps[first]["params"], off_snaps[first]["params"]) and not _same(snaps[-1]["params"], off_snaps[-1]["params"])
    assert eng.clip_auto_state() == autos[-1]


def test_graph_replay_equals_eager(vit):
    (lr, seed), eng, snaps = _tight_run(vit)
    _, eager = _one_run(vit, TIGHT, steps=TIGHT_STEPS, lr=lr, seed=seed, graph=False)
    assert _graphs(eng) >= 2
    for k, (a, b) in enumerate(zip(snaps, eager)):
        for key in ("params", "m", "v", "losses", "rec", "auto"):
            assert _same(a[key], b[key]), (k, key)


def test_the_cap_stays_beside_the_running_norm(vit):
    """Both keys: the threshold is the smaller of the two, step after step; before cls_warmup the cap alone."""
    _, plain = _one_run(vit, fixed=HUGE)
    cap = float(F(0.9) * max(clip_records(s["rec"])[0]["norm"] for s in plain))
    _, snaps = _one_run(vit, _auto(1.5, 0.5, 2), fixed=cap)
    ref = _check_against_restatement(snaps, (1.5, 0.5, 2), cap, 1, 4, "cap")
    thr = [clip_auto_records(s["auto"])[0]["thr"] for s in snaps]
    assert thr[0] == F(cap) and all(t <= F(cap) for t in thr) and ref.clipped >= 1


def test_the_trace_instance_writes_words_6_and_7(vit):
    (lr, seed), _, snaps = _tight_run(vit)
    eng, traced = _one_run(vit, TIGHT, steps=TIGHT_STEPS, lr=lr, seed=seed, trace=True)
    rows = eng.loss_trace()
    assert rows.shape == (TIGHT_STEPS, 8)
    for k, (a, b) in enumerate(zip(snaps, traced)):
        for key in ("params", "rec", "auto", "losses"):
            assert _same(a[key], b[key]), (k, key)                     # the trace changes no bit
        rec = clip_records(b["rec"])[0]
        assert rows[k, 6].tobytes() == rec["norm"].tobytes() and rows[k, 7].tobytes() == rec["coef"].tobytes(), k
        assert rows[k, :6].tobytes() == _np(b["losses"])[0, :6].tobytes(), k
    assert (rows[:, 7] < 1).any() and (rows[:, 7] == 1).any()


def test_three_pairs_equal_their_single_runs(vit):
    cfg = _cfg(**ONE, **TIGHT)
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    imgs = [_pair(71, p) for p in range(3)]
    As, Bs = torch.stack([a for a, _ in imgs]).contiguous(), torch.stack([b for _, b in imgs]).contiguous()
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit)
    for _ in range(7):
        multi.step(As, Bs, As)
    recs, autos = multi.clip_state(), multi.clip_auto_state()
    for p in range(3):
        single = SpliceEngine(cfg, None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for _ in range(7):
            single.step(imgs[p][0], imgs[p][1], imgs[p][0])
        torch.cuda.synchronize()
        assert _same(multi.pair_params(p), single.pair_params()), p
        assert _same(multi.clip_dev[p:p + 1], single.clip_dev) and _same(multi.clip_auto_dev[p:p + 1], single.clip_auto_dev), p
        assert multi.clip_state(p) == recs[p] and multi.clip_auto_state(p) == autos[p] == single.clip_auto_state(), p
    assert sum(r["clipped"] for r in recs) >= 1 and all(a["count"] == [5, 1] for a in autos)
    assert not _same(multi.clip_dev[0], multi.clip_dev[1]) and not _same(multi.clip_auto_dev[0], multi.clip_auto_dev[1])


# the settings of tests/test_clip_gpu.py::test_a_stopped_slot_keeps_the_record_of_its_stop_step
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2, stop_window=4)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 18
_SLOTS = {}


def _slots_run(vit):
    """The first stop_rel under which slots 0 and 2 stop with steps to spare while slot 1 runs on: (rel, engine, stop steps, inputs)."""
    if not _SLOTS:
        gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
        A, B = _pair(71)
        As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
        for rel in SLOT_RELS:
            multi = MultiPairEngine(_cfg(stop_rel=rel, **SLOTS, **TIGHT), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
            for _ in range(SLOT_STEPS):
                multi.step(As, Bs, As)
            ks = multi.stopped_at
            if ks[1] is None and ks[0] is not None and ks[2] is not None:
                break
        # slots 0 and 2 stopped with steps to spare, slot 1 is still running: the cases cannot pass vacuously
        assert ks[1] is None and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4, (rel, ks)
        _SLOTS.update(rel=rel, multi=multi, ks=ks, gens=gens, inputs=(As, Bs, As), one=(A, B, A))
    return _SLOTS


def test_a_stopped_slot_keeps_both_records_of_its_stop_step(vit):
    run = _slots_run(vit)
    multi, ks = run["multi"], run["ks"]
    for p in range(3):
        steps = SLOT_STEPS if ks[p] is None else ks[p] + 1
        single = SpliceEngine(dict(_cfg(lr=SLOT_LRS[p], **SLOTS, **TIGHT), stop_window=0), None, run["gens"][p], (64, 64), (64, 64), vit_engine=vit)
        for _ in range(steps):
            single.step(*run["one"])
        torch.cuda.synchronize()
        assert _same(multi.pair_params(p), single.pair_params()), (run["rel"], p)
        assert _same(multi.clip_dev[p:p + 1], single.clip_dev) and _same(multi.clip_auto_dev[p:p + 1], single.clip_auto_dev), (run["rel"], p)
        assert sum(multi.clip_auto_state(p)["count"]) == steps - 1                                # (step 0 lies before cls_warmup)
    assert multi.clip_state(1)["clipped"] >= 1


def test_stop_compact_carries_the_records(vit):
    run = _slots_run(vit)
    off, ks = run["multi"], run["ks"]
    on = MultiPairEngine(_cfg(stop_rel=run["rel"], stop_compact=True, **SLOTS, **TIGHT), None, run["gens"], (64, 64), (64, 64), vit_engine=vit,
                         pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
    for _ in range(SLOT_STEPS):
        on.step(*run["inputs"])
    torch.cuda.synchronize()
    assert on.live == [1] and sorted(on._parked) == [0, 2] and on.stopped_at == ks
    assert on.clip_state() == off.clip_state() and on.clip_auto_state() == off.clip_auto_state()
    for p in range(3):
        assert _same(on.pair_params(p), off.pair_params(p)), p
        assert on.clip_auto_state(p) == off.clip_auto_state(p) and _same(on.snapshot(p)["clip_auto"], off.snapshot(p)["clip_auto"]), p
    assert _same(on.clip_auto_dev, off.clip_auto_dev[1:2])


def test_a_snapshot_continues_in_an_engine_of_another_slot_count(vit):
    """5 steps of three pairs, slot 1's snapshot through the host into a one-pair engine, 6 more steps of both: slot 1 and the restored
    pair agree on every arena and both records.  A snapshot taken with the key off has no 'clip_auto'."""
    cfg = _cfg(**ONE, **_auto(1.0, 0.0, 2))
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    imgs = [_pair(71, p) for p in range(3)]
    As, Bs = torch.stack([a for a, _ in imgs]).contiguous(), torch.stack([b for _, b in imgs]).contiguous()
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit)
    for _ in range(5):
        multi.step(As, Bs, As)
    state = multi.snapshot(1, device="cpu")
    assert state["format"] == 1 and tuple(state["clip_auto"].shape) == (6,) and state["clip_auto"].dtype == torch.int32 and not state["clip_auto"].is_cuda
    single = SpliceEngine(cfg, None, gens[1], (64, 64), (64, 64), vit_engine=vit)
    single.restore([state])
    assert _same(single.clip_auto_dev, multi.clip_auto_dev[1:2]) and single.clip_auto_state()["count"] == [3, 1]
    for _ in range(6):
        multi.step(As, Bs, As)
        single.step(*imgs[1], imgs[1][0])
    torch.cuda.synchronize()
    for key in ("params", "m", "v"):
        assert _same(getattr(multi, key)[multi.stride:multi.stride + multi.gen.numel], getattr(single, key)[:single.gen.numel]), key
    assert _same(multi.clip_dev[1:2], single.clip_dev) and _same(multi.clip_auto_dev[1:2], single.clip_auto_dev)
    assert single.clip_state()["clipped"] >= 1 and single.clip_auto_state()["count"] == [8, 2]
    fixed = SpliceEngine(_cfg(**ONE, grad_clip_norm=1.0), None, gens[1], (64, 64), (64, 64), vit_engine=vit)
    fixed.step(*imgs[1], imgs[1][0])
    assert "clip" in fixed.snapshot(0) and "clip_auto" not in fixed.snapshot(0)
    with pytest.raises(ValueError, match="another 'grad_clip_auto'"):
        SpliceEngine(_cfg(**ONE, grad_clip_norm=1.0), None, gens[1], (64, 64), (64, 64), vit_engine=vit).restore([state])


def test_multiscale_engine_clips_in_its_own_update(vit):
    def run(rule, steps=6):
        eng = MultiScaleEngine(_cfg(cls_warmup=1, entire_A_every=2, **rule), None, synth.generator_params(84, 0.02), (64, 64), (64, 64), scales=(64, 96), vit_engine=vit)
        A, B = _pair(76)
        snaps = []
        for _ in range(steps):
            eng.step(A, B, A)
            snaps.append(dict(rec=None if eng.clip_dev is None else eng.clip_dev.clone(), auto=None if eng.clip_auto_dev is None else eng.clip_auto_dev.clone()))
        torch.cuda.synchronize()
        return eng, snaps
    off, _ = run({})
    huge, huge_snaps = run(_auto(HUGE))
    assert _same(huge.params, off.params) and _same(huge.engines[0].m, off.engines[0].m) and _same(huge.engines[0].v, off.engines[0].v)
    assert huge.clip_state()["clipped"] == 0 and huge.clip_auto_state()["count"] == [3, 2] and np.isfinite(huge.clip_auto_state()["thr"])
    with pytest.raises(RuntimeError, match="grad_clip_auto == 0"):
        off.clip_auto_state()
    tight, snaps = run(TIGHT)
    ref = _check_against_restatement(snaps, (1.0, 0.0, 1), 0.0, 1, 2, "scales")               # (regimes from the host step index: -1 0 1 0 1 0)
    assert clip_records(snaps[0]["rec"])[0]["sumsq"].tobytes() == clip_records(huge_snaps[0]["rec"])[0]["sumsq"].tobytes()
    assert ref.clipped >= 1 and not _same(tight.params, off.params) and tight.clip_auto_state()["regime"] == 0


def test_the_setter_refusals_and_one_rule_per_handle(vit):
    L = _lib.lib()
    eng = SpliceEngine(_cfg(), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    state, auto = _table(), _table()
    sp, ap = _lib.ptr(state), _lib.ptr(auto)
    for bad in (-1.0, float("nan"), float("inf")):
        assert L.splice_step_set_grad_clip_auto(eng.handle, bad, 2.0, 0.9, 4, sp, ap) != 0 and b"max_norm" in L.splice_last_error(), bad
    for k, beta, warmup in ((0.5, 0.9, 4), (float("nan"), 0.9, 4), (float("inf"), 0.9, 4), (2.0, 1.0, 4), (2.0, -0.5, 4), (2.0, 0.9, 0)):
        assert L.splice_step_set_grad_clip_auto(eng.handle, 0.0, k, beta, warmup, sp, ap) != 0 and b"finite k >= 1" in L.splice_last_error(), (k, beta, warmup)
    assert L.splice_step_set_grad_clip_auto(eng.handle, 0.0, 2.0, 0.9, 4, None, ap) != 0 and L.splice_step_set_grad_clip_auto(eng.handle, 0.0, 2.0, 0.9, 4, sp, None) != 0
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert L.splice_step_set_grad_clip_auto(eng.handle, 0.0, 2.0, 0.9, 4, sp, ap) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    A, B = _pair(62)
    eng.step(A, B)
    assert L.splice_step_set_grad_clip_auto(eng.handle, 0.0, 2.0, 0.9, 4, sp, ap) != 0 and b"before the first step" in L.splice_last_error()
    torch.cuda.synchronize()
    assert not state.any() and not auto.any()                     # never written
    on = SpliceEngine(_cfg(**_auto(2.0)), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"gradient clipping" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 3, None) != 0 and b"gradient clipping" in L.splice_last_error()
    assert L.splice_step_set_grad_clip(on.handle, 1.0, sp) != 0 and b"one of the two" in L.splice_last_error()
    fixed = SpliceEngine(_cfg(grad_clip_norm=1.0), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    assert L.splice_step_set_grad_clip_auto(fixed.handle, 0.0, 2.0, 0.9, 4, sp, ap) != 0 and b"one of the two" in L.splice_last_error()
    on.step(A, B)                                                 # (no entire-image branch on this handle: the rule runs there too)
    on.step(A, B)
    torch.cuda.synchronize()
    assert on.clip_auto_state()["regime"] == 0 and on.clip_auto_state()["count"] == [1, 0] and 0 < on.clip_auto_state()["ref"][0] < np.inf


TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, use_augmentations=False,
             global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0, cls_warmup=1, entire_A_every=5, n_epochs=8)


def _write_pair(root, name):   # (tests/test_ema_gpu.py::_write_pair)
    from PIL import Image
    A, B = synth.smooth_image_pair(60, 0, 72, 72)
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


def test_train_model_reports_the_rule_and_writes_the_two_columns(tmp_path):
    from splice_amd.batch import _write_result
    from splice_amd.train import clip_fields, train_model
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    torch.manual_seed(3)
    eng = train_model(_write_pair(tmp_path, "auto"), cfg_overrides=dict(TRAIN, loss_trace=True, **TIGHT), vit_state=vit_state, progress=False)
    torch.cuda.synchronize()
    _write_result(str(tmp_path), "auto", dict(steps=eng.step_idx + 1, **clip_fields(eng)))      # (as splice_amd.batch.train_runner)
    res = json.loads((tmp_path / "auto" / "out" / "result.json").read_text())
    state, auto = eng.clip_state(), eng.clip_auto_state()
    assert res == dict(steps=8, grad_clip_norm=0.0, grad_clip_auto=1.0, clip_ref=[float(x) for x in auto["ref"]], clipped_steps=state["clipped"], skipped_steps=0)
    assert auto["count"] == [6, 1] and res["clip_ref"][0] > 0 and res["clip_ref"][1] > 0
    with open(tmp_path / "auto" / "out" / "losses.csv") as f:
        rows = list(csv.DictReader(f))
    assert len(rows) == 8 and {"grad_norm", "clip_coef"} <= set(rows[0])
    assert F(rows[-1]["grad_norm"]) == state["norm"] and F(rows[-1]["clip_coef"]) == state["coef"]
    assert sum(F(r["clip_coef"]) < 1 for r in rows) == state["clipped"]
