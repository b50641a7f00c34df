"""GPU: the plateau lr rule.  The two rules alone against the NumPy float32 restatement (engine.np_lr_plateau); then
the engine: its record follows its own losses, a run with the rule equals a run without it that is handed fl(lr * scale) before every
step, a rule that never cuts changes no bit, a slot equals its single run -- beside neighbours, with n_crops > 1, under graph replay, in a
sweep, behind a stop -- and train_model writes the effective lr.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import DEFAULT_CFG, STOP_HISTORY, MultiPairEngine, SpliceEngine, np_lr_plateau, np_plateau, stop_window_closes
from splice_amd.util import LrSchedule

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


# ----------------------------------------------------------------------------------------------------------- the rule alone
def sequences():
    """The three 200-step sequences and the mask of counted steps of tests/test_stop_gpu.py::test_rule_alone_equals_numpy_restatement."""
    steps = 200
    rng = np.random.default_rng(11)
    t = np.arange(steps, dtype=np.float64)
    seqs = np.stack([2.0 * np.exp(-t / 25.0) + 0.1 + 1e-4 * rng.standard_normal(steps),
                     1.0 + 1e-3 * rng.standard_normal(steps),
                     0.5 + 0.01 * t + 1e-3 * rng.standard_normal(steps)]).astype(np.float32)
    return seqs, [(k >= 3 and k % 7 != 0) for k in range(steps)]


# (W, rel, stop_patience, min_steps, factor, lr_patience, min_scale): the slots stop and their lr records then stay; a reset by better windows
# in the falling sequence and the floor after four cuts in the flat and rising ones; the rising sequence hits the cap of 64 cuts
PARAMS = [(5, 0.01, 2, 40, 0.5, 2, 0.1), (5, 0.01, 1000, 0, 0.5, 2, 0.1), (1, 0.01, 1000, 0, 0.9, 1, 0.0)]


def _fresh_records(P):
    state = torch.zeros(P, 6, dtype=torch.int32, device=DEV)
    state[:, 5] = -1
    lr_state = torch.tensor([[int(f32(1).view(np.int32)), 0, 0, -1]] * P, dtype=torch.int32, device=DEV)
    cuts = torch.full((P, STOP_HISTORY), -1, dtype=torch.int32, device=DEV)
    return state, lr_state, cuts


@pytest.mark.parametrize("per_pair", [False, True])
@pytest.mark.parametrize("params", PARAMS)
def test_rules_alone_equal_numpy_restatement(params, per_pair):
    W, rel, patience, min_steps, factor, lr_patience, min_scale = params
    seqs, counted = sequences()
    steps, P = seqs.shape[1], seqs.shape[0]
    margins = []
    want = [np_lr_plateau(seqs[p], counted, *params, margins=margins) for p in range(P)]
    assert margins and min(margins) > 1e-5, min(margins)    # no comparison sits at its threshold: rounding cannot decide a case
    if params == PARAMS[0]:
        assert all(0 <= w["stop_step"] < steps - 10 for w in want) and want[1]["lr"]["cuts"] == 3
    if params == PARAMS[1]:
        assert want[0]["lr"]["cut_steps"][0] > 100 and all(w["lr"]["cuts"] == 4 and w["lr"]["scale"] == f32(0.1) for w in want[1:])
    if params == PARAMS[2]:
        assert want[2]["lr"]["cuts"] == STOP_HISTORY and want[2]["windows"] > STOP_HISTORY + 1
    lr_host = np.array([2e-3, 0.7, 1e-6], dtype=f32) if per_pair else np.array([2e-3], dtype=f32)
    losses = torch.zeros(steps, P, 8)
    losses[:, :, 0] = torch.from_numpy(seqs.T.copy())
    losses[:, :, 1:] = 7.0                                   # (only element 0 of a row is the loss)
    losses = losses.to(DEV)
    lr_in = torch.from_numpy(lr_host).to(DEV)
    lr_eff = torch.full((steps, P), float("nan"), device=DEV)
    state, lr_state, cuts = _fresh_records(P)
    old = state.clone()
    L, s = _lib.lib(), _lib.current_stream()
    for k in range(steps):
        _lib.check(L.splice_plateau_update_lr(_lib.ptr(state), _lib.ptr(lr_state), _lib.ptr(cuts), _lib.ptr(losses[k]), _lib.ptr(lr_in), int(per_pair),
                                              _lib.ptr(lr_eff[k]), P, W, rel, patience, min_steps, factor, lr_patience, min_scale, k, int(counted[k]), s),
                   "plateau_update_lr")
        _lib.check(L.splice_plateau_update(_lib.ptr(old), _lib.ptr(losses[k]), P, W, rel, patience, min_steps, k, int(counted[k]), s), "plateau_update")
    torch.cuda.synchronize()
    assert torch.equal(state, old)                           # the stop records: bit for bit those of the stop rule alone
    got_i, got_lr, got_cuts, got_eff = state.cpu().numpy(), lr_state.cpu().numpy(), cuts.cpu().numpy(), lr_eff.cpu().numpy()
    for p in range(P):
        w = want[p]
        assert (got_i[p, 5], got_i[p, 2], got_i[p, 4], got_i[p, 1]) == (w["stop_step"], w["windows"], w["bad"], w["count"]), (p, got_i[p], w)
        assert got_i[p, 3:4].view(f32).tobytes() == w["best"].tobytes() and got_i[p, 0:1].view(f32).tobytes() == w["sum"].tobytes()
        lr = w["lr"]
        assert got_lr[p, 0:1].view(f32).tobytes() == lr["scale"].tobytes(), (p, got_lr[p], lr)
        assert tuple(got_lr[p, 1:]) == (lr["bad"], lr["cuts"], lr["last_cut_step"]), (p, got_lr[p], lr)
        assert got_cuts[p].tolist() == lr["cut_steps"] + [-1] * (STOP_HISTORY - lr["cuts"]), (p, got_cuts[p], lr)
        eff = (lr_host[p if per_pair else 0] * w["scales"]).astype(f32)   # one fp32 multiply with the scale in force at the step
        assert got_eff[:, p].tobytes() == eff.tobytes(), (p, np.nonzero(got_eff[:, p] != eff))


def test_rules_alone_refuse_bad_arguments():
    P = 2
    state, lr_state, cuts = _fresh_records(P)
    losses, lr_in, lr_eff = torch.ones(P, 8, device=DEV), torch.ones(P, device=DEV), torch.zeros(P, device=DEV)
    L, s = _lib.lib(), _lib.current_stream()
    good = dict(state=state, lr_state=lr_state, cuts=cuts, losses=losses, lr_in=lr_in, lr_eff=lr_eff, pairs=P, window=3, rel=0.01, patience=2, min_steps=0,
                factor=0.5, lr_patience=1, min_scale=0.1, step_idx=0)

    def call(**over):
        a = dict(good, **over)
        return L.splice_plateau_update_lr(_lib.ptr(a["state"]), _lib.ptr(a["lr_state"]), _lib.ptr(a["cuts"]), _lib.ptr(a["losses"]), _lib.ptr(a["lr_in"]), 1,
                                          _lib.ptr(a["lr_eff"]), a["pairs"], a["window"], a["rel"], a["patience"], a["min_steps"], a["factor"], a["lr_patience"],
                                          a["min_scale"], a["step_idx"], 0, s)
    for over in (dict(factor=0.0), dict(factor=1.0), dict(factor=-0.5), dict(factor=float("nan")), dict(lr_patience=0), dict(min_scale=1.0),
                 dict(min_scale=-0.1), dict(window=0), dict(rel=1.5), dict(patience=0), dict(pairs=0), dict(step_idx=-1), dict(state=None),
                 dict(lr_state=None), dict(cuts=None), dict(losses=None), dict(lr_in=None), dict(lr_eff=None)):
        assert call(**over) != 0, over
    torch.cuda.synchronize()
    fresh = _fresh_records(P)
    assert torch.equal(state, fresh[0]) and torch.equal(lr_state, fresh[1]) and torch.equal(cuts, fresh[2]) and not lr_eff.any()   # nothing ran
    assert call() == 0
    torch.cuda.synchronize()
    assert torch.equal(lr_eff, lr_in) and torch.equal(lr_state, fresh[1])   # an uncounted step: lr_eff alone is written


# --------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed, pair=0):
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _arenas(eng, pair=0):
    n, st = eng.gen.numel, eng.stride
    sl = slice(pair * st, pair * st + n)
    out = dict(params=eng.params[sl].clone(), m=eng.m[sl].clone(), v=eng.v[sl].clone(), running=eng.running[pair].clone(),
               tracked=int(eng.state_dict(pair)["1.0.2.num_batches_tracked"]))
    for name in ("ema", "best", "best_ema"):
        if getattr(eng, name, None) is not None:
            out[name] = getattr(eng, name)[sl].clone()
    for name in ("clip_dev", "best_dev", "means_dev"):
        if getattr(eng, name, None) is not None:
            out[name] = getattr(eng, name)[pair].clone()
    if eng.trace_dev is not None:
        out["trace"] = eng.trace_dev[:, pair].clone().view(torch.int32)   # (bits: unwritten rows are NaN)
    return out


def _same(a, b, what=()):
    assert set(a) == set(b), (what, sorted(a), sorted(b))
    for k in a:
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, what + (k,)


def _counted(eng, steps):
    return [stop_window_closes(k, 1, eng.cfg["cls_warmup"], eng.cfg["entire_A_every"] if eng.plan_e is not None else 0) for k in range(steps)]


def _run(eng, steps, step_fn, before=None):
    """`steps` steps; returns the [steps, P] float32 totals.  `before(eng, k)` runs in front of step k."""
    hist = []
    for k in range(steps):
        if before is not None:
            before(eng, k)
        step_fn(eng)
        hist.append(eng.losses_dev[:, 0].clone())
    torch.cuda.synchronize()
    return torch.stack(hist).cpu().numpy()


def _want(cfg, losses, counted):
    return np_lr_plateau(losses, counted, cfg["stop_window"], cfg["stop_rel"], cfg["stop_patience"], cfg["stop_min_steps"], cfg["lr_plateau_factor"],
                         cfg["lr_plateau_patience"], cfg["lr_plateau_min_scale"])


def _check_lr(got, want):
    lr = want["lr"]
    assert f32(got["scale"]).tobytes() == lr["scale"].tobytes(), (got, lr)
    assert (got["bad"], got["cuts"], got["last_cut_step"], got["cut_steps"]) == (lr["bad"], lr["cuts"], lr["last_cut_step"], lr["cut_steps"]), (got, lr)


def _check_stop(state, want):
    assert state["stopped_at"] == (want["stop_step"] if want["stop_step"] >= 0 else None), (state, want)
    assert (state["windows"], state["bad"]) == (want["windows"], want["bad"]) and f32(state["best"]).tobytes() == want["best"].tobytes(), (state, want)


def _graph_stats(eng):
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    return list(stats)


def test_setter_is_refused_where_it_must_be(vit):
    L = _lib.lib()
    _, lr_state, cuts = _fresh_records(1)
    eng = SpliceEngine(_cfg(), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    set_rule = lambda factor=0.5, patience=1, min_scale=0.0, state=lr_state, rows=cuts: L.splice_step_set_lr_plateau(eng.handle, factor, patience, min_scale,
                                                                                                                     _lib.ptr(state), _lib.ptr(rows))
    assert set_rule() != 0 and b"stop rule" in L.splice_last_error()               # needs the windows of the stop rule
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert set_rule() != 0 and b"gradient-only" in L.splice_last_error()           # the whole-step guard of every rule setter
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    assert L.splice_step_set_stop_rule(eng.handle, 3, 0.5, 1000, 0) == 0
    for bad in (dict(factor=0.0), dict(factor=1.0), dict(factor=float("nan")), dict(patience=0), dict(min_scale=1.0), dict(min_scale=-0.5), dict(state=None),
                dict(rows=None)):
        assert set_rule(**bad) != 0, bad
    assert set_rule() == 0
    assert L.splice_step_set_stop_rule(eng.handle, 0, 0.5, 1, 0) != 0 and b"plateau lr rule" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 1, 0) != 0                           # (a handle with the stop rule runs whole steps)
    A, B = _pair(62)
    eng.step(A, B)
    assert set_rule() != 0 and b"before the first step" in L.splice_last_error()
    torch.cuda.synchronize()
    assert lr_state.cpu().tolist() == [[int(f32(1).view(np.int32)), 0, 0, -1]] and (cuts == -1).all()


# test 2: entire-image steps 0, 4, 8, ...; the windows are the counted steps 4w + 1 .. 4w + 3.  No window beats 0.1 x the first: window 0 is
# better, the windows 2, 4, 6 cut at the steps 11, 19, 27
ONE = dict(stop_window=3, stop_rel=0.9, stop_patience=1000, cls_warmup=1, entire_A_every=4, lr_plateau_factor=0.5, lr_plateau_patience=2)
ONE_STEPS = 30
OPTIMS = {"adam": dict(optimizer="adam"), "rmsprop_cosine": dict(optimizer="rmsprop", scheduler_policy="cosine", n_epochs=ONE_STEPS), "sgd": dict(optimizer="sgd")}


class _FedSchedule:
    """What the engine asks for the lr of a step; any policy but "none" makes it hand that lr over through splice_step_set_lr."""
    policy = "fed"

    def __init__(self, lrs):
        self.lrs = lrs

    def lr(self, k):
        return self.lrs[k]


def _one_pair(vit, cfg, steps, graph=True, fed=None):
    eng = SpliceEngine(cfg, None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    if not graph:
        _lib.check(_lib.lib().splice_step_use_graph(eng.handle, 0), "use_graph")
    if fed is not None:
        eng.schedule = _FedSchedule(fed)
    A, B = _pair(62)
    return eng, _run(eng, steps, lambda e: e.step(A, B, A))[:, 0]


@pytest.mark.parametrize("optim", sorted(OPTIMS))
def test_one_pair_equals_the_run_that_is_fed_the_scaled_lr(optim, vit):
    cfg = _cfg(**ONE, **OPTIMS[optim])
    eng, losses = _one_pair(vit, cfg, ONE_STEPS)
    want = _want(cfg, losses, _counted(eng, ONE_STEPS))
    print(optim, "cuts", want["lr"]["cut_steps"], "scale", want["lr"]["scale"])
    assert want["lr"]["cuts"] >= 2 and want["lr"]["cut_steps"][:2] == [11, 19], want["lr"]
    _check_lr(eng.lr_state(), want)
    _check_stop(eng.stop_state()[0], want)
    assert eng.lr_scale == float(want["lr"]["scale"]) and eng.lr_state(0) == eng.lr_state()
    sch = LrSchedule(cfg)
    lrs = [sch.lr(k) for k in range(ONE_STEPS)]
    assert eng.lr == lrs[-1]                                            # engine.lr stays the scheduled lr
    fed = [float(f32(lr) * scale) for lr, scale in zip(lrs, want["scales"])]   # fl(lr_k * scale_k), the multiply the loss kernel makes
    off, off_losses = _one_pair(vit, dict(cfg, lr_plateau_factor=0.0), ONE_STEPS, fed=fed)
    with pytest.raises(RuntimeError, match="lr_plateau_factor"):
        off.lr_state()
    assert off.lr_scale == 1.0
    assert off_losses.tobytes() == losses.tobytes()
    _same(_arenas(eng), _arenas(off), (optim,))
    plain, plain_losses = _one_pair(vit, dict(cfg, lr_plateau_factor=0.0), 14)          # what the cuts changed: from step 12 on
    assert plain_losses[:13].tobytes() == losses[:13].tobytes() and plain_losses[13] != losses[13]


# test 3
EXTRAS = {"plain": {}, "all_rules": dict(ema_decay=0.9, ema_start=2, stop_keep_best=True, grad_clip_norm=5.0, loss_trace=True, n_epochs=16)}
NOCUT = dict(stop_window=3, stop_rel=0.05, stop_patience=2, cls_warmup=1, entire_A_every=5)
NOCUT_STEPS = 14


@pytest.mark.parametrize("extras", sorted(EXTRAS))
@pytest.mark.parametrize("P", [1, 2])
def test_a_rule_that_never_cuts_changes_no_bit(P, extras, vit):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(P)]
    pairs = [_pair(71, p) for p in range(P)]
    As, Bs = torch.stack([a for a, _ in pairs]).contiguous(), torch.stack([b for _, b in pairs]).contiguous()
    runs = []
    for keys in ({}, dict(lr_plateau_factor=0.5, lr_plateau_patience=10 ** 6, lr_plateau_min_scale=0.25)):
        eng = MultiPairEngine(_cfg(**NOCUT, **EXTRAS[extras], **keys), None, gens, (64, 64), (64, 64), vit_engine=vit)
        losses = _run(eng, NOCUT_STEPS, lambda e: e.step(As, Bs, As))
        runs.append((eng, losses, eng.stop_state()))
    (off, off_losses, off_stop), (on, on_losses, on_stop) = runs
    assert on_losses.tobytes() == off_losses.tobytes() and on_stop == off_stop
    for p in range(P):
        _same(_arenas(on, p), _arenas(off, p), (P, extras, p))
        rec = on.lr_state(p)
        assert rec["cuts"] == 0 and rec["scale"] == 1 and rec["cut_steps"] == [] and rec["last_cut_step"] == -1
        assert rec["bad"] == np_plateau(on_losses[:, p], _counted(on, NOCUT_STEPS), 3, 0.05, 10 ** 6, 0)["bad"]   # (counted, never spent; while the slot is live)
    assert on.lr_scale == [1.0] * P and _graph_stats(on)[0] + _graph_stats(on)[2] >= 2


# test 4
SLOTS = dict(stop_window=3, stop_rel=0.9, stop_patience=1000, cls_warmup=1, entire_A_every=5, lr_plateau_factor=0.5, lr_plateau_patience=1, lr_plateau_min_scale=0.2)
SLOT_STEPS = 16   # windows close at the steps 3, 7, 11, 14: cuts at 7, 11 and (to the floor) 14


@pytest.mark.parametrize("n_crops", [1, 2])
def test_slots_equal_their_single_runs(n_crops, vit):
    P = 3
    cfg = _cfg(**SLOTS)
    gens = [synth.generator_params(80 + p, 0.02 if p != 1 else 0.1) for p in range(P)]
    imgs = [_pair(82, p) for p in range(P)]

    def crops(img):
        return img[None].contiguous() if n_crops == 1 else torch.stack([img, img.flip(-1)]).contiguous()
    Ac, Bc = [crops(a) for a, _ in imgs], [crops(b) for _, b in imgs]
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, n_crops=n_crops)
    A_all, B_all, E_all = torch.cat(Ac).contiguous(), torch.cat(Bc).contiguous(), torch.stack([a for a, _ in imgs]).contiguous()
    mlosses = _run(multi, SLOT_STEPS, lambda e: e.step(A_all, B_all, E_all))
    states = multi.lr_state()
    for p in range(P):
        single = SpliceEngine(cfg, None, gens[p], (64, 64), (64, 64), vit_engine=vit, n_crops=n_crops)
        slosses = _run(single, SLOT_STEPS, lambda e: e.step(Ac[p], Bc[p], imgs[p][0]))[:, 0]
        assert mlosses[:, p].tobytes() == slosses.tobytes(), p
        _same(_arenas(multi, p), _arenas(single), (n_crops, p))
        assert states[p] == single.lr_state() == multi.lr_state(p)
        want = _want(cfg, slosses, _counted(single, SLOT_STEPS))
        _check_lr(states[p], want)
        assert want["lr"]["cut_steps"] == [7, 11, 14] and want["lr"]["scale"] == f32(0.2)
    assert multi.lr_scale == [float(f32(0.2))] * P


# test 5
def test_graph_replay_equals_eager(vit):
    """The replaying run captures its graphs at the third step: the cuts at the steps 11, 19 and 27 happen inside replayed graphs, and the
    replay of step 12 already runs with the halved lr -- as the eager run, which reads the same table."""
    cfg = _cfg(**ONE)
    eng, losses = _one_pair(vit, cfg, ONE_STEPS)
    stats = _graph_stats(eng)
    assert stats[0] + stats[2] >= 2                                     # graphs were in use (ordinary and entire-image variant)
    eager, eager_losses = _one_pair(vit, cfg, ONE_STEPS, graph=False)
    assert _graph_stats(eager) == [0, 0, 0]
    assert eager_losses.tobytes() == losses.tobytes()
    assert eager.lr_state() == eng.lr_state() and eager.stop_state() == eng.stop_state() and eng.lr_state()["cut_steps"] == [11, 19, 27]
    _same(_arenas(eager), _arenas(eng))
    fed = [float(f32(cfg["lr"]) * (f32(0.5) if k > 11 else f32(1))) for k in range(14)]
    off, off_losses = _one_pair(vit, dict(cfg, lr_plateau_factor=0.0), 14, fed=fed)
    assert off_losses.tobytes() == losses[:14].tobytes()                # the cut of step 11 acts from step 12 on, inside the replayed graph


# test 6
SWEEP_LRS = [0.0, 2e-3, 1e-3]


def test_a_sweep_with_per_slot_lr(vit):
    cfg = _cfg(**dict(SLOTS, lr_plateau_min_scale=0.0))
    gens = [synth.generator_params(90, 0.02)] * 3
    A, B = _pair(91)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in SWEEP_LRS])
    mlosses = _run(multi, SLOT_STEPS, lambda e: e.step(As, Bs, As))
    assert multi.lr == SWEEP_LRS                                        # (the scheduled lrs; the scales ride beside them)
    for p, lr in enumerate(SWEEP_LRS):
        single = SpliceEngine(dict(cfg, lr=lr), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        slosses = _run(single, SLOT_STEPS, lambda e: e.step(A, B, A))[:, 0]
        assert mlosses[:, p].tobytes() == slosses.tobytes(), p
        _same(_arenas(multi, p), _arenas(single), ("sweep", p))
        assert multi.lr_state(p) == single.lr_state() and single.lr_state()["cuts"] == 3
    assert not torch.equal(multi.pair_params(1), multi.pair_params(2))


# test 7: stop_patience 2 -- window 0 is better, the windows 1 and 2 are not: the slot stops at the close of window 2 (step 11) with the cut of
# that very step in its record, and stays there
STOPPING = dict(ONE, stop_patience=2, lr_plateau_patience=1)


def test_a_stopped_slot_keeps_its_record_and_its_arenas(vit):
    cfg = _cfg(**STOPPING)
    eng, losses = _one_pair(vit, cfg, 24)
    want = _want(cfg, losses, _counted(eng, 24))
    assert want["stop_step"] == 11 and eng.stopped_at == 11 and want["lr"]["cut_steps"] == [7, 11]
    _check_lr(eng.lr_state(), want)                                     # twelve frozen steps, three closed windows: nothing moved
    _check_stop(eng.stop_state()[0], want)
    short, short_losses = _one_pair(vit, cfg, 12)
    assert short_losses.tobytes() == losses[:12].tobytes() and short.lr_state() == eng.lr_state()
    _same(_arenas(eng), _arenas(short))
    # test_stop_gpu's claim: the arenas of the same pair run for exactly k + 1 steps without the stop -- here with the lr the rule gave it
    fed = [float(f32(cfg["lr"]) * want["scales"][k]) for k in range(12)]
    free, _ = _one_pair(vit, dict(cfg, stop_window=0, lr_plateau_factor=0.0), 12, fed=fed)
    got, ref = _arenas(eng), _arenas(free)
    for k in ("params", "m", "v", "running"):
        assert torch.equal(got[k], ref[k]), k


# test 8
TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=8, use_augmentations=False, global_A_crops_min_cover=1.0,
             global_B_crops_min_cover=1.0, cls_warmup=1, entire_A_every=5, stop_window=3, stop_rel=0.9, stop_patience=1000, lr_plateau_factor=0.5,
             lr_plateau_patience=1, lr_plateau_min_scale=0.2, loss_trace=True, scheduler_policy="cosine", n_epochs=16)


def test_train_model_writes_the_effective_lr(tmp_path):
    from PIL import Image
    from splice_amd.train import lr_fields, train_model
    A, B = synth.smooth_image_pair(60, 0, 72, 72)       # square: the full-cover crop has no position draw, the run is deterministic
    for side, img in (("A", A), ("B", B)):
        d = tmp_path / "pair" / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    eng = train_model(str(tmp_path / "pair"), cfg_overrides=dict(TRAIN), vit_state=synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05), progress=False)
    assert eng.step_idx == 15
    fields = lr_fields(eng)
    assert fields == {"lr_plateau_factor": 0.5, "lr_cuts": 3, "lr_cut_steps": [7, 11, 14], "lr_scale": float(f32(0.2))}
    lines = open(tmp_path / "pair" / "out" / "losses.csv").read().split("\n")[1:-1]
    assert len(lines) == 16
    sch = LrSchedule(dict(DEFAULT_CFG, **TRAIN))
    scales = [1.0] * 8 + [0.5] * 4 + [0.25] * 3 + [0.2]
    want = np.array([f32(sch.lr(k)) * f32(s) for k, s in enumerate(scales)], dtype=f32)
    got = np.array([float(ln.split(",")[1]) for ln in lines]).astype(f32)
    assert got.tobytes() == want.tobytes(), (got, want)
    trace = eng.loss_trace()
    _check_lr(eng.lr_state(), _want(eng.cfg, trace[:, 0], _counted(eng, 16)))
