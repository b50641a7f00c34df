"""GPU: keeping the best window's weights under the plateau stop rule.  The rule with its record and history
against the NumPy float32 restatement (engine.np_plateau); the update with its snapshot against splice_optim_step_pairs_clip on the
same inputs; then the engine: the best arena of a slot holds, bit for bit, the parameters (and the average) of the same pair's run
without the rule after exactly best_step + 1 steps -- one pair under graph replay and eager, beside neighbours, with an average and
clipping, with grouped plans, through train_model / train_pairs -- while the live arenas are what they are without the option.
Every comparison is exact."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import STOP_HISTORY, MultiPairEngine, MultiScaleEngine, SpliceEngine, np_plateau, stop_window_closes

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
HP = {0: (0.5, 0.99, 1e-8), 1: (0.99, 0.0, 1e-8), 2: (0.0, 0.0, 0.0)}   # Adam betas / RMSprop alpha / SGD
KINDS = [0, 1, 2]


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return _np(a).tobytes() == _np(b).tobytes()


# ------------------------------------------------------------------------------------------------------------ 1. the rule alone
def test_rule_alone_equals_numpy_restatement():
    """The three sequences of tests/test_stop_gpu.py::test_rule_alone_equals_numpy_restatement (falling then flat, flat, rising; some
    steps not counted) through splice_plateau_update_best: record and history equal the restatement, the state equals what
    splice_plateau_update gives."""
    steps, P, W, rel, patience, min_steps = 200, 3, 5, 0.01, 2, 40
    rng = np.random.default_rng(11)
    t = np.arange(steps, dtype=np.float64)
    seqs = np.stack([2.0 * np.exp(-t / 25.0) + 0.1 + 1e-4 * rng.standard_normal(steps),
                     1.0 + 1e-3 * rng.standard_normal(steps),
                     0.5 + 0.01 * t + 1e-3 * rng.standard_normal(steps)]).astype(np.float32)
    counted = [(k >= 3 and k % 7 != 0) for k in range(steps)]
    margins = []
    want = [np_plateau(seqs[p], counted, W, rel, patience, min_steps, margins) for p in range(P)]
    print("rule alone:", [(w["best_step"], w["best_window"], w["stop_step"], w["moves"]) for w in want], "min margin", min(margins))
    # the shape of the case first: slot 0's best moves often and lies before its stop, no comparison sits at its threshold
    assert want[0]["moves"] > 3 and 0 <= want[0]["best_step"] < want[0]["stop_step"] < steps - 1
    assert min(margins) > 1e-5, min(margins)
    assert (want[0]["moves"], want[0]["best_step"], want[0]["stop_step"]) == (28, 177, 188)   # (what the restatement gives for this input)
    for p in (1, 2):
        assert (want[p]["best_step"], want[p]["best_window"], want[p]["stop_step"]) == (8, 0, 43), (p, want[p])
    losses = torch.zeros(steps, P, 8)
    losses[:, :, 0] = torch.from_numpy(seqs.T.copy())
    losses[:, :, 1:] = 7.0
    losses = losses.to(DEV)

    def fresh():
        s = torch.zeros(P, 6, dtype=torch.int32, device=DEV)
        s[:, 5] = -1
        return s
    state, old = fresh(), fresh()
    best = torch.full((P, 2), -1, dtype=torch.int32, device=DEV)
    means = torch.zeros(P, STOP_HISTORY, device=DEV)
    L = _lib.lib()
    s = _lib.current_stream()
    for k in range(steps):
        _lib.check(L.splice_plateau_update_best(_lib.ptr(state), _lib.ptr(best), _lib.ptr(means), _lib.ptr(losses[k]), P, W, rel, patience, min_steps, k,
                                                int(counted[k]), s), "plateau_update_best")
        _lib.check(L.splice_plateau_update(_lib.ptr(old), _lib.ptr(losses[k]), P, W, rel, patience, min_steps, k, int(counted[k]), s), "plateau_update")
    torch.cuda.synchronize()
    got_best, got_means = _np(best), _np(means)
    for p in range(P):
        assert (got_best[p, 0], got_best[p, 1]) == (want[p]["best_step"], want[p]["best_window"]), (p, got_best[p], want[p])
        row = np.zeros(STOP_HISTORY, dtype=f32)
        row[:want[p]["means"].size] = want[p]["means"]
        assert 0 < want[p]["means"].size < STOP_HISTORY and got_means[p].tobytes() == row.tobytes(), p
        assert got_means[p, got_best[p, 1]].tobytes() == want[p]["means"][want[p]["best_window"]].tobytes()
    assert _same(state, old)
    got_i = _np(state)
    for p in range(P):
        assert (got_i[p, 5], got_i[p, 2], got_i[p, 4], got_i[p, 1]) == (want[p]["stop_step"], want[p]["windows"], want[p]["bad"], want[p]["count"]), p
        assert got_i.view(np.float32)[p, 3].tobytes() == want[p]["best"].tobytes()
    bad = L.splice_plateau_update_best(_lib.ptr(state), None, _lib.ptr(means), _lib.ptr(losses[0]), P, W, rel, patience, min_steps, 0, 1, s)
    assert bad != 0 and L.splice_plateau_update_best(_lib.ptr(state), _lib.ptr(best), None, _lib.ptr(losses[0]), P, W, rel, patience, min_steps, 0, 1, s) != 0


# ---------------------------------------------------------------------------------------------------------- 2. the update alone
def _dev(x, offset=0):
    """A device copy of ``x`` that starts ``offset`` floats into its allocation."""
    base = torch.zeros(x.numel() + offset, device=DEV)
    base[offset:] = x.reshape(-1).to(DEV)
    return base[offset:]


def _records(rows, dtype=torch.int32):
    return torch.tensor(rows, dtype=dtype).to(DEV)


def _clip_records(rows):
    """Hand-built splice_clip_state records from (coef, skip) rows."""
    raw = np.zeros((len(rows), 6), dtype=np.int32)
    raw.view(np.float32)[:, 2] = [c for c, _ in rows]
    raw[:, 3] = [k for _, k in rows]
    return torch.from_numpy(raw).to(DEV)


def _stop_records(stops):
    state = torch.zeros(len(stops), 6, dtype=torch.int32)
    state[:, 5] = torch.tensor(stops)
    return state.to(DEV)


def _sentinel(n):
    return -7.0 - torch.arange(n, dtype=torch.float32) % 13


def _update(export, kind, a, P, stride, n, lrs, step_dev, stop, zero_grad, ema, clip, best=None):
    L = _lib.lib()
    head = (kind, _lib.ptr(a["p"]), _lib.ptr(a["g"]), _lib.ptr(a["g2"]), _lib.ptr(a["m"]), _lib.ptr(a["v"]), _lib.ptr(a["e"]) if ema else None, P, stride, n,
            _lib.ptr(lrs), *HP[kind], _lib.ptr(step_dev), _lib.ptr(stop), zero_grad, 0.9, 1, _lib.ptr(clip))
    if export == "best":
        return L.splice_optim_step_pairs_best(*head, _lib.ptr(best), _lib.ptr(a["bp"]), _lib.ptr(a["be"]) if ema else None, _lib.current_stream())
    return L.splice_optim_step_pairs_clip(*head, _lib.current_stream())


def _arenas(P, stride, n, seed, offset=0):
    gen = torch.Generator().manual_seed(seed)
    tot = P * stride if P > 1 else n
    host = dict(p=torch.randn(tot, generator=gen), m=torch.randn(tot, generator=gen) * 0.1, v=torch.rand(tot, generator=gen) * 0.1,
                e=torch.randn(tot, generator=gen), g=torch.zeros(tot), g2=torch.zeros(tot))
    for s in range(P):   # (the padding between two arenas holds zero gradients)
        host["g"][s * stride: s * stride + n] = torch.randn(n, generator=gen)
        host["g2"][s * stride: s * stride + n] = torch.randn(n, generator=gen) * 0.3
    host["bp"], host["be"] = _sentinel(tot), _sentinel(tot) - 100
    return host, lambda: {k: _dev(x, offset) for k, x in host.items()}


@pytest.mark.parametrize("clip", [None, "scale", "skip"])
@pytest.mark.parametrize("ema", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_update_snapshots_the_taking_slot_alone(kind, ema, clip):
    """Three slots of 4099 floats at stride 4160 at step index 2: slot 0 takes (best_step 2), slot 1 does not (best_step 1), slot 2
    is frozen (stopped at 0; its record names step 2 all the same).  clip 'scale': coefficients 0.5 / 1 / 0.25; 'skip': slot 0's record has
    skip set -- it still takes, its unchanged p and e -- and the gradient is zeroed."""
    P, n, stride = 3, 4099, 4160
    host, dev = _arenas(P, stride, n, 300 + kind)
    lrs = torch.tensor([1e-3, 2e-3, 5e-4], device=DEV)
    step_dev = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    stop = _stop_records([-1, -1, 0])
    best = _records([[2, 0], [1, 0], [2, 0]])
    rows = {None: [(1.0, 0)] * 3, "scale": [(0.5, 0), (1.0, 0), (0.25, 0)], "skip": [(0.0, 1), (0.5, 0), (0.5, 0)]}[clip]
    zero_grad = int(clip == "skip")
    got, ref = dev(), dev()
    assert got["p"].data_ptr() % 16 == 0
    assert _update("best", kind, got, P, stride, n, lrs, step_dev, stop, zero_grad, ema, _clip_records(rows) if clip else None, best) == 0, _lib.lib().splice_last_error()
    assert _update("clip", kind, ref, P, stride, n, lrs, step_dev, stop, zero_grad, ema, _clip_records(rows)) == 0   # (coef 1 changes no bit)
    torch.cuda.synchronize()
    for key in ("p", "g", "m", "v") + (("e",) if ema else ()):
        assert _same(got[key], ref[key]), (kind, ema, clip, key)
    sl0, rest = slice(0, stride), slice(stride, P * stride)
    assert _same(got["bp"][sl0], got["p"][sl0])
    assert _same(got["bp"][rest], host["bp"][rest])                       # slots 1 and 2 keep the sentinel
    if ema:
        assert _same(got["be"][sl0], got["e"][sl0]) and _same(got["be"][rest], host["be"][rest])
    else:
        assert _same(got["e"], host["e"]) and _same(got["be"], host["be"])
    if clip == "skip":
        assert _same(got["p"][sl0], host["p"][sl0]) and _same(got["e"][sl0], host["e"][sl0]) and not got["g"][sl0].any()
        assert not _same(got["p"][stride:2 * stride], host["p"][stride:2 * stride])
    else:
        assert not _same(got["p"][sl0], host["p"][sl0])
        assert not ema or not _same(got["e"][sl0], host["e"][sl0])
    assert _same(got["p"][2 * stride:], host["p"][2 * stride:]) and _same(got["g"][2 * stride:], host["g"][2 * stride:])   # the frozen slot


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_update_of_a_single_arena(kind, offset):
    """One arena of 4099 floats (a float4 body and a tail of three), with an average and a coefficient of 0.5; offset 1: every arena 4
    bytes off its alignment, the whole walk on the scalar path.  The record is read once: taking, not taking, frozen."""
    n = 4099
    host, dev = _arenas(1, 0, n, 330 + kind, offset)
    lrs = torch.tensor([2e-3], device=DEV)
    step_dev = torch.full((1,), 3, dtype=torch.int32, device=DEV)
    clip = _clip_records([(0.5, 0)])
    ref = dev()
    assert ref["p"].data_ptr() % 16 == 4 * offset and ref["bp"].data_ptr() % 16 == 4 * offset
    assert _update("clip", kind, ref, 1, 0, n, lrs, step_dev, _stop_records([-1]), 0, True, clip) == 0
    for case, stop_at, best_step in (("takes", -1, 2), ("does not take", -1, 1), ("stops at this step", 2, 2), ("frozen", 1, 2)):
        got = dev()
        assert _update("best", kind, got, 1, 0, n, lrs, step_dev, _stop_records([stop_at]), 0, True, clip, _records([[best_step, 0]])) == 0
        torch.cuda.synchronize()
        for key in "pgmve":
            assert _same(got[key], host[key] if case == "frozen" else ref[key]), (case, key)
        if best_step == 2 and case != "frozen":
            assert _same(got["bp"], ref["p"]) and _same(got["be"], ref["e"]) and not _same(got["bp"], host["p"]), case
        else:
            assert _same(got["bp"], host["bp"]) and _same(got["be"], host["be"]), case


def test_update_refuses_incomplete_arguments():
    P, n, stride = 2, 1027, 1088
    host, dev = _arenas(P, stride, n, 7)
    a = dev()
    lrs, step_dev = torch.tensor([1e-3, 1e-3], device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    stop, best = _stop_records([-1, -1]), _records([[-1, -1]] * 2)
    L = _lib.lib()
    assert _update("best", 0, a, P, stride, n, lrs, step_dev, None, 0, True, None, best) != 0 and b"stop" in L.splice_last_error()
    assert _update("best", 0, a, P, stride, n, lrs, step_dev, stop, 0, True, None, None) != 0
    s = _lib.current_stream()
    head = lambda e: (0, _lib.ptr(a["p"]), _lib.ptr(a["g"]), None, _lib.ptr(a["m"]), _lib.ptr(a["v"]), e, P, stride, n, _lib.ptr(lrs), *HP[0], _lib.ptr(step_dev),
                      _lib.ptr(stop), 0, 0.9, 1, None, _lib.ptr(best))
    assert L.splice_optim_step_pairs_best(*head(None), None, None, s) != 0                                    # no best arena
    assert L.splice_optim_step_pairs_best(*head(_lib.ptr(a["e"])), _lib.ptr(a["bp"]), None, s) != 0 and b"average" in L.splice_last_error()
    assert L.splice_optim_step_pairs_best(*head(None), _lib.ptr(a["bp"]), _lib.ptr(a["be"]), s) != 0 and b"average" in L.splice_last_error()
    assert L.splice_optim_step_pairs_best(*head(None), _lib.ptr(a["bp"]), None, s) == 0                        # neither clip nor ema: fine
    torch.cuda.synchronize()
    assert _same(a["bp"], host["bp"])                                                                          # (records at -1: nothing taken)


# --------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):   # (tests/test_stop_gpu.py::_cfg)
    from splice_amd.engine import DEFAULT_CFG
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed, pair=0):
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _live(eng, pair=0):
    n, st = eng.gen.numel, eng.stride
    sl = slice(pair * st, pair * st + n)
    out = dict(params=eng.params[sl].clone(), m=eng.m[sl].clone(), v=eng.v[sl].clone(), running=eng.running[pair].clone())
    if eng.ema is not None:
        out["ema"] = eng.ema[sl].clone()
    return out


def _counted(eng, steps):
    return [stop_window_closes(k, 1, eng.cfg["cls_warmup"], eng.cfg["entire_A_every"] if eng.plan_e is not None else 0) for k in range(steps)]


def _run(eng, steps, step_fn, snap=False):
    """`steps` steps; the [steps][P] float32 losses and, with `snap`, every slot's live arenas after every step."""
    hist, snaps = [], []
    for k in range(steps):
        step_fn(eng)
        hist.append(eng.losses_dev[:, 0].clone())
        if snap:
            snaps.append([_live(eng, p) for p in range(eng.P)])
    torch.cuda.synchronize()
    return torch.stack(hist).cpu().numpy(), snaps


def _want(cfg, losses, counted):
    return np_plateau(losses, counted, cfg["stop_window"], cfg["stop_rel"], cfg["stop_patience"], cfg["stop_min_steps"])


def _check_records(eng, pair, want):
    state, means = eng.best_state(pair) if eng.P > 1 else eng.best_state(), eng.window_means(pair) if eng.P > 1 else eng.window_means()
    assert state["best_step"] == (want["best_step"] if want["best_step"] >= 0 else None) and state["best_window"] == want["best_window"], (pair, state, want)
    assert means.dtype == np.float32 and means.tobytes() == want["means"].tobytes(), (pair, means, want["means"])
    if want["best_window"] >= 0:
        assert f32(state["best_mean"]).tobytes() == want["means"][want["best_window"]].tobytes()
    else:
        assert state["best_mean"] is None


# 3. one pair: entire-image steps 0, 4, 8; counted steps 1 2 3 | 5 6 7: the first window sets best at step 3, the second does not halve
# it and the run stops at step 7 (tests/test_stop_gpu.py::ONE)
ONE = dict(cls_warmup=1, entire_A_every=4, stop_window=3, stop_patience=1, stop_rel=0.5)
ONE_STEPS = 12
_ONE = {}


def _one_pair(vit, steps=ONE_STEPS, graph=True, snap=False, **over):
    key = (steps, graph, snap, tuple(sorted(over.items())))
    if key not in _ONE:
        eng = SpliceEngine(_cfg(**dict(ONE, **over)), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
        if not graph:
            _lib.check(_lib.lib().splice_step_use_graph(eng.handle, 0), "use_graph")
        A, B = _pair(62)
        init = eng.params.clone()
        losses, snaps = _run(eng, steps, lambda e: e.step(A, B, A), snap)
        _ONE[key] = (eng, losses[:, 0], snaps, init)
    return _ONE[key]


@pytest.mark.parametrize("graph", [True, False])
def test_one_pair_keeps_the_weights_of_its_best_window(vit, graph):
    eng, losses, _, init = _one_pair(vit, graph=graph, stop_keep_best=True)
    if graph:
        stats = (C.c_longlong * 3)()
        _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
        assert stats[0] + stats[2] >= 2                                # graphs were in use (ordinary and entire-image variant)
    assert eng.stopped_at == 7 and eng.best_state()["best_step"] == 3
    _check_records(eng, 0, _want(eng.cfg, losses, _counted(eng, ONE_STEPS)))
    _, _, short, _ = _one_pair(vit, steps=4, snap=True, stop_window=0)  # the rule off: the parameters after exactly 4 steps
    assert _same(eng.pair_best(), short[3][0]["params"])
    assert not _same(eng.pair_best(), eng.pair_params()) and not _same(eng.pair_best(), init)
    off, off_losses, _, _ = _one_pair(vit, graph=graph)                 # the rule on, the option off: the live arenas and the losses
    assert off.best is None and off.stopped_at == 7
    with pytest.raises(RuntimeError, match="stop_keep_best"):
        off.pair_best()
    with pytest.raises(RuntimeError, match="stop_keep_best"):
        off.best_state()
    for key, val in _live(off).items():
        assert _same(_live(eng)[key], val), key
    assert off_losses.tobytes() == losses.tobytes()
    with pytest.raises(RuntimeError, match="ema_decay"):
        eng.pair_best(ema=True)


def test_before_a_window_closes_best_is_the_initial_weights(vit):
    eng, _, _, init = _one_pair(vit, steps=3, stop_keep_best=True)      # steps 0 1 2: the first window closes at step 3
    assert eng.best_state() == dict(best_step=None, best_window=-1, best_mean=None) and eng.window_means().size == 0
    assert _same(eng.pair_best(), init) and not _same(eng.pair_params(), init)


# 4. three slots (tests/test_stop_gpu.py::SLOTS): slot 0 cannot improve (lr 0), slot 1 learns, slot 2 hardly moves
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_WINDOWS = (4, 3)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 18


def test_best_moves_late_beside_neighbours(vit):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    singles = []
    for p, lr in enumerate(SLOT_LRS):
        single = SpliceEngine(dict(_cfg(lr=lr, **SLOTS), stop_window=0), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        slosses, snaps = _run(single, SLOT_STEPS, lambda e: e.step(A, B, A), True)
        singles.append((slosses[:, 0], [s[0]["params"] for s in snaps]))
    counted = _counted(single, SLOT_STEPS)

    def last_close(w):   # the step that closed the slot's last live window
        return max(k for k in range(SLOT_STEPS) if stop_window_closes(k, w["window"], 1, 7) and (w["stop_step"] < 0 or k <= w["stop_step"]))

    def choose():
        for window in SLOT_WINDOWS:
            for rel in SLOT_RELS:
                cfg = _cfg(stop_window=window, stop_rel=rel, stop_keep_best=True, **SLOTS)
                wants = [dict(_want(cfg, losses, counted), window=window) for losses, _ in singles]
                if wants[1]["best_window"] >= 1 and any(0 <= w["best_step"] < last_close(w) for w in wants):
                    return cfg, wants
        return cfg, wants
    cfg, wants = choose()
    print("slots:", cfg["stop_window"], cfg["stop_rel"], [(w["best_step"], w["best_window"], w["stop_step"]) for w in wants])
    # the learning slot's best moved behind its first window, and some slot's best is not its last window: nothing passes vacuously
    assert wants[1]["best_window"] >= 1 and any(0 <= w["best_step"] < last_close(w) for w in wants), wants
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
    mlosses, _ = _run(multi, SLOT_STEPS, lambda e: e.step(As, Bs, As))
    states = multi.best_state()
    for p, (slosses, snaps) in enumerate(singles):
        assert states[p]["best_step"] == wants[p]["best_step"] >= 0, (p, states[p], wants[p])
        assert _same(multi.pair_best(p), snaps[states[p]["best_step"]]), p           # its own single run after best_step + 1 steps
        _check_records(multi, p, _want(cfg, mlosses[:, p], counted))                 # (the records follow the losses the engine itself reported)
        assert multi.best_state(p) == states[p]
    assert not _same(multi.pair_best(1), multi.pair_params(1))


# 5. with an average and a clipping threshold every step reaches
def test_best_average_under_clipping(vit):
    extra = dict(ema_decay=0.5, ema_start=3, grad_clip_norm=1e-4)
    eng, losses, _, init = _one_pair(vit, stop_keep_best=True, **extra)
    ruled, ruled_losses, _, _ = _one_pair(vit, **extra)                               # the rule on, the option off
    _, off_losses, off_snaps, _ = _one_pair(vit, snap=True, stop_window=0, **extra)
    want = _want(eng.cfg, off_losses, _counted(eng, ONE_STEPS))
    k = want["best_step"]
    print("average under clipping:", k, want["stop_step"], eng.clip_state())
    assert 0 <= k < ONE_STEPS - 1                                                     # a window closed, and steps followed it
    rec = eng.clip_state()
    ran = ONE_STEPS if eng.stopped_at is None else eng.stopped_at + 1
    assert rec["clipped"] == ran and rec["skipped"] == 0                               # every step the slot ran was clipped
    assert eng.best_state()["best_step"] == k and eng.stopped_at == (want["stop_step"] if want["stop_step"] >= 0 else None)
    assert _same(eng.pair_best(ema=True), off_snaps[k][0]["ema"]) and _same(eng.pair_best(), off_snaps[k][0]["params"])
    assert not _same(eng.pair_best(ema=True), eng.pair_best()) and not _same(eng.pair_best(ema=True), eng.pair_ema())
    for key, val in _live(ruled).items():
        assert _same(_live(eng)[key], val), key
    assert ruled_losses.tobytes() == losses.tobytes() and _same(ruled.clip_dev, eng.clip_dev)
    A, _ = _pair(62)
    assert torch.equal(eng.generate(A[None], best=True, ema=True), eng.generate(A[None].clone(), best=True, ema=True))
    assert not torch.equal(eng.generate(A[None], best=True, ema=True), eng.generate(A[None], best=True))
    sd = eng.state_dict(best=True, ema=True)
    assert _same(eng.gen.flatten({n: t for n, t in sd.items() if n in eng.gen.table}), eng.pair_best(ema=True))
    assert all(torch.equal(sd[n], eng.state_dict()[n]) for n in eng.gen.buffer_table)  # the live buffers


# 6. two pairs with two crops each (grouped plans; tests/test_stop_gpu.py::CROPS)
CROPS = dict(cls_warmup=1, entire_A_every=5, stop_window=3, stop_patience=1)
CROPS_RELS = (0.05, 0.1, 0.02, 0.2, 0.01, 0.3)
CROPS_MAX = 30


def test_pairs_with_crops_frozen_best_survives(vit):
    gens = [synth.generator_params(80, 0.02), synth.generator_params(81, 0.1)]
    imgs = [_pair(82, p) for p in range(2)]

    def crops(img):
        return torch.stack([img, img.flip(-1)]).contiguous()
    A_all = torch.cat([crops(a) for a, _ in imgs]).contiguous()
    B_all = torch.cat([crops(b) for _, b in imgs]).contiguous()
    E_all = torch.stack([a for a, _ in imgs]).contiguous()
    step = lambda e: e.step(A_all, B_all, E_all)
    off = MultiPairEngine(_cfg(**dict(CROPS, stop_window=0)), None, gens, (64, 64), (64, 64), vit_engine=vit, n_crops=2)
    off_losses, off_snaps = _run(off, CROPS_MAX, step, True)           # (a pair's bits do not depend on its neighbour: tests/test_pairs_crops_gpu.py)
    counted = _counted(off, CROPS_MAX)
    for rel in CROPS_RELS:
        cfg = _cfg(stop_rel=rel, stop_keep_best=True, **CROPS)
        wants = [_want(cfg, off_losses[:, p], counted) for p in range(2)]
        stops = sorted(w["stop_step"] for w in wants if w["stop_step"] >= 0)
        if stops and wants[0]["stop_step"] != wants[1]["stop_step"]:
            break
    assert stops and wants[0]["stop_step"] != wants[1]["stop_step"], (rel, wants)     # one pair stops while the other still runs
    first = [w["stop_step"] for w in wants].index(stops[0])
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, n_crops=2)
    _run(multi, stops[0] + 1, step)
    assert multi.stopped_at[first] == stops[0] and multi.stopped_at[1 - first] is None
    k = multi.best_state(first)["best_step"]
    assert k == wants[first]["best_step"] and 0 <= k < stops[0]                          # (patience 1: the best window is the one before the stop)
    frozen_best = multi.pair_best(first).clone()
    assert _same(frozen_best, off_snaps[k][first]["params"])
    mlosses, _ = _run(multi, 3, step)                                                    # three steps more: the other pair is still running
    assert multi.step_idx == stops[0] + 3 and _same(multi.pair_best(first), frozen_best)
    assert multi.best_state(first)["best_step"] == k
    other = 1 - first
    want_other = _want(cfg, off_losses[:stops[0] + 4, other], counted[:stops[0] + 4])
    _check_records(multi, other, want_other)
    assert _same(multi.pair_best(other), off_snaps[want_other["best_step"]][other]["params"])
    assert _same(multi.pair_params(other), off_snaps[stops[0] + 3][other]["params"])


# 7. train_model and train_pairs (tests/test_stop_gpu.py::TRAIN, TRAIN_STOP)
TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, use_augmentations=False,
             global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0, cls_warmup=1, entire_A_every=5)
TRAIN_STOP = dict(stop_window=3, stop_patience=1, stop_rel=0.5)   # counted steps 1 2 3 | 4 6 7: stops at step 7


def _write_pair(root, name):
    from PIL import Image
    A, B = synth.smooth_image_pair(60, 0, 72, 72)
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


def test_train_model_and_train_pairs_write_the_best_image(tmp_path, monkeypatch):
    from splice_amd.generator import GeneratorPlan
    from splice_amd.train import best_fields, train_model, train_pairs
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    seen = []
    plain_step = MultiPairEngine.step

    def recording_step(self, *args, **kw):   # the per-step losses, for the restatement
        out = plain_step(self, *args, **kw)
        seen.append(out[:, 0].clone())
        return out
    monkeypatch.setattr(MultiPairEngine, "step", recording_step)
    over = dict(TRAIN, n_epochs=60, stop_keep_best=True, **TRAIN_STOP)
    images = []
    eng = train_model(_write_pair(tmp_path, "on"), callback=lambda im: images.append(1), cfg_overrides=over, vit_state=vit_state, progress=False)
    losses = torch.stack(seen).cpu().numpy()[:, 0]
    want = _want(eng.cfg, losses, _counted(eng, len(losses)))
    assert eng.stopped_at == 7 == want["stop_step"] and len(images) == 3               # the logged images and the callback stay as they are
    for name in ("output.png", "output_best.png"):
        assert (tmp_path / "on" / "out" / name).exists(), name
    assert not (tmp_path / "on" / "out" / "output_best_ema.png").exists()
    _check_records(eng, 0, want)
    fields = json.loads(json.dumps(best_fields(eng)))
    assert fields["best_step"] == want["best_step"] == 3 and fields["window_means"] == [float(x) for x in want["means"]]
    assert fields["best_window_mean"] == float(want["means"][want["best_window"]])
    A = torch.rand(1, 3, 72, 72, generator=torch.Generator().manual_seed(1)).to(DEV)
    plain = GeneratorPlan(eng.gen, 1, A.shape[2], A.shape[3], False).forward(eng.pair_best().clone(), A)
    assert torch.equal(eng.generate(A, best=True), plain) and not torch.equal(eng.generate(A), plain)
    del seen[:]
    roots = [_write_pair(tmp_path, f"p{i}") for i in range(2)]
    both = train_pairs(roots, cfg_overrides=dict(over, ema_decay=0.5), vit_state=vit_state, progress=False)
    mlosses = torch.stack(seen).cpu().numpy()
    for p in range(2):
        _check_records(both, p, _want(both.cfg, mlosses[:, p], _counted(both, len(mlosses))))
        assert both.best_state(p)["best_step"] == 3 and best_fields(both, p)["best_step"] == 3
        assert _same(both.pair_best(p), eng.pair_best())                                # the same pair, the same seed: the same weights
        for name in ("output.png", "output_best.png", "output_ema.png", "output_best_ema.png"):
            assert (tmp_path / f"p{p}" / "out" / name).exists(), (p, name)
    assert best_fields(SpliceEngine(_cfg(), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=both.vit)) == {}


# 8. refusals
def test_keep_best_is_refused_where_it_cannot_hold(vit):
    L = _lib.lib()
    gen = synth.generator_params(61, 0.02)
    A, B = _pair(62)

    def arenas(eng):
        return (eng.params.clone(), torch.full((1, 2), -1, dtype=torch.int32, device=DEV), torch.zeros(1, STOP_HISTORY, device=DEV))

    def keep(eng, bp, be, rec, means):
        return L.splice_step_set_keep_best(eng.handle, _lib.ptr(bp), _lib.ptr(be), _lib.ptr(rec), _lib.ptr(means))
    plain = SpliceEngine(_cfg(), None, gen, (64, 64), None, vit_engine=vit)                       # no stop rule
    bp, rec, means = arenas(plain)
    assert keep(plain, bp, None, rec, means) != 0 and b"stop rule" in L.splice_last_error()
    assert L.splice_step_set_mode(plain.handle, 1, 0) == 0                                          # gradient-only mode
    assert keep(plain, bp, None, rec, means) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(plain.handle, 0, 0) == 0 and L.splice_step_set_phases(plain.handle, 3, None) == 0   # phase mode
    assert keep(plain, bp, None, rec, means) != 0 and b"phase mode" in L.splice_last_error()
    ruled = SpliceEngine(_cfg(**ONE), None, gen, (64, 64), (64, 64), vit_engine=vit)               # a stop rule, no average
    bp, rec, means = arenas(ruled)
    assert keep(ruled, None, None, rec, means) != 0 and keep(ruled, bp, None, None, means) != 0 and keep(ruled, bp, None, rec, None) != 0
    assert keep(ruled, bp, bp.clone(), rec, means) != 0 and b"best_ema" in L.splice_last_error()  # superfluous
    assert keep(ruled, bp, None, rec, means) == 0
    assert L.splice_step_set_mode(ruled.handle, 1, 0) != 0 and L.splice_step_set_phases(ruled.handle, 3, None) != 0   # ... which these modes refuse in turn
    assert L.splice_step_set_stop_rule(ruled.handle, 0, 0.5, 1, 0) != 0 and b"best weights" in L.splice_last_error()
    averaged = SpliceEngine(_cfg(**ONE, ema_decay=0.5), None, gen, (64, 64), (64, 64), vit_engine=vit)
    bp, rec, means = arenas(averaged)
    assert keep(averaged, bp, None, rec, means) != 0 and b"best_ema" in L.splice_last_error()     # missing
    averaged.step(A, B, A)
    assert keep(averaged, bp, bp.clone(), rec, means) != 0 and b"before the first step" in L.splice_last_error()
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError, match="stop_keep_best"):
        MultiScaleEngine(_cfg(stop_keep_best=True, **ONE), None, gen, (64, 64), (64, 64), scales=(64, 96), vit_engine=vit)
    with pytest.raises(ValueError, match="'stop_keep_best' needs"):
        SpliceEngine(_cfg(stop_keep_best=True), None, gen, (64, 64), None, vit_engine=vit)
