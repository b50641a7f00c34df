"""GPU: the plateau stop rule.  The rule alone against its NumPy float32 restatement; then the engine: a slot
that stopped at step k holds, bit for bit and however many steps follow, the parameters, optimiser moments and BatchNorm buffers
of the same pair run for exactly k + 1 steps with the rule off -- alone, beside running neighbours, with n_crops > 1, under graph
replay -- and train_model / train_pairs end early.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import MultiPairEngine, SpliceEngine, stop_window_closes

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32


# ------------------------------------------------------------------------------------------------- the rule, restated in NumPy
def np_rule(losses, counted, window, rel, patience, min_steps, margins=None):
    """The specification, one float32 rounding per operation.  Returns the state after the last step; ``margins`` collects
    |mean - threshold| / |threshold| of every comparison made."""
    s = dict(sum=f32(0), count=0, windows=0, best=f32(0), bad=0, stop_step=-1)
    for t, (loss, c) in enumerate(zip(losses, counted)):
        if not c:
            continue
        s["sum"] = f32(s["sum"] + f32(loss))
        s["count"] += 1
        if s["count"] < window:
            continue
        mean = f32(s["sum"] / f32(window))
        if s["windows"] == 0:
            s["best"], s["bad"] = mean, 0
        else:
            thr = f32(s["best"] * f32(f32(1.0) - f32(rel)))
            if margins is not None:
                margins.append(abs(float(mean) - float(thr)) / abs(float(thr)))
            if mean < thr:
                s["best"], s["bad"] = mean, 0
            else:
                s["bad"] += 1
        s["windows"] += 1
        s["sum"], s["count"] = f32(0), 0
        if s["bad"] >= patience and t >= min_steps and s["stop_step"] < 0:
            s["stop_step"] = t
    return s


def test_rule_alone_equals_numpy_restatement():
    """splice_plateau_update over 200 steps of 3 slots (falling then flat, flat, rising), some steps not counted."""
    steps, P, W, rel, patience, min_steps = 200, 3, 5, 0.01, 2, 40
    rng = np.random.default_rng(11)
    t = np.arange(steps, dtype=np.float64)
    seqs = np.stack([2.0 * np.exp(-t / 25.0) + 0.1 + 1e-4 * rng.standard_normal(steps),      # falls, then flat: stops late
                     1.0 + 1e-3 * rng.standard_normal(steps),                               # flat: held back by min_steps only
                     0.5 + 0.01 * t + 1e-3 * rng.standard_normal(steps)]).astype(np.float32)  # rising
    counted = [(k >= 3 and k % 7 != 0) for k in range(steps)]          # 169 counted steps: the run ends inside a window
    margins = []
    want = [np_rule(seqs[p], counted, W, rel, patience, min_steps, margins) for p in range(P)]
    assert margins and min(margins) > 1e-5, min(margins)    # no comparison sits at its threshold: rounding cannot decide a case
    assert 40 < want[0]["stop_step"] < steps - 1 and want[1]["stop_step"] >= min_steps and want[2]["stop_step"] >= min_steps
    assert want[0]["stop_step"] != want[1]["stop_step"]
    assert all(w["count"] == 4 and w["sum"] > 0 for w in want)
    losses = torch.zeros(steps, P, 8)
    losses[:, :, 0] = torch.from_numpy(seqs.T.copy())
    losses[:, :, 1:] = 7.0                                   # (only element 0 of a row is the loss)
    losses = losses.to(DEV)
    state = torch.zeros(P, 6, dtype=torch.int32, device=DEV)
    state[:, 5] = -1
    L = _lib.lib()
    for k in range(steps):
        _lib.check(L.splice_plateau_update(_lib.ptr(state), _lib.ptr(losses[k]), P, W, rel, patience, min_steps, k, int(counted[k]), _lib.current_stream()),
                   "plateau_update")
    torch.cuda.synchronize()
    got_i = state.cpu().numpy()
    got_f = got_i.view(np.float32)
    for p in range(P):
        assert (got_i[p, 5], got_i[p, 2], got_i[p, 4], got_i[p, 1]) == (want[p]["stop_step"], want[p]["windows"], want[p]["bad"], want[p]["count"]), (p, got_i[p], want[p])
        assert got_f[p, 3].tobytes() == want[p]["best"].tobytes() and got_f[p, 0].tobytes() == want[p]["sum"].tobytes(), (p, got_f[p], want[p])
    assert L.splice_plateau_update(_lib.ptr(state), _lib.ptr(losses[0]), P, W, 1.5, patience, min_steps, 0, 1, _lib.current_stream()) != 0   # rel outside (0, 1)


# --------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):   # (tests/test_facade_gpu.py::_cfg)
    from splice_amd.engine import DEFAULT_CFG
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed, pair=0):
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _arenas(eng, pair=0):
    n, st = eng.gen.numel, eng.stride
    sl = slice(pair * st, pair * st + n)
    return dict(params=eng.params[sl].clone(), m=eng.m[sl].clone(), v=eng.v[sl].clone(), running=eng.running[pair].clone(),
                tracked=int(eng.state_dict(pair)["1.0.2.num_batches_tracked"]))


def _same(a, b, what=()):
    for k in a:
        same = torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k]
        assert same, what + (k,)


def _counted(eng, steps):
    return [stop_window_closes(k, 1, eng.cfg["cls_warmup"], eng.cfg["entire_A_every"] if eng.plan_e is not None else 0) for k in range(steps)]


def _run(eng, steps, step_fn, snap_closes=None):
    """`steps` steps; returns the [steps] float32 losses of every slot and, with `snap_closes` = a window length, the arenas of
    slot 0 after every step that closes such a window (the steps a rule with that window can stop at)."""
    hist, snaps = [], {}
    for k in range(steps):
        step_fn(eng)
        hist.append(eng.losses_dev[:, 0].clone())
        if snap_closes and stop_window_closes(k, snap_closes, eng.cfg["cls_warmup"], eng.cfg["entire_A_every"] if eng.plan_e is not None else 0):
            snaps[k] = _arenas(eng)
    torch.cuda.synchronize()
    return torch.stack(hist).cpu().numpy(), snaps


def _want(eng_cfg, losses, counted):
    return np_rule(losses, counted, eng_cfg["stop_window"], eng_cfg["stop_rel"], eng_cfg["stop_patience"], eng_cfg["stop_min_steps"])


def _check_state(state, want):
    assert state["stopped_at"] == (want["stop_step"] if want["stop_step"] >= 0 else None), (state, want)
    assert (state["windows"], state["bad"]) == (want["windows"], want["bad"]) and f32(state["best"]).tobytes() == want["best"].tobytes(), (state, want)


# case 2 / 5: entire-image steps 0, 4, 8; counted steps 1 2 3 | 5 6 7: the second window closes at step 7
ONE = dict(cls_warmup=1, entire_A_every=4, stop_window=3, stop_patience=1, stop_rel=0.5)
ONE_STEPS = 12


def _one_pair(vit, on, steps, graph=True, snap=False):
    cfg = _cfg(**ONE) if on else _cfg(**dict(ONE, stop_window=0))
    eng = SpliceEngine(cfg, None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    if not graph:
        _lib.check(_lib.lib().splice_step_use_graph(eng.handle, 0), "use_graph")
    A, B = _pair(62)
    losses, snaps = _run(eng, steps, lambda e: e.step(A, B, A), ONE["stop_window"] if snap else None)
    return eng, losses[:, 0], snaps


@pytest.fixture(scope="module")
def one_on(vit):
    return _one_pair(vit, True, ONE_STEPS)


def test_one_pair_rule_changes_nothing_until_it_fires(vit, one_on):
    eng, losses, _ = one_on
    state = eng.stop_state()[0]
    k = state["stopped_at"]
    assert k == 7 and eng.stopped_at == 7 and eng.all_stopped()        # the loss did not halve between the two windows
    _check_state(state, _want(eng.cfg, losses, _counted(eng, ONE_STEPS)))
    off, off_losses, snaps = _one_pair(vit, False, ONE_STEPS, snap=True)
    assert off.stopped_at is None and not off.all_stopped() and not off.window_closes(7) and eng.window_closes(7)
    assert off_losses[:k + 1].tobytes() == losses[:k + 1].tobytes()    # per-step losses bit-equal up to and including the stop step
    short, _, _ = _one_pair(vit, False, k + 1)
    got = _arenas(eng)
    _same(got, _arenas(short), ("k+1 steps",))
    _same(got, snaps[k], ("snapshot",))
    full = _arenas(off)
    assert not torch.equal(got["params"], full["params"]) and not torch.equal(got["v"], full["v"]) and not torch.equal(got["running"], full["running"])
    assert got["tracked"] == 2 * (k + 1) + 2 and full["tracked"] == 2 * ONE_STEPS + 3


def test_graph_replay_equals_eager(vit, one_on):
    """The fixture's run replays captured graphs from its third step on (the stop at step 7 and the frozen steps behind it are
    replays); the same run launched eagerly stops at the same step with the same state and arenas."""
    eng, losses, _ = one_on
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    assert stats[0] + stats[2] >= 2                                     # graphs were in use (ordinary and entire-image variant)
    eager, eager_losses, _ = _one_pair(vit, True, ONE_STEPS, graph=False)
    assert eager.stop_state() == eng.stop_state() and eager.stopped_at == 7
    assert eager_losses[:8].tobytes() == losses[:8].tobytes()
    _same(_arenas(eager), _arenas(eng))


def test_rule_is_set_before_the_first_step_only(vit):
    eng = SpliceEngine(_cfg(), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    L = _lib.lib()
    assert L.splice_step_set_stop_rule(eng.handle, 3, 0.0, 1, 0) != 0 and L.splice_step_set_stop_rule(eng.handle, 3, 0.5, 0, 0) != 0
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert L.splice_step_set_stop_rule(eng.handle, 3, 0.5, 1, 0) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    A, B = _pair(62)
    eng.step(A, B)
    assert L.splice_step_set_stop_rule(eng.handle, 3, 0.5, 1, 0) != 0 and b"before the first step" in L.splice_last_error()
    assert eng.stop_state() == [dict(stopped_at=None, windows=0, best=0.0, bad=0)]


# case 3: slots 0 and 2 cannot improve by stop_rel and stop at the close of their third window (the first sets `best`, two more do
# not beat it); slot 1 learns.  How far a window of lr = 1e-6 steps moves the loss depends on the optimiser (RMSprop's first
# updates are lr * g / sqrt(0.01 g^2) = 10 lr per element, Adam's bias-corrected ones lr), so stop_rel is the first of
# SLOT_RELS that this slot's own single run does not reach while slot 1's does: the NumPy rule's verdicts on the three
# single runs choose it (and, should no stop_rel do at windows of 4, windows of 3), and the test then demands them of the engine.
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_WINDOWS = (4, 3)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 18   # windows of 4: counted steps 1 2 3 4 | 5 6 8 9 | 10 11 12 13, slot 0 stops at step 13; steps 14 (an entire-image step) .. 17 find it frozen


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
def test_slots_stop_alone_and_leave_neighbours_untouched(optimizer, vit):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    singles = []
    for p, lr in enumerate(SLOT_LRS):
        single = SpliceEngine(dict(_cfg(optimizer=optimizer, lr=lr, **SLOTS), stop_window=0), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        slosses, snaps = _run(single, SLOT_STEPS, lambda e: e.step(A, B, A), 1)   # (arenas after every counted step)
        singles.append((slosses[:, 0], snaps, _arenas(single)))
    counted = _counted(single, SLOT_STEPS)
    def verdicts():
        for window in SLOT_WINDOWS:
            for rel in SLOT_RELS:
                cfg = _cfg(optimizer=optimizer, stop_window=window, stop_rel=rel, **SLOTS)
                wants = [_want(cfg, losses, counted) for losses, _, _ in singles]   # the rule on every slot's OWN single-run losses
                ks = [w["stop_step"] for w in wants]
                if ks[1] == -1 and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4:
                    return cfg, rel, wants, ks
        return cfg, rel, wants, ks
    cfg, rel, wants, ks = verdicts()
    # slots 0 and 2 stop with steps to spare, slot 1 is still running at the end: the case cannot pass vacuously
    assert ks[1] == -1 and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4, (optimizer, cfg["stop_window"], rel, wants)
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
    mlosses, _ = _run(multi, SLOT_STEPS, lambda e: e.step(As, Bs, As))
    states = multi.stop_state()
    for p, (slosses, snaps, full) in enumerate(singles):
        k = ks[p]
        if p == 1:
            assert mlosses[:, p].tobytes() == slosses.tobytes()
            ref = full
        else:
            assert mlosses[:k + 1, p].tobytes() == slosses[:k + 1].tobytes()
            ref = snaps[k]                                  # the single run truncated at k + 1 steps
            # what the freeze kept out: these arrays move although the loss hardly does
            assert not torch.equal(full["running"], ref["running"]) and not torch.equal(full["v"], ref["v"])
        assert states[p]["stopped_at"] == (k if k >= 0 else None), (optimizer, rel, p, states[p], wants[p])
        _check_state(states[p], _want(cfg, mlosses[:, p], counted))   # (the state follows the losses the engine itself reported)
        _same(_arenas(multi, p), ref, (optimizer, rel, p))
    assert multi.stopped_at[1] is None and not multi.all_stopped()


# case 4: two pairs with two crops each (grouped plans).  There are no per-slot settings here, so which pair stops first is the
# rule's verdict on each pair's own single run: the test takes the first stop_rel of CROPS_RELS under which the NumPy rule stops
# one pair while the other still runs
CROPS = dict(cls_warmup=1, entire_A_every=5, stop_window=3, stop_patience=1)
CROPS_RELS = (0.05, 0.1, 0.02, 0.2, 0.01, 0.3)
CROPS_MAX = 30


def test_pairs_with_crops_one_frozen_one_running(vit):
    cfg = _cfg(**CROPS)
    gens = [synth.generator_params(80, 0.02), synth.generator_params(81, 0.1)]
    imgs = [_pair(82, p) for p in range(2)]

    def crops(img):   # two crops per image, as [2,3,64,64] (the second one mirrored)
        return torch.stack([img, img.flip(-1)]).contiguous()
    Ac, Bc = [crops(a) for a, _ in imgs], [crops(b) for _, b in imgs]
    singles = []
    for p in range(2):
        single = SpliceEngine(dict(cfg, stop_window=0), None, gens[p], (64, 64), (64, 64), vit_engine=vit, n_crops=2)
        slosses, snaps = _run(single, CROPS_MAX, lambda e: e.step(Ac[p], Bc[p], imgs[p][0]), CROPS["stop_window"])
        singles.append((slosses[:, 0], snaps))
    counted = _counted(single, CROPS_MAX)
    for rel in CROPS_RELS:
        cfg = _cfg(stop_rel=rel, **CROPS)
        wants = [_want(cfg, losses, counted)["stop_step"] for losses, _ in singles]
        stops = sorted(k for k in wants if k >= 0)
        if stops and wants[0] != wants[1]:
            break
    assert stops and wants[0] != wants[1], (rel, wants)   # one pair stops while the other still runs
    steps = stops[0] + 3                                    # (windows close at least 3 steps apart: the other pair is still running)
    first = wants.index(stops[0])
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, n_crops=2)
    A_all, B_all, E_all = torch.cat(Ac).contiguous(), torch.cat(Bc).contiguous(), torch.stack([a for a, _ in imgs]).contiguous()
    mlosses, _ = _run(multi, steps, lambda e: e.step(A_all, B_all, E_all))
    assert multi.stopped_at == [stops[0] if p == first else None for p in range(2)]
    _same(_arenas(multi, first), singles[first][1][stops[0]], ("frozen",))
    other = 1 - first
    ref = SpliceEngine(dict(cfg, stop_window=0), None, gens[other], (64, 64), (64, 64), vit_engine=vit, n_crops=2)
    rlosses, _ = _run(ref, steps, lambda e: e.step(Ac[other], Bc[other], imgs[other][0]))
    assert mlosses[:, other].tobytes() == rlosses[:, 0].tobytes()
    _same(_arenas(multi, other), _arenas(ref), ("running",))
    assert not torch.equal(multi.running[first], multi.running[other])


# case 6
TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, use_augmentations=False,
             global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0, cls_warmup=1, entire_A_every=5)
TRAIN_STOP = dict(stop_window=3, stop_patience=1, stop_rel=0.5)   # counted steps 1 2 3 | 4 6 7: stops at step 7


def _write_pair(root, name):
    from PIL import Image
    A, B = synth.smooth_image_pair(60, 0, 72, 72)       # square: the full-cover crop has no position draw, the run is deterministic
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


def test_train_model_and_train_pairs_end_early(tmp_path):
    from splice_amd.train import train_model, train_pairs
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    seen = []
    eng = train_model(_write_pair(tmp_path, "on"), callback=lambda im: seen.append(tuple(im.shape)), cfg_overrides=dict(TRAIN, n_epochs=60, **TRAIN_STOP),
                      vit_state=vit_state, progress=False)
    k = eng.stopped_at
    assert k == 7 and eng.step_idx == k                     # the loop ended at the poll of the stopping step
    assert (tmp_path / "on" / "out" / "output.png").exists()
    assert seen == [(3, 72, 72)] * 3                        # epochs 4 and 8, and the final image
    off = train_model(_write_pair(tmp_path, "off"), cfg_overrides=dict(TRAIN, n_epochs=k + 1), vit_state=vit_state, progress=False)
    assert off.stopped_at is None and off.step_idx == k
    want = _arenas(off)
    _same(_arenas(eng), want, ("train_model",))
    roots = [_write_pair(tmp_path, f"p{i}") for i in range(2)]
    images = []
    both = train_pairs(roots, callback=lambda p, im: images.append(p), cfg_overrides=dict(TRAIN, n_epochs=60, **TRAIN_STOP), vit_state=vit_state, progress=False)
    assert both.stopped_at == [k, k] and both.step_idx == k and images == [0, 1] * 3
    for p in range(2):
        _same(_arenas(both, p), want, ("train_pairs", p))
        assert (tmp_path / f"p{p}" / "out" / "output.png").exists()
