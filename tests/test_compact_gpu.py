"""GPU: slots that have stopped leave the launches (``stop_compact``), and a run continues from its checkpoint.
The same engine runs with the key off and on: while a slot is live its losses are equal after every step, and at the end every
external slot answers alike -- arenas, buffers, records, window means, trace, ``state_dict`` and generated images -- while
``engine.live`` shrinks at exactly the steps the slots stop at.  ``train_pairs`` writes the same files either way, and ``train_model``
interrupted behind a checkpoint and resumed writes those of the run left alone.  Every comparison is exact."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import DEFAULT_CFG, MultiPairEngine, SpliceEngine, np_plateau, snapshot_cfg_mismatch, stop_window_closes

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed, pair=0):
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _bits(a, b):
    if torch.is_tensor(a):
        a, b = a.detach().cpu().numpy(), b.detach().cpu().numpy()
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _graphs(eng):
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    return stats[0] + stats[2]


# what a slot's snapshot holds that a frozen slot of an engine that parks nothing keeps computing from frozen weights: its reported
# losses and, from them, the open window and the counts of its stop record.  Everything else is compared.
FROZEN_NOISE = ("losses", "stop")


def _same_slots(on, off, A, stops, steps, what=()):
    """Every per-slot answer of the compacted engine ``on`` against the engine ``off`` that parked nothing, for every external slot."""
    slots = off.P
    assert on.P_in == slots and on.step_idx == off.step_idx == steps - 1 and on.generator_calls == off.generator_calls, what
    assert on.stopped_at == off.stopped_at == [k if k >= 0 else None for k in stops] and on.all_stopped() == off.all_stopped(), what + (on.stopped_at, stops)
    assert on.lr == off.lr and on.lr_scale == off.lr_scale, what
    got_states, want_states = on.stop_state(), off.stop_state()
    for p in range(slots):
        w = what + (p,)
        frozen = stops[p] >= 0
        a, b = on.snapshot(p, device="cpu"), off.snapshot(p, device="cpu")
        assert sorted(a) == sorted(b), w
        for k in a:
            if frozen and k in FROZEN_NOISE:
                continue
            if k == "cfg":   # (the two engines differ in stop_compact, which binds no state)
                assert snapshot_cfg_mismatch(a[k], b[k]) is None, w
                continue
            assert _bits(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], w + (k,)
        assert a["stop"][5] == b["stop"][5] == stops[p], w
        if not frozen:
            assert got_states[p] == want_states[p] and on.losses(p) == off.losses(p), w
        for name in ("pair_params", "pair_ema", "pair_best"):
            assert _bits(getattr(on, name)(p), getattr(off, name)(p)), w + (name,)
        assert _bits(on.pair_best(p, ema=True), off.pair_best(p, ema=True)), w
        assert on.best_state(p) == off.best_state(p) and _bits(on.window_means(p), off.window_means(p)), w
        assert on.clip_state(p) == off.clip_state(p) and _bits(on.loss_trace(p), off.loss_trace(p)), w
        if on.lr_state_dev is not None:
            assert on.lr_state(p) == off.lr_state(p), w
        for kind in (dict(), dict(ema=True), dict(best=True), dict(best=True, ema=True)):
            sa, sb = on.state_dict(p, **kind), off.state_dict(p, **kind)
            assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), w + (kind,)
            assert torch.equal(on.generate(A, p, **kind), off.generate(A, p, **kind)), w + (kind,)
    for (ra, la, aa), (rb, lb, ab) in zip(on.loss_trace_columns(), off.loss_trace_columns()):
        assert _bits(ra, rb) and la == lb and aa == ab, what


def _run_both(off, on, steps, inputs, stops):
    """``steps`` steps of both engines on the same inputs; after every step the live list is the slots that have not stopped by then
    (while one of them runs), the returned tensor has a row per live slot and every live slot's losses are equal."""
    slots, seen = off.P, []
    for k in range(steps):
        off.step(*inputs)
        out = on.step(*inputs)
        running = [p for p in range(slots) if stops[p] < 0 or stops[p] > k]
        want = running if running else seen[-1]           # (when the last slots stop nothing is rebuilt: the run is over)
        assert on.live == want and tuple(out.shape) == (len(want), 8) and out is on.losses_dev, (k, on.live, want)
        for p in on.live:
            assert on.losses(p) == off.losses(p), (k, p)
        seen.append(list(on.live))
    assert off.live == list(range(slots)) and not off._parked
    return seen


EXTRA = dict(stop_keep_best=True, ema_decay=0.9, ema_start=2, loss_trace=True, grad_clip_norm=1e-3)

# ------------------------------------------------------------------------------------------------- three slots, two of them stop
# the set-up of tests/test_stop_gpu.py::test_slots_stop_alone_and_leave_neighbours_untouched: slots 0 and 2 cannot improve by stop_rel,
# slot 1 learns; stop_rel and the window are the first of the lists under which the NumPy rule, on each slot's own single run, says so
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_WINDOWS = (4, 3)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 22


def _counted(eng, steps):
    return [stop_window_closes(k, 1, eng.cfg["cls_warmup"], eng.cfg["entire_A_every"] if eng.plan_e is not None else 0) for k in range(steps)]


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop"])
def test_stopped_slots_leave_the_launches_and_nothing_else_changes(optimizer, vit):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    base = dict(optimizer=optimizer, n_epochs=SLOT_STEPS, ema_decay=0.9, ema_start=2, loss_trace=True, grad_clip_norm=1e-3, **SLOTS)
    singles = []
    for p, lr in enumerate(SLOT_LRS):
        single = SpliceEngine(_cfg(lr=lr, **base), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        hist = []
        for _ in range(SLOT_STEPS):
            hist.append(single.step(A, B, A)[0, 0].clone())
        singles.append(torch.stack(hist).cpu().numpy())
    counted = _counted(single, SLOT_STEPS)

    def verdicts(distinct):
        for window in SLOT_WINDOWS:
            for rel in SLOT_RELS:
                ks = [np_plateau(losses, counted, window, rel, SLOTS["stop_patience"], 0)["stop_step"] for losses in singles]
                if ks[1] == -1 and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4 and (ks[0] != ks[2] or not distinct):
                    return window, rel, ks
        return None
    found = verdicts(True) or verdicts(False)    # (at different windows if some setting does that)
    # the premise: slots 0 and 2 stop early, slot 1 runs to the end
    assert found is not None, [np_plateau(losses, counted, 4, 0.01, 2, 0)["stop_step"] for losses in singles]
    window, rel, ks = found
    print(f"{optimizer}: stop_window {window}, stop_rel {rel}, stop steps {ks}")
    cfg = _cfg(stop_window=window, stop_rel=rel, stop_keep_best=True, **base)
    pair_cfgs = [dict(lr=lr) for lr in SLOT_LRS]
    off = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=pair_cfgs)
    on = MultiPairEngine(dict(cfg, stop_compact=True), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=pair_cfgs)
    seen = _run_both(off, on, SLOT_STEPS, (As, Bs, As), ks)
    first = min(ks[0], ks[2])
    assert all(live == [0, 1, 2] for live in seen[:first]) and seen[-1] == [1] and on.P == 1 and sorted(on._parked) == [0, 2]
    if ks[0] != ks[2]:
        assert seen[first] == [1, 2 if ks[0] < ks[2] else 0] and seen[max(ks[0], ks[2])] == [1]
    _same_slots(on, off, A[None], ks, SLOT_STEPS, (optimizer,))
    # fixed crops: the handle of the one slot left has captured graphs and replayed them since it was built
    assert _graphs(on) >= 1
    assert on.compact() is False                                        # nothing more to take out


# ------------------------------------------------------------------------------- two pairs x two crops, one of them stops
CROPS = dict(cls_warmup=1, entire_A_every=5, stop_window=3, stop_patience=1, n_epochs=30, **EXTRA)
CROPS_RELS = (0.05, 0.1, 0.02, 0.2, 0.01, 0.3)
CROPS_MAX = 30


def _first_that_splits(make, inputs, rels, max_steps, slots):
    """The first ``stop_rel`` under which the engine ``make(rel)`` -- the key off -- stops some slot early while another runs on (at
    least for two more windows):
    ``(rel, stop steps, steps to run)``; the rule's own verdicts on the run the compacted engine is held against."""
    tried = []
    for rel in rels:
        eng = make(rel, False)
        for _ in range(max_steps):
            eng.step(*inputs)
        ks = [-1 if k is None else k for k in eng.stopped_at]
        tried.append((rel, ks))
        stopped = sorted(k for k in ks if k >= 0)
        if stopped and len(set(ks)) > 1 and stopped[0] < max_steps - 8:
            return rel, ks, tried
    return None, None, tried


def test_pairs_with_crops_compact_to_a_one_pair_batch_plan(vit):
    """Grouped plans (one netG call per pair's two crops) become the batch-statistics plan of a one-pair engine with n_crops = 2."""
    gens = [synth.generator_params(80, 0.02), synth.generator_params(81, 0.1)]
    imgs = [_pair(82, p) for p in range(2)]

    def crops(img):
        return torch.stack([img, img.flip(-1)]).contiguous()
    inputs = (torch.cat([crops(a) for a, _ in imgs]).contiguous(), torch.cat([crops(b) for _, b in imgs]).contiguous(), torch.stack([a for a, _ in imgs]).contiguous())

    def make(rel, compact):
        return MultiPairEngine(_cfg(stop_rel=rel, stop_compact=compact, **CROPS), None, gens, (64, 64), (64, 64), vit_engine=vit, n_crops=2)
    rel, ks, tried = _first_that_splits(make, inputs, CROPS_RELS, CROPS_MAX, 2)
    assert rel is not None, tried                     # the premise: one pair stops while the other still runs
    first = min(k for k in ks if k >= 0)
    steps = min(CROPS_MAX, first + 8)
    ks = [k if 0 <= k < steps else -1 for k in ks]    # (verdicts behind the steps both engines run do not count)
    off, on = make(rel, False), make(rel, True)
    seen = _run_both(off, on, steps, inputs, ks)
    stopped = ks.index(first)
    assert seen[first - 1] == [0, 1] and seen[first] == [1 - stopped] and on.P == 1 and on.n_crops == 2 and on.plan_a.groups == 0 and on.plan_a.batch_stats
    _same_slots(on, off, imgs[0][0][None], ks, steps, ("crops",))


# ------------------------------------------------------------------------- three pairs that stop one after the other
THREE = dict(cls_warmup=1, entire_A_every=5, stop_window=3, stop_patience=1, n_epochs=30, **EXTRA)
THREE_RELS = (0.1, 0.05, 0.2, 0.02, 0.3, 0.15)
THREE_GAINS = (0.02, 0.1, 0.05)


def test_slots_that_stop_at_different_windows_leave_one_after_the_other(vit):
    """No per-slot settings: three pairs (own images, own generator initialisations) under one rule.  The first stop_rel of the list
    under which the engine with the key off stops two of them at different windows while the third still runs: the engine of the
    live slots is rebuilt twice, the second time out of a compacted engine."""
    gens = [synth.generator_params(80 + p, g) for p, g in enumerate(THREE_GAINS)]
    imgs = [_pair(82, p) for p in range(3)]
    As, Bs = torch.stack([a for a, _ in imgs]).contiguous(), torch.stack([b for _, b in imgs]).contiguous()

    def make(rel, compact):
        return MultiPairEngine(_cfg(stop_rel=rel, stop_compact=compact, **THREE), None, gens, (64, 64), (64, 64), vit_engine=vit)
    tried, found = [], None
    for rel in THREE_RELS:
        off = make(rel, False)
        for _ in range(THREE["n_epochs"]):
            off.step(As, Bs, As)
        ks = sorted(THREE["n_epochs"] if k is None else k for k in off.stopped_at)
        tried.append((rel, off.stopped_at))
        if ks[0] < ks[1] < ks[2] and ks[1] + 4 <= min(ks[2], THREE["n_epochs"] - 1):
            found = (rel, [-1 if k is None else k for k in off.stopped_at], ks[1] + 4)
            break
    assert found is not None, tried                   # the premise
    rel, ks, steps = found
    ks = [k if 0 <= k < steps else -1 for k in ks]    # (a verdict behind the steps both engines run does not count)
    print(f"three pairs: stop_rel {rel}, stop steps {ks}, {steps} steps")
    off, on = make(rel, False), make(rel, True)
    seen = _run_both(off, on, steps, (As, Bs, As), ks)
    sizes = [len(live) for live in seen]
    assert sizes[0] == 3 and sizes[-1] == 1 and 2 in sizes and sizes == sorted(sizes, reverse=True), seen
    _same_slots(on, off, imgs[0][0][None], ks, steps, ("three",))


# --------------------------------------------------------------------- a sweep whose survivors are uniform; every rule on
SWEEP = dict(cls_warmup=1, entire_A_every=7, stop_window=3, stop_patience=2, n_epochs=20, lr_plateau_factor=0.5, lr_plateau_patience=1, **EXTRA)
SWEEP_LRS = [2e-3, 0.0, 2e-3]
SWEEP_STEPS = 20


def test_a_sweep_whose_survivors_are_uniform_takes_the_scalar_path(vit):
    """Slot 1 (lr 0) stops; slots 0 and 2 share every per-slot key, so the engine of the live slots stages one lr and no per-pair
    table -- and the bits agree.  With the plateau lr rule, whose records a parked slot answers from its parked state too."""
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    pair_cfgs = [dict(lr=lr) for lr in SWEEP_LRS]

    def make(rel, compact):
        return MultiPairEngine(_cfg(stop_rel=rel, stop_compact=compact, **SWEEP), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=pair_cfgs)
    tried = []
    for rel in (0.005, 0.01, 0.002, 0.02):
        off = make(rel, False)
        for _ in range(SWEEP_STEPS):
            off.step(As, Bs, As)
        ks = [-1 if k is None else k for k in off.stopped_at]
        tried.append((rel, ks))
        if ks[0] == ks[2] == -1 and 0 <= ks[1] < SWEEP_STEPS - 6:
            break
    assert ks[0] == ks[2] == -1 and 0 <= ks[1] < SWEEP_STEPS - 6, tried     # the premise: only the slot that cannot learn stops
    assert off._pair_lr and off.lr_state(1)["cuts"] >= 1                     # (the stopped slot had its lr cut on the way)
    off, on = make(rel, False), make(rel, True)
    seen = _run_both(off, on, SWEEP_STEPS, (As, Bs, As), ks)
    assert seen[ks[1] - 1] == [0, 1, 2] and seen[ks[1]] == [0, 2] == seen[-1]
    assert on.P == 2 and not on._pair_lr and not on._pair_lambdas and isinstance(on.lr, list) and len(on.lr) == 3
    _same_slots(on, off, A[None], ks, SWEEP_STEPS, ("sweep",))
    assert _graphs(on) >= 1


# ------------------------------------------------------------------------------------------------------------------ the loops
TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, cls_warmup=1, entire_A_every=5, loss_trace=True,
             ema_decay=0.9, stop_keep_best=True)
FILES = ("output.png", "output_ema.png", "output_best.png", "losses.csv")


def _write_pair(root, name, pair=0):
    from PIL import Image
    A, B = synth.smooth_image_pair(60, pair, 72, 72)
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


def _files(root, names=FILES):
    return {n: open(f"{root}/out/{n}", "rb").read() for n in names}


def _train_pairs(tmp_path, tag, vit_state, over):
    from splice_amd import batch
    from splice_amd.train import train_pairs
    roots = [_write_pair(tmp_path, f"{tag}{p}", p) for p in range(3)]
    eng = train_pairs(roots, cfg_overrides=dict(TRAIN, **over), vit_state=vit_state, progress=False)
    fields = [json.dumps(batch._slot_fields(eng, p), sort_keys=True) for p in range(3)]
    return eng, [_files(r) for r in roots], fields


# the first stop_rel of the list under which the rule, with the key off, stops some pair early while another runs on
PAIRS_STOP = dict(n_epochs=40, stop_window=3, stop_patience=1)
PAIRS_RELS = (0.05, 0.1, 0.02, 0.2)


def test_train_pairs_writes_the_same_files_with_the_key_on(tmp_path):
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    for aug in (dict(use_augmentations=True), dict(use_augmentations=False, global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0)):
        found = None
        for rel in PAIRS_RELS:
            over = dict(PAIRS_STOP, stop_rel=rel, **aug)
            ref, files, fields = _train_pairs(tmp_path, f"a{int(aug['use_augmentations'])}r{rel}_", vit_state, over)
            ks = ref.stopped_at
            if len(set(ks)) > 1 and any(k is not None and k < over["n_epochs"] - 7 for k in ks):
                found = (over, ks, files, fields)
                break
        assert found is not None, "no stop_rel of the list stops some pair early while another runs on"
        over, ks, files, fields = found
        print(f"train_pairs, use_augmentations {aug['use_augmentations']}: stop_rel {over['stop_rel']}, stop steps {ks}, {ref.step_idx + 1} steps")
        again, files2, fields2 = _train_pairs(tmp_path, f"b{int(aug['use_augmentations'])}_", vit_state, over)
        if (files2, fields2, again.stopped_at) != (files, fields, ks):
            # the premise does not hold under augmentations on this device: the deterministic full-cover crops decide
            assert aug["use_augmentations"], "two runs with the key off differ under deterministic crops"
            print("train_pairs is not reproducible run to run under use_augmentations: True; falling back to full-cover crops")
            continue
        on, files3, fields3 = _train_pairs(tmp_path, f"c{int(aug['use_augmentations'])}_", vit_state, dict(over, stop_compact=True))
        assert on.stopped_at == ks and on.P < 3 and len(on._parked) >= 1           # slots were parked on the way
        for p in range(3):
            assert files3[p] == files[p], (p, [n for n in FILES if files3[p][n] != files[p][n]])
            assert fields3[p] == fields[p], p
        return
    raise AssertionError("unreachable: the deterministic case returns or fails")


RESUME = dict(TRAIN, n_epochs=12, log_images_freq=3, checkpoint_every=4, grad_clip_norm=1e-3, stop_window=3, stop_patience=1000, lr_plateau_factor=0.5,
              scheduler_policy="cosine")


class Interrupt(Exception):
    pass


def _arenas(eng):
    return {k: getattr(eng, k).clone() for k in ("params", "m", "v", "ema", "best", "running", "trace_dev", "lr_state_dev", "clip_dev")}


def test_train_model_resumes_from_its_checkpoint(tmp_path):
    import os
    from splice_amd.train import CHECKPOINT_NAME, train_model
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    names = ("output.png", "output_ema.png", "output_best.png", "losses.csv")
    for aug in (dict(use_augmentations=True), dict(use_augmentations=False, global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0)):
        tag = f"{int(aug['use_augmentations'])}"
        over = dict(RESUME, **aug)
        # (resume without a file: the run starts at step 0)
        whole = train_model(_write_pair(tmp_path, "whole" + tag), cfg_overrides=dict(over, resume=True), vit_state=vit_state, progress=False)
        twice = train_model(_write_pair(tmp_path, "twice" + tag), cfg_overrides=over, vit_state=vit_state, progress=False)
        want, want_files = _arenas(whole), _files(tmp_path / ("whole" + tag), names)
        if not all(_bits(want[k], v) for k, v in _arenas(twice).items()) or _files(tmp_path / ("twice" + tag), names) != want_files:
            assert aug["use_augmentations"], "two uninterrupted runs differ under deterministic crops"
            print("train_model is not reproducible run to run under use_augmentations: True; falling back to full-cover crops")
            continue
        root = _write_pair(tmp_path, "cut" + tag)
        images = []

        def callback(image):
            images.append(len(images))
            if len(images) == 3:                       # the image of epoch 9: behind the checkpoint of epoch 8
                raise Interrupt()
        with pytest.raises(Interrupt):
            train_model(root, callback=callback, cfg_overrides=over, vit_state=vit_state, progress=False)
        assert os.path.exists(os.path.join(root, "out", CHECKPOINT_NAME)) and not os.path.exists(os.path.join(root, "out", "losses.csv"))
        state = torch.load(os.path.join(root, "out", CHECKPOINT_NAME), map_location="cpu", weights_only=False)
        assert state["epoch"] == 8 and state["feed_step"] == 7 and state["states"][0]["step_idx"] == 7
        resumed = train_model(root, cfg_overrides=dict(over, resume=True), vit_state=vit_state, progress=False)
        assert resumed.step_idx == 11 and whole.step_idx == 11
        for k, v in _arenas(resumed).items():
            assert _bits(want[k], v), k
        assert _files(root, names) == want_files
        assert resumed.lr_state() == whole.lr_state() and resumed.clip_state() == whole.clip_state() and resumed.best_state() == whole.best_state()
        # a checkpoint written under another config is refused by the name of the key
        with pytest.raises(ValueError, match="another 'lr'"):
            train_model(root, cfg_overrides=dict(over, resume=True, lr=0.01), vit_state=vit_state, progress=False)
        return
    raise AssertionError("unreachable: the deterministic case returns or fails")
