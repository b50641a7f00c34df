"""GPU: pair snapshots.  The gather form of the input staging against a handle that is handed the gathered
batches; a run that is snapshotted after k steps and restored into a fresh engine against the same run left alone; a slot moved out of a
three-slot engine into a one-pair engine.  Every comparison is exact: a pair's bits do not depend on the batch it rides in, so a slot
that moves continues bit for bit."""
import ctypes as C
import pickle

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import DEFAULT_CFG, MultiPairEngine, SpliceEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _bits(a, b):
    """Equal bit for bit (NaN rows of a trace included)."""
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and torch.equal(a.cpu(), b.cpu())


def _same_state(a, b, what=()):
    """Two snapshots: the same keys, tensors equal bit for bit, everything else equal."""
    assert sorted(a) == sorted(b), what + (sorted(a), sorted(b))
    for k in a:
        if torch.is_tensor(a[k]):
            assert _bits(a[k], b[k]), what + (k,)
        else:
            assert a[k] == b[k], what + (k, a[k], b[k])


TABLES = tuple(attr for _, attr in MultiPairEngine.SLOT_ARENAS + MultiPairEngine.SLOT_ROWS) + ("trace_dev",)   # the engine's own list of what a slot owns


def _same_engine(a, b, what=()):
    """Every arena, buffer, record, trace row and losses row of two engines with the same slots."""
    assert a.step_idx == b.step_idx and a.generator_calls == b.generator_calls, what
    for name in TABLES:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), what + (name,)
        if ta is not None:
            assert _bits(ta, tb), what + (name,)
    assert a.stop_state() == b.stop_state() and a.stopped_at == b.stopped_at and a.lr_scale == b.lr_scale, what
    for p in range(a.P):
        _same_state(a.snapshot(p, device="cpu"), b.snapshot(p, device="cpu"), what + (p,))


# ------------------------------------------------------------------------------------------------------- the gather staging
def _images(seed, pairs, n, size):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(pairs * n, 3, size, size, generator=g).to(DEV)


GATHER = [("one crop", 1, 64, False), ("crops 2 x 3", (2, 3), 64, False), ("block of 3*61*61 floats", 1, 61, False), ("unaligned source", 1, 64, True)]


@pytest.mark.parametrize("name,n_crops,size,unaligned", GATHER, ids=[g[0] for g in GATHER])
def test_gather_staging_equals_a_handle_given_the_gathered_batches(name, n_crops, size, unaligned, vit):
    """pairs_in = 4, rows [1, 3]: the first step (an entire-image step: all three buffers are staged) of a two-pair handle that gathers
    its pairs out of the four-pair batches leaves the losses, parameters and moments of a two-pair handle given the two pairs."""
    nA, nB = (n_crops, n_crops) if isinstance(n_crops, int) else n_crops
    rows = [1, 3]
    gens = [synth.generator_params(90 + p, 0.02) for p in range(2)]
    A4, B4, E4 = _images(1, 4, nA, size), _images(2, 4, nB, size), _images(3, 4, 1, 64)
    if unaligned:   # the same values at an address that is no multiple of 16: the scalar path
        def shift(t):
            buf = torch.empty(t.numel() + 1, device=DEV)
            buf[1:].copy_(t.reshape(-1))
            return buf[1:].view(t.shape)
        A4, B4, E4 = shift(A4), shift(B4), shift(E4)
        assert A4.data_ptr() % 16 == 4 and A4.is_contiguous()
    assert (nA * 3 * size * size) % 4 == (3 if size == 61 else 0)

    def pick(t, n):
        return torch.cat([t[r * n:(r + 1) * n] for r in rows]).contiguous()
    engines = []
    for gather in (False, True):
        eng = MultiPairEngine(_cfg(), None, gens, (size, size), (64, 64), vit_engine=vit, n_crops=n_crops)
        if gather:
            _lib.check(_lib.lib().splice_step_set_input_rows(eng.handle, 4, (C.c_int * 2)(*rows)), "set_input_rows")
            eng.P_in = 4
            eng.step(A4, B4, E4)
        else:
            eng.step(pick(A4, nA), pick(B4, nB), pick(E4, 1))
        engines.append(eng)
    flat, gathered = engines
    torch.cuda.synchronize()
    assert _bits(flat.losses_dev, gathered.losses_dev) and float(flat.losses_dev[:, 0].min()) > 0
    assert not torch.equal(flat.losses_dev[0], flat.losses_dev[1])          # (the two pairs differ: a swapped or repeated row would show)
    for name in ("params", "m", "v", "running"):
        assert _bits(getattr(flat, name), getattr(gathered, name)), name
    # NULL switches the form off: the handle takes two-pair batches again, and runs on as the flat one
    _lib.check(_lib.lib().splice_step_set_input_rows(gathered.handle, 0, None), "set_input_rows")
    gathered.P_in = 2
    for eng in engines:
        eng.step(pick(A4, nA), pick(B4, nB), pick(E4, 1))
    assert _bits(flat.losses_dev, gathered.losses_dev) and _bits(flat.params, gathered.params)


def test_the_row_setter_refuses_bad_tables(vit):
    eng = MultiPairEngine(_cfg(), None, [synth.generator_params(90 + p, 0.02) for p in range(2)], (64, 64), None, vit_engine=vit)
    L = _lib.lib()

    def rc(pairs_in, rows):
        return L.splice_step_set_input_rows(eng.handle, pairs_in, (C.c_int * len(rows))(*rows))
    assert rc(4, [3, 1]) != 0 and b"strictly increasing" in L.splice_last_error()     # unsorted
    assert rc(4, [1, 1]) != 0                                                          # repeated
    assert rc(4, [1, 4]) != 0 and rc(4, [-1, 2]) != 0                                  # out of range
    assert rc(33, [1, 32]) != 0 and b"at most 32" in L.splice_last_error()             # more than 32 rows
    assert rc(1, [0, 0]) != 0                                                          # fewer pairs than the handle has
    assert rc(32, [0, 31]) == 0 and rc(4, [1, 3]) == 0 and L.splice_step_set_input_rows(eng.handle, 0, None) == 0


# ------------------------------------------------------------------------------------------------------------------- resume
# entire-image steps 0 5 10 15; counted steps 2 3 4 | 6 7 8 | 9 11 12 | 13 14 16: windows close at steps 4, 8, 12 and 16
STEPS = 18
ALL_RULES = dict(cls_warmup=2, entire_A_every=5, n_epochs=STEPS, stop_window=3, stop_rel=0.5, stop_patience=1000, stop_keep_best=True, ema_decay=0.9, ema_start=2,
                 grad_clip_norm=1e-3, lr_plateau_factor=0.5, lr_plateau_patience=1, loss_trace=True)
OPTIMISERS = {"adam": dict(optimizer="adam"), "rmsprop_cosine": dict(optimizer="rmsprop", scheduler_policy="cosine")}
PAIR_LRS = [dict(lr=2e-3), dict(lr=1e-3)]
# k steps before the snapshot: the resumed handle's first step is step k
RESUME_AT = {"before cls_warmup": 1, "between two entire-image steps": 7, "at a window close": 9}


def _inputs(step):
    """The step's batches, a function of the step index alone (two pairs; odd steps see mirrored images)."""
    imgs = [synth.smooth_image_pair(62, p, 64, 64) for p in range(2)]
    A = torch.from_numpy(np.stack([a for a, _ in imgs])).to(DEV)
    B = torch.from_numpy(np.stack([b for _, b in imgs])).to(DEV)
    return (A.flip(-1).contiguous(), B.flip(-2).contiguous(), A) if step % 2 else (A, B, A)


def _engine(vit, opt):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(2)]
    return MultiPairEngine(_cfg(**ALL_RULES, **OPTIMISERS[opt]), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=PAIR_LRS)


_REFERENCE = {}


def _reference(vit, opt):
    """One engine run STEPS steps straight (computed once per optimiser, left unchanged), and its structure-loss column."""
    if opt not in _REFERENCE:
        eng, ssim = _engine(vit, opt), []
        for k in range(STEPS):
            ssim.append(eng.step(*_inputs(k))[:, 1].clone())
        torch.cuda.synchronize()
        _REFERENCE[opt] = (eng, torch.stack(ssim).cpu())
    return _REFERENCE[opt]


@pytest.mark.parametrize("opt", list(OPTIMISERS))
def test_the_reference_run_exercises_every_rule(opt, vit):
    """(the premise of the resume cases: cuts, clipped steps, a moving best record and an average that differs from the weights)"""
    ref, ssim = _reference(vit, opt)
    assert all(r["cuts"] >= 1 for r in ref.lr_state()) and all(r["clipped"] >= 1 for r in ref.clip_state())
    assert all(r["best_step"] is not None for r in ref.best_state()) and not torch.equal(ref.ema, ref.params)
    assert ref.stopped_at == [None, None] and len(ref.loss_trace(0)) == STEPS
    assert bool((ssim[:2] == 0).all()) and bool((ssim[2:] != 0).all())      # the structure term: off below cls_warmup, on from it


@pytest.mark.parametrize("opt", list(OPTIMISERS))
@pytest.mark.parametrize("where", list(RESUME_AT))
def test_resume_continues_bit_for_bit(where, opt, vit):
    """k steps, a snapshot to the host (pickled and back), a new engine from the initial generator states, restore, STEPS - k steps:
    every arena, buffer, record, trace row and losses row is that of the run left alone."""
    k = RESUME_AT[where]
    ref, ref_ssim = _reference(vit, opt)
    first = _engine(vit, opt)
    for s in range(k):
        first.step(*_inputs(s))
    states = pickle.loads(pickle.dumps([first.snapshot(p, device="cpu") for p in range(2)]))
    assert all(s["step_idx"] == k - 1 and s["format"] == 1 and not s["params"].is_cuda and "stride" not in s for s in states)
    del first
    eng = _engine(vit, opt)
    eng.restore(states)
    assert eng.step_idx == k - 1
    ssim = []
    for s in range(k, STEPS):
        ssim.append(eng.step(*_inputs(s))[:, 1].clone())
    torch.cuda.synchronize()
    ssim = torch.stack(ssim).cpu()
    if k > ALL_RULES["cls_warmup"]:   # a handle that starts behind cls_warmup computes the structure term from its first step on
        assert bool((ssim != 0).all())
    assert torch.equal(ssim, ref_ssim[k:])
    _same_engine(eng, ref, (where, opt))
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    if STEPS - k >= 9:                # fixed shapes: the resumed handle captured graphs and replayed them
        assert stats[0] + stats[2] >= 2


def test_restore_is_refused_on_the_device_too(vit):
    """splice_step_restore: before the first step only, and the stop records exactly when the handle has the rule."""
    L = _lib.lib()
    eng = _engine(vit, "adam")
    rec = (_lib.StopState * 2)()
    assert L.splice_step_restore(eng.handle, 3, None, _lib.current_stream()) != 0 and b"stop rule" in L.splice_last_error()
    assert L.splice_step_restore(eng.handle, -1, rec, _lib.current_stream()) != 0
    eng.step(*_inputs(0))
    assert L.splice_step_restore(eng.handle, 3, rec, _lib.current_stream()) != 0 and b"before its first step" in L.splice_last_error()
    with pytest.raises(ValueError, match="already stepped"):
        eng.restore([eng.snapshot(p) for p in range(2)])
    plain = SpliceEngine(_cfg(), None, synth.generator_params(70, 0.02), (64, 64), None, vit_engine=vit)
    assert L.splice_step_restore(plain.handle, 3, rec, _lib.current_stream()) != 0 and L.splice_step_restore(plain.handle, 3, None, _lib.current_stream()) == 0


# ------------------------------------------------------------------------------------------------ the list of what a slot owns
def test_every_per_slot_tensor_is_in_the_slot_tables(vit):
    """Three slots (no unrelated tensor's leading dimension is 3) with every rule that keeps state on -- the third moment arena and both
    clipping records among them -- after two steps: (a) every device tensor of the engine with one row per slot, or ``stride`` floats
    per slot, is named by the engine's tables, or is the gradient arena (scratch of a step) or the trace; (b) a snapshot holds exactly
    the tables' keys, the trace, the stop record and the seven fixed entries.  A tensor a rule allocates per slot and forgets in the
    tables fails (a); a table row that snapshot() does not walk fails (b)."""
    rules = dict(ALL_RULES, optimizer="adam", optimizer_amsgrad=True, grad_clip_auto=2.0)
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    eng = MultiPairEngine(_cfg(**rules), None, gens, (64, 64), (64, 64), vit_engine=vit)
    A, B = synth.smooth_image_pair(62, 0, 64, 64)
    A3 = torch.from_numpy(A).to(DEV)[None].expand(3, -1, -1, -1).contiguous()
    B3 = torch.from_numpy(B).to(DEV)[None].expand(3, -1, -1, -1).contiguous()
    for _ in range(2):
        eng.step(A3, B3, A3)
    torch.cuda.synchronize()
    tables = MultiPairEngine.SLOT_ARENAS + MultiPairEngine.SLOT_ROWS
    assert eng.P == 3 and all(getattr(eng, attr) is not None for _, attr in tables) and eng.trace_dev is not None   # (the premise: every rule is on)
    named = {attr for _, attr in tables} | {"grads", "trace_dev"}
    per_slot = [name for name, t in vars(eng).items()
                if isinstance(t, torch.Tensor) and t.is_cuda and t.dim() > 0 and (t.shape[0] == eng.P or t.numel() == eng.P * eng.stride)]
    assert len(per_slot) == len(tables) + 1 and set(per_slot) <= named, sorted(set(per_slot) - named)   # (+ 1: grads; the trace is time-major)
    fixed = {"format", "step_idx", "cfg", "n_crops", "crop_hw", "entire_hw", "generator_calls"}
    assert set(eng.snapshot(0)) == {key for key, _ in tables} | {"trace", "stop"} | fixed


# ------------------------------------------------------------------------------------------------- a move between batch sizes
def test_a_slot_moves_into_a_one_pair_engine(vit):
    """Slot 2 of a three-slot sweep after 7 steps, restored into a SpliceEngine (another arena stride, the scalar lr path): both go
    on for 6 steps and stay equal."""
    lrs = [2e-3, 5e-4, 1e-3]
    rules = dict(ALL_RULES, optimizer="adam")
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    multi = MultiPairEngine(_cfg(**rules), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in lrs])
    A, B = synth.smooth_image_pair(62, 0, 64, 64)
    A, B = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    A3, B3 = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    for _ in range(7):
        multi.step(A3, B3, A3)
    single = SpliceEngine(_cfg(**dict(rules, lr=lrs[2])), None, synth.generator_params(99, 0.02), (64, 64), (64, 64), vit_engine=vit)
    assert single.stride != multi.stride
    single.restore([multi.snapshot(2)])
    for step in range(7, 13):
        multi.step(A3, B3, A3)
        single.step(A, B, A)
        assert _bits(multi.losses_dev[2], single.losses_dev[0]), step
    a, b = multi.snapshot(2, device="cpu"), single.snapshot(0, device="cpu")
    _same_state(a, b, ("moved",))
    assert a["step_idx"] == 12 and a["trace"].shape == (13, 8) and not torch.isnan(a["trace"][:, :6]).any()
    assert multi.lr_state(2) == single.lr_state() and multi.best_state(2) == single.best_state() and multi.stop_state()[2] == single.stop_state()[0]
    for kind in (dict(), dict(ema=True), dict(best=True)):
        sa, sb = multi.state_dict(2, **kind), single.state_dict(0, **kind)
        assert sorted(sa) == sorted(sb) and all(torch.equal(sa[k], sb[k]) for k in sa), kind
