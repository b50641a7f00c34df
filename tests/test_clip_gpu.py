"""GPU: clipping of every pair's gradient by its global norm inside the fused step.  The two norm stages against
their NumPy restatement (engine.np_grad_clip), the clipped update against the plain update fed the host-scaled gradient, the guard
against a non-finite gradient, frozen slots -- op level; then the fused step: a threshold nothing reaches changes no bit, graph replay
equals eager launches, a pair's bits do not depend on its neighbours or on a neighbour's stop, the several-scales engine, train_model.
Every comparison is exact."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import CLIP_CHUNK, MultiPairEngine, MultiScaleEngine, SpliceEngine, clip_records, np_grad_clip
from splice_amd.generator import optim_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = {0: (0.5, 0.99, 1e-8), 1: (0.99, 0.0, 1e-8), 2: (0.0, 0.0, 0.0)}   # Adam betas / RMSprop alpha / SGD
KINDS = [0, 1, 2]
LR = 2e-3
HUGE = 1e30
F = np.float32


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return _np(a).tobytes() == _np(b).tobytes()


def _dev(x, offset=0):
    """A device copy of ``x`` that starts ``offset`` floats into its allocation."""
    base = torch.zeros(x.numel() + offset, device=DEV)
    base[offset:] = x.reshape(-1).to(DEV)
    return base[offset:]


def _state(P=1):
    return torch.zeros(P, 6, dtype=torch.int32, device=DEV)


def _partials(P, n, guard=8):
    """The caller's scratch of the norm stages with ``guard`` floats behind it that no kernel may touch."""
    chunks = (n + CLIP_CHUNK - 1) // CLIP_CHUNK
    return torch.full((P * chunks + guard,), -7.0, device=DEV), P * chunks


def _norm(g, g2, P, stride, n, c, part, state, stop=None, step_dev=None):
    _lib.check(_lib.lib().splice_grad_norm_pairs(_lib.ptr(g), _lib.ptr(g2), P, stride, n, c, _lib.ptr(part), _lib.ptr(state), _lib.ptr(stop), _lib.ptr(step_dev),
                                                 _lib.current_stream()), "grad_norm_pairs")


def _check_record(rec, want, c, tag):
    sumsq, norm, coef, skip = want
    assert rec["sumsq"].tobytes() == sumsq.tobytes(), (tag, rec["sumsq"], sumsq)
    assert rec["norm"].tobytes() == np.sqrt(sumsq).tobytes(), (tag, rec["norm"], norm)
    assert rec["coef"].tobytes() == coef.tobytes() and rec["skip"] == skip, (tag, rec["coef"], coef)
    if not skip:
        assert rec["coef"].tobytes() == np.minimum(F(1), F(c) / (rec["norm"] + F(1e-6))).tobytes(), tag


# ------------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 4, 1027, 4096, 4097, 9000])
def test_norm_of_one_arena_equals_restatement(n, offset):
    """n = 1027: whole float4s and a straddling one; 4096 / 4097 / 9000: one full chunk, a second of one element, three chunks;
    offset 1: the arena off its 16-byte alignment, every element read on the scalar path -- the same bits."""
    gen = torch.Generator().manual_seed(200 + n)
    g_h, g2_h = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.3
    g, g2 = _dev(g_h, offset), _dev(g2_h, offset)
    assert g.data_ptr() % 16 == (4 * offset) % 16
    for second, second_h in ((None, None), (g2, g2_h)):
        ref = np_grad_clip(_np(g_h), None if second_h is None else _np(second_h), HUGE)
        for c, clipped in ((0.5 * float(ref[1]), 1), (HUGE, 0)):
            part, used = _partials(1, n)
            state = _state()
            _norm(g, second, 1, 0, n, c, part, state)
            torch.cuda.synchronize()
            rec = clip_records(state)[0]
            _check_record(rec, np_grad_clip(_np(g_h), None if second_h is None else _np(second_h), c), c, (n, offset, c))
            assert rec["clipped"] == clipped and rec["skipped"] == 0 and (rec["coef"] < 1) == bool(clipped)
            assert bool((part[used:] == -7.0).all()) and bool((part[:used] >= 0).all())          # the scratch and nothing behind it
    assert _same(g, g_h) and _same(g2, g2_h)                                                      # the norm stages only read


@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("n,stride", [(1027, 1088), (4100, 4160)])
def test_norm_of_three_pairs_equals_restatement_per_pair(n, stride, with_g2):
    """Every pair's chunks are counted from the start of ITS arena: the record of a pair is that of its own one-arena call."""
    P = 3
    gen = torch.Generator().manual_seed(n + with_g2)
    g_h = torch.randn(P, stride, generator=gen) * torch.tensor([1.0, 3.0, 0.2])[:, None]          # (the padding holds values too: it is not read)
    g2_h = torch.randn(P, stride, generator=gen) * 0.3
    g, g2 = _dev(g_h), (_dev(g2_h) if with_g2 else None)
    c = 0.5 * float(np_grad_clip(_np(g_h[0, :n]), _np(g2_h[0, :n]) if with_g2 else None, HUGE)[1])   # clips pairs 0 and 1, not pair 2
    part, used = _partials(P, n)
    state = _state(P)
    _norm(g, g2, P, stride, n, c, part, state)
    torch.cuda.synchronize()
    recs = clip_records(state)
    for p in range(P):
        _check_record(recs[p], np_grad_clip(_np(g_h[p, :n]), _np(g2_h[p, :n]) if with_g2 else None, c), c, (n, p))
        one, one_part = _state(), _partials(1, n)[0]
        _norm(g[p * stride:], None if g2 is None else g2[p * stride:], 1, 0, n, c, one_part, one)
        torch.cuda.synchronize()
        assert _same(one, state[p:p + 1]), p
    assert [r["clipped"] for r in recs] == [1, 1, 0]
    assert bool((part[used:] == -7.0).all())


def _host_scaled(g_h, g2_h, coef):
    s = _np(g_h) if g2_h is None else (_np(g_h) + _np(g2_h)).astype(F)
    return torch.from_numpy((s * F(coef)).astype(F))


@pytest.mark.parametrize("with_g2", [False, True])
@pytest.mark.parametrize("kind", KINDS)
def test_clipped_update_equals_the_plain_update_of_the_scaled_gradient(kind, with_g2):
    """4 consecutive updates, max_norm half the first gradient's norm (the gradients grow: every step is clipped).  The host-step call
    against splice_optim_step_ex, the device-step call (the fused step's form, with an average) against splice_optim_step_pairs_ema, both
    fed fl(fl(g + g2) * coef) with coef read back from the record.  With a threshold nothing reaches: the plain call on g itself."""
    L = _lib.lib()
    n = 1027
    gen = torch.Generator().manual_seed(40 + kind)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen) * (0.5 + k) for k in range(4)]
    g2s = [torch.randn(n, generator=gen) * 0.25 for k in range(4)] if with_g2 else [None] * 4
    half = 0.5 * float(np_grad_clip(_np(grads[0]), None if g2s[0] is None else _np(g2s[0]), HUGE)[1])
    lr_dev = torch.tensor([LR], device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    s = _lib.current_stream()
    for c, clipped in ((half, 4), (HUGE, 0)):
        z = lambda: torch.zeros(n, device=DEV)
        host, host_ref = dict(p=_dev(p0), m=z(), v=z()), dict(p=_dev(p0), m=z(), v=z())
        stride4 = (n + 3) // 4 * 4                        # splice_optim_step_pairs_ema walks n_pairs * stride floats: its arenas are padded with zeros
        pad = lambda x: torch.cat([x.reshape(-1).to(DEV), torch.zeros(stride4 - n, device=DEV)])
        dev, dev_ref = dict(p=_dev(p0), m=z(), v=z(), e=_dev(p0)), dict(p=pad(p0), m=pad(z()), v=pad(z()), e=pad(p0))
        state_h, state_d = _state(), _state()
        part = _partials(1, n)[0]
        for k in range(4):
            step_dev.fill_(k + 1)
            for a, state in ((host, state_h), (dev, state_d)):
                g, g2 = _dev(grads[k]), (None if g2s[k] is None else _dev(g2s[k]))
                _norm(g, g2, 1, 0, n, c, part, state)
                if a is host:
                    _lib.check(L.splice_optim_step_clip(kind, _lib.ptr(a["p"]), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(a["m"]), _lib.ptr(a["v"]), None, n, LR, None,
                                                        *HP[kind], k + 1, 0, 0.0, 0, _lib.ptr(state), s), "optim_step_clip")
                else:
                    _lib.check(L.splice_optim_step_pairs_clip(kind, _lib.ptr(a["p"]), _lib.ptr(g), _lib.ptr(g2), _lib.ptr(a["m"]), _lib.ptr(a["v"]), _lib.ptr(a["e"]), 1, 0, n,
                                                              _lib.ptr(lr_dev), *HP[kind], _lib.ptr(step_dev), None, 0, 0.9, 1, _lib.ptr(state), s), "pairs_clip")
            torch.cuda.synchronize()
            rec = clip_records(state_h)[0]
            assert _same(state_h, state_d) and rec["clipped"] == (k + 1 if clipped else 0) and (rec["coef"] < 1) == bool(clipped)
            if clipped:
                gs, gs2 = _dev(_host_scaled(grads[k], g2s[k], rec["coef"])), None
            else:
                gs, gs2 = _dev(grads[k]), (None if g2s[k] is None else _dev(g2s[k]))
            gd, gd2 = pad(gs), (None if gs2 is None else pad(gs2))
            _lib.check(L.splice_optim_step_ex(kind, _lib.ptr(host_ref["p"]), _lib.ptr(gs), _lib.ptr(gs2), _lib.ptr(host_ref["m"]), _lib.ptr(host_ref["v"]), n, LR, None,
                                              *HP[kind], k + 1, 0, s), "optim_step_ex")
            _lib.check(L.splice_optim_step_pairs_ema(kind, _lib.ptr(dev_ref["p"]), _lib.ptr(gd), _lib.ptr(gd2), _lib.ptr(dev_ref["m"]), _lib.ptr(dev_ref["v"]),
                                                     _lib.ptr(dev_ref["e"]), 1, stride4, n, _lib.ptr(lr_dev), *HP[kind], _lib.ptr(step_dev), None, 0, 0.9, 1, s), "pairs_ema")
            torch.cuda.synchronize()
            for key in "pmv":
                assert _same(host[key], host_ref[key]), (kind, c, k, key)
                assert _same(dev[key], dev_ref[key][:n]), (kind, c, k, key)
            assert _same(dev["e"], dev_ref["e"][:n]), (kind, c, k)
        assert not _same(host["p"], _dev(p0)) and clip_records(state_h)[0]["clipped"] == clipped


def test_optim_step_wrapper_clips():
    n = 1027
    gen = torch.Generator().manual_seed(5)
    p0, g_h = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    p, m, v, g, state = _dev(p0), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV), _dev(g_h), _state()
    optim_step(2, p, g, m, v, LR, *HP[2], 1, clip_norm=1.0, clip_state=state)
    torch.cuda.synchronize()
    rec = clip_records(state)[0]
    _check_record(rec, np_grad_clip(_np(g_h), None, 1.0), 1.0, "wrapper")
    want = (_np(p0) - F(LR) * (_np(g_h) * rec["coef"]).astype(F)).astype(F)                        # SGD: p -= lr * fl(g * coef)
    assert rec["clipped"] == 1 and _np(p).tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="clip_state"):
        optim_step(2, p, g, m, v, LR, *HP[2], 1, clip_norm=1.0)


def _pairs_clip(kind, a, g, P, stride, n, lrs, step_dev, stop, zero_grad, state):
    _lib.check(_lib.lib().splice_optim_step_pairs_clip(kind, _lib.ptr(a["p"]), _lib.ptr(g), None, _lib.ptr(a["m"]), _lib.ptr(a["v"]), _lib.ptr(a["e"]), P, stride, n,
                                                       _lib.ptr(lrs), *HP[kind], _lib.ptr(step_dev), _lib.ptr(stop), zero_grad, 0.9, 1, _lib.ptr(state),
                                                       _lib.current_stream()), "pairs_clip")


def _arenas(p_h):
    return dict(p=_dev(p_h).clone(), m=torch.zeros(p_h.numel(), device=DEV), v=torch.zeros(p_h.numel(), device=DEV), e=_dev(p_h).clone())


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
def test_a_non_finite_gradient_skips_its_slot_alone(kind, zero_grad):
    """One inf and one nan element in slot 1 of 3: the slot's p, m, v and e are not written at that step (its g only as the zeros of
    zero_grad), slots 0 and 2 equal their own one-arena calls, and the slot's next update, with a finite gradient, applies normally."""
    P, n, stride, c = 3, 1027, 1088, 5.0
    gen = torch.Generator().manual_seed(90 + kind)
    p0 = torch.zeros(P, stride)
    p0[:, :n] = torch.randn(P, n, generator=gen)
    lrs = torch.tensor([1e-3, 2e-3, 5e-4], device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    multi, single = _arenas(p0), [_arenas(p0[s]) for s in range(P)]
    state, states = _state(P), [_state() for _ in range(P)]
    part, part1 = _partials(P, n)[0], _partials(1, n)[0]
    for t in (1, 2):
        step_dev.fill_(t)
        g_h = torch.zeros(P, stride)
        g_h[:, :n] = torch.randn(P, n, generator=gen)
        if t == 1:
            g_h[1, 5], g_h[1, 1026] = float("inf"), float("nan")                                  # (the float4 body and the scalar tail)
        g = _dev(g_h).clone()
        _norm(g, None, P, stride, n, c, part, state)
        _pairs_clip(kind, multi, g, P, stride, n, lrs, step_dev, None, zero_grad, state)
        for s in range(P):
            gs = _dev(g_h[s]).clone()
            _norm(gs, None, 1, 0, n, c, part1, states[s])
            _pairs_clip(kind, single[s], gs, 1, 0, n, lrs[s:s + 1], step_dev, None, zero_grad, states[s])
        torch.cuda.synchronize()
        recs = clip_records(state)
        sl1 = slice(stride, 2 * stride)
        if t == 1:
            assert recs[1]["skip"] == 1 and recs[1]["skipped"] == 1 and recs[1]["coef"] == 0 and recs[1]["clipped"] == 0
            for key in "pe":
                assert _same(multi[key][sl1], p0[1]), key
            assert not multi["m"][sl1].any() and not multi["v"][sl1].any()
            if zero_grad:
                assert not g[sl1].any()
            else:
                assert _same(g[sl1], g_h[1])
        else:
            assert recs[1]["skip"] == 0 and recs[1]["skipped"] == 1 and 0 < recs[1]["coef"] <= 1
            assert not _same(multi["p"][sl1], p0[1]) and bool(torch.isfinite(multi["p"]).all())
        for s in range(P):
            sl = slice(s * stride, s * stride + n)
            assert _same(state[s:s + 1], states[s]), (t, s)
            for key in "pmve":
                assert _same(multi[key][sl], single[s][key][:n]), (kind, t, s, key)
        assert [r["skip"] for r in recs] == [0, 1 if t == 1 else 0, 0]
        if zero_grad:
            assert not g.any()


def _stop_records(P, stopped):   # (tests/test_ema_gpu.py::_stop_records)
    state = torch.zeros(P, 6, dtype=torch.int32)
    state[:, 5] = -1
    for slot, k in stopped.items():
        state[slot, 5] = k
    return state.to(DEV)


def test_a_frozen_slot_keeps_its_record_and_its_arenas():
    """Slot 1 of 3 stopped at step index 0: the norm stages and the update of step 1 still see it, those of steps 2 and 3 leave its
    record, its arenas and its gradient alone."""
    kind, P, n, stride, c = 0, 3, 4100, 4160, 20.0
    gen = torch.Generator().manual_seed(17)
    p0 = torch.zeros(P, stride)
    p0[:, :n] = torch.randn(P, n, generator=gen)
    lrs = torch.tensor([1e-3, 2e-3, 5e-4], device=DEV)
    stop = _stop_records(P, {1: 0})
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    multi, state, part = _arenas(p0), _state(P), _partials(P, n)[0]
    frozen = None
    for t in (1, 2, 3):
        step_dev.fill_(t)
        g_h = torch.zeros(P, stride)
        g_h[:, :n] = torch.randn(P, n, generator=gen) * t
        g = _dev(g_h).clone()
        _norm(g, None, P, stride, n, c, part, state, stop, step_dev)
        _pairs_clip(kind, multi, g, P, stride, n, lrs, step_dev, stop, 1, state)
        torch.cuda.synchronize()
        recs = clip_records(state)
        sl1 = slice(stride, 2 * stride)
        for s in (0, 2) + ((1,) if t == 1 else ()):
            _check_record(recs[s], np_grad_clip(_np(g_h[s, :n]), None, c), c, (t, s))
        if t == 1:
            frozen = dict(rec=state[1].clone(), **{k: multi[k][sl1].clone() for k in "pmve"})
            assert not _same(frozen["p"], p0[1]) and recs[1]["clipped"] == 1 and not g[sl1].any()
        else:
            assert _same(state[1], frozen["rec"]) and all(_same(multi[k][sl1], frozen[k]) for k in "pmve"), t
            assert _same(g[sl1], g_h[1])                                                          # not even the gradient arena is written
        assert recs[0]["clipped"] == t and recs[2]["clipped"] == t


def test_invalid_arguments_are_refused():
    L = _lib.lib()
    g, part, state = torch.zeros(4352, device=DEV), torch.zeros(8, device=DEV), _state(2)
    s = _lib.current_stream()
    call = lambda c, P=1, stride=0, n=4, gp=g, pp=part, sp=state: L.splice_grad_norm_pairs(_lib.ptr(gp), None, P, stride, n, c, _lib.ptr(pp), _lib.ptr(sp), None, None, s)
    assert call(1.0) == 0
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(bad) != 0 and b"max_norm" in L.splice_last_error(), bad
    assert call(1.0, sp=None) != 0 and b"max_norm" in L.splice_last_error()
    assert call(1.0, pp=None) != 0 and call(1.0, gp=None) != 0 and call(1.0, n=0) != 0 and call(1.0, P=0) != 0
    assert call(1.0, P=2, stride=2174, n=2170) != 0 and b"multiple of 4" in L.splice_last_error()
    assert call(1.0, P=2, stride=8, n=12) != 0
    assert call(1.0, P=2, stride=2176, n=2170) == 0
    assert call(1.0, P=1, stride=3, n=7) == 0                                                     # one arena: the stride is not used
    stop, step_dev = _stop_records(2, {}), torch.ones(1, dtype=torch.int32, device=DEV)
    assert L.splice_grad_norm_pairs(_lib.ptr(g), None, 2, 2176, 2170, 1.0, _lib.ptr(part), _lib.ptr(state), _lib.ptr(stop), None, s) != 0
    assert L.splice_grad_norm_pairs(_lib.ptr(g), None, 2, 2176, 2170, 1.0, _lib.ptr(part), _lib.ptr(state), _lib.ptr(stop), _lib.ptr(step_dev), s) == 0
    p, m, v, lr = torch.zeros(4352, device=DEV), torch.zeros(4352, device=DEV), torch.zeros(4352, device=DEV), torch.ones(2, device=DEV)
    upd = lambda clip, P=2, stride=2176: L.splice_optim_step_pairs_clip(0, _lib.ptr(p), _lib.ptr(g), None, _lib.ptr(m), _lib.ptr(v), None, P, stride, 2170, _lib.ptr(lr),
                                                                        *HP[0], _lib.ptr(step_dev), None, 0, 0.0, 0, _lib.ptr(clip), s)
    assert upd(state) == 0 and upd(None) != 0 and upd(state, stride=2174) != 0
    assert L.splice_optim_step_clip(0, _lib.ptr(p), _lib.ptr(g), None, _lib.ptr(m), _lib.ptr(v), None, 4, LR, None, *HP[0], 1, 0, 0.0, 0, None, s) != 0
    torch.cuda.synchronize()


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


ONE = dict(cls_warmup=1, entire_A_every=4)
ONE_STEPS, ONE_EMA = 8, dict(ema_decay=0.5, ema_start=3)
_RUNS = {}


def _one_run(vit, clip, ema=False, graph=True):
    """8 steps of one pair (cached per setting); per step the arenas, buffers, losses, the average and the clip record."""
    key = (clip, ema, graph)
    if key in _RUNS:
        return _RUNS[key]
    eng = SpliceEngine(_cfg(**ONE, grad_clip_norm=clip, **(ONE_EMA if ema else {})), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    if not graph:
        _lib.check(_lib.lib().splice_step_use_graph(eng.handle, 0), "use_graph")
    A, B = _pair(62)
    init = eng.params.clone()
    snaps = []
    for _ in range(ONE_STEPS):
        eng.step(A, B, A)
        snaps.append(dict(params=eng.params.clone(), m=eng.m.clone(), v=eng.v.clone(), running=eng.running.clone(), losses=eng.losses_dev.clone(),
                          ema=eng.pair_ema().clone() if ema else None, rec=eng.clip_dev.clone() if clip else None))
    torch.cuda.synchronize()
    _RUNS[key] = (eng, init, snaps)
    return _RUNS[key]


def _half(vit):
    """Half the step-0 gradient norm of the one-pair run, as a float32 value."""
    _, _, snaps = _one_run(vit, HUGE)
    return float(F(0.5) * clip_records(snaps[0]["rec"])[0]["norm"])


@pytest.mark.parametrize("ema", [False, True])
def test_a_threshold_nothing_reaches_changes_no_bit(vit, ema):
    eng, init, snaps = _one_run(vit, HUGE, ema)
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    assert stats[0] + stats[2] >= 2                                   # graphs were in use (ordinary and entire-image variant)
    off, off_init, off_snaps = _one_run(vit, 0.0, ema)
    assert off.clip_dev is None and _same(init, off_init)
    with pytest.raises(RuntimeError, match="grad_clip_norm"):
        off.clip_state()
    for k, (a, b) in enumerate(zip(snaps, off_snaps)):
        for key in ("params", "m", "v", "running", "losses") + (("ema",) if ema else ()):
            assert _same(a[key], b[key]), (k, key)
        rec = clip_records(a["rec"])[0]
        assert 0 < rec["norm"] < np.inf and rec["coef"] == 1 and rec["skip"] == 0 and rec["clipped"] == 0 and rec["skipped"] == 0, (k, rec)
        assert rec["norm"].tobytes() == np.sqrt(rec["sumsq"]).tobytes()
    assert eng.clip_state() == clip_records(snaps[-1]["rec"])[0]


def test_half_the_first_norm_clips_and_step_0_is_exact(vit):
    c = _half(vit)
    eng, init, snaps = _one_run(vit, c)
    _, _, off_snaps = _one_run(vit, 0.0)
    recs = [clip_records(s["rec"])[0] for s in snaps]
    assert recs[0]["coef"] < 1 and recs[-1]["clipped"] >= 1 and recs[-1]["skipped"] == 0
    assert recs[-1]["clipped"] == sum(r["coef"] < 1 for r in recs)
    for k, r in enumerate(recs):
        assert r["coef"].tobytes() == np.minimum(F(1), F(c) / (r["norm"] + F(1e-6))).tobytes() and r["norm"].tobytes() == np.sqrt(r["sumsq"]).tobytes(), k
    assert not _same(snaps[0]["params"], off_snaps[0]["params"])
    # step 0 by hand: its gradient from a second handle in gradient-only mode, then the two exported calls on a copy of the initial arenas
    L = _lib.lib()
    grad_only = SpliceEngine(_cfg(**ONE), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    _lib.check(L.splice_step_set_mode(grad_only.handle, 1, 0), "step_set_mode")
    A, B = _pair(62)
    grad_only.step(A, B, A)
    torch.cuda.synchronize()
    assert _same(grad_only.params, init)
    n = eng.gen.numel
    g = grad_only.grads.clone()
    _check_record(recs[0], np_grad_clip(_np(g), None, c), c, "step 0")
    p, m, v, state = init.clone(), torch.zeros_like(init), torch.zeros_like(init), _state()
    part = _partials(1, n)[0]
    lr_dev, step_dev = torch.tensor([eng.cfg["lr"]], device=DEV), torch.ones(1, dtype=torch.int32, device=DEV)
    _norm(g, None, 1, 0, n, c, part, state)
    _lib.check(L.splice_optim_step_pairs_clip(0, _lib.ptr(p), _lib.ptr(g), None, _lib.ptr(m), _lib.ptr(v), None, 1, 0, n, _lib.ptr(lr_dev), eng.cfg["optimizer_beta1"],
                                              eng.cfg["optimizer_beta2"], 1e-8, _lib.ptr(step_dev), None, 0, 0.0, 0, _lib.ptr(state), _lib.current_stream()), "pairs_clip")
    torch.cuda.synchronize()
    assert _same(state, snaps[0]["rec"])
    assert _same(p, snaps[0]["params"]) and _same(m, snaps[0]["m"]) and _same(v, snaps[0]["v"])


def test_graph_replay_equals_eager(vit):
    c = _half(vit)
    _, _, snaps = _one_run(vit, c)
    _, _, eager = _one_run(vit, c, graph=False)
    for k, (a, b) in enumerate(zip(snaps, eager)):
        for key in ("params", "m", "v", "losses", "rec"):
            assert _same(a[key], b[key]), (k, key)


def test_three_pairs_equal_their_single_runs(vit):
    cfg = _cfg(cls_warmup=1, entire_A_every=4, grad_clip_norm=_half(vit))
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    imgs = [_pair(71, p) for p in range(3)]
    As, Bs = torch.stack([a for a, _ in imgs]).contiguous(), torch.stack([b for _, b in imgs]).contiguous()
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit)
    for _ in range(6):
        multi.step(As, Bs, As)
    recs = multi.clip_state()
    for p in range(3):
        single = SpliceEngine(cfg, None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for _ in range(6):
            single.step(imgs[p][0], imgs[p][1], imgs[p][0])
        torch.cuda.synchronize()
        assert _same(multi.pair_params(p), single.pair_params()), p
        assert _same(multi.clip_dev[p:p + 1], single.clip_dev) and multi.clip_state(p) == recs[p], p
    assert sum(r["clipped"] for r in recs) >= 1 and not _same(multi.clip_dev[0], multi.clip_dev[1])


# the settings of tests/test_ema_gpu.py::test_a_stopped_slot_keeps_the_average_of_its_stop_step
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2, stop_window=4)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 18


def test_a_stopped_slot_keeps_the_record_of_its_stop_step(vit):
    clip = dict(grad_clip_norm=_half(vit))
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    for rel in SLOT_RELS:
        multi = MultiPairEngine(_cfg(stop_rel=rel, **SLOTS, **clip), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
        for _ in range(SLOT_STEPS):
            multi.step(As, Bs, As)
        ks = multi.stopped_at
        if ks[1] is None and ks[0] is not None and ks[2] is not None:
            break
    # slots 0 and 2 stopped with steps to spare, slot 1 is still running: the case cannot pass vacuously
    assert ks[1] is None and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4, (rel, ks)
    for p in range(3):
        steps = SLOT_STEPS if ks[p] is None else ks[p] + 1
        single = SpliceEngine(dict(_cfg(lr=SLOT_LRS[p], **SLOTS, **clip), stop_window=0), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for _ in range(steps):
            single.step(A, B, A)
        torch.cuda.synchronize()
        assert _same(multi.pair_params(p), single.pair_params()), (rel, p)
        assert _same(multi.clip_dev[p:p + 1], single.clip_dev), (rel, p)
    assert multi.clip_state(1)["clipped"] >= 1


def test_multiscale_engine_clips_in_its_own_update(vit):
    def run(clip):
        eng = MultiScaleEngine(_cfg(cls_warmup=1, entire_A_every=2, grad_clip_norm=clip), None, synth.generator_params(84, 0.02), (64, 64), (64, 64),
                               scales=(64, 96), vit_engine=vit)
        A, B = _pair(76)
        recs = []
        for _ in range(4):
            eng.step(A, B, A)
            recs.append(eng.clip_state() if clip else None)
        torch.cuda.synchronize()
        return eng, recs
    off, _ = run(0.0)
    huge, huge_recs = run(HUGE)
    assert _same(huge.params, off.params) and _same(huge.engines[0].m, off.engines[0].m) and _same(huge.engines[0].v, off.engines[0].v)
    assert huge_recs[-1]["clipped"] == 0 and all(0 < r["norm"] < np.inf and r["coef"] == 1 for r in huge_recs)
    with pytest.raises(RuntimeError, match="grad_clip_norm"):
        off.clip_state()
    c = float(F(0.5) * huge_recs[0]["norm"])
    half, recs = run(c)
    assert recs[-1]["clipped"] >= 1 and recs[0]["sumsq"].tobytes() == huge_recs[0]["sumsq"].tobytes() and not _same(half.params, off.params)
    for r in recs:
        assert r["coef"].tobytes() == np.minimum(F(1), F(c) / (r["norm"] + F(1e-6))).tobytes() and r["norm"].tobytes() == np.sqrt(r["sumsq"]).tobytes()


def test_set_grad_clip_state_and_mode_refusals(vit):
    L = _lib.lib()
    eng = SpliceEngine(_cfg(), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    state = _state()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert L.splice_step_set_grad_clip(eng.handle, bad, _lib.ptr(state)) != 0 and b"max_norm" in L.splice_last_error(), bad
    assert L.splice_step_set_grad_clip(eng.handle, 1.0, None) != 0
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert L.splice_step_set_grad_clip(eng.handle, 1.0, _lib.ptr(state)) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    A, B = _pair(62)
    eng.step(A, B)
    assert L.splice_step_set_grad_clip(eng.handle, 1.0, _lib.ptr(state)) != 0 and b"before the first step" in L.splice_last_error()
    torch.cuda.synchronize()
    assert not state.any()                                        # never written
    on = SpliceEngine(_cfg(grad_clip_norm=1.0), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"gradient clipping" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 3, None) != 0 and b"gradient clipping" in L.splice_last_error()
    on.step(A, B)                                                 # (no entire-image branch on this handle: the rule runs there too)
    torch.cuda.synchronize()
    assert 0 < on.clip_state()["norm"] < np.inf


TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, use_augmentations=False,
             global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0, cls_warmup=1, entire_A_every=5, n_epochs=6)


def _write_pair(root, name):   # (tests/test_ema_gpu.py::_write_pair)
    from PIL import Image
    A, B = synth.smooth_image_pair(60, 0, 72, 72)
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


def test_train_model_reports_the_clipping_in_result_json(tmp_path):
    from splice_amd.batch import _write_result
    from splice_amd.train import clip_fields, train_model
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    engines = {}
    for name, clip in (("off", 0.0), ("huge", HUGE), ("tight", 1e-3)):
        torch.manual_seed(3)
        engines[name] = train_model(_write_pair(tmp_path, name), cfg_overrides=dict(TRAIN, grad_clip_norm=clip), vit_state=vit_state, progress=False)
        torch.cuda.synchronize()
        _write_result(str(tmp_path), name, dict(steps=engines[name].step_idx + 1, **clip_fields(engines[name])))   # (as splice_amd.batch.train_runner)
    res = {name: json.loads((tmp_path / name / "out" / "result.json").read_text()) for name in engines}
    assert res["off"] == dict(steps=6, grad_clip_norm=0.0, clipped_steps=0, skipped_steps=0)
    assert res["huge"] == dict(steps=6, grad_clip_norm=HUGE, clipped_steps=0, skipped_steps=0)
    assert res["tight"]["grad_clip_norm"] == 1e-3 and res["tight"]["clipped_steps"] == 6 and res["tight"]["skipped_steps"] == 0
    png = lambda name: (tmp_path / name / "out" / "output.png").read_bytes()
    assert png("huge") == png("off")
    assert _same(engines["huge"].params, engines["off"].params) and not _same(engines["tight"].params, engines["off"].params)
