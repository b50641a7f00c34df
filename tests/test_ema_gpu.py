"""GPU: the weight average kept inside the fused update.  The rule against its NumPy float32 restatement
(engine.np_ema) fed with the parameters read back after every update -- op level, per-pair and masked, inside the fused step under
graph replay and eagerly, beside neighbours, behind a plateau stop, in the several-scales engine -- and the image train_model writes
from it.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import MultiPairEngine, MultiScaleEngine, SpliceEngine, np_ema
from splice_amd.generator import GeneratorPlan, optim_step

pytestmark = pytest.mark.gpu
DEV = "cuda"
HP = {0: (0.5, 0.99, 1e-8), 1: (0.99, 0.0, 1e-8), 2: (0.0, 0.0, 0.0)}   # Adam betas / RMSprop alpha / SGD
KINDS = [0, 1, 2]
LR = 2e-3


def _np(t):
    return t.detach().cpu().numpy()


def _same(a, b):
    return _np(a).tobytes() == _np(b).tobytes()


# ------------------------------------------------------------------------------------------------------------------- op level
def _arenas(n, offset, seed):
    """p, m, v, e (e starts as p) and six gradient arenas of n floats; ``offset`` floats into their allocations."""
    g = torch.Generator().manual_seed(seed)
    def make(x):
        base = torch.zeros(n + offset, device=DEV)
        base[offset:] = x.to(DEV)
        return base[offset:]
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) * (0.5 + k) for k in range(6)]
    return p0, make, grads


@pytest.mark.parametrize("n,offset", [(1, 0), (3, 0), (4, 0), (1027, 0), (1027, 1)])
@pytest.mark.parametrize("kind", KINDS)
def test_op_equals_numpy_restatement(kind, n, offset):
    """6 consecutive updates, ema_start 2, decay 0.9.  n = 1027: the float4 body and the scalar tail; offset 1: every arena off its
    16-byte alignment, the whole call on the scalar path."""
    L = _lib.lib()
    d, start = 0.9, 2
    p0, make, grads = _arenas(n, offset, 100 + n)
    pa, ma, va, ea = make(p0), make(torch.zeros(n)), make(torch.zeros(n)), make(p0)      # with the average
    pb, mb, vb = make(p0), make(torch.zeros(n)), make(torch.zeros(n))                    # the same calls without it
    assert pa.data_ptr() % 16 == (4 * offset) % 16
    e_np = _np(ea).copy()
    for k in range(6):
        ga, gb = make(grads[k]), make(grads[k])
        _lib.check(L.splice_optim_step_ema(kind, _lib.ptr(pa), _lib.ptr(ga), None, _lib.ptr(ma), _lib.ptr(va), _lib.ptr(ea), n, LR, None, *HP[kind], k + 1, 0,
                                           d, start, _lib.current_stream()), "optim_step_ema")
        _lib.check(L.splice_optim_step_ex(kind, _lib.ptr(pb), _lib.ptr(gb), None, _lib.ptr(mb), _lib.ptr(vb), n, LR, None, *HP[kind], k + 1, 0,
                                          _lib.current_stream()), "optim_step_ex")
        torch.cuda.synchronize()
        assert _same(pa, pb) and _same(ma, mb) and _same(va, vb), (kind, n, offset, k)
        assert not _same(pa, make(p0))
        e_np = np_ema(e_np, _np(pa), k + 1, d, start)
        assert _np(ea).tobytes() == e_np.tobytes(), (kind, n, offset, k)
        if k + 1 <= start:
            assert _same(ea, pa)
    assert not _same(ea, pa)                                                              # (the average did leave the weights)


def test_optim_step_wrapper_passes_the_average():
    n = 1027
    p0, make, grads = _arenas(n, 0, 7)
    p, m, v, e, g = make(p0), make(torch.zeros(n)), make(torch.zeros(n)), make(p0), make(grads[0])
    optim_step(1, p, g, m, v, LR, *HP[1], 1, ema=e, ema_decay=0.9, ema_start=0)
    torch.cuda.synchronize()
    assert _np(e).tobytes() == np_ema(_np(p0), _np(p), 1, 0.9, 0).tobytes() and not _same(e, p)


def _stop_records(P, stopped):
    """[P] splice_stop_state records as the step handle starts them (zeros, stop_step -1), slot -> stop step of ``stopped`` set."""
    state = torch.zeros(P, 6, dtype=torch.int32)
    state[:, 5] = -1
    for slot, k in stopped.items():
        state[slot, 5] = k
    return state.to(DEV)


@pytest.mark.parametrize("kind", KINDS)
def test_pairs_masked_slot_is_skipped_and_neighbours_equal_their_single_calls(kind):
    """3 arenas of stride 1088 (n = 1027), per-pair lrs, slot 1 stopped at step index 0: update 1 still applies to it, updates 2 .. 5
    find it frozen -- e, p, m, v AND its gradient arena stay what they were.  Slots 0 and 2 equal their own one-arena calls."""
    L = _lib.lib()
    P, n, stride, d, start = 3, 1027, 1088, 0.9, 2
    gen = torch.Generator().manual_seed(31 + kind)
    p0 = torch.zeros(P, stride)
    p0[:, :n] = torch.randn(P, n, generator=gen)
    lrs = torch.tensor([1e-3, 2e-3, 5e-4], device=DEV)
    stop = _stop_records(P, {1: 0})
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    multi = dict(p=p0.to(DEV).reshape(-1).clone(), m=torch.zeros(P * stride, device=DEV), v=torch.zeros(P * stride, device=DEV))
    multi["e"] = multi["p"].clone()
    single = [dict(p=p0[s].to(DEV).clone(), m=torch.zeros(stride, device=DEV), v=torch.zeros(stride, device=DEV), e=p0[s].to(DEV).clone()) for s in range(P)]
    frozen = None
    e_np = {s: _np(p0[s]) for s in (0, 2)}
    for t in range(1, 6):
        step_dev.fill_(t)
        g = torch.zeros(P, stride)
        g[:, :n] = torch.randn(P, n, generator=gen)
        gm = g.to(DEV).reshape(-1).clone()
        _lib.check(L.splice_optim_step_pairs_ema(kind, _lib.ptr(multi["p"]), _lib.ptr(gm), None, _lib.ptr(multi["m"]), _lib.ptr(multi["v"]), _lib.ptr(multi["e"]), P, stride,
                                                 n, _lib.ptr(lrs), *HP[kind], _lib.ptr(step_dev), _lib.ptr(stop), 1, d, start, _lib.current_stream()), "pairs_ema")
        for s in range(P):
            if s == 1 and t > 1:
                continue
            a, gs = single[s], g[s].to(DEV).clone()
            _lib.check(L.splice_optim_step_pairs_ema(kind, _lib.ptr(a["p"]), _lib.ptr(gs), None, _lib.ptr(a["m"]), _lib.ptr(a["v"]), _lib.ptr(a["e"]), 1, stride, n,
                                                     _lib.ptr(lrs[s:s + 1]), *HP[kind], _lib.ptr(step_dev), None, 1, d, start, _lib.current_stream()), "single_ema")
        torch.cuda.synchronize()
        sl1 = slice(stride, 2 * stride)
        if t == 1:
            frozen = {k: multi[k][sl1].clone() for k in "pmve"}
            assert not gm[sl1].any()                                       # zero_grad reached the slot at its stop step
        else:
            assert all(_same(multi[k][sl1], frozen[k]) for k in "pmve"), (kind, t)
            assert _same(gm[sl1], g[1].to(DEV))                            # not even the gradient arena is written
        for s in range(P):
            sl = slice(s * stride, (s + 1) * stride)
            assert all(_same(multi[k][sl], single[s][k]) for k in "pmve"), (kind, t, s)
        for s in (0, 2):                                                   # ... and those follow the restatement
            e_np[s] = np_ema(e_np[s], _np(single[s]["p"]), t, d, start)
            assert _np(single[s]["e"]).tobytes() == e_np[s].tobytes(), (kind, t, s)
    assert not _same(multi["e"][:n], multi["p"][:n]) and not _same(single[1]["p"], p0[1].to(DEV))
    assert _same(multi["e"][stride + n:2 * stride], torch.zeros(stride - n, device=DEV))   # padding: zero weights, zero average


def test_invalid_arguments_are_refused():
    L = _lib.lib()
    t = [torch.zeros(4, device=DEV) for _ in range(5)]
    p, g, m, v, e = (_lib.ptr(x) for x in t)
    s = _lib.current_stream()
    call = lambda kind, decay, start, step, ema=e: L.splice_optim_step_ema(kind, p, g, None, m, v, ema, 4, LR, None, *HP[kind], step, 0, decay, start, s)
    assert call(0, 0.9, 0, 1) == 0
    assert call(0, 0.0, 0, 1) != 0 and b"ema_decay" in L.splice_last_error()
    assert call(0, 1.0, 0, 1) != 0 and call(1, 0.9, -1, 1) != 0
    assert call(2, 0.9, 0, 0) != 0 and b"step count" in L.splice_last_error()   # SGD reads no count of its own: the average needs one
    assert call(2, 0.9, 0, 1) == 0 and call(2, 0.9, 0, 1, None) != 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the engine
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


ONE = dict(cls_warmup=1, entire_A_every=4)
ONE_STEPS, ONE_EMA = 8, dict(ema_decay=0.5, ema_start=3)


def _one_run(vit, ema, graph=True):
    """8 steps of one pair; per step the arenas, buffers and losses (and the average)."""
    eng = SpliceEngine(_cfg(**ONE, **(ONE_EMA if ema else {})), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    if not graph:
        _lib.check(_lib.lib().splice_step_use_graph(eng.handle, 0), "use_graph")
    A, B = _pair(62)
    init = eng.params.clone()
    snaps = []
    for _ in range(ONE_STEPS):
        eng.step(A, B, A)
        snaps.append(dict(params=eng.params.clone(), m=eng.m.clone(), v=eng.v.clone(), running=eng.running.clone(), losses=eng.losses_dev.clone(),
                          ema=eng.pair_ema().clone() if ema else None))
    torch.cuda.synchronize()
    return eng, init, snaps


@pytest.fixture(scope="module")
def one_on(vit):
    return _one_run(vit, True)


def test_engine_average_equals_restatement_and_changes_nothing_else(vit, one_on):
    eng, init, snaps = one_on
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    assert stats[0] + stats[2] >= 2                                   # graphs were in use (ordinary and entire-image variant)
    off, off_init, off_snaps = _one_run(vit, False)
    assert off.ema is None and _same(init, off_init)
    with pytest.raises(RuntimeError, match="ema_decay"):
        off.pair_ema()
    e_np = _np(init)
    for k, (a, b) in enumerate(zip(snaps, off_snaps)):
        for key in ("params", "m", "v", "running", "losses"):
            assert _same(a[key], b[key]), (k, key)
        e_np = np_ema(e_np, _np(a["params"]), k + 1, ONE_EMA["ema_decay"], ONE_EMA["ema_start"])
        assert _np(a["ema"]).tobytes() == e_np.tobytes(), k
    assert _same(snaps[2]["ema"], snaps[2]["params"]) and not _same(snaps[-1]["ema"], snaps[-1]["params"])


def test_engine_graph_replay_equals_eager(vit, one_on):
    _, _, snaps = one_on
    _, _, eager = _one_run(vit, True, graph=False)
    for k, (a, b) in enumerate(zip(snaps, eager)):
        for key in ("params", "ema", "losses"):
            assert _same(a[key], b[key]), (k, key)


def test_three_pairs_equal_their_single_runs(vit):
    cfg = _cfg(cls_warmup=1, entire_A_every=4, ema_decay=0.9, ema_start=2)
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    imgs = [_pair(71, p) for p in range(3)]
    As, Bs = torch.stack([a for a, _ in imgs]).contiguous(), torch.stack([b for _, b in imgs]).contiguous()
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit)
    for _ in range(6):
        multi.step(As, Bs, As)
    for p in range(3):
        single = SpliceEngine(cfg, None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for _ in range(6):
            single.step(imgs[p][0], imgs[p][1], imgs[p][0])
        torch.cuda.synchronize()
        assert _same(multi.pair_params(p), single.pair_params()) and _same(multi.pair_ema(p), single.pair_ema()), p
        assert not _same(single.pair_ema(), single.pair_params())
    assert multi.pair_ema(1).numel() == multi.gen.numel and not _same(multi.pair_ema(0), multi.pair_ema(1))


# the settings of tests/test_stop_gpu.py::test_slots_stop_alone_and_leave_neighbours_untouched: slots 0 and 2 (lr 0 and 1e-6) cannot
# improve by stop_rel and stop at the close of their third window, slot 1 learns.  stop_rel is the first of SLOT_RELS under which the
# engine shows that picture.
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2, stop_window=4)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 18


def test_a_stopped_slot_keeps_the_average_of_its_stop_step(vit):
    ema = dict(ema_decay=0.9, ema_start=2)
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    for rel in SLOT_RELS:
        multi = MultiPairEngine(_cfg(stop_rel=rel, **SLOTS, **ema), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
        for _ in range(SLOT_STEPS):
            multi.step(As, Bs, As)
        ks = multi.stopped_at
        if ks[1] is None and ks[0] is not None and ks[2] is not None:
            break
    # slots 0 and 2 stopped with steps to spare, slot 1 is still running: the case cannot pass vacuously
    assert ks[1] is None and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4, (rel, ks)
    for p in range(3):
        steps = SLOT_STEPS if ks[p] is None else ks[p] + 1
        single = SpliceEngine(dict(_cfg(lr=SLOT_LRS[p], **SLOTS, **ema), stop_window=0), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for _ in range(steps):
            single.step(A, B, A)
        torch.cuda.synchronize()
        assert _same(multi.pair_params(p), single.pair_params()), (rel, p)
        assert _same(multi.pair_ema(p), single.pair_ema()), (rel, p)
    assert not _same(multi.pair_ema(2), multi.pair_params(2))   # (lr 1e-6 moves the weights: the average trails them)


def test_generate_with_the_average_books_nothing(vit, one_on):
    eng, _, _ = one_on
    A, _ = _pair(62)
    running, calls, logged = eng.running.clone(), list(eng.generator_calls), list(getattr(eng, "_logged", []))
    out = eng.generate(A[None], ema=True)
    torch.cuda.synchronize()
    assert _same(eng.running, running) and eng.generator_calls == calls and list(getattr(eng, "_logged", [])) == logged
    want = GeneratorPlan(eng.gen, 1, 64, 64, False).forward(eng.pair_ema().clone(), A[None].contiguous())
    live = eng.generate(A[None], track_running_stats=False)
    eng._logged = logged                                         # (the live call above joined the logged forwards: undo, the fixture is shared)
    assert _same(out, want) and not _same(out, live)
    sd, sd_live = eng.state_dict(ema=True), eng.state_dict()
    flat = eng.gen.flatten({k: v for k, v in sd.items() if k in eng.gen.table})
    assert _same(flat, eng.pair_ema())
    for name in eng.gen.buffer_table:
        assert _same(sd[name], sd_live[name])                    # the live buffers


def test_set_ema_state_and_mode_refusals(vit):
    L = _lib.lib()
    eng = SpliceEngine(_cfg(), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    ema = eng.params.clone()
    ema0 = ema.clone()
    assert L.splice_step_set_ema(eng.handle, _lib.ptr(ema), 0.0, 0) != 0 and L.splice_step_set_ema(eng.handle, _lib.ptr(ema), 1.0, 0) != 0
    assert L.splice_step_set_ema(eng.handle, _lib.ptr(ema), 0.5, -1) != 0 and L.splice_step_set_ema(eng.handle, None, 0.5, 0) != 0
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert L.splice_step_set_ema(eng.handle, _lib.ptr(ema), 0.5, 0) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    A, B = _pair(62)
    eng.step(A, B)
    assert L.splice_step_set_ema(eng.handle, _lib.ptr(ema), 0.5, 0) != 0 and b"before the first step" in L.splice_last_error()
    torch.cuda.synchronize()
    assert _same(ema, ema0) and not _same(eng.params, ema0)   # never written
    on = SpliceEngine(_cfg(ema_decay=0.5), None, synth.generator_params(61, 0.02), (64, 64), None, vit_engine=vit)
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"weight average" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 3, None) != 0 and b"weight average" in L.splice_last_error()


def test_multiscale_engine_keeps_the_average_in_its_own_update(vit):
    d, start = 0.9, 1
    eng = MultiScaleEngine(_cfg(cls_warmup=1, entire_A_every=2, ema_decay=d, ema_start=start), None, synth.generator_params(84, 0.02), (64, 64), (64, 64),
                           scales=(64, 96), vit_engine=vit)
    A, B = _pair(76)
    e_np = _np(eng.params)
    assert _same(eng.ema, eng.params) and eng.ema.data_ptr() != eng.params.data_ptr()
    for k in range(4):
        eng.step(A, B, A)
        torch.cuda.synchronize()
        e_np = np_ema(e_np, _np(eng.params), k + 1, d, start)
        assert _np(eng.pair_ema()).tobytes() == e_np.tobytes(), k
    assert not _same(eng.pair_ema(), eng.engines[0].pair_params())
    assert eng.generate(A[None], ema=True).shape == (1, 3, 64, 64)


TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, use_augmentations=False,
             global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0, cls_warmup=1, entire_A_every=5, n_epochs=6)


def _write_pair(root, name):   # (tests/test_stop_gpu.py::_write_pair)
    from PIL import Image
    A, B = synth.smooth_image_pair(60, 0, 72, 72)
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


def test_train_model_writes_the_averaged_image(tmp_path):
    from splice_amd.train import train_model
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    seen = []
    torch.manual_seed(3)
    on = train_model(_write_pair(tmp_path, "on"), callback=lambda im: seen.append(tuple(im.shape)), cfg_overrides=dict(TRAIN, ema_decay=0.5, ema_start=2),
                     vit_state=vit_state, progress=False)
    torch.manual_seed(3)
    off = train_model(_write_pair(tmp_path, "off"), cfg_overrides=TRAIN, vit_state=vit_state, progress=False)
    assert seen == [(3, 72, 72)]                                  # epoch 4 only: the averaged image is not a callback
    assert (tmp_path / "on" / "out" / "output_ema.png").exists() and not (tmp_path / "off" / "out" / "output_ema.png").exists()
    png = lambda name, f: (tmp_path / name / "out" / f).read_bytes()
    assert png("on", "output.png") == png("off", "output.png")
    assert png("on", "output_ema.png") != png("on", "output.png")
    assert _same(on.params, off.params) and _same(on.running, off.running) and on.generator_calls == off.generator_calls
    assert not _same(on.pair_ema(), on.pair_params())
