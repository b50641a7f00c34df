"""GPU: the per-step loss trace.  The loss kernel's TRACE instances alone; then the engine: words 0-5 of row s are the
bits of the losses row step s reported, words 6-7 the bits of its clip record, under graph replay, beside the stop rule, in a sweep and
with several crops; the run itself -- parameters, moments, BatchNorm buffers, losses -- is bit for bit the run without the key; and
train_model / train_sweep end by writing losses.csv.  Every comparison is exact."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import DEFAULT_CFG, LOSS_KEYS, MultiPairEngine, SpliceEngine, np_plateau, stop_window_closes
from splice_amd.util import LrSchedule

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL = np.float32(np.nan).view(np.uint32)   # the bits torch.full(..., nan) writes


def _bits(t):
    """uint32 view of a float32 tensor / array on the host (NaN rows compare by their bits)."""
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------- 1: the kernel alone
P1, LP, LSTRIDE, CAP = 3, 70, 8 + 6 * 70 + 4, 5
WEIGHTS = (1.0, 0.5, 10.0, 10.0, 2.0)   # w_ssim, w_essim, w_ecls, w_cls, w_id


def _total_trace(step_count, stop=None, ssim_on=1, entire=1):
    g = torch.Generator().manual_seed(5)
    lbase = torch.rand(P1, LSTRIDE, generator=g).to(DEV)
    out8 = torch.full((P1, 8), 7.0, device=DEV)
    trace = torch.full((CAP, P1, 8), float("nan"), device=DEV)
    dev_t = torch.tensor([step_count, 0, 0, 0], dtype=torch.int32, device=DEV)
    _lib.check(_lib.lib().splice_total_loss_pairs_trace(_lib.ptr(lbase), LSTRIDE, LP, *WEIGHTS, _lib.ptr(out8), P1, 1, 1, 1, 1, None, ssim_on, entire,
                                                        _lib.ptr(stop), 3, 0.5, 1, 0, _lib.ptr(dev_t), _lib.ptr(trace), CAP, _lib.current_stream()), "total_loss_pairs_trace")
    torch.cuda.synchronize()
    return _bits(out8), _bits(trace), lbase


def test_kernel_alone_writes_its_row_and_nothing_else():
    out8, trace, lbase = _total_trace(3)
    # (the out8 row is what splice_total_loss_pairs writes: the TRACE instance changes none of it)
    plain, again = torch.full((P1, 8), 7.0, device=DEV), lbase.clone()
    _lib.check(_lib.lib().splice_total_loss_pairs(_lib.ptr(again), LSTRIDE, LP, *WEIGHTS, _lib.ptr(plain), P1, 1, 1, 1, 1, None, 1, 1, _lib.current_stream()),
               "total_loss_pairs")
    assert np.array_equal(_bits(plain), out8) and np.all(out8[:, :6] != FILL) and len({tuple(r) for r in out8[:, :6]}) == P1
    for p in range(P1):
        assert trace[2, p, :6].tobytes() == out8[p, :6].tobytes(), p
    assert np.all(trace[2, :, 6:] == FILL)                               # words 6-7 are the clip kernel's
    assert np.all(trace[[0, 1, 3, 4]] == FILL)                           # every other row still holds the fill


def test_kernel_alone_beyond_capacity_writes_nothing():
    out8, trace, _ = _total_trace(CAP + 1)
    assert np.all(trace == FILL) and np.all(out8[:, :6] != FILL)
    _, trace, _ = _total_trace(CAP)                                      # the last row that fits
    assert np.all(trace[CAP - 1, :, :6] != FILL) and np.all(trace[:CAP - 1] == FILL)


@pytest.mark.parametrize("ssim_on,entire", [(1, 0), (1, 1)])            # a counted step (the rule runs behind the store) and one that is not
def test_kernel_alone_leaves_a_stopped_slot_out(ssim_on, entire):
    stop = torch.zeros(P1, 6, dtype=torch.int32, device=DEV)
    stop[:, 5] = torch.tensor([-1, 0, 2], dtype=torch.int32)            # slot 1 stopped at step 0; slot 2 stops at THIS step (index 2): still written
    out8, trace, _ = _total_trace(3, stop=stop, ssim_on=ssim_on, entire=entire)
    assert np.all(trace[2, 1] == FILL)
    for p in (0, 2):
        assert trace[2, p, :6].tobytes() == out8[p, :6].tobytes(), p
    assert np.all(trace[[0, 1, 3, 4]] == FILL) and np.all(trace[2, :, 6:] == FILL)
    L = _lib.lib()
    zeros = torch.zeros(P1, LSTRIDE, device=DEV)
    args = lambda **kw: (_lib.ptr(zeros), LSTRIDE, LP, *WEIGHTS, None, P1, 1, 1, 1, 1, None, 1, 0, kw.get("stop"), kw.get("window", 3), 0.5, 1, 0,
                         kw.get("dev_t", _lib.ptr(stop)), kw.get("trace", _lib.ptr(stop)), kw.get("cap", CAP), _lib.current_stream())
    assert L.splice_total_loss_pairs_trace(*args(trace=None)) != 0 and L.splice_total_loss_pairs_trace(*args(dev_t=None)) != 0
    assert L.splice_total_loss_pairs_trace(*args(cap=0)) != 0 and L.splice_total_loss_pairs_trace(*args(stop=_lib.ptr(stop), window=0)) != 0


# --------------------------------------------------------------------------------------------------------------- the engine
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


REGIMES = dict(cls_warmup=2, entire_A_every=3)   # ten steps cross warm-up (0 1), entire-image (0 3 6 9) and ordinary steps
STEPS = 10


def _cfg(**over):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **dict(dict(REGIMES, n_epochs=STEPS), **over))


def _pair(seed, pair=0):
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _arenas(eng, pair=0):
    n, st = eng.gen.numel, eng.stride
    sl = slice(pair * st, pair * st + n)
    return dict(params=eng.params[sl].clone(), m=eng.m[sl].clone(), v=eng.v[sl].clone(), running=eng.running[pair].clone(), losses=eng.losses_dev[pair].clone())


def _same(a, b, what=()):
    for k in a:
        assert torch.equal(a[k], b[k]), what + (k,)


def _run(eng, steps, step_fn, after=None):
    """`steps` steps; the [steps, P, 8] loss rows every step reported (clones on the device, one copy at the end)."""
    hist = []
    for k in range(steps):
        step_fn(eng)
        hist.append(eng.losses_dev.clone())
        if after:
            after(eng, k)
    torch.cuda.synchronize()
    return _bits(torch.stack(hist))


def _one(vit, steps=STEPS, graph=True, **over):
    eng = SpliceEngine(_cfg(**over), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    if not graph:
        _lib.check(_lib.lib().splice_step_use_graph(eng.handle, 0), "use_graph")
    A, B = _pair(62)
    return eng, _run(eng, steps, lambda e: e.step(A, B, A))


@pytest.fixture(scope="module")
def eager_on(vit):
    return _one(vit, graph=False, loss_trace=True)


def test_off_engine_has_no_trace(vit):
    eng = SpliceEngine(_cfg(), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    assert eng.trace_dev is None
    with pytest.raises(RuntimeError, match="loss_trace"):
        eng.loss_trace()


def test_one_pair_eager_trace_is_the_loss_rows_and_the_run_is_unchanged(vit, eager_on):
    eng, rows = eager_on
    trace = eng.loss_trace()
    assert trace.dtype == np.float32 and trace.shape == (STEPS, 8)
    assert _bits(trace)[:, :6].tobytes() == rows[:, 0, :6].tobytes()
    assert np.all(_bits(trace)[:, 6:] == FILL)                           # no clipping: words 6-7 keep the fill
    # the three regimes were crossed: a term that is off reports 0
    ssim, essim = LOSS_KEYS.index("loss_global_ssim"), LOSS_KEYS.index("loss_entire_ssim")
    assert [bool(trace[s, ssim]) for s in range(4)] == [False, False, True, True] and [bool(trace[s, essim]) for s in range(4)] == [True, False, False, True]
    off, off_rows = _one(vit, graph=False)
    assert off_rows.tobytes() == rows.tobytes()
    _same(_arenas(eng), _arenas(off))
    assert eng.losses() == off.losses()


def test_graph_replay_writes_every_steps_own_row(vit, eager_on):
    eager, rows = eager_on
    eng, grows = _one(vit, graph=True, loss_trace=True)
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    captures = stats[0] + stats[2]
    # graphs from the third step on: STEPS - 2 steps went through an executable, fewer executables than that were made -- the others replayed
    assert 1 <= captures < STEPS - 2, list(stats)
    assert grows.tobytes() == rows.tobytes()
    assert _bits(eng.loss_trace()).tobytes() == _bits(eager.loss_trace()).tobytes()
    assert _bits(eng.trace_dev).tobytes() == _bits(eager.trace_dev).tobytes()
    _same(_arenas(eng), _arenas(eager))


# 4: the construction of tests/test_stop_gpu.py::test_slots_stop_alone_and_leave_neighbours_untouched: slots 0 and 2 (lr 0 and 1e-6) cannot
# improve by stop_rel and stop; slot 1 learns.  stop_rel / window are the first of the lists under which the NumPy rule says so on the
# slots' own single runs.
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_WINDOWS = (4, 3)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 18


def test_slots_with_the_stop_rule_trace_as_alone_cut_at_the_stop(vit):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    singles = []
    for p, lr in enumerate(SLOT_LRS):
        single = SpliceEngine(_cfg(lr=lr, n_epochs=SLOT_STEPS, loss_trace=True, **SLOTS), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        _run(single, SLOT_STEPS, lambda e: e.step(A, B, A))
        singles.append(single.loss_trace())
    counted = [stop_window_closes(k, 1, SLOTS["cls_warmup"], SLOTS["entire_A_every"]) for k in range(SLOT_STEPS)]

    def verdicts():
        for window in SLOT_WINDOWS:
            for rel in SLOT_RELS:
                ks = [np_plateau(t[:, 0], counted, window, rel, SLOTS["stop_patience"], 0)["stop_step"] for t in singles]
                if ks[1] == -1 and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4:
                    return window, rel, ks
        return window, rel, ks
    window, rel, ks = verdicts()
    assert ks[1] == -1 and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4, (window, rel, ks)
    multi = MultiPairEngine(_cfg(n_epochs=SLOT_STEPS, loss_trace=True, stop_window=window, stop_rel=rel, **SLOTS), None, gens, (64, 64), (64, 64), vit_engine=vit,
                            pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
    _run(multi, SLOT_STEPS, lambda e: e.step(As, Bs, As))
    assert multi.stopped_at == [ks[0], None, ks[2]]
    traces = multi.loss_trace()
    dev = _bits(multi.trace_dev)
    for p, k in enumerate(ks):
        rows = SLOT_STEPS if k < 0 else k + 1
        assert traces[p].shape == (rows, 8) and _bits(traces[p]).tobytes() == _bits(singles[p][:rows]).tobytes(), p
        assert _bits(multi.loss_trace(p)).tobytes() == _bits(traces[p]).tobytes()
        if k >= 0:   # on the device: the stop step's row is written, nothing behind it
            assert np.all(dev[k + 1:, p] == FILL) and np.all(dev[k, p, :6] != FILL), p
        else:
            assert np.all(dev[:, p, :6] != FILL)


def test_clipping_fills_words_six_and_seven(vit):
    seen = []

    def after(e, k):
        seen.append(e.clip_state())   # (a synchronising copy per step: this test only)
    eng = SpliceEngine(_cfg(loss_trace=True, grad_clip_norm=1e-3), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    A, B = _pair(62)
    rows = _run(eng, 6, lambda e: e.step(A, B, A), after)
    trace = eng.loss_trace()
    assert trace.shape == (6, 8) and _bits(trace)[:, :6].tobytes() == rows[:, 0, :6].tobytes()
    for s, rec in enumerate(seen):
        assert _bits(trace[s, 6]) == _bits(rec["norm"]) and _bits(trace[s, 7]) == _bits(rec["coef"]), (s, trace[s], rec)
    assert any(rec["coef"] < 1 for rec in seen) and all(rec["norm"] > 0 for rec in seen)   # the clip bit: the coefficient is no constant 1
    assert np.all(_bits(eng.trace_dev)[6:] == FILL)
    # the clipped run itself is the clipped run without the key
    off = SpliceEngine(_cfg(grad_clip_norm=1e-3), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    off_rows = _run(off, 6, lambda e: e.step(A, B, A))
    assert off_rows.tobytes() == rows.tobytes() and off.clip_state() == eng.clip_state()
    _same(_arenas(eng), _arenas(off))


def test_clipping_beside_the_stop_rule_and_graph_replay(vit):
    """Two slots, clipping, the stop rule and the trace together under graph replay: the clip kernel's words follow the frozen slot's
    rule as the loss kernel's do."""
    gens = [synth.generator_params(70 + p, 0.02) for p in range(2)]
    A, B = _pair(71)
    As, Bs = A[None].expand(2, -1, -1, -1).contiguous(), B[None].expand(2, -1, -1, -1).contiguous()
    cfg = _cfg(n_epochs=14, loss_trace=True, grad_clip_norm=1e-3, cls_warmup=1, entire_A_every=7, stop_window=3, stop_patience=1, stop_rel=0.5)
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=0.0), dict(lr=2e-3)])
    rows = _run(multi, 14, lambda e: e.step(As, Bs, As))
    k = multi.stopped_at[0]
    assert k is not None and k < 12                                      # the slot that cannot learn stopped with steps to spare
    dev = _bits(multi.trace_dev)
    assert np.all(dev[k + 1:, 0] == FILL) and np.all(dev[:k + 1, 0] != FILL)
    live = 14 if multi.stopped_at[1] is None else multi.stopped_at[1] + 1
    assert np.all(dev[:live, 1] != FILL)
    for p, n in ((0, k + 1), (1, live)):
        assert dev[:n, p, :6].tobytes() == rows[:n, p, :6].tobytes()
    rec = multi.clip_state(0)                                            # the frozen slot's record is that of its stop step
    assert dev[k, 0, 6] == _bits(rec["norm"]) and dev[k, 0, 7] == _bits(rec["coef"])


def test_sweep_slots_trace_their_own_loss_rows(vit):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(2)]
    A, B = _pair(71)
    As, Bs = A[None].expand(2, -1, -1, -1).contiguous(), B[None].expand(2, -1, -1, -1).contiguous()
    variants = [dict(lr=0.002), dict(lr=0.004, lambda_global_ssim=2.0, lambda_global_identity=0.0, lambda_entire_cls=5)]
    multi = MultiPairEngine(_cfg(loss_trace=True), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=variants)
    assert multi._pair_lambdas and multi._pair_lr                        # the wtab path
    rows = _run(multi, STEPS, lambda e: e.step(As, Bs, As))
    traces = multi.loss_trace()
    for p in range(2):
        assert _bits(traces[p])[:, :6].tobytes() == rows[:, p, :6].tobytes(), p
    assert not np.array_equal(traces[0][:, 0], traces[1][:, 0])
    cols = multi.loss_trace_columns()
    assert [lrs for _, lrs, _ in cols] == [[0.002] * STEPS, [0.004] * STEPS]
    assert not any(act["loss_global_id_B"] for act in cols[1][2]) and cols[0][2][2]["loss_global_id_B"]


def test_pairs_with_crops_trace_their_loss_rows(vit):
    gens = [synth.generator_params(80, 0.02), synth.generator_params(81, 0.1)]
    imgs = [_pair(82, p) for p in range(2)]
    crops = lambda img: torch.stack([img, img.flip(-1)]).contiguous()
    A_all = torch.cat([crops(a) for a, _ in imgs]).contiguous()
    B_all = torch.cat([crops(b) for _, b in imgs]).contiguous()
    E_all = torch.stack([a for a, _ in imgs]).contiguous()
    multi = MultiPairEngine(_cfg(loss_trace=True), None, gens, (64, 64), (64, 64), vit_engine=vit, n_crops=2)
    rows = _run(multi, STEPS, lambda e: e.step(A_all, B_all, E_all))
    assert multi.trace_dev.shape == (STEPS, 2, 8)
    for p, t in enumerate(multi.loss_trace()):
        assert t.shape == (STEPS, 8) and _bits(t)[:, :6].tobytes() == rows[:, p, :6].tobytes(), p


def test_steps_beyond_the_capacity_write_nothing_and_change_nothing(vit):
    eng, rows = _one(vit, steps=6, n_epochs=4, loss_trace=True)
    assert eng.trace_dev.shape == (4, 1, 8)
    trace = eng.loss_trace()
    assert trace.shape == (4, 8) and _bits(trace)[:, :6].tobytes() == rows[:4, 0, :6].tobytes()
    off, off_rows = _one(vit, steps=6, n_epochs=4)
    assert off_rows.tobytes() == rows.tobytes()
    _same(_arenas(eng), _arenas(off))


def test_call_rules(vit):
    L = _lib.lib()
    buf = torch.full((4, 1, 8), float("nan"), device=DEV)
    new = lambda **over: SpliceEngine(_cfg(**over), None, synth.generator_params(61, 0.02), (64, 64), (64, 64), vit_engine=vit)
    eng = new()
    assert L.splice_step_set_loss_trace(eng.handle, None, 4) != 0 and L.splice_step_set_loss_trace(eng.handle, _lib.ptr(buf), 0) != 0
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0                 # a gradient-only handle
    assert L.splice_step_set_loss_trace(eng.handle, _lib.ptr(buf), 4) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    assert L.splice_step_set_phases(eng.handle, 3, None) == 0            # a phase-mode handle
    assert L.splice_step_set_loss_trace(eng.handle, _lib.ptr(buf), 4) != 0 and b"phase mode" in L.splice_last_error()
    assert L.splice_step_set_phases(eng.handle, 7, None) == 0
    A, B = _pair(62)
    eng.step(A, B, A)
    assert L.splice_step_set_loss_trace(eng.handle, _lib.ptr(buf), 4) != 0 and b"before the first step" in L.splice_last_error()
    torch.cuda.synchronize()
    assert np.all(_bits(buf) == FILL)
    on = new(loss_trace=True)                                            # ... and those modes are refused on a handle that has it
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"loss trace" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 3, None) != 0 and b"loss trace" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 2, eng.handle) != 0
    assert L.splice_step_set_mode(on.handle, 0, 0) == 0 and L.splice_step_set_phases(on.handle, 7, None) == 0


# 10: the drop-in entry points
TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, use_augmentations=False,
             global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0, cls_warmup=1, entire_A_every=5, loss_trace=True)
TRAIN_STOP = dict(stop_window=3, stop_patience=1, stop_rel=0.5)   # (tests/test_stop_gpu.py: the run stops at step 7)


def _write_pair(root, name):
    from PIL import Image
    A, B = synth.smooth_image_pair(60, 0, 72, 72)
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


def _read_csv(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    header = lines[0].split(",")
    return header, [dict(zip(header, ln.split(","))) for ln in lines[1:-1]]


def _check_csv(path, trace, cfg, clip=False):
    header, body = _read_csv(path)
    assert header == ["step", "lr"] + LOSS_KEYS + (["grad_norm", "clip_coef"] if clip else [])
    assert len(body) == len(trace)
    sch = LrSchedule(cfg)
    for s, ln in enumerate(body):
        assert int(ln["step"]) == s
        assert _bits(float(ln["loss"])) == _bits(trace[s, 0]), (s, ln["loss"], trace[s, 0])
        assert np.float32(float(ln["lr"])) == np.float32(sch.lr(s)), (s, ln["lr"], sch.lr(s))
        assert (ln["loss_global_ssim"] == "") == (s < cfg["cls_warmup"]) and (ln["loss_entire_cls"] == "") == (s % cfg["entire_A_every"] != 0)
        for i, k in enumerate(LOSS_KEYS):
            assert ln[k] == "" or _bits(float(ln[k])) == _bits(trace[s, i])
    return body


def test_train_model_writes_losses_csv(tmp_path):
    from splice_amd import batch
    from splice_amd.train import train_model, trace_fields
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    over = dict(TRAIN, n_epochs=9, scheduler_policy="cosine", grad_clip_norm=1e-3)
    eng = train_model(_write_pair(tmp_path, "full"), cfg_overrides=over, vit_state=vit_state, progress=False)
    trace = eng.loss_trace()
    assert trace.shape == (9, 8)
    body = _check_csv(tmp_path / "full" / "out" / "losses.csv", trace, eng.cfg, clip=True)
    assert len({ln["lr"] for ln in body}) == 9                           # the schedule's own value on every line
    assert all(_bits(float(ln["grad_norm"])) == _bits(trace[s, 6]) and _bits(float(ln["clip_coef"])) == _bits(trace[s, 7]) for s, ln in enumerate(body))
    assert trace_fields(eng) == {"loss_trace": "losses.csv"} and batch._slot_fields(eng)["loss_trace"] == "losses.csv"
    # fewer lines after a plateau stop
    stopped = train_model(_write_pair(tmp_path, "stop"), cfg_overrides=dict(TRAIN, n_epochs=60, **TRAIN_STOP), vit_state=vit_state, progress=False)
    k = stopped.stopped_at
    assert k is not None and k + 1 < 60
    assert len(_check_csv(tmp_path / "stop" / "out" / "losses.csv", stopped.loss_trace(), stopped.cfg)) == k + 1
    # and with the key off nothing new is written
    off = train_model(_write_pair(tmp_path, "off"), cfg_overrides=dict(TRAIN, n_epochs=4, loss_trace=False), vit_state=vit_state, progress=False)
    assert sorted(f.name for f in (tmp_path / "off" / "out").iterdir()) == ["output.png"] and trace_fields(off) == {}
    assert "loss_trace" not in batch._slot_fields(off)


def test_train_sweep_writes_one_losses_csv_per_variant(tmp_path):
    from splice_amd.train import train_sweep
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    variants = [dict(lr=0.002), dict(lr=0.004, scheduler_policy="linear", scheduler_n_epochs_decay=20, lambda_global_identity=0.0)]
    eng = train_sweep(_write_pair(tmp_path, "sweep"), variants, cfg_overrides=dict(TRAIN, n_epochs=8), vit_state=vit_state, progress=False)
    traces = eng.loss_trace()
    for k in range(2):
        d = tmp_path / "sweep" / "out" / "sweep" / str(k)
        body = _check_csv(d / "losses.csv", traces[k], eng.cfgs[k])
        assert len(body) == 8 and (body[3]["loss_global_id_B"] == "") == (k == 1)
        with open(d / "variant.json") as f:
            assert json.load(f)["loss_trace"] == "losses.csv"
    assert traces[0][:, 0].tobytes() != traces[1][:, 0].tobytes()
