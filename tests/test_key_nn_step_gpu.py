"""GPU, step level: the nearest-neighbour key appearance term (``lambda_global_key_nn`` / ``dino_nn_layer``) inside
the fused step, on the small synthetic ViT and crops of tests/test_key_gram_gpu.py: the reported value and assignment against np_key_nn on
the keys read back from the engine, word 0, the generator gradient against the oracle's autograd at the engine's assignment, shared and
own key-gradient buffers beside the structure and key second-moment lists, and bit identity where the step promises it."""
import ctypes as C
import shutil

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import KEY_NN_LOSS_KEY, MultiPairEngine, SpliceEngine, np_key_nn
from splice_amd.generator import GeneratorPlan
from splice_amd.vit import KIND_QKV_STORED
from test_key_gram_gpu import (GEN_SEED, TEACHER_FORCED_BAR, VALUE_BAR, _arenas, _bits, _cfg, _engine, _fmaf32, _oracle_keys, _pair, _same,  # noqa: F401
                               grad_errs, oracle_vit, vit, vit_state)
from test_key_nn_cpu import EPS, U24, cosine_reference, top_two_gap

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
LAM, LAYER = "lambda_global_key_nn", "dino_nn_layer"
G_LAM, G_LAYER, G_LAYERS = "lambda_global_key_gram", "dino_gram_layer", "dino_gram_layers"
S_LAYERS = "dino_ssim_layers"
NN_LAM = 1.5


def _engine_keys(eng, layer, p):
    """the [T][D] bf16 keys of block `layer` of pass p of the engine's global context, as the step's last forward left them"""
    D, T = eng.vit.dim, eng.ctx_g.T
    return eng.ctx_g.read(KIND_QKV_STORED, layer)[p, :T, D:2 * D].cpu()


def _check_against_engine_keys(eng, layer, pairs=1, pair=0, crops=1, tag=""):
    """key_nn_match / key_nn_value of slot `pair` against float64 on the engine's own bf16 keys: every row whose reference top-two gap is at
    least twice its derived cosine bound reports the reference's arg-max; the cosines lie within the bound at the reported index; the value
    within the bound tests/test_key_nn_gpu.py derives (per crop, the crops added)."""
    T = eng.ctx_g.T
    m, c = eng.key_nn_match(pair)
    assert m.shape == (crops, T) and c.shape == (crops, T) and m.dtype == np.int32 and c.dtype == np.float32
    Pa = pairs * crops
    want_v = bound_v = 0.0
    for i in range(crops):
        kb, kx = _engine_keys(eng, layer, Pa + pair * crops + i), _engine_keys(eng, layer, 2 * Pa + pair * crops + i)
        cr, E = cosine_reference(kx, kb)
        clear = top_two_gap(cr) >= 2 * E.max(axis=1)
        assert clear.any() and np.array_equal(m[i][clear], np.argmax(cr, axis=1)[clear]), (int(clear.sum()), np.nonzero(m[i] != np.argmax(cr, axis=1))[0])
        raw, _, cos, _ = np_key_nn(kx.double().numpy(), kb.double().numpy(), 1.0, eps=EPS, match=m[i])
        Et = E[np.arange(T), m[i]]
        assert (np.abs(c[i].astype(np.float64) - cos) <= Et).all()
        R = -(-(-(-T // 4)) // 64) + 11
        want_v += raw
        bound_v += np.mean(Et + U24 * np.abs(1 - cos)) * (1 + R * U24) * (1 + 1e-5) + R * U24 * np.mean(np.abs(1 - cos))
    got = eng.key_nn_value(pair)
    print(f"KEY_NN step {tag}: value {got:.7g}, np_key_nn on the engine's keys {want_v:.7g}, err/bound {abs(got - want_v) / bound_v:.4f}; distinct targets {len(set(m[0]))} of {T}, rows with a clear reference arg-max {int(clear.sum())}")
    assert abs(got - want_v) <= bound_v + U24 * abs(want_v) * crops
    return got, m


def _word0(row, cfg, entire, kg, nn):
    """the total-loss kernel's chain on the reported words, in float32: one product, four fused multiply-adds, then the key second-moment
    term's fused multiply-add where it is on, then this term's (the steps compared lie behind cls_warmup)"""
    w = {k: f32(cfg[k]) for k in ("lambda_global_ssim", "lambda_entire_ssim", "lambda_entire_cls", "lambda_global_cls", "lambda_global_identity")}
    w_essim, w_ecls = (w["lambda_entire_ssim"], w["lambda_entire_cls"]) if entire else (f32(0), f32(0))
    t = f32(w_essim * f32(row[2]))
    t = _fmaf32(w["lambda_global_ssim"], row[1], t)
    t = _fmaf32(w_ecls, row[3], t)
    t = _fmaf32(w["lambda_global_cls"], row[4], t)
    t = _fmaf32(w["lambda_global_identity"], row[5], t)
    if kg is not None:
        t = _fmaf32(f32(cfg[G_LAM]), f32(kg), t)
    return t, _fmaf32(f32(cfg[LAM]), f32(nn), t)


@pytest.mark.parametrize("layer,gram", [(None, False), (5, False), (5, True)], ids=["top", "5", "5-with-key-gram"])
def test_step_reports_the_value_the_match_and_word_0(vit, layer, gram):
    """lr 0, cls_warmup 0, entire_A_every 2: step 0 is an entire-image step, step 1 an ordinary one.  Value and assignment against np_key_nn on
    the keys read back from the engine; word 0 is the fused multiply-add of lambda * raw onto the total without the term (behind the key
    second-moment term's where both are on: the instance with both), exactly; the parameters do not move."""
    A, B = _pair()
    extra = {G_LAM: 2.0, G_LAYER: 7} if gram else {}
    eng = _engine(vit, lr=0.0, cls_warmup=0, entire_A_every=2, **{LAM: NN_LAM, LAYER: layer}, **extra)
    l = 11 if layer is None else layer
    assert eng.key_nn == (NN_LAM, l) and eng.cfg[LAYER] == l
    assert eng.key_nn_value() == 0.0 and not eng.key_nn_match()[0].any()   # (no step yet)
    p0 = eng.params.clone()
    for step in range(2):
        eng.step(A, B, A)
        entire = step % 2 == 0
        row = eng.losses_dev[0].cpu().numpy()
        got, _ = _check_against_engine_keys(eng, l, tag=f"{step} ({'entire-image' if entire else 'ordinary'}) layer {l}")
        losses = eng.losses()
        assert losses[KEY_NN_LOSS_KEY] == got and losses["loss"] == float(row[0]) and got > 0
        assert ("loss_entire_ssim" in losses) == entire
        without, want = _word0(row, eng.cfg, entire, eng.key_gram_value() if gram else None, got)
        assert row[0].tobytes() == want.tobytes() and want != without, (step, row, got)
    assert torch.equal(eng.params, p0)


def _oracle_nn_loss(m, x, b, layer, match):
    """lambda-free: (1 / T) sum_i (1 - cos(k_i, b_match(i))) on the oracle ViT's fp32 keys, the target under no_grad; and every row's best cosine"""
    with torch.no_grad():
        kb = _oracle_keys(m, b, layer)
    kx = _oracle_keys(m, x, layer)
    cos = (kx @ kb.T) / torch.clamp(kx.norm(dim=1)[:, None] * kb.norm(dim=1)[None, :], min=1e-8)
    idx = torch.from_numpy(np.asarray(match, dtype=np.int64))
    chosen = cos[torch.arange(cos.shape[0]), idx]
    return (1.0 - chosen).mean(), chosen.detach(), cos.detach().max(dim=1).values


@pytest.mark.parametrize("layer", [None, 5], ids=["top", "5"])
def test_step_gradient_against_the_oracle_at_the_engines_match(vit, oracle_vit, grad_errs, layer):
    """Only this term on.  The oracle differentiates (lambda / T) sum (1 - cos(k_i, b_m(i))) with m the engine's reported assignment (the
    gradient of max is the gradient at the chosen index; bf16 and fp32 keys may break a near-tie differently).  The bar is the one
    tests/test_key_gram_gpu.py holds the same engine-against-oracle comparison to: the larger of three times the structure term's own
    figure and the teacher-forced bar.  Every engine match lies within VALUE_BAR, that test's tolerance on key-derived values, of the
    oracle's row maximum."""
    A, B = _pair()
    l = 11 if layer is None else layer
    off = dict(lambda_global_cls=0.0, lambda_global_identity=0.0, lambda_entire_cls=0.0, lambda_entire_ssim=0.0, lambda_global_ssim=0.0, cls_warmup=0, lr=0.0)
    eng = _engine(vit, entire=False, **off, **{LAM: NN_LAM, LAYER: layer})
    p0 = eng.params.clone()
    eng.step(A, B)
    assert torch.equal(eng.params, p0)
    match = eng.key_nn_match()[0][0]
    plan = GeneratorPlan(eng.gen, 1, 64, 64, True, 0)
    x = plan.forward(eng.params, A[None])[0].cpu().clone().requires_grad_(True)
    raw, chosen, best = _oracle_nn_loss(oracle_vit, x, B.cpu(), l, match)
    loss = NN_LAM * raw
    dx, = torch.autograd.grad(loss, x)
    g_ref = plan.backward(eng.params, dx[None].to(DEV).contiguous())
    num = den = 0.0
    for (pname, g), r in zip(eng.gen.unflatten(eng.grads).items(), eng.gen.unflatten(g_ref).values()):
        if pname.endswith("0.bias") and pname != "9.0.bias":
            continue   # zero-gradient conv biases (feed a BatchNorm)
        num += (g.double() - r.double()).pow(2).sum().item()
        den += r.double().pow(2).sum().item()
    err = (num / den) ** 0.5
    loss_err = abs(eng.losses_dev[0, 0].item() - loss.item()) / loss.item()
    yard, yard_loss, _ = grad_errs("ssim")
    bar = max(3 * yard, TEACHER_FORCED_BAR)
    short = float((best - chosen).max())
    print(f"KEY_NN gradient layer {l}: rel L2 {err:.3e} (total rel {loss_err:.2e}); structure term, default layer {yard:.3e}; bar {bar:.3e}; "
          f"largest oracle shortfall of an engine match {short:.2e} (tolerance {VALUE_BAR:.0e}); matches that are the oracle's arg-max: "
          f"{int((best == chosen).sum())} of {len(match)}")
    assert den > 0 and err <= bar and loss_err < 1e-2
    assert short <= VALUE_BAR


@pytest.mark.parametrize("nn_layer", [5, 2, 7], ids=["shared-with-structure-5", "shared-with-key-gram-2", "own-7"])
def test_on_a_lower_block_beside_the_structure_and_key_gram_lists(vit, grad_errs, nn_layer):
    """dino_ssim_layers [5, 11], dino_gram_layers [2, 5] and this term on block 5 (the structure list's buffer: that term stores, the other
    two add), on block 2 (the key second-moment term's own buffer) or on block 7 (a buffer of its own).  lr 0, only these terms on.  The
    generator gradient equals the sum of the gradients of the engine without this term and of the engine with this term alone, within the
    gradient bar; value and assignment have the bits of the engine that carries this term alone; two pairs stay batch-independent."""
    A, B = _pair()
    others = {S_LAYERS: [5, 11], G_LAM: 2.0, G_LAYERS: [2, 5]}
    nk = {LAM: NN_LAM, LAYER: nn_layer}
    base = dict(lr=0.0, cls_warmup=0, lambda_global_cls=0.0, lambda_global_identity=0.0)
    both = _engine(vit, entire=False, **base, **others, **nk)
    rest = _engine(vit, entire=False, **base, **others)
    only = _engine(vit, entire=False, **base, **nk, lambda_global_ssim=0.0)
    for e in (both, rest, only):
        e.step(A, B)
    assert f32(both.key_nn_value()).tobytes() == f32(only.key_nn_value()).tobytes() and both.key_nn_value() > 0
    assert all(np.array_equal(a, b) for a, b in zip(both.key_nn_match(), only.key_nn_match()))
    assert f32(both.key_gram_value()).tobytes() == f32(rest.key_gram_value()).tobytes()
    assert both.ssim_layer_values().tobytes() == rest.ssim_layer_values().tobytes()
    want = rest.grads.double() + only.grads.double()
    rel = ((both.grads.double() - want).norm() / want.norm()).item()
    share = (only.grads.double().norm() / want.norm()).item()
    bar = max(3 * grad_errs("ssim")[0], TEACHER_FORCED_BAR)
    print(f"KEY_NN block {nn_layer} beside structure layers [5, 11] and key second-moment layers [2, 5]: combined gradient against the sum rel L2 {rel:.3e} "
          f"(this term's share of the norm {share:.2e}); bar {bar:.3e}")
    assert rel <= bar and share > 1e-3
    _check_against_engine_keys(both, nn_layer, tag=f"block {nn_layer} beside the lists")
    if nn_layer != 5:
        return
    pairs = [_pair(40, 2), _pair(62, 0)]
    gens = [synth.generator_params(41, 0.02), synth.generator_params(61, 0.02)]
    cfg = _cfg(cls_warmup=0, **others, **nk)
    multi = MultiPairEngine(cfg, None, gens, (64, 64), None, vit_engine=vit)
    A2, B2 = torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()
    for _ in range(2):
        multi.step(A2, B2)
    for p in range(2):
        single = SpliceEngine(cfg, None, gens[p], (64, 64), None, vit_engine=vit)
        for _ in range(2):
            single.step(pairs[p][0], pairs[p][1])
        assert _same(_arenas(multi, p), _arenas(single)), p
        assert f32(multi.key_nn_value(p)).tobytes() == f32(single.key_nn_value()).tobytes()


@pytest.mark.parametrize("keys", [{}, {LAM: 0.0}, {LAM: 0, LAYER: None}], ids=["absent", "zero", "int-zero-null"])
def test_the_term_off_is_the_engine_without_the_keys(vit, keys):
    """6 steps over the regimes -- [CLS] warm-up (steps 0-1), entire-image steps (0, 4), an unequal crop (step 3) --: losses, gradients and
    every arena are the bytes of an engine whose config never held the keys (no setter is called, no launch differs)"""
    A, B = _pair()
    A2 = A[:, :60, :60].contiguous()
    cfg = {k: v for k, v in _cfg(cls_warmup=2, entire_A_every=4).items() if k not in (LAM, LAYER)}
    twin = SpliceEngine(cfg, None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64), vit_engine=vit)
    eng = SpliceEngine(dict(cfg, **keys), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64), vit_engine=vit)
    assert eng.key_nn is None
    for i in range(6):
        for e in (eng, twin):
            e.step(A2 if i == 3 else A, B, A)
        assert torch.equal(_bits(eng.losses_dev), _bits(twin.losses_dev)) and torch.equal(_bits(eng.grads), _bits(twin.grads)), i
        assert KEY_NN_LOSS_KEY not in eng.losses()
    assert _same(_arenas(eng), _arenas(twin))
    with pytest.raises(RuntimeError, match="lambda_global_key_nn"):
        eng.key_nn_value()
    with pytest.raises(RuntimeError, match="lambda_global_key_nn"):
        eng.key_nn_match()


def test_batch_independence_two_pairs(vit):
    """default lr, 3 steps behind the warm-up, block 5: each pair of a two-pair engine is, bit for bit, its own SpliceEngine run, value and
    assignment included"""
    keys = {LAM: NN_LAM, LAYER: 5}
    pairs = [_pair(40, 2), _pair(62, 0)]
    gens = [synth.generator_params(41, 0.02), synth.generator_params(61, 0.02)]
    multi = MultiPairEngine(_cfg(cls_warmup=1, **keys), None, gens, (64, 64), (64, 64), vit_engine=vit)
    A2, B2 = torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()
    rows, vals, matches = [], [], []
    for _ in range(3):
        multi.step(A2, B2, A2)
        rows.append(multi.losses_dev.clone())
        vals.append(multi.key_nn_value())
        matches.append(multi.key_nn_match())
    assert matches[2][0].shape == (2, 1, multi.ctx_g.T)
    for p in range(2):
        single = SpliceEngine(_cfg(cls_warmup=1, **keys), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for k in range(3):
            single.step(pairs[p][0], pairs[p][1], pairs[p][0])
            assert torch.equal(_bits(single.losses_dev[0]), _bits(rows[k][p])), (p, k)
            assert f32(single.key_nn_value()).tobytes() == f32(vals[k][p]).tobytes(), (p, k)
            sm, sc = single.key_nn_match()
            assert np.array_equal(sm, matches[k][0][p]) and sc.tobytes() == matches[k][1][p].tobytes(), (p, k)
            assert (KEY_NN_LOSS_KEY in single.losses()) == (k >= 1)
        assert multi.key_nn_value(p) == vals[2][p]
        assert _same(_arenas(multi, p), _arenas(single)), p
        assert vals[2][p] > 0 and vals[0][p] == 0   # (step 0 lies before the warm-up step: the term has not run)
    _check_against_engine_keys(multi, 5, pairs=2, pair=1, tag="pair 1 of two")


def test_graph_replay_equals_eager(vit):
    """Four steps on fixed crops with lr 0: step 1 is launched eagerly, step 2 captures the graph, step 3 replays it; then an engine that
    never captures.  Gradient arena, first moment, losses row, value and assignment agree bit for bit.  Behind it other settings in the
    same process: their own graphs, their own numbers."""
    A, B = _pair()
    keys = {LAM: NN_LAM, LAYER: 5}
    eng = _engine(vit, lr=0.0, cls_warmup=0, **keys)
    seen = []
    for _ in range(4):
        eng.step(A, B, A)
        seen.append((eng.grads.clone(), eng.m.clone(), eng.losses_dev.clone()))
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    assert stats[0] + stats[2] >= 1                                     # a graph was in use
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(seen[3], seen[1]))   # (both ordinary steps; steps 0 and 2 are entire-image steps)
    val, (m, c) = eng.key_nn_value(), eng.key_nn_match()
    eager = _engine(vit, lr=0.0, cls_warmup=0, **keys)
    _lib.check(_lib.lib().splice_step_use_graph(eager.handle, 0), "use_graph")
    for _ in range(4):
        eager.step(A, B, A)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((eager.grads, eager.m, eager.losses_dev), seen[3]))
    em, ec = eager.key_nn_match()
    assert eager.key_nn_value() == val and val > 0 and np.array_equal(em, m) and ec.tobytes() == c.tobytes()
    for other_keys in ({LAM: NN_LAM, LAYER: 11}, {LAM: 0.5, LAYER: 5}):   # (the pool's salt carries the block and the weight)
        other = _engine(vit, lr=0.0, cls_warmup=0, **other_keys)
        other_eager = _engine(vit, lr=0.0, cls_warmup=0, **other_keys)
        _lib.check(_lib.lib().splice_step_use_graph(other_eager.handle, 0), "use_graph")
        for _ in range(4):
            other.step(A, B, A)
            other_eager.step(A, B, A)
        assert torch.equal(_bits(other.m), _bits(other_eager.m)) and torch.equal(_bits(other.losses_dev), _bits(other_eager.losses_dev))
        assert not torch.equal(_bits(other.losses_dev), _bits(seen[3][2]))


def test_value_over_two_crops_is_the_sum_over_the_zip(vit):
    """n_crops = 2 on one pair: value and assignment per crop against np_key_nn on the engine's keys, the crops added"""
    A, B = _pair()
    A2 = torch.stack([A, A.flip(-1)]).contiguous()
    B2 = torch.stack([B, B.flip(-2)]).contiguous()
    eng = SpliceEngine(_cfg(lr=0.0, cls_warmup=0, **{LAM: NN_LAM}), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit, n_crops=2)
    eng.step(A2, B2)
    _, m = _check_against_engine_keys(eng, 11, crops=2, tag="two crops")
    assert not np.array_equal(m[0], m[1])


# the settings of tests/test_ema_gpu.py::test_a_stopped_slot_keeps_the_average_of_its_stop_step: slots 0 and 2 (lr 0 and 1e-6) cannot improve
# by stop_rel and stop at the close of their third window, slot 1 learns
SLOTS = dict(cls_warmup=1, entire_A_every=7, stop_patience=2, stop_window=4)
SLOT_RELS = (0.01, 0.02, 0.05, 0.1, 0.2, 0.3, 0.5)
SLOT_LRS = [0.0, 2e-3, 1e-6]
SLOT_STEPS = 18


def test_a_pair_frozen_by_the_stop_rule_keeps_its_value(vit):
    """a slot the stop rule froze reports, at every later step, the value and assignment of its frozen weights -- bit for bit those of the
    first step behind its stop step -- while its neighbour goes on; up to its stop step it is its own SpliceEngine run"""
    keys = {LAM: NN_LAM, LAYER: 5}
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    for rel in SLOT_RELS:
        multi = MultiPairEngine(_cfg(stop_rel=rel, **SLOTS, **keys), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in SLOT_LRS])
        vals, matches = [], []
        for _ in range(SLOT_STEPS):
            multi.step(As, Bs, As)
            vals.append(multi.key_nn_value())
            matches.append(multi.key_nn_match()[0].copy())
        ks = multi.stopped_at
        if ks[1] is None and ks[0] is not None and ks[2] is not None:
            break
    assert ks[1] is None and 0 <= ks[0] < SLOT_STEPS - 4 and 0 <= ks[2] < SLOT_STEPS - 4, (rel, ks)
    for p in (0, 2):
        first = ks[p] + 1
        for k in range(first + 1, SLOT_STEPS):
            assert f32(vals[k][p]).tobytes() == f32(vals[first][p]).tobytes() and np.array_equal(matches[k][p], matches[first][p]), (p, k)
        single = SpliceEngine(dict(_cfg(lr=SLOT_LRS[p], **SLOTS, **keys), stop_window=0), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for k in range(ks[p] + 1):
            single.step(A, B, A)
            assert f32(single.key_nn_value()).tobytes() == f32(vals[k][p]).tobytes(), (p, k)
    assert len({f32(vals[k][1]).tobytes() for k in range(2, SLOT_STEPS)}) > SLOT_STEPS // 2   # (the running slot's value moves)


def test_snapshot_restore_continues_bit_for_bit_and_is_refused_under_another_value(vit):
    A, B = _pair()
    eng = _engine(vit, **{LAM: NN_LAM, LAYER: 5})
    eng.step(A, B, A)
    eng.step(A, B, A)
    state = eng.snapshot(0)
    with pytest.raises(ValueError, match="dino_nn_layer|lambda_global_key_nn"):   # (either key: the comparison names the first that differs)
        _engine(vit).restore([state])
    with pytest.raises(ValueError, match="'" + LAYER + "'"):
        _engine(vit, **{LAM: NN_LAM, LAYER: 7}).restore([state])
    with pytest.raises(ValueError, match="'" + LAM + "'"):
        _engine(vit, **{LAM: 1.0, LAYER: 5}).restore([state])
    same = _engine(vit, **{LAM: NN_LAM, LAYER: 5})
    same.restore([state])
    for _ in range(2):
        eng.step(A, B, A)
        same.step(A, B, A)
        assert torch.equal(_bits(same.params), _bits(eng.params)) and torch.equal(_bits(same.losses_dev), _bits(eng.losses_dev))
        assert same.key_nn_value() == eng.key_nn_value() and np.array_equal(same.key_nn_match()[0], eng.key_nn_match()[0])
    assert _same(_arenas(same), _arenas(eng))


def test_a_sweep_slot_equals_its_own_train_model_run(tmp_path):
    """train_sweep with the keys in the shared config against train_model per variant: losses (the term's among them), weights, the image, and
    the keys in variant.json / the run's fields"""
    import json
    from splice_amd.train import key_nn_fields, train_model, train_sweep
    from test_sweep_gpu import OVER, _write_pair
    vit_state_ = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    over = dict(OVER, n_epochs=6, log_images_freq=3, **{LAM: NN_LAM, LAYER: 5})
    variants = [dict(lr=0.002), dict(lr=0.004, lambda_global_ssim=0.5)]
    _write_pair(tmp_path / "sweep")
    eng = train_sweep(str(tmp_path / "sweep"), variants, cfg_overrides=over, vit_state=vit_state_, progress=False)
    assert key_nn_fields(eng) == {LAM: NN_LAM, LAYER: 5}
    for k, v in enumerate(variants):
        shutil.copytree(tmp_path / "sweep" / "A", tmp_path / f"single{k}" / "A")
        shutil.copytree(tmp_path / "sweep" / "B", tmp_path / f"single{k}" / "B")
        single = train_model(str(tmp_path / f"single{k}"), cfg_overrides=dict(over, **v), vit_state=vit_state_, progress=False)
        assert single.losses() == eng.losses(k) and KEY_NN_LOSS_KEY in eng.losses(k), (k, single.losses(), eng.losses(k))
        assert f32(single.key_nn_value()).tobytes() == f32(eng.key_nn_value(k)).tobytes()
        assert torch.equal(single.params, eng.pair_params(k))
        assert (tmp_path / f"single{k}" / "out" / "output.png").read_bytes() == (tmp_path / "sweep" / "out" / "sweep" / str(k) / "output.png").read_bytes()
        with open(tmp_path / "sweep" / "out" / "sweep" / str(k) / "variant.json") as f:
            rec = json.load(f)
        assert rec[LAM] == NN_LAM and rec[LAYER] == 5 and rec["losses"] == eng.losses(k)
    assert eng.losses(0)["loss"] != eng.losses(1)["loss"]


def test_setter_refusals(vit, vit_state):
    L = _lib.lib()
    A, B = _pair()
    eng = _engine(vit)
    for lam, layer, word in ((0.0, 5, b"finite and > 0"), (-1.0, 5, b"finite and > 0"), (float("nan"), 5, b"finite and > 0"), (float("inf"), 5, b"finite and > 0"),
                             (1.0, -1, b"block index"), (1.0, 12, b"block index")):
        assert L.splice_step_set_key_nn(eng.handle, lam, layer) != 0 and word in L.splice_last_error()
    out = (C.c_float * 8)()
    assert L.splice_step_key_nn_values(eng.handle, out) != 0 and b"no nearest-neighbour key term" in L.splice_last_error()
    assert L.splice_step_key_nn_match(eng.handle, out, out) != 0 and b"no nearest-neighbour key term" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert L.splice_step_set_key_nn(eng.handle, 1.0, 5) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    lead = _engine(vit)
    assert L.splice_step_set_phases(eng.handle, 2, lead.handle) == 0
    assert L.splice_step_set_key_nn(eng.handle, 1.0, 5) != 0 and b"phase mode" in L.splice_last_error()
    assert L.splice_step_set_phases(eng.handle, 7, None) == 0
    eng.step(A, B, A)
    assert L.splice_step_set_key_nn(eng.handle, 1.0, 5) != 0 and b"before the first step" in L.splice_last_error()
    on = _engine(vit, **{LAM: 1.0, LAYER: 5})
    assert L.splice_step_set_key_nn(on.handle, 1.0, 5) != 0 and b"once" in L.splice_last_error()
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"nearest-neighbour" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 2, lead.handle) != 0 and b"nearest-neighbour" in L.splice_last_error()
    # the setters whose key-gradient buffers this term shares come first
    two, w2 = (C.c_int * 2)(3, 11), (C.c_float * 2)(1.0, 1.0)
    assert L.splice_step_set_ssim_layers(on.handle, 2, two, w2) != 0 and b"in front of splice_step_set_key_nn" in L.splice_last_error()
    assert L.splice_step_set_id_layers(on.handle, 2, two, w2) != 0 and b"in front of splice_step_set_key_nn" in L.splice_last_error()
    assert L.splice_step_set_key_gram(on.handle, 1.0, 5) != 0 and b"in front of splice_step_set_key_nn" in L.splice_last_error()
    assert L.splice_step_set_key_gram_layers(on.handle, 1.0, 2, two, w2, 0) != 0 and b"in front of splice_step_set_key_nn" in L.splice_last_error()
    assert L.splice_step_key_nn_values(on.handle, out) == 0 and out[0] == 0.0   # (no step yet)
    # several pairs with different crop counts per side: the host refuses it by name
    with pytest.raises(ValueError, match="'lambda_global_key_nn'.*crop counts"):
        MultiPairEngine(_cfg(**{LAM: 1.0}), None, [synth.generator_params(41, 0.02)] * 2, (64, 64), None, vit_engine=vit, n_crops=(2, 1))
    # fp8: the C setter refuses what the Python engine refuses on the host (an engine of its own: the e4m3 weights stay with it)
    from splice_amd.vit import VitEngine
    vit8 = VitEngine("dino_vits8", device=DEV).load_state_dict(vit_state)
    e8 = SpliceEngine(_cfg(), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit8, fp8=True)
    assert L.splice_step_set_key_nn(e8.handle, 1.0, 5) != 0 and b"fp8" in L.splice_last_error()
    with pytest.raises(ValueError, match="fp8"):
        SpliceEngine(_cfg(**{LAM: 1.0}), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit8, fp8=True)
