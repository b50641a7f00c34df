"""GPU: hyper-parameter sweeps inside the fused multi-pair step.  Slot p of a MultiPairEngine with per-slot configs
(loss weights, lr and its schedule) is, bit for bit, the SpliceEngine run of its merged config: losses of every step, parameters,
optimiser moments, BatchNorm statistics.  Op level: the per-pair-lr optimiser kernels against one call per pair.  End to end:
train_sweep against train_model per variant, and run_batch(sweep=...) against train_sweep."""
import ctypes as C
import json
import shutil

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import MultiPairEngine, SpliceEngine
from splice_amd.generator import OPTIMIZER_KINDS
from splice_amd.util import fused_optimizer

pytestmark = pytest.mark.gpu
DEV = "cuda"


# ---------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("name", ["adam", "rmsprop", "sgd"])
def test_optim_step_pairs_equals_one_call_per_pair(name):
    kind, (_, hp0, hp1, eps) = OPTIMIZER_KINDS[name], fused_optimizer(dict(optimizer=name, optimizer_beta1=0.0, optimizer_beta2=0.99))
    P, n = 5, 40001                     # odd n: every pair has a scalar tail in its own call
    stride = (n + 63) // 64 * 64
    lrs = [2e-3, 1e-3, 5e-4, 3e-2, 7.5e-4]
    gen = torch.Generator().manual_seed(5)
    p0 = torch.zeros(P * stride)
    for p in range(P):
        p0[p * stride: p * stride + n] = torch.randn(n, generator=gen)
    arenas = [p0.to(DEV)] + [torch.zeros(P * stride, device=DEV) for _ in range(2)]   # params, m, v
    singles = [[t[p * stride: p * stride + n].clone() for t in arenas] for p in range(P)]
    lr_dev = torch.tensor(lrs, dtype=torch.float32, device=DEV)
    L = _lib.lib()
    for step in (1, 2, 3):
        g = torch.zeros(P * stride)
        g2 = torch.zeros(P * stride)
        for p in range(P):
            g[p * stride: p * stride + n] = torch.randn(n, generator=gen) * 0.1
            g2[p * stride: p * stride + n] = torch.randn(n, generator=gen) * 0.1
        g, g2 = g.to(DEV), g2.to(DEV)
        _lib.check(L.splice_optim_step_pairs(kind, _lib.ptr(arenas[0]), _lib.ptr(g.clone()), _lib.ptr(g2), _lib.ptr(arenas[1]), _lib.ptr(arenas[2]),
                                             P, stride, n, _lib.ptr(lr_dev), hp0, hp1, eps, step, 1, _lib.current_stream()), "optim_step_pairs")
        for p, (pp, m, v) in enumerate(singles):
            gp, g2p = g[p * stride: p * stride + n].clone(), g2[p * stride: p * stride + n].clone()
            _lib.check(L.splice_optim_step_ex(kind, _lib.ptr(pp), _lib.ptr(gp), _lib.ptr(g2p), _lib.ptr(m), _lib.ptr(v), n, lrs[p], None,
                                              hp0, hp1, eps, step, 1, _lib.current_stream()), "optim_step_ex")
        torch.cuda.synchronize()
        for p, single in enumerate(singles):
            for a, b in zip(arenas, single):
                assert torch.equal(a[p * stride: p * stride + n], b), (name, step, p)
    assert not torch.equal(arenas[0], p0.to(DEV))
    # the stride must keep float4 groups inside a pair
    with pytest.raises(RuntimeError):
        _lib.check(L.splice_optim_step_pairs(kind, _lib.ptr(arenas[0]), _lib.ptr(g), None, _lib.ptr(arenas[1]), _lib.ptr(arenas[2]),
                                             P, stride - 2, n - 100, _lib.ptr(lr_dev), hp0, hp1, eps, 4, 0, _lib.current_stream()), "optim_step_pairs")


# -------------------------------------------------------------------------------------------------------------- step level
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


BASE = dict(dino_model_name="dino_vits8", dino_global_patch_size=64, cls_warmup=2, entire_A_every=4, n_epochs=7)
# every per-slot key differs somewhere; slot 1 has no identity term, slot 2 no entire structure term
VARIANTS = [dict(lambda_global_cls=10.0, lambda_global_ssim=1.0, lambda_global_identity=1.0, lambda_entire_cls=10, lambda_entire_ssim=1.0,
                 lr=0.002, scheduler_policy="none"),
            dict(lambda_global_cls=5.0, lambda_global_ssim=2.0, lambda_global_identity=0.0, lambda_entire_cls=3, lambda_entire_ssim=0.5,
                 lr=0.004, scheduler_policy="linear", scheduler_n_epochs_decay=5),
            dict(lambda_global_cls=2.5, lambda_global_ssim=0.25, lambda_global_identity=3.0, lambda_entire_cls=1, lambda_entire_ssim=0.0,
                 lr=0.001, scheduler_policy="step", scheduler_lr_decay_iters=2),
            dict(lambda_global_cls=20.0, lambda_global_ssim=0.5, lambda_global_identity=0.5, lambda_entire_cls=7.5, lambda_entire_ssim=2.0,
                 lr=0.003, scheduler_policy="cosine")]


def _inputs(P, seed=77):
    A, B = synth.smooth_image_pair(seed, 0, 64, 64)
    A, B = torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    return A, B, A[None].expand(P, -1, -1, -1).contiguous(), B[None].expand(P, -1, -1, -1).contiguous()


def _run_and_compare(cfg, variants, crop_at, steps, vit, fp8=False):
    """The sweep engine over `steps` steps (crop_at(i): A crop size of step i) against one SpliceEngine per slot."""
    P = len(variants)
    gens = [synth.generator_params(90 + p, 0.02) for p in range(P)]
    A, B, As, Bs = _inputs(P)
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit, fp8=fp8, pair_cfgs=variants)
    assert multi._pair_lambdas and multi._pair_lr
    hist, lrs = [], []
    for i in range(steps):
        s = crop_at(i)
        multi.step(As[:, :, :s, :s].contiguous(), Bs, As)
        hist.append(multi.losses_dev.clone())
        lrs.append(list(multi.lr))
    torch.cuda.synchronize()
    n = multi.gen.numel
    for p in range(P):
        single = SpliceEngine(dict(cfg, **variants[p]), None, gens[p], (64, 64), (64, 64), vit_engine=vit, fp8=fp8)
        assert multi.cfgs[p] == single.cfg
        for i in range(steps):
            s = crop_at(i)
            single.step(A[:, :s, :s].contiguous(), B, A)
            assert single.lr == lrs[i][p], (p, i)
            assert torch.equal(single.losses_dev[0], hist[i][p]), (p, i, single.losses_dev[0], hist[i][p])
        torch.cuda.synchronize()
        assert single.losses() == multi.losses(p)
        sl = slice(p * multi.stride, p * multi.stride + n)
        assert torch.equal(single.params, multi.params[sl]), (p, (single.params - multi.params[sl]).abs().max().item())
        assert torch.equal(single.m, multi.m[sl]) and torch.equal(single.v, multi.v[sl])
        assert torch.equal(single.running[0], multi.running[p])
        assert single.generator_calls[0] == multi.generator_calls[p]
    return multi, hist, lrs


@pytest.mark.parametrize("optimizer", ["adam", "rmsprop", "sgd"])
def test_sweep_slots_bit_identical_to_single_runs(optimizer, vit):
    """4 slots, 7 steps through every regime (CLS warm-up, entire steps 0 and 4, an unequal crop at step 5)."""
    cfg = dict(BASE, optimizer=optimizer)
    multi, hist, lrs = _run_and_compare(cfg, VARIANTS, lambda i: 60 if i == 5 else 64, 7, vit)
    assert hist[4][1][5].item() == 0.0 and hist[4][2][2].item() == 0.0       # the zero-weight terms report 0 ...
    assert hist[4][0][5].item() > 0.0 and hist[4][0][2].item() > 0.0         # ... where the others' do not
    assert "loss_global_id_B" not in multi.losses(1) and "loss_global_id_B" in multi.losses(0)
    assert len({tuple(x) for x in lrs}) > 2 and len(set(lrs[-1])) == 4


def test_sweep_under_graph_replay(vit):
    """Fixed crops for 8 steps: the step graph is captured and replayed while the scheduled lrs change every step."""
    cfg = dict(BASE, entire_A_every=100, cls_warmup=1, n_epochs=8)
    variants = [dict(v, scheduler_lr_decay_iters=1) for v in VARIANTS]
    multi, _, lrs = _run_and_compare(cfg, variants, lambda i: 64, 8, vit)
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(multi.handle, stats))
    assert stats[0] + stats[2] >= 1
    assert len({x[3] for x in lrs[2:]}) == 6 and len({x[2] for x in lrs[2:]}) == 6


def test_sweep_fp8_slots_equal_single_fp8_runs(vit):
    _run_and_compare(dict(BASE), VARIANTS, lambda i: 60 if i == 5 else 64, 6, vit, fp8=True)


def test_all_equal_pair_cfgs_are_the_plain_engine(vit):
    v = dict(lambda_global_ssim=0.5, lr=0.003, scheduler_policy="step", scheduler_lr_decay_iters=2)
    gens = [synth.generator_params(95 + p, 0.02) for p in range(3)]
    _, _, As, Bs = _inputs(3)
    a = MultiPairEngine(BASE, None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[v] * 3)
    b = MultiPairEngine(dict(BASE, **v), None, gens, (64, 64), (64, 64), vit_engine=vit)
    assert not a._pair_lambdas and not a._pair_lr
    for _ in range(5):
        a.step(As, Bs, As)
        b.step(As, Bs, As)
        torch.cuda.synchronize()
        assert torch.equal(a.losses_dev, b.losses_dev)
        assert a.lr == [b.lr] * 3
    assert torch.equal(a.params, b.params) and torch.equal(a.v, b.v) and torch.equal(a.running, b.running)


# ------------------------------------------------------------------------------------------------------------ end to end
OVER = dict(seed=3, n_epochs=12, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=6, entire_A_every=5)
E2E_VARIANTS = [dict(lambda_global_ssim=1.0),
                dict(lambda_global_cls=5.0, lambda_global_identity=0.0, lr=0.004, scheduler_policy="cosine"),
                dict(lambda_entire_ssim=0.0, lr=0.001, scheduler_policy="step", scheduler_lr_decay_iters=3, init_gain=0.05)]


def _write_pair(root, seed=60, h=64, w=80):
    from PIL import Image
    A, B = synth.smooth_image_pair(seed, 0, h, w)
    for name, img in (("A", A), ("B", B)):
        d = root / name
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")


def test_train_sweep_equals_train_model_per_variant(tmp_path):
    from splice_amd.train import train_model, train_sweep
    from splice_amd.networks import define_G
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    _write_pair(tmp_path / "sweep")
    variants = E2E_VARIANTS + [dict(seed=11, lr=0.003)]
    seen = []
    eng = train_sweep(str(tmp_path / "sweep"), variants, cfg_overrides=OVER, vit_state=vit_state, progress=False,
                      callback=lambda k, img: seen.append(k))
    assert seen == [0, 1, 2, 3] * 2
    for k, v in enumerate(E2E_VARIANTS):
        shutil.copytree(tmp_path / "sweep" / "A", tmp_path / f"single{k}" / "A")
        shutil.copytree(tmp_path / "sweep" / "B", tmp_path / f"single{k}" / "B")
        single = train_model(str(tmp_path / f"single{k}"), cfg_overrides=dict(OVER, **v), vit_state=vit_state, progress=False)
        assert single.losses() == eng.losses(k), (k, single.losses(), eng.losses(k))
        assert (tmp_path / f"single{k}" / "out" / "output.png").read_bytes() == (tmp_path / "sweep" / "out" / "sweep" / str(k) / "output.png").read_bytes()
        assert torch.equal(single.params, eng.pair_params(k))
        with open(tmp_path / "sweep" / "out" / "sweep" / str(k) / "variant.json") as f:
            rec = json.load(f)
        assert rec["overrides"] == v and rec["losses"] == eng.losses(k) and rec["seed"] == 3
    assert eng.losses(0)["loss"] != eng.losses(1)["loss"]
    # a variant with its own seed starts from define_G under that seed
    _write_pair(tmp_path / "init")
    eng0 = train_sweep(str(tmp_path / "init"), [{}, dict(seed=11, init_gain=0.05)], cfg_overrides=dict(OVER, n_epochs=0), vit_state=vit_state,
                       progress=False)
    torch.manual_seed(11)
    netG = define_G("xavier", 0.05, device=DEV)
    want = eng0.gen.flatten({n: t.detach() for n, t in netG.state_dict().items() if n in netG.engine.table})
    assert torch.equal(eng0.pair_params(1), want)
    assert not torch.equal(eng0.pair_params(0), want)


def test_train_sweep_end_of_run_equals_train_model(tmp_path, capsys):
    """The end of a sweep under every optional rule at once -- the stop rule (counted steps 1 2 3 | 4 6 7: a window mean must halve to
    count as better, so a slot stops at step 7 of 12), its best window's weights and the weight average: each slot's three weight sets and
    its three images are, bit for bit, those of the ``train_model`` run of its merged config."""
    from splice_amd.train import train_model, train_sweep
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    over = dict(OVER, stop_window=3, stop_patience=1, stop_rel=0.5, stop_keep_best=True, ema_decay=0.9)
    variants = [dict(lr=0.002), dict(lr=0.004)]
    _write_pair(tmp_path / "sweep")
    eng = train_sweep(str(tmp_path / "sweep"), variants, cfg_overrides=over, vit_state=vit_state, progress=False)
    with capsys.disabled():
        print(f"\nsweep: stopped_at {eng.stopped_at}, step_idx {eng.step_idx}")
    assert any(at is not None and at + 1 < over["n_epochs"] for at in eng.stopped_at), eng.stopped_at
    for k, v in enumerate(variants):
        shutil.copytree(tmp_path / "sweep" / "A", tmp_path / f"single{k}" / "A")
        shutil.copytree(tmp_path / "sweep" / "B", tmp_path / f"single{k}" / "B")
        single = train_model(str(tmp_path / f"single{k}"), cfg_overrides=dict(over, **v), vit_state=vit_state, progress=False)
        assert single.stopped_at == eng.stopped_at[k]
        for which in ({}, dict(ema=True), dict(best=True)):
            want, got = single.state_dict(**which), eng.state_dict(k, **which)
            assert want.keys() == got.keys()
            for name in want:
                assert torch.equal(want[name], got[name]), (k, which, name)
        for name in ("output.png", "output_ema.png", "output_best.png"):
            assert (tmp_path / f"single{k}" / "out" / name).read_bytes() == (tmp_path / "sweep" / "out" / "sweep" / str(k) / name).read_bytes(), (k, name)


def test_run_batch_sweep_equals_train_sweep(tmp_path, monkeypatch):
    from splice_amd import batch
    from splice_amd.train import train_sweep
    monkeypatch.setenv("SPLICE_SYNTHETIC_WEIGHTS", "1")
    for i in range(2):
        for r in ("queue", "serial"):
            _write_pair(tmp_path / r / f"p{i}", seed=61 + i)
    specs = ["lr=0.002,0.004", "lambda_global_identity=1,0"]
    res = batch.run_batch(str(tmp_path / "queue"), 1, OVER, sweep=specs)
    variants = batch.sweep_variants(specs)
    assert [r["pair"] for r in res] == ["p0", "p1"]
    for i, r in enumerate(res):
        eng = train_sweep(str(tmp_path / "serial" / f"p{i}"), variants, cfg_overrides=OVER, progress=False)
        assert r["steps"] == OVER["n_epochs"] and [x["overrides"] for x in r["variants"]] == variants
        assert [x["losses"] for x in r["variants"]] == eng.losses()
        for k in range(len(variants)):
            got = tmp_path / "queue" / f"p{i}" / "out" / "sweep" / str(k) / "output.png"
            assert got.read_bytes() == (tmp_path / "serial" / f"p{i}" / "out" / "sweep" / str(k) / "output.png").read_bytes()
