"""GPU: RMSprop, SGD and learning-rate schedules inside the fused step.  Op level: the fused optimiser kernels against
torch.optim, the device learning rate against the argument.  Step level (the 64x64 dino_vits8 setup of test_multipair_gpu.py):
a fused update equals the gradient of a skip-mode step followed by torch.optim, a schedule survives graph replay, pairs stay
bit-identical to their single runs, the several-scales engine and train_model run the configured optimiser and schedule."""
import ctypes as C

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import MultiPairEngine, MultiScaleEngine, SpliceEngine
from splice_amd.generator import OPTIMIZER_KINDS, optim_step
from splice_amd.util import LrSchedule, fused_optimizer

pytestmark = pytest.mark.gpu
DEV = "cuda"
TORCH_OPT = {"rmsprop": torch.optim.RMSprop, "sgd": torch.optim.SGD}


# ---------------------------------------------------------------------------------------------------------------- op level
@pytest.mark.parametrize("name", ["rmsprop", "sgd"])
@pytest.mark.parametrize("n,off", [(100003, 0), (4099, 1)])   # vector body + scalar tail; a view 4 bytes off 16-byte alignment: all tail
@pytest.mark.parametrize("use_g2", [False, True])
def test_optim_step_matches_torch(name, n, off, use_g2):
    kind, (_, hp0, hp1, eps) = OPTIMIZER_KINDS[name], fused_optimizer(dict(optimizer=name))
    gen = torch.Generator(device=DEV).manual_seed(5 + n + off)

    def arena(fill=None):
        buf = torch.randn(n + off, device=DEV, generator=gen) if fill is None else torch.full((n + off,), fill, device=DEV)
        return buf[off:]

    p0 = arena()
    p, m, v = arena(0.0), arena(7.0), arena(0.0)
    p.copy_(p0)
    ref = torch.nn.Parameter(p0.clone())
    opt = TORCH_OPT[name]([ref], lr=2e-3)
    for step, lr in enumerate((2e-3, 1.5e-3, 7e-4, 3e-3), start=1):
        g = arena() * (10.0 ** -step)
        g2 = arena() * 1e-2 if use_g2 else None
        opt.param_groups[0]["lr"] = lr
        ref.grad = g + g2 if use_g2 else g.clone()
        opt.step()
        gg = arena(0.0)
        gg.copy_(g)
        zero = step % 2 == 0
        optim_step(kind, p, gg, m, v, lr, hp0, hp1, eps, step, zero_grad=zero, g2=g2)
        if zero:
            assert gg.abs().max().item() == 0.0
        else:
            assert torch.equal(gg, ref.grad)   # g2 folded in and written back (untouched without g2)
        assert (p - ref.data).abs().max().item() < 1e-6, (name, step, (p - ref.data).abs().max().item())
        assert torch.equal(m, torch.full_like(m, 7.0))   # no optimiser here reads or writes m
        if name == "sgd":
            assert v.abs().max().item() == 0.0
        else:
            sq = opt.state[ref]["square_avg"]
            assert ((v - sq).abs() / sq.clamp_min(1e-30)).max().item() < 1e-5


def test_optim_step_plain_export_leaves_unused_arenas():
    """``splice_optim_step`` (the op-level form without g2 / device lr): RMSprop never touches m, SGD neither m nor v."""
    n = 1029
    for kind in (1, 2):
        p, g = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
        m, v = torch.full((n,), 3.0, device=DEV), torch.full((n,), 0.5, device=DEV)
        p_ref = p.clone()
        _lib.check(_lib.lib().splice_optim_step(kind, _lib.ptr(p), _lib.ptr(g), _lib.ptr(m), _lib.ptr(v), n, 1e-3, 0.99, 0.0, 1e-8, 1, 0,
                                                _lib.current_stream()))
        torch.cuda.synchronize()
        assert torch.equal(m, torch.full_like(m, 3.0))
        assert torch.equal(v, torch.full_like(v, 0.5)) == (kind == 2)
        assert not torch.equal(p, p_ref)


@pytest.mark.parametrize("name", ["adam", "rmsprop", "sgd"])
def test_device_lr_bit_identical_to_argument(name):
    """lr read from device memory == the same lr as the kernel argument, bit for bit (the argument is then ignored)."""
    kind, (_, hp0, hp1, eps) = OPTIMIZER_KINDS[name], fused_optimizer(dict(optimizer=name, optimizer_beta1=0.0, optimizer_beta2=0.99))
    n = 50001
    p0 = torch.randn(n, device=DEV)
    a = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    b = [p0.clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)]
    lr_dev = torch.zeros(1, device=DEV)
    for step, lr in enumerate((2e-3, 1e-3, 5e-4), start=1):
        g = torch.randn(n, device=DEV) * 0.1
        lr_dev.fill_(lr)
        optim_step(kind, a[0], g.clone(), a[1], a[2], lr, hp0, hp1, eps, step)
        optim_step(kind, b[0], g.clone(), b[1], b[2], 123.0, hp0, hp1, eps, step, lr_dev=lr_dev)
        for x, y in zip(a, b):
            assert torch.equal(x, y), (name, step)
    assert not torch.equal(a[0], p0)


# -------------------------------------------------------------------------------------------------------------- step level
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):
    return dict(dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed=73, P=None):
    if P is None:
        A, B = synth.smooth_image_pair(seed, 0, 64, 64)
        return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    imgs = [synth.smooth_image_pair(seed, p, 64, 64) for p in range(P)]
    return (torch.from_numpy(np.stack([a for a, _ in imgs])).to(DEV), torch.from_numpy(np.stack([b for _, b in imgs])).to(DEV))


def _skip_mode(eng):
    _lib.check(_lib.lib().splice_step_set_mode(eng.handle, 1, 0), "step_set_mode")
    return eng


@pytest.mark.parametrize("name", ["rmsprop", "sgd"])
def test_fused_step_equals_gradient_then_torch(name, vit):
    """Teacher-forced: from the same parameters, one fused step == a skip-mode step (gradient only) followed by torch.optim on
    that gradient.  Steps 0 and 2 take the entire-image branch (the B-crop gradient is added separately), step 1 folds it into
    the optimiser kernel."""
    cfg = _cfg(optimizer=name, entire_A_every=2)
    gen = synth.generator_params(81, 0.02)
    A, B = _pair()
    fused = SpliceEngine(cfg, None, gen, (64, 64), (64, 64), vit_engine=vit)
    skip = _skip_mode(SpliceEngine(cfg, None, gen, (64, 64), (64, 64), vit_engine=vit))
    ref = torch.nn.Parameter(fused.params.clone())
    opt = TORCH_OPT[name]([ref], lr=fused.cfg["lr"])
    for k in range(3):
        skip.params.copy_(fused.params)
        ref.data.copy_(fused.params)
        skip.step(A, B, A)
        fused.step(A, B, A)
        torch.cuda.synchronize()
        assert torch.equal(skip.losses_dev, fused.losses_dev), k
        ref.grad = skip.grads.clone()
        opt.step()
        err = (fused.params - ref.data).abs().max().item()
        assert err < 1e-6, (name, k, err)
        assert not torch.equal(fused.params, skip.params)
    if name == "rmsprop":
        sq = opt.state[ref]["square_avg"]
        assert ((fused.v - sq).abs() / sq.clamp_min(1e-30)).max().item() < 1e-5
        assert fused.m.abs().max().item() == 0.0
    else:
        assert fused.m.abs().max().item() == 0.0 and fused.v.abs().max().item() == 0.0


@pytest.mark.parametrize("name,policy,over", [("rmsprop", "step", dict(scheduler_lr_decay_iters=1)),
                                              ("sgd", "linear", dict(scheduler_n_epochs_decay=8)),
                                              ("adam", "cosine", dict(n_epochs=6))])
def test_schedule_under_graph_replay(name, policy, over, vit):
    """A schedule with a new lr every step, 7 steps at fixed crops: the graph is captured at the third step and replayed after
    it.  Graph on == graph off == a chain of skip-mode steps + splice_optim_step with the host's lr, bit for bit (a lr baked
    into the captured graph would break the first equality from the fourth step on)."""
    cfg = _cfg(optimizer=name, scheduler_policy=policy, entire_A_every=100, **over)
    gen = synth.generator_params(82, 0.02)
    A, B = _pair(74)
    graph = SpliceEngine(cfg, None, gen, (64, 64), (64, 64), vit_engine=vit)
    eager = SpliceEngine(cfg, None, gen, (64, 64), (64, 64), vit_engine=vit)
    _lib.check(_lib.lib().splice_step_use_graph(eager.handle, 0))
    chain = _skip_mode(SpliceEngine(cfg, None, gen, (64, 64), (64, 64), vit_engine=vit))
    kind, *hp = fused_optimizer(graph.cfg)
    sched = LrSchedule(graph.cfg)
    lrs = []
    for k in range(7):
        for e in (graph, eager, chain):
            e.step(A, B, A)
        optim_step(kind, chain.params, chain.grads, chain.m, chain.v, sched.lr(k), *hp, k + 1)
        torch.cuda.synchronize()
        assert graph.lr == eager.lr == sched.lr(k)
        lrs.append(graph.lr)
        for other in (eager, chain):
            assert torch.equal(graph.losses_dev, other.losses_dev), (k, graph.losses_dev, other.losses_dev)
            assert torch.equal(graph.params, other.params), (k, (graph.params - other.params).abs().max().item())
    assert len(set(lrs[2:])) == 5, lrs   # the lr changes on every replayed step
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(graph.handle, stats))
    assert stats[0] + stats[2] >= 1   # a graph was captured (and replayed on steps 3..6)
    _lib.check(_lib.lib().splice_step_graph_stats(eager.handle, stats))
    assert stats[0] + stats[2] == 0


def test_multipair_rmsprop_cosine_bit_identical_to_single_runs(vit):
    cfg = _cfg(optimizer="rmsprop", scheduler_policy="cosine", n_epochs=5, entire_A_every=3)
    gens = [synth.generator_params(83 + p, 0.02) for p in range(2)]
    A, B = _pair(75, P=2)
    multi = MultiPairEngine(cfg, None, gens, (64, 64), (64, 64), vit_engine=vit)
    hist = []
    for _ in range(5):
        multi.step(A, B, A)
        hist.append(multi.losses_dev.clone())
    torch.cuda.synchronize()
    n = multi.gen.numel
    for p in range(2):
        single = SpliceEngine(cfg, None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for i in range(5):
            single.step(A[p], B[p], A[p])
            assert torch.equal(single.losses_dev[0], hist[i][p]), (p, i)
        torch.cuda.synchronize()
        assert torch.equal(single.params, multi.pair_params(p)), (p, (single.params - multi.pair_params(p)).abs().max().item())
        assert torch.equal(single.v, multi.v[p * multi.stride: p * multi.stride + n])
    assert not torch.equal(multi.pair_params(0), multi.pair_params(1))


def test_multiscale_sgd_step_schedule(vit):
    """2 scales, SGD + step schedule: every update is p -= lr * (summed gradient) with the scheduled lr."""
    cfg = _cfg(optimizer="sgd", scheduler_policy="step", scheduler_lr_decay_iters=1, entire_A_every=2, lr=0.05)
    eng = MultiScaleEngine(cfg, None, synth.generator_params(84, 0.02), (64, 64), (64, 64), scales=(64, 96), vit_engine=vit)
    sched = LrSchedule(eng.cfg)
    A, B = _pair(76)
    for k in range(3):
        before = eng.params.clone()
        eng.step(A, B, A)
        torch.cuda.synchronize()
        assert eng.lr == sched.lr(k) == 0.05 * 0.5 ** k
        assert torch.equal(eng.params, before - eng.grads * float(np.float32(eng.lr)))   # (contraction off: lr * g rounded, then the subtraction)
        if k > 0:   # and not the unscheduled lr
            assert not torch.equal(eng.params, before - eng.grads * float(np.float32(0.05)))
        assert eng.engines[0].m.abs().max().item() == 0.0


def _write_pair(root, h=72, w=96, seed=50):
    from PIL import Image
    A, B = synth.smooth_image_pair(seed, 0, h, w)
    for name, img in (("A", A), ("B", B)):
        d = root / name
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")


def test_train_model_rmsprop_cosine(tmp_path, capsys):
    from splice_amd.train import train_model
    _write_pair(tmp_path)
    over = dict(seed=3, n_epochs=50, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=25,
                optimizer="rmsprop", scheduler_policy="cosine")
    eng = train_model(str(tmp_path), cfg_overrides=over, vit_state=synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))
    assert (tmp_path / "out" / "output.png").exists()
    assert eng.step_idx == 49 and np.isfinite(eng.losses()["loss"])
    want = LrSchedule(dict(eng.cfg)).lr(49)
    assert eng.lr == want and want < 1e-4
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("Epoch ")]
    assert lines[0].endswith(f" lr={eng.cfg['lr']}")   # step 0: the base lr
    assert lines[-1].startswith("Epoch 50:") and lines[-1].endswith(f" lr={want}"), lines


def test_batch_forwards_optimizer_and_schedule(tmp_path, monkeypatch):
    """splice_amd.batch hands the overrides to train_model in its worker: same loss as the run in this process."""
    from splice_amd import batch
    from splice_amd.train import train_model
    monkeypatch.setenv("SPLICE_SYNTHETIC_WEIGHTS", "1")
    over = dict(seed=3, n_epochs=6, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=3,
                optimizer="sgd", scheduler_policy="step", scheduler_lr_decay_iters=2)
    for r in ("queue", "serial"):
        _write_pair(tmp_path / r / "p0", 64, 80, seed=60)
    res = batch.run_batch(str(tmp_path / "queue"), 1, over)
    eng = train_model(str(tmp_path / "serial" / "p0"), cfg_overrides=over, progress=False)
    assert res[0]["steps"] == 6 and eng.lr == 0.002 * 0.5 ** 2
    assert eng.losses()["loss"] == res[0]["loss"]
