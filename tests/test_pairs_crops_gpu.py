"""GPU: several pairs per step with several global crops per image.  Pair p of an engine with P pairs and (nA, nB) crops per pair
is bit for bit the ``SpliceEngine(n_crops=(nA, nB))`` run of that pair: losses, parameters, optimiser moments, BatchNorm running
statistics and ``num_batches_tracked``.  At op level, a generator plan of P groups of g images (``groups=g`` + an arena stride) is
bit for bit P batch-statistics plans of g images."""
import ctypes as C

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import MultiPairEngine, SpliceEngine
from splice_amd.generator import GeneratorEngine, GeneratorPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _running_update(plan, run, stride):
    plans = (C.c_void_p * 1)(plan.handle)
    _lib.check(_lib.lib().splice_gen_running_stats_update(plans, 1, _lib.ptr(run), stride, 0.1, _lib.current_stream()))


@pytest.mark.parametrize("hw", [(64, 64), (96, 130), (224, 224)])
@pytest.mark.parametrize("g", [2, 3])
@pytest.mark.parametrize("P", [2, 3])
def test_grouped_plan_equals_batch_stat_plans(P, g, hw):
    """P groups of g images in one plan == P batch-statistics plans of g images: output, every arena's gradient and the running
    statistics bit for bit ((96, 130): odd plane sizes; (224, 224): the big-plane segment kernels and the split-K policies)."""
    gen = GeneratorEngine(device=DEV)
    n = gen.numel
    stride = (n + 63) // 64 * 64
    H, W = hw
    params = torch.zeros(P * stride, device=DEV)
    for p in range(P):
        params[p * stride: p * stride + n] = gen.flatten(synth.generator_params(70 + p, 0.02, perturb_bias=0.05))
    x = torch.from_numpy(np.stack([synth.uniform(8, f"pc/x{i}", (3, H, W)) for i in range(P * g)])).to(DEV)
    dy = torch.from_numpy(np.stack([synth.normal(9, f"pc/dy{i}", (3, H, W)) for i in range(P * g)])).to(DEV)
    plan = GeneratorPlan(gen, P * g, H, W, True, stride, groups=g)
    y = plan.forward(params, x)
    grads = plan.backward(params, dy)
    assert grads.numel() == P * stride
    run = torch.zeros(P, gen.buffer_numel, device=DEV)
    _running_update(plan, run, run.stride(0))
    for p in range(P):
        single = GeneratorPlan(gen, g, H, W, True, batch_stats=True)
        pp = params[p * stride: p * stride + n].clone()
        sl = slice(p * g, (p + 1) * g)
        y1 = single.forward(pp, x[sl].contiguous())
        g1 = single.backward(pp, dy[sl].contiguous())
        r1 = torch.zeros(gen.buffer_numel, device=DEV)
        _running_update(single, r1, 0)
        assert torch.equal(y[sl], y1), (p, (y[sl] - y1).abs().max().item())
        assert torch.equal(grads[p * stride: p * stride + n], g1), (p, (grads[p * stride: p * stride + n] - g1).abs().max().item())
        assert torch.equal(run[p], r1), p
    assert not torch.equal(y[0], y[g])


def test_set_groups_refusals():
    gen = GeneratorEngine(device=DEV)
    plan = GeneratorPlan(gen, 6, 64, 64, True)
    lib = _lib.lib()
    assert lib.splice_gen_plan_set_groups(plan.handle, 4) != 0      # 6 % 4
    assert b"multiple" in lib.splice_last_error()
    assert lib.splice_gen_plan_set_groups(plan.handle, 9) != 0      # > 8
    assert b"1..8" in lib.splice_last_error()
    assert lib.splice_gen_plan_set_groups(plan.handle, 3) != 0      # two groups without an arena stride
    assert b"arena stride" in lib.splice_last_error()
    assert lib.splice_gen_plan_set_groups(plan.handle, 6) == 0      # one group: batch statistics
    assert lib.splice_gen_plan_set_groups(plan.handle, 1) == 0      # independent images


def _cfg(**kw):
    return dict(dict(dino_model_name="dino_vits8", dino_global_patch_size=64, entire_A_every=3, cls_warmup=1), **kw)


def _crop_inputs(P, nA, nB, seed):
    """[P*nA,3,64,64] / [P*nB,3,64,64] crops (pair-major) of P 72x80 pairs, and the [P,3,72,80] entire structure images."""
    As, Bs = zip(*[synth.smooth_image_pair(seed, p, 72, 80) for p in range(P)])
    offs_a = [(0, 0), (8, 16), (4, 9)]
    offs_b = [(8, 0), (0, 16), (3, 7)]
    Ac = torch.stack([torch.from_numpy(As[p])[:, t:t + 64, l:l + 64] for p in range(P) for t, l in offs_a[:nA]]).contiguous().to(DEV)
    Bc = torch.stack([torch.from_numpy(Bs[p])[:, t:t + 64, l:l + 64] for p in range(P) for t, l in offs_b[:nB]]).contiguous().to(DEV)
    Ae = torch.from_numpy(np.stack(As)).contiguous().to(DEV)
    return Ac, Bc, Ae


def _step_inputs(Ac, Bc, i):
    """crop sizes change between steps: 64 / 56 / (A 64, B 48) / 64"""
    if i == 1:
        return Ac[:, :, :56, :56].contiguous(), Bc[:, :, :56, :56].contiguous()
    if i == 2:
        return Ac, Bc[:, :, 4:52, 2:50].contiguous()
    return Ac, Bc


@pytest.mark.parametrize("P,n_crops,opt", [(2, 2, "adam"), (3, 2, "sgd"), (2, (3, 2), "rmsprop"), (3, (3, 2), "adam"), (2, (1, 3), "sgd"),
                                           (3, (1, 3), "rmsprop")])
def test_pairs_with_crops_equal_single_pair_crop_runs(P, n_crops, opt):
    """4 steps: entire-image step 0 (before the [CLS] warm-up ends), new crop sizes at steps 1 and 2, entire step 3 again.
    Per step the loss row of every pair; at the end parameters, moments, running statistics and num_batches_tracked."""
    over = dict(optimizer=opt)
    if opt == "rmsprop":
        over.update(scheduler_policy="cosine", n_epochs=6)
    cfg = _cfg(**over)
    nA, nB = (n_crops, n_crops) if isinstance(n_crops, int) else n_crops
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    gens = [synth.generator_params(100 + p, 0.02) for p in range(P)]
    Ac, Bc, Ae = _crop_inputs(P, nA, nB, 91)
    multi = MultiPairEngine(cfg, vit_state, gens, (64, 64), (72, 80), n_crops=n_crops)
    hist = []
    for i in range(4):
        a, b = _step_inputs(Ac, Bc, i)
        multi.step(a, b, Ae)
        hist.append(multi.losses_dev.clone())
    torch.cuda.synchronize()
    assert len(multi.losses()) == P
    n = multi.gen.numel
    for p in range(P):
        single = SpliceEngine(cfg, None, gens[p], (64, 64), (72, 80), vit_engine=multi.vit, n_crops=n_crops)
        for i in range(4):
            a, b = _step_inputs(Ac, Bc, i)
            single.step(a[p * nA:(p + 1) * nA].contiguous(), b[p * nB:(p + 1) * nB].contiguous(), Ae[p].contiguous())
            assert torch.equal(single.losses_dev[0], hist[i][p]), (p, i, single.losses_dev[0], hist[i][p])
        torch.cuda.synchronize()
        assert torch.equal(single.params, multi.pair_params(p)), (p, (single.params - multi.pair_params(p)).abs().max().item())
        assert torch.equal(single.m, multi.m[p * multi.stride: p * multi.stride + n])
        assert torch.equal(single.v, multi.v[p * multi.stride: p * multi.stride + n])
        assert torch.equal(single.running[0], multi.running[p])
        one, got = single.state_dict(), multi.state_dict(p)
        for k in one:
            assert torch.equal(one[k], got[k]), (p, k)
        assert single.generator_calls[0] == multi.generator_calls[p] == 2 * 4 + 2
    assert not torch.equal(multi.pair_params(0), multi.pair_params(1))


def test_pairs_with_crops_accept_stacked_layout_and_refuse_too_many_images():
    cfg = _cfg()
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    gens = [synth.generator_params(120 + p, 0.02) for p in range(2)]
    Ac, Bc, Ae = _crop_inputs(2, 2, 2, 92)
    flat = MultiPairEngine(cfg, vit_state, gens, (64, 64), (72, 80), n_crops=2)
    stacked = MultiPairEngine(cfg, None, gens, (64, 64), (72, 80), n_crops=2, vit_engine=flat.vit)
    for _ in range(2):
        flat.step(Ac, Bc, Ae)
        stacked.step(Ac.view(2, 2, 3, 64, 64), Bc.view(2, 2, 3, 64, 64), Ae)
    torch.cuda.synchronize()
    assert torch.equal(flat.params, stacked.params) and torch.equal(flat.losses_dev, stacked.losses_dev)
    with pytest.raises(ValueError, match="images per side"):
        MultiPairEngine(cfg, None, [gens[0]] * 17, (64, 64), (72, 80), n_crops=2, vit_engine=flat.vit)


def test_full_size_pairs_with_crops_graph_and_eager_equal_single_runs():
    """224x224, ViT-B/8, P = 4 pairs x 2 crops with fixed crops: steps 2 and 3 capture and replay a graph.  Graph + overlap and
    eager + serial give the same bits, and pairs 0 and 3 equal their single-pair n_crops = 2 runs (which capture graphs too)."""
    P, nc = 4, 2
    cfg = dict(dino_model_name="dino_vitb8", dino_global_patch_size=224)
    vit_state = synth.vit_params(7, "dino_vitb8", img_size=224, w_std=0.03)
    gens = [synth.generator_params(130 + p, 0.02) for p in range(P)]
    imgs = [synth.smooth_image_pair(93, k, 224, 224) for k in range(P * nc)]
    A = torch.from_numpy(np.stack([a for a, _ in imgs])).to(DEV)
    B = torch.from_numpy(np.stack([b for _, b in imgs])).to(DEV)
    Ae = A[::nc].contiguous()
    ref, vit = None, None
    for graph, overlap in ((1, 1), (0, 0)):
        multi = MultiPairEngine(cfg, vit_state if vit is None else None, gens, (224, 224), (224, 224), vit_engine=vit, n_crops=nc)
        vit = multi.vit
        _lib.check(_lib.lib().splice_step_use_graph(multi.handle, graph))
        _lib.check(_lib.lib().splice_step_use_overlap(multi.handle, overlap))
        for _ in range(4):
            multi.step(A, B, Ae)
        torch.cuda.synchronize()
        if graph:
            st = (C.c_longlong * 3)()
            _lib.check(_lib.lib().splice_step_graph_stats(multi.handle, st))
            assert st[0] + st[2] >= 1   # a graph was captured (and replayed)
        if ref is None:
            ref = (multi.params.clone(), multi.losses_dev.clone(), multi.running.clone())
        else:
            assert torch.equal(multi.params, ref[0]) and torch.equal(multi.losses_dev, ref[1]) and torch.equal(multi.running, ref[2])
    stride, n = multi.stride, multi.gen.numel
    del multi
    for p in (0, P - 1):
        single = SpliceEngine(cfg, None, gens[p], (224, 224), (224, 224), vit_engine=vit, n_crops=nc)
        for _ in range(4):
            single.step(A[p * nc:(p + 1) * nc].contiguous(), B[p * nc:(p + 1) * nc].contiguous(), Ae[p].contiguous())
        torch.cuda.synchronize()
        assert torch.equal(single.losses_dev[0], ref[1][p]), (p, single.losses_dev[0], ref[1][p])
        assert torch.equal(single.params, ref[0][p * stride: p * stride + n]), (p, (single.params - ref[0][p * stride: p * stride + n]).abs().max().item())
        assert torch.equal(single.running[0], ref[2][p])
        del single


OVER = dict(seed=3, n_epochs=9, dino_model_name="dino_vits8", dino_global_patch_size=64, log_images_freq=4, use_augmentations=False,
            global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0, global_A_crops_n_crops=2, global_B_crops_n_crops=2)


def _write_pairs(root, k, h=72, w=72):
    from PIL import Image
    for i in range(k):
        A, B = synth.smooth_image_pair(61, i, h, w)
        for side, img in (("A", A), ("B", B)):
            d = root / f"p{i}" / side
            d.mkdir(parents=True)
            Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")


def test_train_pairs_with_crops_equal_single_runs(tmp_path, monkeypatch):
    """train_pairs with global_{A,B}_crops_n_crops = 2 and deterministic full crops: every pair's state_dict and output.png
    equal its own train_model run."""
    from splice_amd.train import train_model, train_pairs
    monkeypatch.setenv("SPLICE_SYNTHETIC_WEIGHTS", "1")
    grouped, serial = tmp_path / "grouped", tmp_path / "serial"
    for r in (grouped, serial):
        r.mkdir()
        _write_pairs(r, 2)
    both = train_pairs([str(grouped / f"p{i}") for i in range(2)], cfg_overrides=OVER, progress=False)
    assert both.n_crops_ab == (2, 2) and both.slots_ab == (4, 4)
    for i in range(2):
        one = train_model(str(serial / f"p{i}"), cfg_overrides=OVER, progress=False)
        want, got = one.state_dict(), both.state_dict(i)
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k], want[k]), (i, k)
        assert (serial / f"p{i}" / "out" / "output.png").read_bytes() == (grouped / f"p{i}" / "out" / "output.png").read_bytes()


def test_run_batch_pairs_per_gpu_with_crops_equals_one_per_gpu(tmp_path, monkeypatch):
    from splice_amd import batch
    monkeypatch.setenv("SPLICE_SYNTHETIC_WEIGHTS", "1")
    g2, g1 = tmp_path / "g2", tmp_path / "g1"
    for r in (g2, g1):
        r.mkdir()
        _write_pairs(r, 2)
    res2 = batch.run_batch(str(g2), 1, OVER, pairs_per_gpu=2)
    res1 = batch.run_batch(str(g1), 1, OVER, pairs_per_gpu=1)
    assert [r.get("pairs_in_step", 1) for r in res2] == [2, 2]
    for i in range(2):
        assert res2[i]["loss"] == res1[i]["loss"], (i, res2[i]["loss"], res1[i]["loss"])
        assert (g2 / f"p{i}" / "out" / "output.png").read_bytes() == (g1 / f"p{i}" / "out" / "output.png").read_bytes()
