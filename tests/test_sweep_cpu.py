"""CPU: the host side of hyper-parameter sweeps (per-slot configs inside one MultiPairEngine): variant validation refuses
before anything touches the GPU, ``--sweep`` forms the cartesian product in argument order, ``run_batch(sweep=...)`` makes one
work item per pair, and the new C exports are declared, bound and present."""
import ctypes
import json
import os

import numpy as np
import pytest

from splice_amd import _lib, batch, synth
from splice_amd.engine import MAX_PAIR_CFGS, PAIR_KEYS, MultiPairEngine, merge_pair_cfgs


def _engine(pair_cfgs, cfg=None, n_crops=1):
    # device="cpu", no ViT state: every refusal below must come before the engine touches a GPU
    return MultiPairEngine(dict(cfg or {}), None, [{}] * len(pair_cfgs), (64, 64), (64, 64), device="cpu", n_crops=n_crops, pair_cfgs=pair_cfgs)


def test_every_per_slot_key_is_allowed():
    variants = [dict(lambda_global_cls=1.0, lambda_global_ssim=0.5, lambda_global_identity=0.0, lambda_entire_cls=3, lambda_entire_ssim=0,
                     lr=1e-3, scheduler_policy="step", scheduler_lr_decay_iters=2, seed=5, init_type="normal", init_gain=0.1),
                dict(scheduler_policy="linear", scheduler_n_epochs_decay=7)]
    cfgs = merge_pair_cfgs(dict(n_epochs=9), variants)
    assert cfgs[0]["lambda_global_ssim"] == 0.5 and cfgs[0]["scheduler_policy"] == "step" and cfgs[0]["n_epochs"] == 9
    assert cfgs[1]["lambda_global_ssim"] == 1.0 and cfgs[1]["scheduler_n_epochs_decay"] == 7
    assert set(PAIR_KEYS) == set(variants[0]) | {"scheduler_n_epochs_decay"}


@pytest.mark.parametrize("key,value", [("optimizer", "sgd"), ("optimizer_beta1", 0.5), ("optimizer_beta2", 0.9), ("cls_warmup", 3),
                                       ("entire_A_every", 5), ("n_epochs", 11), ("log_images_freq", 3), ("dino_model_name", "dino_vits8"),
                                       ("dino_global_patch_size", 96), ("fp8", True), ("direction", "BtoA"), ("A_resize", 128),
                                       ("global_A_crops_n_crops", 2), ("use_augmentations", False)])
def test_shared_key_refused_by_name_before_the_gpu(key, value):
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        _engine([{}, {key: value}])


def test_shared_key_at_the_base_value_is_accepted():
    cfgs = merge_pair_cfgs(dict(optimizer="sgd"), [dict(optimizer="sgd", lr=0.1), dict(lr=0.2)])
    assert [c["lr"] for c in cfgs] == [0.1, 0.2]


def test_entire_branch_disagreement_refused():
    with pytest.raises(ValueError, match="entire-image branch"):
        _engine([dict(lambda_entire_cls=0, lambda_entire_ssim=0), {}])
    # a zero term inside an active branch is fine
    merge_pair_cfgs({}, [dict(lambda_entire_cls=0), dict(lambda_entire_ssim=0)])


def test_too_many_slots_refused():
    with pytest.raises(ValueError, match=f"at most {MAX_PAIR_CFGS}"):
        _engine([{}] * (MAX_PAIR_CFGS + 1))
    assert MAX_PAIR_CFGS == 32


def test_bad_slot_values_refused():
    with pytest.raises(ValueError, match="lambda_global_cls"):
        _engine([dict(lambda_global_cls=-1.0), {}])
    with pytest.raises(NotImplementedError, match="plateau"):
        _engine([dict(scheduler_policy="plateau"), {}])
    with pytest.raises(ValueError, match="2 generator states"):
        MultiPairEngine({}, None, [{}, {}], (64, 64), device="cpu", pair_cfgs=[{}])


def test_n_crops_refused():
    with pytest.raises(ValueError, match="n_crops"):
        _engine([{}], n_crops=2)


def test_train_sweep_refusals_before_the_gpu(tmp_path):
    from splice_amd.train import train_sweep
    with pytest.raises(NotImplementedError, match="n_crops"):
        train_sweep(str(tmp_path), [{}, {}], cfg_overrides=dict(global_A_crops_n_crops=2))
    with pytest.raises(NotImplementedError, match="dino_global_scales"):
        train_sweep(str(tmp_path), [{}, {}], cfg_overrides=dict(dino_global_scales=[224, 320]))
    with pytest.raises(ValueError, match="'optimizer' is shared"):
        train_sweep(str(tmp_path), [{}, dict(optimizer="sgd")])


def test_sweep_specs_product_order_and_types():
    v = batch.sweep_variants(["lr=0.001,0.002", "lambda_global_ssim=1,0.5,0", "scheduler_policy=none,cosine"])
    assert len(v) == 12
    assert v[0] == dict(lr=0.001, lambda_global_ssim=1, scheduler_policy="none")
    assert v[1] == dict(lr=0.001, lambda_global_ssim=1, scheduler_policy="cosine")
    assert v[2] == dict(lr=0.001, lambda_global_ssim=0.5, scheduler_policy="none")
    assert v[-1] == dict(lr=0.002, lambda_global_ssim=0, scheduler_policy="cosine")
    assert isinstance(v[0]["lambda_global_ssim"], int) and isinstance(v[2]["lambda_global_ssim"], float) and isinstance(v[0]["lr"], float)
    with pytest.raises(ValueError, match="KEY=V1"):
        batch.sweep_variants(["lr"])
    with pytest.raises(ValueError, match="twice"):
        batch.sweep_variants(["lr=1,2", "lr=3"])


def test_sweep_cli_refuses_pairs_per_gpu(tmp_path):
    with pytest.raises(SystemExit, match="--sweep"):
        batch.main(["--root", str(tmp_path), "--sweep", "lr=0.1,0.2", "--pairs-per-gpu", "2"])
    with pytest.raises(ValueError, match="pairs_per_gpu"):
        batch.run_batch(str(tmp_path), 1, {}, pairs_per_gpu=2, sweep=[{}, {}])


def stub_sweep_runner(pair_dir, overrides, variants):
    """Stand-in for train_sweep_runner: records what the worker handed over."""
    return {"pair_dir": os.path.basename(pair_dir), "overrides": overrides, "variants": variants, "pid": os.getpid()}


def _make_pairs(root, k):
    for i in range(k):
        A, B = synth.image_pair(99, i, 8, 8)
        for side, img in (("A", A), ("B", B)):
            d = root / f"pair{i:02d}" / side
            d.mkdir(parents=True)
            np.save(d / "img.npy", img)


def test_run_batch_sweep_one_item_per_pair(tmp_path):
    _make_pairs(tmp_path, 3)
    res = batch.run_batch(str(tmp_path), 2, dict(n_epochs=4), runner=stub_sweep_runner, pin_gpu=False, sweep=["lr=0.1,0.2", "seed=1,2"])
    want = [dict(lr=0.1, seed=1), dict(lr=0.1, seed=2), dict(lr=0.2, seed=1), dict(lr=0.2, seed=2)]
    assert [r["pair"] for r in res] == ["pair00", "pair01", "pair02"]
    for r in res:
        assert r["pair_dir"] == r["pair"] and r["overrides"] == dict(n_epochs=4) and r["variants"] == want
        with open(tmp_path / r["pair"] / "out" / "result.json") as f:
            assert json.load(f)["variants"] == want
    # variant dicts are taken as they are
    res = batch.run_batch(str(tmp_path), 1, {}, runner=stub_sweep_runner, pin_gpu=False, sweep=[dict(lr=0.3), dict(lr=0.4)])
    assert all(r["variants"] == [dict(lr=0.3), dict(lr=0.4)] for r in res)


def test_sweep_exports_bound_and_present():
    names = ("splice_step_set_pair_weights", "splice_step_set_pair_lr", "splice_optim_step_pairs")
    assert set(names) <= set(_lib.exported_symbols())
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splice_hip.h")) as f:
        header = f.read()
    assert all(f"int {n}(" in header for n in names)
    assert "#define SPLICE_STEP_MAX_PAIR_CFGS 32" in header
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert all(hasattr(lib, n) for n in names)
