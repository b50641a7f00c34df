"""CPU: the host side of the key second-moment appearance term (``lambda_global_key_gram`` / ``dino_gram_layer``):
defaults, every refusal by name before a GPU is touched, the float64 restatement against torch autograd, the facade and the bindings."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, KEY_GRAM_KEYS, KEY_GRAM_LOSS_KEY, LOSS_KEYS, PAIR_KEYS, SNAPSHOT_FREE_KEYS, MultiPairEngine, MultiScaleEngine,
                               SpliceEngine, active_terms, key_gram_active, key_gram_rule, merge_pair_cfgs, np_key_gram, snapshot_cfg_mismatch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM, LAYER = KEY_GRAM_KEYS


def test_the_keys_are_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    assert KEY_GRAM_KEYS == ("lambda_global_key_gram", "dino_gram_layer") and KEY_GRAM_LOSS_KEY == "loss_global_key_gram"
    for cfg in (DEFAULT_CFG, packaged):
        assert cfg[LAM] == 0.0 and cfg[LAYER] is None
        assert key_gram_rule(cfg, 12) is None
    assert key_gram_rule({}, 12) is None and key_gram_rule({LAM: 0}, 12) is None and key_gram_rule({LAM: 0.0, LAYER: None}, 12) is None
    assert not set(PAIR_KEYS) & set(KEY_GRAM_KEYS) and not set(SNAPSHOT_FREE_KEYS) & set(KEY_GRAM_KEYS)
    assert KEY_GRAM_LOSS_KEY not in LOSS_KEYS   # (the [P][8] losses row keeps its words)


def test_the_rule_gives_the_weight_and_the_block():
    assert key_gram_rule({LAM: 2.5}, 12) == (2.5, 11)           # null = the top block of that ViT
    assert key_gram_rule({LAM: 2.5}, 6) == (2.5, 5)
    assert key_gram_rule({LAM: 1, LAYER: 5}, 12) == (1.0, 5)
    assert key_gram_rule({LAM: np.float32(0.5), LAYER: np.int64(0)}, 12) == (0.5, 0)
    lam, layer = key_gram_rule({LAM: 3, LAYER: 11}, 12)
    assert type(lam) is float and type(layer) is int


@pytest.mark.parametrize("bad", [-1.0, -1e-30, float("nan"), float("inf"), 1e39, 1e-60, True, "1", None, [1.0]])
def test_a_bad_weight_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="'lambda_global_key_gram'"):
        key_gram_rule({LAM: bad}, 12)


@pytest.mark.parametrize("bad", [-1, 12, 1.0, True, "5", [5], (5,)])
def test_a_bad_layer_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="'dino_gram_layer'"):
        key_gram_rule({LAM: 1.0, LAYER: bad}, 12)


def test_the_layer_is_checked_against_the_depth_given_and_needs_the_weight():
    assert key_gram_rule({LAM: 1.0, LAYER: 5}, 6) == (1.0, 5)
    with pytest.raises(ValueError, match="'dino_gram_layer'"):
        key_gram_rule({LAM: 1.0, LAYER: 6}, 6)
    with pytest.raises(ValueError, match="'dino_gram_layer' needs 'lambda_global_key_gram'"):
        key_gram_rule({LAYER: 5}, 12)
    with pytest.raises(ValueError, match="'dino_gram_layer' needs 'lambda_global_key_gram'"):
        key_gram_rule({LAM: 0.0, LAYER: 11}, 12)


@pytest.mark.parametrize("key,val", [(LAM, 2.0), (LAYER, 5)])
def test_keys_are_shared_by_the_slots_of_a_sweep(key, val):
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs({LAM: 1.0, LAYER: 7}, [{key: val}, {}])
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs({}, [{}, {key: val}])
    assert len(merge_pair_cfgs({LAM: 2.0, LAYER: 5}, [{key: val}, {"lambda_global_identity": 2.0}])) == 2   # (the base value itself is no per-slot value)


def test_snapshot_config_comparison_sees_the_keys():
    assert snapshot_cfg_mismatch({LAM: 1.0}, {}) == LAM
    assert snapshot_cfg_mismatch({LAM: 1.0, LAYER: 5}, {LAM: 1.0, LAYER: 11}) == LAYER
    assert snapshot_cfg_mismatch({LAM: 1.0, LAYER: 5}, {LAM: 1.0, LAYER: 5}) is None and snapshot_cfg_mismatch({LAM: 0.0, LAYER: None}, {}) is None


def test_the_term_is_active_from_the_warm_up_on_beside_active_terms():
    c = dict(DEFAULT_CFG, cls_warmup=3, **{LAM: 1.0})
    assert [key_gram_active(c, s) for s in (0, 2, 3, 4, 75)] == [False, False, True, True, True]   # (entire-image steps included)
    assert not key_gram_active(dict(DEFAULT_CFG, cls_warmup=0), 5)
    assert KEY_GRAM_LOSS_KEY not in active_terms(c, 5, True)   # (that dict keeps its keys)


def _cfg(**kw):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **kw)


def test_engines_refuse_on_the_host_before_anything_touches_a_gpu(monkeypatch):
    """Every constructor raises from the host checks at its head: the library is never asked for (a lib() call would fail the test)."""
    def no_lib():
        raise AssertionError("the library was loaded before the host checks were done")
    monkeypatch.setattr(_lib, "lib", no_lib)
    for bad, key in (({LAM: -1.0}, LAM), ({LAM: float("nan")}, LAM), ({LAM: float("inf")}, LAM), ({LAM: 1.0, LAYER: 12}, LAYER), ({LAM: 1.0, LAYER: -1}, LAYER),
                     ({LAYER: 5}, LAYER), ({LAM: 0.0, LAYER: 11}, LAYER)):
        with pytest.raises(ValueError, match=f"'{key}'"):
            SpliceEngine(_cfg(**bad), None, None, (64, 64), device="cpu")
        with pytest.raises(ValueError, match=f"'{key}'"):
            MultiPairEngine(_cfg(**bad), None, [None, None], (64, 64), device="cpu")
    for fp8 in (True, "gemm", "attention"):
        with pytest.raises(ValueError, match="'lambda_global_key_gram'.*fp8"):
            SpliceEngine(_cfg(**{LAM: 1.0}), None, None, (64, 64), device="cpu", fp8=fp8)
    # a per-slot value
    for key, val in ((LAM, 1.0), (LAYER, 5)):
        with pytest.raises(ValueError, match=f"'{key}' is shared"):
            MultiPairEngine(_cfg(), None, [None, None], (64, 64), device="cpu", pair_cfgs=[{key: val}, {}])
    # several pairs with different crop counts per side
    with pytest.raises(ValueError, match="'lambda_global_key_gram'.*crop counts"):
        MultiPairEngine(_cfg(**{LAM: 1.0}), None, [None, None], (64, 64), device="cpu", n_crops=(2, 1))
    # the several-scales engine
    with pytest.raises(NotImplementedError, match="lambda_global_key_gram"):
        MultiScaleEngine(_cfg(**{LAM: 1.0, LAYER: 5}), None, None, (64, 64), scales=(64, 96), device="cpu")
    with pytest.raises(ValueError, match=f"'{LAYER}'"):   # (a bad value is a bad value there too)
        MultiScaleEngine(_cfg(**{LAM: 1.0, LAYER: 12}), None, None, (64, 64), scales=(64, 96), device="cpu")


@pytest.mark.parametrize("T", [5, 65])
def test_np_key_gram_against_torch_autograd_in_float64(T):
    D, lam = 64, 1.7
    rng = np.random.default_rng(100 + T)
    kx, kb = rng.standard_normal((T, D)), rng.standard_normal((T, D)) * 0.8 + 0.1
    raw, dk = np_key_gram(kx, kb, lam)
    x = torch.from_numpy(kx).requires_grad_(True)
    b = torch.from_numpy(kb)
    want = torch.nn.functional.mse_loss(x.T @ x / T, b.T @ b / T)
    (lam * want).backward()
    assert dk.shape == (T, D) and dk.dtype == np.float64 and isinstance(raw, float)
    assert abs(raw - want.item()) <= 1e-10 * abs(want.item())
    g = x.grad.numpy()
    assert np.abs(dk - g).max() <= 1e-10 * np.abs(g).max()
    assert np.linalg.norm(dk - g) <= 1e-10 * np.linalg.norm(g)
    # the target carries no gradient and equal keys give zero
    raw0, dk0 = np_key_gram(kx, kx, lam)
    assert raw0 == 0.0 and not dk0.any()


def test_result_fields_carry_the_keys_where_the_term_is_on():
    from types import SimpleNamespace
    from splice_amd.train import key_gram_fields
    assert key_gram_fields(SimpleNamespace(cfg=dict(DEFAULT_CFG))) == {}
    assert key_gram_fields(SimpleNamespace(key_gram=None)) == {}
    assert key_gram_fields(SimpleNamespace(key_gram=(2.0, 5))) == {LAM: 2.0, LAYER: 5}


class _StubExtractor:
    """``get_keys_from_input(img, layer_num)``: a [heads][T][d] tensor, a differentiable function of the image that differs per block."""
    H, T, d = 2, 5, 4

    def __init__(self):
        self.calls = []

    def get_keys_from_input(self, img, layer_num):
        self.calls.append(layer_num)
        n = self.H * self.T * self.d
        return (layer_num + 1) * (img.mean(dim=(0, 1)).reshape(-1)[:n].reshape(self.H, self.T, self.d) - 0.4)


def test_lossg_facade_equals_np_key_gram():
    from splice_amd.losses import LossG
    rng = np.random.default_rng(9)
    off = dict(lambda_global_ssim=0, lambda_global_cls=0, lambda_entire_cls=0, lambda_entire_ssim=0, lambda_global_identity=0)
    cfg = dict(_cfg(**off), cls_warmup=1, **{LAM: 3.0, LAYER: 5})
    ex = _StubExtractor()
    loss_g = LossG(cfg, extractor=ex)
    assert loss_g.key_gram == (3.0, 5)
    x = torch.from_numpy(rng.random((2, 3, 64, 64))).double().requires_grad_(True)
    b = torch.from_numpy(rng.random((3, 3, 64, 64))).double()   # (one crop more on the target side: the zip drops it)
    loss_g.global_transform = lambda img: img   # (the HIP Resize is not what this test is about)
    assert set(loss_g({"x_global": x}, {"step": 0, "B_global": b})) == {"loss"}   # (before the warm-up step: off)
    ex.calls.clear()
    out = loss_g({"x_global": x}, {"step": 1, "B_global": b})
    assert set(out) == {"loss", KEY_GRAM_LOSS_KEY} and ex.calls == [5, 5] * 2

    def keys(img):   # the stub's block-5 keys as [T][heads * d], float64
        n = ex.H * ex.T * ex.d
        k = 6 * (img.detach().numpy().mean(0).reshape(-1)[:n].reshape(ex.H, ex.T, ex.d) - 0.4)
        return k.transpose(1, 0, 2).reshape(ex.T, ex.H * ex.d)
    want = sum(np_key_gram(keys(x[i]), keys(b[i]), 3.0)[0] for i in range(2))
    assert abs(out[KEY_GRAM_LOSS_KEY].item() - want) <= 1e-10 * abs(want)
    assert abs(out["loss"].item() - 3.0 * want) <= 1e-10 * abs(3.0 * want)
    assert abs(loss_g.calculate_key_gram_loss(x.detach(), b).item() - want) <= 1e-10 * abs(want)
    out["loss"].backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    # absent keys: no such term
    plain = LossG({k: v for k, v in cfg.items() if k not in KEY_GRAM_KEYS}, extractor=_StubExtractor())
    plain.global_transform = lambda img: img
    assert plain.key_gram is None and set(plain({"x_global": x.detach()}, {"step": 1, "B_global": b})) == {"loss"}


def test_binding_and_header_agree_on_the_new_entry_points():
    names = ("splice_step_set_key_gram", "splice_step_key_gram_values", "splice_key_gram_pairs")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splice_hip.h")).read(), flags=re.S)
    for n in names:
        assert n in _lib._SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
        args = re.search(r"\b%s\s*\((.*?)\);" % n, header, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[n][0]), n
    assert len(_lib._SIGNATURES["splice_key_gram_pairs"][0]) == 21
    lib = _lib.lib()   # (loads without a GPU: the exports are there)
    for n in names:
        assert hasattr(lib, n), n
