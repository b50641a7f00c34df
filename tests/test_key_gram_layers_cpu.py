"""CPU: the host side of the key second-moment term over several ViT blocks and of its centred form (``dino_gram_layers`` /
``dino_gram_layer_weights`` / ``dino_gram_centered``): defaults, the canonical form, every refusal by name before a
GPU is touched, the float64 restatement against torch autograd, the facade, the result fields and the bindings."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, KEY_GRAM_KEYS, KEY_GRAM_LAYER_KEYS, KEY_GRAM_LOSS_KEY, MAX_KEY_GRAM_LAYERS, PAIR_KEYS, SNAPSHOT_FREE_KEYS, MultiPairEngine,
                               MultiScaleEngine, SpliceEngine, key_gram_canonical, key_gram_layers_rule, key_gram_rule, merge_pair_cfgs, np_key_gram,
                               np_key_gram_layers, snapshot_cfg_mismatch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM, LAYER = KEY_GRAM_KEYS
LAYERS, WEIGHTS, CENTERED = KEY_GRAM_LAYER_KEYS


def test_the_keys_are_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    assert KEY_GRAM_LAYER_KEYS == ("dino_gram_layers", "dino_gram_layer_weights", "dino_gram_centered") and MAX_KEY_GRAM_LAYERS == 12
    assert KEY_GRAM_KEYS == ("lambda_global_key_gram", "dino_gram_layer")   # (the old tuple keeps its two keys)
    for cfg in (DEFAULT_CFG, packaged):
        assert cfg[LAYERS] is None and cfg[WEIGHTS] is None and cfg[CENTERED] is False
        assert key_gram_layers_rule(cfg, 12) is None and key_gram_rule(cfg, 12) is None
    assert key_gram_layers_rule({}, 12) is None and key_gram_layers_rule({LAM: 2.0}, 12) is None and key_gram_layers_rule({LAM: 2.0, LAYER: 5}, 12) is None
    assert not set(PAIR_KEYS) & set(KEY_GRAM_LAYER_KEYS) and not set(SNAPSHOT_FREE_KEYS) & set(KEY_GRAM_LAYER_KEYS)


def test_the_rule_gives_the_canonical_form():
    assert key_gram_layers_rule({LAM: 2.0, LAYERS: [11, 2, 7]}, 12) == (2.0, [2, 7, 11], [1.0, 1.0, 1.0], False)
    assert key_gram_layers_rule({LAM: 2.0, LAYERS: [11, 2, 7], WEIGHTS: [3, 0.5, 1]}, 12) == (2.0, [2, 7, 11], [0.5, 1.0, 3.0], False)   # (a weight stays beside its block)
    assert key_gram_layers_rule({LAM: 1, LAYERS: (2, 5), CENTERED: True}, 12) == (1.0, [2, 5], [1.0, 1.0], True)
    assert key_gram_layers_rule({LAM: 1.0, LAYERS: [2, 5]}, 12)[1] == [2, 5]   # (the top block is not required)
    assert key_gram_layers_rule({LAM: 1.0, LAYERS: list(range(12))}, 12)[1] == list(range(12))
    lam, layers, weights, centered = key_gram_layers_rule({LAM: np.float32(0.5), LAYERS: [np.int64(3), 1], WEIGHTS: [np.float32(2), 1], CENTERED: np.bool_(True)}, 12)
    assert type(lam) is float and all(type(l) is int for l in layers) and all(type(w) is float for w in weights) and centered is True
    # the centred form without a list: on the one block
    assert key_gram_layers_rule({LAM: 1.0, CENTERED: True}, 12) == (1.0, [11], [1.0], True)
    assert key_gram_layers_rule({LAM: 1.0, LAYER: 5, CENTERED: True}, 12) == (1.0, [5], [1.0], True)
    # a one-entry list with another weight is a list
    assert key_gram_layers_rule({LAM: 1.0, LAYERS: [5], WEIGHTS: [0.5]}, 12) == (1.0, [5], [0.5], False)


def test_a_one_entry_list_of_weight_one_uncentred_is_the_one_block_term():
    for cfg in ({LAM: 2.0, LAYERS: [5]}, {LAM: 2.0, LAYERS: [5], WEIGHTS: [1.0]}, {LAM: 2.0, LAYERS: (5,), WEIGHTS: [1], CENTERED: False}):
        assert key_gram_layers_rule(cfg, 12) is None
        canon = key_gram_canonical(cfg, 12)
        assert canon == {LAYER: 5, LAYERS: None, WEIGHTS: None, CENTERED: False}
        assert key_gram_rule(dict(cfg, **canon), 12) == (2.0, 5) and key_gram_layers_rule(dict(cfg, **canon), 12) is None
    assert key_gram_canonical({LAM: 2.0, LAYERS: [11]}, 12)[LAYER] == 11
    # the list form and the centred one-block form are recorded as the list, the block key null
    assert key_gram_canonical({LAM: 2.0, LAYERS: [7, 2], WEIGHTS: [2, 1]}, 12) == {LAYER: None, LAYERS: [2, 7], WEIGHTS: [1.0, 2.0], CENTERED: False}
    assert key_gram_canonical({LAM: 2.0, LAYER: 5, CENTERED: True}, 12) == {LAYER: None, LAYERS: [5], WEIGHTS: [1.0], CENTERED: True}
    c = {LAM: 2.0, LAYER: 5, CENTERED: True}
    c.update(key_gram_canonical(c, 12))
    assert key_gram_layers_rule(c, 12) == (2.0, [5], [1.0], True) and key_gram_canonical(c, 12) == {k: c[k] for k in (LAYER,) + KEY_GRAM_LAYER_KEYS}   # (a fixed point)
    # the old keys alone keep what the old rule makes of them
    assert key_gram_canonical({}, 12) == {LAYER: None, LAYERS: None, WEIGHTS: None, CENTERED: False}
    assert key_gram_canonical({LAM: 1.0}, 12)[LAYER] == 11 and key_gram_canonical({LAM: 1.0, LAYER: 3}, 12)[LAYER] == 3


@pytest.mark.parametrize("bad", [[], [12], [-1], [1.0], [True], ["5"], [5, 5], 5, "5", list(range(13)), [[5]]])
def test_a_bad_list_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="'dino_gram_layers'"):
        key_gram_layers_rule({LAM: 1.0, LAYERS: bad}, 13 if isinstance(bad, list) and len(bad) == 13 else 12)


@pytest.mark.parametrize("bad", [[1.0], [1.0, 2.0, 3.0], [0.0, 1.0], [-1.0, 1.0], [float("nan"), 1.0], [float("inf"), 1.0], [1e39, 1.0], [1e-60, 1.0], [True, 1.0], ["1", 1.0], 1.0])
def test_bad_weights_are_refused_by_name(bad):
    with pytest.raises(ValueError, match="'dino_gram_layer_weights'"):
        key_gram_layers_rule({LAM: 1.0, LAYERS: [2, 5], WEIGHTS: bad}, 12)


@pytest.mark.parametrize("bad", [1, 0, "true", None, 1.0, [True]])
def test_a_bad_flag_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="'dino_gram_centered'"):
        key_gram_layers_rule({LAM: 1.0, CENTERED: bad}, 12)


def test_the_combinations_that_are_refused():
    with pytest.raises(ValueError, match="'dino_gram_layer_weights' needs 'dino_gram_layers'"):
        key_gram_layers_rule({LAM: 1.0, WEIGHTS: [1.0]}, 12)
    with pytest.raises(ValueError, match="'dino_gram_layers' and 'dino_gram_layer'"):
        key_gram_layers_rule({LAM: 1.0, LAYERS: [2, 5], LAYER: 5}, 12)
    with pytest.raises(ValueError, match="'dino_gram_layers' and 'dino_gram_layer'"):
        key_gram_layers_rule({LAM: 1.0, LAYERS: [5], LAYER: 5}, 12)
    for lam in ({}, {LAM: 0.0}, {LAM: 0}):
        with pytest.raises(ValueError, match="'dino_gram_layers' needs 'lambda_global_key_gram'"):
            key_gram_layers_rule(dict(lam, **{LAYERS: [2, 5]}), 12)
        with pytest.raises(ValueError, match="'dino_gram_layers' needs 'lambda_global_key_gram'"):
            key_gram_layers_rule(dict(lam, **{LAYERS: [2, 5], CENTERED: True}), 12)
        with pytest.raises(ValueError, match="'dino_gram_centered' needs 'lambda_global_key_gram'"):
            key_gram_layers_rule(dict(lam, **{CENTERED: True}), 12)
    with pytest.raises(ValueError, match="'lambda_global_key_gram'"):
        key_gram_layers_rule({LAM: -1.0, LAYERS: [2, 5]}, 12)
    with pytest.raises(ValueError, match="'dino_gram_layer'"):   # (the one block of the centred form is checked as before)
        key_gram_layers_rule({LAM: 1.0, LAYER: 12, CENTERED: True}, 12)
    with pytest.raises(ValueError, match="'dino_gram_layers'"):  # (checked against the depth given)
        key_gram_layers_rule({LAM: 1.0, LAYERS: [2, 6]}, 6)


@pytest.mark.parametrize("key,val", [(LAYERS, [2, 5]), (WEIGHTS, [1.0, 2.0]), (CENTERED, True)])
def test_keys_are_shared_by_the_slots_of_a_sweep(key, val):
    base = {LAM: 1.0, LAYERS: [2, 7], WEIGHTS: [1.0, 1.0]}
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs(base, [{key: val}, {}])
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs({}, [{}, {key: val}])
    assert len(merge_pair_cfgs(dict(base, **{key: val}), [{key: val}, {"lambda_global_identity": 2.0}])) == 2   # (the base value itself is no per-slot value)


def test_snapshot_config_comparison_sees_the_keys():
    a = {LAM: 1.0, LAYERS: [2, 5], WEIGHTS: [0.5, 1.0], CENTERED: False}
    assert snapshot_cfg_mismatch(a, dict(a, **{LAYERS: [2, 7]})) == LAYERS
    assert snapshot_cfg_mismatch(a, dict(a, **{WEIGHTS: [0.5, 2.0]})) == WEIGHTS
    assert snapshot_cfg_mismatch(a, dict(a, **{CENTERED: True})) == CENTERED
    assert snapshot_cfg_mismatch(a, dict(a)) is None
    assert snapshot_cfg_mismatch({LAYERS: None, WEIGHTS: None, CENTERED: False}, {}) is None and snapshot_cfg_mismatch(a, {LAM: 1.0}) == WEIGHTS   # (the first in sorted order)


def _cfg(**kw):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **kw)


def test_engines_refuse_on_the_host_before_anything_touches_a_gpu(monkeypatch):
    """Every constructor raises from the host checks at its head: the library is never asked for (a lib() call would fail the test)."""
    def no_lib():
        raise AssertionError("the library was loaded before the host checks were done")
    monkeypatch.setattr(_lib, "lib", no_lib)
    on = {LAM: 1.0, LAYERS: [2, 5]}
    for bad, key in (({LAM: 1.0, LAYERS: [12]}, LAYERS), ({LAM: 1.0, LAYERS: [2, 2]}, LAYERS), ({LAYERS: [2, 5]}, LAYERS), ({LAM: 0.0, CENTERED: True}, CENTERED),
                     ({LAM: 1.0, LAYERS: [2, 5], WEIGHTS: [1.0]}, WEIGHTS), ({LAM: 1.0, WEIGHTS: [1.0]}, WEIGHTS), ({LAM: 1.0, CENTERED: 1}, CENTERED),
                     ({LAM: 1.0, LAYERS: [2, 5], LAYER: 5}, LAYERS)):
        with pytest.raises(ValueError, match=f"'{key}'"):
            SpliceEngine(_cfg(**bad), None, None, (64, 64), device="cpu")
        with pytest.raises(ValueError, match=f"'{key}'"):
            MultiPairEngine(_cfg(**bad), None, [None, None], (64, 64), device="cpu")
    for fp8 in (True, "gemm", "attention"):
        with pytest.raises(ValueError, match="'lambda_global_key_gram'.*fp8"):
            SpliceEngine(_cfg(**on), None, None, (64, 64), device="cpu", fp8=fp8)
    for key, val in ((LAYERS, [2, 5]), (WEIGHTS, [1.0, 1.0]), (CENTERED, True)):
        with pytest.raises(ValueError, match=f"'{key}' is shared"):
            MultiPairEngine(_cfg(), None, [None, None], (64, 64), device="cpu", pair_cfgs=[{key: val}, {}])
    with pytest.raises(ValueError, match="'lambda_global_key_gram'.*crop counts"):
        MultiPairEngine(_cfg(**on), None, [None, None], (64, 64), device="cpu", n_crops=(2, 1))
    for keys in (on, {LAM: 1.0, CENTERED: True}, {LAM: 1.0, LAYERS: [5]}):
        with pytest.raises(NotImplementedError, match="lambda_global_key_gram"):
            MultiScaleEngine(_cfg(**keys), None, None, (64, 64), scales=(64, 96), device="cpu")
    with pytest.raises(ValueError, match=f"'{LAYERS}'"):   # (a bad value is a bad value there too)
        MultiScaleEngine(_cfg(**{LAM: 1.0, LAYERS: [12]}), None, None, (64, 64), scales=(64, 96), device="cpu")


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
@pytest.mark.parametrize("T", [5, 65])
def test_np_key_gram_layers_against_torch_autograd_in_float64(T, centered):
    """the tolerance tests/test_key_gram_cpu.py holds np_key_gram to: 1e-10 relative on the value, on every gradient element against the
    largest, and norm-wise"""
    D, lam, weights = 64, 1.7, [0.5, 1.0, 3.0]
    rng = np.random.default_rng(200 + T)
    kxs = [rng.standard_normal((T, D)) + rng.standard_normal(D) for _ in weights]           # (a per-feature mean of order 1)
    kbs = [0.8 * rng.standard_normal((T, D)) + 0.8 * kx.mean(0) + 0.3 * rng.standard_normal(D) for kx in kxs]
    raw, addends, dks = np_key_gram_layers(kxs, kbs, lam, weights, centered)
    xs = [torch.from_numpy(k).requires_grad_(True) for k in kxs]

    def moment(k):
        g = k.T @ k / T
        if centered:
            mu = k.mean(0)
            g = g - torch.outer(mu, mu)
        return g
    terms = [w * torch.nn.functional.mse_loss(moment(x), moment(torch.from_numpy(b))) for x, b, w in zip(xs, kbs, weights)]
    want = sum(terms)
    (lam * want).backward()
    assert isinstance(raw, float) and len(addends) == len(dks) == 3
    assert abs(raw - want.item()) <= 1e-10 * abs(want.item())
    for i, x in enumerate(xs):
        g = x.grad.numpy()
        assert dks[i].shape == (T, D) and dks[i].dtype == np.float64
        assert abs(addends[i] - terms[i].item()) <= 1e-10 * abs(terms[i].item())
        assert np.abs(dks[i] - g).max() <= 1e-10 * np.abs(g).max()
        assert np.linalg.norm(dks[i] - g) <= 1e-10 * np.linalg.norm(g)
        if centered:   # every row loses the same vector: the gradient sums to zero over the tokens, to rounding
            assert np.abs(dks[i].sum(0)).max() <= 1e-12 * np.abs(dks[i]).sum(0).max()
    # one uncentred block of weight 1 is np_key_gram; weights None means all 1; equal keys give zero; the two forms differ
    raw1, add1, dk1 = np_key_gram_layers(kxs[:1], kbs[:1], lam)
    ref_raw, ref_dk = np_key_gram(kxs[0], kbs[0], lam)
    assert raw1 == ref_raw == add1[0] and np.array_equal(dk1[0], ref_dk)
    raw0, add0, dk0 = np_key_gram_layers(kxs, kxs, lam, weights, centered)
    assert raw0 == 0.0 and not any(d.any() for d in dk0)
    other = np_key_gram_layers(kxs, kbs, lam, weights, not centered)[0]
    assert abs(other - raw) > 0.1 * max(other, raw)


def test_result_fields_carry_the_keys_where_they_are_not_default():
    from types import SimpleNamespace
    from splice_amd.train import key_gram_fields
    assert key_gram_fields(SimpleNamespace(cfg=dict(DEFAULT_CFG))) == {}
    assert key_gram_fields(SimpleNamespace(key_gram=None, key_gram_layers=None)) == {}
    assert key_gram_fields(SimpleNamespace(key_gram=(2.0, 5), key_gram_layers=None)) == {LAM: 2.0, LAYER: 5}
    assert key_gram_fields(SimpleNamespace(key_gram=(2.0, 11), key_gram_layers=(2.0, [2, 5], [0.5, 1.0], True))) == \
        {LAM: 2.0, LAYERS: [2, 5], WEIGHTS: [0.5, 1.0], CENTERED: True}


class _StubExtractor:
    """``get_keys_from_input(img, layer_num)``: a [heads][T][d] tensor, a differentiable function of the image that differs per block."""
    H, T, d = 2, 5, 4

    def __init__(self):
        self.calls = []

    def get_keys_from_input(self, img, layer_num):
        self.calls.append(layer_num)
        n = self.H * self.T * self.d
        return (layer_num + 1) * (img.mean(dim=(0, 1)).reshape(-1)[:n].reshape(self.H, self.T, self.d) - 0.4)


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_lossg_facade_equals_np_key_gram_layers(centered):
    from splice_amd.losses import LossG
    rng = np.random.default_rng(9)
    off = dict(lambda_global_ssim=0, lambda_global_cls=0, lambda_entire_cls=0, lambda_entire_ssim=0, lambda_global_identity=0)
    cfg = dict(_cfg(**off), cls_warmup=1, **{LAM: 3.0, LAYERS: [7, 2], WEIGHTS: [2.0, 0.5], CENTERED: centered})
    ex = _StubExtractor()
    loss_g = LossG(cfg, extractor=ex)
    assert loss_g.key_gram_layers == (3.0, [2, 7], [0.5, 2.0], centered) and loss_g.key_gram is not None
    x = torch.from_numpy(rng.random((2, 3, 64, 64))).double().requires_grad_(True)
    b = torch.from_numpy(rng.random((3, 3, 64, 64))).double()   # (one crop more on the target side: the zip drops it)
    loss_g.global_transform = lambda img: img
    assert set(loss_g({"x_global": x}, {"step": 0, "B_global": b})) == {"loss"}
    ex.calls.clear()
    out = loss_g({"x_global": x}, {"step": 1, "B_global": b})
    assert set(out) == {"loss", KEY_GRAM_LOSS_KEY} and sorted(set(ex.calls)) == [2, 7] and len(ex.calls) == 8

    def keys(img, l):
        n = ex.H * ex.T * ex.d
        k = (l + 1) * (img.detach().numpy().mean(0).reshape(-1)[:n].reshape(ex.H, ex.T, ex.d) - 0.4)
        return k.transpose(1, 0, 2).reshape(ex.T, ex.H * ex.d)
    want = sum(np_key_gram_layers([keys(x[i], 2), keys(x[i], 7)], [keys(b[i], 2), keys(b[i], 7)], 3.0, [0.5, 2.0], centered)[0] for i in range(2))
    assert abs(out[KEY_GRAM_LOSS_KEY].item() - want) <= 1e-10 * abs(want)
    assert abs(out["loss"].item() - 3.0 * want) <= 1e-10 * abs(3.0 * want)
    out["loss"].backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    # the one-entry spelling is the one-block facade
    one = LossG(dict(cfg, **{LAYERS: [5], WEIGHTS: None, CENTERED: False}), extractor=_StubExtractor())
    assert one.key_gram == (3.0, 5) and one.key_gram_layers is None


def test_binding_and_header_agree_on_the_new_entry_points():
    names = ("splice_step_set_key_gram_layers", "splice_step_key_gram_layer_values", "splice_key_gram_layers_pairs")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splice_hip.h")).read(), flags=re.S)
    for n in names:
        assert n in _lib._SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
        args = re.search(r"\b%s\s*\((.*?)\);" % n, header, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[n][0]), n
    assert len(_lib._SIGNATURES["splice_key_gram_layers_pairs"][0]) == 26 and len(_lib._SIGNATURES["splice_step_set_key_gram_layers"][0]) == 6
    lib = _lib.lib()   # (loads without a GPU: the exports are there)
    for n in names:
        assert hasattr(lib, n), n
