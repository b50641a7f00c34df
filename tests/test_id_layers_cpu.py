"""CPU: the host side of the key-identity loss over several ViT blocks (``dino_id_layers`` / ``dino_id_layer_weights``; DESIGN.md
section 9m): defaults, every refusal by name before a GPU is touched, the canonical order, the facade and the bindings."""
import os
import re

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, ID_LAYER_KEYS, MAX_ID_LAYERS, PAIR_KEYS, SNAPSHOT_FREE_KEYS, MultiPairEngine, MultiScaleEngine, SpliceEngine,
                               id_layers_rule, merge_pair_cfgs, np_id_layers, snapshot_cfg_mismatch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS, WEIGHTS = ID_LAYER_KEYS


def test_the_keys_are_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    assert ID_LAYER_KEYS == ("dino_id_layers", "dino_id_layer_weights")
    for cfg in (DEFAULT_CFG, packaged):
        assert cfg[LAYERS] is None and cfg[WEIGHTS] is None
        assert id_layers_rule(cfg, 12) is None
    assert id_layers_rule({}, 12) is None
    # the default spelled out is the default: the setter is not called for it either
    assert id_layers_rule({LAYERS: [11]}, 12) is None
    assert id_layers_rule({LAYERS: [11], WEIGHTS: [1]}, 12) is None
    assert id_layers_rule({LAYERS: (11,), WEIGHTS: [np.float32(1)]}, 12) is None
    assert id_layers_rule({LAYERS: [11], WEIGHTS: [2.0]}, 12) == ([11], [2.0])   # (another weight is another function)
    assert id_layers_rule({LAYERS: [5]}, 6) is None and id_layers_rule({LAYERS: [5]}, 12) == ([5], [1.0])   # (the top block of that ViT)
    assert not set(PAIR_KEYS) & set(ID_LAYER_KEYS) and not set(SNAPSHOT_FREE_KEYS) & set(ID_LAYER_KEYS)
    # the structure and appearance keys are their own pairs: one does not set the other
    assert id_layers_rule({"dino_ssim_layers": [2, 7], "dino_cls_layers": [3]}, 12) is None


def test_canonical_order_is_ascending_with_each_weight_beside_its_block():
    assert id_layers_rule({LAYERS: [7, 11, 2]}, 12) == ([2, 7, 11], [1.0, 1.0, 1.0])
    assert id_layers_rule({LAYERS: [7, 11, 2], WEIGHTS: [0.5, 2, 0.25]}, 12) == ([2, 7, 11], [0.25, 0.5, 2.0])
    assert id_layers_rule({LAYERS: (np.int64(3), 0), WEIGHTS: (np.float32(0.5), 3)}, 12) == ([0, 3], [3.0, 0.5])
    assert id_layers_rule({LAYERS: list(range(12))}, 12) == (list(range(12)), [1.0] * 12)
    assert id_layers_rule({LAYERS: [0, 5]}, 12) == ([0, 5], [1.0, 1.0])   # (the top block need not be listed)
    layers, weights = id_layers_rule({LAYERS: [11, 0]}, 12)
    assert all(type(l) is int for l in layers) and all(type(w) is float for w in weights)


@pytest.mark.parametrize("bad", [[], [3, 3], [2, 7, 2], [-1], [12], [0, 12], [1.0], [True], ["3"], 3, "3", "[3]", list(range(13)), [None]])
def test_bad_layers_are_refused_by_name(bad):
    with pytest.raises(ValueError, match="'dino_id_layers'"):
        id_layers_rule({LAYERS: bad}, 12)


def test_layers_are_checked_against_the_depth_given():
    assert id_layers_rule({LAYERS: [5, 3]}, 6) == ([3, 5], [1.0, 1.0])
    with pytest.raises(ValueError, match="'dino_id_layers'"):
        id_layers_rule({LAYERS: [6]}, 6)
    with pytest.raises(ValueError, match="'dino_id_layers'"):
        id_layers_rule({LAYERS: [0, 1, 2, 3]}, 3)   # (more entries than blocks)
    with pytest.raises(ValueError, match="'dino_id_layers'"):
        id_layers_rule({LAYERS: list(range(13))}, 24)   # (more than the kernel's table holds, whatever the depth)
    assert MAX_ID_LAYERS == 12


@pytest.mark.parametrize("bad", [[1.0], [1.0, 1.0, 1.0], [], [1.0, 0.0], [1.0, -2.0], [float("nan"), 1.0], [1.0, float("inf")], [1.0, 1e39], [1e-60, 1.0],
                                 [True, 1.0], ["1", 1.0], [None, 1.0], 1.0, "1,1"])
def test_bad_weights_are_refused_by_name(bad):
    with pytest.raises(ValueError, match="'dino_id_layer_weights'"):
        id_layers_rule({LAYERS: [2, 11], WEIGHTS: bad}, 12)


def test_weights_without_layers_are_refused():
    with pytest.raises(ValueError, match="'dino_id_layer_weights' needs 'dino_id_layers'"):
        id_layers_rule({WEIGHTS: [1.0]}, 12)
    with pytest.raises(ValueError, match="'dino_id_layer_weights'"):
        id_layers_rule({LAYERS: None, WEIGHTS: [2.0, 1.0]}, 12)


@pytest.mark.parametrize("key,val", [(LAYERS, [2, 11]), (WEIGHTS, [0.5, 1.0])])
def test_keys_are_shared_by_the_slots_of_a_sweep(key, val):
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs({LAYERS: [3, 11], WEIGHTS: [1.0, 1.0]}, [{key: val}, {}])
    with pytest.raises(ValueError, match=f"'{key}' is shared"):
        merge_pair_cfgs({}, [{}, {key: val}])
    base = {LAYERS: [2, 11], WEIGHTS: [0.5, 1.0]}
    assert len(merge_pair_cfgs(base, [{key: val}, {"lambda_global_identity": 2.0}])) == 2   # (the base value itself is no per-slot value)


def test_snapshot_config_comparison_sees_the_keys():
    assert snapshot_cfg_mismatch({LAYERS: [2, 7, 11]}, {}) == LAYERS
    assert snapshot_cfg_mismatch({LAYERS: [2, 7, 11], WEIGHTS: [1.0, 1.0, 1.0]}, {LAYERS: [2, 7, 11], WEIGHTS: [1.0, 2.0, 1.0]}) == WEIGHTS
    assert snapshot_cfg_mismatch({LAYERS: [2, 7, 11]}, {LAYERS: [2, 7, 11]}) is None and snapshot_cfg_mismatch({LAYERS: None}, {}) is None


def _cfg(**kw):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **kw)


def test_engines_refuse_on_the_host_before_anything_touches_a_gpu(monkeypatch):
    """Every constructor raises from the host checks at its head: the library is never asked for (a lib() call would fail the test)."""
    def no_lib():
        raise AssertionError("the library was loaded before the host checks were done")
    monkeypatch.setattr(_lib, "lib", no_lib)
    for bad, key in (({LAYERS: [3, 3]}, LAYERS), ({LAYERS: [12]}, LAYERS), ({LAYERS: list(range(13))}, LAYERS), ({LAYERS: [2, 11], WEIGHTS: [1.0]}, WEIGHTS),
                     ({LAYERS: [2, 11], WEIGHTS: [1.0, 0.0]}, WEIGHTS), ({LAYERS: [2, 11], WEIGHTS: [1.0, float("nan")]}, WEIGHTS),
                     ({LAYERS: [2, 11], WEIGHTS: [1.0, 1e39]}, WEIGHTS), ({WEIGHTS: [1.0]}, WEIGHTS)):
        with pytest.raises(ValueError, match=f"'{key}'"):
            SpliceEngine(_cfg(**bad), None, None, (64, 64), device="cpu")
        with pytest.raises(ValueError, match=f"'{key}'"):
            MultiPairEngine(_cfg(**bad), None, [None, None], (64, 64), device="cpu")
    # fp8 in any spelling, with a layer set that is not the default
    for fp8 in (True, "gemm", "attention"):
        with pytest.raises(ValueError, match="'dino_id_layers'.*fp8"):
            SpliceEngine(_cfg(**{LAYERS: [2, 11]}), None, None, (64, 64), device="cpu", fp8=fp8)
    # a per-slot value
    with pytest.raises(ValueError, match=f"'{LAYERS}' is shared"):
        MultiPairEngine(_cfg(), None, [None, None], (64, 64), device="cpu", pair_cfgs=[{LAYERS: [2, 11]}, {}])
    # the several-scales engine
    with pytest.raises(NotImplementedError, match="dino_id_layers"):
        MultiScaleEngine(_cfg(**{LAYERS: [2, 11]}), None, None, (64, 64), scales=(64, 96), device="cpu")
    with pytest.raises(ValueError, match=f"'{LAYERS}'"):   # (a bad value is a bad value there too)
        MultiScaleEngine(_cfg(**{LAYERS: [2, 2]}), None, None, (64, 64), scales=(64, 96), device="cpu")


def test_np_id_layers_is_the_float32_sum_in_order():
    f = np.float32
    v = [f(0.1), f(0.7), f(1e-8), f(3.3)]
    assert np_id_layers(v) == f(f(f(f(f(0) + v[0]) + v[1]) + v[2]) + v[3])
    w = [0.5, 2.0, 1.0, 0.3]
    assert np_id_layers(v, w) == f(f(f(f(f(0) + f(f(w[0]) * v[0])) + f(f(w[1]) * v[1])) + f(f(w[2]) * v[2])) + f(f(w[3]) * v[3]))
    assert np_id_layers(v).dtype == np.float32 and np_id_layers([]) == 0


def test_result_fields_carry_the_keys_where_they_are_not_default():
    from types import SimpleNamespace
    from splice_amd.train import id_layers_fields
    assert id_layers_fields(SimpleNamespace(cfg=dict(DEFAULT_CFG))) == {}
    assert id_layers_fields(SimpleNamespace(id_layers=None)) == {}
    assert id_layers_fields(SimpleNamespace(id_layers=([2, 7, 11], [0.25, 0.5, 2.0]))) == {LAYERS: [2, 7, 11], WEIGHTS: [0.25, 0.5, 2.0]}


class _StubExtractor:
    """``get_keys_from_input(img, layer_num)``: a [heads][T][d] tensor, a differentiable function of the image that differs per block."""

    def __init__(self):
        self.calls = []

    def get_keys_from_input(self, img, layer_num):
        self.calls.append(layer_num)
        return (layer_num + 1) * img.mean(dim=(0, 1)).reshape(-1)[:48].reshape(2, 3, 8) ** 2


def test_lossg_facade_sums_the_layers_with_their_weights():
    from splice_amd.losses import LossG
    rng = np.random.default_rng(5)
    off = dict(lambda_global_ssim=0, lambda_global_cls=0, lambda_entire_cls=0, lambda_entire_ssim=0)
    cfg = dict(_cfg(**off), lambda_global_identity=2.0, cls_warmup=0, **{LAYERS: [7, 2], WEIGHTS: [0.5, 3.0]})
    ex = _StubExtractor()
    loss_g = LossG(cfg, extractor=ex)
    assert loss_g.id_layers == ([2, 7], [3.0, 0.5])
    y = torch.from_numpy(rng.random((2, 3, 64, 64))).float().requires_grad_(True)
    b = torch.from_numpy(rng.random((2, 3, 64, 64))).float()
    loss_g.global_transform = lambda img: img   # (the HIP Resize is not what this test is about)
    out = loss_g({"y_global": y}, {"step": 0, "B_global": b})

    def keys(img, l):   # block l's stub keys
        return (l + 1) * img.mean(0).reshape(-1)[:48] ** 2
    want = 0.0
    for i in range(2):   # per crop, the blocks ascending; then the crops in order
        crop = 0.0
        for l, w in ((2, 3.0), (7, 0.5)):
            crop = crop + w * torch.nn.functional.mse_loss(keys(y[i], l), keys(b[i], l))
        want = want + crop
    assert set(out) == {"loss", "loss_global_id_B"} and ex.calls == [2, 2, 7, 7] * 2
    assert abs(out["loss_global_id_B"].item() - want.item()) <= 1e-6 * abs(want.item())
    assert abs(out["loss"].item() - 2.0 * want.item()) <= 2e-6 * abs(want.item())
    assert abs(loss_g.calculate_global_id_loss(y.detach(), b).item() - want.item()) <= 1e-6 * abs(want.item())
    out["loss"].backward()
    assert y.grad is not None and float(y.grad.abs().max()) > 0
    # absent keys: the reference's layer
    ex2 = _StubExtractor()
    plain = LossG({k: v for k, v in cfg.items() if k not in ID_LAYER_KEYS}, extractor=ex2)
    plain.global_transform = lambda img: img
    assert plain.id_layers is None
    got = plain({"y_global": y.detach()}, {"step": 0, "B_global": b})
    top = sum(torch.nn.functional.mse_loss(keys(y[i].detach(), 11), keys(b[i], 11)) for i in range(2))
    assert abs(got["loss_global_id_B"].item() - top.item()) <= 1e-6 * abs(top.item()) and set(ex2.calls) == {11}


def test_binding_and_header_agree_on_the_new_entry_points():
    names = ("splice_step_set_id_layers", "splice_step_id_layer_values", "splice_id_loss_layers", "splice_vit_ctx_set_key_f32_layers")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splice_hip.h")).read(), flags=re.S)
    for n in names:
        assert n in _lib._SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
        args = re.search(r"\b%s\s*\((.*?)\);" % n, header, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[n][0]), n
    assert len(_lib._SIGNATURES["splice_id_loss_layers"][0]) == 23 and len(_lib._SIGNATURES["splice_vit_get_tensor"][0]) == 4   # (the getter keeps its signature)
    lib = _lib.lib()   # (loads without a GPU: the exports are there)
    for n in names:
        assert hasattr(lib, n), n
