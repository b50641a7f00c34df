"""CPU: the host side of the image-space loss terms -- the NumPy restatement against torch autograd in float64, the
host check of the two config keys, what the engine reports, the LossG facade's arithmetic and the ctypes signatures.  No GPU."""
import numpy as np
import pytest
import torch

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, IMAGE_LOSS_KEYS, LOSS_KEYS, PAIR_KEYS, SNAPSHOT_FREE_KEYS, active_terms, image_terms_rule, merge_pair_cfgs,
                               np_image_terms, snapshot_cfg_mismatch)

KEYS = ("lambda_global_tv", "lambda_global_pixel_identity")


def _torch_tv(x):
    dv, dh = x[:, 1:, :] - x[:, :-1, :], x[:, :, 1:] - x[:, :, :-1]
    return (dv.abs().mean() if dv.numel() else x.sum() * 0) + (dh.abs().mean() if dh.numel() else x.sum() * 0)


@pytest.mark.parametrize("hw", [(2, 2), (3, 5), (1, 4), (4, 1), (24, 40), (67, 131)])
def test_np_image_terms_against_torch_autograd_float64(hw):
    """Value and gradient, bar 1e-12 (float64 on both sides; the sums are at most 3 * 67 * 131 terms long).  Equal neighbours are planted in
    both directions and at the borders: torch.abs has derivative 0 at 0, and so has the restatement."""
    h, w = hw
    rng = np.random.default_rng(h * 1000 + w)
    x = rng.random((3, h, w))
    if h > 1:
        x[0, 1, :] = x[0, 0, :]          # a whole row of vertical ties, touching the top border
        x[2, h - 1, 0] = x[2, h - 2, 0]  # the bottom-left corner
    if w > 1:
        x[1, :, w - 1] = x[1, :, w - 2]  # a whole column of horizontal ties at the right border
        x[2, 0, 1] = x[2, 0, 0]
    y, b = rng.random((3, h, w)), rng.random((3, h, w))
    y[1, 0, 0] = b[1, 0, 0]
    tv, dtv, pix, dpix = np_image_terms(x, y, b)
    xt = torch.from_numpy(x).requires_grad_(True)
    yt = torch.from_numpy(y).requires_grad_(True)
    ref_tv = _torch_tv(xt)
    ref_pix = torch.nn.functional.mse_loss(yt, torch.from_numpy(b))
    (ref_tv + ref_pix).backward()
    assert abs(tv - ref_tv.item()) <= 1e-12 and abs(pix - ref_pix.item()) <= 1e-12
    assert np.abs(dtv - xt.grad.numpy()).max() <= 1e-12
    assert np.abs(dpix - yt.grad.numpy()).max() <= 1e-12
    if h > 1 and w > 2:   # the planted ties did reach a zero derivative somewhere (a check of the test's own inputs)
        assert ((x[0, 1, :] == x[0, 0, :]).all() and (np.sign(x[:, 1:, :] - x[:, :-1, :]) == 0).any())


def test_np_image_terms_float32_inputs_and_absent_sides():
    """fp32 inputs: the sign is that of the fp32 difference; a side that is not given comes back as None."""
    rng = np.random.default_rng(5)
    x = (np.round(16 * rng.random((3, 6, 7))) / 16).astype(np.float32)
    tv, dtv, pix, dpix = np_image_terms(x)
    assert pix is None and dpix is None and dtv.dtype == np.float64 and dtv.shape == x.shape
    xt = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    _torch_tv(xt).backward()
    assert abs(tv - _torch_tv(xt).item()) <= 1e-12 and np.abs(dtv - xt.grad.numpy()).max() <= 1e-12
    assert (np.sign(x[:, :, 1:] - x[:, :, :-1]) == 0).any()   # the 1/16 grid ties
    tv, dtv, pix, dpix = np_image_terms(None, x, x)
    assert tv is None and dtv is None and pix == 0.0 and not dpix.any()
    # a direction without differences contributes 0
    one_row = rng.random((3, 1, 5))
    assert abs(np_image_terms(one_row)[0] - np.abs(np.diff(one_row, axis=2)).mean()) <= 1e-15
    assert np_image_terms(rng.random((3, 1, 1)))[0] == 0.0


@pytest.mark.parametrize("key", KEYS)
def test_image_terms_rule_refusals_name_the_key(key):
    assert image_terms_rule({}) == (0.0, 0.0)
    assert image_terms_rule({key: 0.25})[KEYS.index(key)] == 0.25
    assert image_terms_rule({key: np.float32(2)})[KEYS.index(key)] == 2.0
    for bad in (-0.1, float("nan"), float("inf"), "0.1", True, None, 1e39):
        with pytest.raises(ValueError, match=key):
            image_terms_rule({key: bad})


@pytest.mark.parametrize("key", KEYS)
def test_keys_are_shared_by_the_slots_of_a_sweep(key):
    assert key not in PAIR_KEYS and key not in SNAPSHOT_FREE_KEYS and DEFAULT_CFG[key] == 0.0
    with pytest.raises(ValueError, match=key):
        merge_pair_cfgs({}, [{key: 0.5}, {}])
    assert len(merge_pair_cfgs({key: 0.5}, [{key: 0.5}, {"lr": 0.001}])) == 2   # (the base value itself is no per-slot value)


def test_snapshot_config_comparison_sees_the_keys():
    assert snapshot_cfg_mismatch({"lambda_global_tv": 0.1}, {}) == "lambda_global_tv"
    assert snapshot_cfg_mismatch({"lambda_global_pixel_identity": 1.0}, {"lambda_global_pixel_identity": 0.5}) == "lambda_global_pixel_identity"
    assert snapshot_cfg_mismatch({"lambda_global_tv": 0.0}, {}) is None


def test_active_terms_report_the_names_exactly_when_the_key_is_on():
    assert IMAGE_LOSS_KEYS == ["loss_global_tv", "loss_global_pix_id_B"]
    assert LOSS_KEYS == ["loss", "loss_global_ssim", "loss_entire_ssim", "loss_entire_cls", "loss_global_cls", "loss_global_id_B"]   # (as it was)
    for tv, pix in ((0.0, 0.0), (0.1, 0.0), (0.0, 2.0), (0.1, 2.0)):
        c = dict(DEFAULT_CFG, lambda_global_tv=tv, lambda_global_pixel_identity=pix)
        for step in (0, 1, 75):   # before cls_warmup, ordinary, entire-image: no schedule gates the two
            act = active_terms(c, step, True)
            assert act["loss_global_tv"] == (tv > 0) and act["loss_global_pix_id_B"] == (pix > 0)
            assert set(act) == set(LOSS_KEYS + IMAGE_LOSS_KEYS)
    assert active_terms({k: v for k, v in DEFAULT_CFG.items() if k not in KEYS}, 3, False)["loss_global_tv"] is False   # (a config from before the keys)


def test_result_fields_carry_the_keys_where_they_are_not_zero():
    from types import SimpleNamespace
    from splice_amd.train import image_terms_fields
    assert image_terms_fields(SimpleNamespace(cfg=dict(DEFAULT_CFG))) == {}
    assert image_terms_fields(SimpleNamespace(cfg=dict(DEFAULT_CFG, lambda_global_tv=0.1))) == {"lambda_global_tv": 0.1}
    assert image_terms_fields(SimpleNamespace(cfg=dict(DEFAULT_CFG, lambda_global_tv=0.1, lambda_global_pixel_identity=2))) == {
        "lambda_global_tv": 0.1, "lambda_global_pixel_identity": 2}


def test_lossg_facade_adds_the_two_terms_with_torch_ops():
    """The facade on CPU tensors, the five DINO weights at 0 (no extractor call): the two keys add sum-over-crops TV / mse with their weights, and
    autograd gives the gradients of np_image_terms."""
    from splice_amd.losses import LossG
    rng = np.random.default_rng(11)
    cfg = dict(DEFAULT_CFG, lambda_global_cls=0, lambda_global_ssim=0, lambda_global_identity=0, lambda_entire_cls=0, lambda_entire_ssim=0,
               lambda_global_tv=0.3, lambda_global_pixel_identity=1.7)
    loss_g = LossG(cfg, extractor=object())
    x = torch.from_numpy(rng.random((2, 3, 5, 7))).requires_grad_(True)
    y = torch.from_numpy(rng.random((2, 3, 4, 6))).requires_grad_(True)
    b = torch.from_numpy(rng.random((2, 3, 4, 6)))
    out = loss_g({"x_global": x, "y_global": y}, {"step": 0, "B_global": b})
    refs = [np_image_terms(x[i].detach().numpy(), y[i].detach().numpy(), b[i].numpy()) for i in range(2)]
    assert set(out) == {"loss", "loss_global_tv", "loss_global_pix_id_B"}
    assert abs(out["loss_global_tv"].item() - (refs[0][0] + refs[1][0])) <= 1e-12
    assert abs(out["loss_global_pix_id_B"].item() - (refs[0][2] + refs[1][2])) <= 1e-12
    assert abs(out["loss"].item() - (0.3 * (refs[0][0] + refs[1][0]) + 1.7 * (refs[0][2] + refs[1][2]))) <= 1e-12
    out["loss"].backward()
    for i in range(2):
        assert np.abs(x.grad[i].numpy() - 0.3 * refs[i][1]).max() <= 1e-12
        assert np.abs(y.grad[i].numpy() - 1.7 * refs[i][3]).max() <= 1e-12
    # both keys 0 (or absent): the dict is what it was
    off = LossG({k: v for k, v in cfg.items() if k not in KEYS}, extractor=object())({"x_global": x, "y_global": y}, {"step": 0, "B_global": b})
    assert set(off) == {"loss"} and off["loss"] == 0


def test_binding_and_header_agree_on_the_new_entry_points():
    import os
    import re
    names = ("splice_step_set_image_terms", "splice_image_terms_value", "splice_image_terms_grad_add", "splice_total_loss_pairs_img")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "splice_hip.h")).read(), flags=re.S)
    for n in names:
        assert n in _lib._SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
        args = re.search(r"\b%s\s*\((.*?)\);" % n, header, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[n][0]), n
    assert len(_lib._SIGNATURES["splice_total_loss_pairs_img"][0]) == len(_lib._SIGNATURES["splice_total_loss_pairs"][0]) + 2
    assert len(_lib._SIGNATURES["splice_total_loss_pairs"][0]) == 18   # (as it was)
