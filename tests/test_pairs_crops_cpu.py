"""CPU: the host side of several pairs per step with several global crops per image -- the pair batch feed with n crops per
pair, the refusals that come before the GPU, and the new C export."""
import os
import re

import numpy as np
import pytest
import torch

from splice_amd import _lib


def _feed(n_a, n_b, P=3, min_cover=0.6):
    from splice_amd.train import PairBatchFeed
    cfg = dict(use_augmentations=False, entire_A_every=75, global_A_crops_min_cover=min_cover, global_B_crops_min_cover=min_cover,
               global_A_crops_n_crops=n_a, global_B_crops_n_crops=n_b)
    g = torch.Generator().manual_seed(5)
    As = [torch.rand(3, 40, 52, generator=g) for _ in range(P)]
    Bs = [torch.rand(3, 44, 36, generator=g) for _ in range(P)]
    return PairBatchFeed(cfg, As, Bs, device=torch.device("cpu")), As, Bs


def _find(img, crop):
    """(top, left) of `crop` inside `img`, or None"""
    s = crop.shape[-1]
    for t in range(img.shape[1] - s + 1):
        for l in range(img.shape[2] - s + 1):
            if torch.equal(img[:, t:t + s, l:l + s], crop):
                return t, l
    return None


@pytest.mark.parametrize("n_a,n_b", [(2, 2), (3, 1), (1, 4)])
def test_pair_batch_feed_n_crops_layout(n_a, n_b):
    np.random.seed(0)
    torch.manual_seed(0)
    P = 3
    feed, As, Bs = _feed(n_a, n_b, P)
    for _ in range(3):
        s = feed.next()
        a, b = s["A_global"], s["B_global"]
        assert a.shape[0] == P * n_a and b.shape[0] == P * n_b
        assert a.shape[-1] == a.shape[-2] and b.shape[-1] == b.shape[-2]    # one size per side per step, square
        for imgs, crops, n in ((As, a, n_a), (Bs, b, n_b)):
            for k in range(crops.shape[0]):
                assert _find(imgs[k // n], crops[k]) is not None, k       # pair-major: crop k comes from pair k // n, inside the image


def test_pair_batch_feed_one_crop_is_unchanged():
    """n = 1 per side: the draws and the crops of the feed before n_crops existed (one size per side, one position per pair)."""
    from splice_amd import augment
    np.random.seed(1)
    torch.manual_seed(1)
    feed, As, Bs = _feed(1, 1)
    got = feed.next()
    np.random.seed(1)
    torch.manual_seed(1)
    for key, imgs in (("A_global", As), ("B_global", Bs)):
        _, h, w = imgs[0].shape
        size, boxes = augment.global_crop_boxes(h, w, 0.6, len(imgs))
        want = torch.stack([im[:, t:t + size, l:l + size] for im, (t, l) in zip(imgs, boxes)])
        assert torch.equal(got[key], want)


def _pairs(tmp_path, k):
    roots = []
    for i in range(k):
        for side in ("A", "B"):
            (tmp_path / f"p{i}" / side).mkdir(parents=True)
        roots.append(str(tmp_path / f"p{i}"))
    return roots


def test_train_pairs_refusals_before_the_gpu(tmp_path):
    from splice_amd.train import train_pairs
    roots = _pairs(tmp_path, 17)
    with pytest.raises(NotImplementedError, match="images per side"):
        train_pairs(roots, cfg_overrides=dict(global_A_crops_n_crops=2))
    with pytest.raises(NotImplementedError, match="1..8 global crops"):
        train_pairs(roots[:2], cfg_overrides=dict(global_B_crops_n_crops=9))
    with pytest.raises(NotImplementedError, match="dino_global_scales"):
        train_pairs(roots[:2], cfg_overrides=dict(global_A_crops_n_crops=2, dino_global_scales=[224, 320]))


def test_multipair_engine_refusals_before_the_gpu():
    from splice_amd.engine import MultiPairEngine
    with pytest.raises(ValueError, match="images per side"):
        MultiPairEngine({}, None, [{}] * 9, (64, 64), (64, 64), device="cpu", n_crops=4)
    with pytest.raises(ValueError, match="n_crops"):
        MultiPairEngine({}, None, [{}] * 2, (64, 64), (64, 64), device="cpu", n_crops=(9, 1))


def test_set_groups_export_bound_and_present():
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "splice_hip.h")).read()
    assert re.search(r"int splice_gen_plan_set_groups\(void\* plan, int images_per_group\);", hdr)
    assert "#define SPLICE_STEP_MAX_GROUP_IMAGES 32" in hdr
    assert "splice_gen_plan_set_groups" in _lib.exported_symbols()
    assert hasattr(_lib.lib(), "splice_gen_plan_set_groups")
