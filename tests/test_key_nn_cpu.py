"""CPU: the host side of the nearest-neighbour key appearance term (``lambda_global_key_nn`` / ``dino_nn_layer``):
defaults, every refusal by name before a GPU is touched, the float64 restatement against torch autograd, the facade, the bindings, and
the properties of the seeded inputs the GPU tests rely on (``planted_keys`` / ``iid_keys`` live here and are imported there)."""
import functools
import os
import re

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import (DEFAULT_CFG, KEY_NN_KEYS, KEY_NN_LOSS_KEY, LOSS_KEYS, PAIR_KEYS, SNAPSHOT_FREE_KEYS, MultiPairEngine, MultiScaleEngine,
                               SpliceEngine, active_terms, key_nn_active, key_nn_rule, merge_pair_cfgs, np_key_nn, snapshot_cfg_mismatch)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM, LAYER = KEY_NN_KEYS
U24 = 2.0 ** -24           # unit roundoff of float32
U23 = 2.0 ** -23           # per-term unit of an fp32 MFMA accumulation whose internal order and rounding are not specified
EPS = float(np.float32(1e-8))   # the eps of the term as the kernels take it: a float32
OP_SHAPES = [(5, 64), (65, 128), (197, 192), (130, 768)]
IID_SHAPE = (197, 192)
IID_SEED = 3               # chosen on the CPU: test_iid_inputs_keep_the_exemptions_under_the_cap holds it to the cap


# ------------------------------------------------------------------------------------------------ the seeded inputs of the op tests
@functools.lru_cache(maxsize=None)
def planted_keys(T, D, pairs):
    """``(kx, kb, pi)``: bf16 tensors [pairs][T][D] and an int64 array [pairs][T].  The target is ``bf16(randn)``; for a seeded many-to-one
    map ``pi`` into the first third of the tokens, ``kx_i = bf16(0.8 s_i kb_pi(i) + 0.35 randn)`` with ``s_i`` in [0.5, 2.5].  Never modified."""
    g = torch.Generator().manual_seed(9100 + 10 * T + D + pairs)
    kb = torch.randn(pairs, T, D, generator=g).to(torch.bfloat16)
    third = max(1, T // 3)
    pi = torch.randint(0, third, (pairs, T), generator=g)
    s = 0.5 + 2.0 * torch.rand(pairs, T, 1, generator=g)
    src = torch.gather(kb.float(), 1, pi[:, :, None].expand(pairs, T, D))
    kx = (0.8 * s * src + 0.35 * torch.randn(pairs, T, D, generator=g)).to(torch.bfloat16)
    return kx, kb, pi.numpy()


@functools.lru_cache(maxsize=None)
def iid_keys(pairs, seed=IID_SEED):
    """independent ``bf16(randn)`` keys at IID_SHAPE, [pairs][T][D] each; never modified"""
    T, D = IID_SHAPE
    g = torch.Generator().manual_seed(9500 + seed)
    return torch.randn(pairs, T, D, generator=g).to(torch.bfloat16), torch.randn(pairs, T, D, generator=g).to(torch.bfloat16)


def cosine_reference(kx, kb):
    """float64 on one pair's bf16 values: ``(c, E)``, the ``[T][T]`` cosines and the bound of every entry the kernels compute, derived from
    the arithmetic include/splice_hip.h states for splice_key_nn_pairs:
      a_ij: an fp32 MFMA accumulation of D exact bf16 x bf16 products: |error| <= D 2^-23 (|k_i| . |b_j|)
      n_i:  squares added by at most D / 64 fused multiply-adds per lane and 6 tree levels, all non-negative: relative (D / 64 + 6) 2^-24 on
            the sum, half of it behind the square root, whose own rounding adds 2^-24: eps_n = ((D / 64 + 6) / 2 + 1) 2^-24
      fl(n_i m_j): 2 eps_n + 2^-24;  the division: 2^-24
          E_ij = D 2^-23 (|k_i| . |b_j|) / (n_i m_j) + |c_ij| (2 eps_n + 2 2^-24)
    times SLACK = 1 + 1e-5 for the products of these first-order terms.  (Rows whose n_i m_j is <= eps are not in these inputs but for the
    all-zero row, whose cosines are exactly 0.)"""
    x, b = kx.double().numpy(), kb.double().numpy()
    D = x.shape[1]
    nx, nb = np.sqrt((x * x).sum(1)), np.sqrt((b * b).sum(1))
    den = np.maximum(np.outer(nx, nb), EPS)
    c = (x @ b.T) / den
    eps_n = ((D / 64 + 6) / 2 + 1) * U24
    E = (D * U23 * (np.abs(x) @ np.abs(b).T) / den + np.abs(c) * (2 * eps_n + 2 * U24)) * (1 + 1e-5)
    return c, E


def top_two_gap(c):
    s = np.sort(c, axis=1)
    return s[:, -1] - s[:, -2] if c.shape[1] > 1 else np.full(c.shape[0], np.inf)


@pytest.mark.parametrize("T,D", OP_SHAPES)
def test_planted_inputs_have_one_clear_nearest_neighbour(T, D):
    """what the GPU test's `match == pi on every row` stands on: the float64 reference recovers pi on every row, and the smallest gap between
    the best and the second-best cosine is at least a thousand times the derived bound of a cosine's error"""
    for pairs in (1, 3):
        kx, kb, pi = planted_keys(T, D, pairs)
        for p in range(pairs):
            c, E = cosine_reference(kx[p], kb[p])
            assert (np.argmax(c, axis=1) == pi[p]).all()
            gap = top_two_gap(c).min()
            print(f"KEY_NN planted T={T} D={D} pairs={pairs} pair {p}: smallest top-two gap {gap:.3f}, largest cosine bound {E.max():.2e}, distinct targets {len(set(pi[p]))}")
            assert E.max() < 1e-4 and gap >= 1000 * E.max()
            assert T < 9 or len(set(pi[p])) < T // 2   # (many-to-one)
            _, m, cos, _ = np_key_nn(kx[p].double().numpy(), kb[p].double().numpy(), 1.0)
            assert (m == pi[p]).all() and np.abs(cos - c[np.arange(T), pi[p]]).max() < 1e-12


def iid_exempt_rows(kx, kb):
    """rows of one iid pair whose reference top-two gap is below twice the row's largest derived cosine bound"""
    c, E = cosine_reference(kx, kb)
    return np.nonzero(top_two_gap(c) < 2 * E.max(axis=1))[0], c, E


def test_iid_inputs_keep_the_exemptions_under_the_cap():
    T, D = IID_SHAPE
    for pairs in (1, 3):
        kx, kb = iid_keys(pairs)
        for p in range(pairs):
            rows, c, E = iid_exempt_rows(kx[p], kb[p])
            print(f"KEY_NN iid T={T} D={D} pairs={pairs} pair {p}: smallest top-two gap {top_two_gap(c).min():.2e}, largest cosine bound {E.max():.2e}, exempt rows {list(rows)}")
            assert len(rows) <= T // 100


# ------------------------------------------------------------------------------------------------ the rule
def test_the_keys_are_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    assert KEY_NN_KEYS == ("lambda_global_key_nn", "dino_nn_layer") and KEY_NN_LOSS_KEY == "loss_global_key_nn"
    for cfg in (DEFAULT_CFG, packaged):
        assert cfg[LAM] == 0.0 and cfg[LAYER] is None
        assert key_nn_rule(cfg, 12) is None
    assert key_nn_rule({}, 12) is None and key_nn_rule({LAM: 0}, 12) is None and key_nn_rule({LAM: 0.0, LAYER: None}, 12) is None
    assert not set(PAIR_KEYS) & set(KEY_NN_KEYS) and not set(SNAPSHOT_FREE_KEYS) & set(KEY_NN_KEYS)
    assert KEY_NN_LOSS_KEY not in LOSS_KEYS   # (the [P][8] losses row keeps its words)


def test_the_rule_gives_the_weight_and_the_block():
    assert key_nn_rule({LAM: 2.5}, 12) == (2.5, 11)           # null = the top block of that ViT
    assert key_nn_rule({LAM: 2.5}, 6) == (2.5, 5)
    assert key_nn_rule({LAM: 1, LAYER: 5}, 12) == (1.0, 5)
    assert key_nn_rule({LAM: np.float32(0.5), LAYER: np.int64(0)}, 12) == (0.5, 0)
    lam, layer = key_nn_rule({LAM: 3, LAYER: 11}, 12)
    assert type(lam) is float and type(layer) is int


@pytest.mark.parametrize("bad", [-1.0, -1e-30, float("nan"), float("inf"), 1e39, 1e-60, True, "1", None, [1.0]])
def test_a_bad_weight_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="'lambda_global_key_nn'"):
        key_nn_rule({LAM: bad}, 12)


@pytest.mark.parametrize("bad", [-1, 12, 1.0, True, "5", [5], (5,)])
def test_a_bad_layer_is_refused_by_name(bad):
    with pytest.raises(ValueError, match="'dino_nn_layer'"):
        key_nn_rule({LAM: 1.0, LAYER: bad}, 12)


def test_the_layer_is_checked_against_the_depth_given_and_needs_the_weight():
    assert key_nn_rule({LAM: 1.0, LAYER: 5}, 6) == (1.0, 5)
    with pytest.raises(ValueError, match="'dino_nn_layer'"):
        key_nn_rule({LAM: 1.0, LAYER: 6}, 6)
    with pytest.raises(ValueError, match="'dino_nn_layer' needs 'lambda_global_key_nn'"):
        key_nn_rule({LAYER: 5}, 12)
    with pytest.raises(ValueError, match="'dino_nn_layer' needs 'lambda_global_key_nn'"):
        key_nn_rule({LAM: 0.0, LAYER: 11}, 12)


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
    assert [key_nn_active(c, s) for s in (0, 2, 3, 4, 75)] == [False, False, True, True, True]   # (entire-image steps included)
    assert not key_nn_active(dict(DEFAULT_CFG, cls_warmup=0), 5)
    assert KEY_NN_LOSS_KEY not in active_terms(c, 5, True)   # (that dict keeps its keys)


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
        with pytest.raises(ValueError, match="'lambda_global_key_nn'.*fp8"):
            SpliceEngine(_cfg(**{LAM: 1.0}), None, None, (64, 64), device="cpu", fp8=fp8)
    for key, val in ((LAM, 1.0), (LAYER, 5)):   # a per-slot value
        with pytest.raises(ValueError, match=f"'{key}' is shared"):
            MultiPairEngine(_cfg(), None, [None, None], (64, 64), device="cpu", pair_cfgs=[{key: val}, {}])
    with pytest.raises(ValueError, match="'lambda_global_key_nn'.*crop counts"):   # several pairs with different crop counts per side
        MultiPairEngine(_cfg(**{LAM: 1.0}), None, [None, None], (64, 64), device="cpu", n_crops=(2, 1))
    with pytest.raises(NotImplementedError, match="lambda_global_key_nn"):   # the several-scales engine
        MultiScaleEngine(_cfg(**{LAM: 1.0, LAYER: 5}), None, None, (64, 64), scales=(64, 96), device="cpu")
    with pytest.raises(ValueError, match=f"'{LAYER}'"):   # (a bad value is a bad value there too)
        MultiScaleEngine(_cfg(**{LAM: 1.0, LAYER: 12}), None, None, (64, 64), scales=(64, 96), device="cpu")


# ------------------------------------------------------------------------------------------------ the restatement
def _torch_nn(kx, kb, lam, eps=EPS):
    x = torch.from_numpy(kx).requires_grad_(True)
    b = torch.from_numpy(kb)
    cos = (x @ b.T) / torch.clamp(x.norm(dim=1)[:, None] * b.norm(dim=1)[None, :], min=eps)
    best = cos.max(dim=1)
    raw = (1.0 - best.values).mean()
    (lam * raw).backward()
    return raw.item(), best.indices.numpy(), best.values.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("T", [5, 65])
def test_np_key_nn_against_torch_autograd_in_float64(T):
    """1 - cos through clamp and max, to 1e-10: the bar np_optim_step is held to against torch"""
    D, lam = 64, 1.7
    rng = np.random.default_rng(300 + T)
    kb = rng.standard_normal((T, D)) * 0.8 + 0.1
    kx = kb[rng.integers(0, T, T)] * rng.uniform(0.5, 2.0, (T, 1)) + 0.5 * rng.standard_normal((T, D))
    raw, m, cos, dk = np_key_nn(kx, kb, lam)
    want, wm, wcos, g = _torch_nn(kx, kb, lam)
    assert dk.shape == (T, D) and dk.dtype == np.float64 and isinstance(raw, float) and m.dtype == np.int64
    assert (m == wm).all() and np.abs(cos - wcos).max() <= 1e-10
    assert abs(raw - want) <= 1e-10 * abs(want)
    assert np.abs(dk - g).max() <= 1e-10 * np.abs(g).max()
    assert np.linalg.norm(dk - g) <= 1e-10 * np.linalg.norm(g)
    # a given assignment is used instead of the arg-max: the cosines and the gradient at those indices
    other = (m + 1) % T
    raw2, m2, cos2, dk2 = np_key_nn(kx, kb, lam, match=other)
    x = torch.from_numpy(kx).requires_grad_(True)
    b = torch.from_numpy(kb)[torch.from_numpy(other)]
    c2 = (x * b).sum(1) / torch.clamp(x.norm(dim=1) * b.norm(dim=1), min=EPS)
    (lam * (1.0 - c2).mean()).backward()
    assert (m2 == other).all() and abs(raw2 - (1.0 - c2).mean().item()) <= 1e-10 and np.abs(dk2 - x.grad.numpy()).max() <= 1e-10 * np.abs(dk2).max()
    assert raw2 > raw


def test_np_key_nn_ties_zero_rows_and_equal_keys():
    rng = np.random.default_rng(5)
    T, D, lam = 12, 16, 0.9
    kb = rng.standard_normal((T, D))
    kb[7] = kb[2]                                  # two equal targets: the lowest index wins
    kx = 1.5 * kb[[2] * 4 + [7] * 4 + [0, 1, 3, 4]] + 0.01 * rng.standard_normal((T, D))
    kx[11] = 0.0                                   # an all-zero row: every cosine is 0, match 0, the clamped branch
    raw, m, cos, dk = np_key_nn(kx, kb, lam, eps=EPS)
    assert list(m[:8]) == [2] * 8 and m[11] == 0 and cos[11] == 0.0
    assert np.allclose(dk[11], -(lam / T) * kb[0] / EPS, rtol=1e-14, atol=0.0)
    want, wm, wcos, g = _torch_nn(kx, kb, lam)
    assert np.abs(dk[:11] - g[:11]).max() <= 1e-10 * np.abs(g[:11]).max() and np.abs(dk[11] - g[11]).max() <= 1e-10 * np.abs(g[11]).max()
    raw0, m0, cos0, dk0 = np_key_nn(kb[[0, 1, 2, 3]], kb[[0, 1, 2, 3]], lam)
    assert list(m0) == [0, 1, 2, 3] and abs(raw0) <= 1e-15 and np.abs(dk0).max() <= 1e-15


def test_result_fields_carry_the_keys_where_the_term_is_on():
    from types import SimpleNamespace
    from splice_amd.train import key_nn_fields
    assert key_nn_fields(SimpleNamespace(cfg=dict(DEFAULT_CFG))) == {}
    assert key_nn_fields(SimpleNamespace(key_nn=None)) == {}
    assert key_nn_fields(SimpleNamespace(key_nn=(2.0, 5))) == {LAM: 2.0, LAYER: 5}


class _StubExtractor:
    """``get_keys_from_input(img, layer_num)``: a [heads][T][d] tensor, a differentiable function of the image that differs per block."""
    H, T, d = 2, 5, 4

    def __init__(self):
        self.calls = []

    def get_keys_from_input(self, img, layer_num):
        self.calls.append(layer_num)
        n = self.H * self.T * self.d
        return (layer_num + 1) * (img.mean(dim=(0, 1)).reshape(-1)[:n].reshape(self.H, self.T, self.d) - 0.4)


def test_lossg_facade_equals_np_key_nn():
    from splice_amd.losses import LossG
    rng = np.random.default_rng(9)
    off = dict(lambda_global_ssim=0, lambda_global_cls=0, lambda_entire_cls=0, lambda_entire_ssim=0, lambda_global_identity=0)
    cfg = dict(_cfg(**off), cls_warmup=1, **{LAM: 3.0, LAYER: 5})
    ex = _StubExtractor()
    loss_g = LossG(cfg, extractor=ex)
    assert loss_g.key_nn == (3.0, 5)
    x = torch.from_numpy(rng.random((2, 3, 64, 64))).double().requires_grad_(True)
    b = torch.from_numpy(rng.random((3, 3, 64, 64))).double()   # (one crop more on the target side: the zip drops it)
    loss_g.global_transform = lambda img: img   # (the HIP Resize is not what this test is about)
    assert set(loss_g({"x_global": x}, {"step": 0, "B_global": b})) == {"loss"}   # (before the warm-up step: off)
    ex.calls.clear()
    out = loss_g({"x_global": x}, {"step": 1, "B_global": b})
    assert set(out) == {"loss", KEY_NN_LOSS_KEY} and ex.calls == [5, 5] * 2

    def keys(img):   # the stub's block-5 keys as [T][heads * d], float64
        n = ex.H * ex.T * ex.d
        k = 6 * (img.detach().numpy().mean(0).reshape(-1)[:n].reshape(ex.H, ex.T, ex.d) - 0.4)
        return k.transpose(1, 0, 2).reshape(ex.T, ex.H * ex.d)
    want = sum(np_key_nn(keys(x[i]), keys(b[i]), 3.0)[0] for i in range(2))
    assert abs(out[KEY_NN_LOSS_KEY].item() - want) <= 1e-10 * abs(want)
    assert abs(out["loss"].item() - 3.0 * want) <= 1e-10 * abs(3.0 * want)
    assert abs(loss_g.calculate_key_nn_loss(x.detach(), b).item() - want) <= 1e-10 * abs(want)
    out["loss"].backward()
    assert x.grad is not None and float(x.grad.abs().max()) > 0
    # with the key second-moment term too: both values, the total their weighted sum
    both = LossG(dict(cfg, lambda_global_key_gram=2.0), extractor=_StubExtractor())
    both.global_transform = lambda img: img
    out2 = both({"x_global": x.detach()}, {"step": 1, "B_global": b})
    assert set(out2) == {"loss", KEY_NN_LOSS_KEY, "loss_global_key_gram"}
    assert abs(out2["loss"].item() - (2.0 * out2["loss_global_key_gram"].item() + 3.0 * want)) <= 1e-10 * abs(out2["loss"].item())
    # absent keys: no such term
    plain = LossG({k: v for k, v in cfg.items() if k not in KEY_NN_KEYS}, extractor=_StubExtractor())
    plain.global_transform = lambda img: img
    assert plain.key_nn is None and set(plain({"x_global": x.detach()}, {"step": 1, "B_global": b})) == {"loss"}


def test_binding_and_header_agree_on_the_new_entry_points():
    names = ("splice_step_set_key_nn", "splice_step_key_nn_values", "splice_step_key_nn_match", "splice_key_nn_ws_bytes", "splice_key_nn_pairs")
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splice_hip.h")).read(), flags=re.S)
    for n in names:
        assert n in _lib._SIGNATURES and re.search(r"\b%s\s*\(" % n, header), n
        args = re.search(r"\b%s\s*\((.*?)\);" % n, header, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib._SIGNATURES[n][0]), n
    assert len(_lib._SIGNATURES["splice_key_nn_pairs"][0]) == 20
    lib = _lib.lib()   # (loads without a GPU: the exports are there)
    for n in names:
        assert hasattr(lib, n), n
    assert lib.splice_key_nn_ws_bytes(197, 192, 3) == 3 * 256 * (2 + 2 * 4) * 4 and lib.splice_key_nn_ws_bytes(0, 64, 1) == 0
