"""CPU: the optimiser options beyond the reference's three constructor calls (weight decay, momentum / dampening / nesterov, amsgrad,
centred RMSprop, AdamW) are off by default, checked on the host before anything touches a GPU and shared by the
slots of a sweep; the option record's ctypes mirror has the header's layout; and the NumPy restatement of the rules
(util.np_optim_step) is torch.optim's mathematics."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import DEFAULT_CFG, PAIR_KEYS, MultiPairEngine, MultiScaleEngine, merge_pair_cfgs, snapshot_cfg_mismatch
from splice_amd.generator import OPTIMIZER_KINDS
from splice_amd.util import (OPTIM_EXT_DEFAULTS, OPTIM_EXT_FIELDS, fused_optimizer, fused_optimizer_ext, get_optimizer, np_optim_step, optim_ext_uses,
                             optimizer_options)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every option set of the issue: (optimizer, the optimizer_* keys it sets)
WD = dict(optimizer_weight_decay=0.01)
OPTION_SETS = {}
for _wd_name, _wd in (("", {}), ("_wd", WD)):
    OPTION_SETS["sgd_momentum" + _wd_name] = ("sgd", dict(optimizer_momentum=0.9, **_wd))
    OPTION_SETS["sgd_dampening" + _wd_name] = ("sgd", dict(optimizer_momentum=0.9, optimizer_dampening=0.25, **_wd))
    OPTION_SETS["sgd_nesterov" + _wd_name] = ("sgd", dict(optimizer_momentum=0.9, optimizer_nesterov=True, **_wd))
    OPTION_SETS["rmsprop_momentum" + _wd_name] = ("rmsprop", dict(optimizer_momentum=0.9, **_wd))
    OPTION_SETS["rmsprop_centered" + _wd_name] = ("rmsprop", dict(optimizer_centered=True, **_wd))
    OPTION_SETS["rmsprop_both" + _wd_name] = ("rmsprop", dict(optimizer_momentum=0.9, optimizer_centered=True, **_wd))
OPTION_SETS.update(adam_wd=("adam", dict(WD)), adam_amsgrad=("adam", dict(optimizer_amsgrad=True)), adam_both=("adam", dict(optimizer_amsgrad=True, **WD)),
                   adamw_wd=("adamw", dict(WD)), adamw_amsgrad=("adamw", dict(optimizer_amsgrad=True, **WD)))


def _cfg(name, keys):
    return dict(DEFAULT_CFG, optimizer=name, optimizer_beta1=0.9, optimizer_beta2=0.99, **keys)


def test_options_are_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    for key, default in OPTIM_EXT_DEFAULTS.items():
        assert DEFAULT_CFG[key] == default and packaged[key] == default and type(packaged[key]) is type(default), key
    assert fused_optimizer_ext({}) is None and fused_optimizer_ext(DEFAULT_CFG) is None and fused_optimizer_ext(packaged) is None
    for name in ("adam", "adamw", "rmsprop", "sgd"):   # (adamw without decay is Adam: the plain kernels)
        assert fused_optimizer_ext(dict(DEFAULT_CFG, optimizer=name)) is None, name
    assert set(OPTIM_EXT_DEFAULTS).isdisjoint(PAIR_KEYS)
    assert OPTIMIZER_KINDS == {"adam": 0, "rmsprop": 1, "sgd": 2}
    assert fused_optimizer(dict(DEFAULT_CFG, optimizer="adamw")) == fused_optimizer(dict(DEFAULT_CFG, optimizer="adam")) == (0, 0.0, 0.99, 1e-8)


def test_option_record_of_every_set():
    for tag, (name, keys) in OPTION_SETS.items():
        ext = fused_optimizer_ext(_cfg(name, keys))
        assert ext is not None and tuple(ext) == OPTIM_EXT_FIELDS, tag
        assert ext["decoupled"] == (name == "adamw") and ext["weight_decay"] == keys.get("optimizer_weight_decay", 0.0), tag
        assert ext["momentum"] == keys.get("optimizer_momentum", 0.0) and ext["nesterov"] == keys.get("optimizer_nesterov", False), tag
        kind = fused_optimizer(_cfg(name, keys))[0]
        assert optim_ext_uses(kind, ext) == (kind == 0 or "optimizer_momentum" in keys, kind in (0, 1),
                                            bool(keys.get("optimizer_amsgrad") or keys.get("optimizer_centered"))), tag
        rec = _lib.optim_ext(ext)
        assert [getattr(rec, f) for f in OPTIM_EXT_FIELDS] == [pytest.approx(float(ext[f])) if isinstance(ext[f], float) else int(ext[f]) for f in OPTIM_EXT_FIELDS]


REFUSALS = [
    ("adam", dict(optimizer_momentum=0.9), "'optimizer_momentum'"), ("adamw", dict(optimizer_momentum=0.9), "'optimizer_momentum'"),
    ("adam", dict(optimizer_dampening=0.1), "'optimizer_dampening'"), ("adam", dict(optimizer_nesterov=True), "'optimizer_nesterov'"),
    ("adam", dict(optimizer_centered=True), "'optimizer_centered'"), ("sgd", dict(optimizer_centered=True), "'optimizer_centered'"),
    ("sgd", dict(optimizer_amsgrad=True), "'optimizer_amsgrad'"), ("rmsprop", dict(optimizer_amsgrad=True), "'optimizer_amsgrad'"),
    ("rmsprop", dict(optimizer_dampening=0.1), "'optimizer_dampening'"), ("rmsprop", dict(optimizer_momentum=0.9, optimizer_nesterov=True), "'optimizer_nesterov'"),
    ("sgd", dict(optimizer_nesterov=True), "'optimizer_nesterov'"),                                                  # no momentum
    ("sgd", dict(optimizer_nesterov=True, optimizer_momentum=0.9, optimizer_dampening=0.1), "'optimizer_nesterov'"),   # dampening
    ("sgd", dict(optimizer_weight_decay=-0.1), "'optimizer_weight_decay'"), ("adamw", dict(optimizer_weight_decay=float("inf")), "'optimizer_weight_decay'"),
    ("adam", dict(optimizer_weight_decay=float("nan")), "'optimizer_weight_decay'"), ("adam", dict(optimizer_weight_decay="0.1"), "'optimizer_weight_decay'"),
    ("adam", dict(optimizer_weight_decay=True), "'optimizer_weight_decay'"), ("sgd", dict(optimizer_momentum=-0.5), "'optimizer_momentum'"),
    ("sgd", dict(optimizer_momentum=float("inf")), "'optimizer_momentum'"), ("sgd", dict(optimizer_momentum=0.9, optimizer_dampening=float("nan")), "'optimizer_dampening'"),
    ("sgd", dict(optimizer_nesterov=1), "'optimizer_nesterov'"), ("adam", dict(optimizer_amsgrad="yes"), "'optimizer_amsgrad'"),
    ("rmsprop", dict(optimizer_centered=None), "'optimizer_centered'"),
]


@pytest.mark.parametrize("name,keys,match", REFUSALS)
def test_bad_options_refused_by_key_before_the_gpu(name, keys, match):
    cfg = dict(optimizer=name, **keys)
    with pytest.raises(ValueError, match=match):
        optimizer_options(cfg)
    with pytest.raises(ValueError, match=match):
        fused_optimizer_ext(cfg)
    with pytest.raises(ValueError, match=match):
        MultiPairEngine(cfg, None, [{}], (64, 64), device="cpu")
    with pytest.raises(ValueError, match=match):
        MultiPairEngine(cfg, None, [{}, {}], (64, 64), (64, 64), device="cpu")
    with pytest.raises(ValueError, match=match):
        MultiScaleEngine(cfg, None, {}, (64, 64), device="cpu")
    with pytest.raises(ValueError, match=match):
        get_optimizer(dict(DEFAULT_CFG, **cfg), [torch.nn.Parameter(torch.zeros(3))])


def test_options_are_shared_by_the_slots_of_a_sweep():
    for key, value in (("optimizer_weight_decay", 0.01), ("optimizer_momentum", 0.9), ("optimizer_dampening", 0.1), ("optimizer_nesterov", True),
                       ("optimizer_amsgrad", True), ("optimizer_centered", True)):
        with pytest.raises(ValueError, match=f"'{key}' is shared"):
            merge_pair_cfgs({}, [{}, {key: value}])
        with pytest.raises(ValueError, match=f"'{key}' is shared"):
            MultiPairEngine({}, None, [{}, {}], (64, 64), (64, 64), device="cpu", pair_cfgs=[{}, {key: value}])
    base = dict(optimizer="sgd", optimizer_momentum=0.9)
    assert merge_pair_cfgs(base, [{}, {"optimizer_momentum": 0.9, "lr": 0.1}])[1]["optimizer_momentum"] == 0.9   # the base value is accepted


def test_a_snapshot_from_before_the_options_restores_into_a_default_config():
    old = {k: v for k, v in DEFAULT_CFG.items() if k not in OPTIM_EXT_DEFAULTS}
    assert len(old) == len(DEFAULT_CFG) - 6
    assert snapshot_cfg_mismatch(old, dict(DEFAULT_CFG)) is None and snapshot_cfg_mismatch(dict(DEFAULT_CFG), old) is None
    assert snapshot_cfg_mismatch(old, dict(DEFAULT_CFG, optimizer="sgd", optimizer_momentum=0.9)) == "optimizer"
    assert snapshot_cfg_mismatch(dict(old, optimizer="sgd"), dict(DEFAULT_CFG, optimizer="sgd", optimizer_momentum=0.9)) == "optimizer_momentum"
    assert ("w", "w") in MultiPairEngine.SLOT_ARENAS   # the third moment arena is kept under the state key `w`


def test_exports_declared_bound_and_present():
    names = ("splice_optim_step_ext", "splice_optim_step_pairs_ext", "splice_step_set_optimizer_ext")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["splice_optim_step_ext"][0]) == len(_lib._SIGNATURES["splice_optim_step_ex"][0]) + 2
    assert len(_lib._SIGNATURES["splice_optim_step_pairs_ext"][0]) == len(_lib._SIGNATURES["splice_optim_step_pairs_best"][0]) + 3


def test_option_record_layout_matches_header(tmp_path):
    """The ctypes mirror of splice_optim_ext agrees with the C compiler's layout of the header, and lists the header's fields in order."""
    import re
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splice_hip.h")).read(), flags=re.S)
    body = re.search(r"typedef struct splice_optim_ext \{(.*?)\} splice_optim_ext;", hdr, flags=re.S).group(1)
    header_fields = [d.split()[-1] for d in body.split(";") if d.strip()]
    fields = [f[0] for f in _lib.OptimExt._fields_]
    assert header_fields == fields == list(OPTIM_EXT_FIELDS)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "splice_hip.h"\nint main(void) {\n    printf("%zu", sizeof(splice_optim_ext));\n'
                   + "".join(f'    printf(" %zu", offsetof(splice_optim_ext, {f}));\n' for f in fields) + "    return 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(_lib.OptimExt)] + [getattr(_lib.OptimExt, f).offset for f in fields]


# ---- np_optim_step(float64) is torch.optim in float64: six steps, a changing lr, n = 4099, gradients randn * 10^-step.  Both sides are
# fp64 sequences of fewer than 20 operations per step on the same inputs, each rounding to 2^-53 of its result: 6 * 20 * 1.1e-16 =
# 1.3e-14 of the largest operand, so 1e-10 of the tensor's largest magnitude is four orders above what rounding can produce and far
# below any error of the mathematics (a wrong first-step buffer rule moves p by lr * mu * |g|, about 1e-3).
N, STEPS, LRS = 4099, 6, (2e-3, 1e-3, 5e-3, 2e-3, 4e-4, 3e-3)
TORCH_STATE = {0: ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"), 1: ("momentum_buffer", "square_avg", "grad_avg"), 2: ("momentum_buffer", None, None)}


def _close(got, want, what):
    want = np.asarray(want, dtype=np.float64)
    scale = np.abs(want).max()
    err = np.abs(np.asarray(got, dtype=np.float64) - want).max()
    assert err <= 1e-10 * scale, (what, err, scale)


@pytest.mark.parametrize("tag", sorted(OPTION_SETS))
def test_np_optim_step_is_torch_optim_in_float64(tag):
    name, keys = OPTION_SETS[tag]
    cfg = _cfg(name, keys)
    kind, hp0, hp1, eps = fused_optimizer(cfg)
    ext = fused_optimizer_ext(cfg)
    uses = optim_ext_uses(kind, ext)
    gen = torch.Generator().manual_seed(1234)
    param = torch.nn.Parameter(torch.randn(N, dtype=torch.float64, generator=gen))
    opt = get_optimizer(cfg, [param])
    assert type(opt).__name__.lower() == name
    p = param.detach().numpy().copy()
    m, v, w = (np.zeros(N) if u else None for u in uses)
    for step in range(STEPS):
        g = torch.randn(N, dtype=torch.float64, generator=gen) * 10.0 ** -step
        opt.param_groups[0]["lr"] = LRS[step]
        param.grad = g.clone()
        opt.step()
        p, m, v, w = np_optim_step(kind, p, g.numpy(), m, v, w, LRS[step], hp0, hp1, eps, step + 1, ext, np.float64)
        assert p.dtype == np.float64
        _close(p, param.detach().numpy(), (tag, step, "p"))
        state = opt.state[param]
        for arena, key, used in zip((m, v, w), TORCH_STATE[kind], uses):
            assert (arena is not None) == used
            if used:
                _close(arena, state[key].numpy(), (tag, step, key))


def test_np_optim_step_neutral_is_the_plain_rule():
    rng = np.random.default_rng(3)
    p, g = rng.standard_normal(257).astype(np.float32), rng.standard_normal(257).astype(np.float32)
    f = np.float32
    got = np_optim_step(2, p, g, None, None, None, 0.01, 0.0, 0.0, 0.0, 1)
    assert got[0].dtype == np.float32 and got[0].tobytes() == (p - f(0.01) * g).astype(f).tobytes() and got[1:] == (None, None, None)
    v0 = np.abs(rng.standard_normal(257)).astype(f)
    got = np_optim_step(1, p, g, None, v0, None, 0.01, 0.99, 0.0, 1e-8, 3, dict(weight_decay=0.0))
    v1 = f(0.99) * v0 + (f(1) - f(0.99)) * g * g
    assert got[2].tobytes() == v1.tobytes() and got[0].tobytes() == (p - f(0.01) * (g / (np.sqrt(v1) + f(1e-8)))).tobytes()
