"""CPU: gradient clipping is off by default, its setting is checked on the host before anything touches a GPU, it is shared by the slots
of a sweep, and the NumPy restatement of its rule (engine.np_grad_clip) agrees with torch.nn.utils.clip_grad_norm_."""
import ctypes
import os

import numpy as np
import pytest
import torch
import yaml

from splice_amd import _lib
from splice_amd.engine import CLIP_CHUNK, DEFAULT_CFG, PAIR_KEYS, MultiPairEngine, MultiScaleEngine, grad_clip_rule, merge_pair_cfgs, np_grad_clip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clipping_is_off_by_default():
    with open(os.path.join(ROOT, "splice_amd", "conf", "default", "config.yaml")) as f:
        packaged = yaml.safe_load(f)
    assert DEFAULT_CFG["grad_clip_norm"] == 0.0 and packaged["grad_clip_norm"] == 0.0
    assert grad_clip_rule({}) == 0.0 and grad_clip_rule(packaged) == 0.0


def test_grad_clip_rule_accepts():
    assert grad_clip_rule(dict(grad_clip_norm=1.0)) == 1.0
    assert grad_clip_rule(dict(grad_clip_norm=0)) == 0.0
    assert grad_clip_rule(dict(grad_clip_norm=1e30)) == 1e30
    assert grad_clip_rule(dict(grad_clip_norm=np.float32(0.5))) == 0.5 and grad_clip_rule(dict(grad_clip_norm=np.int64(3))) == 3.0


@pytest.mark.parametrize("value", [True, -0.1, -1, "1.0", None, float("nan"), float("inf"), 1e39])
def test_bad_values_refused_by_key_before_the_gpu(value):
    with pytest.raises(ValueError, match="'grad_clip_norm'"):
        grad_clip_rule({"grad_clip_norm": value})
    with pytest.raises(ValueError, match="'grad_clip_norm'"):
        MultiPairEngine({"grad_clip_norm": value}, None, [{}], (64, 64), device="cpu")
    with pytest.raises(ValueError, match="'grad_clip_norm'"):
        MultiPairEngine({"grad_clip_norm": value}, None, [{}, {}], (64, 64), (64, 64), device="cpu")
    with pytest.raises(ValueError, match="'grad_clip_norm'"):
        MultiScaleEngine({"grad_clip_norm": value}, None, {}, (64, 64), device="cpu")


def test_grad_clip_norm_is_shared_by_the_slots_of_a_sweep():
    assert "grad_clip_norm" not in PAIR_KEYS
    with pytest.raises(ValueError, match="'grad_clip_norm' is shared"):
        merge_pair_cfgs({}, [{}, {"grad_clip_norm": 1.0}])
    with pytest.raises(ValueError, match="'grad_clip_norm' is shared"):
        MultiPairEngine({}, None, [{}, {}], (64, 64), (64, 64), device="cpu", pair_cfgs=[{}, {"grad_clip_norm": 1.0}])
    assert merge_pair_cfgs({"grad_clip_norm": 1.0}, [{}, {"grad_clip_norm": 1.0, "lr": 0.1}])[1]["grad_clip_norm"] == 1.0   # the base value is accepted


def test_clip_exports_declared_bound_and_present():
    names = ("splice_grad_norm_pairs", "splice_optim_step_pairs_clip", "splice_optim_step_clip", "splice_step_set_grad_clip")
    assert set(names) <= set(_lib.exported_symbols())
    hdr = open(os.path.join(ROOT, "include", "splice_hip.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert f"int {n}(" in hdr and hasattr(lib, n), n
    assert len(_lib._SIGNATURES["splice_grad_norm_pairs"][0]) == 11 and len(_lib._SIGNATURES["splice_step_set_grad_clip"][0]) == 3
    assert len(_lib._SIGNATURES["splice_optim_step_pairs_clip"][0]) == len(_lib._SIGNATURES["splice_optim_step_pairs_ema"][0]) + 1
    assert "#define SPLICE_CLIP_CHUNK 4096" in hdr and CLIP_CHUNK == 4096
    assert ctypes.sizeof(_lib.ClipState) == 24 and [f[0] for f in _lib.ClipState._fields_] == ["sumsq", "norm", "coef", "skip", "clipped", "skipped"]
    assert "splice_step_config" in hdr and "grad_clip" not in hdr[hdr.index("typedef struct splice_step_config"):hdr.index("} splice_step_config;")]


def test_clip_state_layout_matches_header(tmp_path):
    """The ctypes mirror of the record agrees with the C compiler's layout of the header."""
    import subprocess
    fields = [f[0] for f in _lib.ClipState._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "splice_hip.h"\nint main(void) {\n    printf("%zu", sizeof(splice_clip_state));\n'
                   + "".join(f'    printf(" %zu", offsetof(splice_clip_state, {f}));\n' for f in fields) + "    return 0;\n}\n")
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "layout")], check=True)
    out = [int(x) for x in subprocess.run([str(tmp_path / "layout")], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [ctypes.sizeof(_lib.ClipState)] + [getattr(_lib.ClipState, f).offset for f in fields]


def test_numpy_restatement_by_hand():
    """n = 6: elements 0..3 are the four components of thread 0, elements 4 and 5 the first two of thread 1 (round 0 of chunk 0); the
    tree then adds thread 1's sum to thread 0's (off = 1, the last level; every other operand is +0)."""
    f = np.float32
    g = np.array([0.1, 0.2, 0.3, 0.4, 0.5, 0.6], dtype=f)
    t0 = f(f(f(f(g[0] * g[0]) + f(g[1] * g[1])) + f(g[2] * g[2])) + f(g[3] * g[3]))
    t1 = f(f(g[4] * g[4]) + f(g[5] * g[5]))
    sumsq, norm, coef, skip = np_grad_clip(g, None, 0.5)
    assert sumsq.dtype == f and norm.dtype == f and coef.dtype == f and skip == 0
    assert sumsq.tobytes() == f(t0 + t1).tobytes()
    assert norm.tobytes() == np.sqrt(f(t0 + t1)).tobytes() and coef.tobytes() == f(f(0.5) / f(norm + f(1e-6))).tobytes() and coef < 1
    assert np_grad_clip(g, None, 10.0)[2] == f(1)                       # under the threshold: the coefficient is exactly 1
    g2 = np.array([1e-8, 0, 0, 0, 0, 0], dtype=f)                       # the second arena is added first: fl(g + g2), then the square
    assert np_grad_clip(g, g2, 0.5)[0].tobytes() == sumsq.tobytes()     # (0.1 + 1e-8 rounds to 0.1)
    assert np_grad_clip(g, g * f(2), 0.5)[0] > f(8) * sumsq


@pytest.mark.parametrize("n", [1, 4097, 100003])
def test_restatement_against_torch_clip_grad_norm(n):
    """sumsq within 2e-6 relative of fp64: at most 2 (the sum of the arenas and its square) + 16 (a thread's adds) + 8 (the tree) + 1 (the
    cast of the fp64 total) = 27 fp32 roundings of 2^-24 each, 1.6e-6; the fp64 stage adds nothing visible."""
    gen = torch.Generator().manual_seed(n)
    g, g2 = torch.randn(n, generator=gen), torch.randn(n, generator=gen) * 0.5
    for second in (None, g2):
        s64 = (g + second).double() if second is not None else g.double()
        ref_norm = float(s64.norm())
        c = 0.5 * ref_norm
        sumsq, norm, coef, skip = np_grad_clip(g.numpy(), None if second is None else second.numpy(), c)
        assert skip == 0 and abs(float(sumsq) - ref_norm ** 2) <= 2e-6 * ref_norm ** 2, (n, float(sumsq), ref_norm ** 2)
        f = np.float32
        assert norm.tobytes() == np.sqrt(sumsq).tobytes() and coef.tobytes() == np.minimum(f(1), f(c) / (norm + f(1e-6))).tobytes()
        # the gradient torch leaves behind: clip_grad_norm_ multiplies by clamp(max_norm / (norm + 1e-6), max=1)
        p = torch.nn.Parameter(torch.zeros(n, dtype=torch.float64))
        p.grad = s64.clone()
        total = torch.nn.utils.clip_grad_norm_([p], c)
        assert abs(float(total) - float(norm)) <= 2e-6 * ref_norm
        mine = (s64.numpy().astype(f) * coef).astype(np.float64)
        assert np.abs(mine - p.grad.numpy()).max() <= 4e-6 * np.abs(p.grad.numpy()).max()   # (s in fp32, the coefficient, the product: 3 roundings + sumsq's)


@pytest.mark.parametrize("bad", [float("inf"), float("-inf"), float("nan")])
def test_a_non_finite_gradient_is_skipped(bad):
    g = np.ones(5000, dtype=np.float32)
    g[4321] = bad
    sumsq, norm, coef, skip = np_grad_clip(g, None, 1.0)
    assert skip == 1 and coef == 0 and not np.isfinite(norm)
    g[4321] = 1.0
    assert np_grad_clip(g, None, 1.0)[3] == 0
    g2 = np.zeros_like(g)
    g2[7] = bad                                                         # ... in the second arena alike
    assert np_grad_clip(g, g2, 1.0)[3] == 1
    big = np.full(8, 3e19, dtype=np.float32)                            # finite elements whose squares overflow fp32: skipped as well
    assert np_grad_clip(big, None, 1.0)[3] == 1
