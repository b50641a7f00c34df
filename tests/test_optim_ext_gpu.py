"""GPU: the extended rules of the fused update -- weight decay, momentum / dampening / nesterov, amsgrad, centred RMSprop, AdamW
(DESIGN.md section 9i).  Op level: neutral options give the plain kernels' bits; every option set against the fp64 restatement
(util.np_optim_step) under a bar measured from the fp32 restatement; SGD exactly; an element's result does not depend on alignment,
batch or where the lr comes from; the stop, clip, average and best-window parts compose; the launcher refuses incomplete calls.
Step level (the 64x64 dino_vits8 setup of test_optim_gpu.py): the fused step is a skip-mode step's gradient followed by the op-level
call, graph replay included; pairs equal their single runs; frozen and parked slots, snapshots, checkpoints, the several-scales
engine and train_model carry the third arena."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.engine import DEFAULT_CFG, MultiPairEngine, MultiScaleEngine, SpliceEngine, np_ema
from splice_amd.generator import optim_step
from splice_amd.util import fused_optimizer, fused_optimizer_ext, np_optim_step, optim_ext_uses

pytestmark = pytest.mark.gpu
DEV = "cuda"

# every option set of tests/test_optim_ext_cpu.py: (optimizer, the optimizer_* keys it sets)
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
TAGS = sorted(OPTION_SETS)
# the three sets of the step-level tests: between them every arena, the decoupled decay and all three kinds
STEP_SETS = {"sgd_nesterov": ("sgd", dict(optimizer_momentum=0.9, optimizer_nesterov=True)),
             "rmsprop_both": ("rmsprop", dict(optimizer_momentum=0.9, optimizer_centered=True)),
             "adamw_amsgrad": ("adamw", dict(optimizer_amsgrad=True, **WD))}
SHAPES = [(100003, 0), (4099, 1)]   # vector body + scalar tail; a view 4 bytes off 16-byte alignment: all tail (tests/test_optim_gpu.py)
LRS = (2e-3, 1.5e-3, 7e-4, 3e-3)
ARENAS = ("p", "m", "v", "w")


def _rule(tag, sets=OPTION_SETS):
    """(kind, (hp0, hp1, eps), ext, (uses_m, uses_v, uses_w)) of an option set; Adam with betas (0.9, 0.99)."""
    name, keys = sets[tag]
    cfg = dict(DEFAULT_CFG, optimizer=name, optimizer_beta1=0.9, optimizer_beta2=0.99, **keys)
    kind, *hp = fused_optimizer(cfg)
    ext = fused_optimizer_ext(cfg)
    return kind, tuple(hp), ext, optim_ext_uses(kind, ext)


def _bits(a, b):
    a, b = (x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x) for x in (a, b))
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _dev(x, off=0):
    """A device copy of ``x`` that starts ``off`` floats into its allocation."""
    base = torch.zeros(x.numel() + off, device=DEV)
    base[off:] = x.reshape(-1).to(DEV)
    return base[off:]


# ---------------------------------------------------------------------------------------------------------------- op level
_INPUTS, _KERNEL, _NUMPY = {}, {}, {}


def _inputs(n):
    """Host inputs of the four-step runs, a function of n alone: p0 and per step (g, g2).  Magnitudes stay within [1e-6, 1e2] but
    for the odd normal deviate near zero -- nothing comes near a denormal."""
    if n not in _INPUTS:
        gen = torch.Generator().manual_seed(900 + n)
        p0 = torch.randn(n, generator=gen)
        _INPUTS[n] = (p0, [(torch.randn(n, generator=gen) * 10.0 ** -step, torch.randn(n, generator=gen) * 1e-2) for step in range(1, 5)])
    return _INPUTS[n]


def _kernel_run(tag, n, off, lr_dev=False):
    """Four steps of the extended kernels from zero moments (computed once, left unchanged): the final arenas on the host."""
    key = (tag, n, off, lr_dev)
    if key not in _KERNEL:
        kind, hp, ext, uses = _rule(tag)
        p0, steps = _inputs(n)
        p, m, v, w = _dev(p0, off), _dev(torch.zeros(n), off), _dev(torch.zeros(n), off), _dev(torch.zeros(n), off)
        assert p.data_ptr() % 16 == 4 * off and w.data_ptr() % 16 == 4 * off
        lrd = torch.zeros(1, device=DEV)
        for t, (lr, (g, _)) in enumerate(zip(LRS, steps), start=1):
            lrd.fill_(lr)
            optim_step(kind, p, _dev(g, off), m, v, 123.0 if lr_dev else lr, *hp, t, ext=ext, w=w, lr_dev=lrd if lr_dev else None)
        torch.cuda.synchronize()
        got = dict(p=p, m=m, v=v, w=w)
        for name, used in zip(ARENAS[1:], uses):
            if not used:
                assert not got[name].any(), (tag, name)   # an arena the rule does not keep is never written
        _KERNEL[key] = {k: x.cpu().numpy().copy() for k, x in got.items()}
    return _KERNEL[key]


def _numpy_run(tag, n, dtype):
    """The same four steps by util.np_optim_step at ``dtype`` (computed once, left unchanged)."""
    key = (tag, n, np.dtype(dtype).name)
    if key not in _NUMPY:
        kind, hp, ext, uses = _rule(tag)
        p0, steps = _inputs(n)
        p = p0.numpy().astype(dtype)
        m, v, w = (np.zeros(n, dtype) if u else None for u in uses)
        for t, (lr, (g, _)) in enumerate(zip(LRS, steps), start=1):
            p, m, v, w = np_optim_step(kind, p, g.numpy(), m, v, w, np.float32(lr), *hp, t, ext, dtype)
        _NUMPY[key] = dict(p=p, m=m, v=v, w=w)
    return _NUMPY[key]


@pytest.mark.parametrize("n,off", SHAPES)
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_neutral_options_give_the_plain_kernels_bits(kind, n, off):
    """An explicit neutral record takes the extended kernels (a zero weight_decay / momentum is a branch) and leaves p, g, m, v as the
    plain export does, over four steps with g2 and zero_grad alternating."""
    hp = fused_optimizer(dict(optimizer=("adam", "rmsprop", "sgd")[kind], optimizer_beta1=0.9, optimizer_beta2=0.99))[1:]
    p0, steps = _inputs(n)
    runs = []
    for ext in (None, {}):
        p, m, v = _dev(p0, off), _dev(torch.full((n,), 0.25), off), _dev(torch.full((n,), 0.5), off)
        gs = []
        for t, (lr, (g, g2)) in enumerate(zip(LRS, steps), start=1):
            gg = _dev(g, off)
            optim_step(kind, p, gg, m, v, lr, *hp, t, zero_grad=t % 2 == 0, g2=_dev(g2, off) if t > 2 else None, ext=ext)
            gs.append(gg)
        torch.cuda.synchronize()
        runs.append([p, m, v] + gs)
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), (kind, i)
    assert not torch.equal(runs[0][0], _dev(p0, off)) and not runs[0][4].any() and _bits(runs[0][5], steps[2][0] + steps[2][1])


@pytest.mark.parametrize("n,off", SHAPES)
@pytest.mark.parametrize("tag", TAGS)
def test_every_option_set_against_float64(tag, n, off):
    """Four steps against np_optim_step(float64) on the same inputs.  The bar is measured here: e32 is the deviation of
    np_optim_step(float32) -- the reference at the kernel's precision -- from the fp64 run; the kernel's deviation must be
    <= 2 * e32 + one ulp of max|x| (two legitimate fp32 evaluations of the same dozen operations may round apart by about their own
    error), for p and for every moment arena the rule keeps.  Measured on an MI355X: DESIGN.md section 9i."""
    got, r32, r64 = _kernel_run(tag, n, off), _numpy_run(tag, n, np.float32), _numpy_run(tag, n, np.float64)
    for name in ARENAS:
        if r64[name] is None:
            continue
        assert np.isfinite(got[name]).all() and np.isfinite(r64[name]).all(), (tag, name)
        dev = np.abs(got[name].astype(np.float64) - r64[name]).max()
        e32 = np.abs(r32[name].astype(np.float64) - r64[name]).max()
        ulp = float(np.spacing(np.float32(np.abs(r64[name]).max())))
        print(f"{tag} n={n} off={off} {name}: kernel {dev:.3e}  fp32 restatement {e32:.3e}  ulp {ulp:.3e}")
        assert dev <= 2 * e32 + ulp, (tag, name, dev, e32, ulp)


@pytest.mark.parametrize("n,off", SHAPES)
@pytest.mark.parametrize("tag", [t for t in TAGS if t.startswith("sgd")])
def test_sgd_rules_are_exact(tag, n, off):
    """No sqrt, division or pow in the extended SGD rules: the kernel equals np_optim_step(float32) bit for bit."""
    got, r32 = _kernel_run(tag, n, off), _numpy_run(tag, n, np.float32)
    assert _bits(got["p"], r32["p"]) and _bits(got["m"], r32["m"]), tag
    assert np.abs(r32["m"]).max() > 0 and not _bits(r32["p"], _inputs(n)[0])


@pytest.mark.parametrize("tag", TAGS)
def test_alignment_and_lr_source_change_no_bit(tag):
    """The same 4099 values on the vector path and on the all-scalar path, and with the lr read from the device: every arena equal."""
    a, b, c = _kernel_run(tag, 4099, 0), _kernel_run(tag, 4099, 1), _kernel_run(tag, 4099, 0, lr_dev=True)
    for name in ARENAS:
        assert _bits(a[name], b[name]) and _bits(a[name], c[name]), (tag, name)


def _pairs_ext(kind, hp, ext, a, P, stride, n, lrs, step=0, step_dev=None, stop=None, zero_grad=0, ema=False, clip=None, best=None, w=True):
    L = _lib.lib()
    return L.splice_optim_step_pairs_ext(kind, _lib.ptr(a["p"]), _lib.ptr(a["g"]), _lib.ptr(a.get("g2")), _lib.ptr(a["m"]), _lib.ptr(a["v"]),
                                         _lib.ptr(a["w"]) if w else None, _lib.ptr(a["e"]) if ema else None, P, stride, n, _lib.ptr(lrs), *hp, step,
                                         _lib.ptr(step_dev), _lib.ptr(stop), zero_grad, 0.9, 1, _lib.ptr(clip), _lib.ptr(best),
                                         _lib.ptr(a["bp"]) if best is not None else None, _lib.ptr(a["be"]) if best is not None and ema else None,
                                         C.byref(_lib.optim_ext(ext)), _lib.current_stream())


def _sentinel(n):
    return -7.0 - torch.arange(n, dtype=torch.float32) % 13


def _arenas(P, stride, n, seed):
    """Host arenas of P slots mid-run: moments a run could hold (v > w^2, so the centred rule stays real), zero gradients in the padding."""
    gen = torch.Generator().manual_seed(seed)
    tot = P * stride if P > 1 else n
    host = dict(p=torch.randn(tot, generator=gen), m=torch.randn(tot, generator=gen) * 0.1, v=torch.rand(tot, generator=gen) * 0.1 + 0.01,
                w=torch.rand(tot, generator=gen) * 0.05, e=torch.randn(tot, generator=gen), g=torch.zeros(tot), g2=torch.zeros(tot))
    for s in range(P):
        host["g"][s * stride: s * stride + n] = torch.randn(n, generator=gen)
        host["g2"][s * stride: s * stride + n] = torch.randn(n, generator=gen) * 0.3
        for k in "pmvwe":   # (the padding of a run's arenas holds zeros)
            host[k][s * stride + n: (s + 1) * stride] = 0.0
    host["bp"], host["be"] = _sentinel(tot), _sentinel(tot) - 100
    return host, lambda: {k: _dev(x) for k, x in host.items()}


@pytest.mark.parametrize("tag", TAGS)
def test_three_pairs_equal_three_single_calls(tag):
    """P = 3 arenas of 4099 floats at stride 4160 with per-pair lrs in one launch == three single-arena calls, every arena, w
    included; the padding floats between two arenas stay zero under every rule."""
    kind, hp, ext, uses = _rule(tag)
    P, n, stride, t = 3, 4099, 4160, 3
    host, dev = _arenas(P, stride, n, 40 + kind)
    lrs = [1e-3, 2e-3, 5e-4]
    got = dev()
    assert _pairs_ext(kind, hp, ext, got, P, stride, n, torch.tensor(lrs, device=DEV), step=t, zero_grad=1) == 0, _lib.lib().splice_last_error()
    torch.cuda.synchronize()
    for s in range(P):
        sl = slice(s * stride, s * stride + n)
        one = {k: _dev(host[k][sl]) for k in ("p", "g", "g2", "m", "v", "w")}
        optim_step(kind, one["p"], one["g"], one["m"], one["v"], lrs[s], *hp, t, zero_grad=True, g2=one["g2"], ext=ext, w=one["w"])
        for name, used in zip(ARENAS, (True,) + uses):
            assert _bits(got[name][sl], one[name] if used else host[name][sl]), (tag, s, name)
        assert not got["g"][sl].any() and not _bits(got["p"][sl], host["p"][sl])
        for name in ARENAS:
            assert not got[name][s * stride + n: (s + 1) * stride].any(), (tag, s, name, "padding")


COMPOSE = ["sgd_nesterov_wd", "rmsprop_both_wd", "adamw_amsgrad"]


@pytest.mark.parametrize("zero_grad", [0, 1])
@pytest.mark.parametrize("tag", COMPOSE)
def test_stop_clip_average_and_best_compose(tag, zero_grad):
    """Three slots at step index 2 through the pairs export, every optional part at once.  Slot 0 runs with a clip coefficient of 0.5
    and takes the best snapshot; slot 1's clip record has skip set; slot 2 was frozen by its stop record at step 0."""
    kind, hp, ext, uses = _rule(tag)
    P, n, stride, t = 3, 4099, 4160, 3
    host, dev = _arenas(P, stride, n, 60 + kind)
    lrs = [1e-3, 2e-3, 5e-4]
    step_dev = torch.full((1,), t, dtype=torch.int32, device=DEV)
    stop = torch.tensor([[0, 0, 0, 0, 0, -1], [0, 0, 0, 0, 0, -1], [0, 0, 0, 0, 0, 0]], dtype=torch.int32).to(DEV)
    raw = np.zeros((P, 6), dtype=np.int32)
    raw.view(np.float32)[:, 2] = [0.5, 0.0, 0.5]
    raw[:, 3] = [0, 1, 0]
    clip = torch.from_numpy(raw).to(DEV)
    best = torch.tensor([[2, 0], [2, 0], [2, 0]], dtype=torch.int32).to(DEV)
    got = dev()
    rc = _pairs_ext(kind, hp, ext, got, P, stride, n, torch.tensor(lrs, device=DEV), step_dev=step_dev, stop=stop, zero_grad=zero_grad, ema=True, clip=clip, best=best)
    assert rc == 0, _lib.lib().splice_last_error()
    torch.cuda.synchronize()
    s0, s1, s2 = (slice(s * stride, s * stride + n) for s in range(P))
    # slot 0: the update of the clipped sum fl(fl(g + g2) * 0.5) -- a single-arena call on that gradient -- and where g is written back
    # it holds that sum, without the decay term
    clipped = (_dev(host["g"][s0]) + _dev(host["g2"][s0])) * 0.5
    one = dict({k: _dev(host[k][s0]) for k in ARENAS}, g=clipped.clone())
    assert _pairs_ext(kind, hp, ext, one, 1, 0, n, torch.tensor(lrs[:1], device=DEV), step_dev=step_dev) == 0, _lib.lib().splice_last_error()
    for name, used in zip(ARENAS, (True,) + uses):
        assert _bits(got[name][s0], one[name] if used else host[name][s0]), (tag, name)
    assert not _bits(got["p"][s0], host["p"][s0])
    assert not got["g"][s0].any() if zero_grad else _bits(got["g"][s0], clipped), tag
    # ... the average and the best copies follow the p just written
    assert _bits(got["e"][s0], np_ema(host["e"][s0].numpy(), got["p"][s0].cpu().numpy(), t, 0.9, 1))
    assert _bits(got["bp"][s0], got["p"][s0]) and _bits(got["be"][s0], got["e"][s0])
    # slot 1, skipped by the clip guard: nothing written, no decoupled decay; its g only as the zeros of zero_grad; it still takes
    for name in ARENAS + ("e",):
        assert _bits(got[name][s1], host[name][s1]), (tag, name)
    assert not got["g"][s1].any() if zero_grad else _bits(got["g"][s1], host["g"][s1])
    assert _bits(got["bp"][s1], host["p"][s1]) and _bits(got["be"][s1], host["e"][s1])
    # slot 2, frozen: untouched, its gradient too
    for name in ARENAS + ("e", "g", "bp", "be"):
        assert _bits(got[name][s2], host[name][s2]), (tag, name)


def test_launcher_refusals():
    """An error and a message, and no launch: the arenas stay what they were."""
    L = _lib.lib()
    n = 1027
    host, dev = _arenas(1, 0, n, 5)
    a = dev()
    s = _lib.current_stream()

    def call(kind, ext, m=True, v=True, w=True, step=1):
        return L.splice_optim_step_ext(kind, _lib.ptr(a["p"]), _lib.ptr(a["g"]), None, _lib.ptr(a["m"]) if m else None, _lib.ptr(a["v"]) if v else None,
                                       _lib.ptr(a["w"]) if w else None, n, 1e-3, None, 0.9, 0.99, 1e-8, step, 0, C.byref(_lib.optim_ext(ext)), s)
    assert call(0, dict(amsgrad=True), w=False) != 0 and b"w arena" in L.splice_last_error()
    assert call(1, dict(centered=True), w=False) != 0 and b"w arena" in L.splice_last_error()
    assert call(2, dict(momentum=0.9), m=False) != 0 and b"m arena" in L.splice_last_error()
    assert call(1, dict(momentum=0.9), m=False) != 0 and b"m arena" in L.splice_last_error()
    assert call(1, dict(), v=False) != 0 and b"v arena" in L.splice_last_error()
    assert call(2, dict(nesterov=True)) != 0 and b"nesterov" in L.splice_last_error()
    assert call(2, dict(nesterov=True, momentum=0.9, dampening=0.5)) != 0 and b"nesterov" in L.splice_last_error()
    assert call(2, dict(momentum=0.9), step=0) != 0 and b"step count" in L.splice_last_error()
    assert call(0, dict(weight_decay=0.01), step=0) != 0 and b"step count" in L.splice_last_error()
    assert call(0, dict(momentum=0.9)) != 0 and b"Adam has no momentum" in L.splice_last_error()
    assert call(2, dict(centered=True)) != 0 and call(1, dict(amsgrad=True)) != 0 and call(2, dict(decoupled=True)) != 0
    assert call(2, dict(weight_decay=-1.0)) != 0 and call(2, dict(momentum=float("inf"))) != 0 and call(2, dict(momentum=0.5, dampening=float("nan"))) != 0
    assert L.splice_optim_step_ext(2, _lib.ptr(a["p"]), _lib.ptr(a["g"]), None, None, None, None, n, 1e-3, None, 0.0, 0.0, 0.0, 1, 0, None, s) != 0
    torch.cuda.synchronize()
    for k in ("p", "g", "m", "v", "w"):
        assert _bits(a[k], host[k]), k
    assert call(2, dict(momentum=0.9), v=False, w=False) == 0 and call(0, dict(amsgrad=True)) == 0   # (complete calls go through)
    torch.cuda.synchronize()
    assert not _bits(a["p"], host["p"]) and not _bits(a["w"], host["w"])


# -------------------------------------------------------------------------------------------------------------- step level
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


REGIMES = dict(cls_warmup=2, entire_A_every=4)


def _cfg(tag=None, **over):
    name, keys = STEP_SETS[tag] if tag else ("adam", {})
    cfg = dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, optimizer=name, optimizer_beta1=0.9, **REGIMES)
    cfg.update(keys)
    cfg.update(over)
    return cfg


def _pair(seed=73, P=None):
    if P is None:
        A, B = synth.smooth_image_pair(seed, 0, 64, 64)
        return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)
    imgs = [synth.smooth_image_pair(seed, p, 64, 64) for p in range(P)]
    return (torch.from_numpy(np.stack([a for a, _ in imgs])).to(DEV), torch.from_numpy(np.stack([b for _, b in imgs])).to(DEV))


def _graphs(eng):
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    return stats[0] + stats[2]


def _moments(eng):
    return dict(params=eng.params, m=eng.m, v=eng.v, **({} if eng.w is None else dict(w=eng.w)))


@pytest.mark.parametrize("tag", list(STEP_SETS))
def test_fused_step_is_gradient_then_op_level_call_under_graph_replay(tag, vit):
    """8 steps at fixed crops (the graph is captured at the third step and replayed; steps 0 and 4 take the entire-image branch, steps
    0 and 1 lie before cls_warmup): graph on == graph off == a chain of skip-mode steps, each followed by the op-level call with the
    step count on the device, on params, m, v and w, bit for bit."""
    cfg = _cfg(tag)
    gen = synth.generator_params(82, 0.02)
    A, B = _pair(74)
    graph = SpliceEngine(cfg, None, gen, (64, 64), (64, 64), vit_engine=vit)
    eager = SpliceEngine(cfg, None, gen, (64, 64), (64, 64), vit_engine=vit)
    _lib.check(_lib.lib().splice_step_use_graph(eager.handle, 0))
    chain = SpliceEngine(dict(cfg, optimizer_weight_decay=0.0, optimizer_momentum=0.0, optimizer_nesterov=False, optimizer_amsgrad=False, optimizer_centered=False),
                         None, gen, (64, 64), (64, 64), vit_engine=vit)
    _lib.check(_lib.lib().splice_step_set_mode(chain.handle, 1, 0), "step_set_mode")
    kind, *hp = fused_optimizer(graph.cfg)
    ext = graph.opt_ext
    uses = optim_ext_uses(kind, ext)
    assert ext is not None and chain.opt_ext is None and chain.w is None and (graph.w is not None) == uses[2]
    w = torch.zeros_like(chain.params) if uses[2] else None
    lr_dev = torch.full((1,), graph.cfg["lr"], device=DEV)
    step_dev = torch.zeros(1, dtype=torch.int32, device=DEV)
    arenas = dict(p=chain.params, g=chain.grads, m=chain.m, v=chain.v, w=w)
    for k in range(8):
        for e in (graph, eager, chain):
            e.step(A, B, A)
        step_dev.fill_(k + 1)
        assert _pairs_ext(kind, hp, ext, arenas, 1, 0, chain.gen.numel, lr_dev, step_dev=step_dev, w=w is not None) == 0, _lib.lib().splice_last_error()
        torch.cuda.synchronize()
        for other in (eager, chain):
            assert torch.equal(graph.losses_dev, other.losses_dev), (tag, k)
            assert torch.equal(graph.params, other.params), (tag, k, (graph.params - other.params).abs().max().item())
        assert torch.equal(graph.m, chain.m) and torch.equal(graph.v, chain.v) and torch.equal(graph.m, eager.m) and torch.equal(graph.v, eager.v), (tag, k)
        if w is not None:
            assert torch.equal(graph.w, w) and torch.equal(graph.w, eager.w), (tag, k)
    assert graph.m.any() and (w is None or w.any())
    assert _graphs(graph) >= 1 and _graphs(eager) == 0


_MULTI = {}


def _multi(tag, vit):
    """A three-slot sweep over the lr run 8 steps (once per set, left unchanged): the engine, its per-step losses, a snapshot of
    slot 2 behind step 3."""
    if tag not in _MULTI:
        lrs = [2e-3, 5e-4, 1e-3]
        gens = [synth.generator_params(83 + p, 0.02) for p in range(3)]
        A, B = _pair(75, P=3)
        multi = MultiPairEngine(_cfg(tag), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=[dict(lr=lr) for lr in lrs])
        hist, snap = [], None
        for k in range(8):
            hist.append(multi.step(A, B, A).clone())
            if k == 3:
                snap = multi.snapshot(2)
        torch.cuda.synchronize()
        _MULTI[tag] = (multi, hist, snap, lrs, gens, A, B)
    return _MULTI[tag]


@pytest.mark.parametrize("tag", list(STEP_SETS))
def test_three_pairs_equal_their_single_runs(tag, vit):
    multi, hist, _, lrs, gens, A, B = _multi(tag, vit)
    n = multi.gen.numel
    assert (multi.w is not None) == optim_ext_uses(multi.opt_kind, multi.opt_ext)[2]
    for p in range(3):
        single = SpliceEngine(_cfg(tag, lr=lrs[p]), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for i in range(8):
            single.step(A[p], B[p], A[p])
            assert torch.equal(single.losses_dev[0], hist[i][p]), (tag, p, i)
        torch.cuda.synchronize()
        for name, arena in _moments(single).items():
            assert torch.equal(arena, getattr(multi, name)[p * multi.stride: p * multi.stride + n]), (tag, p, name)
    assert not torch.equal(multi.pair_params(0), multi.pair_params(1))


@pytest.mark.parametrize("tag", list(STEP_SETS))
def test_a_snapshot_moves_into_an_engine_of_another_slot_count(tag, vit):
    """Slot 2 of the three-slot engine behind step 3, restored into a fresh one-pair engine (another arena stride, the scalar lr path):
    steps 4 .. 7 are, bit for bit, the unbroken run's."""
    multi, hist, snap, lrs, gens, A, B = _multi(tag, vit)
    assert snap["step_idx"] == 3 and ("w" in snap) == (multi.w is not None) and "m" in snap
    single = SpliceEngine(_cfg(tag, lr=lrs[2]), None, synth.generator_params(99, 0.02), (64, 64), (64, 64), vit_engine=vit)
    assert single.stride != multi.stride
    single.restore([snap])
    for k in range(4, 8):
        single.step(A[2], B[2], A[2])
        assert torch.equal(single.losses_dev[0], hist[k][2]), (tag, k)
    a, b = multi.snapshot(2, device="cpu"), single.snapshot(0, device="cpu")
    assert sorted(a) == sorted(b)
    for key in ("params", "m", "v", "w", "running"):
        if key in a:
            assert _bits(a[key], b[key]), (tag, key)
    if multi.w is not None:   # a state without the arena the rule keeps is refused by its name
        fresh = SpliceEngine(_cfg(tag, lr=lrs[2]), None, gens[2], (64, 64), (64, 64), vit_engine=vit)
        with pytest.raises(ValueError, match="'w'"):
            fresh.restore([{k: v for k, v in snap.items() if k != "w"}])


# entire-image steps 0 4 8 12; counted steps 2 3 | 5 6 | 7 9 | 10 11: windows close at steps 3, 6, 9 and 11.  Slots 0 and 2 run with lr 0:
# their loss never moves, so with stop_patience 2 they stop at the close of the third window, step 9
STOP = dict(stop_window=2, stop_rel=0.01, stop_patience=2, n_epochs=13)
STOP_LRS = [0.0, 2e-3, 0.0]


@pytest.mark.parametrize("tag", list(STEP_SETS))
def test_a_frozen_slot_keeps_its_four_arenas_and_parking_it_changes_nothing(tag, vit):
    gens = [synth.generator_params(70 + p, 0.02) for p in range(3)]
    A, B = _pair(71)
    As, Bs = A[None].expand(3, -1, -1, -1).contiguous(), B[None].expand(3, -1, -1, -1).contiguous()
    pair_cfgs = [dict(lr=lr) for lr in STOP_LRS]
    off = MultiPairEngine(_cfg(tag, **STOP), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=pair_cfgs)
    on = MultiPairEngine(_cfg(tag, stop_compact=True, **STOP), None, gens, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=pair_cfgs)
    at_step = []
    for k in range(13):
        off.step(As, Bs, As)
        on.step(As, Bs, As)
        at_step.append({name: arena.clone() for name, arena in _moments(off).items()})
    torch.cuda.synchronize()
    stops = off.stopped_at
    print(f"{tag}: stop steps {stops}")
    assert stops[0] == stops[2] == 9 and stops[1] is None, stops                # the premise
    assert on.stopped_at == stops and on.live == [1] and sorted(on._parked) == [0, 2]
    n, stride = off.gen.numel, off.stride
    for p in (0, 2):   # frozen behind step 9: the four arenas are those of the stop step, which still updated them
        for name, arena in _moments(off).items():
            sl = slice(p * stride, p * stride + n)
            assert torch.equal(arena[sl], at_step[9][name][sl]), (tag, p, name)
            if name != "params" and dict(zip(("m", "v", "w"), optim_ext_uses(off.opt_kind, off.opt_ext)))[name]:   # (lr 0 moves no weight; the moments went on until the stop step)
                assert not torch.equal(at_step[9][name][sl], at_step[8][name][sl]), (tag, p, name)
    for p in range(3):
        a, b = on.snapshot(p, device="cpu"), off.snapshot(p, device="cpu")
        assert sorted(a) == sorted(b) and ("w" in a) == (off.w is not None)
        for key in ("params", "m", "v", "w", "running"):
            if key in a:
                assert _bits(a[key], b[key]), (tag, p, key)
    assert on.losses(1) == off.losses(1)


def test_multiscale_sgd_momentum_is_the_hand_formula(vit):
    """Scales 64 and 96, SGD with momentum 0.9 and weight decay: b = d at the first step, then 0.9 b + d, and p -= lr b, exactly."""
    cfg = _cfg(None, optimizer="sgd", optimizer_momentum=0.9, optimizer_weight_decay=0.01, entire_A_every=2, lr=0.05)
    eng = MultiScaleEngine(cfg, None, synth.generator_params(84, 0.02), (64, 64), (64, 64), scales=(64, 96), vit_engine=vit)
    assert eng.opt_ext is not None and eng.w is None and all(e.opt_ext is None for e in eng.engines)
    A, B = _pair(76)
    buf = None
    f = lambda x: float(np.float32(x))
    for k in range(3):
        before = eng.params.clone()
        eng.step(A, B, A)
        torch.cuda.synchronize()
        d = eng.grads + before * f(0.01)
        buf = d if k == 0 else buf * f(0.9) + d           # (separate launches: every operation rounded once; 1 - dampening is 1)
        assert torch.equal(eng.engines[0].m, buf), k
        assert torch.equal(eng.params, before - buf * f(0.05)), k
        assert not torch.equal(eng.params, before - eng.grads * f(0.05))


def test_a_default_engine_is_what_it_was(vit):
    """Every new key at its default: no third arena, no option record, the snapshot's keys are those of before, and 8 steps capture
    the same two graphs -- the ordinary sequence at step 2 (the third step of equal shapes, the first behind cls_warmup) and the
    entire-image sequence at step 4 -- as an engine under an extended rule does."""
    A, B = _pair(77)
    counts = []
    for tag in (None, "rmsprop_both"):
        eng = SpliceEngine(_cfg(tag), None, synth.generator_params(85, 0.02), (64, 64), (64, 64), vit_engine=vit)
        for _ in range(8):
            eng.step(A, B, A)
        torch.cuda.synchronize()
        counts.append(_graphs(eng))
        if tag is None:
            assert eng.opt_ext is None and eng.w is None
            assert sorted(eng.snapshot(0)) == sorted(["format", "step_idx", "cfg", "n_crops", "crop_hw", "entire_hw", "generator_calls", "params", "m", "v", "running", "losses"])
    assert counts == [2, 2], counts


def _write_pair(root, name, size=72, seed=60):
    from PIL import Image
    A, B = synth.smooth_image_pair(seed, 0, size, size)
    for side, img in (("A", A), ("B", B)):
        d = root / name / side
        d.mkdir(parents=True)
        Image.fromarray((img.transpose(1, 2, 0) * 255).astype(np.uint8)).save(d / "img.png")
    return str(root / name)


TRAIN = dict(seed=3, dino_model_name="dino_vits8", dino_global_patch_size=64, cls_warmup=1, entire_A_every=5, use_augmentations=False,
             global_A_crops_min_cover=1.0, global_B_crops_min_cover=1.0)


class Interrupt(Exception):
    pass


def test_train_model_resumes_under_sgd_momentum(tmp_path):
    """12 epochs with a checkpoint every 4, interrupted at the image of epoch 9 and resumed: output.png and the final arenas -- the
    momentum buffer among them -- are those of the run left alone."""
    from splice_amd.train import CHECKPOINT_NAME, train_model
    vit_state = synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)
    over = dict(TRAIN, n_epochs=12, log_images_freq=3, checkpoint_every=4, optimizer="sgd", optimizer_momentum=0.9, optimizer_weight_decay=0.01, lr=0.01)
    whole = train_model(_write_pair(tmp_path, "whole"), cfg_overrides=over, vit_state=vit_state, progress=False)
    root = _write_pair(tmp_path, "cut")
    images = []

    def callback(image):
        images.append(len(images))
        if len(images) == 3:
            raise Interrupt()
    with pytest.raises(Interrupt):
        train_model(root, callback=callback, cfg_overrides=over, vit_state=vit_state, progress=False)
    state = torch.load(os.path.join(root, "out", CHECKPOINT_NAME), map_location="cpu", weights_only=False)
    assert state["states"][0]["step_idx"] == 7 and state["states"][0]["m"].any() and "w" not in state["states"][0]
    resumed = train_model(root, cfg_overrides=dict(over, resume=True), vit_state=vit_state, progress=False)
    assert resumed.step_idx == whole.step_idx == 11 and whole.m.any()
    for name in ("params", "m", "v", "running"):
        assert _bits(getattr(resumed, name), getattr(whole, name)), name
    assert open(os.path.join(root, "out", "output.png"), "rb").read() == open(tmp_path / "whole" / "out" / "output.png", "rb").read()
    with pytest.raises(ValueError, match="another 'optimizer_momentum'"):
        train_model(root, cfg_overrides=dict(over, resume=True, optimizer_momentum=0.5), vit_state=vit_state, progress=False)


def test_train_model_adamw_and_its_result_fields(tmp_path, monkeypatch):
    """``optimizer: adamw`` end to end through the batch runner of one pair: result.json carries the optimiser and the options set."""
    from splice_amd import batch
    monkeypatch.setenv("SPLICE_SYNTHETIC_WEIGHTS", "1")
    _write_pair(tmp_path, "p0", 64)
    over = dict(TRAIN, n_epochs=6, log_images_freq=3, optimizer="adamw", optimizer_weight_decay=0.01, optimizer_amsgrad=True)
    res = batch.train_runner(str(tmp_path / "p0"), over)
    batch._write_result(str(tmp_path), "p0", res)
    with open(tmp_path / "p0" / "out" / "result.json") as f:
        got = json.load(f)
    assert got["optimizer"] == "adamw" and got["optimizer_weight_decay"] == 0.01 and got["optimizer_amsgrad"] is True
    assert "optimizer_momentum" not in got and "optimizer_centered" not in got and got["steps"] == 6 and np.isfinite(got["loss"])
    assert (tmp_path / "p0" / "out" / "output.png").exists()
