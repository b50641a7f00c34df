"""Host side of the generator engine (C ABI ``splice_gen_*``): flat parameter arena in the
reference's ``netG.parameters()`` order, per-shape plans, forward / backward / Adam.
"""
import ctypes as C
from collections import OrderedDict

import torch

from . import _lib


DEFAULT_ARCH = dict(num_input_channels=3, num_output_channels=3, num_channels_down=[16, 32, 64, 128, 128], num_channels_up=[16, 32, 64, 128, 128],
                    num_channels_skip=[4, 4, 4, 4, 4], filter_size_down=[3] * 5, filter_size_up=[3] * 5, filter_skip_size=1, pad='zero')


def arch_param_specs(arch):
    """(name, shape, kind) of every parameter of a ``skip()`` net in ``parameters()`` order with the reference's state_dict
    names (models/unet/skip.py:46-99 + the ``add`` numbering of models/unet/common.py:6-9): kind in conv_w / conv_b / bn_w / bn_b."""
    down, up, skipc = arch["num_channels_down"], arch["num_channels_up"], arch["num_channels_skip"]
    kd, ku, ks = arch["filter_size_down"], arch["filter_size_up"], arch["filter_skip_size"]
    cv = ".1" if arch["pad"] == "reflection" else ".0"      # Conv2d sits behind a ReflectionPad2d inside its Sequential
    n, specs = len(down), []

    def conv(name, cout, cin, k):
        specs.append((name + ".weight", (cout, cin, k, k), "conv_w"))
        specs.append((name + ".bias", (cout,), "conv_b"))

    def bn(name, c):
        specs.append((name + ".weight", (c,), "bn_w"))
        specs.append((name + ".bias", (c,), "bn_b"))

    def scale(i, cin, p):
        conv(p + "1.0.1" + cv, skipc[i], cin, ks); bn(p + "1.0.2", skipc[i])
        conv(p + "1.1.1" + cv, down[i], cin, kd[i]); bn(p + "1.1.2", down[i])
        conv(p + "1.1.4" + cv, down[i], down[i], kd[i]); bn(p + "1.1.5", down[i])
        k = down[i]
        if i < n - 1:
            scale(i + 1, down[i], p + "1.1.7.")
            k = up[i + 1]
        bn(p + "2", skipc[i] + k)
        conv(p + "3" + cv, up[i], skipc[i] + k, ku[i]); bn(p + "4", up[i])
        conv(p + "6" + cv, up[i], up[i], 1); bn(p + "7", up[i])

    scale(0, arch["num_input_channels"], "")
    conv("9" + cv, arch["num_output_channels"], up[0], 1)
    return specs


class GeneratorEngine:
    def __init__(self, device="cuda", arch=None):
        """``arch`` = None: the default ``skip()`` of ``define_G``; else a dict of ``skip()`` keyword arguments (lists per
        scale for channels and filter sizes, ``pad`` 'zero' | 'reflection'), e.g. the feature-inversion net."""
        self.device = torch.device(device)
        self.arch = dict(DEFAULT_ARCH if arch is None else arch)
        h = C.c_void_p()
        if arch is None:
            _lib.check(_lib.lib().splice_gen_create(C.byref(h)), "gen_create")
        else:
            a = _lib.GenArch()
            n = len(self.arch["num_channels_down"])
            if n > 6:
                raise NotImplementedError("the HIP generator covers up to 6 scales")
            a.n_scales, a.in_channels, a.out_channels = n, self.arch["num_input_channels"], self.arch["num_output_channels"]
            for i in range(n):
                a.down[i], a.up[i], a.skip[i] = self.arch["num_channels_down"][i], self.arch["num_channels_up"][i], self.arch["num_channels_skip"][i]
                a.filter_down[i], a.filter_up[i] = self.arch["filter_size_down"][i], self.arch["filter_size_up"][i]
            a.filter_skip, a.reflect = self.arch["filter_skip_size"], int(self.arch["pad"] == "reflection")
            _lib.check(_lib.lib().splice_gen_create_arch(C.byref(a), C.byref(h)), "gen_create_arch")
        self.handle = h
        self.in_channels, self.out_channels = self.arch["num_input_channels"], self.arch["num_output_channels"]
        L = _lib.lib()
        self.numel = L.splice_gen_param_count(h)
        self.table = OrderedDict()
        for i in range(L.splice_gen_num_tensors(h)):
            name, off, n = C.c_char_p(), C.c_longlong(), C.c_longlong()
            _lib.check(L.splice_gen_tensor_info(h, i, C.byref(name), C.byref(off), C.byref(n)))
            self.table[name.value.decode()] = (off.value, n.value)
        self.param_specs = arch_param_specs(self.arch)
        if [(n_, int(torch.Size(sh).numel())) for n_, sh, _ in self.param_specs] != [(n_, cnt) for n_, (_, cnt) in self.table.items()]:
            raise RuntimeError("generator engine: the parameter table of the library and arch_param_specs disagree")
        # BatchNorm buffers of netG.state_dict(): "<bn>.running_mean" / "<bn>.running_var" -> (offset, numel) in the buffer arena
        self.buffer_numel = L.splice_gen_buffer_count(h)
        self.buffer_table = OrderedDict()
        for i in range(L.splice_gen_num_buffers(h)):
            name, off, n = C.c_char_p(), C.c_longlong(), C.c_longlong()
            _lib.check(L.splice_gen_buffer_info(h, i, C.byref(name), C.byref(off), C.byref(n)))
            self.buffer_table[name.value.decode()] = (off.value, n.value)
        self._plans = {}

    def __del__(self):
        try:
            self._plans.clear()
            if getattr(self, "handle", None):
                _lib.lib().splice_gen_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def flatten(self, state):
        """name -> array/tensor mapping (reference state_dict names) -> flat fp32 arena on the device."""
        flat = torch.zeros(self.numel, device=self.device)
        for name, (off, n) in self.table.items():
            t = torch.as_tensor(state[name]).to(self.device, torch.float32).reshape(-1)
            assert t.numel() == n, (name, t.numel(), n)
            flat[off:off + n] = t
        return flat

    def unflatten(self, flat, shapes=None):
        out = OrderedDict()
        for name, (off, n) in self.table.items():
            v = flat[off:off + n]
            out[name] = v.view(shapes[name]) if shapes else v
        return out

    def plan(self, N, H, W, need_grad=True):
        key = (N, H, W, bool(need_grad))
        if key not in self._plans:
            self._plans[key] = GeneratorPlan(self, N, H, W, need_grad)
        return self._plans[key]


class GeneratorPlan:
    def __init__(self, engine, N, H, W, need_grad, arena_stride=0, batch_stats=False, groups=0):
        """``arena_stride`` > 0: the N images are INDEPENDENT generators -- image n uses ``params[n * stride:]`` and its
        gradient goes to ``grads[n * stride:]`` (several pairs in one launch); 0: one generator applied to N images.
        ``groups`` = g > 0 (``splice_gen_plan_set_groups``): images ``[k*g, (k+1)*g)`` are ONE netG call -- BatchNorm statistics
        over those g images, parameters / gradients in arena k (several pairs with n_crops > 1 crops each)."""
        self.engine, self.N, self.H, self.W, self.need_grad, self.arena_stride = engine, N, H, W, need_grad, arena_stride
        h = C.c_void_p()
        _lib.check(_lib.lib().splice_gen_plan_create(engine.handle, N, H, W, int(need_grad), C.byref(h)), "gen_plan_create")
        self.handle = h
        if arena_stride:
            _lib.check(_lib.lib().splice_gen_plan_set_arena_stride(h, arena_stride), "gen_plan_set_arena_stride")
        self.batch_stats = bool(batch_stats)
        if batch_stats:   # ONE netG call on the batch: BatchNorm statistics over all N images (the reference with n_crops > 1)
            _lib.check(_lib.lib().splice_gen_plan_set_batch_stats(h, 1), "gen_plan_set_batch_stats")
        self.groups = int(groups)
        if groups:
            _lib.check(_lib.lib().splice_gen_plan_set_groups(h, int(groups)), "gen_plan_set_groups")
            self.batch_stats = groups > 1

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().splice_gen_plan_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def forward(self, params, x):
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and tuple(x.shape) == (self.N, self.engine.in_channels, self.H, self.W)
        y = torch.empty(self.N, self.engine.out_channels, self.H, self.W, device=x.device)
        _lib.check(_lib.lib().splice_gen_forward(self.handle, _lib.ptr(params), _lib.ptr(x), _lib.ptr(y), _lib.current_stream()), "gen_forward")
        return y

    def backward(self, params, dy, grads=None, accumulate=False):
        assert dy.is_cuda and dy.dtype == torch.float32 and dy.is_contiguous() and tuple(dy.shape) == (self.N, self.engine.out_channels, self.H, self.W)
        if grads is None:
            arenas = self.N // self.groups if self.groups else self.N
            grads = torch.zeros(arenas * self.arena_stride if self.arena_stride else self.engine.numel, device=self.engine.device)
        _lib.check(_lib.lib().splice_gen_backward(self.handle, _lib.ptr(params), _lib.ptr(dy), _lib.ptr(grads), int(accumulate),
                                                  _lib.current_stream()), "gen_backward")
        return grads


def adam_step(params, grads, m, v, lr, beta1, beta2, eps, step, zero_grad=False):
    _lib.check(_lib.lib().splice_adam_step(_lib.ptr(params), _lib.ptr(grads), _lib.ptr(m), _lib.ptr(v), params.numel(), lr, beta1, beta2,
                                           eps, step, int(zero_grad), _lib.current_stream()), "adam_step")


OPTIMIZER_KINDS = {"adam": 0, "rmsprop": 1, "sgd": 2}   # the `kind` of splice_optim_step


def optim_step(kind, params, grads, m, v, lr, hp0, hp1, eps, step, zero_grad=False, g2=None, lr_dev=None, ema=None, ema_decay=0.0, ema_start=0,
               clip_norm=0.0, clip_state=None, clip_auto=None, clip_regime=0, clip_auto_state=None, ext=None, w=None):
    """One fused optimiser step over a flat arena (``splice_optim_step_ex``): kind 0 Adam (hp0 / hp1 = betas, step >= 1),
    1 RMSprop (hp0 = alpha, ``v`` = square_avg, ``m`` unused), 2 SGD (``m`` / ``v`` unused).  ``g2``: second gradient arena
    added to ``grads`` first; ``lr_dev``: one-element device tensor read as the learning rate when the kernel runs.
    ``ema``: the weight-average arena, written in the same walk (``splice_optim_step_ema``): ``step <= ema_start``: a copy of the
    parameters just written, later ``ema_decay * ema + (1 - ema_decay) * params``; every kind then needs ``step >= 1``.
    ``clip_norm > 0``: the gradient (``grads + g2``) is clipped to that global norm first, as ``torch.nn.utils.clip_grad_norm_``, and an
    update whose norm is not finite is skipped (``splice_grad_norm_pairs`` then ``splice_optim_step_clip``); ``clip_state``: the int32
    CUDA tensor of 6 elements that receives the ``splice_clip_state`` record (its two counts are the caller's to start at zero).
    ``clip_auto = (k, beta, warmup)``: the threshold is ``k`` times the running norm of the step's regime ``clip_regime`` (-1, 0 or 1)
    kept in ``clip_auto_state``, an int32 CUDA tensor of 6 elements like ``clip_state`` (zeros at the start of a run), under the cap
    ``clip_norm`` where that is > 0 (``splice_grad_norm_pairs_auto``).
    ``ext``: the options of the extended rules (``util.fused_optimizer_ext``: a dict of the ``splice_optim_ext`` fields, or the
    record itself) -- an explicit ``ext`` ALWAYS takes the extended kernels, also when its options are neutral (they then compute the
    plain rules' bits); every kind then needs ``step >= 1``.  ``m`` also holds the momentum buffer of SGD / RMSprop, and ``w`` is the
    third moment arena: Adam's ``max_exp_avg_sq`` under amsgrad, RMSprop's ``grad_avg`` when centered (``splice_optim_step_pairs_ext``)."""
    if kind not in OPTIMIZER_KINDS.values():
        raise ValueError(f"optim_step: unknown optimiser kind {kind}")
    rec = None if ext is None else _lib.optim_ext(ext)
    mom = rec is not None and kind != 0 and rec.momentum > 0
    needs_w = rec is not None and bool(rec.amsgrad if kind == 0 else rec.centered if kind == 1 else False)
    m = m if kind == 0 or mom else None     # arenas the rule does not touch are not passed
    v = v if kind in (0, 1) else None
    w = w if needs_w else None
    n = params.numel()
    for name, t, needed in (("params", params, True), ("grads", grads, True), ("g2", g2, False), ("m", m, kind == 0 or mom), ("v", v, kind in (0, 1)),
                            ("ema", ema, False), ("w", w, needs_w)):
        if t is None and not needed:
            continue
        if t is None or not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
            raise ValueError(f"optim_step: {name} must be a contiguous fp32 CUDA tensor of {n} elements")
    if lr_dev is not None and not (lr_dev.is_cuda and lr_dev.dtype == torch.float32 and lr_dev.numel() >= 1):
        raise ValueError("optim_step: lr_dev must be a fp32 CUDA tensor")
    if clip_norm or clip_auto is not None:
        if clip_state is None or not (clip_state.is_cuda and clip_state.dtype == torch.int32 and clip_state.is_contiguous() and clip_state.numel() == 6):
            raise ValueError("optim_step: clip_state must be a contiguous int32 CUDA tensor of 6 elements")
        partials = torch.empty((n + 4095) // 4096, dtype=torch.float32, device=params.device)
        if clip_auto is not None:
            a = clip_auto_state
            if a is None or not (a.is_cuda and a.dtype == torch.int32 and a.is_contiguous() and a.numel() == 6):
                raise ValueError("optim_step: clip_auto_state must be a contiguous int32 CUDA tensor of 6 elements")
            k, beta, warmup = clip_auto
            _lib.check(_lib.lib().splice_grad_norm_pairs_auto(_lib.ptr(grads), _lib.ptr(g2), 1, 0, n, float(clip_norm), float(k), float(beta), int(warmup),
                                                              int(clip_regime), _lib.ptr(partials), _lib.ptr(clip_state), _lib.ptr(a), None, None,
                                                              _lib.current_stream()), "grad_norm_pairs_auto")
        else:
            _lib.check(_lib.lib().splice_grad_norm_pairs(_lib.ptr(grads), _lib.ptr(g2), 1, 0, n, float(clip_norm), _lib.ptr(partials), _lib.ptr(clip_state),
                                                         None, None, _lib.current_stream()), "grad_norm_pairs")
        if rec is not None:   # (one arena, the host's step count: the pairs form with its one clip record)
            lr1 = lr_dev if lr_dev is not None else torch.full((1,), float(lr), dtype=torch.float32, device=params.device)
            _lib.check(_lib.lib().splice_optim_step_pairs_ext(int(kind), _lib.ptr(params), _lib.ptr(grads), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), _lib.ptr(w),
                                                              _lib.ptr(ema), 1, 0, n, _lib.ptr(lr1), float(hp0), float(hp1), float(eps), int(step), None, None,
                                                              int(zero_grad), float(ema_decay), int(ema_start), _lib.ptr(clip_state), None, None, None,
                                                              C.byref(rec), _lib.current_stream()), "optim_step_pairs_ext")
            return
        _lib.check(_lib.lib().splice_optim_step_clip(int(kind), _lib.ptr(params), _lib.ptr(grads), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), _lib.ptr(ema), n,
                                                     float(lr), _lib.ptr(lr_dev), float(hp0), float(hp1), float(eps), int(step), int(zero_grad),
                                                     float(ema_decay), int(ema_start), _lib.ptr(clip_state), _lib.current_stream()), "optim_step_clip")
        return
    if rec is not None and ema is not None:
        lr1 = lr_dev if lr_dev is not None else torch.full((1,), float(lr), dtype=torch.float32, device=params.device)
        _lib.check(_lib.lib().splice_optim_step_pairs_ext(int(kind), _lib.ptr(params), _lib.ptr(grads), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), _lib.ptr(w),
                                                          _lib.ptr(ema), 1, 0, n, _lib.ptr(lr1), float(hp0), float(hp1), float(eps), int(step), None, None,
                                                          int(zero_grad), float(ema_decay), int(ema_start), None, None, None, None, C.byref(rec),
                                                          _lib.current_stream()), "optim_step_pairs_ext")
        return
    if rec is not None:
        _lib.check(_lib.lib().splice_optim_step_ext(int(kind), _lib.ptr(params), _lib.ptr(grads), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), _lib.ptr(w), n,
                                                    float(lr), _lib.ptr(lr_dev), float(hp0), float(hp1), float(eps), int(step), int(zero_grad), C.byref(rec),
                                                    _lib.current_stream()), "optim_step_ext")
        return
    if ema is not None:
        _lib.check(_lib.lib().splice_optim_step_ema(int(kind), _lib.ptr(params), _lib.ptr(grads), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), _lib.ptr(ema), n,
                                                    float(lr), _lib.ptr(lr_dev), float(hp0), float(hp1), float(eps), int(step), int(zero_grad),
                                                    float(ema_decay), int(ema_start), _lib.current_stream()), "optim_step_ema")
        return
    _lib.check(_lib.lib().splice_optim_step_ex(int(kind), _lib.ptr(params), _lib.ptr(grads), _lib.ptr(g2), _lib.ptr(m), _lib.ptr(v), n,
                                               float(lr), _lib.ptr(lr_dev), float(hp0), float(hp1), float(eps), int(step), int(zero_grad),
                                               _lib.current_stream()), "optim_step")
