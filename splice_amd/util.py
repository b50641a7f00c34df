"""Drop-in for ``util/util.py``: optimizer / scheduler factories (host-side torch.optim objects
over the generator's arena-backed parameters), ``tensor2im``, ``save_result``."""
from pathlib import Path

import math
import os
import numpy as np
import torch
from torch.optim import lr_scheduler


# ---- scheduler / optimizer factories -------------------------------------------------------------------------------------
# One entry per policy the reference's config accepts (util/util.py:8-39).  Each builder gets the optimizer and the keyword
# arguments of get_scheduler and returns a torch.optim.lr_scheduler object with the reference's hyper-parameters.
def _linear_decay(opt, n_epochs_decay=None, **_):
    span = float(n_epochs_decay + 1)
    return lr_scheduler.LambdaLR(opt, lr_lambda=lambda epoch: max(1.0 - max(0, epoch) / span, 0))


_SCHEDULERS = {
    'linear': _linear_decay,
    'step': lambda opt, lr_decay_iters=None, **_: lr_scheduler.StepLR(opt, step_size=lr_decay_iters, gamma=0.5),
    'plateau': lambda opt, **_: lr_scheduler.ReduceLROnPlateau(opt, mode='min', factor=0.2, threshold=0.01, patience=5),
    'cosine': lambda opt, n_epochs=None, **_: lr_scheduler.CosineAnnealingLR(opt, T_max=n_epochs, eta_min=0),
    'none': lambda opt, **_: lr_scheduler.LambdaLR(opt, lr_lambda=lambda _epoch: 1),
}
# The optimiser options beyond the reference's three constructor calls (extensions), every one at torch.optim's
# neutral value by default; which optimiser takes which key: OPTIM_EXT_TAKES.
OPTIM_EXT_DEFAULTS = dict(optimizer_weight_decay=0.0, optimizer_momentum=0.0, optimizer_dampening=0.0, optimizer_nesterov=False,
                          optimizer_amsgrad=False, optimizer_centered=False)
OPTIM_EXT_TAKES = {
    'adam': ('optimizer_weight_decay', 'optimizer_amsgrad'),
    'adamw': ('optimizer_weight_decay', 'optimizer_amsgrad'),
    'rmsprop': ('optimizer_weight_decay', 'optimizer_momentum', 'optimizer_centered'),
    'sgd': ('optimizer_weight_decay', 'optimizer_momentum', 'optimizer_dampening', 'optimizer_nesterov'),
}


def optimizer_options(cfg):
    """The optimiser options of config ``cfg`` (the OPTIM_EXT_DEFAULTS keys, an absent key standing for its default), checked on the
    host as torch.optim checks its arguments: ``optimizer_weight_decay`` and ``optimizer_momentum`` finite and >= 0,
    ``optimizer_dampening`` finite, the three flags bools, ``optimizer_nesterov`` only with momentum > 0 and dampening == 0, and no key
    at a non-default value for an optimiser that has no such argument.  Returns ``{key: value}``; raises ValueError naming the key
    (an unknown optimiser is left to ``fused_optimizer`` / ``get_optimizer``)."""
    opts = {}
    for key, default in OPTIM_EXT_DEFAULTS.items():
        v = cfg.get(key, default)
        if isinstance(default, bool):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"'{key}' must be true or false, got {v!r}")
            v = bool(v)
        else:
            if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
                raise ValueError(f"'{key}' must be a finite number, got {v!r}")
            if key != 'optimizer_dampening' and v < 0:
                raise ValueError(f"'{key}' must be >= 0, got {v!r}")
            v = float(v)
        opts[key] = v
    name = cfg.get('optimizer', 'adam')
    takes = OPTIM_EXT_TAKES.get(name)
    if takes is not None:
        for key, v in opts.items():
            if key not in takes and v != OPTIM_EXT_DEFAULTS[key]:
                hint = " ('optimizer_beta1' is its momentum)" if key == 'optimizer_momentum' and name in ('adam', 'adamw') else ""
                raise ValueError(f"'{key}' = {v!r}: optimizer [{name}] has no such argument{hint}")
    if opts['optimizer_nesterov'] and (opts['optimizer_momentum'] <= 0 or opts['optimizer_dampening'] != 0):
        raise ValueError("'optimizer_nesterov' needs 'optimizer_momentum' > 0 and 'optimizer_dampening' == 0")
    return opts


def _torch_options(cfg):
    """The torch.optim keyword arguments of ``optimizer_options(cfg)`` for the config's optimiser."""
    names = dict(optimizer_weight_decay='weight_decay', optimizer_momentum='momentum', optimizer_dampening='dampening',
                 optimizer_nesterov='nesterov', optimizer_amsgrad='amsgrad', optimizer_centered='centered')
    opts = optimizer_options(cfg)
    return {names[k]: opts[k] for k in OPTIM_EXT_TAKES[cfg['optimizer']]}


_OPTIMIZERS = {
    'adam': lambda cfg, params: torch.optim.Adam(params, lr=cfg['lr'], betas=(cfg['optimizer_beta1'], cfg['optimizer_beta2']), **_torch_options(cfg)),
    'adamw': lambda cfg, params: torch.optim.AdamW(params, lr=cfg['lr'], betas=(cfg['optimizer_beta1'], cfg['optimizer_beta2']), **_torch_options(cfg)),
    'rmsprop': lambda cfg, params: torch.optim.RMSprop(params, lr=cfg['lr'], **_torch_options(cfg)),
    'sgd': lambda cfg, params: torch.optim.SGD(params, lr=cfg['lr'], **_torch_options(cfg)),
}


def get_scheduler(optimizer, lr_policy, n_epochs=None, n_epochs_decay=None, lr_decay_iters=None):
    """``util/util.py:8-25``.  An unknown policy RETURNS (does not raise) a NotImplementedError, as the reference does."""
    build = _SCHEDULERS.get(lr_policy)
    if build is None:
        return NotImplementedError('learning rate policy [%s] is not implemented', lr_policy)
    return build(optimizer, n_epochs=n_epochs, n_epochs_decay=n_epochs_decay, lr_decay_iters=lr_decay_iters)


def get_optimizer(cfg, params):
    """``util/util.py:28-39``; same return-the-exception convention for unknown names."""
    build = _OPTIMIZERS.get(cfg['optimizer'])
    if build is None:
        return NotImplementedError('optimizer [%s] is not implemented', cfg['optimizer'])
    return build(cfg, params)


# ---- the same on the host for the fused engines -----------------------------------------------------------------------
# The reference's loop (train.py:79-80) calls optimizer.step() and then scheduler.step() once per step: step k (0-based) runs with
# the lr the scheduler holds after k calls.  LrSchedule restates torch's recurrences in Python floats, with the arithmetic of the
# torch.optim.lr_scheduler classes above in the same order (CosineAnnealingLR and StepLR are chainable recurrences, not closed
# forms), so every value equals torch's float for float; a sequential lr() call costs about a microsecond.
class LrSchedule:
    """``lr(k)``: learning rate of optimisation step ``k`` (0-based) under the config's ``scheduler_policy`` with ``lr``,
    ``n_epochs``, ``scheduler_n_epochs_decay`` and ``scheduler_lr_decay_iters`` (the arguments train.py passes to get_scheduler).
    Policies: none, linear, step, cosine.  ``plateau`` is refused: the reference calls ``scheduler.step()`` without a metric
    (train.py:80), which ReduceLROnPlateau rejects, and a plateau rule would need the loss on the host every step -- the rule that is
    decided on the device instead is the config key ``lr_plateau_factor`` (``engine.lr_plateau_rule``)."""

    POLICIES = ("none", "linear", "step", "cosine")

    def __init__(self, cfg):
        self.policy = cfg.get("scheduler_policy", "none")
        if self.policy == "plateau":
            raise NotImplementedError("scheduler_policy 'plateau' is not supported: the reference's loop calls scheduler.step() with no metric "
                                      "(train.py:80), which ReduceLROnPlateau rejects, and a plateau rule would need the loss on the host every step; "
                                      "the rule decided on the device is 'lr_plateau_factor' (with 'stop_window' > 0)")
        if self.policy not in self.POLICIES:
            raise NotImplementedError(f"learning rate policy [{self.policy}] is not implemented")
        self.base_lr = cfg["lr"]
        if self.policy == "linear":
            self.span = float(cfg["scheduler_n_epochs_decay"] + 1)
        elif self.policy == "step":
            self.step_size = cfg["scheduler_lr_decay_iters"]
            if self.step_size is None or self.step_size < 1:
                raise ValueError("scheduler_policy 'step' needs scheduler_lr_decay_iters >= 1")
        elif self.policy == "cosine":
            self.T_max, self.eta_min = cfg["n_epochs"], 0
            if self.T_max is None or self.T_max < 1:
                raise ValueError("scheduler_policy 'cosine' needs n_epochs >= 1")
        self._k, self._lr = 0, self.base_lr   # recurrence state: lr after _k scheduler steps

    def lr(self, k):
        if self.policy == "none":      # LambdaLR(lambda _: 1)
            return self.base_lr * 1
        if self.policy == "linear":    # LambdaLR, closed form
            return self.base_lr * max(1.0 - max(0, k) / self.span, 0)
        if k < self._k:
            self._k, self._lr = 0, self.base_lr
        while self._k < k:
            self._k += 1
            self._lr = self._next(self._k, self._lr)
        return self._lr

    def _next(self, e, lr):
        """The lr after the e-th scheduler step from ``lr`` (torch's get_lr with last_epoch = e)."""
        if self.policy == "step":      # StepLR(step_size=lr_decay_iters, gamma=0.5)
            return lr if e % self.step_size != 0 else lr * 0.5
        T, eta = self.T_max, self.eta_min   # CosineAnnealingLR(T_max=n_epochs, eta_min=0)
        if (e - 1 - T) % (2 * T) == 0:
            return lr + (self.base_lr - eta) * (1 - math.cos(math.pi / T)) / 2
        return (1 + math.cos(math.pi * e / T)) / (1 + math.cos(math.pi * (e - 1) / T)) * (lr - eta) + eta


def fused_optimizer(cfg):
    """``(kind, hp0, hp1, eps)`` of the config's ``optimizer`` for the fused update (splice_optim_step): the torch.optim
    arguments get_optimizer uses, every other one at torch's default."""
    name = cfg.get("optimizer", "adam")
    if name in ("adam", "adamw"):   # (adamw: Adam's kind, the decoupled flag of fused_optimizer_ext)
        return 0, cfg["optimizer_beta1"], cfg["optimizer_beta2"], 1e-8
    if name == "rmsprop":
        return 1, 0.99, 0.0, 1e-8
    if name == "sgd":
        return 2, 0.0, 0.0, 0.0
    raise NotImplementedError(f"optimizer [{name}] is not implemented")


OPTIM_EXT_FIELDS = ("weight_decay", "momentum", "dampening", "nesterov", "decoupled", "amsgrad", "centered")   # splice_optim_ext
OPTIM_EXT_NEUTRAL = dict(weight_decay=0.0, momentum=0.0, dampening=0.0, nesterov=False, decoupled=False, amsgrad=False, centered=False)


def fused_optimizer_ext(cfg):
    """The option record of the fused update's extended rules (``splice_optim_ext``) for config ``cfg``, as a
    dict of OPTIM_EXT_FIELDS -- or None when every option is neutral: the engine then launches the plain rules, exactly what it
    launched before the options existed.  ``adamw`` is Adam with ``decoupled`` set; with ``optimizer_weight_decay`` 0 it is Adam,
    bit for bit, and counts as neutral.  Checked by ``optimizer_options`` (ValueError naming the key)."""
    o = optimizer_options(cfg)
    ext = dict(weight_decay=o["optimizer_weight_decay"], momentum=o["optimizer_momentum"], dampening=o["optimizer_dampening"],
               nesterov=o["optimizer_nesterov"], decoupled=cfg.get("optimizer", "adam") == "adamw" and o["optimizer_weight_decay"] > 0,
               amsgrad=o["optimizer_amsgrad"], centered=o["optimizer_centered"])
    return None if ext == OPTIM_EXT_NEUTRAL else ext


def optim_ext_uses(kind, ext):
    """``(m, v, w)``: which moment arenas the rule of ``kind`` keeps under the options ``ext`` (None: the plain rule).  ``w`` holds
    Adam's ``max_exp_avg_sq`` (amsgrad) or RMSprop's ``grad_avg`` (centered); ``m`` also the momentum buffer of SGD and RMSprop."""
    e = ext or OPTIM_EXT_NEUTRAL
    mom = e["momentum"] > 0
    return (kind == 0 or mom, kind in (0, 1), (kind == 0 and bool(e["amsgrad"])) or (kind == 1 and bool(e["centered"])))


def np_optim_step(kind, p, g, m, v, w, lr, hp0, hp1, eps, t, ext=None, dtype=np.float32):
    """One update of the fused optimiser's rules (include/splice_hip.h) restated in NumPy at ``dtype``, one
    rounding per operation in the kernel's association: kind 0 Adam / AdamW (hp0, hp1 = betas), 1 RMSprop (hp0 = alpha), 2 SGD.
    ``g``: the gradient the rule sees (the sum of the two arenas, times the clip coefficient under clipping); ``t``: the update's
    step count (>= 1); ``ext``: the options (a dict of OPTIM_EXT_FIELDS; None: neutral); ``m`` / ``v`` / ``w``: the moment arenas
    (None where the rule keeps none, see ``optim_ext_uses``).  Returns the new ``(p, m, v, w)``; the arguments are not written."""
    f = np.dtype(dtype).type
    e = dict(OPTIM_EXT_NEUTRAL, **(ext or {}))
    arr = lambda x: None if x is None else np.array(x, dtype=f)
    p, g, m, v, w = arr(p), arr(g), arr(m), arr(v), arr(w)
    lr, hp0, hp1, eps, one = f(lr), f(hp0), f(hp1), f(eps), f(1)
    wd, mu, damp = f(e["weight_decay"]), f(e["momentum"]), f(e["dampening"])
    with np.errstate(all="ignore"):
        if kind == 0 and e["decoupled"] and wd != 0:
            p = p * (one - lr * wd)
        d = g + wd * p if wd != 0 and not (kind == 0 and e["decoupled"]) else g
        if kind == 2:
            if mu > 0:
                m = d.copy() if t == 1 else mu * m + (one - damp) * d
                d = d + mu * m if e["nesterov"] else m
            p = p - lr * d
        elif kind == 1:
            v = hp0 * v + (one - hp0) * d * d
            if e["centered"]:
                w = hp0 * w + (one - hp0) * d
                avg = np.sqrt(v - w * w) + eps
            else:
                avg = np.sqrt(v) + eps
            if mu > 0:
                m = mu * m + d / avg
                p = p - lr * m
            else:
                p = p - lr * (d / avg)
        elif kind == 0:
            bc1 = one - hp0 ** f(t)
            bc2_sqrt = np.sqrt(one - hp1 ** f(t))
            m = hp0 * m + (one - hp0) * d
            v = hp1 * v + (one - hp1) * d * d
            if e["amsgrad"]:
                w = np.maximum(w, v)
                denom = np.sqrt(w) / bc2_sqrt + eps
            else:
                denom = np.sqrt(v) / bc2_sqrt + eps
            p = p - (lr / bc1) * (m / denom)
        else:
            raise ValueError(f"np_optim_step: unknown optimiser kind {kind}")
    return p, m, v, w


def write_loss_trace(path, rows, lrs, active, clip):
    """``losses.csv`` of one slot's loss trace (``engine.loss_trace``): ``rows`` float32 ``[n, 8]``, ``lrs`` the n learning rates,
    ``active`` per row the dict of ``engine.active_terms`` (an inactive term is an empty field), ``clip``: the run clipped its gradient
    (the columns ``grad_norm,clip_coef`` exist).  Floats are written with ``%.9g``: every float32, denormals included, parses back to
    its bits.  The file appears whole (written beside, then renamed)."""
    from .engine import LOSS_KEYS
    rows = np.asarray(rows, dtype=np.float32).reshape(-1, 8)
    lines = ["step,lr," + ",".join(LOSS_KEYS) + (",grad_norm,clip_coef" if clip else "")]
    for s, (row, lr, act) in enumerate(zip(rows, lrs, active)):
        fields = [str(s), "%.9g" % lr] + ["%.9g" % row[i] if act[k] else "" for i, k in enumerate(LOSS_KEYS)]
        if clip:
            fields += ["%.9g" % row[6], "%.9g" % row[7]]
        lines.append(",".join(fields))
    path = Path(path)
    path.parent.mkdir(exist_ok=True, parents=True)
    tmp = path.with_name(path.name + ".tmp")
    tmp.write_text("\n".join(lines) + "\n")
    tmp.replace(path)


def _to_uint8_hwc(chw):
    """[3,H,W] float tensor in (roughly) [0,1] -> HxWx3 array scaled to 0..255 (still float)."""
    return chw.detach().clamp(0.0, 1.0).cpu().float().numpy().transpose(1, 2, 0) * 255.0


def tensor2im(input_image, imtype=np.uint8):
    """``util/util.py:42-52``: first image of a batch tensor -> HxWx3 array of ``imtype``; arrays are only cast, anything
    that is neither a tensor nor an array is handed back untouched."""
    if isinstance(input_image, np.ndarray):
        return input_image.astype(imtype)
    if not isinstance(input_image, torch.Tensor):
        return input_image
    return _to_uint8_hwc(input_image[0]).astype(imtype)


def save_result(image_t, dataroot):
    """``util/util.py:55-59``: writes ``<dataroot>/out/output.png`` (ToPILImage semantics: [3,H,W] float in [0,1] -> uint8)."""
    from PIL import Image
    arr = _to_uint8_hwc(image_t).astype(np.uint8)
    path = Path(f"{dataroot}/out")
    path.mkdir(exist_ok=True, parents=True)
    Image.fromarray(arr).save(f"{path}/output.png")


class AsyncResultWriter:
    """``save_result`` off the critical path.

    The reference's ``train.py:70-76`` stalls the loop every ``log_images_freq`` steps on a device->host copy plus
    a PNG encode.  ``submit`` only enqueues an asynchronous copy into a pinned host buffer on the current stream and
    an event; a worker thread waits for the event, converts (ToPILImage semantics) and writes
    ``<dataroot>/out/output.png``.  At most one image is in flight per slot (two slots): a newer result simply
    overwrites the file later, as the reference does.  ``close()`` drains the queue (called at the end of
    ``train_model`` so the final PNG is on disk when it returns)."""

    def __init__(self, dataroot, slots=2, out_dir=None):
        """``out_dir``: where output.png goes (default ``<dataroot>/out``; a sweep writes ``<dataroot>/out/sweep/<k>``)."""
        import queue
        import threading
        self.dir = Path(out_dir) if out_dir is not None else Path(f"{dataroot}/out")
        self.dir.mkdir(exist_ok=True, parents=True)
        self._q = queue.Queue()
        self._free = queue.Queue()
        for _ in range(slots):
            self._free.put(None)
        self._err = None
        # Round 5: out/output.png is OVERWRITTEN by every logged image (util/util.py:55-59 called from train.py:75), so only the latest one matters to a
        # reader.  At ~270 steps/s a logged image every 10 steps is 27 PNG encodes per second on a thread that shares the GIL with the launch loop
        # (measured: 8.1 -> 7.6 s per 2000-step pair without them).  Intermediate images closer than min_interval seconds are skipped; the caller forces the
        # last one.  SPLICE_LOG_MIN_INTERVAL=0 writes every logged image.
        self.min_interval = float(os.environ.get("SPLICE_LOG_MIN_INTERVAL", "0.25"))
        # (_last is written by the submitting thread only, _gap by the writer thread only and read by submit(): single float stores, atomic under the
        # interpreter lock; a stale _gap only moves ONE skip decision.  A run killed mid-training leaves a file at most max(min_interval, _gap) old.)
        self._last = -1e9
        self._gap = 0.0         # 10 x the duration of the last convert + encode + write (a 1200 x 900 image takes ~60 ms: the writer thread stays under 10 % duty)
        self.skipped = 0
        self._t = threading.Thread(target=self._run, name="splice-result-writer", daemon=True)
        self._t.start()

    def submit(self, image_t, force=True, name="output.png"):
        """force=False: the image may be skipped when the previous one was submitted less than ``min_interval`` seconds ago (the file is
        overwritten every time anyway; the encoder thread shares the interpreter lock with the loop that launches the steps).
        ``name``: the file in the writer's directory (``output_ema.png``: the image of the averaged weights at the end of a run)."""
        import time
        now = time.monotonic()
        if not force and now - self._last < max(self.min_interval, self._gap):
            self.skipped += 1
            return
        self._last = now
        buf = self._free.get()                      # blocks only if `slots` images are still being written
        img = image_t.detach()
        if buf is None or buf.shape != img.shape:
            buf = torch.empty(img.shape, dtype=torch.float32, pin_memory=img.is_cuda)
        buf.copy_(img, non_blocking=True)
        ev = None
        if img.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
        self._q.put((buf, ev, name))

    def _run(self):
        from PIL import Image
        while True:
            item = self._q.get()
            if item is None:
                return
            buf, ev, name = item
            try:
                if ev is not None:
                    ev.synchronize()
                import time
                t0 = time.monotonic()
                arr = (buf.clamp(0.0, 1.0).numpy().transpose(1, 2, 0) * 255.0).astype(np.uint8)
                tmp = self.dir / (name + ".tmp")
                Image.fromarray(arr).save(tmp, format="PNG")
                tmp.replace(self.dir / name)              # readers never see a half-written file
                if self.min_interval > 0:
                    self._gap = 10.0 * (time.monotonic() - t0)
            except Exception as e:                         # surfaced by close()
                self._err = e
            self._free.put(buf)

    def close(self):
        self._q.put(None)
        self._t.join()
        if self._err is not None:
            raise self._err
