"""The host side of the per-pair rules: what an engine reads of a config before it touches a GPU, and what the tests hold the kernels against.

In this order: the config's defaults and key groups; the checks of every rule's keys (``*_rule``: ValueError naming the key); the NumPy
restatements of the rules' arithmetic (``np_*``); the decoders of the device records; the step arithmetic.  Nothing here launches
anything: the module needs neither the generator nor the ViT engine.  ``splice_amd.engine`` hands every public name on."""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .util import LrSchedule

# ---------------------------------------------------------------------------------------------------------- config and keys
LOSS_KEYS = ["loss", "loss_global_ssim", "loss_entire_ssim", "loss_entire_cls", "loss_global_cls", "loss_global_id_B"]
# words 6 and 7 of a losses row: the image-space terms, reported exactly when their lambda is > 0
IMAGE_LOSS_KEYS = ["loss_global_tv", "loss_global_pix_id_B"]
IMAGE_LAMBDA_KEYS = ("lambda_global_tv", "lambda_global_pixel_identity")   # (the weight of IMAGE_LOSS_KEYS[i])

DEFAULT_CFG = dict(  # conf/default/config.yaml of the reference
    init_type="xavier", init_gain=0.02,
    lambda_global_cls=10.0, lambda_global_ssim=1.0, lambda_global_identity=1.0,
    entire_A_every=75, lambda_entire_cls=10, lambda_entire_ssim=1.0,
    dino_model_name="dino_vitb8", dino_global_patch_size=224,
    cls_warmup=1, n_epochs=10000, scheduler_policy="none",
    optimizer="adam", optimizer_beta1=0.0, optimizer_beta2=0.99, lr=0.002,
    log_images_freq=10,
    # extensions (absent from the reference's config): the plateau stop rule, off by default
    stop_window=0, stop_rel=0.01, stop_patience=2, stop_min_steps=0,
    # ... and the weight average kept by the fused update, off by default
    ema_decay=0.0, ema_start=0,
    # ... and clipping of every pair's gradient by its global norm inside the fused step, off by default
    grad_clip_norm=0.0,
    # ... and clipping against k times the pair's own running gradient norm, kept per regime on the device, off by default
    grad_clip_auto=0.0, grad_clip_auto_beta=0.98, grad_clip_auto_warmup=8,
    # ... and the weights of the window the stop rule judged best, kept on the device beside the live ones, off by default
    stop_keep_best=False,
    # ... and one row per step and slot of the loss values (and the gradient norm under clipping), kept on the device, off by default
    loss_trace=False,
    # ... and a cut of a slot's learning rate where the stop rule's windows stop getting better, decided in the loss kernel, off by default
    lr_plateau_factor=0.0, lr_plateau_patience=1, lr_plateau_min_scale=0.0,
    # ... and pair snapshots: stopped slots leave the launches; a run writes checkpoints and continues from one; off by default
    stop_compact=False, checkpoint_every=0, resume=False,
    # ... and torch.optim's further arguments of the config's optimiser, run by the fused update's extended rules (`optimizer`
    # also takes adamw): neutral by default -- the update is then the reference's, the very kernels it always was
    optimizer_weight_decay=0.0, optimizer_momentum=0.0, optimizer_dampening=0.0, optimizer_nesterov=False, optimizer_amsgrad=False,
    optimizer_centered=False,
    # ... and two loss terms on the generated crops themselves: total variation of G(A_crop), mse(G(B_crop), B_crop); off by default
    lambda_global_tv=0.0, lambda_global_pixel_identity=0.0,
    # ... and the ViT blocks whose keys the two structure terms compare, with a weight each; null: the top block, weight 1
    dino_ssim_layers=None, dino_ssim_layer_weights=None,
    # ... and the blocks whose [CLS] row the two appearance terms compare, with a weight each; null: the top block, weight 1
    dino_cls_layers=None, dino_cls_layer_weights=None,
    # ... and the blocks whose keys the identity term compares, with a weight each; null: the top block, weight 1
    dino_id_layers=None, dino_id_layer_weights=None,
    # ... and the key second-moment appearance term (the D x D Gram of a block's keys over its tokens): its weight and block; off by default
    lambda_global_key_gram=0.0, dino_gram_layer=None,
    # ... over a list of blocks with a weight each, and its centred (covariance) form; null / false: the one-block uncentred term
    dino_gram_layers=None, dino_gram_layer_weights=None, dino_gram_centered=False,
    # ... and the nearest-neighbour key appearance term (every key of G(A_crop) towards its most similar key of the B crop, in cosine;
    # DESIGN.md section 9p): its weight and block; off by default
    lambda_global_key_nn=0.0, dino_nn_layer=None)
# The three plain per-layer terms -- a list of blocks with a weight each and nothing else -- in the order the engine sets them (the identity
# list behind the structure list, whose key-gradient buffers it shares).  keys: the two config keys; most: entries of the term's by-value
# kernel table (SELFSIM_MAX_LAYERS / CLS_MAX_LAYERS / ID_MAX_LAYERS); attr: the engine attribute that holds the canonical (layers,
# weights) or None; setter: the C call that takes them; fp8: why the engine refuses the keys with fp8; section: of DESIGN.md.
LayerListTerm = namedtuple("LayerListTerm", "keys most attr setter fp8 section")
LAYER_LIST_TERMS = (
    LayerListTerm(("dino_ssim_layers", "dino_ssim_layer_weights"), 12, "ssim_layers", "splice_step_set_ssim_layers",
                  "the e4m3 Gram path of the structure term reads the top block alone", "9k"),
    LayerListTerm(("dino_cls_layers", "dino_cls_layer_weights"), 12, "cls_layers", "splice_step_set_cls_layers",
                  "the e4m3 forward is validated against the top block's [CLS] row alone", "9l"),
    LayerListTerm(("dino_id_layers", "dino_id_layer_weights"), 12, "id_layers", "splice_step_set_id_layers",
                  "the e4m3 forward keeps fp32 keys of the top block alone", "9m"))
SSIM_LAYER_KEYS, CLS_LAYER_KEYS, ID_LAYER_KEYS = (t.keys for t in LAYER_LIST_TERMS)
MAX_SSIM_LAYERS, MAX_CLS_LAYERS, MAX_ID_LAYERS = (t.most for t in LAYER_LIST_TERMS)
KEY_GRAM_KEYS = ("lambda_global_key_gram", "dino_gram_layer")
KEY_GRAM_LAYER_KEYS = ("dino_gram_layers", "dino_gram_layer_weights", "dino_gram_centered")
MAX_KEY_GRAM_LAYERS = 12   # KEY_GRAM_MAX_LAYERS: entries of the layered key second-moment kernels' by-value table
KEY_GRAM_LOSS_KEY = "loss_global_key_gram"   # the term's raw value in engine.losses(), on the steps it is active

KEY_NN_KEYS = ("lambda_global_key_nn", "dino_nn_layer")
KEY_NN_LOSS_KEY = "loss_global_key_nn"   # the term's raw value in engine.losses(), on the steps it is active

SNAPSHOT_FORMAT = 1
# Keys of a config that do not enter a slot's arithmetic (paths, logging, and how the loop parks and checkpoints): a snapshot is restored
# into a slot whose config equals its own on every other key.
SNAPSHOT_FREE_KEYS = ("dataroot", "log_images_freq", "stop_compact", "checkpoint_every", "resume")

# Per-slot keys of a sweep (MultiPairEngine(pair_cfgs=...), train.train_sweep): the five loss weights in the order of
# splice_step_set_pair_weights, the learning rate and its schedule, and what only the host-side generator initialisation reads.
# Every other key is shared by the slots of one engine.
PAIR_LAMBDA_KEYS = ("lambda_global_cls", "lambda_global_ssim", "lambda_global_identity", "lambda_entire_cls", "lambda_entire_ssim")
PAIR_LR_KEYS = ("lr", "scheduler_policy", "scheduler_n_epochs_decay", "scheduler_lr_decay_iters")
PAIR_INIT_KEYS = ("seed", "init_type", "init_gain")
PAIR_KEYS = PAIR_LAMBDA_KEYS + PAIR_LR_KEYS + PAIR_INIT_KEYS
MAX_PAIR_CFGS = 32   # SPLICE_STEP_MAX_PAIR_CFGS
MAX_GROUP_IMAGES = 32   # SPLICE_STEP_MAX_GROUP_IMAGES: images per side (pairs x n_crops) of several pairs with n_crops > 1

STOP_HISTORY = _lib.STOP_HISTORY   # SPLICE_STOP_HISTORY: window means kept per slot
CLIP_CHUNK = 4096   # SPLICE_CLIP_CHUNK


# ------------------------------------------------------------------------------------------------------------------- checks
def _number(c, key, kinds, ok, what):
    """``c[key]`` (absent: the default) when it is one of ``kinds``, no bool, and ``ok(value)``; else ValueError naming the key."""
    v = c.get(key, DEFAULT_CFG[key])
    if isinstance(v, bool) or not isinstance(v, kinds) or not ok(v):
        raise ValueError(f"'{key}' must be {what}, got {v!r}")
    return v


_INT, _REAL = (int, np.integer), (int, float, np.integer, np.floating)


def _integer(c, key, lo):
    return int(_number(c, key, _INT, lambda v: v >= lo, f"an integer >= {lo}"))


def stop_rule(c):
    """``(window, rel, patience, min_steps)`` of the plateau stop rule in config ``c``, checked on the host:
    ``stop_window >= 0`` (0: the rule is off), ``0 < stop_rel < 1``, ``stop_patience >= 1``, ``stop_min_steps >= 0``.  Raises
    ValueError naming the key."""
    rel = float(_number(c, "stop_rel", _REAL, lambda v: 0 < v < 1, "a number in (0, 1)"))
    return _integer(c, "stop_window", 0), rel, _integer(c, "stop_patience", 1), _integer(c, "stop_min_steps", 0)


def ema_rule(c):
    """``(decay, start)`` of the weight average in config ``c``, checked on the host: ``0 <= ema_decay < 1``
    (0: no average is kept) and an integer ``ema_start >= 0``, the number of updates the average merely copies the weights for.
    Raises ValueError naming the key."""
    return float(_number(c, "ema_decay", _REAL, lambda v: 0 <= v < 1, "a number in [0, 1)")), _integer(c, "ema_start", 0)


def grad_clip_rule(c):
    """``max_norm`` of the gradient clipping in config ``c``, checked on the host: a finite number
    ``grad_clip_norm >= 0`` (0: the gradient is not clipped).  Raises ValueError naming the key."""
    v = _number(c, "grad_clip_norm", _REAL, lambda v: 0 <= v < float("inf"), "a finite number >= 0")
    with np.errstate(over="ignore"):
        if not np.isfinite(np.float32(v)):   # (the kernels take it as a float)
            raise ValueError(f"'grad_clip_norm' must be a finite float32 number, got {v!r}")
    return float(v)


def grad_clip_auto_rule(c):
    """``(k, beta, warmup)`` of the adaptive gradient clipping in config ``c``, checked on the host:
    ``grad_clip_auto`` is 0 (off) or a finite float32 number ``k >= 1``, ``grad_clip_auto_beta`` a float32 number in ``[0, 1)`` and
    ``grad_clip_auto_warmup`` an integer >= 1 (observations per regime before that regime's threshold acts).  Raises ValueError
    naming the key."""
    k = float(_number(c, "grad_clip_auto", _REAL, lambda v: v == 0 or 1 <= v < float("inf"), "0 (off) or a finite number >= 1"))
    beta = float(_number(c, "grad_clip_auto_beta", _REAL, lambda v: 0 <= v < 1, "a number in [0, 1)"))
    with np.errstate(over="ignore"):   # (the kernel takes both as floats)
        if not np.isfinite(np.float32(k)):
            raise ValueError(f"'grad_clip_auto' must be a finite float32 number, got {k!r}")
        if not np.float32(beta) < 1:
            raise ValueError(f"'grad_clip_auto_beta' must be a float32 number in [0, 1), got {beta!r}")
    return k, beta, _integer(c, "grad_clip_auto_warmup", 1)


def best_rule(c):
    """``stop_keep_best`` of config ``c``, checked on the host: a bool, and ``True`` only with the plateau stop
    rule on (``stop_window > 0``) -- the snapshot is taken where that rule moves its ``best``.  Raises ValueError naming the key."""
    v = c.get("stop_keep_best", DEFAULT_CFG["stop_keep_best"])
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"'stop_keep_best' must be true or false, got {v!r}")
    if v and stop_rule(c)[0] == 0:
        raise ValueError("'stop_keep_best' needs the plateau stop rule: 'stop_window' > 0")
    return bool(v)


def trace_rule(c):
    """``loss_trace`` of config ``c``, checked on the host: a bool.  Raises ValueError naming the key."""
    v = c.get("loss_trace", DEFAULT_CFG["loss_trace"])
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"'loss_trace' must be true or false, got {v!r}")
    return bool(v)


def lr_plateau_rule(c):
    """``(factor, patience, min_scale)`` of the plateau lr rule in config ``c``, checked on the host:
    ``lr_plateau_factor`` 0 (the rule is off) or in (0, 1), an integer ``lr_plateau_patience >= 1`` (windows) and
    ``0 <= lr_plateau_min_scale < 1``; a factor > 0 needs the plateau stop rule (``stop_window > 0``), whose windows and ``stop_rel``
    it uses.  Raises ValueError naming the key."""
    factor = float(_number(c, "lr_plateau_factor", _REAL, lambda v: 0 <= v < 1, "0 (off) or a number in (0, 1)"))
    patience = _integer(c, "lr_plateau_patience", 1)
    min_scale = float(_number(c, "lr_plateau_min_scale", _REAL, lambda v: 0 <= v < 1, "a number in [0, 1)"))
    if factor > 0:
        if not 0 < float(np.float32(factor)) < 1:   # (the kernels take it as a float)
            raise ValueError(f"'lr_plateau_factor' must be in (0, 1) as a float32 number, got {factor!r}")
        if stop_rule(c)[0] == 0:
            raise ValueError("'lr_plateau_factor' > 0 needs the windows of the plateau stop rule: 'stop_window' > 0 "
                             "(cuts without a stop: a large 'stop_patience')")
    return factor, patience, min_scale


def compact_rule(c):
    """``stop_compact`` of config ``c``, checked on the host: a bool, and ``True`` only with the plateau stop
    rule on (``stop_window > 0``) -- only a stopped slot leaves the launches.  Raises ValueError naming the key."""
    v = c.get("stop_compact", DEFAULT_CFG["stop_compact"])
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"'stop_compact' must be true or false, got {v!r}")
    if v and stop_rule(c)[0] == 0:
        raise ValueError("'stop_compact' needs the plateau stop rule: 'stop_window' > 0")
    return bool(v)


def checkpoint_rule(c):
    """``(checkpoint_every, resume)`` of config ``c``, checked on the host: an integer >= 0 (0: no checkpoint is
    written) and a bool.  Raises ValueError naming the key."""
    v = c.get("resume", DEFAULT_CFG["resume"])
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError(f"'resume' must be true or false, got {v!r}")
    return _integer(c, "checkpoint_every", 0), bool(v)


def image_terms_rule(c):
    """``(lambda_tv, lambda_pix)`` of the image-space loss terms in config ``c``, checked on the host: finite
    numbers ``lambda_global_tv >= 0`` and ``lambda_global_pixel_identity >= 0`` (0: the term is off; both 0: the step launches what it
    launches without the keys).  Shared by the slots of a sweep (``merge_pair_cfgs`` refuses a per-slot value).  Raises ValueError
    naming the key."""
    out = []
    for key in IMAGE_LAMBDA_KEYS:
        v = _number(c, key, _REAL, lambda v: 0 <= v < float("inf"), "a finite number >= 0")
        with np.errstate(over="ignore"):
            if not np.isfinite(np.float32(v)):   # (the kernels take it as a float)
                raise ValueError(f"'{key}' must be a finite float32 number, got {v!r}")
        out.append(float(v))
    return tuple(out)


def ssim_layers_rule(c, depth):
    """The blocks of the structure terms in config ``c`` for a ViT of ``depth`` blocks, checked on the host:
    ``None`` -- both keys null: the top block with weight 1, the step launches what it launches without the keys -- or
    ``(layers, weights)``, the canonical form: the block indices ascending, each weight beside its block.  ``dino_ssim_layers`` is a list
    of 1..``depth`` distinct integers in ``[0, depth)`` (at most MAX_SSIM_LAYERS); ``dino_ssim_layer_weights`` a list of as many finite
    float32 numbers > 0 (null: all 1), refused without ``dino_ssim_layers``.  ``[depth - 1]`` with weight 1 is the default and also
    returns ``None``.  Shared by the slots of a sweep (``merge_pair_cfgs`` refuses a per-slot value).  Raises ValueError naming the
    key."""
    return layer_list_rule(LAYER_LIST_TERMS[0], c, depth)


def layer_list_rule(term, c, depth):
    """The rule of one of LAYER_LIST_TERMS (``ssim_layers_rule`` / ``cls_layers_rule`` / ``id_layers_rule`` state it) on config ``c``."""
    return _layers_rule(c, depth, term.keys, term.most)


def _layers_rule(c, depth, keys, most):
    """A (layers, weights) pair of config keys ``keys`` (``ssim_layers_rule`` / ``cls_layers_rule`` / ``id_layers_rule`` state the rule), at most ``most`` entries."""
    lk, wk = keys
    layers, weights = (c.get(k, DEFAULT_CFG[k]) for k in keys)
    if layers is None:
        if weights is not None:
            raise ValueError(f"'{wk}' needs '{lk}': a weight goes with a named block")
        return None
    if isinstance(layers, (str, bytes)) or not isinstance(layers, (list, tuple)) or not 1 <= len(layers) <= min(depth, most):
        raise ValueError(f"'{lk}' must be a list of 1..{min(depth, most)} block indices, got {layers!r}")
    for l in layers:
        if isinstance(l, bool) or not isinstance(l, _INT) or not 0 <= l < depth:
            raise ValueError(f"'{lk}' must hold integers in [0, {depth}), got {l!r}")
    layers = [int(l) for l in layers]
    if len(set(layers)) != len(layers):
        raise ValueError(f"'{lk}' must hold distinct block indices, got {layers!r}")
    if weights is None:
        weights = [1.0] * len(layers)
    if isinstance(weights, (str, bytes)) or not isinstance(weights, (list, tuple)) or len(weights) != len(layers):
        raise ValueError(f"'{wk}' must be a list of {len(layers)} numbers, one per entry of '{lk}', got {weights!r}")
    for w in weights:
        with np.errstate(over="ignore"):   # (the kernels take it as a float)
            if isinstance(w, bool) or not isinstance(w, _REAL) or not 0 < w < float("inf") or not 0 < np.float32(w) < np.float32("inf"):
                raise ValueError(f"'{wk}' must hold finite float32 numbers > 0, got {w!r}")
    order = sorted(range(len(layers)), key=layers.__getitem__)
    layers, weights = [layers[i] for i in order], [float(weights[i]) for i in order]
    if layers == [depth - 1] and weights == [1.0]:
        return None
    return layers, weights


def cls_layers_rule(c, depth):
    """The blocks of the two appearance terms in config ``c`` for a ViT of ``depth`` blocks, checked on the host:
    ``None`` -- both keys null, or ``[depth - 1]`` with weight 1: the top block, the step launches what it launches without the keys -- or
    ``(layers, weights)``, the canonical form: the block indices ascending, each weight beside its block.  ``dino_cls_layers`` is a list of
    1..``min(depth, MAX_CLS_LAYERS)`` distinct integers in ``[0, depth)``, the top block not required; ``dino_cls_layer_weights`` a list of
    as many finite float32 numbers > 0 (null: all 1), refused without ``dino_cls_layers``.  Shared by the slots of a sweep
    (``merge_pair_cfgs`` refuses a per-slot value).  Raises ValueError naming the key."""
    return layer_list_rule(LAYER_LIST_TERMS[1], c, depth)


def id_layers_rule(c, depth):
    """The blocks of the key-identity term in config ``c`` for a ViT of ``depth`` blocks, checked on the host:
    ``None`` -- both keys null, or ``[depth - 1]`` with weight 1: the top block, the step launches what it launches without the keys -- or
    ``(layers, weights)``, the canonical form: the block indices ascending, each weight beside its block.  ``dino_id_layers`` is a list of
    1..``min(depth, MAX_ID_LAYERS)`` distinct integers in ``[0, depth)``, the top block not required; ``dino_id_layer_weights`` a list of
    as many finite float32 numbers > 0 (null: all 1), refused without ``dino_id_layers``.  Shared by the slots of a sweep
    (``merge_pair_cfgs`` refuses a per-slot value).  Raises ValueError naming the key."""
    return layer_list_rule(LAYER_LIST_TERMS[2], c, depth)


def key_gram_rule(c, depth):
    """The key second-moment appearance term in config ``c`` for a ViT of ``depth`` blocks, checked on the host:
    ``None`` -- ``lambda_global_key_gram`` is 0 and ``dino_gram_layer`` null: the step launches what it launches without the keys -- or
    ``(lambda, layer)``.  ``lambda_global_key_gram`` is a finite float32 number >= 0 (0: off); ``dino_gram_layer`` one integer block
    index in ``[0, depth)`` (null: ``depth - 1``, the top block), refused while the weight is 0.  Shared by the slots of a sweep
    (``merge_pair_cfgs`` refuses a per-slot value).  Raises ValueError naming the key."""
    lk, yk = KEY_GRAM_KEYS
    lam = _number(c, lk, _REAL, lambda v: 0 <= v < float("inf"), "a finite number >= 0")
    with np.errstate(over="ignore"):
        if not np.isfinite(np.float32(lam)) or (lam > 0 and not np.float32(lam) > 0):   # (the kernels take it as a float)
            raise ValueError(f"'{lk}' must be a finite float32 number, 0 or > 0 in float32, got {lam!r}")
    layer = c.get(yk, DEFAULT_CFG[yk])
    if layer is None:
        return None if lam == 0 else (float(lam), depth - 1)
    if isinstance(layer, bool) or not isinstance(layer, _INT) or not 0 <= layer < depth:
        raise ValueError(f"'{yk}' must be one integer block index in [0, {depth}) or null, got {layer!r}")
    if lam == 0:
        raise ValueError(f"'{yk}' needs '{lk}' > 0 (the term is off), got {layer!r}")
    return float(lam), int(layer)


def key_nn_rule(c, depth):
    """The nearest-neighbour key appearance term in config ``c`` for a ViT of ``depth`` blocks, checked on the host:
    ``None`` -- ``lambda_global_key_nn`` is 0 and ``dino_nn_layer`` null: the step launches what it launches without the keys -- or
    ``(lambda, layer)``.  ``lambda_global_key_nn`` is a finite float32 number >= 0 (0: off); ``dino_nn_layer`` one integer block index in
    ``[0, depth)`` (null: ``depth - 1``, the top block), refused while the weight is 0.  Shared by the slots of a sweep
    (``merge_pair_cfgs`` refuses a per-slot value).  Raises ValueError naming the key."""
    lk, yk = KEY_NN_KEYS
    lam = _number(c, lk, _REAL, lambda v: 0 <= v < float("inf"), "a finite number >= 0")
    with np.errstate(over="ignore"):
        if not np.isfinite(np.float32(lam)) or (lam > 0 and not np.float32(lam) > 0):   # (the kernels take it as a float)
            raise ValueError(f"'{lk}' must be a finite float32 number, 0 or > 0 in float32, got {lam!r}")
    layer = c.get(yk, DEFAULT_CFG[yk])
    if layer is None:
        return None if lam == 0 else (float(lam), depth - 1)
    if isinstance(layer, bool) or not isinstance(layer, _INT) or not 0 <= layer < depth:
        raise ValueError(f"'{yk}' must be one integer block index in [0, {depth}) or null, got {layer!r}")
    if lam == 0:
        raise ValueError(f"'{yk}' needs '{lk}' > 0 (the term is off), got {layer!r}")
    return float(lam), int(layer)


def np_key_nn(kx, kb, lam, eps=1e-8, match=None):
    """The nearest-neighbour key term restated in NumPy float64: ``kx``, ``kb`` the ``[T][D]`` keys of the generated
    and of the target pass (every token, the heads concatenated).  With ``c_ij = kx_i . kb_j / max(|kx_i| |kb_j|, eps)`` and ``m(i)`` the
    lowest ``j`` among those with the largest ``c_ij`` -- or ``match`` where given: that assignment instead of the arg-max -- returns
    ``(raw, m, cos, dK)``: ``cos[i] = c_i,m(i)``, ``raw = mean(1 - cos)``, ``dK`` the gradient of ``lam * raw`` with respect to ``kx`` as
    autograd takes it through ``clamp`` and ``max``: ``dK_i = -(lam / T) (kb_m / f - [n_i n_m > eps] cos_i kx_i / n_i^2)``,
    ``f = max(n_i n_m, eps)``.  The target carries no gradient."""
    kx, kb = np.asarray(kx, np.float64), np.asarray(kb, np.float64)
    T = kx.shape[0]
    nx, nb = np.sqrt((kx * kx).sum(1)), np.sqrt((kb * kb).sum(1))
    if match is None:
        c = (kx @ kb.T) / np.maximum(np.outer(nx, nb), eps)
        m = np.argmax(c, axis=1)   # (the first occurrence: the lowest index among equals)
    else:
        m = np.asarray(match, np.int64)
    bm, nm = kb[m], nb[m]
    prod = nx * nm
    f = np.maximum(prod, eps)
    cos = (kx * bm).sum(1) / f
    with np.errstate(divide="ignore", invalid="ignore"):
        own = np.where(prod > eps, cos / np.where(nx > 0, nx * nx, 1.0), 0.0)
    dK = -(float(lam) / T) * (bm / f[:, None] - own[:, None] * kx)
    return float(np.mean(1.0 - cos)), m.astype(np.int64), cos, dK


def key_gram_layers_rule(c, depth):
    """The key second-moment term over several blocks, or centred, in config ``c`` for a ViT of ``depth`` blocks,
    checked on the host: ``None`` -- the three KEY_GRAM_LAYER_KEYS at their defaults, or a one-entry ``dino_gram_layers`` with weight 1 and
    ``dino_gram_centered`` false, which IS the one-block term of ``key_gram_rule`` (``key_gram_canonical`` spells it that way) -- or
    ``(lambda, layers, weights, centered)``, the canonical form: the block indices ascending, each weight beside its block.
    ``dino_gram_layers`` is a list of 1..``min(depth, MAX_KEY_GRAM_LAYERS)`` distinct integers in ``[0, depth)``, the top block not required,
    refused together with a non-null ``dino_gram_layer``; ``dino_gram_layer_weights`` a list of as many finite float32 numbers > 0 (null: all
    1), refused without the list; ``dino_gram_centered`` a bool: with it and no list the term runs centred on ``dino_gram_layer`` (null: the
    top block).  The list and ``dino_gram_centered: true`` are refused while ``lambda_global_key_gram`` is 0.  Shared by the slots of a
    sweep (``merge_pair_cfgs`` refuses a per-slot value).  Raises ValueError naming the key."""
    lk, wk, ck = KEY_GRAM_LAYER_KEYS
    centered = c.get(ck, DEFAULT_CFG[ck])
    if not isinstance(centered, (bool, np.bool_)):
        raise ValueError(f"'{ck}' must be true or false, got {centered!r}")
    centered = bool(centered)
    listed = c.get(lk, DEFAULT_CFG[lk]) is not None
    canon = _layers_rule(c, depth, (lk, wk), MAX_KEY_GRAM_LAYERS)   # (None for [depth - 1] with weight 1 too)
    single = c.get(KEY_GRAM_KEYS[1], DEFAULT_CFG[KEY_GRAM_KEYS[1]])
    if listed and single is not None:
        raise ValueError(f"'{lk}' and '{KEY_GRAM_KEYS[1]}' name the blocks of one term: give one of them, got {c.get(lk)!r} and {single!r}")
    base = key_gram_rule({KEY_GRAM_KEYS[0]: c.get(KEY_GRAM_KEYS[0], DEFAULT_CFG[KEY_GRAM_KEYS[0]]), KEY_GRAM_KEYS[1]: None if listed else single}, depth)
    if base is None:
        for key, on in ((lk, listed), (ck, centered)):
            if on:
                raise ValueError(f"'{key}' needs '{KEY_GRAM_KEYS[0]}' > 0 (the term is off), got {c.get(key)!r}")
        return None
    if not listed:
        return (base[0], [base[1]], [1.0], True) if centered else None
    layers, weights = canon if canon is not None else ([depth - 1], [1.0])
    if len(layers) == 1 and weights == [1.0] and not centered:
        return None
    return base[0], layers, weights, centered


def key_gram_canonical(c, depth):
    """The values of KEY_GRAM_KEYS[1] and KEY_GRAM_LAYER_KEYS a run with config ``c`` is recorded (and a snapshot compared) under: a
    one-entry list with weight 1, uncentred, becomes ``dino_gram_layer``; any other list or the centred form becomes the canonical list with
    ``dino_gram_layer`` null; a config without the new keys keeps what ``key_gram_rule`` makes of it.  Checks what the two rules check."""
    lk, wk, ck = KEY_GRAM_LAYER_KEYS
    rule = key_gram_layers_rule(c, depth)
    if rule is not None:
        return {KEY_GRAM_KEYS[1]: None, lk: list(rule[1]), wk: list(rule[2]), ck: rule[3]}
    out = {lk: None, wk: None, ck: False}
    layers = c.get(lk, DEFAULT_CFG[lk])
    if layers is not None:
        out[KEY_GRAM_KEYS[1]] = int(layers[0])
    else:
        base = key_gram_rule(c, depth)
        out[KEY_GRAM_KEYS[1]] = None if base is None else base[1]
    return out


def np_key_gram_layers(kx_list, kb_list, lam, weights=None, centered=False):
    """The term over several blocks restated in NumPy float64: ``kx_list[i]``, ``kb_list[i]`` the ``[T][D]`` keys of
    block i of the generated and of the target pass; ``weights`` one number per block (None: all 1).  With ``M(K) = K^T K / T`` --
    ``centered``: ``- mu mu^T``, ``mu = K^T 1 / T`` -- and ``Delta_i = M(kx_i) - M(kb_i)`` returns ``(raw, addends, dK)``:
    ``addends[i] = w_i mean(Delta_i^2)`` over the ``D * D`` entries, ``raw`` their sum ascending, ``dK[i] = (4 lam w_i / (T D^2))
    (kx_i Delta_i - 1 (Delta_i mu_i)^T)`` (the second part where centred), the gradient of ``lam * raw`` with respect to ``kx_i``."""
    n = len(kx_list)
    weights = [1.0] * n if weights is None else [float(w) for w in weights]
    raw, addends, grads = 0.0, [], []
    for kx, kb, w in zip(kx_list, kb_list, weights):
        kx, kb = np.asarray(kx, np.float64), np.asarray(kb, np.float64)
        T, D = kx.shape
        delta = (kx.T @ kx - kb.T @ kb) / T
        g = kx @ delta
        if centered:
            mx, mb = kx.mean(0), kb.mean(0)
            delta = delta - (np.outer(mx, mx) - np.outer(mb, mb))
            g = kx @ delta - np.outer(np.ones(T), delta @ mx)
        addends.append(w * float(np.mean(delta * delta)))
        raw += addends[-1]
        grads.append((4.0 * float(lam) * w / (T * D * D)) * g)
    return raw, addends, grads


def np_key_gram(kx, kb, lam):
    """The key second-moment term restated in NumPy float64: ``kx``, ``kb`` the ``[T][D]`` keys of the generated
    and of the target pass (every token, the heads concatenated).  With ``G(K) = K^T K / T`` and ``Delta = G(kx) - G(kb)`` returns
    ``(raw, dK)``: ``raw = mean(Delta^2)`` over the ``D * D`` entries, ``dK = (4 lam / (T D^2)) kx Delta``, the gradient of ``lam * raw``
    with respect to ``kx``.  The target carries no gradient."""
    kx, kb = np.asarray(kx, np.float64), np.asarray(kb, np.float64)
    T, D = kx.shape
    delta = (kx.T @ kx - kb.T @ kb) / T
    return float(np.mean(delta * delta)), (4.0 * float(lam) / (T * D * D)) * (kx @ delta)


def np_ssim_layers(values, weights=None):
    """A word of a losses row -- 1 / 2, 4 / 3, 5 -- from the per-layer addends ``engine.ssim_layer_values`` / ``cls_layer_values`` /
    ``id_layer_values`` report (already weighted; ``weights`` given: unweighted values, multiplied in float32 first): their float32 sum over
    the blocks ascending, one rounding per addition, from 0."""
    f = np.float32
    acc = f(0)
    for i, v in enumerate(values):
        acc = f(acc + (f(v) if weights is None else f(f(weights[i]) * f(v))))
    return acc


np_cls_layers = np_id_layers = np_ssim_layers


def snapshot_cfg_mismatch(a, b):
    """The first key (sorted) on which the configs ``a`` and ``b`` differ among those that enter a slot's arithmetic -- every key but
    SNAPSHOT_FREE_KEYS, an absent key standing for its default -- or None."""
    for key in sorted((set(a) | set(b)) - set(SNAPSHOT_FREE_KEYS)):
        if a.get(key, DEFAULT_CFG.get(key)) != b.get(key, DEFAULT_CFG.get(key)):
            return key
    return None


def _entire_branch(c):
    return c["lambda_entire_ssim"] > 0 or c["lambda_entire_cls"] > 0


def merge_pair_cfgs(cfg, pair_cfgs):
    """The per-slot configs of a sweep: ``cfg`` (base) merged with each override dict of ``pair_cfgs``.  Checked on the host
    alone (nothing touches the GPU): at most MAX_PAIR_CFGS slots; a variant may set only PAIR_KEYS (a shared key only to the
    base value); every slot's optimiser / schedule must be valid; all slots must agree on whether the entire-image branch
    exists (a slot without it makes no G(A) call, so its BatchNorm statistics would not be its single run's).  Raises
    ValueError naming the offending key."""
    base = dict(DEFAULT_CFG, **cfg)
    pair_cfgs = list(pair_cfgs)
    if not pair_cfgs:
        raise ValueError("pair_cfgs: at least one variant")
    if len(pair_cfgs) > MAX_PAIR_CFGS:
        raise ValueError(f"pair_cfgs: {len(pair_cfgs)} variants, at most {MAX_PAIR_CFGS} slots per engine")
    out = []
    for k, over in enumerate(pair_cfgs):
        if not isinstance(over, dict):
            raise ValueError(f"pair_cfgs[{k}]: a dict of per-slot overrides")
        for key, val in over.items():
            if key not in PAIR_KEYS and (key not in base or base[key] != val):
                raise ValueError(f"pair_cfgs[{k}]: '{key}' is shared by every slot of a sweep (per-slot keys: {', '.join(PAIR_KEYS)})")
        c = dict(base, **over)
        for key in PAIR_LAMBDA_KEYS:
            if not c[key] >= 0:
                raise ValueError(f"pair_cfgs[{k}]: '{key}' must be >= 0")
        LrSchedule(c)   # (refuses plateau / unknown policies with the reason)
        out.append(c)
    if len({_entire_branch(c) for c in out}) > 1:
        raise ValueError("pair_cfgs: the variants disagree on whether the entire-image branch exists (lambda_entire_cls / lambda_entire_ssim > 0): "
                         "a slot without it makes no G(A) call and its BatchNorm statistics would differ from its single run")
    return out


# ------------------------------------------------------------------------------------------------------------- restatements
def np_ema(e, p, step, decay, start):
    """The rule of the weight average restated in NumPy float32, one rounding per operation: ``e`` after the update number
    ``step`` (1-based) that wrote the parameters ``p``."""
    f = np.float32
    if step <= start:
        return np.array(p, dtype=f)
    d = f(decay)
    return (d * np.asarray(e, dtype=f) + (f(1) - d) * np.asarray(p, dtype=f)).astype(f)


def np_plateau(losses, counted, window, rel, patience, min_steps, margins=None):
    """The plateau stop rule with its keep-best record and window history (include/splice_hip.h) restated in NumPy float32, one
    rounding per operation: the slot's state after the steps ``losses`` (``counted[t]``: step t is counted).  Returns a dict of the
    ``splice_stop_state`` fields (``sum count windows best bad stop_step``), the record ``best_step`` / ``best_window`` (-1 until a
    window has closed), ``means`` -- float32, the means of the windows closed while the slot was live, at most STOP_HISTORY of them --
    and ``moves``, how often the record moved.  ``margins`` collects |mean - threshold| / |threshold| of every comparison made."""
    f = np.float32
    s = dict(sum=f(0), count=0, windows=0, best=f(0), bad=0, stop_step=-1, best_step=-1, best_window=-1, moves=0)
    means = []
    for t, (loss, c) in enumerate(zip(losses, counted)):
        if not c:
            continue
        s["sum"] = f(s["sum"] + f(loss))
        s["count"] += 1
        if s["count"] < window:
            continue
        mean = f(s["sum"] / f(window))
        live = s["stop_step"] < 0            # on entry: the stopping step itself is still live
        better = s["windows"] == 0
        if not better:
            thr = f(s["best"] * f(f(1.0) - f(rel)))
            if margins is not None:
                margins.append(abs(float(mean) - float(thr)) / abs(float(thr)))
            better = bool(mean < thr)
        if better:
            s["best"], s["bad"] = mean, 0
            if live:
                s["best_step"], s["best_window"] = t, s["windows"]
                s["moves"] += 1
        else:
            s["bad"] += 1
        if live and s["windows"] < STOP_HISTORY:
            means.append(mean)
        s["windows"] += 1
        s["sum"], s["count"] = f(0), 0
        if s["bad"] >= patience and t >= min_steps and s["stop_step"] < 0:
            s["stop_step"] = t
    s["means"] = np.array(means, dtype=f)
    return s


def np_lr_plateau(losses, counted, window, rel, patience, min_steps, factor, lr_patience, min_scale, margins=None):
    """The plateau lr rule on top of the stop rule (include/splice_hip.h) restated in NumPy float32, one rounding per operation: the
    slot's state after the steps ``losses`` (``counted[t]``: step t is counted).  Returns the ``splice_stop_state`` fields of
    ``np_plateau`` (``sum count windows best bad stop_step``), ``lr`` -- the ``splice_lr_state`` record as ``lr_state()`` gives it:
    ``scale bad cuts last_cut_step`` and ``cut_steps``, the step indices of the cuts -- and ``scales``, float32, the scale in force at
    each step (what the step's update multiplied its lr by: a cut made at step t first shows at t + 1; for a stopped slot the scale
    its record holds).  ``margins`` as in ``np_plateau``."""
    f = np.float32
    s = dict(sum=f(0), count=0, windows=0, best=f(0), bad=0, stop_step=-1)
    lr = dict(scale=f(1), bad=0, cuts=0, last_cut_step=-1, cut_steps=[])
    scales = []
    for t, (loss, c) in enumerate(zip(losses, counted)):
        scales.append(lr["scale"])           # read before this step's rule runs
        if not c:
            continue
        s["sum"] = f(s["sum"] + f(loss))
        s["count"] += 1
        if s["count"] < window:
            continue
        mean = f(s["sum"] / f(window))
        live = s["stop_step"] < 0            # on entry: the stopping step itself is still live
        better = s["windows"] == 0
        if not better:
            thr = f(s["best"] * f(f(1.0) - f(rel)))
            if margins is not None:
                margins.append(abs(float(mean) - float(thr)) / abs(float(thr)))
            better = bool(mean < thr)
        if better:
            s["best"], s["bad"] = mean, 0
        else:
            s["bad"] += 1
        s["windows"] += 1
        s["sum"], s["count"] = f(0), 0
        if s["bad"] >= patience and t >= min_steps and s["stop_step"] < 0:
            s["stop_step"] = t
        if not live:                         # a frozen slot's record is never written again
            continue
        if better:
            lr["bad"] = 0
            continue
        lr["bad"] += 1
        if lr["bad"] >= lr_patience and lr["scale"] > f(min_scale) and lr["cuts"] < STOP_HISTORY:
            lr["scale"] = max(f(lr["scale"] * f(factor)), f(min_scale))
            lr["cut_steps"].append(t)
            lr["cuts"] += 1
            lr["last_cut_step"] = t
            lr["bad"] = 0
    s["lr"] = lr
    s["scales"] = np.array(scales, dtype=f)
    return s


def replay_lr_scales(cut_steps, steps, factor, min_scale):
    """The scale in force at each of ``steps`` steps, float32, replayed on the host from a slot's ``cut_steps``: the cut made at step
    t first acts on step t + 1, each cut is ``scale = max(fl(scale * factor), min_scale)``."""
    f = np.float32
    out, scale, cuts = [], f(1), sorted(int(t) for t in cut_steps)
    k = 0
    for t in range(steps):
        while k < len(cuts) and cuts[k] < t:
            scale = max(f(scale * f(factor)), f(min_scale))
            k += 1
        out.append(scale)
    return np.array(out, dtype=f)


def np_image_terms(x, y=None, b=None):
    """The image-space terms (include/splice_hip.h) restated in NumPy float64, value and gradient, for ONE image each:
    ``x`` ``[3, h, w]`` -> ``TV(x) = mean|x[:,1:,:] - x[:,:-1,:]| + mean|x[:,:,1:] - x[:,:,:-1]|`` (each mean over its own count, a
    direction without differences contributes 0) and ``dTV/dx`` with ``sign(0) = 0``; ``y``, ``b`` -> ``mean((y - b)^2)`` and
    ``2 (y - b) / (3 h w)``.  The differences are taken in the inputs' own dtype (the sign of an fp32 difference is exact), everything
    else in float64.  Returns ``(tv, dtv, pix, dpix)``, the pair of an absent input as ``None``."""
    tv = dtv = pix = dpix = None
    if x is not None:
        x = np.asarray(x)
        dv, dh = (x[:, 1:, :] - x[:, :-1, :]).astype(np.float64), (x[:, :, 1:] - x[:, :, :-1]).astype(np.float64)
        tv, dtv = 0.0, np.zeros(x.shape, dtype=np.float64)
        if dv.size:
            tv += np.abs(dv).sum() / dv.size
            dtv[:, 1:, :] += np.sign(dv) / dv.size
            dtv[:, :-1, :] -= np.sign(dv) / dv.size
        if dh.size:
            tv += np.abs(dh).sum() / dh.size
            dtv[:, :, 1:] += np.sign(dh) / dh.size
            dtv[:, :, :-1] -= np.sign(dh) / dh.size
        tv = float(tv)
    if y is not None:
        d = np.asarray(y).astype(np.float64) - np.asarray(b).astype(np.float64)
        pix, dpix = float((d * d).sum() / d.size), 2.0 * d / d.size
    return tv, dtv, pix, dpix


def _halving_tree(a):
    """``a[..., t] += a[..., t + off]`` for off = 128, 64, ..., 1 over the last axis (256 wide); returns ``a[..., 0]``."""
    a = a.copy()
    off = 128
    while off:
        a[..., :off] = a[..., :off] + a[..., off:2 * off]
        off //= 2
    return a[..., 0]


def np_grad_clip(g, g2, max_norm):
    """The rule of the gradient clipping (``splice_grad_norm_pairs``; include/splice_hip.h) restated in NumPy, one float32 rounding
    per operation where the kernels work in fp32: ``(sumsq, norm, coef, skip)`` of ONE pair's gradient ``g`` (+ ``g2`` unless None),
    the first three float32 scalars."""
    f = np.float32
    with np.errstate(all="ignore"):
        s = np.asarray(g, dtype=f).reshape(-1)
        if g2 is not None:
            s = (s + np.asarray(g2, dtype=f).reshape(-1)).astype(f)
        n = s.size
        chunks = (n + CLIP_CHUNK - 1) // CLIP_CHUNK
        sq = np.zeros(chunks * CLIP_CHUNK, dtype=f)
        sq[:n] = s * s
        sq = sq.reshape(chunks, 4, 256, 4)   # [chunk][round j][thread t][component c]
        acc = np.zeros((chunks, 256), dtype=f)
        for j in range(4):
            for c in range(4):
                acc = (acc + sq[:, j, :, c]).astype(f)
        partials = _halving_tree(acc).astype(np.float64)   # stage 2 in fp64
        rows = (chunks + 255) // 256
        pad = np.zeros(rows * 256, dtype=np.float64)
        pad[:chunks] = partials
        pad = pad.reshape(rows, 256)
        acc2 = np.zeros(256, dtype=np.float64)
        for r in range(rows):
            acc2 = acc2 + pad[r]
        sumsq = f(_halving_tree(acc2))
        norm = np.sqrt(sumsq)
        if np.isfinite(norm):
            return sumsq, norm, np.minimum(f(1), f(max_norm) / (norm + f(1e-6))), 0
        return sumsq, norm, f(0), 1


def np_clip_auto(state, norm, regime, k, beta, warmup, max_norm):
    """One step of one pair of the adaptive clipping rule (``splice_grad_norm_pairs_auto``; include/splice_hip.h) restated in NumPy
    float32, one rounding per operation.  ``state``: the pair's ``splice_clip_auto_state`` as a dict ``ref`` (two float32),
    ``count`` (two ints), ``thr``, ``regime`` -- None: the zeros a run starts from; ``norm``: the float32 gradient norm of the step
    (``np_grad_clip``); ``max_norm``: the absolute cap, 0 for none.  Returns ``(new_state, coef, skip)``; ``state`` is not written."""
    f = np.float32
    ref, count = ([f(0), f(0)], [0, 0]) if state is None else ([f(x) for x in state["ref"]], [int(n) for n in state["count"]])
    norm, r = f(norm), int(regime)
    with np.errstate(all="ignore"):
        thr_auto = f(k) * ref[r] if r >= 0 and count[r] >= warmup and ref[r] > 0 else f(np.inf)
        thr = np.minimum(f(max_norm), thr_auto) if max_norm > 0 else thr_auto
        if np.isfinite(norm):
            coef, skip = np.minimum(f(1), thr / (norm + f(1e-6))), 0
            if r >= 0:
                x = np.minimum(norm, thr_auto)   # (a spike raises ref by at most the factor k)
                ref[r] = x if count[r] == 0 else f(f(beta) * ref[r]) + f((f(1) - f(beta)) * x)
                count[r] += 1
        else:
            coef, skip = f(0), 1
    return dict(ref=ref, count=count, thr=f(thr), regime=r), f(coef), skip


# ----------------------------------------------------------------------------------------------------------------- decoders
def lr_records(state_dev, cuts_dev):
    """Host dicts of device ``splice_lr_state`` records (int32 ``[P, 4]``) and their ``cut_steps`` rows (int32 ``[P, STOP_HISTORY]``):
    one synchronising copy."""
    raw = torch.cat([state_dev, cuts_dev], dim=1).cpu().numpy()
    scale = raw[:, :1].copy().view(np.float32)
    return [dict(scale=scale[p, 0], bad=int(raw[p, 1]), cuts=int(raw[p, 2]), last_cut_step=int(raw[p, 3]),
                 cut_steps=[int(t) for t in raw[p, 4:4 + max(0, min(int(raw[p, 2]), STOP_HISTORY))]]) for p in range(raw.shape[0])]


def clip_records(clip_dev):
    """Host dicts of device ``splice_clip_state`` records held as an int32 tensor ``[P, 6]`` (a synchronising copy)."""
    raw = clip_dev.cpu().numpy()
    fl = raw[:, :3].copy().view(np.float32)
    return [dict(sumsq=fl[p, 0], norm=fl[p, 1], coef=fl[p, 2], skip=int(raw[p, 3]), clipped=int(raw[p, 4]), skipped=int(raw[p, 5]))
            for p in range(raw.shape[0])]


def clip_auto_records(auto_dev):
    """Host dicts of device ``splice_clip_auto_state`` records held as an int32 tensor ``[P, 6]`` (a synchronising copy)."""
    raw = auto_dev.cpu().numpy()
    fl = raw.copy().view(np.float32)
    return [dict(ref=[fl[p, 0], fl[p, 1]], count=[int(raw[p, 2]), int(raw[p, 3])], thr=fl[p, 4], regime=int(raw[p, 5])) for p in range(raw.shape[0])]


# ---------------------------------------------------------------------------------------------------------- step arithmetic
def clip_regime(step_idx, cls_warmup, entire):
    """The regime of step ``step_idx`` under the adaptive clipping (host arithmetic only): -1 while ``step_idx < cls_warmup`` (the
    loss has not its full set of terms yet: observed by no reference), 1 on an entire-image step (``entire``), else 0."""
    return -1 if step_idx < cls_warmup else 1 if entire else 0


def counted_steps(step_idx, cls_warmup, entire_every=0):
    """Steps among 0 .. ``step_idx`` that the stop rule counts: ``step >= cls_warmup`` and not an entire-image step
    (``step % entire_every == 0``; ``entire_every`` 0: the engine has no entire-image branch).  These are the steps whose loss is
    composed alike."""
    w, e = int(cls_warmup), int(entire_every)
    if step_idx < w or step_idx < 0:
        return 0
    lo = max(w, 0)
    n = step_idx - lo + 1
    if e > 0:
        n -= step_idx // e - (lo - 1) // e   # multiples of e in [lo, step_idx]
    return n


def stop_window_closes(step_idx, window, cls_warmup, entire_every=0):
    """True when step ``step_idx`` is counted and closes a window of ``window`` counted steps (host arithmetic only)."""
    if window <= 0 or step_idx < 0:
        return False
    n = counted_steps(step_idx, cls_warmup, entire_every)
    return n > counted_steps(step_idx - 1, cls_warmup, entire_every) and n % window == 0


def active_terms(c, step_idx, entire_branch):
    """Which of LOSS_KEYS the step ``step_idx`` of a slot with config ``c`` computes (host arithmetic only): the global structure
    and identity terms from ``cls_warmup`` on, the entire-image terms on every ``entire_A_every``-th step of an engine that has the
    branch (``entire_branch``), each only with its lambda > 0."""
    on = step_idx >= c["cls_warmup"]
    ent = bool(entire_branch) and step_idx % c["entire_A_every"] == 0
    return {"loss": True, "loss_global_ssim": on and c["lambda_global_ssim"] > 0, "loss_entire_ssim": ent and c["lambda_entire_ssim"] > 0,
            "loss_entire_cls": ent and c["lambda_entire_cls"] > 0, "loss_global_cls": c["lambda_global_cls"] > 0,
            "loss_global_id_B": on and c["lambda_global_identity"] > 0,
            # the image-space terms: every step, no schedule
            **{k: c.get(lam, 0.0) > 0 for k, lam in zip(IMAGE_LOSS_KEYS, IMAGE_LAMBDA_KEYS)}}


def key_gram_active(c, step_idx):
    """Whether step ``step_idx`` of a run with config ``c`` computes the key second-moment term (KEY_GRAM_LOSS_KEY; host arithmetic only):
    from ``cls_warmup`` on, ordinary and entire-image steps alike, with its lambda > 0.  Beside ``active_terms``, whose dict keeps its keys."""
    return step_idx >= c["cls_warmup"] and c.get("lambda_global_key_gram", 0.0) > 0


def key_nn_active(c, step_idx):
    """Whether step ``step_idx`` of a run with config ``c`` computes the nearest-neighbour key term (KEY_NN_LOSS_KEY; host arithmetic only):
    the steps of the key second-moment term -- from ``cls_warmup`` on, ordinary and entire-image steps alike -- with its lambda > 0."""
    return step_idx >= c["cls_warmup"] and c.get("lambda_global_key_nn", 0.0) > 0


def resize_output_size(h, w, size, max_size=480):
    """Output (h, w) of torchvision-0.10 ``Resize(size, max_size)`` (util/losses.py:20): shorter
    edge -> size, aspect kept (long edge truncated), both shrunk if the long edge exceeds max_size;
    unchanged when the shorter edge already equals ``size``."""
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_short, new_long = size, int(size * long / short)
    if max_size is not None and new_long > max_size:
        new_short, new_long = int(max_size * new_short / new_long), max_size
    return (new_long, new_short) if w <= h else (new_short, new_long)
