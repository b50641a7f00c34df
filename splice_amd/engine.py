"""SpliceEngine / MultiPairEngine: the per-pair optimisation loop of ``train.py:34-80`` on one MI355X.

Owns the frozen DINO-ViT engine, the generator arenas (parameters / gradients / optimiser moments,
flat fp32 in ``netG.parameters()`` order, one arena per pair) and the fused step handle.  One engine = one
GPU = one stream; pairs are independent (no collectives): P of them ride one engine's launches
(``MultiPairEngine``), and GPUs run independent engines (``bench.py --gpus N``, ``splice_amd.batch``).
"""
import ctypes as C

import numpy as np
import torch

from . import _lib, synth
from .generator import GeneratorEngine, GeneratorPlan
from .rules import *  # noqa: F401,F403  (the host side of the rules: every public name of it is handed on from here, as it always was)
from .util import OPTIM_EXT_DEFAULTS, LrSchedule, fused_optimizer, fused_optimizer_ext, optim_ext_uses
from .vit import VitContext, VitEngine, fp8_mode


class MultiPairEngine:
    """P image pairs optimised side by side on one GPU (``pairs`` = P; P = 1 is the reference's one pair per process).

    The pairs share the frozen ViT and every kernel launch of a step; each has its own generator (parameter / gradient /
    Adam-moment arena ``[P, stride]``), its own BatchNorm statistics and its own loss values.  A pair's trajectory is
    bit-identical whichever batch it rides in (tests/test_multipair_gpu.py).  All pairs of a batch share the image and
    crop sizes."""

    # What a slot owns on the device, as (state key, engine attribute): THE list that snapshot(), restore() (so compact()), its host
    # checks and the accessors walk; an attribute that is None belongs to a rule that is off and is not kept.
    # Arenas hold `numel` floats per slot at row * stride, row tables one row per slot.  Beside them a slot owns its loss trace
    # (`trace_dev`: time-major, kept up to the step count) and its stop record (in the step handle); `grads` is scratch of a step.
    SLOT_ARENAS = (("params", "params"), ("m", "m"), ("v", "v"), ("w", "w"), ("ema", "ema"), ("best", "best"), ("best_ema", "best_ema"))
    SLOT_ROWS = (("running", "running"), ("losses", "losses_dev"), ("best_rec", "best_dev"), ("means", "means_dev"), ("clip", "clip_dev"),
                 ("clip_auto", "clip_auto_dev"), ("lr_state", "lr_state_dev"), ("lr_cuts", "lr_cuts_dev"))
    PAIR_NONE = None   # the slot `pair=None` stands for in the per-slot accessors; None: every slot, as a list

    def __init__(self, cfg, vit_state, gen_states, crop_hw, entire_hw=None, device="cuda", vit_engine=None, n_crops=1, fp8=False, top_cls_only=True,
                 pair_cfgs=None):
        """cfg: reference config keys (conf/default/config.yaml); vit_state: DINO state dict; gen_states: list of P generator
        state dicts (reference names); crop_hw: (h, w) of the (largest) global crops; entire_hw: (H, W) of the whole
        structure image or None to disable the entire branch.  ``n_crops`` > 1: the reference's ``global_{A,B}_crops_n_crops``
        -- every step takes ``[P*n_crops,3,h,w]`` crops (pair-major; ``[P,n_crops,3,h,w]`` is the same memory), netG sees each
        pair's crops as ONE batch (BatchNorm statistics over the pair's crops), every loss term is summed over the pair's crops.
        Pair p is bit for bit the ``SpliceEngine(n_crops=...)`` run of that pair.
        ``pair_cfgs``: one dict of per-slot overrides per pair (a sweep: PAIR_KEYS -- the five lambdas, lr and its schedule; the
        init keys are the caller's business), checked by ``merge_pair_cfgs``.  Slot p then runs, bit for bit, as a
        ``SpliceEngine`` with ``cfgs[p]`` would; ``lr`` becomes a list of P values."""
        # (what compact() builds the engine of the live slots from)
        self._ctor = dict(cfg=dict(cfg), crop_hw=crop_hw, entire_hw=entire_hw, device=device, n_crops=n_crops, fp8=fp8, top_cls_only=top_cls_only,
                          pair_cfgs=None if pair_cfgs is None else [dict(v) for v in pair_cfgs])
        self.cfg = dict(DEFAULT_CFG, **cfg)
        self.stop_rule = stop_rule(self.cfg)   # (host checks first: nothing below this line has touched a GPU yet)
        self.stop_compact = compact_rule(self.cfg)
        self.ema_rule = ema_rule(self.cfg)
        self.ema = None
        self.grad_clip = grad_clip_rule(self.cfg)
        self.clip_dev = None
        self.clip_auto = grad_clip_auto_rule(self.cfg)
        self.clip_auto_dev = None
        self.keep_best = best_rule(self.cfg)
        self.best = self.best_ema = self.best_dev = self.means_dev = None
        self.trace_on = trace_rule(self.cfg)
        self.trace_dev = None
        self.lr_rule = lr_plateau_rule(self.cfg)
        self.lr_state_dev = self.lr_cuts_dev = None
        self.opt_ext = fused_optimizer_ext(self.cfg)   # None: the plain rules, today's launches
        self.w = None
        self.image_terms = image_terms_rule(self.cfg)
        # the blocks of the structure terms, the two appearance terms and the key-identity term (LAYER_LIST_TERMS; DESIGN.md sections 9k, 9l,
        # 9m): ssim_layers / cls_layers / id_layers are None -- the top block, today's launches -- or the canonical (layers, weights), which the
        # config then holds too (what a snapshot is compared on)
        depth = vit_engine.depth if vit_engine is not None else synth.DINO_CONFIGS[self.cfg["dino_model_name"]][2]
        for term in LAYER_LIST_TERMS:
            rule = layer_list_rule(term, self.cfg, depth)
            setattr(self, term.attr, rule)
            if rule is not None:
                if fp8_mode(fp8):
                    raise ValueError(f"'{term.keys[0]}': not with fp8 -- {term.fp8}")
                self.cfg.update(zip(term.keys, (list(rule[0]), list(rule[1]))))
        # the key second-moment appearance term: None -- off, today's launches -- or (lambda, block); the config then
        # holds the block it runs on (what a snapshot is compared on)
        # ... over a list of blocks, or centred: key_gram_layers is None -- the one-block term or none, today's launches --
        # or (lambda, layers, weights, centered); the config holds the canonical spelling (a one-entry list of weight 1, uncentred, IS
        # dino_gram_layer), and key_gram stays key_gram_rule of that config: not None exactly where the term is on
        self.cfg.update(key_gram_canonical(self.cfg, depth))
        self.key_gram_layers = key_gram_layers_rule(self.cfg, depth)
        self.key_gram = key_gram_rule(self.cfg, depth)
        if self.key_gram is not None:
            if fp8_mode(fp8):
                raise ValueError("'lambda_global_key_gram': not with fp8 -- the term reads the bf16 key copies of a bf16 forward")
            nA_, nB_ = (int(n_crops), int(n_crops)) if isinstance(n_crops, int) else (int(n_crops[0]), int(n_crops[1]))
            if len(gen_states) > 1 and nA_ != nB_:
                raise ValueError(f"'lambda_global_key_gram': not with several pairs of different crop counts per side, got n_crops = {(nA_, nB_)}")
            self.cfg.update(lambda_global_key_gram=self.key_gram[0], dino_gram_layer=None if self.key_gram_layers is not None else self.key_gram[1])
        # the nearest-neighbour key appearance term: None -- off, today's launches -- or (lambda, block); the config then
        # holds the block it runs on (what a snapshot is compared on)
        self.key_nn = key_nn_rule(self.cfg, depth)
        if self.key_nn is not None:
            if fp8_mode(fp8):
                raise ValueError("'lambda_global_key_nn': not with fp8 -- the term reads the bf16 keys of a bf16 forward")
            nA_, nB_ = (int(n_crops), int(n_crops)) if isinstance(n_crops, int) else (int(n_crops[0]), int(n_crops[1]))
            if len(gen_states) > 1 and nA_ != nB_:
                raise ValueError(f"'lambda_global_key_nn': not with several pairs of different crop counts per side, got n_crops = {(nA_, nB_)}")
            self.cfg.update(lambda_global_key_nn=self.key_nn[0], dino_nn_layer=self.key_nn[1])
        P_in = len(gen_states)
        self.cfgs = [self.cfg] * P_in
        self._pair_lambdas = self._pair_lr = False
        if pair_cfgs is not None:
            if len(pair_cfgs) != P_in:
                raise ValueError(f"pair_cfgs: {len(pair_cfgs)} variants for {P_in} generator states")
            if (int(n_crops) if isinstance(n_crops, int) else max(int(n) for n in n_crops)) > 1:
                raise ValueError("pair_cfgs: a sweep takes one global crop per image (n_crops > 1 is not supported)")
            self.cfgs = merge_pair_cfgs(self.cfg, pair_cfgs)
            # a group of keys that is equal over the slots stays on the scalar path (no per-pair table, today's launches)
            self._pair_lambdas = len({tuple(cp[k] for k in PAIR_LAMBDA_KEYS) for cp in self.cfgs}) > 1
            self._pair_lr = len({tuple(cp.get(k) for k in PAIR_LR_KEYS) for cp in self.cfgs}) > 1
            c0 = self.cfgs[0]
            if self._pair_lambdas:   # (scalar fields: the largest weight of each term -- > 0 exactly where some slot needs the term)
                self.cfg.update({k: max(cp[k] for cp in self.cfgs) for k in PAIR_LAMBDA_KEYS})
            else:
                self.cfg.update({k: c0[k] for k in PAIR_LAMBDA_KEYS})
            if not self._pair_lr:
                self.cfg.update({k: c0[k] for k in PAIR_LR_KEYS if k in c0})
        c = self.cfg
        # n_crops: int, or (nA, nB) = (global_A_crops_n_crops, global_B_crops_n_crops) -- the reference zips the crop lists
        # (util/losses.py:76,87,98): structure term over the A crops, identity term over the B crops, appearance term over min pairs
        nA, nB = (int(n_crops), int(n_crops)) if isinstance(n_crops, int) else (int(n_crops[0]), int(n_crops[1]))
        self.n_crops_ab = (nA, nB)
        self.n_crops = max(nA, nB)
        if self.n_crops > 1 and len(gen_states) > 1:
            if min(nA, nB) < 1 or self.n_crops > 8:
                raise ValueError(f"n_crops: 1..8 crops per side, got {(nA, nB)}")
            if len(gen_states) * self.n_crops > MAX_GROUP_IMAGES:
                raise ValueError(f"n_crops: {len(gen_states)} pairs x {self.n_crops} crops = {len(gen_states) * self.n_crops} images per side, "
                                 f"at most {MAX_GROUP_IMAGES}")
        # optimizer adam / rmsprop / sgd and scheduler_policy none / linear / step / cosine (util/util.py:8-39); the lr of every step is
        # computed on the host and staged on the device (splice_step_set_lr), so a replayed graph runs with the scheduled value
        self.opt_kind, *self.opt_hp = fused_optimizer(c)
        self.schedule = LrSchedule(c)
        self.schedules = [LrSchedule(cp) for cp in self.cfgs] if self._pair_lr else None
        self._lr_staged = None
        self.lr = None   # the lr the last step used (a list of P values with pair_cfgs)
        self._lr_list = pair_cfgs is not None
        self.device = torch.device(device)
        self.P = P = len(gen_states)
        self.vit = vit_engine or VitEngine(c["dino_model_name"], device=device).load_state_dict(vit_state)
        # fp8 (vit.fp8_mode; BASELINE configs[4]): True / "gemm" -- the QKV, fc1 and fc2 forward projections (e4m3, block-scaled K = 128
        # MFMA) and the key self-similarity Gram matrices; "attention" -- the attention forward (Q K^T and P V on the fp8 MFMA) too;
        # proj and the whole backward stay bf16 / fp32.  The mode is a property of THIS engine's contexts: another engine sharing
        # the frozen ViT keeps its own.  Tolerances: tests/test_fp8_gpu.py.
        self.fp8 = fp8_mode(fp8)
        if self.fp8:
            self.vit.prepare_fp8()
        self.gen = GeneratorEngine(device=device)
        n = self.gen.numel
        self.stride = n if P == 1 else (n + 63) // 64 * 64
        self.params = torch.zeros(P * self.stride, device=self.device)
        for p_, st in enumerate(gen_states):
            if st is not None:   # (None: the slot is filled by restore())
                self.params[p_ * self.stride: p_ * self.stride + n] = self.gen.flatten(st)
        self.grads = torch.zeros_like(self.params)
        self.m = torch.zeros_like(self.params)
        self.v = torch.zeros_like(self.params)
        # BatchNorm buffers of every pair's netG (running_mean 0 / running_var 1 at construction, as nn.BatchNorm2d)
        self.running = torch.zeros(P, self.gen.buffer_numel, device=self.device)
        for name, (off, cnt) in self.gen.buffer_table.items():
            if name.endswith("running_var"):
                self.running[:, off:off + cnt] = 1.0
        self.generator_calls = [0] * len(gen_states)   # per pair: every BatchNorm's num_batches_tracked (one per netG call)
        # pair snapshots.  The slots keep their external numbers: P_in of them, of which `live` (ascending) are
        # still in the launches -- P = len(live), slot live[i] is row i of every arena and record -- and `_parked` holds the device
        # snapshot of every slot compact() took out.  Without stop_compact nothing is ever parked: live = 0 .. P - 1.
        self.P_in, self.live, self._parked = P, list(range(P)), {}
        Pz = c["dino_global_patch_size"]
        ch, cw = crop_hw
        vh, vw = resize_output_size(ch, cw, Pz, 480)
        self.crop_hw, self.vit_hw = (ch, cw), (vh, vw)
        slots = self.slots = P * self.n_crops    # images per generator plan / per ViT pass group (maximum of the two sides)
        sa, sb = (P * nA, P * nB) if self.n_crops > 1 else (P, P)
        self.slots_ab = (sa, sb)
        batch = self.n_crops > 1
        # A step engine's contexts are PRIVATE, never taken from the shape-keyed cache of ``VitEngine.context()``: with an identity
        # Resize the staged inputs, the generator outputs and their gradients live in the context's image slots, and the
        # [CLS]-only mode is a property of the context -- two engines (or an engine and the extractor API) sharing one would
        # overwrite each other's images.
        self.ctx_g = VitContext(self.vit, 2 * (sa + sb), vh, vw, True, fp8=self.fp8)
        arena_stride = self.stride if P > 1 else 0
        # private plan objects (the shape-keyed plan cache could hand out one plan twice)
        if batch and P > 1:   # several pairs: one netG call per pair's crops (grouped plans, arena per pair)
            self.plan_a = GeneratorPlan(self.gen, sa, ch, cw, True, arena_stride, groups=nA)
            self.plan_b = GeneratorPlan(self.gen, sb, ch, cw, True, arena_stride, groups=nB)
        else:
            self.plan_a = GeneratorPlan(self.gen, sa, ch, cw, True, arena_stride, batch_stats=batch and sa > 1)
            self.plan_b = GeneratorPlan(self.gen, sb, ch, cw, True, arena_stride, batch_stats=batch and sb > 1)
        sc = _lib.StepConfig()
        sc.crop_h, sc.crop_w, sc.vit_h, sc.vit_w = ch, cw, vh, vw
        sc.pairs, sc.arena_stride, sc.fp8_selfsim = P, arena_stride, int(bool(self.fp8))
        sc.n_crops, sc.n_crops_b = (nA, nB) if self.n_crops > 1 else (1, 0)
        # behind the last QKV projection only the [CLS] rows go on (all the losses read of the top block besides its keys):
        # +2.7 % / +5.2 % pair-steps/s at 4 / 8 pairs per GPU, neutral at one pair; top_cls_only=False
        # computes the whole top block as the reference does
        sc.top_cls_only = int(bool(top_cls_only))
        self.ctx_e = self.plan_e = None
        self.entire_hw = entire_hw
        use_entire = entire_hw is not None and (c["lambda_entire_ssim"] > 0 or c["lambda_entire_cls"] > 0)
        if use_entire:
            eh, ew = entire_hw
            evh, evw = resize_output_size(eh, ew, Pz, 480)
            self.ctx_e = VitContext(self.vit, 2 * P, evh, evw, True, fp8=self.fp8)   # (one entire image per pair, whatever n_crops)
            self.plan_e = GeneratorPlan(self.gen, P, eh, ew, True, arena_stride)
            sc.ent_h, sc.ent_w, sc.ent_vit_h, sc.ent_vit_w = eh, ew, evh, evw
        sc.lambda_global_cls, sc.lambda_global_ssim = c["lambda_global_cls"], c["lambda_global_ssim"]
        sc.lambda_global_identity = c["lambda_global_identity"]
        sc.lambda_entire_cls, sc.lambda_entire_ssim = c["lambda_entire_cls"], c["lambda_entire_ssim"]
        sc.entire_every, sc.cls_warmup = c["entire_A_every"], c["cls_warmup"]
        sc.lr, sc.beta1, sc.beta2, sc.eps = c["lr"], c["optimizer_beta1"], c["optimizer_beta2"], 1e-8
        h = C.c_void_p()
        _lib.check(_lib.lib().splice_step_create(C.byref(sc), self.ctx_g.handle, self.ctx_e.handle if self.ctx_e else None,
                                                 self.plan_a.handle, self.plan_b.handle, self.plan_e.handle if self.plan_e else None, C.byref(h)),
                   "step_create")
        self.handle = h
        if self.opt_kind != 0:
            _lib.check(_lib.lib().splice_step_set_optimizer(self.handle, self.opt_kind, *self.opt_hp), "step_set_optimizer")
        # the extended rules (shared by the slots): the option record, and the third moment arena exactly where the rule keeps one (Adam's
        # max_exp_avg_sq under amsgrad, RMSprop's grad_avg when centered); m then also holds the momentum buffer; before the first step
        if self.opt_ext is not None:
            if optim_ext_uses(self.opt_kind, self.opt_ext)[2]:
                self.w = torch.zeros_like(self.params)
            _lib.check(_lib.lib().splice_step_set_optimizer_ext(self.handle, C.byref(_lib.optim_ext(self.opt_ext)), _lib.ptr(self.w)), "step_set_optimizer_ext")
        _lib.check(_lib.lib().splice_step_set_running_stats(self.handle, _lib.ptr(self.running), self.running.stride(0)), "step_set_running_stats")
        # the plateau stop rule (shared by the slots; decided per slot on the device): before the first step
        if self.stop_rule[0] > 0:
            _lib.check(_lib.lib().splice_step_set_stop_rule(self.handle, *self.stop_rule), "step_set_stop_rule")
        # the weight average (shared by the slots): an arena like params, written by the step's own optimiser launch; before the first step
        if self.ema_rule[0] > 0:
            self.ema = self.params.clone()
            _lib.check(_lib.lib().splice_step_set_ema(self.handle, _lib.ptr(self.ema), *self.ema_rule), "step_set_ema")
        # gradient clipping (shared by the slots): one record per slot on the device, written by the step's norm launches; before the first step
        # -- against the absolute norm, k times the slot's own running norm (a second record per slot, written by the same launch), or both
        if self.clip_auto[0] > 0:
            self.clip_dev = torch.zeros(P, 6, dtype=torch.int32, device=self.device)
            self.clip_auto_dev = torch.zeros(P, 6, dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().splice_step_set_grad_clip_auto(self.handle, self.grad_clip, *self.clip_auto, _lib.ptr(self.clip_dev),
                                                                 _lib.ptr(self.clip_auto_dev)), "step_set_grad_clip_auto")
        elif self.grad_clip > 0:
            self.clip_dev = torch.zeros(P, 6, dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().splice_step_set_grad_clip(self.handle, self.grad_clip, _lib.ptr(self.clip_dev)), "step_set_grad_clip")
        # the best window's weights (shared by the slots): arenas like params / ema -- until a window closes, "best" is the initial weights --
        # written by the step's own optimiser launch where the rule's record, written by the same step's loss kernel, says so; behind the
        # rule and the average, before the first step
        if self.keep_best:
            self.best = self.params.clone()
            self.best_ema = self.ema.clone() if self.ema is not None else None
            self.best_dev = torch.full((P, 2), -1, dtype=torch.int32, device=self.device)
            self.means_dev = torch.zeros(P, STOP_HISTORY, device=self.device)
            _lib.check(_lib.lib().splice_step_set_keep_best(self.handle, _lib.ptr(self.best), _lib.ptr(self.best_ema), _lib.ptr(self.best_dev),
                                                            _lib.ptr(self.means_dev)), "step_set_keep_best")
        # the loss trace (shared by the slots): one row of 8 floats per step and slot, NaN until the step's own launches write it; before
        # the first step
        if self.trace_on:
            self.trace_dev = torch.full((max(int(c["n_epochs"]), 1), P, 8), float("nan"), device=self.device)
            _lib.check(_lib.lib().splice_step_set_loss_trace(self.handle, _lib.ptr(self.trace_dev), self.trace_dev.shape[0]), "step_set_loss_trace")
        # the plateau lr rule (shared by the slots; decided per slot in the loss kernel): one record and one row of cut steps per slot, the
        # caller's; behind the stop rule, before the first step
        if self.lr_rule[0] > 0:
            self.lr_state_dev = torch.tensor([[np.float32(1).view(np.int32).item(), 0, 0, -1]] * P, dtype=torch.int32, device=self.device)
            self.lr_cuts_dev = torch.full((P, STOP_HISTORY), -1, dtype=torch.int32, device=self.device)
            _lib.check(_lib.lib().splice_step_set_lr_plateau(self.handle, *self.lr_rule, _lib.ptr(self.lr_state_dev), _lib.ptr(self.lr_cuts_dev)),
                       "step_set_lr_plateau")
        # the image-space terms (shared by the slots): a value launch, a gradient-add launch per chain, another loss-kernel instance; before
        # the first step.  Both 0: the call is not made and the handle launches what it always did
        if max(self.image_terms) > 0:
            _lib.check(_lib.lib().splice_step_set_image_terms(self.handle, *self.image_terms), "step_set_image_terms")
        # the blocks of the three plain per-layer terms (shared by the slots), before the first step: the structure terms (the layer is one
        # more grid dimension of the three self-similarity launches), the appearance terms (one layered launch per term, [CLS]-row seeds into
        # the ViT backward), then the identity term (two layered launches, fp32 keys and key gradients of the named blocks on the y' chain),
        # behind the structure layers whose buffers it shares.  The default: the call is not made and the handle launches what it always did
        for term in LAYER_LIST_TERMS:
            rule = getattr(self, term.attr)
            if rule is not None:
                n = len(rule[0])
                _lib.check(getattr(_lib.lib(), term.setter)(self.handle, n, (C.c_int * n)(*rule[0]), (C.c_float * n)(*rule[1])), term.setter[len("splice_"):])
        # the key second-moment term (shared by the slots): three launches on the x' chain from cls_warmup on; before the first step, behind
        # the structure and identity layers (shared key-gradient buffers).  The default: the call is not made
        if self.key_gram_layers is not None:   # (the list, or the centred form: the layered launches)
            lam, layers, weights, centered = self.key_gram_layers
            n = len(layers)
            _lib.check(_lib.lib().splice_step_set_key_gram_layers(self.handle, C.c_float(lam), n, (C.c_int * n)(*layers), (C.c_float * n)(*weights), int(centered)),
                       "step_set_key_gram_layers")
        elif self.key_gram is not None:
            _lib.check(_lib.lib().splice_step_set_key_gram(self.handle, C.c_float(self.key_gram[0]), int(self.key_gram[1])), "step_set_key_gram")
        # the nearest-neighbour key term (shared by the slots): four launches on the x' chain from cls_warmup on; before the first step, behind
        # the setters above (shared key-gradient buffers).  The default: the call is not made
        if self.key_nn is not None:
            _lib.check(_lib.lib().splice_step_set_key_nn(self.handle, C.c_float(self.key_nn[0]), int(self.key_nn[1])), "step_set_key_nn")
        self._lr_scale = [1.0] * P   # the host's copy of every slot's lr scale, refreshed with the stop steps
        self._stopped = [None] * P   # the host's copy of every slot's stop step, refreshed by stop_state()
        self._stop_dirty = False     # a window has closed since the last stop_state(): the copy may be behind
        if self._pair_lambdas:
            lam = (C.c_float * (5 * P))(*[float(cp[k]) for cp in self.cfgs for k in PAIR_LAMBDA_KEYS])
            _lib.check(_lib.lib().splice_step_set_pair_weights(self.handle, lam), "step_set_pair_weights")
        self.losses_dev = torch.zeros(P, 8, device=self.device)
        self.step_idx = -1  # data/Dataset.py:57 -- the first step is 0
        self._cur_crops = (ch, cw, ch, cw)
        self._log_plans = {}

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                _lib.lib().splice_step_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def step(self, A_crop, B_crop, A_entire=None, _repeat=False):
        """One optimisation step of every pair, asynchronous on the current stream.  Tensors: fp32 CUDA ``[P,3,h,w]`` in
        [0,1] (``[3,h,w]`` accepted for P = 1).  Returns the device tensor ``[P,8]`` of losses (see LOSS_KEYS).
        ``_repeat``: another phase of the step just run (``splice_step_set_phases``): no bookkeeping.
        With ``stop_compact`` the inputs keep the ``P_in`` pairs the engine was built for, whatever has been parked since (the
        staging launch gathers the live pairs), and the returned tensor -- ``losses_dev`` -- has one row per entry of ``engine.live``,
        in that order; after a step that closes a window the engine calls ``compact()`` itself."""
        if not _repeat:
            self.step_idx += 1
            if self._pair_lr:   # every slot's own schedule; staged per step, re-sent only when a value changes
                self.lr = [sch.lr(self.step_idx) for sch in self.schedules]
                if self.lr != self._lr_staged:
                    _lib.check(_lib.lib().splice_step_set_pair_lr(self.handle, (C.c_float * self.P)(*self.lr)), "step_set_pair_lr")
                    self._lr_staged = list(self.lr)
            else:
                self.lr = self.schedule.lr(self.step_idx)
                if self.schedule.policy != "none":   # (without a schedule the handle keeps cfg lr as a kernel argument, as before)
                    _lib.check(_lib.lib().splice_step_set_lr(self.handle, self.lr), "step_set_lr")
                if self._lr_list:
                    self.lr = [self.lr] * self.P
            if self._parked and self._lr_list:   # (a parked slot's entry: its own schedule goes on, as the frozen slot's does)
                live_lr = dict(zip(self.live, self.lr))
                self.lr = [live_lr[p] if p in live_lr else self._parked_schedules[p].lr(self.step_idx) for p in range(self.P_in)]
        for t, n in ((A_crop, self.slots_ab[0]), (B_crop, self.slots_ab[1])):
            assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()
            assert t.numel() == n // self.P * self.P_in * 3 * t.shape[-2] * t.shape[-1], (tuple(t.shape), n)
        crops = tuple(A_crop.shape[-2:]) + tuple(B_crop.shape[-2:])
        if crops != self._cur_crops:   # per-step random crop sizes (data/transforms.py:21-22)
            _lib.check(_lib.lib().splice_step_set_crops(self.handle, *crops), "step_set_crops")
            self._cur_crops = crops
        entire = self.plan_e is not None and self.step_idx % self.cfg["entire_A_every"] == 0
        if A_entire is not None:
            assert A_entire.is_cuda and A_entire.is_contiguous() and A_entire.numel() == self.P_in * 3 * self.entire_hw[0] * self.entire_hw[1]
        _lib.check(_lib.lib().splice_step_run(self.handle, _lib.ptr(self.params), _lib.ptr(self.grads), _lib.ptr(self.m), _lib.ptr(self.v),
                                              _lib.ptr(A_crop), _lib.ptr(B_crop), _lib.ptr(A_entire), self.step_idx,
                                              _lib.ptr(self.losses_dev), _lib.current_stream()), "step_run")
        if not _repeat:
            self.generator_calls = [n + (3 if entire else 2) for n in self.generator_calls]   # models/model.py:15-23: G(A_global) [, G(A)], G(B_global)
            if self.stop_rule[0] > 0 and self.window_closes(self.step_idx):
                self._stop_dirty = True
                if self.stop_compact:   # (the host reads the stop records after such a step anyway: no step gains a synchronisation)
                    self.compact()
        return self.losses_dev

    # ---- the plateau stop rule: decided per slot on the device; the host asks only where the answer can change
    def window_closes(self, step_idx):
        """True when step ``step_idx`` closes a window of the stop rule (host arithmetic only): the only steps at which a slot can
        stop, so the only ones after which ``stop_state()`` is worth a device-to-host copy."""
        return stop_window_closes(step_idx, self.stop_rule[0], self.cfg["cls_warmup"], self.cfg["entire_A_every"] if self.plan_e is not None else 0)

    def stop_state(self):
        """One dict per slot -- ``stopped_at`` (step index, or None while the slot runs), ``windows`` closed, ``best`` window mean,
        ``bad`` consecutive windows that were not better -- copied from the device (waits for the current stream)."""
        rec = self._stop_records()
        self._stopped = [r[5] if r[5] >= 0 else None for r in rec]
        if self.lr_state_dev is not None:   # (a window closed: the only steps at which a scale can move)
            self._lr_scale = [float(d["scale"]) for d in self._decoded(lr_records, "lr_state", "lr_cuts")]
        self._stop_dirty = False
        return [dict(stopped_at=k, windows=r[2], best=r[3], bad=r[4]) for k, r in zip(self._stopped, rec)]

    def _stop_records(self):
        """Per external slot the ``splice_stop_state`` record as a tuple ``(sum, count, windows, best, bad, stop_step)``: the live
        slots' from the device (waits for the current stream), a parked slot's as it stood when the slot was parked -- behind its stop
        step a slot's record only digests the losses of frozen weights."""
        rec = (_lib.StopState * self.P)()
        _lib.check(_lib.lib().splice_step_stop_state(self.handle, rec, _lib.current_stream()), "step_stop_state")
        return self._per_slot([(r.sum, r.count, r.windows, r.best, r.bad, r.stop_step) for r in rec], lambda s: tuple(s["stop"]))

    # ---- pair snapshots: external slot numbers over the rows of the live slots and the parked states
    def _parked_states(self):
        return getattr(self, "_parked", None) or {}

    def _row(self, pair):
        """Row of external slot ``pair`` in the arenas and records; None: the slot is parked."""
        live = getattr(self, "live", None)
        return pair if live is None else live.index(pair) if pair in live else None

    def _per_slot(self, rows, parked):
        """A list over the external slots: ``rows[i]`` of live slot ``live[i]``, ``parked(state)`` of a parked one."""
        states = self._parked_states()
        if not states:
            return list(rows)
        return [parked(states[p]) if p in states else rows[self.live.index(p)] for p in range(self.P_in)]

    def _kept(self, table):
        """``(state key, tensor)`` of the entries of ``table`` (SLOT_ARENAS / SLOT_ROWS) that this engine's rules keep."""
        return [(key, t) for key, t in ((key, getattr(self, attr, None)) for key, attr in table) if t is not None]

    def _decoded(self, decode, *keys):
        """The row tables ``keys`` (SLOT_ROWS) on the host, a list over the external slots: ``decode(*tables)`` gives one value per live
        row in one device-to-host copy (waits for the current stream); a parked slot's is decoded alike from the rows of its state."""
        attrs = dict(self.SLOT_ROWS)
        return self._per_slot(decode(*(getattr(self, attrs[k]) for k in keys)), lambda s: decode(*(s[k][None] for k in keys))[0])

    def _pick(self, per_slot, pair):
        """What a per-slot accessor hands out of its list over the slots: slot ``pair``'s entry, for ``pair=None`` the class's PAIR_NONE."""
        pair = self.PAIR_NONE if pair is None else pair
        return per_slot if pair is None else per_slot[pair]

    def _trace_rows(self):
        """Rows of ``trace_dev`` the steps so far have written: what a state, and an answer, holds of the trace."""
        return max(0, min(self.step_idx + 1, self.trace_dev.shape[0]))

    def snapshot(self, pair, device=None, _stop=None):
        """Everything that makes external slot ``pair`` continue, as a dict (``format`` 1): the ``numel`` floats of
        its parameters and optimiser moments, its BatchNorm buffers and ``generator_calls``, and with the rule that keeps them its weight
        average, best weights and record with the window means, stop record, clip record(s), lr record with the cut steps, and rows
        ``0 .. step_idx`` of its loss trace; its last losses row, ``step_idx`` and its config.  The gradient arena is not state: every
        backward overwrites it.  No arena stride either: a slot continues in an engine of any number of slots (``restore``).
        ``device="cpu"``: host tensors, a picklable state (waits for the current stream); None: device copies."""
        states = self._parked_states()
        if pair in states:
            # (as the frozen slot of an engine that parks nothing stands now: the step count and the netG calls went on, nothing else did)
            s = dict(states[pair], step_idx=self.step_idx, generator_calls=self.generator_calls[pair])
            if "trace" in s:   # (no step behind the stop step writes a frozen slot's rows: they stay NaN)
                rows = self._trace_rows() - s["trace"].shape[0]
                s["trace"] = torch.cat([s["trace"], torch.full((rows, 8), float("nan"), device=s["trace"].device)])
            return {k: (v.clone() if device is None else v.to(device, copy=True)) if torch.is_tensor(v) else v for k, v in s.items()}
        if not 0 <= pair < self.P_in:
            raise ValueError(f"snapshot: no slot {pair} among {self.P_in}")
        i = self._row(pair)
        take = (lambda t: t.detach().clone()) if device is None else (lambda t: t.detach().to(device, copy=True))   # (never a view of the engine's memory)
        s = dict(format=SNAPSHOT_FORMAT, step_idx=self.step_idx, cfg=dict(self.cfgs[pair]), n_crops=tuple(self.n_crops_ab), crop_hw=tuple(self.crop_hw),
                 entire_hw=tuple(self.entire_hw) if self.plan_e is not None else None, generator_calls=self.generator_calls[pair])
        for key, arena in self._kept(self.SLOT_ARENAS):
            s[key] = take(self._pair_arena(arena, pair, key))
        for key, table in self._kept(self.SLOT_ROWS):
            s[key] = take(table[i])
        if self.trace_dev is not None:
            s["trace"] = take(self.trace_dev[:self._trace_rows(), i])
        if self.stop_rule[0] > 0:
            s["stop"] = tuple((_stop or self._stop_records())[pair])
        return s

    def _check_states(self, states):
        """The host side of ``restore``: raises ValueError naming what does not fit, before anything touches a GPU."""
        states = list(states)
        if self.step_idx >= 0:
            raise ValueError(f"restore: the engine has already stepped (step_idx {self.step_idx}); a run is restored into a fresh engine")
        if len(states) != self.P:
            raise ValueError(f"restore: {len(states)} states for {self.P} slots (state count)")
        for k, s in enumerate(states):
            if not isinstance(s, dict) or s.get("format") != SNAPSHOT_FORMAT:
                raise ValueError(f"restore: states[{k}] is not a snapshot of 'format' {SNAPSHOT_FORMAT}")
        if len({s["step_idx"] for s in states}) > 1:
            raise ValueError(f"restore: the states disagree on 'step_idx' ({[s['step_idx'] for s in states]}): the slots of an engine share the step count")
        shape = dict(n_crops=tuple(self.n_crops_ab), crop_hw=tuple(self.crop_hw), entire_hw=tuple(self.entire_hw) if self.plan_e is not None else None)
        for k, s in enumerate(states):
            key = snapshot_cfg_mismatch(s["cfg"], self.cfgs[self.live[k]])
            if key is not None:
                raise ValueError(f"restore: states[{k}] was taken under another '{key}' ({s['cfg'].get(key)!r}, the slot has {self.cfgs[self.live[k]].get(key)!r})")
            for key, val in shape.items():
                if s[key] != val:
                    raise ValueError(f"restore: states[{k}] was taken with '{key}' {s[key]!r}, the engine has {val!r}")
            # (equal configs keep the same rules: a state that lacks a rule's part is damaged; an engine that has no such attribute at all --
            # a host-only stand-in -- is not asked about it)
            for key, attr in self.SLOT_ARENAS + self.SLOT_ROWS + (("trace", "trace_dev"),):
                if hasattr(self, attr) and (getattr(self, attr) is not None) != (key in s):
                    raise ValueError(f"restore: states[{k}] {'lacks' if key not in s else 'carries'} '{key}', which this engine's rules {'need' if key not in s else 'do not keep'}")
            if (self.stop_rule[0] > 0) != ("stop" in s):
                raise ValueError(f"restore: states[{k}] {'lacks' if 'stop' not in s else 'carries'} 'stop', the stop rule's record")
        return states

    def restore(self, states):
        """Continue a run: ``states`` holds one ``snapshot()`` per slot of this engine, which has not stepped; all of one ``step_idx``,
        each taken under the slot's config (every key but ``SNAPSHOT_FREE_KEYS``) -- else ValueError naming the key, before anything
        touches the GPU.  Fills the arenas, buffers and records, starts the step handle at ``step_idx + 1`` (``splice_step_restore``)
        and refreshes the host's copies of the stop steps and lr scales.  The next ``step()`` is, bit for bit, the one the snapshotted
        engine would have run -- whatever number of slots that engine had."""
        states = self._check_states(states)
        n, dev = self.gen.numel, self.device
        for i, s in enumerate(states):
            sl = slice(i * self.stride, i * self.stride + n)
            for key, arena in self._kept(self.SLOT_ARENAS):
                arena[sl].copy_(s[key])
            for key, table in self._kept(self.SLOT_ROWS):
                table[i].copy_(s[key])
            if self.trace_dev is not None:
                self.trace_dev[:s["trace"].shape[0], i].copy_(s["trace"])
            self.generator_calls[self.live[i]] = int(s["generator_calls"])
        self.step_idx = int(states[0]["step_idx"])
        rec = (_lib.StopState * self.P)(*[_lib.StopState(*s["stop"]) for s in states]) if self.stop_rule[0] > 0 else None
        _lib.check(_lib.lib().splice_step_restore(self.handle, self.step_idx + 1, rec, _lib.current_stream()), "step_restore")
        if self.stop_rule[0] > 0:
            self.stop_state()

    def compact(self):
        """Take the slots that have stopped out of the launches (``stop_compact`` calls it after every step that closes a window; DESIGN.md
        section 9g).  Nothing happens -- returns False -- unless some live slot has stopped and some other still runs.  Else every
        stopped slot's device snapshot is parked, a step handle, ViT contexts and generator plans for the remaining slots are built on
        the same ``VitEngine``, those slots' state moves over (``snapshot`` / ``restore``, device to device), the handle is told which
        rows of the caller's batches are its pairs, and the old handle is destroyed.  The slots keep their numbers: ``engine.live``
        lists those still in the launches, every per-slot accessor answers for a parked slot from its parked state, ``step()`` keeps
        taking ``P_in`` pairs.  Waits for the device."""
        if self.stop_rule[0] <= 0 or self.step_idx < 0:
            return False
        stops = self._stops()
        gone = [p for p in self.live if stops[p] is not None]
        keep = [p for p in self.live if stops[p] is None]
        if not gone or not keep:
            return False
        torch.cuda.synchronize(self.device)
        rec = self._stop_records()
        parked = {p: self.snapshot(p, _stop=rec) for p in gone}
        states = [self.snapshot(p, _stop=rec) for p in keep]
        ct = self._ctor
        new = MultiPairEngine(ct["cfg"], None, [None] * len(keep), ct["crop_hw"], ct["entire_hw"], device=ct["device"], vit_engine=self.vit,
                              n_crops=ct["n_crops"], fp8=ct["fp8"], top_cls_only=ct["top_cls_only"],
                              pair_cfgs=None if ct["pair_cfgs"] is None else [ct["pair_cfgs"][p] for p in keep])
        new.P_in, new.live, new.cfgs = self.P_in, keep, self.cfgs   # (the external numbering, before restore() looks the configs up)
        new.generator_calls = self.generator_calls
        new.restore(states)
        new.step_idx = self.step_idx
        _lib.check(_lib.lib().splice_step_set_input_rows(new.handle, self.P_in, (C.c_int * len(keep))(*keep)), "step_set_input_rows")
        # this engine becomes the new one: its handle, contexts, plans, arenas and records; the old handle goes the way __del__ sends it
        # (destroyed in front of the contexts and plans it was built on, which go with the last reference to them below)
        _lib.lib().splice_step_destroy(self.handle)
        self.handle = None
        mine = {k: self.__dict__[k] for k in ("_ctor", "_log_plans", "_logged", "lr", "_parked") if k in self.__dict__}
        schedules = getattr(self, "_parked_schedules", {})
        self.__dict__.update(new.__dict__)
        self.__dict__.update(mine)
        new.handle = None
        self._parked.update(parked)
        self._parked_schedules = {**schedules, **{p: LrSchedule(self.cfgs[p]) for p in gone}}
        self._lr_scale = [1.0] * self.P_in   # (the host's copies in the external numbering: refreshed from the records by the next question)
        self._stop_dirty = True
        return True

    def _stops(self):
        if self._stop_dirty:   # (asks the device only if a window closed since the last answer)
            self.stop_state()
        return self._stopped

    @property
    def stopped_at(self):
        """Per slot: the step index it stopped at, or None (``SpliceEngine``: its one pair's, no list)."""
        return self._pick(list(self._stops()), None)

    def all_stopped(self):
        """Every slot has stopped (never true with the rule off)."""
        return self.stop_rule[0] > 0 and all(k is not None for k in self._stops())

    def _frozen(self, pair):
        k = self._stops()[pair] if self.stop_rule[0] > 0 else None
        return k is not None and self.step_idx > k

    # ---- the plateau lr rule
    @property
    def lr_scale(self):
        """Per slot: the factor the loss kernel multiplies the slot's scheduled lr (``engine.lr``) by, 1.0 with the rule off.  The
        host's copy: refreshed, like the stop steps, only after a step that closed a window -- no other step can change it.
        (``SpliceEngine``: its one pair's, no list.)"""
        self._stops()
        return self._pick(list(self._lr_scale), None)

    def lr_state(self, pair=None):
        """Per slot the plateau lr rule's record (``lr_plateau_factor > 0``): ``scale`` (float32, what the next update multiplies its lr
        by), ``bad`` (consecutive windows that were not better since the last cut), ``cuts``, ``last_cut_step`` (-1: none) and
        ``cut_steps``, the step index of every cut.  One device-to-host copy (waits for the current stream).  One dict for ``pair``, a
        list over the slots for ``pair=None``."""
        if self.lr_state_dev is None:
            raise RuntimeError("lr_state: the lr is not cut on a plateau (lr_plateau_factor == 0)")
        return self._pick(self._decoded(lr_records, "lr_state", "lr_cuts"), pair)

    # ---- the best window's weights
    def _need_best(self, who):
        if self.best is None:
            raise RuntimeError(f"{who}: the best weights are not kept (stop_keep_best is off)")

    def pair_best(self, pair=0, ema=False):
        """View of one pair's weights after the step that closed its best window so far (``stop_keep_best``; the initial weights
        until a window has closed), laid out like ``pair_params``.  ``ema=True``: the weight average of that step."""
        self._need_best("pair_best")
        if ema and self.best_ema is None:
            raise RuntimeError("pair_best: no weight average is kept (ema_decay == 0)")
        return self._pair_arena(self.best_ema if ema else self.best, pair, "best_ema" if ema else "best")

    def _best_records(self):
        # one device-to-host copy of the records and the histories (the ints ride as float bit patterns); waits for the current stream
        raw = np.stack(self._decoded(lambda rec, means: list(torch.cat([rec.view(torch.float32), means], dim=1).cpu().numpy()), "best_rec", "means"))
        return raw[:, :2].copy().view(np.int32), raw[:, 2:]

    def best_state(self, pair=None):
        """Per slot ``best_step`` (the index of the step that closed the best window so far; None until a window has closed),
        ``best_window`` (that window's index, -1 alike) and ``best_mean`` (its mean; None until then, and for a window beyond the
        STOP_HISTORY the device keeps), copied from the device (waits for the current stream): call it at the end of a run or after a
        step that closes a window.  One dict for ``pair``, a list over the slots for ``pair=None``."""
        self._need_best("best_state")
        rec, means = self._best_records()
        dicts = [dict(best_step=int(r[0]) if r[0] >= 0 else None, best_window=int(r[1]),
                      best_mean=float(mu[r[1]]) if 0 <= r[1] < STOP_HISTORY else None) for r, mu in zip(rec, means)]
        return self._pick(dicts, pair)

    def window_means(self, pair=None):
        """The means of the windows every slot closed while it was live (float32 arrays, at most STOP_HISTORY each), copied from the
        device as ``best_state``.  One array for ``pair``, a list over the slots for ``pair=None``."""
        self._need_best("window_means")
        _, means = self._best_records()
        ent = self.cfg["entire_A_every"] if self.plan_e is not None else 0
        out = []
        for p, k in enumerate(self._stops()):   # (how many windows a slot closed is host arithmetic on its last live step)
            last = self.step_idx if k is None else k
            out.append(means[p, :min(counted_steps(last, self.cfg["cls_warmup"], ent) // self.stop_rule[0], STOP_HISTORY)].copy())
        return self._pick(out, pair)

    def clip_state(self, pair=None):
        """The gradient-clipping record(s) of the last step (``grad_clip_norm > 0`` or ``grad_clip_auto > 0``), copied from the device
        (waits for the current stream): ``sumsq`` / ``norm`` of the slot's gradient, the ``coef`` its update multiplied it by, ``skip``
        (the norm was not finite, the slot was not updated) and the counts ``clipped`` / ``skipped`` of such steps so far.  One dict for
        ``pair``, a list over the slots for ``pair=None``."""
        if self.clip_dev is None:
            raise RuntimeError("clip_state: the gradient is not clipped (grad_clip_norm == 0)")
        return self._pick(self._decoded(clip_records, "clip"), pair)

    def clip_auto_state(self, pair=None):
        """The record(s) of the adaptive clipping (``grad_clip_auto > 0``), copied from the device (waits for the
        current stream): ``ref``, the running gradient norm of the ordinary and of the entire-image steps (float32), ``count``, how many
        steps of either regime it has seen, and ``thr`` / ``regime``, the threshold (inf: none) and the regime (-1: before
        ``cls_warmup``) of the last step.  One dict for ``pair``, a list over the slots for ``pair=None``."""
        if self.clip_auto_dev is None:
            raise RuntimeError("clip_auto_state: the gradient is not clipped against its running norm (grad_clip_auto == 0)")
        return self._pick(self._decoded(clip_auto_records, "clip_auto"), pair)

    def losses(self, pair=None):
        """Host dict(s) of the last step's losses with the reference's keys (inactive terms omitted): one dict for ``pair``,
        a list over the pairs for ``pair=None``."""
        rows = self._decoded(lambda t: t.cpu().tolist(), "losses")   # (a parked slot: its last own row)
        acts = self.active_terms(self.step_idx)
        out = [{k: vals[i] for i, k in enumerate(LOSS_KEYS + IMAGE_LOSS_KEYS) if act[k]} for vals, act in zip(rows, acts)]
        if self.key_gram is not None and key_gram_active(self.cfg, self.step_idx):   # (its raw value lives beside the row; a parked slot's left with its handle)
            vals = self._key_gram_host()
            for p, d in enumerate(out):
                row = self._row(p)
                if row is not None:
                    d[KEY_GRAM_LOSS_KEY] = float(vals[row])
        if self.key_nn is not None and key_nn_active(self.cfg, self.step_idx):   # (likewise the nearest-neighbour term's)
            vals = self._key_nn_host()
            for p, d in enumerate(out):
                row = self._row(p)
                if row is not None:
                    d[KEY_NN_LOSS_KEY] = float(vals[row])
        return self._pick(out, pair)

    def _key_nn_host(self):
        buf = (C.c_float * self.P)()
        _lib.check(_lib.lib().splice_step_key_nn_values(self.handle, buf), "step_key_nn_values")
        return np.frombuffer(buf, dtype=np.float32).copy()

    def _key_nn_row(self, pair, who):
        if self.key_nn is None:
            raise RuntimeError(f"{who}: the term is off ('lambda_global_key_nn' is 0)")
        if pair is None and self.PAIR_NONE is None:
            return None
        row = self._row(self.PAIR_NONE if pair is None else pair)
        if row is None:
            raise RuntimeError(f"{who}: slot {pair} is parked (stop_compact): its value left the device with its handle")
        return row

    def key_nn_value(self, pair=None):
        """The raw nearest-neighbour key term (``lambda_global_key_nn``) of the last step that computed it, copied from
        the device (waits for the device): ``mean over the tokens of 1 - cos(k_i, b_j*(i))``, summed over the pair's zipped crops -- the
        total, word 0 of the losses row, holds ``lambda`` times it.  0 before the first such step.  One float for ``pair``, a list over the
        live slots for ``pair=None``."""
        row = self._key_nn_row(pair, "key_nn_value")
        vals = [float(v) for v in self._key_nn_host()]
        return vals if row is None else vals[row]

    def key_nn_match(self, pair=None):
        """The assignment of that step, copied from the device (waits for the device): ``(match, cos)``, an int32 and a float32 array
        ``[crops][T]`` for ``pair`` (``[slots][crops][T]`` over the live slots for ``pair=None``): ``match[c][i]`` the token of crop c of the
        target pass that key i of G(A_crop c) was pulled towards -- the lowest index among the most similar -- and ``cos`` that cosine."""
        row = self._key_nn_row(pair, "key_nn_match")
        nc, T = (min(self.n_crops_ab) if self.n_crops > 1 else 1), self.ctx_g.T
        m, c = np.zeros((self.P, nc, T), np.int32), np.zeros((self.P, nc, T), np.float32)
        _lib.check(_lib.lib().splice_step_key_nn_match(self.handle, m.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p)), "step_key_nn_match")
        return (m, c) if row is None else (m[row], c[row])

    def _key_gram_host(self):
        buf = (C.c_float * self.P)()
        _lib.check(_lib.lib().splice_step_key_gram_values(self.handle, buf), "step_key_gram_values")
        return np.frombuffer(buf, dtype=np.float32).copy()

    def key_gram_value(self, pair=None):
        """The raw key second-moment term (``lambda_global_key_gram``) of the last step that computed it, copied from
        the device (waits for the device): ``mean((G(K_x') - G(K_B'))^2)`` over the ``D * D`` entries, summed over the pair's zipped crops --
        the total, word 0 of the losses row, holds ``lambda`` times it.  0 before the first such step.  One float for ``pair``, a list over
        the live slots for ``pair=None``."""
        if self.key_gram is None:
            raise RuntimeError("key_gram_value: the term is off ('lambda_global_key_gram' is 0)")
        vals = [float(v) for v in self._key_gram_host()]
        if pair is None and self.PAIR_NONE is None:
            return vals
        row = self._row(self.PAIR_NONE if pair is None else pair)
        if row is None:
            raise RuntimeError(f"key_gram_value: slot {pair} is parked (stop_compact): its value left the device with its handle")
        return vals[row]

    def key_gram_layer_values(self, pair=None):
        """The per-layer addends of the key second-moment term over ``dino_gram_layers`` of the last step that computed
        it, copied from the device (waits for the device): a float32 array ``[n]`` for ``pair`` -- ``w_i`` times block i's raw term, the pair's
        zipped crops added in crop order; ``key_gram_value`` is their float32 sum, ascending from 0 (with one crop per pair exactly) -- a
        list of such arrays over the live slots for ``pair=None``.  Zeros before the first such step."""
        if self.key_gram_layers is None:
            raise RuntimeError("key_gram_layer_values: the term runs on one block or is off ('dino_gram_layers' is null and 'dino_gram_centered' false)")
        n = len(self.key_gram_layers[1])
        buf = (C.c_float * (self.P * n))()
        _lib.check(_lib.lib().splice_step_key_gram_layer_values(self.handle, buf), "step_key_gram_layer_values")
        return self._layer_rows(np.frombuffer(buf, dtype=np.float32).reshape(self.P, 1, n), pair, "key_gram_layer_values", "values")

    def _layer_rows(self, host, pair, who, noun):
        """The shared tail of the ``*_layer_values`` methods.  ``host``: float32 ``[P][slots][n]``, a pair's crops (slots) in crop order.  Per
        pair the slots are added per layer in float32 in slot order; then one array for ``pair``, a list over the live slots for
        ``pair=None``.  ``who`` / ``noun``: the method and what a parked slot lost, for the error text."""
        rows = []
        for slots in host:
            acc = slots[0].copy()
            for row in slots[1:]:
                acc = (acc + row).astype(np.float32)
            rows.append(acc)
        if pair is None and self.PAIR_NONE is None:
            return rows
        row = self._row(self.PAIR_NONE if pair is None else pair)
        if row is None:
            raise RuntimeError(f"{who}: slot {pair} is parked (stop_compact): its {noun} left the device with its handle")
        return rows[row]

    def ssim_layer_values(self, pair=None, entire=False):
        """The per-layer addends of the last step's structure term (``dino_ssim_layers``), copied from the device
        (waits for the current stream): a float32 array with one entry per block of the canonical list, ``w_l * mse(S_l, S*_l)`` as the
        loss kernels summed it -- ``loss_global_ssim`` (``entire=True``: ``loss_entire_ssim``) is their float32 sum in that order
        (``np_ssim_layers``), exactly so with one crop per pair.  Zeros at a step that does not compute the term.  One array for ``pair``,
        a list over the live slots for ``pair=None``."""
        if self.ssim_layers is None:
            raise RuntimeError("ssim_layer_values: the structure terms read the top block alone ('dino_ssim_layers' is null or the default)")
        if entire and self.plan_e is None:
            raise RuntimeError("ssim_layer_values: the engine has no entire-image branch")
        out = torch.zeros(len(self.ssim_layers[0]), self.P, device=self.device)
        _lib.check(_lib.lib().splice_step_ssim_layer_values(self.handle, 2 if entire else 1, _lib.ptr(out), _lib.current_stream()), "step_ssim_layer_values")
        return self._layer_rows(out.cpu().numpy().T[:, None, :], pair, "ssim_layer_values", "partials")

    def cls_layer_values(self, pair=None, entire=False):
        """The per-layer addends of the appearance term (``dino_cls_layers``) of the last step that computed it, copied
        from the device (waits for the device): a float32 array with one entry per block of the canonical list, ``w_l * mse(cls_l(generated),
        cls_l(B'))`` as the loss kernel formed it -- ``loss_global_cls`` (``entire=True``: ``loss_entire_cls``) is their float32 sum in that
        order (``np_cls_layers``), exactly so with one crop per pair; with several crops the pair's crops are added per layer in crop order.
        Zeros for a slot whose term never ran.  One array for ``pair``, a list over the live slots for ``pair=None``."""
        if self.cls_layers is None:
            raise RuntimeError("cls_layer_values: the appearance terms read the top block alone ('dino_cls_layers' is null or the default)")
        if entire and self.plan_e is None:
            raise RuntimeError("cls_layer_values: the engine has no entire-image branch")
        n = len(self.cls_layers[0])
        nc = 1 if entire or self.n_crops == 1 else min(self.n_crops_ab)
        buf = (C.c_float * (self.P * nc * n))()
        _lib.check(_lib.lib().splice_step_cls_layer_values(self.handle, 1 if entire else 0, buf, len(buf)), "step_cls_layer_values")
        return self._layer_rows(np.frombuffer(buf, dtype=np.float32).reshape(self.P, nc, n), pair, "cls_layer_values", "values")

    def id_layer_values(self, pair=None):
        """The per-layer addends of the key-identity term (``dino_id_layers``) of the last step that computed it, copied
        from the device (waits for the device): a float32 array with one entry per block of the canonical list, ``w_l * mse(k_l(G(B_crop)),
        k_l(B_crop))`` as the finish launch formed it -- ``loss_global_id_B`` is their float32 sum in that order (``np_id_layers``), exactly so
        with one crop per pair; with several crops the pair's crops are added per layer in crop order.  Zeros for a slot whose term never
        ran.  One array for ``pair``, a list over the live slots for ``pair=None``."""
        if self.id_layers is None:
            raise RuntimeError("id_layer_values: the identity term reads the top block alone ('dino_id_layers' is null or the default)")
        n = len(self.id_layers[0])
        nb = self.n_crops_ab[1]
        buf = (C.c_float * (self.P * nb * n))()
        _lib.check(_lib.lib().splice_step_id_layer_values(self.handle, buf, len(buf)), "step_id_layer_values")
        return self._layer_rows(np.frombuffer(buf, dtype=np.float32).reshape(self.P, nb, n), pair, "id_layer_values", "values")

    def active_terms(self, step_idx):
        """Per slot: which of LOSS_KEYS and IMAGE_LOSS_KEYS step ``step_idx`` computes (``engine.active_terms``; a slot's terms follow that slot's own
        lambdas).  Host arithmetic only."""
        slots = getattr(self, "P_in", self.P)
        return [active_terms(c, step_idx, self.plan_e is not None) for c in (self.cfgs if len(self.cfgs) == slots else [self.cfg] * slots)]

    # ---- the loss trace
    def loss_trace(self, pair=None):
        """The rows the steps so far wrote (``loss_trace``): per slot a float32 array ``[rows, 8]`` -- the six LOSS_KEYS values of every
        step (inactive terms are 0, as in ``losses_dev``), then the gradient norm and the clip coefficient (NaN without
        ``grad_clip_norm`` / ``grad_clip_auto``) -- with ``rows = min(step_idx + 1, n_epochs)``, cut behind a stopped slot's stop step.  One device-to-host
        copy (waits for the current stream): call it at the end of a run.  One array for ``pair``, a list over the slots for
        ``pair=None``."""
        return self._pick(self._traces(), pair)

    def _traces(self):
        if self.trace_dev is None:
            raise RuntimeError("loss_trace: no trace is kept (loss_trace is off)")
        rows = self._trace_rows()
        host = self.trace_dev[:rows].cpu().numpy()
        per = self._per_slot([host[:, i] for i in range(host.shape[1])], lambda s: s["trace"].cpu().numpy())
        stops = self._stops() if self.stop_rule[0] > 0 else [None] * len(per)
        return [per[p][:rows if k is None else min(rows, k + 1)].copy() for p, k in enumerate(stops)]

    def loss_trace_columns(self):
        """What ``losses.csv`` holds (``util.write_loss_trace``), per slot ``(rows, lrs, active)``: the slot's trace, the learning rate
        of every row from the host's schedule (the slot's own in a sweep) and the terms every row's step computed.  With the plateau
        lr rule the learning rate is the effective one, ``float32(lr) * float32(scale)`` as the loss kernel forms it, the scale of
        every step replayed on the host from the slot's ``cut_steps``."""
        traces = self._traces()
        acts = [self.active_terms(s) for s in range(max(len(r) for r in traces))]
        cuts = self._decoded(lr_records, "lr_state", "lr_cuts") if self.lr_state_dev is not None else None
        out = []
        for p, rows in enumerate(traces):
            # (a fresh recurrence: the engine's own stays where it is; a sweep that has parked slots may have left the per-pair path)
            sch = LrSchedule(self.cfgs[p] if self._pair_lr or self._parked_states() else self.cfg)
            lrs = [sch.lr(s) for s in range(len(rows))]
            if cuts is not None:
                scales = replay_lr_scales(cuts[p]["cut_steps"], len(rows), self.lr_rule[0], self.lr_rule[2])
                lrs = [float(np.float32(lr) * k) for lr, k in zip(lrs, scales)]
            out.append((rows, lrs, [acts[s][p] for s in range(len(rows))]))
        return out

    def pair_params(self, pair=0):
        """View of one pair's parameter arena (``numel`` floats)."""
        return self._pair_arena(self.params, pair, "params")

    def _pair_arena(self, arena, pair, key):
        """The ``numel`` floats of external slot ``pair`` in ``arena``, or -- the slot is parked -- its parked tensor ``key``."""
        row = self._row(pair)
        if row is None:
            return self._parked[pair][key]
        return arena[row * self.stride: row * self.stride + self.gen.numel]

    def _running_row(self, pair):
        row = self._row(pair)
        return self._parked[pair]["running"] if row is None else self.running[row]

    def pair_grads(self, pair=0):
        """(the gradient arena is scratch of a step: a parked slot has none)"""
        return self._pair_arena(self.grads, pair, "grads")

    def pair_ema(self, pair=0):
        """View of one pair's weight average (``ema_decay > 0``), laid out like ``pair_params``."""
        if self.ema is None:
            raise RuntimeError("pair_ema: no weight average is kept (ema_decay == 0)")
        return self._pair_arena(self.ema, pair, "ema")

    def generate(self, img, pair=0, track_running_stats=False, ema=False, best=False):
        """netG_pair(img) under no_grad (the logging forward of train.py:70-73); img ``[n,3,H,W]``.  The reference's net
        is in train mode there too, so the call also moves the BatchNorm running statistics: pass
        ``track_running_stats=True`` to book that (train_model does, after the step whose forwards precede it).
        ``ema=True``: the forward with the averaged weights (a plan of its own); the reference has no such call, so it never
        books BatchNorm statistics and is not among the logged forwards.  ``best=True`` (``stop_keep_best``): alike with the best
        window's weights, or with ``ema=True`` too that step's average."""
        n, _, h, w = img.shape
        # one plan per pair and weight set: a plan holds the BatchNorm statistics of its last forward until they are booked
        key = (("best", bool(ema)) if best else ("ema",) if ema else ()) + (pair, n, h, w)
        if key not in self._log_plans:
            self._log_plans[key] = GeneratorPlan(self.gen, n, h, w, False, batch_stats=n > 1)   # ONE netG call on n images: batch statistics, as nn.BatchNorm2d
        plan = self._log_plans[key]
        if best or ema:
            return plan.forward(self.pair_best(pair, ema=ema) if best else self.pair_ema(pair), img.contiguous())
        out = plan.forward(self.pair_params(pair), img.contiguous())
        if track_running_stats:
            self.book_running_stats(plan, pair)
        else:
            self._logged = [(q, k) for q, k in getattr(self, "_logged", []) if k != pair] + [(plan, pair)]
        return out

    def book_logged_forward(self):
        """Book the BatchNorm statistics of the last ``generate()`` call NOW: the reference's logging forward sits between
        the step's generator calls and the optimizer update (train.py:70-79), so ``train_model`` generates with the
        pre-update weights BEFORE the fused step and books the statistics AFTER it -- the reference's buffer order."""
        for plan, pair in getattr(self, "_logged", []):   # (every pair generated since the last booking, in call order)
            self.book_running_stats(plan, pair)
        self._logged = []

    def book_running_stats(self, plan, pair=0):
        if self._frozen(pair):   # (a slot that stopped at an earlier step: its buffers stay those of its last own step)
            return
        plans = (C.c_void_p * 1)(plan.handle)
        _lib.check(_lib.lib().splice_gen_running_stats_update(plans, 1, _lib.ptr(self._running_row(pair)), 0, 0.1, _lib.current_stream()), "running_stats_update")
        self.generator_calls[pair] += 1

    def state_dict(self, pair=0, ema=False, best=False):
        """``netG.state_dict()`` of one pair: parameters, BatchNorm running statistics and ``num_batches_tracked``.
        ``ema=True``: the averaged parameters with the live buffers; ``best=True`` (``stop_keep_best``): the best window's weights
        (its average with ``ema=True`` too) with the live buffers -- buffers are not snapshotted, the generator runs on batch statistics."""
        flat = self.pair_best(pair, ema=ema) if best else self.pair_ema(pair) if ema else self.pair_params(pair)
        out = {k: v.clone() for k, v in self.gen.unflatten(flat).items()}
        calls = self.generator_calls[pair]
        if self._frozen(pair):   # the netG calls of the steps behind its stop step did not move this slot's buffers
            step_calls = lambda k: 2 * (k + 1) + (k // int(self.cfg["entire_A_every"]) + 1 if self.plan_e is not None else 0)
            calls -= step_calls(self.step_idx) - step_calls(self._stops()[pair])
        for name, (off, cnt) in self.gen.buffer_table.items():
            out[name] = self._running_row(pair)[off:off + cnt].clone()
            if name.endswith("running_var"):
                out[name[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(calls, dtype=torch.long, device=self.device)
        return out


class SpliceEngine(MultiPairEngine):
    """The per-pair optimisation loop of ``train.py:34-80`` for ONE pair (P = 1): the reference's unit of work."""

    def __init__(self, cfg, vit_state, gen_state, crop_hw, entire_hw=None, device="cuda", vit_engine=None, n_crops=1, fp8=False):
        super().__init__(cfg, vit_state, [gen_state], crop_hw, entire_hw, device=device, vit_engine=vit_engine, n_crops=n_crops, fp8=fp8)

    PAIR_NONE = 0   # the accessors (``losses()``, ``lr_state()``, ``stopped_at``, ...) answer for the one pair, without a list


class MultiScaleEngine:
    """One pair, every loss term evaluated at SEVERAL ViT input scales (BASELINE configs[4]: 224 / 320 / 448): the same global
    crops are resized to each ``dino_global_patch_size`` in ``scales`` and the reference loss (util/losses.py:46-72) of every
    scale is summed; one update of the configured optimiser (scheduled lr) per step on the summed gradient.  An extension beyond the reference (it has one
    scale).  The generator runs ONCE per step: the first scale's engine (the leader) does the generator forward and its own
    ViT part, the other scales (followers, ``splice_step_set_phases``) run only their ViT part on the leader's images and add
    their image gradients to the leader's, then the leader backpropagates the summed image gradient through the generator
    (linear in it, so this equals the sum of the per-scale backpropagations) and the fused optimiser launch follows."""

    def __init__(self, cfg, vit_state, gen_state, crop_hw, entire_hw=None, scales=(224, 320, 448), device="cuda", vit_engine=None, n_crops=1,
                 fp8=False):
        self.cfg = dict(DEFAULT_CFG, **cfg)
        if self.cfg.get("stop_compact"):
            raise NotImplementedError("stop_compact: stopped slots leave the launches of a MultiPairEngine under its stop rule; MultiScaleEngine has one pair and no stop rule")
        if best_rule(self.cfg):
            raise NotImplementedError("stop_keep_best: the snapshot rides in the fused step's own update under its stop rule; MultiScaleEngine updates outside the step")
        self.best = None
        if trace_rule(self.cfg):
            raise NotImplementedError("loss_trace: the rows are written by a whole fused step under its own step count; MultiScaleEngine runs each scale as a phase-mode handle")
        self.trace_dev = None
        if lr_plateau_rule(self.cfg)[0] > 0:
            raise NotImplementedError("lr_plateau_factor > 0: the plateau lr rule lives in the fused step's loss kernel and its own update; MultiScaleEngine updates outside the step")
        if stop_rule(self.cfg)[0] > 0:
            raise NotImplementedError("stop_window > 0: the plateau stop rule lives in the fused step's own update; MultiScaleEngine updates outside the step")
        for key, lam in zip(IMAGE_LAMBDA_KEYS, image_terms_rule(self.cfg)):
            if lam > 0:
                raise NotImplementedError(f"{key} > 0: the term's gradient is added to a whole fused step's image gradient; MultiScaleEngine's per-scale "
                                          "follower handles add theirs into the leader's, which would count the term once per scale")
        depth = vit_engine.depth if vit_engine is not None else synth.DINO_CONFIGS[self.cfg["dino_model_name"]][2]
        for term in LAYER_LIST_TERMS:
            if layer_list_rule(term, self.cfg, depth) is not None:
                raise NotImplementedError(f"{term.keys[0]}: the layer table is set on a whole fused step; MultiScaleEngine runs each scale as a gradient-only "
                                          "or phase-mode handle, which refuses it")
        key_gram_layers_rule(self.cfg, depth)   # (a bad value is refused by name here too)
        if key_gram_rule(dict(self.cfg, dino_gram_layer=None if self.cfg.get("dino_gram_layers") is not None else self.cfg.get("dino_gram_layer")), depth) is not None:
            raise NotImplementedError("lambda_global_key_gram: the term is set on a whole fused step; MultiScaleEngine runs each scale as a gradient-only "
                                      "or phase-mode handle, which refuses it")
        if key_nn_rule(self.cfg, depth) is not None:
            raise NotImplementedError("lambda_global_key_nn: the term is set on a whole fused step; MultiScaleEngine runs each scale as a gradient-only "
                                      "or phase-mode handle, which refuses it")
        self.ema_rule = ema_rule(self.cfg)
        self.ema = None
        self.grad_clip = grad_clip_rule(self.cfg)
        self.clip_dev = None
        self.clip_auto = grad_clip_auto_rule(self.cfg)
        self.clip_auto_dev = None
        self.opt_ext = fused_optimizer_ext(self.cfg)
        self.w = None
        self.scales = tuple(scales)
        self.engines = []
        for k, sz in enumerate(self.scales):
            # (ema_decay=0, grad_clip_norm=0, grad_clip_auto=0: the handles are gradient-only, the average and the clipping ride in this engine's own update below)
            # (... and the optimiser options neutral: the extended rule rides in that update too)
            e = SpliceEngine(dict(self.cfg, dino_global_patch_size=sz, ema_decay=0.0, grad_clip_norm=0.0, grad_clip_auto=0.0, **OPTIM_EXT_DEFAULTS), vit_state if k == 0 else None, gen_state, crop_hw, entire_hw, device=device,
                             vit_engine=vit_engine if k == 0 else self.engines[0].vit, n_crops=n_crops, fp8=fp8)
            _lib.check(_lib.lib().splice_step_set_mode(e.handle, 1, 0), "step_set_mode")
            if k > 0:   # one parameter set: every scale sees the arenas of the first engine; netG bookkeeping once
                e.params, e.grads, e.m, e.v = self.engines[0].params, self.engines[0].grads, self.engines[0].m, self.engines[0].v
                _lib.check(_lib.lib().splice_step_set_running_stats(e.handle, None, 0), "step_set_running_stats")
                _lib.check(_lib.lib().splice_step_set_phases(e.handle, 2, self.engines[0].handle), "step_set_phases")
            self.engines.append(e)
        self.vit, self.gen = self.engines[0].vit, self.engines[0].gen
        self.params, self.grads = self.engines[0].params, self.engines[0].grads
        if self.ema_rule[0] > 0:
            self.ema = self.engines[0].ema = self.params.clone()   # (the leader serves pair_ema / generate / state_dict with it)
        if self.grad_clip > 0 or self.clip_auto[0] > 0:
            self.clip_dev = torch.zeros(1, 6, dtype=torch.int32, device=self.params.device)
        if self.clip_auto[0] > 0:
            self.clip_auto_dev = torch.zeros(1, 6, dtype=torch.int32, device=self.params.device)
        self.step_idx = -1
        self.opt_kind, *self.opt_hp = fused_optimizer(self.cfg)
        if optim_ext_uses(self.opt_kind, self.opt_ext)[2]:
            self.w = torch.zeros_like(self.params)
        self.schedule = LrSchedule(self.cfg)
        self.lr = None

    def clip_state(self, pair=None):
        """The gradient-clipping record of the last step, as ``SpliceEngine.clip_state``."""
        if self.clip_dev is None:
            raise RuntimeError("clip_state: the gradient is not clipped (grad_clip_norm == 0)")
        return clip_records(self.clip_dev)[0]

    def clip_auto_state(self, pair=None):
        """The record of the adaptive clipping, as ``SpliceEngine.clip_auto_state``."""
        if self.clip_auto_dev is None:
            raise RuntimeError("clip_auto_state: the gradient is not clipped against its running norm (grad_clip_auto == 0)")
        return clip_auto_records(self.clip_auto_dev)[0]

    def step(self, A_crop, B_crop, A_entire=None):
        from .generator import optim_step
        self.step_idx += 1
        e0, L = self.engines[0], _lib.lib()
        _lib.check(L.splice_step_set_phases(e0.handle, 1 | 2, None), "step_set_phases")
        e0.step(A_crop, B_crop, A_entire)                    # G forward, the leader's ViT part
        for e in self.engines[1:]:
            e.step(A_crop, B_crop, A_entire)                 # the other scales' ViT parts: d(images) += ...
        _lib.check(L.splice_step_set_phases(e0.handle, 4, None), "step_set_phases")
        e0.step(A_crop, B_crop, A_entire, _repeat=True)      # G backward of the summed image gradient
        self.lr = self.schedule.lr(self.step_idx)
        # (the adaptive clipping's regime is baked into the fused step's graph variants; here the host step index gives it)
        entire = e0.plan_e is not None and self.step_idx % self.cfg["entire_A_every"] == 0
        optim_step(self.opt_kind, e0.params, e0.grads, e0.m, e0.v, self.lr, *self.opt_hp, self.step_idx + 1, ema=self.ema,
                   ema_decay=self.ema_rule[0], ema_start=self.ema_rule[1], clip_norm=self.grad_clip, clip_state=self.clip_dev,
                   clip_auto=self.clip_auto if self.clip_auto[0] > 0 else None, clip_regime=clip_regime(self.step_idx, self.cfg["cls_warmup"], entire),
                   clip_auto_state=self.clip_auto_dev, ext=self.opt_ext, w=self.w)

    def losses(self):
        """Per-scale loss dicts and their sum: ``{"loss": total, "scales": {224: {...}, ...}}``."""
        per = {sz: e.losses() for sz, e in zip(self.scales, self.engines)}
        return {"loss": sum(d["loss"] for d in per.values()), "scales": per}

    def generate(self, img, pair=0, track_running_stats=False, ema=False, best=False):
        return self.engines[0].generate(img, pair, track_running_stats, ema=ema, best=best)

    def pair_ema(self, pair=0):
        return self.engines[0].pair_ema(pair)

    def book_logged_forward(self):
        self.engines[0].book_logged_forward()

    def snapshot(self, pair=0, device=None):
        raise NotImplementedError("snapshot: the run state of a MultiScaleEngine is spread over one phase-mode handle per scale and an update outside the step; "
                                  "pair snapshots are a MultiPairEngine / SpliceEngine feature")

    def restore(self, states):
        raise NotImplementedError("restore: the run state of a MultiScaleEngine is spread over one phase-mode handle per scale and an update outside the step; "
                                  "pair snapshots are a MultiPairEngine / SpliceEngine feature")

    stopped_at = None   # (no stop rule here)
    lr_rule = (0.0, 1, 0.0)   # (nor the plateau lr rule)
    lr_scale = 1.0

    def window_closes(self, step_idx):
        return False

    def state_dict(self, pair=0, ema=False, best=False):
        return self.engines[0].state_dict(pair, ema=ema, best=best)


def synthetic_engine(cfg, pair_id=0, hw=(224, 224), seed=1234, device="cuda", vit_engine=None, entire=True, pairs=1, fp8=False, top_cls_only=True, crop_hw=None):
    """Engine + inputs for the BASELINE benchmark configs: seeded synthetic ViT weights, xavier generator init and U[0,1)
    pairs.  ``pairs`` > 1: pairs ``pair_id .. pair_id + pairs - 1`` side by side on one engine
    (inputs ``[P,3,h,w]``); ``pairs == 1``: the single-pair ``SpliceEngine`` with ``[3,h,w]`` inputs.
    ``crop_hw``: the global crops are the top-left ``crop_hw`` window of the ``hw`` images (the reference's default shape: 900 x 900 crops of
    900 x 1200 images, every crop resized to ``dino_global_patch_size``); the return value then carries the entire image as a fourth entry."""
    if crop_hw is not None and pairs != 1:
        raise ValueError("crop_hw: one pair per engine")
    c = dict(DEFAULT_CFG, **cfg)
    vit_state = None if vit_engine is not None else synth.vit_params(seed, c["dino_model_name"], img_size=c["dino_global_patch_size"])
    ids = [pair_id + k for k in range(pairs)]
    gen_states = [synth.generator_params(seed + 1 + i, c["init_gain"]) for i in ids]
    imgs = [synth.image_pair(seed, i, hw[0], hw[1]) for i in ids]
    ent = hw if entire else None
    if pairs > 1:
        eng = MultiPairEngine(c, vit_state, gen_states, hw, ent, device=device, vit_engine=vit_engine, fp8=fp8, top_cls_only=top_cls_only)
        return eng, torch.from_numpy(np.stack([a for a, _ in imgs])).to(device), torch.from_numpy(np.stack([b for _, b in imgs])).to(device)
    eng = SpliceEngine(c, vit_state, gen_states[0], crop_hw or hw, ent, device=device, vit_engine=vit_engine, fp8=fp8)
    A, B = torch.from_numpy(imgs[0][0]).to(device), torch.from_numpy(imgs[0][1]).to(device)
    if crop_hw is None:
        return eng, A, B
    return eng, A[:, :crop_hw[0], :crop_hw[1]].contiguous(), B[:, :crop_hw[0], :crop_hw[1]].contiguous(), A
