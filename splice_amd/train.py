"""Drop-in for ``train.py``: ``train_model(dataroot, callback=None)``.

Same contract as the reference (``train.py:15-80``): reads ``conf/default/config.yaml`` from the
working directory (falling back to the packaged copy), seeds python / numpy / torch, opens the first
image of ``<dataroot>/A`` and ``<dataroot>/B``, runs ``n_epochs`` optimisation steps and every
``log_images_freq`` steps writes ``<dataroot>/out/output.png`` (asynchronously: ``util.AsyncResultWriter``) and calls
``callback(output[0])`` with the ``[3,H,W]`` float image.  With ``loss_trace`` (an extension) the run ends by writing
``<dataroot>/out/losses.csv``, one line per step, from rows its own kernels kept on the device.  With ``ema_decay > 0`` (an extension) the run ends by writing one more image,
``<dataroot>/out/output_ema.png``, from the averaged weights; with ``stop_keep_best`` (an extension of the stop rule) ``output_best.png``,
from the weights of the step that closed the best window.  With ``checkpoint_every`` K > 0 (an extension) every K-th step leaves
``<dataroot>/out/checkpoint.pt``, and ``resume: true`` continues a run from it, bit for bit.  The step itself is the fused HIP engine (``SpliceEngine``), one host
call per step, losses read back only when a progress line is printed.

Data feed: the reference augments PIL images on the CPU every step (``data/Dataset.py:62-70``).
Here the images live on the GPU and the same pipelines run on device tensors (``splice_amd/augment.py``):
structure image = h-flip(0.5), ColorJitter(.4,.4,.2,.1)@0.5, GaussianBlur(3)@0.2; texture image = h-flip(0.5);
then one random square crop covering >= ``min_cover`` of the height (``data/transforms.py:7-41``).
"""
import json
import os
import random
from argparse import ArgumentParser

import numpy as np
import torch
import yaml

from . import augment
from .engine import SpliceEngine
from .util import AsyncResultWriter, write_loss_trace

device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')
_PKG_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "conf", "default", "config.yaml")



def fp8_mode(cfg):
    """Engine ``fp8`` argument of the config key ``fp8`` (one meaning everywhere: ``splice_amd.vit.fp8_mode``): False -- bf16;
    True / ``"gemm"`` -- e4m3 operands for the QKV / fc1 / fc2 projections and the self-similarity Gram matrices (the fastest
    measured setting); ``"attention"`` / ``"all"`` -- the attention forward in e4m3 as well (BASELINE configs[4] as written)."""
    from .vit import fp8_mode as _mode
    return _mode(cfg.get('fp8', False))


def _load_image(path, resize):
    from PIL import Image
    img = Image.open(path).convert('RGB')
    if resize and resize > 0:   # transforms.Resize(int) on a PIL image: shorter edge -> resize, bilinear
        w, h = img.size
        short, long = (w, h) if w <= h else (h, w)
        if short != resize:
            ns, nl = resize, int(resize * long / short)
            img = img.resize((ns, nl) if w <= h else (nl, ns), Image.BILINEAR)
    arr = np.asarray(img, dtype=np.float32) / 255.0          # ToTensor
    return torch.from_numpy(arr).permute(2, 0, 1).contiguous()


def _first_file(d):
    return os.path.join(d, os.listdir(d)[0])


_VIT_ENGINES = {}


def _release_process_caches():
    """Interpreter exit: free the process-wide ViT engine (weights, contexts, captured graphs) while the interpreter and the HIP
    runtime are still whole -- left to module teardown, its destructor runs in an arbitrary order against `_lib` and torch."""
    try:
        _VIT_ENGINES.clear()
        if torch.cuda.is_available():
            torch.cuda.synchronize()
    except Exception:
        pass


import atexit
atexit.register(_release_process_caches)


def _shared_vit_engine(model_name, who):
    """The frozen DINO ViT of this process: loaded / packed once per (weight source, model) and shared by every run that follows
    (a batch worker optimises many pairs; reading and packing 86 M parameters per pair was 2 s of a 12 s run).  Weight
    source: ``SPLICE_DINO_CHECKPOINT=<dino .pth>`` or ``SPLICE_SYNTHETIC_WEIGHTS=1`` (seeded stand-in weights)."""
    from .vit import VitEngine
    ckpt = os.environ.get("SPLICE_DINO_CHECKPOINT")
    if ckpt:
        key = ("checkpoint", os.path.abspath(ckpt), os.path.getmtime(ckpt), model_name)
    elif os.environ.get("SPLICE_SYNTHETIC_WEIGHTS") == "1":
        key = ("synthetic", model_name)
    else:
        raise RuntimeError(f"{who}: no DINO weights (set SPLICE_DINO_CHECKPOINT=<dino .pth>, pass vit_state=..., "
                           "or SPLICE_SYNTHETIC_WEIGHTS=1); the reference's torch.hub download is not available here")
    if key not in _VIT_ENGINES:
        if ckpt:
            from .checkpoint import load_dino_checkpoint
            _, state = load_dino_checkpoint(ckpt, model_name)
        else:
            from . import synth
            state = synth.vit_params(1234, model_name, img_size=224)
        _VIT_ENGINES.clear()   # one resident weight set per process
        _VIT_ENGINES[key] = VitEngine(model_name, device=device).load_state_dict(state)
    return _VIT_ENGINES[key]


class DeviceDataFeed:
    """GPU-side counterpart of ``SingleImageDataset`` (data/Dataset.py:12-73)."""

    def __init__(self, cfg, A, B):
        self.cfg, self.A, self.B = cfg, A.to(device), B.to(device)
        self.step = -1

    def get_A(self):
        return self.A[None]

    @staticmethod
    def _crops(img, min_cover, n_crops):
        """``[n_crops,3,s,s]``: one size per call, one position per crop (data/transforms.py:19-27)."""
        _, h, w = img.shape
        size, boxes = augment.global_crop_boxes(h, w, min_cover, n_crops)
        return torch.stack([img[:, top:top + size, left:left + size] for top, left in boxes]).contiguous()

    def next(self):
        self.step += 1
        aug = bool(self.cfg['use_augmentations'])
        sample = {'step': self.step}
        if self.step % self.cfg['entire_A_every'] == 0:
            sample['A'] = self.get_A()
        # data/Dataset.py:67-68: augment the whole image, then crop
        A = augment.structure_transforms(self.A) if aug else self.A
        sample['A_global'] = self._crops(A, self.cfg['global_A_crops_min_cover'], self.cfg['global_A_crops_n_crops'])
        B = augment.texture_transforms(self.B) if aug else self.B
        sample['B_global'] = self._crops(B, self.cfg['global_B_crops_min_cover'], self.cfg['global_B_crops_n_crops'])
        return sample


def _load_cfg(dataroot, cfg_overrides):
    cfg_path = "conf/default/config.yaml" if os.path.exists("conf/default/config.yaml") else _PKG_CFG
    with open(cfg_path, "r") as f:
        cfg = yaml.safe_load(f)
    if dataroot is not None:
        cfg['dataroot'] = dataroot
    cfg.update(cfg_overrides or {})
    return cfg


def _seed_host(seed):
    """Seeds python and numpy (``-1``: with a drawn seed) and returns the seed; torch is the caller's business."""
    if seed == -1:
        seed = np.random.randint(2 ** 32 - 1, dtype=np.int64)
    random.seed(int(seed))
    np.random.seed(int(seed) % (2 ** 32))
    return seed


def _load_pair(root, cfg):
    A = _load_image(_first_file(os.path.join(root, 'A')), cfg['A_resize'])
    B = _load_image(_first_file(os.path.join(root, 'B')), cfg['B_resize'])
    return (B, A) if cfg['direction'] == 'BtoA' else (A, B)


def _crop_max(A, B):
    return max(min(A.shape[1], A.shape[2]), min(B.shape[1], B.shape[2]))   # crops are squares of side <= min(h, w)


def _one_scale(cfg):
    """``dino_global_scales`` with one entry is the ViT input size, the reference's ``dino_global_patch_size``."""
    if cfg.get('dino_global_scales'):
        cfg['dino_global_patch_size'] = int(cfg['dino_global_scales'][0])


def _init_generator(cfg):
    """The parameters of ``define_G(init_type, init_gain)``, drawn from the torch RNG as it stands."""
    from .networks import define_G
    netG = define_G(cfg['init_type'], cfg['init_gain'], device=device)
    return {k: v.detach().clone() for k, v in netG.state_dict().items() if k in netG.engine.table}


CHECKPOINT_NAME = "checkpoint.pt"


def save_checkpoint(path, engine, feed, epoch):
    """One file that continues the run (``checkpoint_every``): the host snapshot of every slot, the feed's step and
    the states of ``random``, NumPy and torch's CPU and CUDA generators, as they stand after ``epoch`` steps.  Written to a temporary
    file and moved into place: a reader finds the old file or the new one.  The copies wait for the device: a stall per checkpoint."""
    slots = getattr(engine, "P_in", getattr(engine, "P", 1))
    state = {"format": 1, "epoch": int(epoch), "states": [engine.snapshot(p, device="cpu") for p in range(slots)],
             "feed_step": getattr(feed, "step", None),
             "rng": {"python": random.getstate(), "numpy": np.random.get_state(), "torch": torch.get_rng_state(),
                     "cuda": torch.cuda.get_rng_state_all() if torch.cuda.is_available() else []}}
    tmp = path + ".tmp"
    torch.save(state, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, engine, feed):
    """Continue from ``save_checkpoint``'s file: restores every slot of the fresh ``engine`` (``engine.restore``: a file written under
    another config is refused by the name of the key), the feed's step and the random generators; returns the number of steps done."""
    state = torch.load(path, map_location="cpu", weights_only=False)
    if not isinstance(state, dict) or state.get("format") != 1:
        raise ValueError(f"{path}: not a checkpoint of format 1")
    engine.restore(state["states"])
    if feed is not None and state["feed_step"] is not None:
        feed.step = state["feed_step"]
    rng = state["rng"]
    random.setstate(rng["python"])
    np.random.set_state(rng["numpy"])
    torch.set_rng_state(rng["torch"])
    if rng["cuda"] and torch.cuda.is_available():
        torch.cuda.set_rng_state_all(rng["cuda"])
    return int(state["epoch"])


def _optimise(cfg, engine, next_inputs, As, writers, callback, progress, single=False, feed=None):
    """The optimisation loop of every entry point, and the end of a run: ``cfg['n_epochs']`` steps of ``engine`` on the crops
    ``next_inputs()`` returns (the arguments of ``engine.step``); every ``log_images_freq`` steps one image per slot from ``As`` goes to
    the slot's writer and to ``callback(slot, image)``.  ``single``: the engine is a one-pair engine (one loss in the progress line, and
    the stop is announced).  Closes the writers.
    ``checkpoint_every`` K > 0: after every K-th step ``checkpoint.pt`` is written beside the first slot's ``output.png``
    (``save_checkpoint``; ``feed``: the data feed whose step it keeps); ``resume``: a run that finds the file continues behind the step it
    holds, bit for bit as the run that wrote it would have."""
    from .engine import checkpoint_rule
    n_epochs, freq = cfg['n_epochs'], cfg['log_images_freq']
    every, resume = checkpoint_rule(cfg)
    ckpt = os.path.join(writers[0].dir, CHECKPOINT_NAME) if every or resume else None
    done = 0
    try:
        if resume and os.path.exists(ckpt):
            done = load_checkpoint(ckpt, engine, feed)
            if progress:
                print(f"resuming behind epoch {done} from {ckpt}")
        for epoch in range(done + 1, n_epochs + 1):
            inputs = next_inputs()
            log = epoch % freq == 0
            # train.py:70-76 generates the logged image between the loss and backward(): with the weights of epoch - 1
            # updates.  The fused step updates in place, so the images are generated BEFORE it (same weights) ...
            outputs = [engine.generate(A, pair=p) for p, A in enumerate(As)] if log else None
            engine.step(*inputs)
            if log:
                engine.book_logged_forward()   # ... and their BatchNorm bookkeeping lands AFTER the step's, as in the reference
                for p, out in enumerate(outputs):
                    # (out/output.png is overwritten every time: intermediate images may be skipped when they come faster than the writer's interval, the last one never)
                    writers[p].submit(out[0], force=epoch + freq > n_epochs)
                    if callback is not None:
                        callback(p, out[0])
            if progress and (epoch % 50 == 0 or epoch == 1):
                losses = f"{engine.losses()['loss']:.4f}" if single else ", ".join(f"{d['loss']:.4f}" for d in engine.losses())
                # (the plateau lr rule: the factor the loss kernel multiplies that lr by, the host's copy of the last closed window)
                scale = f" lr_scale={engine.lr_scale}" if getattr(engine, "lr_rule", (0,))[0] > 0 else ""
                print(f"Epoch {epoch}: loss={losses} lr={engine.lr}{scale}")
            if every and epoch % every == 0:
                save_checkpoint(ckpt, engine, feed, epoch)
            # the plateau stop rule (stop_window > 0; decided on the device): the host asks only after a step that closes a window -- no
            # other step can stop a slot -- and ends the run, once every slot has stopped, with an image of each slot's final parameters
            if engine.window_closes(engine.step_idx) and engine.all_stopped():
                for p, A in enumerate(As):
                    out = engine.generate(A, pair=p)
                    writers[p].submit(out[0], force=True)
                    if callback is not None:
                        callback(p, out[0])
                if single and progress:
                    print(f"Epoch {epoch}: the loss has plateaued, stopping")
                break
        _ema_images(engine, writers, As)
        _best_images(engine, writers, As)
        _loss_traces(cfg, engine, writers)
    finally:
        for w in writers:   # PNG encode + disk write happen on a worker thread
            w.close()


def train_model(dataroot, callback=None, cfg_overrides=None, vit_state=None, progress=True):
    cfg = _load_cfg(dataroot, cfg_overrides)
    n_crops = (int(cfg['global_A_crops_n_crops']), int(cfg['global_B_crops_n_crops']))
    if not all(1 <= n <= 8 for n in n_crops):
        raise NotImplementedError("the fused engine takes 1..8 global crops per image (global_{A,B}_crops_n_crops)")
    if n_crops[0] == n_crops[1]:
        n_crops = n_crops[0]   # (unequal counts: the reference zips the crop lists, util/losses.py:76,87,98 -- so does the engine)
    if device.type != 'cuda':
        raise RuntimeError("train_model needs an MI355X: the product path has no CPU fallback")

    seed = _seed_host(cfg['seed'])
    torch.manual_seed(int(seed))
    print(f'running with seed: {seed}.')

    A, B = _load_pair(cfg['dataroot'], cfg)
    print("Image sizes %s and %s" % (str((A.shape[2], A.shape[1])), str((B.shape[2], B.shape[1]))))
    feed = DeviceDataFeed(cfg, A, B)

    vit_engine = None if vit_state is not None else _shared_vit_engine(cfg['dino_model_name'], "train_model")
    gen_state = _init_generator(cfg)   # exactly as define_G(init_type, init_gain): xavier-normal from the torch RNG seeded above
    # Extensions beyond the reference's config (BASELINE configs[4]): `dino_global_scales` = list of ViT input sizes at which every
    # loss term is evaluated each step (the reference has the single `dino_global_patch_size`), `fp8` = e4m3 operands for the
    # QKV / fc1 / fc2 projections and the self-similarity Gram matrices.  Absent keys = the reference's behaviour.
    scales = [int(x) for x in (cfg.get('dino_global_scales') or [])]
    crops, entire = (_crop_max(A, B),) * 2, tuple(A.shape[1:])
    if len(scales) > 1:
        from .engine import MultiScaleEngine, checkpoint_rule
        if any(checkpoint_rule(cfg)):
            raise NotImplementedError("checkpoint_every / resume: a MultiScaleEngine has no pair snapshots (dino_global_scales with several entries)")
        engine = MultiScaleEngine(cfg, vit_state, gen_state, crops, entire, scales=scales, device=device, n_crops=n_crops, vit_engine=vit_engine, fp8=fp8_mode(cfg))
    else:
        _one_scale(cfg)
        engine = SpliceEngine(cfg, vit_state, gen_state, crops, entire, device=device, n_crops=n_crops, vit_engine=vit_engine, fp8=fp8_mode(cfg))

    def next_inputs():
        inputs = feed.next()
        return inputs['A_global'], inputs['B_global'], inputs['A'][0] if 'A' in inputs else None
    _optimise(cfg, engine, next_inputs, [feed.get_A()], [AsyncResultWriter(cfg['dataroot'])], callback and (lambda p, image: callback(image)), progress, single=True,
              feed=feed)
    return engine


class PairBatchFeed:
    """Device data feed of P pairs that share image sizes: per step ONE crop size per side (A / B), as ``Global_crops`` draws it
    (data/transforms.py:21), and ``global_{A,B}_crops_n_crops`` random positions per pair; augmentations once per pair image, before
    cropping (data/Dataset.py:67-68, as ``DeviceDataFeed``).  Every pair sees the reference's marginal distribution of crops; the sizes
    are shared so that the crops stack into one ``[P*n,3,s,s]`` batch, pair-major (pair p's crops are rows ``[p*n, (p+1)*n)``)."""

    def __init__(self, cfg, As, Bs, device=device):
        if len({tuple(a.shape) for a in As}) != 1 or len({tuple(b.shape) for b in Bs}) != 1:
            raise ValueError("pairs optimised side by side must share the structure-image size and the appearance-image size")
        self.cfg, self.A, self.B = cfg, [a.to(device) for a in As], [b.to(device) for b in Bs]
        self.n_crops = (int(cfg.get('global_A_crops_n_crops', 1)), int(cfg.get('global_B_crops_n_crops', 1)))
        self.step = -1

    def get_A(self, pair):
        return self.A[pair][None]

    def _crops(self, imgs, min_cover, n):
        _, h, w = imgs[0].shape
        size, boxes = augment.global_crop_boxes(h, w, min_cover, len(imgs) * n)
        return torch.stack([imgs[k // n][:, t:t + size, l:l + size] for k, (t, l) in enumerate(boxes)]).contiguous()

    def next(self):
        self.step += 1
        aug = bool(self.cfg['use_augmentations'])
        sample = {'step': self.step}
        if self.step % self.cfg['entire_A_every'] == 0:
            sample['A'] = torch.stack(self.A).contiguous()
        sample['A_global'] = self._crops([augment.structure_transforms(a) if aug else a for a in self.A], self.cfg['global_A_crops_min_cover'], self.n_crops[0])
        sample['B_global'] = self._crops([augment.texture_transforms(b) if aug else b for b in self.B], self.cfg['global_B_crops_min_cover'], self.n_crops[1])
        return sample


def _ema_images(engine, writers, As):
    """The end of a run that keeps a weight average (``ema_decay > 0``), however it ended: one more image per slot,
    ``output_ema.png`` beside ``output.png``, from the averaged weights.  No callback and no bookkeeping: the logged images stay
    those of the live weights."""
    if engine.ema is None or engine.step_idx < 0:
        return
    for p, A in enumerate(As):
        writers[p].submit(engine.generate(A, pair=p, ema=True)[0], force=True, name="output_ema.png")


def _best_images(engine, writers, As):
    """The end of a run that keeps the best window's weights (``stop_keep_best``), however it ended: one more image per slot,
    ``output_best.png`` beside ``output.png``, from the weights of the step that closed the best window -- and with a weight average
    ``output_best_ema.png`` from that step's average.  No callback and no bookkeeping, as ``_ema_images``."""
    if getattr(engine, "best", None) is None or engine.step_idx < 0:
        return
    for p, A in enumerate(As):
        writers[p].submit(engine.generate(A, pair=p, best=True)[0], force=True, name="output_best.png")
        if engine.best_ema is not None:
            writers[p].submit(engine.generate(A, pair=p, best=True, ema=True)[0], force=True, name="output_best_ema.png")


def _loss_traces(cfg, engine, writers):
    """The end of a run that keeps a loss trace (``loss_trace``), however it ended: ``losses.csv`` beside every slot's ``output.png``,
    one line per step the slot ran (``util.write_loss_trace``).  The one device-to-host copy of the curve."""
    if not cfg.get('loss_trace', False) or engine.step_idx < 0:
        return
    for w, (rows, lrs, active) in zip(writers, engine.loss_trace_columns()):
        write_loss_trace(os.path.join(w.dir, "losses.csv"), rows, lrs, active, engine.grad_clip > 0 or getattr(engine, "clip_auto", (0.0,))[0] > 0)


def trace_fields(engine, out_dir=""):
    """What ``result.json`` / ``variant.json`` say about the loss trace of a run: ``loss_trace``, the file's name below ``out/``
    (``out_dir``: the variant's directory there).  Without the option: nothing."""
    if getattr(engine, "trace_dev", None) is None or engine.step_idx < 0:
        return {}
    return {"loss_trace": os.path.join(out_dir, "losses.csv")}


def lr_fields(engine, slot=None):
    """What ``result.json`` / ``variant.json`` say about the plateau lr rule of a run: ``lr_plateau_factor`` (0: the rule was off), and
    for ``slot`` (None: the one pair of the engine) ``lr_cuts``, ``lr_cut_steps`` -- the step index of every cut -- and ``lr_scale``,
    the factor the slot's lr ended at."""
    factor = getattr(engine, "lr_rule", (0.0,))[0]
    if getattr(engine, "lr_state_dev", None) is None or engine.step_idx < 0:
        return {"lr_plateau_factor": factor, "lr_cuts": 0, "lr_cut_steps": [], "lr_scale": 1.0}
    rec = engine.lr_state(0 if slot is None else slot)
    return {"lr_plateau_factor": factor, "lr_cuts": rec["cuts"], "lr_cut_steps": list(rec["cut_steps"]), "lr_scale": float(rec["scale"])}


def optim_fields(engine):
    """What ``result.json`` / ``variant.json`` say about the optimiser of a run (shared by the slots): ``optimizer``, and every
    ``optimizer_*`` option (``util.OPTIM_EXT_DEFAULTS``) the run set to another value than its default."""
    from .util import OPTIM_EXT_DEFAULTS
    cfg = getattr(engine, "cfg", None) or {}
    return {"optimizer": cfg.get("optimizer", "adam"), **{k: cfg[k] for k, d in OPTIM_EXT_DEFAULTS.items() if k in cfg and cfg[k] != d}}


def image_terms_fields(engine):
    """What ``result.json`` / ``variant.json`` say about the image-space loss terms of a run (shared by the slots; DESIGN.md section
    9j): ``lambda_global_tv`` / ``lambda_global_pixel_identity`` where the run set them to another value than 0."""
    from .engine import IMAGE_LAMBDA_KEYS
    cfg = getattr(engine, "cfg", None) or {}
    return {k: cfg[k] for k in IMAGE_LAMBDA_KEYS if cfg.get(k, 0) != 0}


def layer_list_fields(engine, only=None):
    """What ``result.json`` / ``variant.json`` say about the blocks of the structure, appearance and key-identity terms of a run (shared by
    the slots; ``rules.LAYER_LIST_TERMS``, DESIGN.md sections 9k, 9l, 9m): a term's two config keys -- ``dino_ssim_layers`` /
    ``dino_ssim_layer_weights`` and so on -- in canonical order where the run named other blocks than the default.  ``only``: the engine
    attribute of the one term to report (None: all three)."""
    from .rules import LAYER_LIST_TERMS
    out = {}
    for term in LAYER_LIST_TERMS:
        rule = getattr(engine, term.attr, None) if only in (None, term.attr) else None
        if rule is not None:
            out.update(zip(term.keys, (list(rule[0]), list(rule[1]))))
    return out


def ssim_layers_fields(engine):
    return layer_list_fields(engine, "ssim_layers")


def cls_layers_fields(engine):
    return layer_list_fields(engine, "cls_layers")


def id_layers_fields(engine):
    return layer_list_fields(engine, "id_layers")


def key_gram_fields(engine):
    """What ``result.json`` / ``variant.json`` say about the key second-moment appearance term of a run (shared by the slots; DESIGN.md
    section 9n): ``lambda_global_key_gram`` and the block it ran on, ``dino_gram_layer``, where the term was on."""
    rule = getattr(engine, "key_gram", None)
    listed = getattr(engine, "key_gram_layers", None)   # (the list, its weights and the centred flag in place of the block)
    if rule is not None and listed is not None:
        return {"lambda_global_key_gram": listed[0], "dino_gram_layers": list(listed[1]), "dino_gram_layer_weights": list(listed[2]), "dino_gram_centered": listed[3]}
    return {} if rule is None else {"lambda_global_key_gram": rule[0], "dino_gram_layer": rule[1]}


def key_nn_fields(engine):
    """What ``result.json`` / ``variant.json`` say about the nearest-neighbour key appearance term of a run (shared by the slots; DESIGN.md
    section 9p): ``lambda_global_key_nn`` and the block it ran on, ``dino_nn_layer``, where the term was on."""
    rule = getattr(engine, "key_nn", None)
    return {} if rule is None else {"lambda_global_key_nn": rule[0], "dino_nn_layer": rule[1]}


def best_fields(engine, slot=None):
    """What ``result.json`` says about the stop rule's windows (``splice_amd.batch``) of a run with ``stop_keep_best``: ``best_step`` (the
    step whose weights ``output_best.png`` shows; None: no window closed, they are the initial weights), ``best_window_mean`` and
    ``window_means``, the means of the windows the slot closed while it ran.  Without the option: nothing."""
    if getattr(engine, "best", None) is None or engine.step_idx < 0:
        return {}
    rec = engine.best_state(0 if slot is None else slot)
    means = engine.window_means(0 if slot is None else slot)
    return {"best_step": rec["best_step"], "best_window_mean": rec["best_mean"], "window_means": [float(x) for x in means]}


def clip_fields(engine, slot=None):
    """What ``result.json`` says about the gradient clipping of a run (``splice_amd.batch``): ``grad_clip_norm`` (0: the gradient was
    not clipped), and for ``slot`` (None: the one pair of the engine) ``clipped_steps`` -- steps whose gradient norm exceeded it --
    and ``skipped_steps`` -- steps whose norm was not finite and did not update the slot.  A run that clipped against the slot's own
    running norm (``grad_clip_auto > 0``) also says ``grad_clip_auto`` and ``clip_ref``, the two running norms it ended with (ordinary
    and entire-image steps); ``clipped_steps`` then counts the steps either threshold clipped."""
    auto = {}
    if getattr(engine, "clip_auto_dev", None) is not None:
        ref = engine.clip_auto_state(slot)["ref"] if engine.step_idx >= 0 else [0.0, 0.0]
        auto = {"grad_clip_auto": engine.clip_auto[0], "clip_ref": [float(x) for x in ref]}
    if engine.clip_dev is None or engine.step_idx < 0:
        return {"grad_clip_norm": engine.grad_clip, "clipped_steps": 0, "skipped_steps": 0, **auto}
    rec = engine.clip_state(slot)
    return {"grad_clip_norm": engine.grad_clip, "clipped_steps": rec["clipped"], "skipped_steps": rec["skipped"], **auto}


def train_pairs(dataroots, callback=None, cfg_overrides=None, vit_state=None, progress=True):
    """``train_model`` for P pairs on ONE GPU in the same kernel launches (``MultiPairEngine``): P independent optimisations that
    share only the frozen ViT -- the throughput form of the reference's one-pair-per-process loop (train.py:34-80).  ``dataroots``:
    P directories with ``A/`` and ``B/``; all structure images must share one size and all appearance images one size
    (``A_resize`` / ``B_resize`` apply).  Every pair's generator is initialised as its own ``train_model`` run would
    (the seed is re-applied before each ``define_G``); writes ``<dataroot>/out/output.png`` per pair; ``callback(pair, image)``.
    ``global_{A,B}_crops_n_crops`` (1..8, equal or not) run as one netG call per pair's crops (at most 32 images per side).
    With deterministic full crops (``use_augmentations: False``, ``min_cover: 1``) the result of every pair is bit-identical to
    its single ``train_model`` run.  With ``stop_compact`` (and the stop rule) pairs that have stopped leave the launches; every file
    the run writes stays the same.  ``checkpoint_every`` / ``resume``: as ``train_model``, the file in the first pair's ``out/``."""
    from .engine import MAX_GROUP_IMAGES, MultiPairEngine
    cfg = _load_cfg(None, cfg_overrides)
    n_crops = (int(cfg['global_A_crops_n_crops']), int(cfg['global_B_crops_n_crops']))
    if not all(1 <= n <= 8 for n in n_crops):
        raise NotImplementedError("train_pairs: the fused engine takes 1..8 global crops per image (global_{A,B}_crops_n_crops)")
    if len(dataroots) * max(n_crops) > MAX_GROUP_IMAGES:
        raise NotImplementedError(f"train_pairs: {len(dataroots)} pairs x {max(n_crops)} global crops = {len(dataroots) * max(n_crops)} images per side, "
                                  f"at most {MAX_GROUP_IMAGES} (global_{{A,B}}_crops_n_crops)")
    if len(cfg.get('dino_global_scales') or []) > 1:
        raise NotImplementedError("train_pairs: dino_global_scales with several entries is a single-pair option (train_model / MultiScaleEngine); "
                                  "grouped pairs would silently train single-scale")
    if device.type != 'cuda':
        raise RuntimeError("train_pairs needs an MI355X: the product path has no CPU fallback")
    seed = _seed_host(cfg['seed'])
    print(f'running {len(dataroots)} pairs with seed: {seed}.')
    As, Bs = zip(*[_load_pair(root, cfg) for root in dataroots])
    feed = PairBatchFeed(cfg, As, Bs)
    vit_engine = None if vit_state is not None else _shared_vit_engine(cfg['dino_model_name'], "train_pairs")
    gen_states = []
    for _ in dataroots:
        torch.manual_seed(int(seed))     # every pair starts as its own train_model run would
        gen_states.append(_init_generator(cfg))
    torch.manual_seed(int(seed))
    _one_scale(cfg)
    engine = MultiPairEngine(cfg, vit_state, gen_states, (_crop_max(As[0], Bs[0]),) * 2, tuple(As[0].shape[1:]), device=device, vit_engine=vit_engine, fp8=fp8_mode(cfg),
                             n_crops=n_crops[0] if n_crops[0] == n_crops[1] else n_crops)

    def next_inputs():
        inputs = feed.next()
        return inputs['A_global'], inputs['B_global'], inputs.get('A')
    _optimise(cfg, engine, next_inputs, [feed.get_A(p) for p in range(len(dataroots))], [AsyncResultWriter(root) for root in dataroots], callback, progress, feed=feed)
    return engine


def _sweep_checks(cfg, variants):
    """Host-side refusals of ``train_sweep`` (before anything touches the GPU); returns the per-slot configs."""
    from .engine import merge_pair_cfgs
    if int(cfg['global_A_crops_n_crops']) != 1 or int(cfg['global_B_crops_n_crops']) != 1:
        raise NotImplementedError("train_sweep: a sweep takes one global crop per image (global_{A,B}_crops_n_crops > 1 is not supported)")
    if len(cfg.get('dino_global_scales') or []) > 1:
        raise NotImplementedError("train_sweep: dino_global_scales with several entries is not supported (the slots of a sweep share one ViT scale)")
    return merge_pair_cfgs(cfg, variants)


def train_sweep(dataroot, variants, cfg_overrides=None, vit_state=None, callback=None, progress=True):
    """One pair, K settings (``variants``: K dicts of per-slot overrides, ``engine.PAIR_KEYS``: the loss weights, lr and its
    schedule, seed / init_type / init_gain) optimised side by side in ONE ``MultiPairEngine``.  Every slot sees the same crops
    and augmentations each step (one data feed, the crops stacked K times); slot k's generator is ``define_G`` under its own
    seed.  The random state right after variant 0's ``define_G`` drives the loop, so when the variants share the seed every
    slot is, bit for bit, the ``train_model`` run of its merged config, random crops included (``seed: -1`` draws one seed for
    every variant that has it).  Writes ``<dataroot>/out/sweep/<k>/output.png`` and ``variant.json`` (overrides, seed, final
    losses; with ``loss_trace`` the name of the variant's ``losses.csv`` beside it); ``callback(k, image)``.  Returns the engine."""
    from .engine import MultiPairEngine
    cfg = _load_cfg(dataroot, cfg_overrides)
    variants = [dict(v) for v in variants]
    cfgs = _sweep_checks(cfg, variants)
    if device.type != 'cuda':
        raise RuntimeError("train_sweep needs an MI355X: the product path has no CPU fallback")
    K = len(variants)
    drawn = None
    seeds = []
    for c in cfgs:
        seed = c['seed']
        if seed == -1:
            if drawn is None:
                drawn = np.random.randint(2 ** 32 - 1, dtype=np.int64)
            seed = drawn
        seeds.append(int(seed))
    _seed_host(seeds[0])
    torch.manual_seed(seeds[0])
    print(f'running a sweep of {K} variants with seeds: {seeds}.')

    A, B = _load_pair(cfg['dataroot'], cfg)
    feed = DeviceDataFeed(cfg, A, B)
    vit_engine = None if vit_state is not None else _shared_vit_engine(cfg['dino_model_name'], "train_sweep")
    gen_states, rng = [], None
    for k, c in enumerate(cfgs):
        if k > 0:
            torch.manual_seed(seeds[k])
        gen_states.append(_init_generator(c))
        if k == 0:   # the state train_model's loop starts from (variant 0's)
            rng = (random.getstate(), np.random.get_state(), torch.get_rng_state(), torch.cuda.get_rng_state_all())
    random.setstate(rng[0])
    np.random.set_state(rng[1])
    torch.set_rng_state(rng[2])
    torch.cuda.set_rng_state_all(rng[3])
    _one_scale(cfg)
    engine = MultiPairEngine(cfg, vit_state, gen_states, (_crop_max(A, B),) * 2, tuple(A.shape[1:]), device=device, vit_engine=vit_engine,
                             fp8=fp8_mode(cfg), pair_cfgs=variants)
    out_dirs = [os.path.join(cfg['dataroot'], 'out', 'sweep', str(k)) for k in range(K)]

    def next_inputs():   # every slot sees the one feed's crops
        inputs = feed.next()
        return tuple(t.expand(K, -1, -1, -1).contiguous() if t is not None else None for t in (inputs['A_global'], inputs['B_global'], inputs.get('A')))
    _optimise(cfg, engine, next_inputs, [feed.get_A()] * K, [AsyncResultWriter(cfg['dataroot'], out_dir=d) for d in out_dirs], callback, progress, feed=feed)
    losses = engine.losses() if engine.step_idx >= 0 else [{} for _ in range(K)]
    for k in range(K):
        with open(os.path.join(out_dirs[k], 'variant.json'), 'w') as f:
            json.dump({"index": k, "overrides": variants[k], "seed": seeds[k], "losses": losses[k], "stopped_at": engine.stopped_at[k], **trace_fields(engine), **lr_fields(engine, k), **optim_fields(engine), **image_terms_fields(engine), **layer_list_fields(engine), **key_gram_fields(engine), **key_nn_fields(engine)}, f)
    return engine


if __name__ == '__main__':
    parser = ArgumentParser()
    parser.add_argument("--dataroot", type=str)
    args = parser.parse_args()
    train_model(args.dataroot)
