"""Drop-in for ``util/losses.py``: ``LossG(cfg)`` with ``.extractor``, ``.global_transform``,
``.lambdas``, ``update_lambda_config``, ``forward(outputs, inputs) -> dict`` and the three
``calculate_*`` methods, composed from the HIP ops (ViT features, key self-similarity, bilinear
Resize with its adjoint).  This is the API-parity path (one ViT forward per reference call site,
autograd between ops); ``train_model`` uses the fused ``SpliceEngine`` step instead.
"""
import torch
import torch.nn.functional as F

from . import _lib
from .engine import (CLS_LAYER_KEYS, ID_LAYER_KEYS, KEY_GRAM_KEYS, KEY_GRAM_LAYER_KEYS, KEY_GRAM_LOSS_KEY, KEY_NN_KEYS, KEY_NN_LOSS_KEY, SSIM_LAYER_KEYS,
                     cls_layers_rule, id_layers_rule, key_gram_canonical, key_gram_layers_rule, key_gram_rule, key_nn_rule, resize_output_size, ssim_layers_rule)
from .extractor import VitExtractor
from .synth import DINO_CONFIGS

device = torch.device('cuda' if torch.cuda.is_available() else 'cpu')

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)


class _Resize(torch.autograd.Function):
    @staticmethod
    def forward(ctx, img, oh, ow):
        c, h, w = img.shape
        out = torch.empty(c, oh, ow, device=img.device)
        _lib.check(_lib.lib().splice_resize_bilinear_fwd(_lib.ptr(img), _lib.ptr(out), c, h, w, oh, ow, _lib.current_stream()), "resize_fwd")
        ctx.dims = (c, h, w, oh, ow)
        return out

    @staticmethod
    def backward(ctx, dout):
        c, h, w, oh, ow = ctx.dims
        din = torch.empty(c, h, w, device=dout.device)
        dout = dout.contiguous().float()
        _lib.check(_lib.lib().splice_resize_bilinear_bwd(_lib.ptr(dout), _lib.ptr(din), c, h, w, oh, ow, _lib.current_stream()), "resize_bwd")
        return din, None, None


class GlobalTransform:
    """``transforms.Compose([Resize(size, max_size=480), Normalize(imagenet)])`` of util/losses.py:19-24
    for ``[3,H,W]`` CUDA tensors (torchvision 0.10 tensor semantics: bilinear, no antialias)."""

    def __init__(self, size, max_size=480):
        self.size, self.max_size = size, max_size

    def __call__(self, img):
        c, h, w = img.shape
        oh, ow = resize_output_size(h, w, self.size, self.max_size)
        if (oh, ow) != (h, w):
            img = _Resize.apply(img.contiguous().float(), oh, ow)
        mean = torch.tensor(IMAGENET_MEAN, device=img.device).view(3, 1, 1)
        std = torch.tensor(IMAGENET_STD, device=img.device).view(3, 1, 1)
        return (img - mean) / std


def total_variation(img):
    """``mean|img[..., 1:, :] - img[..., :-1, :]| + mean|img[..., :, 1:] - img[..., :, :-1]|`` of one image ``[3, h, w]``, each mean over
    its own count; a direction without differences contributes 0."""
    dv, dh = img[..., 1:, :] - img[..., :-1, :], img[..., :, 1:] - img[..., :, :-1]
    return (dv.abs().mean() if dv.numel() else 0.0) + (dh.abs().mean() if dh.numel() else 0.0)


# One row per entry of the dict LossG.forward returns (util/losses.py:46-72), in the reference's evaluation order:
# (dict key, lambda name, feature compared, key of the generated batch in `outputs`, key of the target batch in `inputs`)
_TERMS = (
    ("loss_global_ssim", "lambda_global_ssim", "self_sim", "x_global", "A_global"),
    ("loss_entire_ssim", "lambda_entire_ssim", "self_sim", "x_entire", "A"),
    ("loss_entire_cls", "lambda_entire_cls", "cls", "x_entire", "B_global"),
    ("loss_global_cls", "lambda_global_cls", "cls", "x_global", "B_global"),
    ("loss_global_id_B", "lambda_global_identity", "keys", "y_global", "B_global"),
)
# The image-space terms (an extension beyond the reference), on the generated crops themselves, every step, no
# schedule: (dict key, lambda name, key of the generated batch in `outputs`, key of the compared batch in `inputs` or None)
_IMAGE_TERMS = (
    ("loss_global_tv", "lambda_global_tv", "x_global", None),
    ("loss_global_pix_id_B", "lambda_global_pixel_identity", "y_global", "B_global"),
)
_SCHEDULED_AT_WARMUP = ("lambda_global_ssim", "lambda_global_identity")
_SCHEDULED_PERIODIC = ("lambda_entire_ssim", "lambda_entire_cls")
_LAST_LAYER = 11


class LossG(torch.nn.Module):
    """``util/losses.py:11-105``.  The five terms are rows of ``_TERMS``; each compares ONE DINO feature of a generated
    image with the same feature of a target image (no gradient into the target) crop by crop, and the three public
    ``calculate_*`` methods are that comparison with the feature fixed."""

    def __init__(self, cfg, extractor=None, **extractor_kwargs):
        super().__init__()
        self.cfg = cfg
        self.extractor = extractor or VitExtractor(model_name=cfg['dino_model_name'], device=device, **extractor_kwargs)
        self.global_transform = GlobalTransform(cfg['dino_global_patch_size'], max_size=480)
        # only the [CLS] appearance term is live before the warm-up step (util/losses.py:25-32)
        self.lambdas = {name: 0 for _, name, _, _, _ in _TERMS}
        self.lambdas['lambda_global_cls'] = cfg['lambda_global_cls']
        # the blocks of the two structure terms (an extension beyond the reference): None -- the top block -- or the
        # canonical (layers, weights), what the fused step minimises under the same two keys
        self.ssim_layers = ssim_layers_rule({k: cfg.get(k) for k in SSIM_LAYER_KEYS}, DINO_CONFIGS[cfg['dino_model_name']][2])
        # ... and the blocks of the two appearance terms, likewise
        self.cls_layers = cls_layers_rule({k: cfg.get(k) for k in CLS_LAYER_KEYS}, DINO_CONFIGS[cfg['dino_model_name']][2])
        # ... and the blocks of the key-identity term
        self.id_layers = id_layers_rule({k: cfg.get(k) for k in ID_LAYER_KEYS}, DINO_CONFIGS[cfg['dino_model_name']][2])
        # ... and the key second-moment appearance term: None -- off -- or (lambda, block)
        # ... over a list of blocks, or centred: None, or (lambda, layers, weights, centered)
        kg_cfg = {k: cfg[k] for k in KEY_GRAM_KEYS + KEY_GRAM_LAYER_KEYS if k in cfg}
        kg_cfg.update(key_gram_canonical(kg_cfg, DINO_CONFIGS[cfg['dino_model_name']][2]))
        self.key_gram_layers = key_gram_layers_rule(kg_cfg, DINO_CONFIGS[cfg['dino_model_name']][2])
        self.key_gram = key_gram_rule(kg_cfg, DINO_CONFIGS[cfg['dino_model_name']][2])
        # ... and the nearest-neighbour key appearance term: None -- off -- or (lambda, block)
        self.key_nn = key_nn_rule({k: cfg[k] for k in KEY_NN_KEYS if k in cfg}, DINO_CONFIGS[cfg['dino_model_name']][2])
        self._features = {
            "self_sim": lambda img: self.extractor.get_keys_self_sim_from_input(img, layer_num=_LAST_LAYER),
            "cls": lambda img: self.extractor.get_feature_from_input(img)[-1][0, 0, :],
            "keys": lambda img: self.extractor.get_keys_from_input(img, _LAST_LAYER),
        }

    def update_lambda_config(self, step):
        """Lambda schedule of util/losses.py:34-44: structure + identity terms are switched on for good at
        ``cls_warmup``; the entire-image terms are live only on multiples of ``entire_A_every``."""
        cfg = self.cfg
        if step == cfg['cls_warmup']:
            self.lambdas.update((name, cfg[name]) for name in _SCHEDULED_AT_WARMUP)
        entire_step = step % cfg['entire_A_every'] == 0
        self.lambdas.update((name, cfg[name] if entire_step else 0) for name in _SCHEDULED_PERIODIC)

    def forward(self, outputs, inputs):
        self.update_lambda_config(int(inputs['step']))
        losses, total = {}, 0
        for key, lam_name, feature, out_key, in_key in _TERMS:
            lam = self.lambdas[lam_name]
            if lam > 0:
                losses[key] = self._feature_mse(feature, outputs[out_key], inputs[in_key])
                total = total + lam * losses[key]
        # the two image-space terms, summed over the crops as the others: what the fused step adds under the same two keys
        for key, lam_name, out_key, in_key in _IMAGE_TERMS:
            lam = self.cfg.get(lam_name, 0)
            if lam > 0:
                if in_key is None:
                    losses[key] = sum(total_variation(img) for img in outputs[out_key])
                else:
                    losses[key] = sum(F.mse_loss(img, ref.to(img.device)) for img, ref in zip(outputs[out_key], inputs[in_key]))
                total = total + lam * losses[key]
        # the key second-moment term, on the steps of the structure and identity terms (from cls_warmup on, entire-image steps included)
        if self.key_gram is not None and int(inputs['step']) >= self.cfg['cls_warmup']:
            losses[KEY_GRAM_LOSS_KEY] = self.calculate_key_gram_loss(outputs['x_global'], inputs['B_global'])
            total = total + self.key_gram[0] * losses[KEY_GRAM_LOSS_KEY]
        # the nearest-neighbour key term, on the same steps, behind it
        if self.key_nn is not None and int(inputs['step']) >= self.cfg['cls_warmup']:
            losses[KEY_NN_LOSS_KEY] = self.calculate_key_nn_loss(outputs['x_global'], inputs['B_global'])
            total = total + self.key_nn[0] * losses[KEY_NN_LOSS_KEY]
        losses['loss'] = total
        return losses

    def calculate_key_nn_loss(self, generated, targets, eps=1e-8):
        """The raw nearest-neighbour key term: sum over the zipped crops of mean over the tokens i of 1 - max_j cos(k_i, b_j), k / b the T x D
        keys of block ``dino_nn_layer`` (every token, the heads concatenated) of the generated and of the target crop, the cosine as the key
        self-similarity forms it (the product of the norms clamped at ``eps``); target side under no_grad.  ``max`` hands the gradient to
        the first index among equals, the engine's choice."""
        layer = self.key_nn[1] if self.key_nn is not None else DINO_CONFIGS[self.cfg['dino_model_name']][2] - 1

        def keys(img):
            per_head = self.extractor.get_keys_from_input(img, layer_num=layer)   # [heads, T, d]
            return per_head.permute(1, 0, 2).reshape(per_head.shape[1], -1)       # [T, heads * d]
        acc = 0.0
        for gen_img, tgt_img in zip(generated, targets):
            with torch.no_grad():
                b = keys(self.global_transform(tgt_img).unsqueeze(0).to(device))
            k = keys(self.global_transform(gen_img).unsqueeze(0).to(device))
            cos = (k @ b.transpose(0, 1)) / torch.clamp(k.norm(dim=1)[:, None] * b.norm(dim=1)[None, :], min=eps)
            acc = acc + (1.0 - cos.max(dim=1).values).mean()
        return acc

    def calculate_key_gram_loss(self, generated, targets):
        """The raw key second-moment term: sum over the zipped crops of mean((G(K_gen) - G(K_tgt))^2) over the D * D entries, G(K) = K^T K / T of
        the T x D keys of block ``dino_gram_layer`` (every token, the heads concatenated); target side under no_grad."""
        layer = self.key_gram[1] if self.key_gram is not None else DINO_CONFIGS[self.cfg['dino_model_name']][2] - 1
        # over ``dino_gram_layers``: the sum over the blocks, ascending, of weight * that; ``dino_gram_centered``: G(K) less
        # the outer product of the mean key
        layers, weights, centered = ([layer], [1.0], False) if getattr(self, "key_gram_layers", None) is None else self.key_gram_layers[1:]

        def gram(img, l):
            per_head = self.extractor.get_keys_from_input(img, layer_num=l)       # [heads, T, d]
            k = per_head.permute(1, 0, 2).reshape(per_head.shape[1], -1)          # [T, heads * d]
            g = k.transpose(0, 1) @ k / k.shape[0]
            if centered:
                mu = k.mean(0)
                g = g - torch.outer(mu, mu)
            return g
        acc = 0.0
        for l, w in zip(layers, weights):
            term = 0.0
            for gen_img, tgt_img in zip(generated, targets):
                with torch.no_grad():
                    want = gram(self.global_transform(tgt_img).unsqueeze(0).to(device), l)
                term = term + F.mse_loss(gram(self.global_transform(gen_img).unsqueeze(0).to(device), l), want)
            acc = acc + (term if w == 1.0 else w * term)
        return acc

    def _feature_mse(self, feature, generated, targets):
        """sum over crops of mse(feature(T(generated_i)), feature(T(target_i))), target side under no_grad."""
        if feature == "self_sim" and self.ssim_layers is not None:
            return self._layered_self_sim_mse(generated, targets)
        if feature == "cls" and self.cls_layers is not None:
            return self._layered_cls_mse(generated, targets)
        if feature == "keys" and self.id_layers is not None:
            return self._layered_keys_mse(generated, targets)
        f = self._features[feature]
        acc = 0.0
        for gen_img, tgt_img in zip(generated, targets):   # one crop at a time: the extractor is batch-1
            with torch.no_grad():
                want = f(self.global_transform(tgt_img).unsqueeze(0).to(device))
            got = f(self.global_transform(gen_img).unsqueeze(0).to(device))
            acc = acc + F.mse_loss(got, want)
        return acc

    def _layered_self_sim_mse(self, generated, targets):
        """The structure term over ``dino_ssim_layers``: per crop, sum over the blocks ascending of w_l mse(S_l(generated), S_l(target))."""
        acc = 0.0
        for gen_img, tgt_img in zip(generated, targets):
            tgt, gen = self.global_transform(tgt_img).unsqueeze(0).to(device), self.global_transform(gen_img).unsqueeze(0).to(device)
            crop = 0.0
            for layer, w in zip(*self.ssim_layers):
                with torch.no_grad():
                    want = self.extractor.get_keys_self_sim_from_input(tgt, layer_num=layer)
                crop = crop + w * F.mse_loss(self.extractor.get_keys_self_sim_from_input(gen, layer_num=layer), want)
            acc = acc + crop
        return acc

    def _layered_cls_mse(self, generated, targets):
        """The appearance term over ``dino_cls_layers``: per crop, sum over the blocks ascending of w_l mse(cls_l(generated), cls_l(target)),
        cls_l = the [CLS] row of block l's output."""
        acc = 0.0
        for gen_img, tgt_img in zip(generated, targets):
            tgt, gen = self.global_transform(tgt_img).unsqueeze(0).to(device), self.global_transform(gen_img).unsqueeze(0).to(device)
            with torch.no_grad():
                want = self.extractor.get_feature_from_input(tgt)
            got = self.extractor.get_feature_from_input(gen)
            crop = 0.0
            for layer, w in zip(*self.cls_layers):
                crop = crop + w * F.mse_loss(got[layer][0, 0, :], want[layer][0, 0, :])
            acc = acc + crop
        return acc

    def _layered_keys_mse(self, generated, targets):
        """The identity term over ``dino_id_layers``: per crop, sum over the blocks ascending of w_l mse(k_l(generated), k_l(target)),
        k_l = the keys of block l."""
        acc = 0.0
        for gen_img, tgt_img in zip(generated, targets):
            tgt, gen = self.global_transform(tgt_img).unsqueeze(0).to(device), self.global_transform(gen_img).unsqueeze(0).to(device)
            crop = 0.0
            for layer, w in zip(*self.id_layers):
                with torch.no_grad():
                    want = self.extractor.get_keys_from_input(tgt, layer_num=layer)
                crop = crop + w * F.mse_loss(self.extractor.get_keys_from_input(gen, layer_num=layer), want)
            acc = acc + crop
        return acc

    # the reference's public per-term entry points (argument order as in util/losses.py:74,85,96)
    def calculate_global_ssim_loss(self, outputs, inputs):
        return self._feature_mse("self_sim", outputs, inputs)

    def calculate_crop_cls_loss(self, outputs, inputs):
        return self._feature_mse("cls", outputs, inputs)

    def calculate_global_id_loss(self, outputs, inputs):
        return self._feature_mse("keys", outputs, inputs)
