"""GPU: the image-space loss terms of the fused step -- total variation of x' = G(A_crop) and pixel identity
mse(G(B_crop), B_crop).  Op level: the value launch, the gradient-add launch and the IMG instance of the total-loss kernel on caller
buffers against float64.  Step level: reported values, the gradient by difference against a twin engine with both keys 0, graph replay,
batch independence, "off is off", and one small case each with the stop rule, snapshots and MultiScaleEngine."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest
import torch

from oracle import loss_stage as ls
from splice_amd import _lib, synth
from splice_amd.engine import (DEFAULT_CFG, IMAGE_LOSS_KEYS, MultiPairEngine, MultiScaleEngine, SpliceEngine, np_image_terms, np_plateau,
                               stop_window_closes)
from splice_amd.generator import GeneratorPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
CHUNK = 4096   # SPLICE_IMAGE_TERMS_CHUNK
K_TV, K_PIX = 6, 7
SHAPES = [(2, 2), (3, 5), (24, 40), (67, 131)]   # the minimum; odd widths; (67, 131): 7 chunks per image


def _st():
    return _lib.current_stream()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _grid(seed, *shape):
    """round(16 u) / 16: every |difference| is a multiple of 2^-4 <= 1 and every squared difference one of 2^-8, so the kernel's unscaled
    sums are exact in fp32 in any order (at (67, 131): 8610.6, 8729.4, 4375.5, far below 2^24 * 2^-8); ~6 % of neighbours tie."""
    g = torch.Generator().manual_seed(seed)
    return (torch.round(16 * torch.rand(*shape, generator=g)) / 16).float()


def _chunks(h, w):
    return (3 * h * w + CHUNK - 1) // CHUNK


def _value(x, y, b, lp, fill=0.0):
    """the value launch on a partials buffer of x.shape[0] / y.shape[0] slots in the step's layout; returns (buffer after, lstride)"""
    n = max(x.shape[0] if x is not None else 0, y.shape[0] if y is not None else 0)
    lstride = 8 + 8 * lp + 4
    buf = torch.full((n * lstride,), fill, device=DEV)
    xs, ys = (x.shape if x is not None else (0, 3, 0, 0)), (y.shape if y is not None else (0, 3, 0, 0))
    xd, yd, bd = (None if t is None else t.to(DEV).contiguous() for t in (x, y, b))
    rc = _lib.lib().splice_image_terms_value(_lib.ptr(xd), xs[0], xs[2], xs[3], _lib.ptr(yd), _lib.ptr(bd), ys[0], ys[2], ys[3], _lib.ptr(buf), lstride, lp, _st())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().splice_last_error()
    return buf, lstride


def _total_img(buf, lstride, lp, pairs, n, w5, w_tv, w_pix, wtab=None, ssim_on=1, entire=1):
    bd = buf.to(DEV).clone()
    out8 = torch.full((pairs + 1, 8), float("nan"), device=DEV)
    wt = None if wtab is None else wtab.to(DEV)
    rc = _lib.lib().splice_total_loss_pairs_img(_lib.ptr(bd), lstride, lp, *w5, _lib.ptr(out8), pairs, n["a"], n["b"], n["c"], n["e"], _lib.ptr(wt), ssim_on,
                                                entire, w_tv, w_pix, _st())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().splice_last_error()
    assert torch.isnan(out8[pairs]).all()
    return out8[:pairs].cpu(), bd.cpu()


def _refs(x, y, b):
    """fp64 raw terms of every image: ([tv_i], [pix_i])"""
    tv = [np_image_terms(x[i].numpy())[0] for i in range(x.shape[0])]
    pix = [np_image_terms(None, y[i].numpy(), b[i].numpy())[2] for i in range(y.shape[0])]
    return tv, pix


# ------------------------------------------------------------------------------------------------ value
@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_values_against_fp64(hw, n_img):
    """Raw terms as the step forms them (value launch, then the IMG total launch, one slot per pair) against float64, relative 2^-18 = 64
    roundings of 2^-24.  On the 1/16 grid the chunk sums are exact; the roundings on the longest path here ((67, 131): 7 chunks, lp = 1024)
    are 3 per chunk (two divisions by the counts and their sum; pixel identity: 1), 0 in the lane loop (7 chunks: one nonzero partial per
    lane), at most 6 in the wave tree and 0 for the one slot: 9."""
    h, w = hw
    lp = 1024
    x, y, b = _grid(h * w + n_img, n_img, 3, h, w), _grid(h * w + 7, n_img, 3, h, w), _grid(h * w + 9, n_img, 3, h, w)
    assert ((x[..., 1:, :] == x[..., :-1, :]).any() or h * w < 16) and _chunks(*SHAPES[-1]) == 7
    buf, lstride = _value(x, y, b, lp)
    out8, _ = _total_img(buf, lstride, lp, n_img, dict(a=1, b=1, c=1, e=1), [0.0] * 5, 1.0, 1.0)
    tv, pix = _refs(x, y, b)
    for i in range(n_img):
        e_tv, e_pix = abs(out8[i, 6].item() - tv[i]) / tv[i], abs(out8[i, 7].item() - pix[i]) / pix[i]
        print(f"IMAGE_TERMS value {h}x{w} n={n_img} image {i}: rel err tv {e_tv:.3e} pix {e_pix:.3e} (bar {2.0 ** -18:.3e})")
        assert e_tv <= 2.0 ** -18 and e_pix <= 2.0 ** -18
    # written: the first ceil(3 h w / 4096) slots of terms 6 and 7 of every image, with these bits; nothing else
    fill, _ = _value(x, y, b, lp, fill=-7.5)
    fill, buf = fill.cpu(), buf.cpu()
    written = torch.zeros(fill.numel(), dtype=torch.bool)
    for i in range(n_img):
        for k in (K_TV, K_PIX):
            o = i * lstride + 8 + k * lp
            written[o:o + _chunks(h, w)] = True
    assert torch.equal(_bits(fill[written]), _bits(buf[written])) and (fill[~written] == -7.5).all() and (buf[~written] == 0).all()


def test_values_grouped_two_slots_of_two_crops_and_unequal_sides():
    """2 pairs x 2 crops, the A crops (3, 5) and the B crops (24, 40): pair p's raw terms are its two crops' sums, added in crop order."""
    lp = 70
    x, y, b = _grid(1, 4, 3, 3, 5), _grid(2, 4, 3, 24, 40), _grid(3, 4, 3, 24, 40)
    buf, lstride = _value(x, y, b, lp)
    out8, _ = _total_img(buf, lstride, lp, 2, dict(a=2, b=2, c=2, e=1), [0.0] * 5, 0.5, 2.0)
    tv, pix = _refs(x, y, b)
    for p in range(2):
        r_tv, r_pix = tv[2 * p] + tv[2 * p + 1], pix[2 * p] + pix[2 * p + 1]
        assert abs(out8[p, 6].item() - r_tv) <= 2.0 ** -18 * r_tv and abs(out8[p, 7].item() - r_pix) <= 2.0 ** -18 * r_pix
        assert abs(out8[p, 0].item() - (0.5 * r_tv + 2.0 * r_pix)) <= 2.0 ** -18 * (0.5 * r_tv + 2.0 * r_pix)
    # one term alone: the other's slots are not written (and not read: its operands are NULL)
    only_tv, _ = _value(x, None, None, lp, fill=-7.5)
    only_pix, _ = _value(None, y, b, lp, fill=-7.5)
    for i in range(4):
        o6, o7 = i * lstride + 8 + K_TV * lp, i * lstride + 8 + K_PIX * lp
        assert torch.equal(_bits(only_tv[o6:o6 + lp]), _bits(buf[o6:o6 + lp].clone().masked_fill_(torch.arange(lp, device=DEV) >= 1, -7.5)))
        assert (only_tv[o7:o7 + lp] == -7.5).all() and (only_pix[o6:o6 + lp] == -7.5).all()
        assert torch.equal(_bits(only_pix[o7:o7 + lp]), _bits(buf[o7:o7 + lp].clone().masked_fill_(torch.arange(lp, device=DEV) >= 1, -7.5))) and _chunks(24, 40) == 1


# ------------------------------------------------------------------------------------------------ gradient add
GUARD = 1024


def _grad_add(x, b, d0, lam, x_off=1, d_off=3):
    """d0 + lambda * gradient through the launch, the operands at odd dword offsets of their allocations (no 16-byte alignment) and a
    guard band of sentinels on both sides of d.  Returns (d after, rc, whether the whole allocation kept its bits)."""
    n = d0.numel()
    dbuf = torch.full((d_off + n + GUARD,), 123.25, device=DEV)
    dbuf[d_off:d_off + n] = d0.reshape(-1).to(DEV)
    xbuf = torch.zeros(x_off + n, device=DEV)
    xbuf[x_off:] = x.reshape(-1).to(DEV)
    bbuf = None
    if b is not None:
        bbuf = torch.zeros(x_off + n, device=DEV)
        bbuf[x_off:] = b.reshape(-1).to(DEV)
    before = dbuf.clone()
    rc = _lib.lib().splice_image_terms_grad_add(_lib.ptr(xbuf[x_off:]), _lib.ptr(bbuf[x_off:]) if b is not None else None, _lib.ptr(dbuf[d_off:]),
                                                x.shape[0], x.shape[2], x.shape[3], lam, _st())
    torch.cuda.synchronize()
    assert torch.equal(_bits(dbuf[:d_off]), _bits(before[:d_off])) and torch.equal(_bits(dbuf[d_off + n:]), _bits(before[d_off + n:]))   # the guard bands, bit for bit
    return dbuf[d_off:d_off + n].reshape(d0.shape).cpu(), rc, torch.equal(_bits(dbuf), _bits(before))


def _border_masks(h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[0, :] = m[-1, :] = m[:, 0] = m[:, -1] = True
    c = torch.zeros(h, w, dtype=torch.bool)
    c[0, 0] = c[0, -1] = c[-1, 0] = c[-1, -1] = True
    return m, c


@pytest.mark.parametrize("n_img", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gradient_add_against_fp64(hw, n_img):
    """|got - (d0 + g_ref)| <= 2^-23 (|d0| + |g_ref|) element-wise: g_ref = (lambda / nv) sv + (lambda / nh) sh of integer signs (TV), or
    (2 lambda / 3hw) (y - b) of an exact difference (pixel identity), is rounded to fp32 once by the kernel, and the add once more.  Border
    and corner pixels asserted on their own."""
    h, w = hw
    x, y, b = _grid(h * w + n_img, n_img, 3, h, w), _grid(h * w + 7, n_img, 3, h, w), _grid(h * w + 9, n_img, 3, h, w)
    d0 = torch.randn(n_img, 3, h, w, generator=torch.Generator().manual_seed(h + w))
    lam = 0.37
    lam32 = float(f32(lam))
    border, corner = _border_masks(h, w)
    for tag, got, g_ref in (
            ("tv", _grad_add(x, None, d0, lam), np.stack([lam32 * np_image_terms(x[i].numpy())[1] for i in range(n_img)])),
            ("pix", _grad_add(y, b, d0, lam), np.stack([lam32 * np_image_terms(None, y[i].numpy(), b[i].numpy())[3] for i in range(n_img)]))):
        got, rc, untouched = got
        assert rc == 0 and not untouched
        g_ref = torch.from_numpy(g_ref)
        err = (got.double() - (d0.double() + g_ref)).abs()
        bound = 2.0 ** -23 * (d0.double().abs() + g_ref.abs())
        print(f"IMAGE_TERMS grad {tag} {h}x{w} n={n_img}: worst err/bound {(err / bound.clamp(min=1e-300)).max().item():.3f}, ties {(g_ref == 0).double().mean().item():.3f}")
        assert (err <= bound).all()
        assert (err[..., border] <= bound[..., border]).all() and (err[..., corner] <= bound[..., corner]).all()
        # the term did move the border: what arrived there is d0 + a nonzero gradient, to the same bound (a stencil that skipped or
        # doubled a border neighbour is off by lambda / n, thousands of bounds)
        moved = (got.double() - d0.double())[..., border]
        assert ((moved - g_ref[..., border]).abs() <= bound[..., border]).all() and (g_ref[..., border] != 0).any()


def test_sign_of_zero_is_zero_and_rows_and_planes_do_not_leak():
    """A constant image has zero TV gradient everywhere (sign(0) = 0), whatever stands in the neighbouring rows' ends or the next plane;
    a single step edge moves exactly the two pixels beside it."""
    h, w = 4, 5
    x = torch.zeros(2, 3, h, w)
    x[0, 1] = 1.0          # plane 1 of image 0 differs from planes 0 and 2 as a whole: no gradient unless planes leak
    x[1, 0, :, :] = torch.arange(h, dtype=torch.float32)[:, None]   # rows differ, columns do not: horizontal signs are all 0
    d0 = torch.zeros_like(x)
    got, rc, _ = _grad_add(x, None, d0, 1.0)
    assert rc == 0
    assert not got[0].any()                                  # three constant planes
    ref = torch.from_numpy(np_image_terms(x[1].numpy())[1]).float()
    assert torch.equal(got[1], ref) and not got[1, 1:].any()
    assert (got[1, 0, 0] < 0).all() and (got[1, 0, -1] > 0).all() and not got[1, 0, 1:-1].any()   # interior rows: +1 - 1 = 0


def test_pair_independence_image_1_of_3_is_its_own_launch():
    h, w = 67, 131
    lp = 70
    x, y, b = _grid(21, 3, 3, h, w), _grid(22, 3, 3, h, w), _grid(23, 3, 3, h, w)
    d0 = torch.randn(3, 3, h, w, generator=torch.Generator().manual_seed(5))
    buf3, lstride = _value(x, y, b, lp)
    buf1, _ = _value(x[1:2], y[1:2], b[1:2], lp)
    assert torch.equal(_bits(buf3[lstride:2 * lstride]), _bits(buf1[:lstride]))
    for xi, bi in ((x, None), (y, b)):
        g3 = _grad_add(xi, bi, d0, 0.37)[0]
        g1 = _grad_add(xi[1:2], None if bi is None else bi[1:2], d0[1:2], 0.37)[0]
        assert torch.equal(_bits(g3[1:2]), _bits(g1))


# ------------------------------------------------------------------------------------------------ total, IMG instance
def _total_ref_img(buf, lstride, lp, pairs, n, w5, w_tv, w_pix, **kw):
    """oracle.loss_stage.total_ref for the five terms, extended by terms 6 (n_a slots) and 7 (n_b slots) with ITS bar -- "|err raw_k| <=
    lp * 2^-24 * sum|partials| (the add chain is ceil(lp / 64) + 6 + slots <= lp long), and the total adds sum |w_k| bound_k + 6 * 2^-24 *
    sum |w_k raw_k| (one product and four adds per term)" (tests/test_loss_stage_gpu.py::test_total_loss_pairs_against_fp64) -- the two
    further terms entering through two more fused multiply-adds: 8 * 2^-24 for each of them, 2 * 2^-24 more for the five."""
    ref, bound = ls.total_ref(buf, lstride, lp, pairs, n, w5, **kw)
    b64 = buf.double()
    for p in range(pairs):
        five = sum(abs(w * ref[p, k].item()) for w, k in zip(ls.total_weights(p, w5, kw.get("wtab"), kw.get("ssim_on", 1), kw.get("entire", 1)), (1, 2, 3, 4, 5)))   # (TOTAL_TERMS: weight i belongs to term i + 1)
        bound[p, 0] += 2 * 2.0 ** -24 * five          # the five terms' sum passes through two more fused adds
        for k, wk, ns in ((K_TV, w_tv, n["a"]), (K_PIX, w_pix, n["b"])):
            parts = torch.cat([b64[(p * ns + s) * lstride + 8 + k * lp:(p * ns + s) * lstride + 8 + (k + 1) * lp] for s in range(ns)])
            ref[p, k] = parts.sum()
            bound[p, k] = lp * 2.0 ** -24 * parts.abs().sum()
            ref[p, 0] += wk * ref[p, k]
            bound[p, 0] += abs(wk) * bound[p, k] + 8 * 2.0 ** -24 * abs(wk * ref[p, k].item())
    return ref, bound


@pytest.mark.parametrize("slots", [(1, 1, 1, 1), (3, 2, 2, 1)], ids=["slots1", "slots3221"])
@pytest.mark.parametrize("lp", [70, 1024])
def test_total_loss_pairs_img_against_fp64(lp, slots):
    pairs = 2
    n = dict(zip("abce", slots))
    lstride = 8 + 8 * lp + 4
    g = torch.Generator().manual_seed(lp + slots[0])
    buf = torch.rand(pairs * max(slots) * lstride, generator=g)
    w5 = [float(f32(v)) for v in (10.0, 0.1, 3.0, 0.25, 1.0)]
    w_tv, w_pix = float(f32(0.3)), float(f32(1.7))
    wtab = torch.tensor([[1.0, 10.0, 2.0, 0.5, 0.25], [0.3, 1.0, 0.7, 1.0, 1.5]])
    for tag, kw in (("scalar", {}), ("table", dict(wtab=wtab, ssim_on=1, entire=0))):
        out8, after = _total_img(buf, lstride, lp, pairs, n, w5, w_tv, w_pix, **kw)
        ref, bound = _total_ref_img(buf, lstride, lp, pairs, n, w5, w_tv, w_pix, **kw)
        err = (out8.double() - ref).abs()
        print(f"IMAGE_TERMS total lp={lp} slots={slots} {tag}: worst err/bound {(err / bound.clamp(min=1e-300)).max().item():.3f}")
        assert (err <= bound).all(), (err, bound)
        for p in range(pairs):   # the slot's own values [0..7] hold the same numbers; the partials are not touched
            assert torch.equal(_bits(after[p * lstride:p * lstride + 8]), _bits(out8[p]))
        keep = torch.ones(buf.numel(), dtype=torch.bool)
        for p in range(pairs):
            keep[p * lstride:p * lstride + 8] = False
        assert torch.equal(_bits(after[keep]), _bits(buf[keep]))
        # both weights 0: words 0-5 are, bit for bit, what splice_total_loss_pairs writes from the same buffer -- and the whole row when the
        # two terms' partials are zero, as they are in a step without the terms
        plain = torch.full((pairs, 8), float("nan"), device=DEV)
        bd = buf.to(DEV).clone()
        wt = kw["wtab"].to(DEV) if "wtab" in kw else None
        assert _lib.lib().splice_total_loss_pairs(_lib.ptr(bd), lstride, lp, *w5, _lib.ptr(plain), pairs, n["a"], n["b"], n["c"], n["e"], _lib.ptr(wt),
                                                  kw.get("ssim_on", 1), kw.get("entire", 1), _st()) == 0
        torch.cuda.synchronize()
        zero_w, _ = _total_img(buf, lstride, lp, pairs, n, w5, 0.0, 0.0, **kw)
        assert torch.equal(_bits(zero_w[:, :6]), _bits(plain.cpu()[:, :6]))
        cleared = buf.clone()
        for s in range(pairs * max(slots)):
            cleared[s * lstride + 8 + K_TV * lp:s * lstride + 8 + 8 * lp] = 0
        zero_p, _ = _total_img(cleared, lstride, lp, pairs, n, w5, 0.0, 0.0, **kw)
        assert torch.equal(_bits(zero_p), _bits(plain.cpu()))


# ------------------------------------------------------------------------------------------------ the engine
@pytest.fixture(scope="module")
def vit():
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05))


def _cfg(**over):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed=40, pair=2):   # (the pair and generator of tests/test_step_gpu.py::test_step_gradients_vs_oracle_teacher_forced)
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


GEN_SEED = 41


def _engine(vit, n_crops=1, **over):
    return SpliceEngine(_cfg(**over), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64), vit_engine=vit, n_crops=n_crops)


def _crops(A, B, n_crops):
    """nA / nB crops of one pair: the image, then its mirror images"""
    flips = [lambda t: t, lambda t: t.flip(-1), lambda t: t.flip(-2)]
    return (torch.stack([flips[i](A) for i in range(n_crops[0])]).contiguous(), torch.stack([flips[i](B) for i in range(n_crops[1])]).contiguous())


def _plans(eng, n_crops):
    """the generator plans a one-pair engine runs its crops through (the pair's crops are one netG call: batch statistics)"""
    return [GeneratorPlan(eng.gen, n, 64, 64, True, 0, batch_stats=max(n_crops) > 1 and n > 1) for n in n_crops]


def _term_seeds(x, y, b, lam_tv, lam_pix):
    """lambda * d(term)/d(image) in float64 from the plans' own forward outputs, cast to fp32: (d for the A plan, d for the B plan)"""
    xn, yn, bn = x.cpu().numpy(), y.cpu().numpy(), b.cpu().numpy()
    da = np.stack([float(f32(lam_tv)) * np_image_terms(xn[i])[1] for i in range(xn.shape[0])])
    db = np.stack([float(f32(lam_pix)) * np_image_terms(None, yn[i], bn[i])[3] for i in range(yn.shape[0])])
    return torch.from_numpy(da.astype(f32)).to(DEV), torch.from_numpy(db.astype(f32)).to(DEV)


def _rel_l2(eng, got, ref):
    """whole-arena relative L2, the conv biases in front of a BatchNorm left out (analytically zero gradient, fp32 noise on both sides;
    tests/test_generator_gpu.py)"""
    num = den = 0.0
    for (name, g), r in zip(eng.gen.unflatten(got).items(), eng.gen.unflatten(ref).values()):
        if name.endswith("0.bias") and name != "9.0.bias":
            continue
        num += (g.double() - r.double()).pow(2).sum().item()
        den += r.double().pow(2).sum().item()
    return (num / den) ** 0.5, den ** 0.5


def _fmaf32(a, b, c):
    """fl32(a * b + c) with one rounding, from exact rationals (ties to even)"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    g = f32(float(exact))
    cands = [np.nextafter(g, f32(-np.inf)), g, np.nextafter(g, f32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.int32)) & 1))


# (step 0 of this synthetic pair has ||g_off|| = 2.1e4: weights of this size put ||g_ref|| / ||g_off|| at 0.2 - 0.5)
LAMBDAS = dict(tv=(2048.0, 0.0), pix=(0.0, 2048.0), both=(2048.0, 2048.0))
# Bars of the gradient test: 8 x the linearity defect of the generator backward WITHOUT this feature, measured with the plan API alone on an
# MI355X as the issue prescribes -- ||bwd(d1 + d2) - bwd(d1) - bwd(d2)|| / ||bwd(d2)||, d2 the term's seed, d1 seeded normals scaled so that
# ||bwd(d1)|| = ||g_off|| -- with the ratio ||g_ref|| / ||g_off|| the lambdas above give (DESIGN.md section 9j has the table).
#                         (floor, ratio)
FLOORS = {("tv", (1, 1)): (3.267e-06, 0.232), ("pix", (1, 1)): (2.889e-06, 0.234), ("both", (1, 1)): (3.118e-06, 0.335),
          ("tv", (2, 1)): (1.848e-06, 0.384), ("pix", (2, 1)): (1.591e-06, 0.349), ("both", (2, 1)): (1.711e-06, 0.519)}


@pytest.fixture(scope="module")
def twins(vit):
    """per (terms, n_crops): the engine with the keys on and its twin with both 0 after steps 0 and 1 on the same crops, lr 0"""
    cache = {}

    def get(terms, n_crops):
        if (terms, n_crops) not in cache:
            A, B = _pair()
            Ac, Bc = _crops(A, B, n_crops)
            lam_tv, lam_pix = LAMBDAS[terms]
            on = _engine(vit, n_crops if max(n_crops) > 1 else 1, lr=0.0, lambda_global_tv=lam_tv, lambda_global_pixel_identity=lam_pix)
            off = _engine(vit, n_crops if max(n_crops) > 1 else 1, lr=0.0)
            p0 = on.params.clone()
            rec = []
            for _ in range(2):
                on.step(Ac, Bc, A)
                off.step(Ac, Bc, A)
                rec.append(dict(on=on.losses_dev.cpu().numpy().copy(), off=off.losses_dev.cpu().numpy().copy(), g_on=on.grads.clone(), g_off=off.grads.clone(),
                                d_on=on.losses(), d_off=off.losses()))
            assert torch.equal(on.params, p0) and torch.equal(off.params, p0)   # lr 0: the parameters stayed put
            cache[(terms, n_crops)] = (on, off, rec, (Ac, Bc))
        return cache[(terms, n_crops)]
    return get


@pytest.mark.parametrize("n_crops", [(1, 1), (2, 1)], ids=["1x1", "2x1"])
@pytest.mark.parametrize("terms", ["tv", "pix", "both"])
def test_step_reports_the_terms_and_extends_the_total(twins, terms, n_crops):
    """Steps 0 (before cls_warmup, entire-image) and 1: words 6 and 7 against float64 TV / mse of the plan's forward output on the same
    parameters, bar 2^-18 relative + the 2e-5 absolute output agreement tests/test_generator_gpu.py holds the plan to; loss =
    fmaf(l_pix, raw7, fmaf(l_tv, raw6, loss_off)) in float32 exactly."""
    on, off, rec, (Ac, Bc) = twins(terms, n_crops)
    lam_tv, lam_pix = LAMBDAS[terms]
    pa, pb = _plans(on, n_crops)
    x, y = pa.forward(on.params, Ac), pb.forward(on.params, Bc)
    tv = sum(np_image_terms(x[i].cpu().numpy())[0] for i in range(n_crops[0]))
    pix = sum(np_image_terms(None, y[i].cpu().numpy(), Bc[i].cpu().numpy())[2] for i in range(n_crops[1]))
    for step, r in enumerate(rec):
        row, row_off = r["on"][0], r["off"][0]
        print(f"IMAGE_TERMS step {step} {terms} {n_crops}: raw6 {row[6]:.7g} (fp64 {tv:.7g}) raw7 {row[7]:.7g} (fp64 {pix:.7g})")
        assert row[1:6].tobytes() == row_off[1:6].tobytes() and not row_off[6:].any()
        want6, want7 = (tv if lam_tv > 0 else 0.0), (pix if lam_pix > 0 else 0.0)
        assert abs(float(row[6]) - want6) <= 2.0 ** -18 * want6 + (2e-5 if lam_tv > 0 else 0)
        assert abs(float(row[7]) - want7) <= 2.0 ** -18 * want7 + (2e-5 if lam_pix > 0 else 0)
        assert row[0].tobytes() == _fmaf32(f32(lam_pix), row[7], _fmaf32(f32(lam_tv), row[6], row_off[0])).tobytes()
        assert row[0] > row_off[0]
        names = {k for k, lam in zip(IMAGE_LOSS_KEYS, (lam_tv, lam_pix)) if lam > 0}
        assert set(r["d_on"]) - set(r["d_off"]) == names and not set(IMAGE_LOSS_KEYS) & set(r["d_off"])
        assert r["d_on"]["loss"] == float(row[0]) and all(r["d_on"][k] == float(row[6 + IMAGE_LOSS_KEYS.index(k)]) for k in names)


@pytest.mark.parametrize("n_crops", [(1, 1), (2, 1)], ids=["1x1", "2x1"])
@pytest.mark.parametrize("terms", ["tv", "pix", "both"])
def test_step_gradient_by_difference(twins, terms, n_crops):
    """Step 0 is an entire-image step: the gradient arena holds the sum of all three chains.  g_on - g_off against the plans' backward of the
    terms' float64 seeds; whole-arena relative L2 within 8 x the measured linearity floor of the generator backward (FLOORS)."""
    on, off, rec, (Ac, Bc) = twins(terms, n_crops)
    lam_tv, lam_pix = LAMBDAS[terms]
    pa, pb = _plans(on, n_crops)
    x, y = pa.forward(on.params, Ac), pb.forward(on.params, Bc)
    da, db = _term_seeds(x, y, Bc, lam_tv, lam_pix)
    g_ref = pa.backward(on.params, da) + pb.backward(on.params, db)
    diff = rec[0]["g_on"] - rec[0]["g_off"]
    err, ref_norm = _rel_l2(on, diff, g_ref)
    _, off_norm = _rel_l2(on, rec[0]["g_off"], rec[0]["g_off"])
    floor, ratio = FLOORS[(terms, n_crops)]
    print(f"IMAGE_TERMS grad-by-difference {terms} {n_crops}: rel L2 {err:.3e}, bar {8 * floor:.3e}, ||g_ref|| / ||g_off|| {ref_norm / off_norm:.3f}")
    assert 0.1 <= ref_norm / off_norm <= 10 and 8 * floor <= 1e-3
    assert err <= 8 * floor


def test_graph_replay_equals_eager(vit):
    """Four steps on fixed crops with lr 0: steps 1-3 are one regime; step 1 is launched eagerly, step 2 captures the graph, step 3 replays
    it.  The gradient arena, Adam's first moment (beta1 = 0: the summed gradient of all chains, the y' chain's included) and words 6-7 after
    step 3 are those of steps 1 and 2, bit for bit."""
    A, B = _pair()
    eng = _engine(vit, lr=0.0, lambda_global_tv=4.0, lambda_global_pixel_identity=50.0)
    seen = []
    for _ in range(4):
        eng.step(A, B, A)
        seen.append((eng.grads.clone(), eng.m.clone(), eng.losses_dev.clone()))
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    assert stats[0] + stats[2] >= 1                                     # a graph was in use
    for k in (2, 3):
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(seen[k], seen[1])), k
    assert seen[3][2][0, 6] > 0 and seen[3][2][0, 7] > 0
    eager = _engine(vit, lr=0.0, lambda_global_tv=4.0, lambda_global_pixel_identity=50.0)
    _lib.check(_lib.lib().splice_step_use_graph(eager.handle, 0), "use_graph")
    for _ in range(4):
        eager.step(A, B, A)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((eager.grads, eager.m, eager.losses_dev), seen[3]))


def _arenas(eng, pair=0):
    n, st = eng.gen.numel, eng.stride
    sl = slice(pair * st, pair * st + n)
    return dict(params=eng.params[sl].clone(), m=eng.m[sl].clone(), v=eng.v[sl].clone(), running=eng.running[pair].clone(), losses=eng.losses_dev[pair].clone())


def test_batch_independence_two_pairs(vit):
    """default lr, 3 steps, both keys on: each pair of a two-pair engine is, bit for bit, its own SpliceEngine run"""
    keys = dict(lambda_global_tv=0.5, lambda_global_pixel_identity=2.0)
    pairs = [_pair(40, 2), _pair(62, 0)]
    gens = [synth.generator_params(41, 0.02), synth.generator_params(61, 0.02)]
    multi = MultiPairEngine(_cfg(**keys), None, gens, (64, 64), (64, 64), vit_engine=vit)
    A2, B2 = torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()
    rows = []
    for _ in range(3):
        multi.step(A2, B2, A2)
        rows.append(multi.losses_dev.clone())
    for p in range(2):
        single = SpliceEngine(_cfg(**keys), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for k in range(3):
            single.step(pairs[p][0], pairs[p][1], pairs[p][0])
            assert torch.equal(_bits(single.losses_dev[0]), _bits(rows[k][p])), (p, k)
        a, b = _arenas(multi, p), _arenas(single)
        for name in a:
            assert torch.equal(_bits(a[name]), _bits(b[name])), (p, name)
        assert a["losses"][6] > 0 and a["losses"][7] > 0


def test_off_is_off(vit):
    """both keys explicitly 0 = a config that lacks them, bit for bit after 3 steps"""
    A, B = _pair()
    zero = _engine(vit, lambda_global_tv=0.0, lambda_global_pixel_identity=0.0)
    cfg = {k: v for k, v in _cfg().items() if k not in ("lambda_global_tv", "lambda_global_pixel_identity")}
    lacks = SpliceEngine(cfg, None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64), vit_engine=vit)
    for _ in range(3):
        zero.step(A, B, A)
        lacks.step(A, B, A)
    a, b = _arenas(zero), _arenas(lacks)
    for name in a:
        assert torch.equal(_bits(a[name]), _bits(b[name])), name
    assert torch.equal(_bits(zero.grads), _bits(lacks.grads)) and not zero.losses_dev[0, 6:].any()
    assert not set(IMAGE_LOSS_KEYS) & set(zero.losses())


# ------------------------------------------------------------------------------------------------ refusals and composition
def test_refusals_launch_nothing(vit):
    L = _lib.lib()
    x, d0 = _grid(1, 1, 3, 3, 5), torch.randn(1, 3, 3, 5, generator=torch.Generator().manual_seed(1))
    for lam in (-0.5, float("nan"), float("inf")):
        got, rc, untouched = _grad_add(x, None, d0, lam)
        assert rc != 0 and untouched, lam
    # more chunks than partial slots: refused, the buffer is not written
    big = _grid(2, 1, 3, 67, 131).to(DEV)
    buf = torch.full((8 + 8 * 4,), -7.5, device=DEV)
    assert L.splice_image_terms_value(_lib.ptr(big), 1, 67, 131, None, None, 0, 0, 0, _lib.ptr(buf), 8 + 8 * 4, 4, _st()) != 0 and b"partial slots" in L.splice_last_error()
    assert L.splice_image_terms_value(None, 0, 0, 0, None, None, 0, 0, 0, _lib.ptr(buf), 8 + 8 * 4, 4, _st()) != 0
    assert L.splice_total_loss_pairs_img(_lib.ptr(buf), 8 + 6 * 4, 4, 1.0, 1.0, 1.0, 1.0, 1.0, None, 1, 1, 1, 1, 1, None, 1, 1, 1.0, 1.0, _st()) != 0   # lstride < 8 + 8 lp
    assert L.splice_total_loss_pairs_img(_lib.ptr(buf), 8 + 8 * 4, 4, 1.0, 1.0, 1.0, 1.0, 1.0, None, 1, 1, 1, 1, 1, None, 1, 1, -1.0, 1.0, _st()) != 0
    torch.cuda.synchronize()
    assert (buf == -7.5).all()
    # the setter: a negative or non-finite weight; a gradient-only handle; a follower; after a run -- and a handle with the terms refuses
    # gradient-only and phase mode in turn
    A, B = _pair()
    eng = _engine(vit)
    for bad in ((-1.0, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("inf"))):
        assert L.splice_step_set_image_terms(eng.handle, *bad) != 0 and b"finite" in L.splice_last_error(), bad
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert L.splice_step_set_image_terms(eng.handle, 0.1, 0.1) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    lead = _engine(vit)
    assert L.splice_step_set_phases(eng.handle, 2, lead.handle) == 0
    assert L.splice_step_set_image_terms(eng.handle, 0.1, 0.1) != 0 and b"phase mode" in L.splice_last_error()
    assert L.splice_step_set_phases(eng.handle, 7, None) == 0
    assert L.splice_step_set_phases(eng.handle, 3, None) == 0
    assert L.splice_step_set_image_terms(eng.handle, 0.1, 0.1) != 0 and b"phase mode" in L.splice_last_error()
    assert L.splice_step_set_phases(eng.handle, 7, None) == 0
    eng.step(A, B, A)
    assert L.splice_step_set_image_terms(eng.handle, 0.1, 0.1) != 0 and b"before the first step" in L.splice_last_error()
    assert not eng.losses_dev[0, 6:].any()
    on = _engine(vit, lambda_global_tv=0.1)
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"image-space" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 2, lead.handle) != 0 and b"image-space" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 3, None) != 0


def test_stop_rule_sees_the_extended_total(vit):
    """stop_window 2: the stop record's window sums are those of the NumPy rule fed the reported totals, which include the terms"""
    A, B = _pair()
    rule = dict(stop_window=2, stop_rel=0.01, stop_patience=50, stop_min_steps=0)
    eng = _engine(vit, cls_warmup=1, entire_A_every=4, lambda_global_tv=4.0, lambda_global_pixel_identity=50.0, **rule)
    off = _engine(vit, cls_warmup=1, entire_A_every=4, **rule)
    totals, totals_off = [], []
    for _ in range(8):
        eng.step(A, B, A)
        off.step(A, B, A)
        totals.append(eng.losses_dev[0, 0].item())
        totals_off.append(off.losses_dev[0, 0].item())
    counted = [stop_window_closes(k, 1, 1, 4) for k in range(8)]
    want = np_plateau(np.array(totals, dtype=f32), counted, 2, 0.01, 50, 0)
    s, count, windows, best, bad, stop_step = eng._stop_records()[0]
    assert (count, windows, bad, stop_step) == (want["count"], want["windows"], want["bad"], want["stop_step"]) and windows == 3
    assert f32(s).tobytes() == want["sum"].tobytes() and f32(best).tobytes() == want["best"].tobytes()
    assert all(a > b for a, b in zip(totals, totals_off)) and f32(best) != f32(off._stop_records()[0][3])


def test_snapshot_is_refused_under_another_weight(vit):
    A, B = _pair()
    eng = _engine(vit, lambda_global_tv=0.25)
    eng.step(A, B, A)
    state = eng.snapshot(0)
    with pytest.raises(ValueError, match="lambda_global_tv"):
        _engine(vit).restore([state])
    same = _engine(vit, lambda_global_tv=0.25)
    same.restore([state])
    eng.step(A, B, A)
    same.step(A, B, A)
    assert torch.equal(_bits(same.params), _bits(eng.params)) and torch.equal(_bits(same.losses_dev), _bits(eng.losses_dev))


@pytest.mark.parametrize("key", ["lambda_global_tv", "lambda_global_pixel_identity"])
def test_multi_scale_engine_refuses_the_keys(key):
    with pytest.raises(NotImplementedError, match=key):
        MultiScaleEngine(_cfg(**{key: 0.1}), None, None, (64, 64), None, scales=(64,))
