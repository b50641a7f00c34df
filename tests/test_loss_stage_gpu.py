"""GPU: the loss stage AS THE FUSED STEP RUNS IT -- selfsim_tgt / selfsim_loss / selfsim_dk (upper-triangular tiles, mirror tiles,
norms from the operand stream, per-tile row / column partial dots, the fp8 variant), mse_batched_kernel (pair strides, the per-pair
gradient table) and total_loss_kernel (crop slots, per-pair lambda tables, schedule gates) -- through the test hooks
splice_selfsim_loss_pairs / splice_mse_pairs / splice_total_loss_pairs, which call the step's own launchers with the step's operand
layout.  References and every tolerance come from oracle/loss_stage.py: fp64 torch-CPU, worst-case bounds derived from the reference
alone (tests/test_loss_stage_cpu.py checks them without a GPU).  Bit-identity where the kernels promise it: padding contents, the
other pairs of a batch, a per-pair table against the scalar weight.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import loss_stage as ls
from splice_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_BITS = 0x7FC0DEAD      # a quiet NaN with a payload: what the kernels must leave alone
PART_FILL = -123.0         # prefill of partial slots
ERR_ARG = -1               # SPLICE_ERR_ARG
LAM = ls.LAMBDA
EPS = ls.EPS


def _st():
    return _lib.current_stream()


def _at(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _nan_filled(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.contiguous().view(torch.int32).cpu()


def _f32(x):
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ structure term
@functools.lru_cache(maxsize=None)
def _struct_ref(T, D, regime, seed):
    """keys, fp64 loss / dK and their bounds of one pair: computed once, shared, never modified"""
    Kt, Kx = ls.fp8_case(T, D, seed) if regime == "fp8" else ls.structure_case(T, D, regime, seed)
    loss, dK = ls.structure_ref(Kx, Kt, LAM, EPS)
    loss_b, dk_b = ls.structure_bounds(Kx, Kt, LAM, EPS)
    return Kt, Kx, loss, dK, loss_b, dk_b


def _ntiles(T):
    nt = (T + 63) // 64
    return nt * (nt + 1) // 2


def _run_structure(keys, T, D, lddk=None, pad=1e3, fp8=0, tab=None, lam=LAM, part_pstride=None):
    """One splice_selfsim_loss_pairs call in the step's layout: keys at column offset D of bf16 [pairs * Tld][3D] matrices (targets and
    generated), the transpose as rows D..2D-1 of a [3D][pairs * Tld] matrix (ldt = pairs * Tld, kT_pstride = Tld).  Everything that is
    not a key -- padding rows, padding columns of the transpose, the q / v parts -- holds `pad`.  Returns (rc, partials
    [pairs][part_pstride] fp32, dK bit patterns int32 [pairs][Tld][lddk]), both on the host."""
    pairs, Tld = len(keys), ls.tld(T)
    lddk = lddk or D
    part_pstride = _ntiles(T) + 3 if part_pstride is None else part_pstride
    m_t = torch.full((pairs * Tld, 3 * D), pad)
    m_x = torch.full((pairs * Tld, 3 * D), pad)
    m_xT = torch.full((3 * D, pairs * Tld), pad)
    for p, (Kt, Kx) in enumerate(keys):
        m_t[p * Tld:p * Tld + T, D:2 * D] = Kt
        m_x[p * Tld:p * Tld + T, D:2 * D] = Kx
        m_xT[D:2 * D, p * Tld:p * Tld + T] = Kx.T
    m_t, m_x, m_xT = (m.to(torch.bfloat16).to(DEV) for m in (m_t, m_x, m_xT))
    L = _lib.lib()
    ws = torch.zeros(L.splice_selfsim_loss_pairs_ws_bytes(T, D, pairs), dtype=torch.uint8, device=DEV)
    part = torch.full((pairs, max(part_pstride, 1)), PART_FILL, device=DEV)
    dk = _nan_filled(pairs, Tld, lddk)
    tab_d = None if tab is None else torch.tensor(tab, dtype=torch.float32, device=DEV)
    rc = L.splice_selfsim_loss_pairs(_at(m_t, D), _at(m_x, D), 3 * D, Tld * 3 * D, _at(m_xT, D * pairs * Tld), pairs * Tld, Tld, T, D, pairs,
                                     lam, _lib.ptr(tab_d), fp8, EPS, _lib.ptr(part), part_pstride, _lib.ptr(dk), lddk, Tld * lddk,
                                     _lib.ptr(ws), _st())
    torch.cuda.synchronize()
    return rc, part.cpu(), _bits(dk)


def _check_structure(tag, refs, T, D, part, dk_bits):
    """loss and every dK element inside the derived bounds; what must not be written keeps its prefill"""
    nt = _ntiles(T)
    assert (part[:, nt:] == PART_FILL).all(), "partial slots beyond nt (nt + 1) / 2 were written"
    assert (dk_bits[:, T:, :] == NAN_BITS).all(), "dK rows >= T were written"
    assert (dk_bits[:, :, D:] == NAN_BITS).all(), "the dK pitch gap was written"
    dk = dk_bits.view(torch.float32)[:, :T, :D].double()
    for p, (Kt, Kx, loss, dK, loss_b, dk_b) in enumerate(refs):
        got = LAM * part[p, :nt].double().sum().item()
        assert torch.isfinite(dk[p]).all()
        r_loss = abs(got - loss) / loss_b
        r_dk = ((dk[p] - dK).abs() / dk_b.clamp(min=1e-300)).max().item()
        normwise = ((dk[p] - dK).norm() / dK.norm()).item()
        print(f"LOSS_STAGE {tag} pair {p}: loss err/bound {r_loss:.1e}, dK worst err/bound {r_dk:.3f}, dK norm-wise {normwise:.2e}")
        assert r_loss <= 1.0, (got, loss, loss_b)
        assert r_dk <= 1.0, r_dk
        assert normwise < 1e-2, normwise


@pytest.mark.parametrize("regime", ls.STRUCT_REGIMES)
@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("T,D", ls.STRUCT_SHAPES)
def test_structure_bf16_against_fp64(T, D, pairs, regime):
    """(64, 64): one tile; (65, 384): the second tile row holds one valid row and Tp = 128 > Tld = 96; (129, 128): three tile rows;
    (197, 384): ten tiles.  T > 64 carries one all-zero row in Kx (the eps gate).  Then padding independence: another finite sentinel
    in every padding row / column and another dK pitch give the same bits."""
    refs = [_struct_ref(T, D, regime, p + 1) for p in range(pairs)]
    keys = [(r[0], r[1]) for r in refs]
    rc, part, dk = _run_structure(keys, T, D, lddk=D, pad=1e3)
    assert rc == 0
    _check_structure(f"bf16 T={T} D={D} pairs={pairs} {regime}", refs, T, D, part, dk)
    rc, part2, dk2 = _run_structure(keys, T, D, lddk=D + 8, pad=-7e5)
    assert rc == 0
    assert (dk2[:, T:, :] == NAN_BITS).all() and (dk2[:, :, D:] == NAN_BITS).all()
    assert torch.equal(_bits(part), _bits(part2)), "the loss partials depend on what the padding holds"
    assert torch.equal(dk[:, :T, :D], dk2[:, :T, :D]), "dK depends on what the padding holds (or on its pitch)"


@pytest.mark.parametrize("regime", ls.STRUCT_REGIMES)
@pytest.mark.parametrize("T,D", ls.STRUCT_SHAPES)
def test_structure_pair_equals_its_own_call(T, D, regime):
    keys = [_struct_ref(T, D, regime, p + 1)[:2] for p in range(3)]
    rc, part, dk = _run_structure(keys, T, D)
    assert rc == 0
    for p in range(3):
        rc, part1, dk1 = _run_structure(keys[p:p + 1], T, D)
        assert rc == 0
        assert torch.equal(_bits(part[p]), _bits(part1[0])), p
        assert torch.equal(dk[p], dk1[0]), p


@pytest.mark.parametrize("T,D", [(65, 384), (197, 384)])
def test_structure_e_scale_table(T, D):
    """entries {x, 0, x}: pair 1 writes nothing; pairs 0 and 2 are the scalar-weight run bit for bit (x = the step's fp32 e_scale)"""
    keys = [_struct_ref(T, D, "near_target", p + 1)[:2] for p in range(3)]
    x = np.float32(4.0) * np.float32(LAM) * (np.float32(1.0) / (np.float32(T) * np.float32(T)))
    rc, part, dk = _run_structure(keys, T, D)
    assert rc == 0
    rc, part_t, dk_t = _run_structure(keys, T, D, tab=[float(x), 0.0, float(x)], lam=12345.0)   # (the scalar is not read with a table)
    assert rc == 0
    assert (part_t[1] == PART_FILL).all() and (dk_t[1] == NAN_BITS).all()
    for p in (0, 2):
        assert torch.equal(_bits(part[p]), _bits(part_t[p])), p
        assert torch.equal(dk[p], dk_t[p]), p


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("T,D", ls.FP8_SHAPES)
def test_structure_fp8_against_fp64(T, D, pairs):
    """Keys whose row quantisation is exact (oracle.loss_stage.fp8_case), so the fp8 Gram is the cosine up to fp32 accumulation order
    and the bf16 reference and bounds apply unchanged: the row scales cancel, W and r take the TRUE norms, the fp8 tile walk is right.
    The quantiser itself is pinned by test_quantize_rows_matches_e4m3fn.  No zero key row here: what the quantiser does at amax = 0
    is not the subject."""
    refs = [_struct_ref(T, D, "fp8", p + 1) for p in range(pairs)]
    keys = [(r[0], r[1]) for r in refs]
    rc, part, dk = _run_structure(keys, T, D, lddk=D + 8, fp8=1)
    assert rc == 0
    _check_structure(f"fp8 T={T} D={D} pairs={pairs}", refs, T, D, part, dk)


def test_structure_refusals_launch_nothing():
    keys = [ls.structure_case(65, 64, "independent", 1)]
    rc, part, dk = _run_structure(keys, 65, 64, fp8=1)                     # fp8 needs D % 128 == 0
    assert rc == ERR_ARG
    assert (part == PART_FILL).all() and (dk == NAN_BITS).all()
    keys = [_struct_ref(129, 128, "independent", 1)[:2]]
    rc, part, dk = _run_structure(keys, 129, 128, part_pstride=_ntiles(129) - 1)   # 6 tiles, 5 slots
    assert rc == ERR_ARG
    assert (part == PART_FILL).all() and (dk == NAN_BITS).all()


# ------------------------------------------------------------------------------------------------ batched MSE
def _mse_inputs(pairs, rows, cols, lda, ldb, a_ps, b_ps, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((pairs - 1) * a_ps + rows * lda, generator=g)
    b = torch.randn((pairs - 1) * b_ps + rows * ldb, generator=g)
    return a, b


def _view(flat, p, ps, rows, cols, ld):
    return torch.as_strided(flat, (rows, cols), (ld, 1), p * ps)


def _run_mse(a, b, pairs, rows, cols, lda, ldb, a_ps, b_ps, ldg, g_ps, lw, gw, tab=None, part_ps=ls.MSE_MAX_WG + 8):
    ad, bd = a.to(DEV), b.to(DEV)
    part = torch.full((pairs, part_ps), PART_FILL, device=DEV)
    grad = _nan_filled((pairs - 1) * g_ps + rows * ldg)
    tab_d = None if tab is None else torch.tensor(tab, dtype=torch.float32, device=DEV)
    rc = _lib.lib().splice_mse_pairs(_lib.ptr(ad), lda, a_ps, _lib.ptr(bd), ldb, b_ps, rows, cols, lw, gw, _lib.ptr(part), part_ps, _lib.ptr(grad),
                                     ldg, g_ps, pairs, _lib.ptr(tab_d), _st())
    torch.cuda.synchronize()
    assert rc == 0
    return part.cpu(), _bits(grad)


# (rows, cols, lda = ldb, pair stride of a / b, ldg, pair stride of grad): the [CLS] form (one row of a [Tld][D] pass), the key-identity
# form (keys inside fp32 [Tld][3D] qkv, gradient into [Tld][D]) and the smallest shape over the 1024 x 256 grid cap (the grid-stride
# loop wraps: 268 800 elements)
_TLD, _D = ls.tld(65), 384
MSE_FORMS = {"cls": (1, _D, _D, _TLD * _D, _D, _TLD * _D),
             "identity": (65, _D, 3 * _D, _TLD * 3 * _D, _D, _TLD * _D),
             "wrap": (700, _D, _D, 700 * _D, _D + 8, 700 * (_D + 8))}


@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("form", sorted(MSE_FORMS))
def test_mse_pairs_against_fp64(form, pairs):
    rows, cols, ld, ps, ldg, g_ps = MSE_FORMS[form]
    n = rows * cols
    a, b = _mse_inputs(pairs, rows, cols, ld, ld, ps, ps, seed=50 + rows)
    lw, gw = 1.0, 10.0                                        # the step's: raw loss partials, lambda on the gradient
    gmean = _f32(np.float32(gw) / np.float32(n))
    part, grad = _run_mse(a, b, pairs, rows, cols, ld, ld, ps, ps, ldg, g_ps, lw, gw)
    nwg = min(-(-n // 256), ls.MSE_MAX_WG)
    assert (part[:, nwg:] == PART_FILL).all()
    written = torch.zeros(grad.numel(), dtype=torch.bool)
    worst_l = worst_g = 0.0
    for p in range(pairs):
        ref_part, ref_grad = ls.mse_ref(_view(a, p, ps, rows, cols, ld), _view(b, p, ps, rows, cols, ld), lw, gmean)
        got_part = part[p, :nwg].double()
        assert ((got_part - ref_part).abs() <= ls.MSE_LOSS_REL * ref_part).all()
        total, ref_total = got_part.sum().item(), ref_part.sum().item()
        assert abs(total - ref_total) <= ls.MSE_LOSS_REL * ref_total
        got_grad = _view(grad.view(torch.float32), p, g_ps, rows, cols, ldg).double()
        assert ((got_grad - ref_grad).abs() <= ls.MSE_GRAD_REL * ref_grad.abs()).all()
        worst_l = max(worst_l, ((got_part - ref_part).abs() / (ls.MSE_LOSS_REL * ref_part)).max().item())
        worst_g = max(worst_g, ((got_grad - ref_grad).abs() / (ls.MSE_GRAD_REL * ref_grad.abs()).clamp(min=1e-300)).max().item())
        _view(written, p, g_ps, rows, cols, ldg).fill_(True)
    print(f"LOSS_STAGE mse {form} pairs={pairs}: partial worst err/bound {worst_l:.3f}, grad worst err/bound {worst_g:.3f}")
    assert (grad[~written] == NAN_BITS).all(), "gradient written outside [rows][cols] of a pair"
    if pairs == 3:   # per-pair gradient table with a zero entry: that pair is left alone, the others are the scalar call bit for bit
        part_t, grad_t = _run_mse(a, b, pairs, rows, cols, ld, ld, ps, ps, ldg, g_ps, lw, 777.0, tab=[gmean, 0.0, gmean])
        assert (part_t[1] == PART_FILL).all()
        own1 = torch.zeros_like(written)
        _view(own1, 1, g_ps, rows, cols, ldg).fill_(True)
        assert (grad_t[own1] == NAN_BITS).all()
        assert torch.equal(_bits(part[[0, 2]]), _bits(part_t[[0, 2]]))
        assert torch.equal(grad[~own1], grad_t[~own1])


def test_mse_pairs_unequal_crop_form_lands_in_the_documented_slots():
    """several pairs with nA != nB crops: one launch per crop index i, pair p's x'_i against its B'_i into slot p * nc + i of the
    [CLS] term -- part_ps = nc * lstride with the base offset by i * lstride"""
    pairs, na, nb, nc, lp, K_CLS = 2, 3, 2, 2, ls.MSE_MAX_WG, 4
    lstride, passD = 8 + 6 * lp, _TLD * _D
    g = torch.Generator().manual_seed(77)
    x, bt = torch.randn(pairs * na * passD, generator=g), torch.randn(pairs * nb * passD, generator=g)
    xd, bd = x.to(DEV), bt.to(DEV)
    buf = torch.full((pairs * nc * lstride,), PART_FILL, device=DEV)
    grad = _nan_filled(pairs * na * passD)
    gw = 10.0
    gmean = _f32(np.float32(gw) / np.float32(_D))
    for i in range(nc):
        rc = _lib.lib().splice_mse_pairs(_at(xd, i * passD), _D, na * passD, _at(bd, i * passD), _D, nb * passD, 1, _D, 1.0, gw,
                                         _at(buf, 8 + K_CLS * lp + i * lstride), nc * lstride, _at(grad, i * passD), _D, na * passD, pairs, None, _st())
        assert rc == 0
    torch.cuda.synchronize()
    buf, grad = buf.cpu(), _bits(grad)
    expect_written = torch.zeros(buf.numel(), dtype=torch.bool)
    gwritten = torch.zeros(grad.numel(), dtype=torch.bool)
    nwg = -(-_D // 256)
    for p in range(pairs):
        for i in range(nc):
            a_v = x[(p * na + i) * passD:(p * na + i) * passD + _D][None]
            b_v = bt[(p * nb + i) * passD:(p * nb + i) * passD + _D][None]
            ref_part, ref_grad = ls.mse_ref(a_v, b_v, 1.0, gmean)
            o = (p * nc + i) * lstride + 8 + K_CLS * lp
            assert ((buf[o:o + nwg].double() - ref_part).abs() <= ls.MSE_LOSS_REL * ref_part).all(), (p, i)
            expect_written[o:o + nwg] = True
            go = (p * na + i) * passD
            got = grad[go:go + _D].view(torch.float32).double()
            assert ((got - ref_grad[0]).abs() <= ls.MSE_GRAD_REL * ref_grad[0].abs()).all(), (p, i)
            gwritten[go:go + _D] = True
    assert (buf[~expect_written] == PART_FILL).all()
    assert (grad[~gwritten] == NAN_BITS).all()


# ------------------------------------------------------------------------------------------------ total
def _run_total(buf, lstride, lp, pairs, n, w, wtab=None, ssim_on=1, entire=1):
    bd = buf.to(DEV)
    out8 = _nan_filled(pairs + 1, 8)
    wt = None if wtab is None else wtab.to(DEV)
    rc = _lib.lib().splice_total_loss_pairs(_lib.ptr(bd), lstride, lp, w[0], w[1], w[2], w[3], w[4], _lib.ptr(out8), pairs, n["a"], n["b"], n["c"],
                                            n["e"], _lib.ptr(wt), ssim_on, entire, _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert (_bits(out8[pairs]) == NAN_BITS).all()
    return out8[:pairs].cpu(), bd.cpu()


def _pair1_alone(buf, lstride, lp, n):
    """a buffer in which pair 1's slots of every term are pair 0's"""
    ns = max(n.values())
    one = torch.zeros(ns * lstride)
    for k, (_, which) in ls.TOTAL_TERMS.items():
        for s in range(n[which]):
            src = (n[which] + s) * lstride + 8 + k * lp
            one[s * lstride + 8 + k * lp:s * lstride + 8 + (k + 1) * lp] = buf[src:src + lp]
    return one


@pytest.mark.parametrize("mixed", [False, True], ids=["nonneg", "mixed"])
@pytest.mark.parametrize("slots", [(1, 1, 1, 1), (3, 2, 2, 1)], ids=["slots1", "slots3221"])
@pytest.mark.parametrize("lp", [70, 1024])
def test_total_loss_pairs_against_fp64(lp, slots, mixed):
    """lp = 70: a lane tail; 1024: the step's floor.  Scalar weights, then a per-pair table whose gates switch terms off."""
    pairs = 2
    n = dict(zip("abce", slots))
    lstride = 8 + 6 * lp + 4
    g = torch.Generator().manual_seed(lp + slots[0])
    buf = torch.rand(pairs * max(slots) * lstride, generator=g) - (0.5 if mixed else 0.0)
    w = [_f32(x) for x in (10.0, 0.1, 3.0, 0.25, 1.0)]
    wtab = torch.tensor([[1.0, 10.0, 2.0, 0.5, 0.25], [0.3, 1.0, 0.7, 1.0, 1.5]])
    for tag, kw in (("scalar", {}), ("table gated", dict(wtab=wtab, ssim_on=0, entire=1)), ("table", dict(wtab=wtab, ssim_on=1, entire=0))):
        out8, after = _run_total(buf, lstride, lp, pairs, n, w, **kw)
        ref, bound = ls.total_ref(buf, lstride, lp, pairs, n, w, **kw)
        err = (out8.double() - ref).abs()
        print(f"LOSS_STAGE total lp={lp} slots={slots} mixed={mixed} {tag}: worst err/bound {(err[:, :6] / bound[:, :6].clamp(min=1e-300)).max().item():.3f}")
        assert (err[:, :6] <= bound[:, :6]).all(), (err, bound)
        assert (out8[:, 6:] == 0).all()
        for p in range(pairs):   # the slot's own values [0..5] hold the same numbers; the partials are not touched
            assert torch.equal(_bits(after[p * lstride:p * lstride + 6]), _bits(out8[p, :6]))
        keep = torch.ones(buf.numel(), dtype=torch.bool)
        for p in range(pairs):
            keep[p * lstride:p * lstride + 6] = False
        assert torch.equal(_bits(after[keep]), _bits(buf[keep]))
        if "gated" in tag:   # ssim_on = 0: the structure and identity weights are off, whatever the table holds
            assert abs(out8[0, 0].item() - (0.25 * ref[0, 2] + 0.5 * ref[0, 3] + 1.0 * ref[0, 4]).item()) <= bound[0, 0].item()
        # pair 1 of the 2-pair call is its own call, bit for bit
        kw1 = dict(kw)
        if "wtab" in kw1:
            kw1["wtab"] = wtab[1:2].clone()
        alone, _ = _run_total(_pair1_alone(buf, lstride, lp, n), lstride, lp, 1, n, w, **kw1)
        assert torch.equal(_bits(alone[0]), _bits(out8[1]))
