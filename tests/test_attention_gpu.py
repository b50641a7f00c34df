"""GPU: the full-sequence attention kernels held ELEMENT BY ELEMENT to fp64 -- attn_fwd_x32_kernel (plain and pre-scaled q, 2 / 4 / 8 waves), the
32x32x16 backward halves in their three launch forms, the 16x16x32 backward halves, attn_delta_kernel, the e4m3 forward in its five forms and
attn_probs_kernel -- through the op-level C entry points, over a list of sequence lengths that reaches every class of tile walk (prologue
branches, main-loop trips, tail lengths, ring phases, masked-tile forms, Tld % 64, idle waves; oracle/attention.py, asserted on the CPU by
tests/test_attention_cpu.py).  References, bounds and the rescale prediction come from oracle/attention.py: fp64 torch-CPU, worst-case bounds
from the reference and the number formats alone.  Every output sits between guard rows; fp32 outputs are pre-filled with a NaN pattern.  The
backward is handed the REFERENCE's out and lse (independent of the forward kernel); CHAIN_T feeds it the forward kernel's own.  Exact
statements: launch forms agree bit for bit, padding rows of dqkv are zeros in all three column blocks, and no bit of a valid row depends on
what the padding rows hold.  Every case prints `ATTN <kernel> <case>: worst err/bound ...`.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import attention as at
from splice_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_BITS = 0x7FC0DEAD      # a quiet NaN with a payload: what a kernel must leave alone, and what an unwritten fp32 element still holds
BF_FILL = -7.0             # prefill of bf16 outputs
GUARD = 8                  # rows in front of and behind every output
ERR_ARG = -1               # SPLICE_ERR_ARG
D0, H0, B0 = at.BASE_GEOM
CASES = [(T, D0, H0, B0) for T in at.ATTN_T] + at.WIDE_CASES
FWD_VARIANTS = (0, 41, 42, 48)
FP8_VARIANTS = (0, 1, 11, 2, 12)


def _st():
    return _lib.current_stream()


def _at(t, elems):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def _ratio(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


class _Guarded:
    """an output of `rows` rows of `width` between GUARD rows on either side; bf16: BF_FILL everywhere, fp32: the NaN pattern"""

    def __init__(self, rows, width, dtype):
        self.rows, self.width, self.dtype = rows, width, dtype
        if dtype == torch.bfloat16:
            self.t = torch.full((rows + 2 * GUARD, width), BF_FILL, dtype=dtype, device=DEV)
        else:
            self.t = torch.full((rows + 2 * GUARD, width), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)

    def ptr(self):
        return _at(self.t, GUARD * self.width)

    def body(self):
        return self.t[GUARD:GUARD + self.rows]

    def guards_intact(self):
        g = torch.cat([self.t[:GUARD], self.t[GUARD + self.rows:]])
        return bool((g == BF_FILL).all()) if self.dtype == torch.bfloat16 else bool((_bits(g) == NAN_BITS).all())

    def untouched(self):
        return self.guards_intact() and (bool((self.body() == BF_FILL).all()) if self.dtype == torch.bfloat16 else bool((_bits(self.body()) == NAN_BITS).all()))


def _dev_bf16(x):
    """fp32 (bf16-exact) [B][rows][W] -> device bf16 [B * rows][W]"""
    return x.reshape(-1, x.shape[-1]).to(torch.bfloat16).to(DEV)


def _run_fwd(qkv, T, H, fold, variant):
    """splice_attention_fwd on guarded buffers: (out bf16 host [B][Tld][D], lse fp32 host [B][H][Tld])"""
    B, Tld, D3 = qkv.shape
    D = D3 // 3
    L = _lib.lib()
    q = _dev_bf16(qkv)
    out, lse = _Guarded(B * Tld, D, torch.bfloat16), _Guarded(B * H, Tld, torch.float32)
    L.splice_attention_qfold(int(fold))
    L.splice_attention_variant(variant)
    try:
        rc = L.splice_attention_fwd(_lib.ptr(q), None, 0, B, T, Tld, D, H, at.LN2 if fold else at.SCALE, out.ptr(), lse.ptr(), _st())
        torch.cuda.synchronize()
    finally:
        L.splice_attention_qfold(0)
        L.splice_attention_variant(0)
    assert rc == 0
    assert out.guards_intact() and lse.guards_intact(), "the forward wrote outside out / lse"
    assert not (_bits(lse.body()) == NAN_BITS).any(), "an lse element was never written"
    return out.body().cpu().reshape(B, Tld, D), lse.body().cpu().reshape(B, H, Tld)


def _run_fwd8(qkv, T, H, variant):
    B, Tld, D3 = qkv.shape
    D = D3 // 3
    L = _lib.lib()
    q8 = qkv.reshape(B * Tld, D3).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    q8T = q8.T.contiguous()
    out, lse = _Guarded(B * Tld, D, torch.bfloat16), _Guarded(B * H, Tld, torch.float32)
    L.splice_attention_variant(variant)
    try:
        rc = L.splice_attention_fwd_fp8(_lib.ptr(q8), _lib.ptr(q8T), B * Tld, B, T, Tld, D, H, at.SCALE, out.ptr(), lse.ptr(), _st())
        torch.cuda.synchronize()
    finally:
        L.splice_attention_variant(0)
    assert rc == 0
    assert out.guards_intact() and lse.guards_intact(), "the e4m3 forward wrote outside out / lse"
    assert not (_bits(lse.body()) == NAN_BITS).any(), "an lse element was never written"
    return out.body().cpu().reshape(B, Tld, D), lse.body().cpu().reshape(B, H, Tld)


def _run_bwd(qkv, T, H, fold, variant, out_bf, lse32, dout):
    """splice_attention_bwd on guarded buffers: (delta fp32 host [B][H][Tld], dqkv bit patterns int16 [B][Tld][3D])"""
    B, Tld, D3 = qkv.shape
    D = D3 // 3
    L = _lib.lib()
    q, o, d = _dev_bf16(qkv), _dev_bf16(out_bf), _dev_bf16(dout)
    ls = lse32.to(DEV).contiguous()
    delta, dqkv = _Guarded(B * H, Tld, torch.float32), _Guarded(B * Tld, D3, torch.bfloat16)
    L.splice_attention_qfold(int(fold))
    L.splice_attention_bwd_variant(variant)
    try:
        rc = L.splice_attention_bwd(_lib.ptr(q), None, 0, B, T, Tld, D, H, at.LN2 if fold else at.SCALE, _lib.ptr(o), _lib.ptr(ls), _lib.ptr(d), None,
                                    delta.ptr(), dqkv.ptr(), _st())
        torch.cuda.synchronize()
    finally:
        L.splice_attention_qfold(0)
        L.splice_attention_bwd_variant(0)
    assert rc == 0
    assert delta.guards_intact() and dqkv.guards_intact(), "the backward wrote outside delta / dqkv"
    assert not (_bits(delta.body()) == NAN_BITS).any(), "a delta element was never written"
    return delta.body().cpu().reshape(B, H, Tld), _bits(dqkv.body()).reshape(B, Tld, D3)


@functools.lru_cache(maxsize=8)
def _ref(T, D, H, B, regime, fold, fp8=False, ramp=None):
    """operands, fp64 forward reference and the operands with other padding rows and THEIR reference: computed once, shared, never modified"""
    qkv = at.make_qkv(T, D, H, B, regime, fold, fp8=fp8, ramp=ramp)
    qkv2 = at.make_qkv(T, D, H, B, regime, fold, pad_seed=1, fp8=fp8, ramp=ramp)
    if fp8:   # the padding variant is only run, never referenced
        return qkv, at.forward_ref(qkv, T, H), qkv2, None
    return qkv, at.forward_ref(qkv, T, H, fold), qkv2, at.forward_ref(qkv2, T, H, fold)


def _fwd_ratios(f, T, H, out, lse, E_lse, E_out):
    o = at.split_heads(out.double(), H)[0][:, :, :T]
    assert torch.isfinite(o).all() and torch.isfinite(lse[:, :, :T]).all()
    return _ratio((lse[:, :, :T].double() - f["lse"][:, :, :T]).abs(), E_lse), _ratio((o - f["out"][:, :, :T]).abs(), E_out)


# ------------------------------------------------------------------------------------------------ forward, bf16
@pytest.mark.parametrize("T,D,H,B", CASES)
def test_attention_forward_against_fp64(T, D, H, B):
    """attn_fwd_x32_kernel<2 | 4 | 8, plain | pre-scaled>: out and lse inside their bounds in the partner and flat regimes, the four launch forms
    bit for bit, and not a bit of rows < T depends on the padding rows"""
    for regime in at.REGIMES:
        for fold in (False, True):
            qkv, f, qkv2, _ = _ref(T, D, H, B, regime, fold)
            out, lse = _run_fwd(qkv, T, H, fold, 0)
            r_lse, r_out = _fwd_ratios(f, T, H, out, lse, *at.forward_bounds(f))
            print(f"ATTN fwd_x32 T={T} D={D} B={B} {regime} {'prescaled' if fold else 'plain'}: worst err/bound lse {r_lse:.3f}, out {r_out:.3f}")
            assert r_lse <= 1.0 and r_out <= 1.0, (regime, fold, r_lse, r_out)
            for v in FWD_VARIANTS[1:]:
                ov, lv = _run_fwd(qkv, T, H, fold, v)
                assert torch.equal(_bits(ov), _bits(out)) and torch.equal(_bits(lv), _bits(lse)), (regime, fold, v)
            o2, l2 = _run_fwd(qkv2, T, H, fold, 0)
            assert torch.equal(_bits(o2[:, :T]), _bits(out[:, :T])) and torch.equal(_bits(l2[:, :, :T]), _bits(lse[:, :, :T])), \
                f"{regime} {fold}: the forward depends on what the padding rows hold"


@pytest.mark.parametrize("T,tiles,level", at.RAMP_CASES)
def test_attention_forward_lazy_rescale_and_exact_walk(T, tiles, level):
    """Scores that step up by 46 log2 units at the named tiles for a few queries of a wave: the lazy rescale (l.337-353 of attn_x32.h) fires for
    exactly the predicted (query, tile) pairs -- tests/test_attention_cpu.py asserts the set -- and moves o, l, the point and the in-flight scores
    of the next tile.  Level 2 steps by 240: fp32 overflows and the wave takes the exact walk.  Both inside the bounds that count those steps."""
    D, H, B = at.BASE_GEOM
    nt = (T + 63) // 64
    for fold in (False, True):
        qkv, f, qkv2, _ = _ref(T, D, H, B, "ramp", fold, ramp=(tiles, level))
        fire, _, exact = at.rescale_plan(f)
        assert fire[:, :, :T].any() if level == 1 else exact[:, :, :T].any()
        out, lse = _run_fwd(qkv, T, H, fold, 0)
        r_lse, r_out = _fwd_ratios(f, T, H, out, lse, *at.forward_bounds(f, rescales=nt, exact=level == 2))
        print(f"ATTN fwd_x32 T={T} ramp tiles={tiles} level={level} {'prescaled' if fold else 'plain'}: worst err/bound lse {r_lse:.3f}, out {r_out:.3f}")
        assert r_lse <= 1.0 and r_out <= 1.0, (fold, r_lse, r_out)
        for v in FWD_VARIANTS[1:]:
            ov, lv = _run_fwd(qkv, T, H, fold, v)
            assert torch.equal(_bits(ov), _bits(out)) and torch.equal(_bits(lv), _bits(lse)), (fold, v)
        o2, l2 = _run_fwd(qkv2, T, H, fold, 0)
        assert torch.equal(_bits(o2[:, :T]), _bits(out[:, :T])) and torch.equal(_bits(l2[:, :, :T]), _bits(lse[:, :, :T]))


# ------------------------------------------------------------------------------------------------ backward
def _handed(f, T):
    """what the independent backward run is handed: bf16(reference out) [B][Tld][D] and fp32(reference lse) [B][H][Tld], all Tld rows"""
    return at.bf16_round(at.join_heads(f["out"]).float()), f["lse"].float()


def _bwd_check(tag, f, T, H, fold, dout, out_bf, delta, dq_bits, E_lse_in, E_out_in=None):
    B, Tld, D3 = dq_bits.shape
    D = D3 // 3
    r = at.backward_ref(f, dout, out_bf, E_lse_in, E_out_in)
    assert ((dq_bits[:, T:] & 0x7FFF) == 0).all(), f"{tag}: padding rows of dqkv are not zeros (q, k or v block)"
    assert (delta[:, :, T:] == 0).all(), f"{tag}: delta of a padding row (dO = 0) is not zero"
    got = at.split_heads(dq_bits.view(torch.bfloat16).double(), H)
    assert all(torch.isfinite(g).all() for g in got)
    c = at.C2 if fold else 1.0
    ratios = [_ratio((delta[:, :, :T].double() - r["delta"]).abs(), r["E_delta"]), _ratio((got[0][:, :, :T] * c - r["dq"]).abs(), r["E_dq"]),
              _ratio((got[1][:, :, :T] - r["dk"]).abs(), r["E_dk"]), _ratio((got[2][:, :, :T] - r["dv"]).abs(), r["E_dv"])]
    print(f"ATTN {tag}: worst err/bound delta {ratios[0]:.3f}, dq {ratios[1]:.3f}, dk {ratios[2]:.3f}, dv {ratios[3]:.3f}")
    assert max(ratios) <= 1.0, (tag, ratios)


@pytest.mark.parametrize("T,D,H,B", CASES)
def test_attention_backward_against_fp64(T, D, H, B):
    """The 32x32x16 halves (pre-scaled q; one launch, two launches, two-wave workgroups: same bits) and the 16x16x32 halves (plain q), handed the
    reference's out and lse: delta, dq, dk, dv inside their bounds, padding rows of dqkv zero in all three column blocks, and no bit of rows < T
    depends on the padding rows (whose own reference lse and out are handed along)."""
    dout = at.make_dout(T, D, B)
    for regime in at.REGIMES:
        for fold, forms, name in ((True, (2, 3, 4), "bwd_x32"), (False, (0,), "bwd_16x16")):
            qkv, f, qkv2, f2 = _ref(T, D, H, B, regime, fold)
            out_bf, lse32 = _handed(f, T)
            delta, dq_bits = _run_bwd(qkv, T, H, fold, forms[0], out_bf, lse32, dout)
            _bwd_check(f"{name} T={T} D={D} B={B} {regime}", f, T, H, fold, dout, out_bf, delta, dq_bits, at.U32 * f["lse"][:, :, :T].abs())
            for v in forms[1:]:
                dv_, bv = _run_bwd(qkv, T, H, fold, v, out_bf, lse32, dout)
                assert torch.equal(bv, dq_bits) and torch.equal(_bits(dv_), _bits(delta)), (regime, name, v)
            out2, lse2 = _handed(f2, T)
            assert torch.equal(out2[:, :T], out_bf[:, :T]) and torch.equal(lse2[:, :, :T], lse32[:, :, :T])
            d2, b2 = _run_bwd(qkv2, T, H, fold, forms[0], out2, lse2, dout)
            assert torch.equal(b2[:, :T], dq_bits[:, :T]) and torch.equal(_bits(d2[:, :, :T]), _bits(delta[:, :, :T])), \
                f"{regime} {name}: the backward depends on what the padding rows hold"


@pytest.mark.parametrize("T", at.CHAIN_T)
def test_attention_backward_chained_to_the_forward_kernel(T):
    """as the engine runs them: the forward kernel's own out and lse go into the backward; the bounds carry the forward's"""
    D, H, B = at.BASE_GEOM
    dout = at.make_dout(T, D, B)
    for fold, form, name in ((True, 0, "bwd_x32"), (False, 0, "bwd_16x16")):
        qkv, f, _, _ = _ref(T, D, H, B, "partner", fold)
        out, lse = _run_fwd(qkv, T, H, fold, 0)
        E_lse, E_out = at.forward_bounds(f)
        out_bf, _ = _handed(f, T)
        delta, dq_bits = _run_bwd(qkv, T, H, fold, form, out.float(), lse, dout)
        _bwd_check(f"{name} chained T={T}", f, T, H, fold, dout, out_bf, delta, dq_bits, E_lse, E_out + at.UBF * f["out"][:, :, :T].abs())


# ------------------------------------------------------------------------------------------------ e4m3 forward
@pytest.mark.parametrize("T", at.ATTN_T)
def test_attention_forward_fp8_against_fp64(T):
    """attn_fwd8_kernel<1 | 2, 1 | 2> on e4m3-exact operands (quantising them adds nothing): out inside the bound of P's e4m3 step and floor, lse
    inside what the fp8 MFMA can drop of a score (the row sum takes the unquantised P), the five forms bit for bit -- T <= 64 included, where the second wave group
    of the two-group forms walks no tile -- and padding independence.  The flat cases beyond two tiles hit the 448 limit past the first tile."""
    D, H, B = at.BASE_GEOM
    for regime in at.REGIMES:
        qkv, f, qkv2, _ = _ref(T, D, H, B, regime, False, True)
        hits = at.fp8_limit_hits(f)
        out, lse = _run_fwd8(qkv, T, H, 0)
        r_lse, r_out = _fwd_ratios(f, T, H, out, lse, *at.forward_bounds(f, fp8=True))
        print(f"ATTN fwd_fp8 T={T} {regime}: worst err/bound lse {r_lse:.3f}, out {r_out:.3f}; predicted 448-limit hits past the first tile {hits}")
        assert r_lse <= 1.0 and r_out <= 1.0, (regime, r_lse, r_out)
        assert hits > 0 or regime != "flat" or T <= 128
        for v in FP8_VARIANTS[1:]:
            ov, lv = _run_fwd8(qkv, T, H, v)
            assert torch.equal(_bits(ov), _bits(out)) and torch.equal(_bits(lv), _bits(lse)), (regime, v)
        o2, l2 = _run_fwd8(qkv2, T, H, 0)
        assert torch.equal(_bits(o2[:, :T]), _bits(out[:, :T])) and torch.equal(_bits(l2[:, :, :T]), _bits(lse[:, :, :T])), \
            f"{regime}: the e4m3 forward depends on what the padding rows hold"


# ------------------------------------------------------------------------------------------------ probabilities
@pytest.mark.parametrize("T", at.PROBS_T)
def test_attention_probs_against_fp64(T):
    D, H, B = at.BASE_GEOM
    Tld = at.tld(T)
    qkv, f, _, _ = _ref(T, D, H, B, "partner", False)
    lse32 = f["lse"].float().to(DEV).contiguous()
    q = _dev_bf16(qkv)
    probs = _Guarded(B * H * T, T, torch.float32)
    rc = _lib.lib().splice_attention_probs(_lib.ptr(q), B, T, Tld, D, H, at.SCALE, _lib.ptr(lse32), probs.ptr(), _st())
    torch.cuda.synchronize()
    assert rc == 0 and probs.guards_intact()
    got = probs.body().cpu().reshape(B, H, T, T)
    assert not (_bits(got) == NAN_BITS).any()
    r = _ratio((got.double() - f["P"][:, :, :T]).abs(), at.probs_bounds(f, at.U32 * f["lse"][:, :, :T].abs()))
    print(f"ATTN probs T={T}: worst err/bound {r:.3f}")
    assert r <= 1.0, r


# ------------------------------------------------------------------------------------------------ refusals
def test_attention_refusals_launch_nothing():
    """B < 1, T < 1, T > Tld, Tld % 32, D % 64, H != D / 64 and every NULL operand: SPLICE_ERR_ARG, and the pattern-filled outputs stay as they were"""
    T, D, H, B = 33, 128, 2, 2
    Tld = at.tld(T)
    qkv, f, _, _ = _ref(T, D, H, B, "flat", False)
    out_bf, lse32 = _handed(f, T)
    q, o, d = _dev_bf16(qkv), _dev_bf16(out_bf), _dev_bf16(at.make_dout(T, D, B))
    ls = lse32.to(DEV).contiguous()
    q8 = qkv.reshape(B * Tld, 3 * D).to(torch.float8_e4m3fn).view(torch.uint8).to(DEV)
    q8T = q8.T.contiguous()
    L = _lib.lib()
    good = dict(B=B, T=T, Tld=Tld, D=D, H=H)
    shapes = [dict(B=0), dict(B=-1), dict(T=0), dict(T=-3), dict(T=Tld + 1), dict(T=2 * Tld), dict(Tld=40, T=33), dict(D=96), dict(H=3)]
    nulls = ["qkv", "out", "lse", "dout", "delta", "dqkv", "probs", "qkv8", "qkvT8"]
    for change in shapes + [{n: None} for n in nulls]:
        a = dict(good)
        a.update({k: v for k, v in change.items() if k in good})
        null = next(iter(change)) if next(iter(change)) in nulls else None
        out, lse = _Guarded(B * Tld, D, torch.bfloat16), _Guarded(B * H, Tld, torch.float32)
        delta, dqkv = _Guarded(B * H, Tld, torch.float32), _Guarded(B * Tld, 3 * D, torch.bfloat16)
        probs = _Guarded(B * H * T, T, torch.float32)
        p = dict(qkv=_lib.ptr(q), out=out.ptr(), lse=lse.ptr(), dout=_lib.ptr(d), delta=delta.ptr(), dqkv=dqkv.ptr(), probs=probs.ptr(),
                 qkv8=_lib.ptr(q8), qkvT8=_lib.ptr(q8T), out_in=_lib.ptr(o), lse_in=_lib.ptr(ls))
        if null == "out":
            p["out_in"] = None
        if null == "lse":
            p["lse_in"] = None
        if null:
            p[null] = None
        args = (a["B"], a["T"], a["Tld"], a["D"], a["H"])
        if null in (None, "qkv", "out", "lse"):
            assert L.splice_attention_fwd(p["qkv"], None, 0, *args, at.SCALE, p["out"], p["lse"], _st()) == ERR_ARG, change
        if null in (None, "qkv8", "qkvT8", "out", "lse"):
            assert L.splice_attention_fwd_fp8(p["qkv8"], p["qkvT8"], B * Tld, *args, at.SCALE, p["out"], p["lse"], _st()) == ERR_ARG, change
        if null in (None, "qkv", "out", "lse", "dout", "delta", "dqkv"):
            assert L.splice_attention_bwd(p["qkv"], None, 0, *args, at.SCALE, p["out_in"], p["lse_in"], p["dout"], None, p["delta"], p["dqkv"],
                                          _st()) == ERR_ARG, change
        if null in (None, "qkv", "lse", "probs"):
            assert L.splice_attention_probs(p["qkv"], *args, at.SCALE, p["lse_in"], p["probs"], _st()) == ERR_ARG, change
        torch.cuda.synchronize()
        assert out.untouched() and lse.untouched() and delta.untouched() and dqkv.untouched() and probs.untouched(), change
    # and the same buffers with nothing wrong go through
    out, lse = _Guarded(B * Tld, D, torch.bfloat16), _Guarded(B * H, Tld, torch.float32)
    assert L.splice_attention_fwd(_lib.ptr(q), None, 0, B, T, Tld, D, H, at.SCALE, out.ptr(), lse.ptr(), _st()) == 0
    torch.cuda.synchronize()
    assert not out.untouched() and out.guards_intact()
