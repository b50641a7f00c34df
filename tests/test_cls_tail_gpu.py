"""GPU: the [CLS] tail of the top ViT block AS THE ENGINE RUNS IT in top_cls_only mode -- attn_cls_fwd / attn_cls_bwd (single-query attention:
the 1024-token trips, the CLS_NV prefetch and its tail loop, the nz = 1 / 2 / 4 store grid, padding rows and columns), ln_rows_fwd / ln_rows_bwd
(strided rows, split-K slab sums in batches of 16, three clamped columns per thread) and rows_finish (modes 0 / 1 / 2, the pre_lo gate, a NULL
pre_bf) -- through the test hooks splice_attn_cls_fwd / _bwd, splice_ln_rows_fwd / _bwd and splice_rows_finish, which call the engine's own
launchers on the caller's buffers.  References, bit-exact predictions and every bound come from oracle/cls_tail.py: fp64 torch-CPU, worst-case
bounds derived from the reference and the number formats alone (tests/test_cls_tail_cpu.py checks them, and that they bite, without a GPU).
Bit-identity where the kernels promise it: slab sums, dv, g_bf, padding contents, a pass of a batch against its own call, pass ranges of a
context.  Every case prints `CLS_TAIL ...` with its worst err / bound.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import cls_tail as ct
from splice_amd import _lib, synth

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_BITS = 0x7FC0DEAD      # a quiet NaN with a payload: what the kernels must leave alone (fp32 buffers)
BF_FILL = -7.0             # prefill of bf16 outputs
F_FILL = -12345.0          # prefill of fp32 statistics
ERR_ARG = -1               # SPLICE_ERR_ARG
GUARD = 8                  # rows in front of and behind dqkv that must stay


def _st():
    return _lib.current_stream()


def _at(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _nan_filled(*shape):
    return torch.full(shape, NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32).cpu()


def _ratio(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


def _padded_f32(rows, stride, cols, values=None):
    """device fp32 [rows][stride] of NaN bit patterns with `values` [rows][cols] in the leading columns; returns (tensor, host copy of its bits)"""
    t = _nan_filled(rows, stride)
    if values is not None:
        t[:, :cols] = values.to(DEV)
    torch.cuda.synchronize()
    return t, _bits(t)


# ------------------------------------------------------------------------------------------------ single-query attention
@functools.lru_cache(maxsize=None)
def _attn_ref(T, Tld, D, H, B, regime):
    """inputs, fp64 forward reference and bounds of every pass of a case: computed once, shared, never modified"""
    qkv = ct.attn_case(T, D, H, B, regime)
    per = []
    for b in range(B):
        p, out = ct.attn_ref(qkv[b], H)
        per.append((p, out) + ct.attn_fwd_bounds(qkv[b], H, Tld))
    return qkv, per


def _attn_buffers(qkv, Tld, pad):
    """the engine's layout on the device: bf16 [B * Tld][3D] and its transpose [3D][B * Tld]; everything outside the T valid rows of a pass holds `pad`"""
    B, T, D3 = qkv.shape
    m = torch.full((B, Tld, D3), pad)
    m[:, :T] = qkv
    m = m.reshape(B * Tld, D3)
    return m.to(torch.bfloat16).to(DEV), m.T.contiguous().to(torch.bfloat16).to(DEV)


def _run_attn_fwd(qkv, Tld, H, pad=1e3):
    B, T, D3 = qkv.shape
    D = D3 // 3
    m, mT = _attn_buffers(qkv, Tld, pad)
    out = torch.full((B + 1, D), BF_FILL, dtype=torch.bfloat16, device=DEV)
    probs = _nan_filled(B + 1, H, Tld)
    rc = _lib.lib().splice_attn_cls_fwd(_lib.ptr(m), _lib.ptr(mT), B * Tld, B, T, Tld, D, H, ct.SCALE, _lib.ptr(out), _lib.ptr(probs), _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert (out[B] == BF_FILL).all() and (_bits(probs[B]) == NAN_BITS).all(), "written behind the B passes"
    return out[:B].cpu(), probs[:B].cpu()


def _run_attn_bwd(qkv, Tld, H, probs, slabs, pad=1e3):
    """probs [B][H][Tld] fp32 (what lies beyond T is never read: NaN there), slabs [n][B][D].  Returns dqkv bit patterns [B][Tld][3D] (int16)."""
    B, T, D3 = qkv.shape
    D, n = D3 // 3, slabs.shape[0]
    m, mT = _attn_buffers(qkv, Tld, pad)
    stride = B * D + 24
    sl = _nan_filled(n, stride)
    sl[:, :B * D] = slabs.reshape(n, B * D).to(DEV)
    dqkv = torch.full((GUARD + B * Tld + GUARD, D3), BF_FILL, dtype=torch.bfloat16, device=DEV)
    probs_d = probs.to(DEV)
    rc = _lib.lib().splice_attn_cls_bwd(_lib.ptr(m), _lib.ptr(mT), B * Tld, B, T, Tld, D, H, ct.SCALE, _lib.ptr(probs_d), _lib.ptr(sl), n, stride,
                                        _at(dqkv, GUARD * D3), _st())
    torch.cuda.synchronize()
    assert rc == 0
    assert (dqkv[:GUARD] == BF_FILL).all() and (dqkv[GUARD + B * Tld:] == BF_FILL).all(), "dqkv written outside [B * Tld][3D]"
    return _bits(dqkv[GUARD:GUARD + B * Tld]).reshape(B, Tld, D3)


def _handed_probs(per, H, T, Tld):
    """the fp64 reference's probabilities rounded to fp32 (the backward is checked independently of the forward kernel), NaN beyond T"""
    p32 = torch.full((len(per), H, Tld), float("nan"))
    for b, (p, _, _, _) in enumerate(per):
        p32[b, :, :T] = p.float()
    return p32


def _check_attn_bwd(tag, qkv, per, Tld, H, slabs, dq_bits):
    B, T, D3 = qkv.shape
    D = D3 // 3
    got = dq_bits.view(torch.bfloat16).double()                       # [B][Tld][3D]
    assert (dq_bits[:, T:] == 0).all(), "dqkv rows T..Tld-1 are not all-zero bits"
    assert (got[:, 1:T, :D] == 0).all(), "dq slices of rows 1..T-1 are not zero"
    assert torch.isfinite(got).all()
    p32 = _handed_probs(per, H, T, Tld)
    worst = [0.0, 0.0]
    for b in range(B):
        dO = ct.attn_dO(slabs[:, b])
        r = ct.attn_bwd_ref(qkv[b], H, dO)
        E_dk, E_dq, _ = ct.attn_bwd_bounds(qkv[b], H, Tld, dO, ct.U32 * per[b][0], r=r)
        dv_pred = ct.attn_dv_pred(p32[b], dO, T)
        assert torch.equal(dq_bits[b, :T, 2 * D:], _bits(dv_pred.to(torch.bfloat16))), f"{tag} pass {b}: dv is not bf16(fp32(p dO)) bit for bit"
        r_dk = _ratio((got[b, :T, D:2 * D] - r["dk"]).abs(), E_dk)
        r_dq = _ratio((got[b, 0, :D] - r["dq"]).abs(), E_dq)
        worst = [max(worst[0], r_dk), max(worst[1], r_dq)]
        if T == 1:   # [CLS] alone: exact
            assert (got[b, 0, :2 * D] == 0).all() and torch.equal(got[b, 0, 2 * D:], dO.double())
    print(f"CLS_TAIL attn_bwd {tag}: dk worst err/bound {worst[0]:.3f}, dq {worst[1]:.3f}, dv bit-exact")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (tag, worst)


@pytest.mark.parametrize("T,Tld,D,H,B,regime", ct.ATTN_CASES)
def test_attn_cls_fwd_bwd_against_fp64(T, Tld, D, H, B, regime):
    """(1, 32): [CLS] alone, exact; (65, 96): nz = 1; (257, 288): nz = 2 with rows 256..287 on z = 1; (785, 800): nz = 4 and CLS_NV just covers
    it; (840, 864): the tail loop behind the prefetch; (1030, 1056): the second trip of the 1024-token loops.  Then padding independence
    (another finite sentinel in the padding rows of qkv and the padding columns of qkvT: same bits everywhere) and, at B = 3, every pass
    against its own B = 1 call."""
    qkv, per = _attn_ref(T, Tld, D, H, B, regime)
    tag = f"T={T} Tld={Tld} D={D} B={B} {regime}"
    out, probs = _run_attn_fwd(qkv, Tld, H)
    assert (_bits(probs)[:, :, T:] == 0).all(), "probs beyond T are not zero bit for bit"
    worst = [0.0, 0.0]
    for b, (p, o, Ep, Eout) in enumerate(per):
        worst = [max(worst[0], _ratio((probs[b, :, :T].double() - p).abs(), Ep)), max(worst[1], _ratio((out[b].double() - o).abs(), Eout))]
        if T == 1:
            assert (probs[b, :, 0] == 1).all() and torch.equal(out[b].float(), qkv[b, 0, 2 * D:])
    print(f"CLS_TAIL attn_fwd {tag}: probs worst err/bound {worst[0]:.3f}, out {worst[1]:.3f}")
    assert worst[0] <= 1.0 and worst[1] <= 1.0, (tag, worst)
    p32 = _handed_probs(per, H, T, Tld)
    dq6 = None
    for n in ct.ATTN_SLABS:
        slabs = ct.dout_slabs(B, D, n)
        dq_bits = _run_attn_bwd(qkv, Tld, H, p32, slabs)
        _check_attn_bwd(f"{tag} n_slabs={n}", qkv, per, Tld, H, slabs, dq_bits)
        if n == 6:
            dq6 = dq_bits
    # padding independence
    slabs = ct.dout_slabs(B, D, 6)
    out2, probs2 = _run_attn_fwd(qkv, Tld, H, pad=-7e5)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(probs), _bits(probs2)), "the forward depends on what the padding holds"
    assert torch.equal(dq6, _run_attn_bwd(qkv, Tld, H, p32, slabs, pad=-7e5)), "the backward depends on what the padding holds"
    if B > 1:
        for b in range(B):
            out1, probs1 = _run_attn_fwd(qkv[b:b + 1], Tld, H)
            assert torch.equal(_bits(out[b]), _bits(out1[0])) and torch.equal(_bits(probs[b]), _bits(probs1[0])), b
            assert torch.equal(dq6[b], _run_attn_bwd(qkv[b:b + 1], Tld, H, p32[b:b + 1], slabs[:, b:b + 1])[0]), b


# ------------------------------------------------------------------------------------------------ LayerNorm of strided rows
def _run_ln_fwd(c, rows, D, rows_arg=None, D_arg=None, **override):
    """one splice_ln_rows_fwd call with row strides larger than D; returns (rc, dict of host bit patterns / values, dict of prefill bit patterns)"""
    xs, ys, ss, rs = D + 8, D + 16, 3, D + 24
    slabs = c.get("slabs")
    n = 0 if slabs is None else slabs.shape[0]
    stride = rows * D + 8
    x, x0 = _padded_f32(rows + 1, xs, D, None if n else torch.cat([c["x"], torch.zeros(1, D)]))
    y = torch.full((rows + 1, ys), BF_FILL, dtype=torch.bfloat16, device=DEV)
    stat = torch.full((2, (rows + 1) * ss), F_FILL, device=DEV)
    gamma, beta = c["gamma"].to(DEV), c["beta"].to(DEV)
    sl = bias = resid = None
    if n:
        sl = _nan_filled(n, stride)
        sl[:, :rows * D] = slabs.reshape(n, rows * D).to(DEV)
        bias = c["bias"].to(DEV)
        resid, _ = _padded_f32(rows, rs, D, c["resid"])
    a = dict(x=_lib.ptr(x), gamma=_lib.ptr(gamma), beta=_lib.ptr(beta), y=_lib.ptr(y), mean=_lib.ptr(stat[0]), rstd=_lib.ptr(stat[1]),
             slabs=_lib.ptr(sl), n_slabs=n, bias=_lib.ptr(bias), resid=_lib.ptr(resid))
    a.update(override)
    rc = _lib.lib().splice_ln_rows_fwd(a["x"], xs, a["gamma"], a["beta"], a["y"], ys, a["mean"], a["rstd"], ss, rows if rows_arg is None else rows_arg,
                                       D if D_arg is None else D_arg, ct.LN_EPS, a["slabs"], a["n_slabs"], stride, a["bias"], a["resid"], rs, _st())
    torch.cuda.synchronize()
    return rc, dict(x=_bits(x), y=y.cpu(), stat=stat.cpu()), dict(x=x0)


def _ln_fwd_untouched(got, pre, rows, D, ss=3):
    return (got["y"] == BF_FILL).all() and (got["stat"] == F_FILL).all() and torch.equal(got["x"], pre["x"])


def _check_ln_fwd(tag, c, rows, D):
    rc, got, pre = _run_ln_fwd(c, rows, D)
    assert rc == 0
    ss = 3
    x_pred = ct.ln_x_pred(c)
    # the formed row bit for bit (or x left as it was), gaps and the row behind untouched
    expect = pre["x"].clone()
    if "slabs" in c:
        expect[:rows, :D] = _bits(x_pred)
    assert torch.equal(got["x"], expect), f"{tag}: x is not (bias + resid) + s_0 + ... bit for bit, or a gap was written"
    assert (got["y"][:rows, D:] == BF_FILL).all() and (got["y"][rows] == BF_FILL).all(), f"{tag}: y written outside its rows"
    stat = got["stat"].reshape(2, rows + 1, ss)
    assert (stat[:, :, 1:] == F_FILL).all() and (stat[:, rows] == F_FILL).all(), f"{tag}: statistics written outside their slots"
    f = ct.ln_fwd_ref(x_pred, c["gamma"], c["beta"])
    r = (_ratio((stat[0, :rows, 0].double() - f["mean"]).abs(), f["E_mean"]), _ratio((stat[1, :rows, 0].double() - f["rstd"]).abs(), f["E_rstd"]),
         _ratio((got["y"][:rows, :D].double() - f["y"]).abs(), f["E_y"]))
    print(f"CLS_TAIL ln_rows_fwd {tag}: mean worst err/bound {r[0]:.3f}, rstd {r[1]:.3f}, y {r[2]:.3f}, x bit-exact")
    assert max(r) <= 1.0, (tag, r)
    return got, stat


@pytest.mark.parametrize("n_slabs", ct.LN_FWD_SLABS)
@pytest.mark.parametrize("rows", ct.LN_ROWS)
@pytest.mark.parametrize("D", ct.LN_DIMS)
def test_ln_rows_fwd_against_fp64(D, rows, n_slabs):
    """D = 4: one column per row of threads; 100: no multiple of the wave; 384: half the threads surplus for the third column; 768: the limit.
    n_slabs = 0: x is read and not written; 17: the second LNR_SB trip (the engine stops at 16)."""
    _check_ln_fwd(f"D={D} rows={rows} n_slabs={n_slabs}", ct.ln_case(rows, D, n_slabs), rows, D)


@pytest.mark.parametrize("D", ct.LN_DIMS)
def test_ln_rows_fwd_zero_variance_and_large_mean_rows(D):
    """row 0 holds 1.5 everywhere (every partial sum exact): y == bf16(beta), rstd = eps^-1/2; row 1 has mean 1e3 and unit deviation and meets the
    same bounds as any row (the two-pass variance survives it)"""
    c = ct.ln_case(3, D, 0, edge=True)
    got, stat = _check_ln_fwd(f"D={D} edge rows", c, 3, D)
    assert torch.equal(got["y"][0, :D], c["beta"].to(torch.bfloat16))
    assert stat[0, 0, 0].item() == 1.5 and abs(stat[1, 0, 0].item() - 1000.0) < 1e-3


@pytest.mark.parametrize("n_slabs", ct.LN_BWD_SLABS)
@pytest.mark.parametrize("rows", ct.LN_ROWS)
@pytest.mark.parametrize("D", ct.LN_DIMS)
def test_ln_rows_bwd_against_fp64(D, rows, n_slabs):
    """a non-zero g on entry (the kernel accumulates into it); n_slabs = 12: the engine's fc1^T split; 17: the second LNR_SB trip"""
    c = ct.ln_bwd_case(rows, D, n_slabs)
    tag = f"D={D} rows={rows} n_slabs={n_slabs}"
    xs, dys, ss = D + 8, D + 16, 3
    stride = rows * dys + 8
    dy_h = torch.full((n_slabs, stride), NAN_BITS, dtype=torch.int32)
    for s in range(n_slabs):
        dy_h[s, :rows * dys].view(rows, dys)[:, :D] = _bits(c["slabs"][s])
    dy0 = dy_h.clone()
    dy = dy_h.view(torch.float32).to(DEV)
    x, _ = _padded_f32(rows, xs, D, c["x"])
    g, g0 = _padded_f32(rows + 1, xs, D, torch.cat([c["g0"], torch.zeros(1, D)]))
    g_bf = torch.full((rows + 1, xs), BF_FILL, dtype=torch.bfloat16, device=DEV)
    stat = torch.full((2, rows * ss), F_FILL, device=DEV)
    stat[0, ::ss], stat[1, ::ss] = c["mean"].to(DEV), c["rstd"].to(DEV)
    gamma = c["gamma"].to(DEV)
    rc = _lib.lib().splice_ln_rows_bwd(_lib.ptr(dy), dys, _lib.ptr(x), xs, _lib.ptr(gamma), _lib.ptr(stat[0]), _lib.ptr(stat[1]), ss, _lib.ptr(g),
                                       _lib.ptr(g_bf), rows, D, n_slabs, stride, _st())
    torch.cuda.synchronize()
    assert rc == 0
    dy_pred = ct.ln_dy_pred(c)
    expect = dy0.clone()
    expect[0, :rows * dys].view(rows, dys)[:, :D] = _bits(dy_pred)
    assert torch.equal(_bits(dy), expect), f"{tag}: slab 0 is not s_0 + s_1 + ... bit for bit, or something else of dy was written"
    g_ref, E_g = ct.ln_bwd_ref(c, dy_pred)
    gh, gbh = g.cpu(), g_bf.cpu()
    keep = torch.ones(rows + 1, xs, dtype=torch.bool)
    keep[:rows, :D] = False
    assert torch.equal(_bits(g)[keep], g0[keep]) and (gbh[keep] == BF_FILL).all(), f"{tag}: g / g_bf written outside their rows"
    assert torch.equal(gbh[:rows, :D], gh[:rows, :D].to(torch.bfloat16)), f"{tag}: g_bf is not bf16(g)"
    r = _ratio((gh[:rows, :D].double() - g_ref).abs(), E_g)
    print(f"CLS_TAIL ln_rows_bwd {tag}: g worst err/bound {r:.3f}, slab sum and g_bf bit-exact")
    assert r <= 1.0, (tag, r)


# ------------------------------------------------------------------------------------------------ finisher of the split-K row GEMMs
def _run_fin(c, mode, rows, N, pre_lo=0, want_pre=True, rows_arg=None, N_arg=None, mode_arg=None, **override):
    n = c["slabs"].shape[0]
    stride, rs, os_, ps = rows * N + 8, N + 16, N + 8, N + 8
    sl = _nan_filled(n, stride)
    sl[:, :rows * N] = c["slabs"].reshape(n, rows * N).to(DEV)
    bias = c["bias"].to(DEV)
    resid, _ = _padded_f32(rows, rs, N, c["resid"])
    out_f32, _ = _padded_f32(rows + 1, os_, N)
    out_bf = torch.full((rows + 1, N), BF_FILL, dtype=torch.bfloat16, device=DEV)
    pa = torch.full((rows + 1, ps), BF_FILL, dtype=torch.bfloat16, device=DEV)      # pre_bf (mode 1) or aux (mode 2)
    if mode == 2:
        pa[:rows, :N] = c["aux"].to(torch.bfloat16).to(DEV)
    a = dict(slabs=_lib.ptr(sl), n_slabs=n, bias=_lib.ptr(bias) if mode != 2 else None, resid=_lib.ptr(resid) if mode == 0 else None,
             out_f32=_lib.ptr(out_f32) if mode == 0 else None, out_bf=_lib.ptr(out_bf) if mode else None,
             pre_bf=_lib.ptr(pa) if mode == 1 and want_pre else None, aux=_lib.ptr(pa) if mode == 2 else None)
    a.update(override)
    rc = _lib.lib().splice_rows_finish(mode if mode_arg is None else mode_arg, a["slabs"], a["n_slabs"], stride, rows if rows_arg is None else rows_arg, N if N_arg is None else N_arg,
                                       a["bias"], a["resid"], rs, a["out_f32"], os_, a["out_bf"], a["pre_bf"], a["aux"], ps, pre_lo, _st())
    torch.cuda.synchronize()
    return rc, _bits(out_f32), out_bf.cpu(), pa.cpu()


@pytest.mark.parametrize("n_slabs", ct.FIN_SLABS)
@pytest.mark.parametrize("rows,N", ct.FIN_SHAPES)
def test_rows_finish_against_fp64(rows, N, n_slabs):
    """(3, 100): rows * N is no multiple of 256; n_slabs = 9: the second trip of eight.  Mode 0 and mode 1's pre-activation bit for bit, the GELU
    outputs inside common.h's own bars; aux spans [-6, 6] (both saturated branches of gelu_grad_f)."""
    c = ct.fin_case(rows, N, n_slabs)
    tag = f"rows={rows} N={N} n_slabs={n_slabs}"
    # mode 0
    rc, o32, obf, pa = _run_fin(c, 0, rows, N)
    assert rc == 0
    expect = torch.full((rows + 1, N + 8), NAN_BITS, dtype=torch.int32)
    expect[:rows, :N] = _bits(ct.fin_ref(c, 0))
    assert torch.equal(o32, expect), f"{tag}: mode 0 is not (bias + s_0 + ...) + resid bit for bit, or a gap was written"
    assert (obf == BF_FILL).all() and (pa == BF_FILL).all()
    # mode 1
    ref, bar, pre = ct.fin_ref(c, 1)
    worst = 0.0
    first = None
    for pre_lo, want_pre in ((0, True), (1, True), (rows, True), (0, False)):
        rc, o32, obf, pa = _run_fin(c, 1, rows, N, pre_lo=pre_lo, want_pre=want_pre)
        assert rc == 0
        assert (o32 == NAN_BITS).all() and (obf[rows] == BF_FILL).all()
        worst = max(worst, _ratio((obf[:rows].double() - ref).abs(), bar))
        first = obf if first is None else first
        assert torch.equal(_bits(obf), _bits(first)), f"{tag}: the GELU output depends on pre_lo / pre_bf"
        lo = pre_lo if want_pre else rows
        assert (pa[:lo] == BF_FILL).all() and (pa[:, N:] == BF_FILL).all() and (pa[rows] == BF_FILL).all(), f"{tag}: pre_bf written below pre_lo or outside"
        assert torch.equal(_bits(pa[lo:rows, :N]), _bits(pre[lo:].to(torch.bfloat16))), f"{tag}: pre_bf is not bf16(bias + s_0 + ...) bit for bit"
    # mode 2
    ref2, bar2 = ct.fin_ref(c, 2)
    rc, o32, obf, pa = _run_fin(c, 2, rows, N)
    assert rc == 0
    assert (o32 == NAN_BITS).all() and (obf[rows] == BF_FILL).all()
    r2 = _ratio((obf[:rows].double() - ref2).abs(), bar2)
    print(f"CLS_TAIL rows_finish {tag}: gelu worst err/bound {worst:.3f}, gelu' {r2:.3f}, mode 0 and pre_bf bit-exact")
    assert worst <= 1.0 and r2 <= 1.0, (tag, worst, r2)


# ------------------------------------------------------------------------------------------------ refusals
def test_attn_cls_refusals_launch_nothing():
    T, Tld, D, H, B = 17, 32, 128, 2, 2
    qkv = ct.attn_case(T, D, H, B, "flat")
    m, mT = _attn_buffers(qkv, Tld, 1e3)
    p32 = torch.zeros(B, H, Tld, device=DEV)
    sl = torch.zeros(16, B * D, device=DEV)
    L = _lib.lib()
    good = dict(qkv=_lib.ptr(m), qkvT=_lib.ptr(mT), ldt=B * Tld, B=B, T=T, Tld=Tld, D=D, H=H, n=6)
    bad = [dict(qkv=None), dict(qkvT=None), dict(out=None), dict(probs=None), dict(dout=None), dict(dqkv=None), dict(T=0), dict(T=Tld + 1),
           dict(Tld=40, T=17), dict(ldt=B * Tld + 4), dict(ldt=Tld), dict(D=96, H=1), dict(H=3), dict(n=0), dict(n=17),
           dict(Tld=32 * 400, ldt=B * 32 * 400)]   # the last: 76.8 KB of dynamic LDS
    for change in bad:
        a = dict(good)
        a.update({k: v for k, v in change.items() if k in good})
        out = torch.full((B, D), BF_FILL, dtype=torch.bfloat16, device=DEV)
        probs = _nan_filled(B, H, Tld)
        dqkv = torch.full((B * Tld, 3 * D), BF_FILL, dtype=torch.bfloat16, device=DEV)
        po = None if "out" in change else _lib.ptr(out)
        pp = None if "probs" in change else _lib.ptr(probs)
        if not {"dout", "dqkv", "n"} & set(change):
            assert L.splice_attn_cls_fwd(a["qkv"], a["qkvT"], a["ldt"], a["B"], a["T"], a["Tld"], a["D"], a["H"], ct.SCALE, po, pp, _st()) == ERR_ARG, change
        if "out" not in change:
            pin = None if "probs" in change else _lib.ptr(p32)
            assert L.splice_attn_cls_bwd(a["qkv"], a["qkvT"], a["ldt"], a["B"], a["T"], a["Tld"], a["D"], a["H"], ct.SCALE, pin,
                                         None if "dout" in change else _lib.ptr(sl), a["n"], B * D, None if "dqkv" in change else _lib.ptr(dqkv),
                                         _st()) == ERR_ARG, change
        torch.cuda.synchronize()
        assert (out == BF_FILL).all() and (_bits(probs) == NAN_BITS).all() and (dqkv == BF_FILL).all(), change


def test_ln_rows_and_rows_finish_refusals_launch_nothing():
    rows, D = 3, 100
    c0, c6 = ct.ln_case(rows, D, 0), ct.ln_case(rows, D, 6)
    for c, kw in ((c0, dict(D_arg=769)), (c0, dict(rows_arg=0)), (c6, dict(n_slabs=0)), (c6, dict(bias=None)), (c6, dict(resid=None))):
        rc, got, pre = _run_ln_fwd(c, rows, D, **kw)
        assert rc == ERR_ARG, kw
        assert _ln_fwd_untouched(got, pre, rows, D), kw
    for rr, dd in ((rows, 769), (0, D)):
        x = torch.zeros(rows, 769, device=DEV)
        g = _nan_filled(rows, 769)
        g_bf = torch.full((rows, 769), BF_FILL, dtype=torch.bfloat16, device=DEV)
        dy = _nan_filled(rows, 769)
        stat = torch.ones(2, rows, device=DEV)
        gamma = torch.ones(769, device=DEV)
        rc = _lib.lib().splice_ln_rows_bwd(_lib.ptr(dy), 769, _lib.ptr(x), 769, _lib.ptr(gamma), _lib.ptr(stat[0]), _lib.ptr(stat[1]), 1, _lib.ptr(g),
                                           _lib.ptr(g_bf), rr, dd, 1, rows * 769, _st())
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (rr, dd)
        assert (_bits(g) == NAN_BITS).all() and (g_bf == BF_FILL).all() and (_bits(dy) == NAN_BITS).all()
    rows, N = 3, 100
    c = ct.fin_case(rows, N, 8)
    cases = [(0, dict(mode_arg=3)), (0, dict(mode_arg=-1)), (0, dict(rows_arg=0)), (1, dict(N_arg=0)), (1, dict(n_slabs=0)), (0, dict(slabs=None)),
             (0, dict(out_f32=None)), (0, dict(resid=None)), (1, dict(out_bf=None)), (2, dict(out_bf=None)), (2, dict(aux=None))]
    for mode, kw in cases:
        rc, o32, obf, pa = _run_fin(c, mode, rows, N, **kw)
        assert rc == ERR_ARG, (mode, kw)
        assert (o32 == NAN_BITS).all() and (obf == BF_FILL).all(), (mode, kw)
        if mode != 2:
            assert (pa == BF_FILL).all(), (mode, kw)


# ------------------------------------------------------------------------------------------------ wiring through the ViT context
def _oracle_vit(name, img_size, seed, w_std):
    from oracle import dino_vit
    patch, dim, depth, heads = dino_vit.DINO_CONFIGS[name]
    m = dino_vit.VisionTransformer(patch, dim, depth, heads, img_size=img_size).eval()
    sd = synth.vit_params(seed, name, img_size=img_size, w_std=w_std)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    for p in m.parameters():
        p.requires_grad_(False)
    return m, sd


def _relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-30)).item()


def _cos(a, b):
    a, b = a.double().cpu().flatten(), b.double().cpu().flatten()
    return (a @ b / (a.norm() * b.norm() + 1e-30)).item()


@pytest.mark.parametrize("Himg,Wimg", [(40, 40), (32, 48)])
def test_cls_tail_through_the_vit_context(Himg, Wimg):
    """dino_vits8, B = 3, the context in [CLS]-only mode: the [CLS] rows of block depth-1 against the fp32 oracle (test_vits8_golden_features' bar
    for that tensor, 2e-2); d_img from d_block[depth-1] on the [CLS] rows plus d_keys[depth-1] (test_backward_injection's bars, 5e-2 and cosine
    > 0.998); forwards over the passes [0, 1) then [1, 3) give the bits of one forward over [0, 3) -- the [CLS] rows of block depth-1 and all of
    qkv; a backward over [1, 3) leaves pass 0 of d_img exactly zero and gives the bits of the [0, 3) backward on passes 1 and 2 (the pass_begin
    offsets of cls_slabs / cls_probs / cls_h)."""
    from oracle import dino_vit
    from oracle.losses import normalize as onorm
    from splice_amd.vit import KIND_BLOCK, KIND_QKV_STORED, VitContext, VitEngine
    name, B = "dino_vits8", 3
    model, sd = _oracle_vit(name, 40, seed=5, w_std=0.04)
    eng = VitEngine(name).load_state_dict(sd)
    D, L = eng.dim, eng.depth
    lib = _lib.lib()
    imgs = torch.from_numpy(synth.uniform(3, f"cls_tail/{Himg}x{Wimg}", (B, 3, Himg, Wimg)))
    imgs_d = imgs.to(DEV)
    ctx = VitContext(eng, B, Himg, Wimg, True)
    _lib.check(lib.splice_vit_ctx_set_top_cls_only(ctx.handle, 1))
    ctx.forward(imgs_d, normalize=True)
    T, Tld = ctx.T, ctx.Tld
    wb = torch.zeros(B, T, D)
    wb[:, 0] = torch.from_numpy(synth.normal(4, "cls_tail/wb", (B, D)))
    wk = torch.from_numpy(synth.normal(4, "cls_tail/wk", (B, T, D))) * 0.05
    gref, cls_ref = [], []
    for i in range(B):
        x = imgs[i:i + 1].clone().requires_grad_(True)
        f = dino_vit.forward_features(model, onorm(x[0])[None])
        ((f["block"][L - 1][0] * wb[i]).sum() + (f["qkv"][L - 1][0][:, D:2 * D] * wk[i]).sum()).backward()
        gref.append(x.grad[0])
        cls_ref.append(f["block"][L - 1][0, 0].detach())
    cls_full = ctx.read(KIND_BLOCK, L - 1)[:, 0].clone()
    qkv_full = ctx.read(KIND_QKV_STORED, L - 1).clone()
    e = _relerr(cls_full, torch.stack(cls_ref))
    print(f"CLS_TAIL ctx {Himg}x{Wimg}: [CLS] rows of block {L - 1} rel err {e:.2e}")
    assert e < 2e-2, e
    db = torch.zeros(B, Tld, D, device=DEV)
    db[:, :T] = wb.to(DEV)
    dk = torch.zeros(B, Tld, D, device=DEV)
    dk[:, :T] = wk.to(DEV)
    d_full = ctx.backward(0, B, {L - 1: db}, None, {L - 1: dk}, normalize=True)
    torch.cuda.synchronize()
    for i in range(B):
        e, c = _relerr(d_full[i], gref[i]), _cos(d_full[i], gref[i])
        print(f"CLS_TAIL ctx {Himg}x{Wimg}: d_img pass {i} rel err {e:.2e}, cosine {c:.5f}")
        assert e < 5e-2 and c > 0.998, (i, e, c)
    # pass ranges: forward [0, 1) then [1, 3) on a second context, backward [1, 3)
    ctx2 = VitContext(eng, B, Himg, Wimg, True)
    _lib.check(lib.splice_vit_ctx_set_top_cls_only(ctx2.handle, 1))
    for lo, hi in ((0, 1), (1, 3)):
        _lib.check(lib.splice_vit_forward_passes(ctx2.handle, _lib.ptr(imgs_d), 1, 0, lo, hi, _st()), "vit_forward_passes")
    torch.cuda.synchronize()
    assert torch.equal(ctx2.read(KIND_BLOCK, L - 1)[:, 0], cls_full), "the [CLS] rows of the top block depend on the pass range of the forward"
    assert torch.equal(_bits(ctx2.read(KIND_QKV_STORED, L - 1)), _bits(qkv_full)), "qkv of the top block depends on the pass range of the forward"
    d_part = ctx2.backward(1, 3, {L - 1: db}, None, {L - 1: dk}, normalize=True)
    torch.cuda.synchronize()
    assert d_part[0].abs().max().item() == 0.0, "a backward over passes [1, 3) wrote pass 0 of d_img"
    assert torch.equal(_bits(d_part[1:]), _bits(d_full[1:])), "d_img of passes 1-2 depends on the pass range of the backward"
