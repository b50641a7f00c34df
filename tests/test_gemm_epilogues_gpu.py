"""Element-wise parity of every epilogue form of the bf16 NT GEMM (splice_gemm_nt_bf16: the 13 CASE(...) entries of
gemm_nt_launch) against an fp64 reference on the bf16-rounded operands, with padded leading dimensions, offset operand
bases, every forced tile / ring, and sentinels behind every output.

Reference and bounds (derived, not tuned):
  P = A @ B^T and S = |A| @ |B|^T in fp64; ref = P with the epilogue applied in fp64 (alpha, bias, residual with resid_mod,
  exact-erf GELU / gelu').
  acc = (K + 4) * 2^-23 * (|alpha| * S + |bias| + |resid|)   -- a K-term fp32 sum of exact bf16 products in any order, unit
        roundoff taken as 2^-23 so the bar holds whether the matrix core rounds or truncates internally
  fp32 outputs:  |got - ref| <= acc
  bf16 outputs:  |got - ref| <= 2^-8 |ref| + 2 acc           -- one round-to-nearest of a value within acc of ref
  GELU output:   acc * 1.13 (Lipschitz constant of GELU) and + 1.3e-4 absolute (common.h's bound for gelu_f, tails included)
  GELU_GRAD:     ref = P * gelu'(aux) exact; + 6e-4 |P| (5e-5 of the fit inside [-4, 4]; saturation to 0 / 0.99997 outside,
                 where the true values are -5.0e-4 / 1.0005)
  transposed copy: bit-equal to out_bf;  column window: the fp32 bar.
  ROWDOT: (a) against sum_c out_bf[r, c] * rd_other[r, c] of the call's own out_bf: 64 * 2^-24 * sum |term| (64 exact
  products, 63 fp32 additions) -- the "bf16-ROUNDED result" contract; (b) against sum_c P * rd_other: 2^-8 sum |P other| +
  sum 2 acc |other| + the summation term of (a).

Output path reached (gemm_nt_kernel picks by alignment facts alone).  SB = staged bf16 tile (16-byte row stores; "SB/t" = its
8-element scalar tail because ld % 8 != 0 or the chunk is ragged), SF = staged fp32 tile, PRE = per-fragment with pre-loaded
operands, FRAG = scalar per-fragment fallback, 8P = the 8-phase 256 x 256 tile (tile code 5, (300, 256, 128) only).
Every N class runs in both pitch regimes under tile codes 0, 1, 11, 2, 12, 22, 3, 13, 23 (ROWDOT: by shape, 2 / 3 / 4 stages).

  flag set                          | aligned pitches, N%8==0 / N%8==4 | odd pitches, N%4==0 | N%4!=0 (both regimes)
  ----------------------------------+----------------------------------+---------------------+----------------------
  BIAS|OUT_BF|OUT_T                 | SB / SB + SB/t                   | PRE (ldt%8==4)      | FRAG
  BIAS|OUT_BF|OUT_T|COLS_F32        | SB / SB + SB/t                   | PRE                 | FRAG
  BIAS|OUT_F32                      | SF (PRE on 128x128x2)            | PRE (ldo%4!=0)      | FRAG
  BIAS|OUT_BF                       | SB / SB + SB/t, 8P               | SB/t                | FRAG
  BIAS|RESID|OUT_F32 (mod 0 and 48) | SF (PRE on 128x128x2), 8P        | FRAG (ldr%4!=0)     | FRAG
  BIAS|GELU|OUT_BF (+ out_pre)      | SB / SB + SB/t, 8P               | SB/t                | FRAG
  OUT_F32                           | SF (FRAG on 128x128x2)           | FRAG                | FRAG
  OUT_F32|ALPHA                     | SF (FRAG on 128x128x2)           | FRAG                | FRAG
  OUT_BF                            | SB / SB + SB/t                   | SB/t                | FRAG
  OUT_BF|OUT_T                      | SB / SB + SB/t                   | FRAG                | FRAG
  OUT_BF|OUT_T|ROWDOT               | SB                               | FRAG                | (refused: N % 64)
  OUT_BF|ROWDOT                     | SB                               | SB/t                | (refused: N % 64)
  GELU_GRAD|OUT_BF                  | SB / SB + SB/t                   | FRAG (ldaux%4!=0)   | FRAG

Measured worst err / bound on MI355X over everything above (printed by the tests, one line per epilogue; bar = 1.0):
  bf16 outputs: bias_bf_t 0.987, bias_bf_t_cols 0.987, bias_bf 0.987, bias_gelu_bf 0.944 (out_pre 0.987), bf 0.973, bf_t 0.973,
                gelugrad_bf 0.864, the two ROWDOT sets 0.961   (a bf16 rounding reaches its half-ulp bar at the foot of a binade)
  fp32 outputs: bias_f32 0.008, bias_resid_f32 0.010, f32 0.008, f32_alpha 0.011, column window 0.008
  ROWDOT:       0.012 against the call's own out_bf, 0.315 against the fp64 product
  split-K:      slab 0.005, in-order sum 0.001, virtual 0.001
No sentinel was touched and no kernel change was needed.
"""
import ctypes as C
import functools
import math

import pytest
import torch

from splice_amd import _lib
from test_ops_gpu import DEV, _bf, _gemm, _rand, _st

pytestmark = pytest.mark.gpu

E = _lib
U23, U24, U8 = 2.0 ** -23, 2.0 ** -24, 2.0 ** -8
SENT_BF, SENT_F32 = -7.0, -12345.0
ALPHA = -0.37
FORCES = (0, 1, 11, 2, 12, 22, 3, 13, 23)
SHAPES = ((70, 64, 64), (130, 200, 192), (333, 196, 128), (129, 198, 64), (65, 67, 64))
ROWDOT_SHAPES = ((70, 64, 64), (130, 128, 192), (333, 128, 128), (129, 64, 64), (65, 128, 64),
                 (200, 128, 128), (200, 128, 768), (200, 128, 1536))   # the last three: 2-stage, 3-stage ring, 4-stage ring
TABLE = {
    "bias_bf_t": E.EPI_BIAS | E.EPI_OUT_BF | E.EPI_OUT_T,
    "bias_bf_t_cols": E.EPI_BIAS | E.EPI_OUT_BF | E.EPI_OUT_T | E.EPI_COLS_F32,
    "bias_f32": E.EPI_BIAS | E.EPI_OUT_F32,
    "bias_bf": E.EPI_BIAS | E.EPI_OUT_BF,
    "bias_resid_f32": E.EPI_BIAS | E.EPI_RESID | E.EPI_OUT_F32,
    "bias_gelu_bf": E.EPI_BIAS | E.EPI_GELU | E.EPI_OUT_BF,
    "f32": E.EPI_OUT_F32,
    "f32_alpha": E.EPI_OUT_F32 | E.EPI_ALPHA,
    "bf": E.EPI_OUT_BF,
    "bf_t": E.EPI_OUT_BF | E.EPI_OUT_T,
    "bf_t_rowdot": E.EPI_OUT_BF | E.EPI_OUT_T | E.EPI_ROWDOT,
    "bf_rowdot": E.EPI_OUT_BF | E.EPI_ROWDOT,
    "gelugrad_bf": E.EPI_GELU_GRAD | E.EPI_OUT_BF,
}
WORST = {}


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), ratio)


def _worst(got, ref, bound):
    """max over the elements of |got - ref| / bound; a NaN anywhere counts as infinite"""
    r = (got.double() - ref).abs() / bound
    return torch.nan_to_num(r, nan=float("inf")).max().item()


class Buf:
    """An output of `rows` x `ld` elements with 3 guard rows behind it and 32 guard elements on either side, all pre-filled with a
    sentinel (-7 for bf16, -12345 for fp32)."""

    def __init__(self, rows, ld, dtype, guard_rows=3):
        self.sent = SENT_BF if dtype == torch.bfloat16 else SENT_F32
        self.rows, self.ld = rows + guard_rows, ld
        self.flat = torch.full((64 + self.rows * ld,), self.sent, device=DEV, dtype=dtype)
        self.t = self.flat[32:32 + self.rows * ld].view(self.rows, ld)

    def untouched_outside(self, r0, r1, c0, c1):
        f = self.flat.clone()
        f[32:32 + self.rows * self.ld].view(self.rows, self.ld)[r0:r1, c0:c1] = self.sent
        return bool((f == self.sent).all())


def _strided(x, ld, base=8, tail_rows=0):
    """x [R][W] as a view with row pitch ld, `base` elements into a larger buffer whose every other element is NaN"""
    R, W = x.shape
    buf = torch.full((base + (R + tail_rows) * ld + 8,), float("nan"), device=DEV, dtype=x.dtype)
    v = buf[base:base + R * ld].view(R, ld)[:, :W]
    v.copy_(x)
    return v


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """bf16 operands (asymmetric: std 1.0 and 0.05, so a row/column swap cannot pass) and the fp64 P, S; computed once, never modified"""
    A, B = _bf(_rand(M, K, seed=101)), _bf(_rand(N, K, seed=102, std=0.05))
    Ad, Bd = A.double(), B.double()
    return A, B, Ad @ Bd.T, Ad.abs() @ Bd.abs().T


@functools.lru_cache(maxsize=None)
def _epi_operands(M, N):
    return dict(bias=_rand(N, seed=103), resid=_rand(M, N, seed=104), aux=_bf(_rand(M, N, seed=105, std=2.0)),   # aux: ~4.5 % beyond +-4
                other=_bf(_rand(M, N, seed=106)))


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


@functools.lru_cache(maxsize=None)
def _reference(flags, M, N, K, resid_mod):
    """(x, acc, out_ref, out_bound): the value before the activation with its fp32 bar, and the bf16 output with its bar"""
    _, _, P, S = _problem(M, N, K)
    op = _epi_operands(M, N)
    alpha = ALPHA if flags & E.EPI_ALPHA else 1.0
    x, mag = P * alpha, S * abs(alpha)
    if flags & E.EPI_BIAS:
        x, mag = x + op["bias"].double(), mag + op["bias"].double().abs()
    if flags & E.EPI_RESID:
        rows = torch.arange(M, device=DEV) % resid_mod if resid_mod else torch.arange(M, device=DEV)
        r = op["resid"].double()[rows]
        x, mag = x + r, mag + r.abs()
    acc = (K + 4) * U23 * mag
    if flags & E.EPI_GELU:
        ref = _gelu64(x)
        return x, acc, ref, U8 * ref.abs() + 2 * 1.13 * acc + 1.3e-4
    if flags & E.EPI_GELU_GRAD:
        ref = P * _gelu_grad64(op["aux"].double())
        return x, acc, ref, U8 * ref.abs() + 2 * acc + 6e-4 * P.abs()
    return x, acc, x, U8 * x.abs() + 2 * acc


def _pitches(M, N, W, regime):
    if regime == "aligned":      # the logical width rounded up to a multiple of 8, plus 8
        f = lambda v: (v + 7) // 8 * 8 + 8
        return dict(ldo=f(N), ldr=f(N), ldaux=f(N), ldbf=f(N), ldt=f(M), ldp=f(N), ld_cols=f(W), ld_rd=f(N))
    ldt = (M + 3) // 4 * 4       # odd: the smallest legal pitches that fail the vector conditions
    if ldt % 8 != 4:
        ldt += 4
    return dict(ldo=N + 1, ldr=N + 3, ldaux=N + 2, ldbf=N + 4 if N % 8 == 0 else N + 1, ldt=ldt, ldp=N + 5,
                ld_cols=W + 1 if W % 2 == 0 else W + 2, ld_rd=N + 4)


def _rowdot_index(M, N, rd_rows):
    r = torch.arange(M, device=DEV)[:, None]
    b = torch.arange(N // 64, device=DEV)[None, :]
    return (r // rd_rows) * (N // 64) * rd_rows + b * rd_rows + r % rd_rows   # the map of include/splice_hip.h


def _check_rowdot(name, where, rd, got_bf, other, P, acc, M, N, rd_rows):
    nb, total = N // 64, -(-M // rd_rows) * (N // 64) * rd_rows
    idx = _rowdot_index(M, N, rd_rows)
    body = rd.flat[32:32 + total]
    got = body[idx]
    o = other.double()
    t1 = (got_bf.double() * o).view(M, nb, 64)
    sum_bound = 64 * U24 * t1.abs().sum(-1)
    w1 = _worst(got, t1.sum(-1), sum_bound)
    _note(name + " rowdot vs own out_bf", w1)
    assert w1 <= 1.0, (where, "rowdot against the call's own bf16 output", w1)
    t2 = (P * o).view(M, nb, 64)
    b2 = U8 * t2.abs().sum(-1) + (2 * acc * o.abs()).view(M, nb, 64).sum(-1) + 64 * U24 * (1 + U8) * t2.abs().sum(-1)
    w2 = _worst(got, t2.sum(-1), b2)
    _note(name + " rowdot vs P", w2)
    assert w2 <= 1.0, (where, "rowdot against the fp64 product", w2)
    f = rd.flat.clone()
    f[32 + idx.flatten()] = rd.sent
    assert bool((f == rd.sent).all()), (where, "rowdot entries of rows >= M (or outside the buffer) were written")


def _run_case(name, flags, M, N, K, regime, resid_mod=0, rd_rows=96):
    A, B, P, _ = _problem(M, N, K)
    op = _epi_operands(M, N)
    x, acc, out_ref, out_bound = _reference(flags, M, N, K, resid_mod)
    col_lo, col_hi = 6, min(71, N - 2)          # a window that neither starts nor ends on a multiple of 4 or 64
    W = col_hi - col_lo
    ld = _pitches(M, N, W, regime)
    where = (name, M, N, K, regime, resid_mod)
    kw, bufs = {}, {}
    if flags & E.EPI_BIAS:
        kw["bias"] = _strided(op["bias"][None], N + 4, base=4)[0]
    if flags & E.EPI_RESID:
        kw.update(resid=_strided(op["resid"][:resid_mod or M], ld["ldr"]), ldr=ld["ldr"], resid_mod=resid_mod)
    if flags & E.EPI_GELU_GRAD:
        kw.update(aux=_strided(op["aux"], ld["ldaux"]), ldaux=ld["ldaux"])
    if flags & E.EPI_ALPHA:
        kw["alpha"] = ALPHA
    if flags & E.EPI_OUT_F32:
        bufs["f32"] = Buf(M, ld["ldo"], torch.float32)
        kw.update(out_f32=bufs["f32"].t, ldo=ld["ldo"])
    if flags & E.EPI_OUT_BF:
        bufs["bf"] = Buf(M, ld["ldbf"], torch.bfloat16)
        kw.update(out_bf=bufs["bf"].t, ldbf=ld["ldbf"])
    if flags & E.EPI_OUT_T:
        bufs["t"] = Buf(N, ld["ldt"], torch.bfloat16)
        kw.update(out_bf_t=bufs["t"].t, ldt=ld["ldt"])
    pre_lo = M // 3 if regime == "odd" else 5
    if flags & E.EPI_GELU:
        bufs["pre"] = Buf(M, ld["ldp"], torch.bfloat16)
        kw.update(out_pre=bufs["pre"].t, ldp=ld["ldp"], pre_row_lo=pre_lo)
    if flags & E.EPI_COLS_F32:
        bufs["cols"] = Buf(M, ld["ld_cols"], torch.float32)
        kw.update(out_f32_cols=bufs["cols"].t, ld_cols=ld["ld_cols"], col_lo=col_lo, col_hi=col_hi)
    if flags & E.EPI_ROWDOT:
        total = -(-M // rd_rows) * (N // 64) * rd_rows
        bufs["rd"] = Buf(1, total, torch.float32, guard_rows=0)
        # rows up to the end of the last 64-row tile exist behind the matrix (NaN): a load that is not clamped to row M - 1 shows
        kw.update(rd_other=_strided(op["other"], ld["ld_rd"], tail_rows=128), ld_rd=ld["ld_rd"], rd_rows=rd_rows, rowdot=bufs["rd"].flat[32:])
    _gemm(flags, _strided(A, K + 8), _strided(B, K + 16), M, N, K, **kw)

    if "f32" in bufs:
        w = _worst(bufs["f32"].t[:M, :N], x, acc)
        _note(name, w)
        assert w <= 1.0, (where, "out_f32", w)
        assert bufs["f32"].untouched_outside(0, M, 0, N), (where, "out_f32: written outside [M][N]")
    if "bf" in bufs:
        w = _worst(bufs["bf"].t[:M, :N], out_ref, out_bound)
        _note(name, w)
        assert w <= 1.0, (where, "out_bf", w)
        assert bufs["bf"].untouched_outside(0, M, 0, N), (where, "out_bf: written outside [M][N]")
    if "t" in bufs:
        assert torch.equal(bufs["t"].t[:N, :M].T, bufs["bf"].t[:M, :N]), (where, "out_bf_t is not the transpose of out_bf")
        assert bufs["t"].untouched_outside(0, N, 0, M), (where, "out_bf_t: written outside [N][M]")
    if "pre" in bufs:
        w = _worst(bufs["pre"].t[pre_lo:M, :N], x[pre_lo:], U8 * x[pre_lo:].abs() + 2 * acc[pre_lo:])
        _note(name + " out_pre", w)
        assert w <= 1.0, (where, "out_pre", w)
        assert bufs["pre"].untouched_outside(pre_lo, M, 0, N), (where, "out_pre: written outside rows [pre_row_lo, M) x [0, N)")
    if "cols" in bufs:
        w = _worst(bufs["cols"].t[:M, :W], x[:, col_lo:col_hi], acc[:, col_lo:col_hi])
        _note(name + " cols", w)
        assert w <= 1.0, (where, "out_f32_cols", w)
        assert bufs["cols"].untouched_outside(0, M, 0, W), (where, "out_f32_cols: written outside the window")
    if "rd" in bufs:
        _check_rowdot(name, where, bufs["rd"], bufs["bf"].t[:M, :N], op["other"], P, acc, M, N, rd_rows)


def _report(prefix):
    for k in sorted(WORST):
        if k == prefix or k.startswith(prefix + " "):
            print(f"[gemm-epilogue-parity] {k}: worst err / bound = {WORST[k]:.3f}")


@pytest.mark.parametrize("name", [n for n in TABLE if "rowdot" not in n])
def test_gemm_epilogue_table(name):
    """Every non-ROWDOT entry of gemm_nt_launch x 5 alignment-class shapes x aligned / odd pitches x 9 forced tiles (x resid_mod 0 / 48),
    each output element against the fp64 reference under the derived bars of the module docstring, every byte around the outputs a
    sentinel.  Tile code 5 (8-phase) on (300, 256, 128) for the three epilogues it admits.
    Worst err / bound measured on MI355X: 0.987 on the bf16 outputs, 0.011 on the fp32 ones (per epilogue: module docstring)."""
    flags = TABLE[name]
    L = _lib.lib()
    mods = (0, 48) if flags & E.EPI_RESID else (0,)
    try:
        for force in FORCES:
            L.splice_gemm_force_tile(force)
            for M, N, K in SHAPES:
                for regime in ("aligned", "odd"):
                    for mod in mods:
                        try:
                            _run_case(name, flags, M, N, K, regime, mod)
                        except AssertionError as err:
                            raise AssertionError(f"tile code {force}: {err}") from None
        if flags in (E.EPI_BIAS | E.EPI_OUT_BF, E.EPI_BIAS | E.EPI_GELU | E.EPI_OUT_BF, E.EPI_BIAS | E.EPI_RESID | E.EPI_OUT_F32):
            L.splice_gemm_force_tile(5)
            for regime in ("aligned", "odd"):     # odd pitches: gemm8p_operands_ok refuses, the automatic choice runs
                for mod in mods:
                    _run_case(name, flags, 300, 256, 128, regime, mod)
    finally:
        L.splice_gemm_force_tile(0)
        _report(name)


@pytest.mark.parametrize("name", ["bf_t_rowdot", "bf_rowdot"])
def test_gemm_epilogue_table_rowdot(name):
    """The two ROWDOT entries: N in {64, 128}, both pitch regimes; forcing is ignored, so the three instantiations are reached by shape
    ((200, 128, 128): 2 stages, (200, 128, 768): 3-stage ring, (200, 128, 1536): 4-stage ring).  out_bf / out_bf_t as in the table test,
    the row dots as in test_gemm_rowdot."""
    for M, N, K in ROWDOT_SHAPES:
        for regime in ("aligned", "odd"):
            _run_case(name, TABLE[name], M, N, K, regime)
    _report(name)


@pytest.mark.parametrize("name", ["bf_t_rowdot", "bf_rowdot"])
@pytest.mark.parametrize("M,rd_rows", [(288, 96), (192, 64), (250, 96)])
@pytest.mark.parametrize("N", [64, 128])
def test_gemm_rowdot(name, M, rd_rows, N):
    """delta = rowsum(dO * O) where dO is produced: M = passes * rd_rows (the engine's case) and M = 250 with a partial last pass, ld_rd = N + 8,
    rd_other offset into a larger buffer.  Index map of include/splice_hip.h; value against the call's own bf16 output (64 * 2^-24 * sum |term|:
    the "bf16-ROUNDED result" contract) and against the fp64 product; entries of rows >= M keep the sentinel."""
    _run_case(name, TABLE[name], M, N, 128, "aligned", rd_rows=rd_rows)
    _report(name)


def _gemm_rc(flags, A, lda, B, ldb, M, N, K, e):
    rc = _lib.lib().splice_gemm_nt_bf16(flags, _lib.ptr(A), lda, _lib.ptr(B), ldb, M, N, K, C.byref(e), _st())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("ks", [2, 3])
@pytest.mark.parametrize("ldo,gap", [(72, 8), (69, 1)])
def test_gemm_splitk_real_few_rows(ks, ldo, gap):
    """Real split-K: slab s holds the product over its own K slice (fp32 bar against that slice of P), the in-order slab sum meets the bar
    against P, the gaps between the slabs (slab_stride > M * ldo) keep the sentinel."""
    M, N, K = 70, 68, 384
    A, B, P, S = _problem(M, N, K)
    assert _lib.lib().splice_gemm_splitk_slabs(M, ks) == ks
    stride = (M + 3) * ldo + gap
    out = Buf(ks, stride, torch.float32, guard_rows=1)
    e = _lib.GemmEpilogue(); e.out_f32 = out.t.data_ptr(); e.ldo = ldo; e.ksplit = ks; e.slab_stride = stride
    _lib.check(_gemm_rc(E.EPI_OUT_F32, _strided(A, K + 8), K + 8, _strided(B, K + 16), K + 16, M, N, K, e))
    Kp = K // ks
    total = None
    chk = out.flat.clone()
    for s in range(ks):
        slab = out.t[s, :M * ldo].view(M, ldo)[:, :N]
        As, Bs = A[:, s * Kp:(s + 1) * Kp].double(), B[:, s * Kp:(s + 1) * Kp].double()
        w = _worst(slab, As @ Bs.T, (Kp + 4) * U23 * (As.abs() @ Bs.abs().T))
        _note("splitk slab", w)
        assert w <= 1.0, (ks, ldo, s, w)
        total = slab.clone() if total is None else total + slab
        chk[32:].view(-1)[s * stride:s * stride + M * ldo].view(M, ldo)[:, :N] = SENT_F32
    w = _worst(total, P, (K + 4) * U23 * S)
    _note("splitk sum", w)
    assert w <= 1.0, (ks, ldo, w)
    assert bool((chk == SENT_F32).all()), "written between or behind the slabs"
    _report("splitk slab")
    _report("splitk sum")


@pytest.mark.parametrize("ks", [2, 3])
def test_gemm_splitk_virtual(ks):
    """From 2401 rows on one workgroup walks the whole K: one slab, memory behind it untouched, fp32 bar against P; rows [0, 70) equal, bit for
    bit, the in-order slab sum of the same rows from a 70-row (real split-K) call."""
    M, N, K = 2401, 64, 384
    L = _lib.lib()
    A, B, P, S = _problem(M, N, K)
    assert L.splice_gemm_splitk_slabs(M, ks) == 1 and L.splice_gemm_splitk_slabs(70, ks) == ks
    ldo = N + 8
    stride = (M + 3) * ldo
    out = Buf(ks, stride, torch.float32, guard_rows=0)
    e = _lib.GemmEpilogue(); e.out_f32 = out.t.data_ptr(); e.ldo = ldo; e.ksplit = ks; e.slab_stride = stride
    _lib.check(_gemm_rc(E.EPI_OUT_F32, _strided(A, K + 8), K + 8, _strided(B, K + 16), K + 16, M, N, K, e))
    big = out.t[0, :M * ldo].view(M, ldo)[:, :N]
    w = _worst(big, P, (K + 4) * U23 * S)
    _note("splitk virtual", w)
    assert w <= 1.0, (ks, w)
    chk = out.flat.clone()
    chk[32:32 + M * ldo].view(M, ldo)[:, :N] = SENT_F32
    assert bool((chk == SENT_F32).all()), "written outside slab 0"
    small = torch.full((ks, 70, N), SENT_F32, device=DEV)
    e2 = _lib.GemmEpilogue(); e2.out_f32 = small.data_ptr(); e2.ldo = N; e2.ksplit = ks; e2.slab_stride = 70 * N
    _lib.check(_gemm_rc(E.EPI_OUT_F32, _strided(A[:70], K + 8), K + 8, _strided(B, K + 16), K + 16, 70, N, K, e2))
    ref = small[0] + small[1] if ks == 2 else (small[0] + small[1]) + small[2]
    assert torch.equal(big[:70], ref), (ks, (big[:70] - ref).abs().max().item())
    _report("splitk virtual")


def test_gemm_splitk_indivisible_k_runs_unsplit():
    """K % (ksplit * 64) != 0 (K = 320, ksplit = 3): the launcher runs unsplit while splice_gemm_splitk_slabs(M, 3) still answers 3 -- slab 0
    holds the whole product, slabs 1 and 2 are untouched (pinned as it is; the engine's ks rules never reach this case)."""
    M, N, K, ks = 70, 68, 320, 3
    A, B, P, S = _problem(M, N, K)
    assert _lib.lib().splice_gemm_splitk_slabs(M, ks) == 3
    ldo = 72
    stride = (M + 3) * ldo
    out = Buf(ks, stride, torch.float32, guard_rows=0)
    e = _lib.GemmEpilogue(); e.out_f32 = out.t.data_ptr(); e.ldo = ldo; e.ksplit = ks; e.slab_stride = stride
    _lib.check(_gemm_rc(E.EPI_OUT_F32, _strided(A, K + 8), K + 8, _strided(B, K + 16), K + 16, M, N, K, e))
    w = _worst(out.t[0, :M * ldo].view(M, ldo)[:, :N], P, (K + 4) * U23 * S)
    assert w <= 1.0, w
    chk = out.flat.clone()
    chk[32:32 + M * ldo].view(M, ldo)[:, :N] = SENT_F32
    assert bool((chk == SENT_F32).all()), "slabs 1 / 2 (or the padding of slab 0) were written"


@pytest.mark.parametrize("case", ["K=96", "K=32", "lda=K+4", "ldt%4", "rowdot N=96", "rowdot rd_other=NULL", "rowdot rd_rows=0", "flags not in the table"])
def test_gemm_refusals(case):
    """Argument contract: each of these returns non-zero and leaves every output buffer at its sentinel."""
    M, N, K, lda = 70, 64, 128, 136
    flags = E.EPI_BIAS | E.EPI_OUT_BF | E.EPI_OUT_T
    ldt, rd_rows, with_other = 72, 96, True
    if case == "K=96":
        K = 96
    elif case == "K=32":
        K = 32
    elif case == "lda=K+4":
        lda = K + 4
    elif case == "ldt%4":
        ldt = 74
    elif case.startswith("rowdot"):
        flags = E.EPI_OUT_BF | E.EPI_ROWDOT
        N = 96 if case == "rowdot N=96" else 64
        with_other = case != "rowdot rd_other=NULL"
        rd_rows = 0 if case == "rowdot rd_rows=0" else 96
    else:
        flags = E.EPI_OUT_F32 | E.EPI_OUT_BF
    A = torch.zeros(M, 144, device=DEV, dtype=torch.bfloat16)
    B = torch.zeros(N, 144, device=DEV, dtype=torch.bfloat16)
    bias = torch.zeros(N, device=DEV)
    other = torch.zeros(M, N + 8, device=DEV, dtype=torch.bfloat16)
    outs = dict(f32=Buf(M, N + 8, torch.float32), bf=Buf(M, N + 8, torch.bfloat16), t=Buf(N, 80, torch.bfloat16), rd=Buf(1, 2 * 96 * 2, torch.float32))
    e = _lib.GemmEpilogue()
    e.bias = bias.data_ptr()
    e.out_f32, e.ldo = outs["f32"].t.data_ptr(), N + 8
    e.out_bf, e.ldbf = outs["bf"].t.data_ptr(), N + 8
    e.out_bf_t, e.ldt = outs["t"].t.data_ptr(), ldt
    e.rd_other, e.ld_rd, e.rd_rows, e.rowdot = (other.data_ptr() if with_other else None), N + 8, rd_rows, outs["rd"].t.data_ptr()
    rc = _gemm_rc(flags, A, lda, B, 144, M, N, K, e)
    assert rc != 0, case
    for k, b in outs.items():
        assert b.untouched_outside(0, 0, 0, 0), (case, k)
