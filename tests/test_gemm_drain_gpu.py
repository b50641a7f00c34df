"""The ring forms of the bf16 NT GEMM fetch their epilogue operands (bias, residual, GELU' input, row-dot operand) at the head of
the ring's drain, and every wait of the drain is counted by hand (gemm.h, GemmTile::run_ring).  A count that is too permissive reads
a K slice that has not landed; a wrong operand register shows in the epilogue.  Both change bits, so every ring tile the hook can
force is compared BIT FOR BIT with the same call on the 2-stage form of the same tile (run_glds, which has no hand-counted wait),
and the 2-stage result element-wise with an fp64 reference under the bars of tests/test_gemm_epilogues_gpu.py (read there, not re-derived).

Shapes: M in {17, 70, 130} (a lone partial tile; partial last tiles of the 64- and 128-row forms: clamped operand rows), N in {64, 192}
(N = 64: the N - 4 column clamp is active in the last lane group of the 128-column tile), K in {64 ... 320} (1 ... 5 slices: fewer than
the ring has stages, exactly as many, and the first lengths with a steady state, for the 3- and the 4-stage ring).

A slice read too early would find what the LDS stage held before.  Every slice of A and B holds its own random values, and before each
ring call the same launch form runs once on operands rolled by one slice along K (and negated), so that the stage of slice s holds
slice s - 1's negated values, never slice s's own, when the measured call starts.
"""
import functools

import pytest
import torch

from splice_amd import _lib
from test_gemm_epilogues_gpu import U8, U23, Buf, _check_rowdot, _gelu64, _gelu_grad64, _strided, _worst
from test_ops_gpu import DEV, _bf, _gemm, _rand

pytestmark = pytest.mark.gpu

E = _lib
MS, NS_, KS = (17, 70, 130), (64, 192), (64, 128, 192, 256, 320)
RINGS = {1: (11,), 2: (12, 22), 3: (13, 23)}   # 2-stage tile code -> the ring codes of the same tile (4 stages; 3 stages)
FORMS = {
    # name: (flags, resid_mod, pitches that satisfy the vector conditions)
    "bias_resid_f32": (E.EPI_BIAS | E.EPI_RESID | E.EPI_OUT_F32, 0, True),
    "bias_resid_f32_mod48": (E.EPI_BIAS | E.EPI_RESID | E.EPI_OUT_F32, 48, True),
    "bias_resid_f32_oddpitch": (E.EPI_BIAS | E.EPI_RESID | E.EPI_OUT_F32, 0, False),   # the ring waits without operand loads
    "gelugrad_bf": (E.EPI_GELU_GRAD | E.EPI_OUT_BF, 0, True),
    "gelugrad_bf_oddpitch": (E.EPI_GELU_GRAD | E.EPI_OUT_BF, 0, False),
    "bf_rowdot": (E.EPI_OUT_BF | E.EPI_ROWDOT, 0, True),
    "bias_gelu_bf_pre": (E.EPI_BIAS | E.EPI_GELU | E.EPI_OUT_BF, 0, True),
}
RD_ROWS, PRE_LO = 48, 5


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """operands (computed once, never modified), the rolled and negated pair for the scrub launch, and the fp64 P, S"""
    A, B = _bf(_rand(M, K, seed=201)), _bf(_rand(N, K, seed=202, std=0.05))
    Ad, Bd = A.double(), B.double()
    return A, B, -torch.roll(A, 64, 1), -torch.roll(B, 64, 1), Ad @ Bd.T, Ad.abs() @ Bd.abs().T


@functools.lru_cache(maxsize=None)
def _operands(M, N):
    # bias in [0.5, ...): the GELU output stays away from its saturated tail; aux inside [-3, 3]: gelu' is not saturated to 0
    return dict(bias=_rand(N, seed=203).abs() + 0.5, resid=_rand(M, N, seed=204), aux=_bf(_rand(M, N, seed=205).clamp(-3, 3)),
                other=_bf(_rand(M, N, seed=206)))


def _launch(flags, mod, aligned, M, N, K, A, B):
    """one call into fresh sentinel-filled outputs; returns the Bufs"""
    op = _operands(M, N)
    f = (lambda v: (v + 7) // 8 * 8 + 8) if aligned else None
    ld = dict(ldo=f(N), ldr=f(N), ldaux=f(N), ldbf=f(N), ldp=f(N), ld_rd=f(N)) if aligned else \
        dict(ldo=N + 1, ldr=N + 3, ldaux=N + 2, ldbf=N + 4, ldp=N + 5, ld_rd=N + 4)
    kw, bufs = {}, {}
    if flags & E.EPI_BIAS:
        kw["bias"] = _strided(op["bias"][None], N + 4, base=4)[0]
    if flags & E.EPI_RESID:
        kw.update(resid=_strided(op["resid"][:mod or M], ld["ldr"]), ldr=ld["ldr"], resid_mod=mod)
    if flags & E.EPI_GELU_GRAD:
        kw.update(aux=_strided(op["aux"], ld["ldaux"]), ldaux=ld["ldaux"])
    if flags & E.EPI_OUT_F32:
        bufs["f32"] = Buf(M, ld["ldo"], torch.float32)
        kw.update(out_f32=bufs["f32"].t, ldo=ld["ldo"])
    if flags & E.EPI_OUT_BF:
        bufs["bf"] = Buf(M, ld["ldbf"], torch.bfloat16)
        kw.update(out_bf=bufs["bf"].t, ldbf=ld["ldbf"])
    if flags & E.EPI_GELU:
        bufs["pre"] = Buf(M, ld["ldp"], torch.bfloat16)
        kw.update(out_pre=bufs["pre"].t, ldp=ld["ldp"], pre_row_lo=PRE_LO)
    if flags & E.EPI_ROWDOT:
        total = -(-M // RD_ROWS) * (N // 64) * RD_ROWS
        bufs["rd"] = Buf(1, total, torch.float32, guard_rows=0)
        # (rows up to the end of the last tile exist behind the matrix, NaN: a row that is not clamped to M - 1 shows)
        kw.update(rd_other=_strided(op["other"], ld["ld_rd"], tail_rows=128), ld_rd=ld["ld_rd"], rd_rows=RD_ROWS, rowdot=bufs["rd"].flat[32:])
    _gemm(flags, _strided(A, K + 8), _strided(B, K + 16), M, N, K, **kw)
    return bufs


def _check_fp64(name, flags, mod, M, N, K, bufs):
    """the bars of tests/test_gemm_epilogues_gpu.py (_reference / _run_case) for these forms"""
    _, _, _, _, P, S = _problem(M, N, K)
    op = _operands(M, N)
    where = (name, M, N, K)
    x, mag = P, S
    if flags & E.EPI_BIAS:
        x, mag = x + op["bias"].double(), mag + op["bias"].double().abs()
    if flags & E.EPI_RESID:
        rows = torch.arange(M, device=DEV) % mod if mod else torch.arange(M, device=DEV)
        r = op["resid"].double()[rows]
        x, mag = x + r, mag + r.abs()
    acc = (K + 4) * U23 * mag
    if flags & E.EPI_GELU:
        ref = _gelu64(x)
        bound = U8 * ref.abs() + 2 * 1.13 * acc + 1.3e-4
    elif flags & E.EPI_GELU_GRAD:
        ref = P * _gelu_grad64(op["aux"].double())
        bound = U8 * ref.abs() + 2 * acc + 6e-4 * P.abs()
    else:
        ref, bound = x, U8 * x.abs() + 2 * acc
    worst = {}
    if "f32" in bufs:
        got = bufs["f32"].t[:M, :N]
        worst["out_f32"] = _worst(got, x, acc)
        assert bufs["f32"].untouched_outside(0, M, 0, N), (where, "out_f32: written outside [M][N]")
        assert bool((got != 0).all()), (where, "a zero output: the inputs are meant to exclude it")
    if "bf" in bufs:
        got = bufs["bf"].t[:M, :N]
        worst["out_bf"] = _worst(got, ref, bound)
        assert bufs["bf"].untouched_outside(0, M, 0, N), (where, "out_bf: written outside [M][N]")
        assert bool((got != 0).all()), (where, "a zero output: the inputs are meant to exclude it")
    if "pre" in bufs:
        worst["out_pre"] = _worst(bufs["pre"].t[PRE_LO:M, :N], x[PRE_LO:], U8 * x[PRE_LO:].abs() + 2 * acc[PRE_LO:])
        assert bufs["pre"].untouched_outside(PRE_LO, M, 0, N), (where, "out_pre: written outside rows [pre_row_lo, M) x [0, N)")
    for k, w in worst.items():
        assert w <= 1.0, (where, k, "err / bound", w)
    if "rd" in bufs:
        _check_rowdot(name, where, bufs["rd"], bufs["bf"].t[:M, :N], op["other"], P, acc, M, N, RD_ROWS)
    return max(worst.values())


def _same_bits(a, b):
    return all(torch.equal(a[k].flat.view(torch.int16 if a[k].flat.dtype == torch.bfloat16 else torch.int32),
                           b[k].flat.view(torch.int16 if b[k].flat.dtype == torch.bfloat16 else torch.int32)) for k in a)


@pytest.mark.parametrize("name", list(FORMS))
def test_ring_forms_match_two_stage_bits(name):
    """Every ring tile (128x128x4, 128x64x4, 128x64x3, 64x64x4, 64x64x3; the row-dot form: the two 64x64 rings) against the 2-stage form of the
    same tile: every output buffer equal bit for bit, guard elements included; the 2-stage outputs against fp64 under the epilogue-table bars."""
    flags, mod, aligned = FORMS[name]
    L = _lib.lib()
    worst = 0.0
    try:
        for M in MS:
            for N in NS_:
                for K in KS:
                    A, B, A2, B2, _, _ = _problem(M, N, K)
                    for base, rings in RINGS.items():
                        if (flags & E.EPI_ROWDOT) and base != 3:   # the row-dot form exists for the 64 x 64 tile only
                            continue
                        L.splice_gemm_force_tile(base)
                        ref = _launch(flags, mod, aligned, M, N, K, A, B)
                        worst = max(worst, _check_fp64(name, flags, mod, M, N, K, ref))
                        for code in rings:
                            L.splice_gemm_force_tile(code)
                            _launch(flags, mod, aligned, M, N, K, A2, B2)   # leaves the neighbouring slice's negated values in every LDS stage
                            got = _launch(flags, mod, aligned, M, N, K, A, B)
                            assert _same_bits(got, ref), (name, M, N, K, "tile code", code, "differs from the 2-stage form", base)
    finally:
        L.splice_gemm_force_tile(0)
    print(f"[gemm-drain] {name}: worst err / bound of the 2-stage outputs = {worst:.3f}")


@pytest.mark.parametrize("K", [64, 128, 192])
def test_proj_forward_tile_64x96(K):
    """The 64 x 96 three-stage ring of the proj forward (bias + fp32 residual) is chosen by shape: 64-row tiles with N % 96 == 0, more than 256
    tiles of 64 x 64 and at most 256 of 64 x 96 -- (1090, 960): 18 x 10 workgroups, a 2-row last tile.  Bit for bit against the 2-stage
    128 x 64 form (which the shape rule does not redirect), that one against fp64."""
    flags, M, N = E.EPI_BIAS | E.EPI_RESID | E.EPI_OUT_F32, 1090, 960
    L = _lib.lib()
    A, B, A2, B2, _, _ = _problem(M, N, K)
    try:
        L.splice_gemm_force_tile(2)
        ref = _launch(flags, 0, True, M, N, K, A, B)
        w = _check_fp64("bias_resid_f32 64x96", flags, 0, M, N, K, ref)
        L.splice_gemm_force_tile(23)
        _launch(flags, 0, True, M, N, K, A2, B2)
        got = _launch(flags, 0, True, M, N, K, A, B)
        assert _same_bits(got, ref), (M, N, K)
    finally:
        L.splice_gemm_force_tile(0)
    print(f"[gemm-drain] 64x96 K={K}: worst err / bound = {w:.3f}")
