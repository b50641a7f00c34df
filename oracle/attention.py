"""fp64 references, walk classes, worst-case element bounds and an fp32 rounding emulation of the FULL-SEQUENCE attention kernels (test
infrastructure only, torch-CPU): ``attn_fwd_x32_kernel`` (attn_x32.h), the dQ and dK/dV halves of attn_bwd_x32.h, the 16x16x32 backward
halves, the e4m3 forward, ``attn_delta_kernel`` and ``attn_probs_kernel`` of ``splice_amd/csrc/attention.hip``.

Four kinds of statement, none of them taken from what a kernel returns:
  * the CLASS of a tile walk (``fwd_class``, ``bwd_q_class``, ``bwd_kv_class``, ``small_class``): which prologue branches, how many main-loop
    trips, which tail, which ring phase, which masked-tile form and how many idle waves a sequence length T takes.  ``ATTN_T`` reaches every
    value of every component; tests/test_attention_cpu.py asserts it.
  * worst-case element bounds from the fp64 reference and the number formats (``U32``, ``UBF`` of oracle/loss_stage.py), first order in the unit
    roundoffs, every rounding counted where the kernel makes it (the derivations stand with the functions);
  * exact statements: padding rows of dqkv are zeros, launch forms agree bit for bit, nothing depends on what the padding rows hold;
  * the PREDICTION of which (query, tile) pairs of the x32 forward take the lazy rescale, from the fp64 scores and the kernel's stated rule.

Assumed, not derived (hardware accuracy): ``v_exp_f32`` and ``v_log_f32`` are good to one ulp of their result (2 u relative; oracle/cls_tail.py
assumes the same of ``v_exp_f32``), the log additionally to 2 u absolute where its result is below 1; an MFMA accumulates its exact products
in fp32 with at most one rounding per product and one per accumulator pass (``MFMA_R`` roundings for a 64-deep dot in four chained
instructions).  The fp8 MFMA is NOT that exact: fp8_score_bound states what a probe of the instruction found.  The printed err / bound ratios of tests/test_attention_gpu.py confirm or refute these.
"""
import functools
import math

import torch

from .loss_stage import U32, UBF, bf16_round, tld   # noqa: F401  (tld: re-exported for the tests)

F32, F64 = torch.float32, torch.float64
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
DH = 64
SCALE = 0.125
C2 = SCALE * LOG2E          # plain q: log2-unit score = C2 * q . k;  pre-scaled q: the stored q' = bf16(q * C2), score = q' . k, scale = ln 2
MFMA_R = 68                 # roundings a product can pass in a 64-deep dot of four chained 16-deep MFMAs (16 + 1 each)
RESCALE_LIMIT = 2.0 ** 30   # ATTN_RESCALE_LIMIT
FP8_LIMIT = 448.0           # ATTN8_RESCALE_LIMIT
FP8_SHIFT = 6.0             # ATTN8_REF_SHIFT
FLOOR = 1e-36               # flushed subnormals

# ------------------------------------------------------------------------------------------------ the case lists (CPU and GPU tests)
ATTN_T = [1, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129, 160, 161, 192, 193, 224, 256, 257, 289, 320, 321, 352, 384, 385, 416, 448, 449, 481,
          512, 513, 545, 576, 577, 640, 641, 704, 705, 737, 768, 769, 800, 833, 896, 897]
BASE_GEOM = (128, 2, 2)                                        # D, H, B: a head and a pass other than 0, ld = 384
WIDE_CASES = [(65, 384, 6, 1), (224, 384, 6, 1), (449, 384, 6, 1), (33, 768, 12, 1), (128, 768, 12, 1), (257, 768, 12, 1)]   # (T, D, H, B)
REGIMES = ["partner", "flat"]
NWS = (2, 4, 8)
PROBS_T = [33, 128, 197]                                       # < 64, T % 64 == 0, ragged
CHAIN_T = [33, 64, 96, 129, 449, 704]                          # the forward's own out / lse fed to the backward: every remainder class, both Tld % 64
# ramp cases (T, tiles that step up, level): level 1 = +46 log2 units (40 and a margin of 2^4 above the threshold for every query) (lazy rescale), level 2 = +240 (fp32 overflow: the exact walk).
# T = 384: six unmasked tiles (tile 1 = in flight during tile 0, even / odd interior, last unmasked, two in a row); T = 545: nine tiles, two
# main-loop trips, masked last tile; T = 129: a last tile with one live key.  With one tile (T < 64) the reference point is the exact row maximum
# and neither path can be reached by finite scores: the smallest exact-walk case is T = 65.
RAMP_CASES = [(129, (1,), 1), (129, (2,), 1), (384, (1,), 1), (384, (2,), 1), (384, (3,), 1), (384, (5,), 1), (384, (2, 3), 1),
              (545, (1,), 1), (545, (4,), 1), (545, (5,), 1), (545, (8,), 1), (545, (4, 5), 1),
              (65, (1,), 2), (128, (1,), 2), (193, (2,), 2)]
RAMP_STEP = {1: 46.0, 2: 240.0}


def ramp_queries(T):
    """the queries that see the step: a few per wave, never a whole wave of 32"""
    return [i for i in (1, 5, 34, 40, 63, 64, 200, T - 1) if 0 <= i < T]


# ------------------------------------------------------------------------------------------------ walk classes
def rem_class(T):
    r = T % 64
    return "0" if r == 0 else "1..31" if r < 32 else "32" if r == 32 else "33..63"


def _trips(n):
    return min(n, 2)


def fwd_class(T, NW):
    """attn_fwd_x32_kernel<NW, .> (attn_x32.h).  nt = ceil(T / 64) key tiles.
    prologue   l.171-174, 241, 245: issue_k / issue_v (0), then `nt > 1`, `nt > 2`, `nt > 3` -> min(nt, 4);
    main       l.361: `for (; t + 6 < nt; t += 2)`, two tiles a trip -> ceil((nt - 6) / 2) trips, classed 0 / 1 / >= 2;
    tail       l.365-368: the remaining nt - 2 trips tiles, 1..6, each with its own `t + 4 < nt`, `t + 2 < nt`, `t + 3 < nt` pattern;
    phase      slot = t % 3 (l.257, 264) against the parity of sb[] (l.262-263): nt % 6 is the state the walk ends in;
    remainder  l.282-287 masks the last tile (`kt + 64 > T`); T % 64 in {0} (no masked tile), {1..31}, {32}, {33..63} (both sub-tiles live);
    Tld % 64   l.145 `kt + 64 <= Tld`: 0 = the last tile is a full-tile DMA even when it holds masked keys, 32 = the clamped edge form;
    idle       l.124-125: (Tld / 32) % NW waves of the last workgroup have queries, the others only move tiles (0 = none idle)."""
    Tld, nt = tld(T), (T + 63) // 64
    trips = max(0, (nt - 6 + 1) // 2)
    return dict(prologue=min(nt, 4), main=_trips(trips), tail=nt - 2 * trips, phase=nt % 6, rem=rem_class(T), tld64=Tld % 64, idle=(Tld // 32) % NW)


def bwd_q_class(T, NW):
    """attn_bwd_q_x32_body<NW, .> (attn_bwd_x32.h).  nt = ceil(T / 64).
    prologue   l.110-112: issue(0), `nt > 1`, `nt > 2` -> min(nt, 3);   main  l.218: `for (; t + 4 < nt; ++t)` -> nt - 4 trips, 0 / 1 / >= 2;
    phase      slot = t & 3 (l.155): nt % 4;   remainder  l.169-172;   Tld % 64  l.76 (BxDma::tile);   idle  l.98-99."""
    Tld, nt = tld(T), (T + 63) // 64
    return dict(prologue=min(nt, 3), main=_trips(max(0, nt - 4)), phase=nt % 4, rem=rem_class(T), tld64=Tld % 64, idle=(Tld // 32) % NW)


def bwd_kv_class(T, NW):
    """attn_bwd_kv_x32_body<NW> (attn_bwd_x32.h): a wave owns 32 keys and walks the QUERY rows, nblk = Tld / 32 blocks, nt = ceil(Tld / 64) (l.251).
    prologue  l.268-270;  main  l.396;  phase  l.312;  half  l.323 `2 * t + blk >= nblk` breaks out of the half tile past Tld (Tld % 64 == 32);
    pad  l.400: keys T..Tld-1 are stored as zeros (Tld > T);  idle  l.245-246."""
    Tld = tld(T)
    nt = (Tld + 63) // 64
    return dict(prologue=min(nt, 3), main=_trips(max(0, nt - 4)), phase=nt % 4, rem=rem_class(T), tld64=Tld % 64, idle=(Tld // 32) % NW,
                half=Tld % 64 == 32, pad=Tld > T)


def small_class(T, fp8=False):
    """The 16x16x32 backward halves (attention.hip l.550-568, 660-670: full tiles, then <2, true> / <1, true> or the half tile) and the e4m3
    forward (l.359-361 the three tile forms, l.343-344 / 368 the split of the tiles over two ranges: per = ceil(nt / 2), so nt == 1 leaves
    the second range empty and odd / even nt give ranges of unequal / equal length)."""
    nt = (T + 63) // 64
    c = dict(rem=rem_class(T), tld64=tld(T) % 64, nt=min(nt, 4))
    if fp8:
        c["odd"] = nt % 2
    return c


# ------------------------------------------------------------------------------------------------ cases
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def partner_perm(T):
    """pi(i) = (a i + b) mod T with gcd(a, T) = 1: every key is the dominant key of exactly one query"""
    a = max(1, int(T * 0.618))
    while math.gcd(a, T) != 1:
        a += 1
    return (a * torch.arange(T) + T // 3) % T


def e4m3_round(x):
    return x.clamp(-448, 448).to(torch.float8_e4m3fn).to(F32)


def _draw(g, B, H, rows, regime):
    """unrounded q, k, v [B][H][rows][64] and the unit vectors behind them.  Values keep one sign per column, v_jd = s_d (1 + 0.2 N(0, 1)), for
    the reason oracle/cls_tail.py::attn_case gives: with values of random sign no element bound of the output could be small against it."""
    nq, nk = torch.randn(B, H, rows, DH, generator=g), torch.randn(B, H, rows, DH, generator=g)
    u, uq = torch.randn(B, H, rows, DH, generator=g), torch.randn(B, H, rows, DH, generator=g)
    u, uq = u / u.norm(dim=-1, keepdim=True), uq / uq.norm(dim=-1, keepdim=True)
    sgn = (torch.randint(2, (B, H, 1, DH), generator=g) * 2 - 1).float()
    v = 1 + 0.2 * torch.randn(B, H, rows, DH, generator=g)
    w = torch.randn(B, H, 1, DH, generator=g)
    return dict(nq=nq, nk=nk, u=u, uq=uq, sgn=sgn, v=v, w=w / w.norm(dim=-1, keepdim=True))


@functools.lru_cache(maxsize=None)
def make_qkv(T, D, H, B, regime, fold=False, pad_seed=0, fp8=False, ramp=None):
    """The stored operands of a case, fp32 [B][Tld][3D], exact in bf16 (fp8: in e4m3).  Rows < T come from one generator, the padding rows
    T..Tld-1 from another (`pad_seed`) with the same distribution: never zeros, never huge.  fold: the q columns hold bf16(q * C2).
    partner: k_j = 0.25 N + amp u_j, q_i = 0.25 N + amp u_pi(i), amp^2 / 8 = ln T + 1.   flat: q, k ~ N(0, 1).
    ramp = (tiles, level): q, k ~ 0.5 N; the keys at offsets 1 and 6 (one per lane half) of each named tile -- its first key where those are
    masked -- are g w and the queries of ramp_queries(T) carry + g w, g^2 C2 = RAMP_STEP[level] (twice that at the second of two tiles)."""
    Tld = tld(T)
    a, p = _draw(_gen("attn", T, D, B, regime), B, H, Tld, regime), _draw(_gen("attnpad", T, D, B, regime, pad_seed), B, H, Tld, regime)
    pad = (torch.arange(Tld) >= T)[None, None, :, None]
    m = {k: (torch.where(pad, p[k], a[k]) if a[k].shape[2] == Tld else a[k]) for k in a}
    if regime == "partner":
        amp = math.sqrt(8.0 * (math.log(T) + 1.0))
        uq = m["uq"].clone()
        uq[:, :, :T] = m["u"][:, :, partner_perm(T)]
        q, k = 0.25 * m["nq"] + amp * uq, 0.25 * m["nk"] + amp * m["u"]
    elif regime == "flat":
        q, k = m["nq"], m["nk"]
    elif regime == "ramp":
        tiles, level = ramp
        q, k = 0.5 * m["nq"], 0.5 * m["nk"]
        for n, t in enumerate(tiles):
            gk = math.sqrt(RAMP_STEP[level] / C2) * (n + 1)
            keys = [t * 64 + o for o in (1, 6) if t * 64 + o < T] or [t * 64]
            k[:, :, keys] = gk * m["w"]
        q[:, :, ramp_queries(T)] += math.sqrt(RAMP_STEP[level] / C2) * m["w"]
    else:
        raise ValueError(regime)
    v = m["sgn"] * m["v"]
    if fold:
        q = q * C2
    rnd = e4m3_round if fp8 else bf16_round
    qkv = torch.stack([rnd(q), rnd(k), rnd(v)], 0)                 # [3][B][H][Tld][64]
    return qkv.permute(1, 3, 0, 2, 4).reshape(B, Tld, 3 * D).contiguous()


def make_dout(T, D, B, seed=1):
    """bf16-exact upstream gradient [B][Tld][D]; padding rows are zero (the engine's invariant)"""
    d = bf16_round(torch.randn(B, tld(T), D, generator=_gen("dout", T, D, B, seed)))
    d[:, T:] = 0
    return d


def split_heads(x, H):
    """[B][rows][n * H * 64] -> n tensors [B][H][rows][64]"""
    B, rows, W = x.shape
    n = W // (H * DH)
    y = x.reshape(B, rows, n, H, DH).permute(2, 0, 3, 1, 4)
    return [y[i] for i in range(n)]


def join_heads(x):
    """[B][H][rows][64] -> [B][rows][H * 64]"""
    B, H, rows, _ = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, rows, H * DH)


# ------------------------------------------------------------------------------------------------ fp64 references
def fp8_score_bound(f):
    """What v_mfma_f32_16x16x32_fp8_fp8 can lose of a 64-deep e4m3 score, in log2 units, [B][H][T][T].  The instruction does not accumulate its 32
    exact products in fp32: it aligns them to the largest exponent sum E = max_k (e_a + e_b) of its operand pairs (e = floor(log2 |x|), -6 for
    a subnormal) and drops every product bit below 2^(E - 13), sign and magnitude; only the sum meets the accumulator in fp32.  Found with
    designed operands by tools/micro/mfma8_accuracy.hip (profiles/mfma8_accuracy.txt: +256 - 256 + 225 2^-(s+6) returns 224, 192, 128, 0 in
    units of 2^-(s+6) as s grows, the same under +900 - 900, whose operands have the same exponents; on N(0, 1) operands the error reaches
    558 u sum |ab|, far above an fp32 dot's).  Worst case: each of the 32 products loses less than 2^(E - 13), with E at most the sum of
    the largest operand exponents of the instruction; the kernel's score is two instructions, head dimensions d % 16 < 8 and the others."""
    T = f["T"]

    def expo(x):
        return torch.floor(torch.log2(x.abs().clamp(min=2.0 ** -9))).clamp(min=-6.0)

    eq, ek = expo(f["qe"][:, :, :T]), expo(f["k"][:, :, :T])
    first = (torch.arange(DH) % 16) < 8
    E = 0.0
    for sel in (first, ~first):
        E = E + 32 * torch.exp2(eq[..., sel].max(-1).values[..., :, None] + ek[..., sel].max(-1).values[..., None, :] - 13.0)
    return C2 * E


def forward_ref(qkv, T, H, fold=False):
    """fp64, for all Tld query rows against the T valid keys: dict z (log2-unit scores [B][H][Tld][T]), lse (log2 units [B][H][Tld]), P, out
    [B][H][Tld][64], and qe (the q the reference sees: q' / C2 for pre-scaled q), k, v (all Tld rows)."""
    q, k, v = split_heads(qkv.double(), H)
    qe = q / C2 if fold else q
    z = C2 * qe @ k[:, :, :T].transpose(-1, -2)
    zmax = z.max(-1, keepdim=True).values
    lse = zmax[..., 0] + torch.log2(torch.exp2(z - zmax).sum(-1))
    P = torch.exp2(z - lse[..., None])
    return dict(z=z, lse=lse, P=P, out=P @ v[:, :, :T], qe=qe, k=k, v=v, T=T, H=H, fold=fold)


def half_ulp_bf16(x):
    """half the bf16 spacing at magnitude x (8 significant bits, round to nearest: v_cvt_pk_bf16_f32): between 2^-9 x and 2^-8 x = UBF x"""
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp(min=1e-300))) - 8)


def _bf16_grid(x, E):
    """bf16 round-to-nearest-even of fp64 x, and the most a rounding of x + e, |e| <= E, can differ from it: nothing while x + e stays in x's
    rounding cell (distance to the nearest boundary > E), else E + one ulp (taken at |x| + E)."""
    a = x.abs().clamp(min=1e-300)
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    t = x / ulp
    frac = t - torch.floor(t)
    dist = (frac - 0.5).abs() * ulp
    ulp_hi = torch.exp2(torch.floor(torch.log2(a + E)) - 7)
    return bf16_round(x.float()).double(), (dist <= E).double() * (E + ulp_hi)


def backward_ref(f, dout, out_bf, E_lse_in, E_out_in=None):
    """The closed form the kernels restate, fp64, on rows < T, with its bounds.  dout [B][Tld][D]; out_bf [B][Tld][D] is the reference output
    rounded to bf16 (what the independent run hands over); E_lse_in [B][H][T] bounds the error of the handed lse (U32 |lse| for fp32(ref)),
    E_out_in [B][H][T][64] that of the handed out against out_bf (None: it IS out_bf).
    Quantities: delta = sum_d dO out_bf (what attn_delta_kernel defines), dP = dO v^T, ds = P (dP - delta), and -- P and dS are packed to bf16
    before the second MFMA -- dq = SCALE bf16(ds) k, dk = SCALE bf16(ds)^T qe, dv = bf16(P)^T dO, in the coordinates of qe (a kernel that
    took q' = C2 qe returns dq' = dq / C2).  With exact ds and P these are fp64 autograd (checked on the CPU); the bf16 steps stay in the
    reference because dO, k and q have random signs: a worst-case UBF sum_j |ds_j k_jd| is sqrt(T) times the half ulp of dq, and no
    element bound of that kind could be small against the signal.  The bounds instead count where the kernel's bf16(ds^) can differ:
      score   z^: a 64-deep MFMA dot seeded with -lse (x32) or followed by one fma (16x16): MFMA_R u (A + |lse|) + 3 u (|z| + |lse|), A = C2 |q|.|k|;
      p^      = exp2(z^ - lse^): rho = ln 2 (Ez + E_lse_in) + 2 u relative;
      delta^  eight 8-deep fma chains added in order: 10 u sum_d |dO out| + sum_d |dO| E_out_in;
      dP^ - delta^: MFMA_R u (|dO|.|v| + |delta|) + E_delta + u |dP - delta|;
      ds^     = p^ (dP^ - delta^): P (rho |dP - delta| + E_diff) + 2 u |ds|;
      sums    flips of the bf16 roundings (_bf16_grid), (65 nt + 8) u of fp32 accumulation over the Tld / 64 tiles, the scale, the bf16 store
              (half_ulp_bf16 of the value, not UBF times it: with N(0, 1) operands and T near 900 the flips alone take 0.7 % of the signal,
              and the bottom-of-binade figure UBF on top would leave the bound above the 1 % the CPU test asks for)."""
    T, H = f["T"], f["H"]
    P, z, lse = f["P"][:, :, :T], f["z"][:, :, :T], f["lse"][:, :, :T]
    qe, k, v = f["qe"][:, :, :T], f["k"][:, :, :T], f["v"][:, :, :T]
    dO = split_heads(dout.double(), H)[0][:, :, :T]
    ob = split_heads(out_bf.double(), H)[0][:, :, :T]
    delta = (dO * ob).sum(-1)
    dP = dO @ v.transpose(-1, -2)
    diff = dP - delta[..., None]
    ds = P * diff
    A = C2 * qe.abs() @ k.abs().transpose(-1, -2)
    Ez = MFMA_R * U32 * (A + lse.abs()[..., None]) + 3 * U32 * (z.abs() + lse.abs()[..., None])
    rho = LN2 * (Ez + E_lse_in[..., None]) + 2 * U32
    E_delta = 10 * U32 * (dO * ob).abs().sum(-1)
    if E_out_in is not None:
        E_delta = E_delta + (dO.abs() * E_out_in).sum(-1)
    E_diff = MFMA_R * U32 * (dO.abs() @ v.abs().transpose(-1, -2) + delta.abs()[..., None]) + E_delta[..., None] + U32 * diff.abs()
    E_ds = P * (rho * diff.abs() + E_diff) + 2 * U32 * ds.abs() + FLOOR
    dsb, flip_ds = _bf16_grid(ds, E_ds)
    Pb, flip_p = _bf16_grid(P, P * rho + FLOOR)
    nacc = (65 * ((tld(T) + 63) // 64) + 8) * U32
    dq, dk, dv = SCALE * dsb @ k, SCALE * dsb.transpose(-1, -2) @ qe, Pb.transpose(-1, -2) @ dO

    def store(val, pre, c=1.0):   # c: the stored number is val / c (dq' = dq / C2 for pre-scaled q), and it is that number's grid the store rounds on
        pre = pre + 2 * U32 * val.abs()
        return pre + c * half_ulp_bf16((val.abs() + pre) / c) + FLOOR

    E_dq = store(dq, SCALE * (flip_ds @ k.abs() + nacc * dsb.abs() @ k.abs()), C2 if f["fold"] else 1.0)
    E_dk = store(dk, SCALE * (flip_ds.transpose(-1, -2) @ qe.abs() + nacc * dsb.abs().transpose(-1, -2) @ qe.abs()))
    E_dv = store(dv, flip_p.transpose(-1, -2) @ dO.abs() + nacc * Pb.transpose(-1, -2) @ dO.abs())
    return dict(delta=delta, E_delta=E_delta + FLOOR, dP=dP, ds=ds, dq=dq, dk=dk, dv=dv, E_dq=E_dq, E_dk=E_dk, E_dv=E_dv,
                dq_plain=SCALE * ds @ k, dk_plain=SCALE * ds.transpose(-1, -2) @ qe, dv_plain=P.transpose(-1, -2) @ dO)


def backward_autograd(qkv, T, H, dout, fold=False):
    """fp64 autograd of <attention output, dout> with respect to (qe, k, v) on rows < T: three tensors [B][H][T][64]"""
    q, k, v = split_heads(qkv.double(), H)
    leaves = [((q / C2 if fold else q)[:, :, :T]).clone().requires_grad_(True), k[:, :, :T].clone().requires_grad_(True), v[:, :, :T].clone().requires_grad_(True)]
    p = torch.softmax(SCALE * leaves[0] @ leaves[1].transpose(-1, -2), -1)
    ((p @ leaves[2]) * split_heads(dout.double(), H)[0][:, :, :T]).sum().backward()
    return [x.grad for x in leaves]


# ------------------------------------------------------------------------------------------------ forward bounds
def forward_bounds(f, fp8=False, rescales=0, exact=False):
    """(E_lse [B][H][T], E_out [B][H][T][64]) on the query rows < T.  rescales: how many lazy rescales a query may take (0 in the partner and
    flat regimes, which the CPU test asserts; nt in the ramp regime); exact: the query may take the exact walk.
    score  z^_ij: a 64-deep MFMA dot (MFMA_R roundings of A_ij = C2 |q_i|.|k_j|; pre-scaled q seeds the accumulator with the reference
           point, whose magnitude then rides along: M_i = max_j |z_ij| + 1 bounds it as long as no rescale moves it, which the CPU test
           asserts of the regimes these bounds are used in; fp8: the shifted point, + 7) and, for plain q, fma(s, c2, -m) with c2 itself
           rounded: Ez = MFMA_R u (A + M) + 3 u (|z| + M).
    e^_ij  = exp2(z^ - m): the reference point cancels in every ratio, so only rho = ln 2 Ez + 2 u (a 1-ulp exp2) counts.
    l      the row sum of non-negative terms, at most 8 + 3 adds per tile in a lane, one per tile into l, one across the lane pair:
           (nt + 12) u relative, and the terms' own errors S_i = sum_j P_ij rho_ij.
    lse    = m + log2(l): log2(e) (S + (nt + 12) u), the log itself 2 u max(|log2 l|, 1) with |log2 l| <= |lse| + M, the add u (|lse| + M):
           E_lse = log2(e) (S + (nt + 12) u) + 4 u (|lse| + M + 1).
    out    = sum_j bf16(e^_ij) v_jd / l: sum_j P_ij (rho_ij + UBF) |v_jd|, the MFMA accumulation over nt tiles of 64 and the division
           (S + (65 nt + 20) u) sum_j P_ij |v_jd|, then the bf16 store UBF (|out| + all of the above).
    fp8    P goes to e4m3 instead: 2^-4 relative for a normal, 2^-10 absolute below 2^-6; the probabilities are formed against a point at
           most 6 binary orders below the row's running maximum (it only ever moves to `tile maximum - 6`), so 2^-10 there is at most
           2^-16 max_j P_ij of the normalised row: sum_j (P_ij (rho_ij + 2^-4) + 2^-16 Pmax_i) |v_jd|.  The row sum takes the unquantised
           probabilities: E_lse as above.
    rescale  a move of the point by shift = log2(l): alpha = exp2(-shift) (2 u) times l and o (u each, the SAME alpha: out = o / l only sees
           the products' roundings), the new point fl(m + shift) (u M: the mass gathered so far now sits u M log2 units off the frame the
           coming tiles are formed in) and the in-flight scores less shift (one more rounding, u (|z| + M)); the point stays below
           max_j z_ij + log2(T) + 1, so M grows by 12: rescales (4 + M) u on l and on o, 4 u (|z| + M) in Ez.
    exact  x32_exact_rows: 64-deep fma chains for the scores (inside Ez), P not rounded, one fma per key into o and l and a factor alpha
           (3 u) whenever the running maximum moves, at most once per key of the lane's half: 2 T u more on l and on o."""
    T = f["T"]
    z, P, lse = f["z"][:, :, :T], f["P"][:, :, :T], f["lse"][:, :, :T]
    qe, k, v, out = f["qe"][:, :, :T], f["k"][:, :, :T], f["v"][:, :, :T], f["out"][:, :, :T]
    nt = (T + 63) // 64
    A = C2 * qe.abs() @ k.abs().transpose(-1, -2)
    M = z.abs().max(-1, keepdim=True).values + (1 + FP8_SHIFT if fp8 else 1) + (12 if rescales else 0)
    Ez = MFMA_R * U32 * (A + M) + (4 if rescales else 3) * U32 * (z.abs() + M)
    if fp8:
        Ez = Ez + fp8_score_bound(f)
    rho = LN2 * Ez + 2 * U32
    S = (P * rho).sum(-1) + rescales * (4 + M[..., 0]) * U32 + (2 * T * U32 if exact else 0)
    E_lse = LOG2E * (S + (nt + 12) * U32) + 4 * U32 * (lse.abs() + M[..., 0] + 1)
    quant = P * (rho + 2.0 ** -4) + 2.0 ** -16 * P.max(-1, keepdim=True).values if fp8 else P * (rho + UBF)
    pre = quant @ v.abs() + (S + (65 * nt + 20) * U32 + (2.0 ** -8 if fp8 else 0.0))[..., None] * (P @ v.abs())
    return E_lse, pre + UBF * (out.abs() + pre) + FLOOR


def probs_bounds(f, E_lse_in):
    """attn_probs_kernel: exp2(fl(fl(s * scale) * log2e) - lse) with s a 64-term fp32 chain: 70 u (A + |z|) on the exponent, the handed lse"""
    T = f["T"]
    z, P, lse = f["z"][:, :, :T], f["P"][:, :, :T], f["lse"][:, :, :T]
    A = C2 * f["qe"][:, :, :T].abs() @ f["k"][:, :, :T].abs().transpose(-1, -2)
    return P * (LN2 * (70 * U32 * (A + z.abs()) + U32 * lse.abs()[..., None] + E_lse_in[..., None]) + 2 * U32) + FLOOR


# ------------------------------------------------------------------------------------------------ the lazy rescale, predicted
def _lane_half(T):
    return ((torch.arange(T) % 8) >= 4)


def rescale_plan(f):
    """The walk of the x32 forward's reference point in fp64, by the kernel's stated rule (attn_x32.h l.337-353): the point starts at the row
    maximum of tile 0; after tile t a query whose partial row sum of the tile IN EITHER LANE HALF (keys with bit 2 of the index clear / set)
    reaches 2^30 moves it by log2(row sum so far).  Returns fire [B][H][Tld][nt] (bool), ps (log2 of the larger half sum, [B][H][Tld][nt])
    and exact [B][H][Tld]: a score at least 128 above the point in force overflows fp32 and sends the query to the exact walk."""
    z, T = f["z"], f["T"]
    nt = (T + 63) // 64
    half = _lane_half(T)
    m = z[..., :min(T, 64)].max(-1).values
    l = torch.zeros_like(m)
    fire, ps, exact = [], [], torch.zeros_like(m, dtype=torch.bool)
    for t in range(nt):
        zt, ht = z[..., t * 64:min(T, t * 64 + 64)] - m[..., None], half[t * 64:min(T, t * 64 + 64)]
        exact |= (zt >= 128).any(-1)
        e = torch.exp2(zt.clamp(max=1000))
        h0, h1 = (e * (~ht)).sum(-1), (e * ht).sum(-1)
        big = torch.maximum(h0, h1)
        l = l + h0 + h1
        fr = big >= RESCALE_LIMIT
        shift = torch.where(fr, torch.log2(l), torch.zeros_like(l))
        m, l = m + shift, l * torch.exp2(-shift)
        fire.append(fr)
        ps.append(torch.log2(big.clamp(min=1e-300)))
    return torch.stack(fire, -1), torch.stack(ps, -1), exact


def fp8_limit_hits(f):
    """How many (query, tile) pairs of the one-range e4m3 walk take the exact step BEYOND the first tile (which always does: the point starts
    at -1e30): a lane's 16 keys of the tile (8 of each 32-key sub-tile, lane group g = (key % 32) // 8) sum to >= 448 against the point in
    force, which then moves to max(point, tile maximum - 6)."""
    z, T = f["z"][:, :, :f["T"]], f["T"]
    grp = (torch.arange(T) % 32) // 8
    m = z[..., :min(T, 64)].max(-1).values - FP8_SHIFT
    hits = 0
    for t in range(1, (T + 63) // 64):
        zt, gt = z[..., t * 64:min(T, t * 64 + 64)], grp[t * 64:min(T, t * 64 + 64)]
        e = torch.exp2(zt - m[..., None])
        over = torch.stack([(e * (gt == g)).sum(-1) for g in range(4)], -1).max(-1).values >= FP8_LIMIT
        hits += int(over.sum())
        m = torch.where(over, torch.maximum(m, zt.max(-1).values - FP8_SHIFT), m)
    return hits


# ------------------------------------------------------------------------------------------------ fp32 emulation
FWD_MUTS = ["drop_last_key", "admit_pad_key", "stale_tile", "skip_subtile", "heads_swapped", "lse_missing_tile"]
RESCALE_MUTS = ["rescale_o_not_l", "rescale_not_inflight"]
BWD_MUTS = ["drop_last_key", "admit_pad_key", "delta_other_head", "dk_sign", "dk_scale", "pad_dk_kept"]


def forward_emulate(qkv, T, H, fold=False, mut=None, fp8=False):
    """The x32 forward's rounding points in torch fp32, tile by tile: (out bf16-exact [B][H][Tld][64], lse [B][H][Tld], n_rescaled).  fp8: P is
    rounded to e4m3 against a point 6 binary orders below the running maximum instead of to bf16.
    mut: 'drop_last_key' (key T - 1 masked) | 'admit_pad_key' (key T live, T < Tld) | 'stale_tile' (the scores of the last tile come from
    the K rows of the tile before: a ring slot not refilled, nt >= 2) | 'skip_subtile' (the last live 32-key sub-tile of the masked tile
    contributes nothing, T % 64 != 0) | 'heads_swapped' (head h stores to h ^ 1) | 'lse_missing_tile' (lse without the last tile's mass) |
    'rescale_o_not_l' | 'rescale_not_inflight' (the scores of tile t + 1, formed against the old point, are not moved)."""
    q, k, v = split_heads(qkv.to(F32), H)
    Tld = qkv.shape[1]
    Tv = T - 1 if mut == "drop_last_key" else T + 1 if mut == "admit_pad_key" and T < Tld else T
    nt = (Tv + 63) // 64
    c2 = torch.tensor(1.0 if fold else C2, dtype=F32)
    z = (q @ k.transpose(-1, -2)) * c2                                             # [B][H][Tld][Tld]
    if mut == "stale_tile" and nt >= 2:
        lo = (nt - 1) * 64
        z[..., lo:Tv] = z[..., lo - 64:Tv - 64]
    live = torch.arange(Tld) < Tv
    if mut == "skip_subtile" and T % 64:
        lo = (T - 1) // 32 * 32
        live[lo:lo + 32] = False
    z = torch.where(live, z, torch.full_like(z, -1e30))
    m = z[..., :64].max(-1).values - (FP8_SHIFT if fp8 else 0.0)
    ms = m.clone()                                                                 # the point the scores of the coming tile were formed against
    l, o = torch.zeros_like(m), torch.zeros_like(q)
    last_ps, n_resc = torch.zeros_like(m), 0
    for t in range(nt):
        cols = slice(t * 64, min(Tld, t * 64 + 64))
        if fp8:   # the exact step at every tile (a point the kernel may hold as well): the state moves to max(point, tile maximum - 6) first
            mn = torch.maximum(m, z[..., cols].max(-1).values - FP8_SHIFT)
            alpha = torch.exp2(m - mn)
            l, o, m, ms = l * alpha, o * alpha[..., None], mn, mn
        e = torch.exp2(z[..., cols] - ms[..., None])
        ps = e.sum(-1)
        l = l + ps
        o = o + (e4m3_round(e) if fp8 else bf16_round(e)) @ v[:, :, cols]
        last_ps = ps
        ms = m
        fr = ps >= RESCALE_LIMIT
        if not fp8 and bool(fr.any()):
            n_resc += int(fr.sum())
            shift = torch.where(fr, torch.log2(l), torch.zeros_like(l))
            alpha = torch.exp2(-shift)
            old = m
            m = m + shift
            o = o * alpha[..., None]
            if mut != "rescale_o_not_l":
                l = l * alpha
            ms = old if mut == "rescale_not_inflight" else m                       # (a tile formed against the old point is 2^shift too heavy)
    lt = l - last_ps if mut == "lse_missing_tile" else l
    out = bf16_round(o / l[..., None])
    if mut == "heads_swapped":
        out = out[:, torch.arange(H) ^ 1]
    return out, m + torch.log2(lt), n_resc


def backward_emulate(qkv, T, H, dout, out_bf, lse32, fold=False, mut=None):
    """Both backward forms' rounding points in torch fp32: dict delta [B][H][Tld], dq, dk, dv [B][H][Tld][64] (bf16-exact; dq in the stored q's
    coordinates times C2 for pre-scaled q, i.e. comparable with backward_ref).  mut: 'drop_last_key' | 'admit_pad_key' | 'delta_other_head' |
    'dk_sign' | 'dk_scale' (the factor left out) | 'pad_dk_kept' (the dk / dv of the padding keys are stored as accumulated)."""
    q, k, v = split_heads(qkv.to(F32), H)
    Tld = qkv.shape[1]
    dO, ob = split_heads(dout.to(F32), H)[0], split_heads(out_bf.to(F32), H)[0]
    Tv = T - 1 if mut == "drop_last_key" else T + 1 if mut == "admit_pad_key" and T < Tld else T
    sc = torch.tensor(LN2 if fold else SCALE, dtype=F32)
    c2 = torch.tensor(1.0 if fold else C2, dtype=F32)
    delta = (dO * ob).sum(-1)
    dl = delta[:, torch.arange(H) ^ 1] if mut == "delta_other_head" else delta
    p = torch.exp2((q @ k.transpose(-1, -2)) * c2 - lse32.to(F32)[..., None])
    p_all = p.clone()
    p[..., Tv:] = 0
    ds = p * (dO @ v.transpose(-1, -2) - dl[..., None])
    dsb, pb = bf16_round(ds), bf16_round(p)
    dq = bf16_round((dsb @ k) * sc)
    ksc = -sc if mut == "dk_sign" else torch.tensor(1.0, dtype=F32) if mut == "dk_scale" else sc
    dk, dv = bf16_round((dsb.transpose(-1, -2) @ q) * ksc), bf16_round(pb.transpose(-1, -2) @ dO)
    if mut == "pad_dk_kept":
        ds_all = p_all * (dO @ v.transpose(-1, -2) - dl[..., None])
        dk, dv = bf16_round((bf16_round(ds_all).transpose(-1, -2) @ q) * sc), bf16_round(bf16_round(p_all).transpose(-1, -2) @ dO)
    else:
        dk[:, :, T:], dv[:, :, T:] = 0, 0
    dq = dq.double() * (C2 if fold else 1.0)     # dq' C2 = dq;  dk = ln 2 ds^T q' = SCALE ds^T qe as it stands
    return dict(delta=delta, dq=dq, dk=dk, dv=dv)
