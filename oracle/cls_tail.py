"""fp64 references, bit-exact predictions, worst-case element bounds and an fp32 rounding emulation of the [CLS] TAIL of the top ViT
block (test infrastructure only, torch-CPU): the five kernels of ``splice_amd/csrc/vit_cls.hip`` -- single-query attention forward /
backward, LayerNorm of a few strided rows forward / backward, and the finisher of the split-K row GEMMs.

Three kinds of statement, none of them taken from what a kernel returns:
  * bit-exact predictions where the kernel is plain IEEE fp32 in a fixed order: every split-K slab sum (emulated in torch fp32, starting
    where the kernel starts, adding in slab order), ``dv_j = bf16(fp32(p_j dO_d))`` and ``g_bf = bf16(g)``;
  * worst-case element bounds from the fp64 reference and the number formats (``U32``, ``UBF`` of oracle/loss_stage.py), first order in
    the unit roundoffs, every rounding counted where it happens (the derivations stand with the functions);
  * the GELU bars ``common.h`` states for ``gelu_f`` / ``gelu_grad_f`` (1.3e-4 absolute, 6e-4 |P|), as tests/test_gemm_epilogues_gpu.py
    uses them.
``tests/test_cls_tail_cpu.py`` checks on a machine without a GPU that the fp32 emulation of the kernels' roundings stays inside every
bound, that every bound is small against the signal, and that each deliberate small error (the ``mut`` switches of the emulation) leaves
a bound or breaks a prediction; ``tests/test_cls_tail_gpu.py`` holds the kernels to the same statements.
"""
import math

import torch

from .loss_stage import U32, UBF, bf16_round, tld   # noqa: F401  (tld: re-exported for the tests)

F32, F64 = torch.float32, torch.float64
LOG2E = 1.4426950408889634
DH = 64                     # head width of the kernels
SCALE = 0.125

# ------------------------------------------------------------------------------------------------ the case lists (CPU and GPU tests)
ATTN_SHAPES = [(1, 32), (17, 32), (65, 96), (257, 288), (785, 800), (840, 864), (1030, 1056)]   # (T, Tld)
ATTN_DIMS = [(384, 6), (768, 12)]                                                                 # (D, H)
ATTN_REGIMES = ["flat", "sharp"]
ATTN_BATCHED = [65, 257]    # T of the B = 3 cases
ATTN_SLABS = [1, 6, 12, 16]
ATTN_CASES = [(T, Tld, D, H, 1, regime) for T, Tld in ATTN_SHAPES for D, H in ATTN_DIMS for regime in ATTN_REGIMES] + \
             [(T, Tld, D, H, 3, regime) for T, Tld in ATTN_SHAPES if T in ATTN_BATCHED for D, H in ATTN_DIMS for regime in ATTN_REGIMES]
LN_DIMS = [4, 100, 384, 768]
LN_ROWS = [1, 3]
LN_FWD_SLABS = [0, 1, 6, 16, 17]     # 0: no slabs (x is read)
LN_BWD_SLABS = [1, 12, 17]
LN_EPS = 1e-6
FIN_SHAPES = [(1, 384), (3, 100), (2, 1536)]
FIN_SLABS = [1, 8, 9, 16]
GELU_ABS = 1.3e-4           # common.h: gelu_f, tails included
GELU_GRAD_REL = 6e-4        # common.h: gelu_grad_f, saturation included; times |P|


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def split_heads(qkv, H):
    """qkv [T][3D] -> q [H][64] (the [CLS] row), k [H][T][64], v [H][T][64]"""
    T, D = qkv.shape[0], qkv.shape[1] // 3
    q = qkv[0, :D].reshape(H, DH)
    k = qkv[:, D:2 * D].reshape(T, H, DH).transpose(0, 1)
    v = qkv[:, 2 * D:].reshape(T, H, DH).transpose(0, 1)
    return q, k, v


def attn_case(T, D, H, B, regime, seed=1):
    """bf16-exact fp32 qkv [B][T][3D] (the valid rows of B passes).  flat: q, k ~ N(0, 1) (scores ~ N(0, 1) at scale 0.125).  sharp: per
    head the [CLS] query is alpha * (one key), alpha found by bisection so that this key's probability is 0.9 before q is rounded to bf16;
    head 0 takes key T - 1.  In both regimes a value column keeps one sign, v_jd = s_d (1 + 0.2 N(0, 1)): with values of random sign the
    bf16 rounding of p alone (2^-8 sum_j p_j |v_jd|) is sqrt(T) times the half ulp of the output, and no element bound could be small
    against the signal."""
    g = _gen("attn", T, D, B, regime, seed)
    qkv = torch.randn(B, T, 3 * D, generator=g)
    sgn = (torch.randint(2, (B, 1, D), generator=g) * 2 - 1).float()
    qkv[:, :, 2 * D:] = sgn * (1 + 0.2 * torch.randn(B, T, D, generator=g))
    qkv = bf16_round(qkv)
    if regime == "sharp" and T > 1:
        for b in range(B):
            _, k, _ = split_heads(qkv[b].double(), H)
            jstar = torch.tensor([(T - 1 - h * max(T // H, 1)) % T for h in range(H)])
            ks = k[torch.arange(H), jstar]                                   # [H][64]
            base = SCALE * torch.einsum("htd,hd->ht", k, ks)                 # scores at alpha = 1
            lo, hi = torch.zeros(H, dtype=F64), torch.full((H,), 64.0, dtype=F64)
            for _ in range(60):
                mid = (lo + hi) / 2
                p = torch.softmax(mid[:, None] * base, 1)[torch.arange(H), jstar]
                lo, hi = torch.where(p < 0.9, mid, lo), torch.where(p < 0.9, hi, mid)
            qkv[b, 0, :D] = bf16_round((hi[:, None] * ks).float()).reshape(D)
    elif regime not in ("flat", "sharp"):
        raise ValueError(regime)
    return qkv


def dout_slabs(B, D, n, seed=1):
    """n fp32 split-K slabs [n][B][D] of the gradient of the attention output"""
    return torch.randn(n, B, D, generator=_gen("dout", B, D, n, seed)) / math.sqrt(n)


# ------------------------------------------------------------------------------------------------ slab sums (bit-exact)
def slab_sum_f32(start, slabs, mut=None):
    """((start + s_0) + s_1) + ... in fp32, the kernels' order.  mut: 'skip_last_slab' | 'reverse_slabs'."""
    order = list(range(slabs.shape[0]))
    if mut == "skip_last_slab":
        order = order[:-1]
    if mut == "reverse_slabs":
        order = order[::-1]
    v = start.to(F32).clone()
    for s in order:
        v = v + slabs[s].to(F32)
    return v


def attn_dO(slabs, mut=None):
    """dO of attn_cls_bwd: bf16(0 + s_0 + s_1 + ...), [B][D]; mut 'dO_unrounded' leaves the fp32 sum"""
    v = slab_sum_f32(torch.zeros_like(slabs[0]), slabs, mut)
    return v if mut == "dO_unrounded" else bf16_round(v)


# ------------------------------------------------------------------------------------------------ attention: fp64 reference
def attn_ref(qkv, H, scale=SCALE):
    """fp64 single-query softmax attention of one pass, qkv [T][3D]: (p [H][T], out [D])"""
    q, k, v = split_heads(qkv.double(), H)
    p = torch.softmax(scale * torch.einsum("htd,hd->ht", k, q), 1)
    return p, torch.einsum("ht,htd->hd", p, v).reshape(-1)


def attn_bwd_autograd(qkv, H, dO, scale=SCALE):
    """fp64 autograd of <attention output of the [CLS] query, dO> with respect to qkv: [T][3D]"""
    leaf = qkv.double().clone().requires_grad_(True)
    q, k, v = split_heads(leaf, H)
    p = torch.softmax(scale * torch.einsum("htd,hd->ht", k, q), 1)
    (torch.einsum("ht,htd->hd", p, v).reshape(-1) * dO.double()).sum().backward()
    return leaf.grad


def _bf16_grid(x):
    """(ulp, round-to-nearest-even on the bf16 grid, distance to the nearest rounding boundary) of fp64 x, normal range"""
    a = x.abs().clamp(min=1e-300)
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    t = x / ulp
    frac = t - torch.floor(t)
    return ulp, torch.round(t) * ulp, (frac - 0.5).abs() * ulp


def attn_bwd_ref(qkv, H, dO, scale=SCALE):
    """The closed form the kernel restates, fp64, for one pass and a given dO [D]: dict of dP, delta, ds [H][T], dk [T][D], dq_plain [D]
    (= autograd) and dq [D] = sum_j bf16(ds_j) k_j, the quantity the kernel defines (ds packed to bf16 as the full attention kernel does);
    ds_bf, ds_ulp, ds_dist carry the rounding of ds for the bound.  dv is predicted bit for bit (attn_dv_pred), not bounded."""
    q, k, v = split_heads(qkv.double(), H)
    T = qkv.shape[0]
    p = torch.softmax(scale * torch.einsum("htd,hd->ht", k, q), 1)
    dOh = dO.double().reshape(H, DH)
    dP = torch.einsum("htd,hd->ht", v, dOh)
    delta = (p * dP).sum(1)
    ds = p * (dP - delta[:, None]) * scale
    ulp, ds_bf, dist = _bf16_grid(ds)
    dk = (ds[:, :, None] * q[:, None, :]).transpose(0, 1).reshape(T, -1)
    return dict(p=p, dP=dP, delta=delta, ds=ds, ds_bf=ds_bf, ds_ulp=ulp, ds_dist=dist, dk=dk,
                dq_plain=torch.einsum("ht,htd->hd", ds, k).reshape(-1), dq=torch.einsum("ht,htd->hd", ds_bf, k).reshape(-1))


def attn_dv_pred(probs32, dO_bf, T):
    """dv rows < T: bf16(fp32(p_j * dO_d)) from the fp32 probabilities handed to the backward ([H][>= T]) and the bf16 dO [D]: [T][D]"""
    H = probs32.shape[0]
    prod = probs32[:, :T, None].to(F32) * dO_bf.to(F32).reshape(H, 1, DH)
    return bf16_round(prod).transpose(0, 1).reshape(T, -1)


# ------------------------------------------------------------------------------------------------ attention: bounds
def _dot_err(a, b):
    """Rounding error of the 64-term fp32 dot the kernels accumulate two exact bf16 products at a time, in index order (32 dot2 steps): the
    products of step m pass through the roundings of steps m .. 31, at most two each (whether the instruction rounds once or twice is not
    assumed): sum_i 2 (32 - i // 2) u |a_i b_i|.  Over the last axis."""
    w = 2.0 * (32 - torch.arange(DH, dtype=F64) // 2) * U32
    return ((a * b).abs() * w).sum(-1)


def attn_fwd_bounds(qkv, H, Tld, scale=SCALE):
    """(Ep [H][T], Eout [D]) for one pass.
    score:  s_j = fl(scale * dot64): the dot of exact bf16 products (_dot_err) and the scaling (2 u): Es_j.
    p:      p_j = e_j / sum_l e_l with e_j = exp2((s_j - mx) log2e).  The shift mx cancels in the ratio whatever its value, so only the
            score errors and the roundings of e_j count: the subtraction, the constant and the product (3 u |s_j - mx|, |s_j - mx| <=
            R_j + 1 with R_j = max s - s_j) and a 1-ulp exp2 (2 u): rho_j = Es_j + 3 u (R_j + 1) + 2 u.  The sum of non-negative terms
            adds 16 u (at most 5 adds in a thread, 6 butterfly steps, 2 across the waves), 1 / sum and the product 3 u:
            |p^_j - p_j| <= p_j (rho_j + sum_l p_l rho_l + 19 u) + 1e-37   (the last: an exp2 flushed to zero below 2^-126).
    out:    sum_j bf16(p^_j) v_jd in fp32, rounded to bf16: sum_j (Ep_j + UBF (p_j + Ep_j)) |v_jd|, an accumulation of at most Tld / 4 + 4
            roundings per partial chain, and the output's own rounding UBF (|out| + all of the above)."""
    q, k, v = split_heads(qkv.double(), H)
    s = scale * torch.einsum("htd,hd->ht", k, q)
    p = torch.softmax(s, 1)
    Es = scale * (_dot_err(k, q[:, None, :]) + 2 * U32 * torch.einsum("htd,hd->ht", k.abs(), q.abs()))
    rho = Es + 3 * U32 * (s.max(1, keepdim=True).values - s + 1) + 2 * U32
    Ep = p * (rho + (p * rho).sum(1, keepdim=True) + 19 * U32) + 1e-37
    pv = torch.einsum("ht,htd->hd", p, v.abs())
    pre = torch.einsum("ht,htd->hd", Ep + UBF * (p + Ep), v.abs()) + (Tld / 4 + 4) * U32 * pv
    out = torch.einsum("ht,htd->hd", p, v)
    return Ep, (pre + UBF * (out.abs() + pre)).reshape(-1)


def attn_bwd_bounds(qkv, H, Tld, dO, Ep_in, scale=SCALE, r=None):
    """(E_dk [T][D], E_dq [D], E_ds [H][T]) for one pass (r: its attn_bwd_ref, if at hand), dO [D] exact (the bf16 sum is predicted), Ep_in [H][T] the error of the probabilities handed
    to the backward (U32 * p for the fp64 reference rounded to fp32).
    dP_j:   a 64-term dot of exact bf16 products (_dot_err) = E_dP_j.
    delta:  sum_l p^_l dP^_l of the SAME computed dP^_l: its own roundings are sum_l Ep_in_l |dP_l| and 16 u sum_l p_l |dP_l| (the product,
            5 + 6 + 2 adds, cancellation bounded with absolute values) = E_delta.
    dP_j - delta:  the error e_l of dP^_l enters as (1 - p_j) e_j - sum_{l != j} p_l e_l (a key that holds most of the probability
            carries most of delta): (1 - p_j) E_dP_j + sum_{l != j} p_l E_dP_l + E_delta = E_diff_j.
    ds_j:   p_j (dP_j - delta) scale: scale (Ep_in_j |dP_j - delta| + p_j E_diff_j) + 4 u |ds_j| = E_ds_j.
    dk_jd:  bf16(ds_j q_d): |q_d| E_ds_j + u |dk| = e, then UBF (|dk| + e).
    dq_d:   sum_j bf16(ds_j) k_jd against the reference's own bf16(ds_j): the two roundings agree unless ds_j lies within E_ds_j of a
            rounding boundary, where they may differ by one bf16 ulp: sum_j [dist_j <= E_ds_j] ulp_j |k_jd|, an accumulation of
            Tld / 4 + 4 roundings, and the output's rounding."""
    q, k, v = split_heads(qkv.double(), H)
    T = qkv.shape[0]
    r = attn_bwd_ref(qkv, H, dO, scale) if r is None else r
    p, dP, delta, ds = r["p"], r["dP"], r["delta"], r["ds"]
    E_dP = _dot_err(v, dO.double().reshape(H, 1, DH))
    E_delta = (Ep_in * dP.abs()).sum(1) + 16 * U32 * (p * dP.abs()).sum(1)
    S = (p * E_dP).sum(1, keepdim=True)
    E_diff = (1 - p) * E_dP + (S - p * E_dP) + E_delta[:, None]
    E_ds = scale * (Ep_in * (dP - delta[:, None]).abs() + p * E_diff) + 4 * U32 * ds.abs()
    dk = ds[:, :, None] * q[:, None, :]
    e = E_ds[:, :, None] * q.abs()[:, None, :] + U32 * dk.abs()
    E_dk = (e + UBF * (dk.abs() + e)).transpose(0, 1).reshape(T, -1)
    flip = (r["ds_dist"] <= E_ds).double() * r["ds_ulp"]
    pre = torch.einsum("ht,htd->hd", flip, k.abs()) + (Tld / 4 + 4) * U32 * torch.einsum("ht,htd->hd", r["ds_bf"].abs(), k.abs())
    E_dq = (pre + UBF * (r["dq"].abs().reshape(H, DH) + pre)).reshape(-1)
    return E_dk, E_dq, E_ds


# ------------------------------------------------------------------------------------------------ attention: fp32 emulation
def _block_sum256(v):
    """block_sum256 of vit_cls.hip on a [..., 256] fp32 tensor: xor butterfly inside each wave of 64, then (w0 + w1) + (w2 + w3)"""
    w = v.reshape(*v.shape[:-1], 4, 64)
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., idx ^ o]
    w = w[..., 0]
    return (w[..., 0] + w[..., 1]) + (w[..., 2] + w[..., 3])


def _strided_thread_sums(x, n):
    """thread t of 256 adds x[..., t], x[..., t + 256], ... in order (fp32); x [..., n]"""
    pad = (-n) % 256
    x = torch.cat([x, torch.zeros(*x.shape[:-1], pad, dtype=x.dtype)], -1).reshape(*x.shape[:-1], -1, 256)
    acc = torch.zeros(*x.shape[:-2], 256, dtype=x.dtype)
    for i in range(x.shape[-2]):
        acc = acc + x[..., i, :]
    return acc


def _dot64_f32(a, b):
    """fp32 dot over the last axis (64), accumulated two products at a time in index order, as the dot2 chain walks it"""
    acc = torch.zeros(torch.broadcast_shapes(a.shape, b.shape)[:-1], dtype=F32)
    for i in range(0, DH, 2):
        acc = acc + (a[..., i] * b[..., i] + a[..., i + 1] * b[..., i + 1])
    return acc


def _quarters_dot(w, m, Tld):
    """sum_j w[h][j] m[h][j][d] as the kernels walk it: thread quarter `part` owns the 8-token vectors at 8 part + 32 i, adds them in
    order (fp32), and the four partials are added (p0 + p1) + (p2 + p3).  w [H][Tld], m [H][Tld][64] fp32."""
    H = w.shape[0]
    parts = []
    for part in range(4):
        acc = torch.zeros(H, DH, dtype=F32)
        for j0 in range(8 * part, Tld, 32):
            for j in range(j0, j0 + 8, 2):
                acc = acc + (w[:, j, None] * m[:, j] + w[:, j + 1, None] * m[:, j + 1])
        parts.append(acc)
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def attn_fwd_emulate(qkv, H, Tld, scale=SCALE, mut=None):
    """attn_cls_fwd_kernel's roundings in torch fp32 for one pass: (probs fp32 [H][Tld], out bf16-exact fp32 [D]).
    mut: 'drop_last_key' (key T - 1 left out of the softmax) | 'pad_prob' (1e-3 at column T)."""
    q, k, v = split_heads(qkv.to(F32), H)
    T = qkv.shape[0]
    Tv = T - 1 if mut == "drop_last_key" else T
    s = _dot64_f32(k[:, :Tv], q[:, None, :]) * torch.tensor(scale, dtype=F32)
    mx = s.max(1, keepdim=True).values
    e = torch.zeros(H, Tld, dtype=F32)
    e[:, :Tv] = torch.exp2((s - mx) * torch.tensor(LOG2E, dtype=F32))
    tot = _block_sum256(_strided_thread_sums(e, Tld))
    probs = e * (torch.tensor(1.0, dtype=F32) / tot)[:, None]
    if mut == "pad_prob" and T < Tld:
        probs[:, T] = 1e-3
    vp = torch.zeros(H, Tld, DH, dtype=F32)
    vp[:, :T] = v
    out = _quarters_dot(bf16_round(probs), vp, Tld)
    return probs, bf16_round(out).reshape(-1)


def attn_bwd_emulate(qkv, H, Tld, probs32, slabs, scale=SCALE, mut=None):
    """attn_cls_bwd_kernel's roundings in torch fp32 for one pass: slabs [n][D]; returns dict dO [D], dq [D], dk, dv [T][D] (bf16-exact).
    mut: 'skip_last_slab' | 'reverse_slabs' | 'dO_unrounded' | 'delta_short' (delta without its last term)."""
    q, k, v = split_heads(qkv.to(F32), H)
    T = qkv.shape[0]
    dO = attn_dO(slabs, mut)
    dOh = dO.reshape(H, DH)
    p = probs32[:, :T].to(F32)
    dP = _dot64_f32(v, dOh[:, None, :])
    terms = p * dP
    if mut == "delta_short":
        terms = terms[:, :T - 1]
    delta = _block_sum256(_strided_thread_sums(terms, terms.shape[1]))
    ds = p * (dP - delta[:, None]) * torch.tensor(scale, dtype=F32)
    dk = bf16_round(ds[:, :, None] * q[:, None, :]).transpose(0, 1).reshape(T, -1)
    dv = bf16_round(p[:, :, None] * dOh[:, None, :]).transpose(0, 1).reshape(T, -1)
    dsp, kp = torch.zeros(H, Tld, dtype=F32), torch.zeros(H, Tld, DH, dtype=F32)
    dsp[:, :T], kp[:, :T] = bf16_round(ds), k
    return dict(dO=dO, dq=bf16_round(_quarters_dot(dsp, kp, Tld)).reshape(-1), dk=dk, dv=dv)


# ------------------------------------------------------------------------------------------------ LayerNorm of strided rows
LN_TREE = 12   # roundings of a row sum / D: at most 2 adds in a thread (three columns), 6 butterfly steps, 2 across the waves, the division: 11


def ln_case(rows, D, n_slabs, seed=1, edge=False):
    """Forward operands: gamma, beta [D]; n_slabs == 0: x [rows][D]; else bias [D], resid [rows][D], slabs [n][rows][D] (the row is formed
    from them).  edge (rows == 3, no slabs): row 0 holds 1.5 everywhere (zero variance, every partial sum exact), row 1 has mean 1e3 and
    unit deviation, row 2 is ordinary."""
    g = _gen("ln", rows, D, n_slabs, seed, int(edge))
    c = dict(gamma=1 + 0.1 * torch.randn(D, generator=g), beta=0.1 * torch.randn(D, generator=g))
    if n_slabs == 0:
        c["x"] = 0.5 + 3.0 * torch.randn(rows, D, generator=g)
        if edge:
            c["x"][0] = 1.5
            c["x"][1] = 1e3 + torch.randn(D, generator=g)
    else:
        c.update(bias=torch.randn(D, generator=g), resid=0.5 + 3.0 * torch.randn(rows, D, generator=g), slabs=torch.randn(n_slabs, rows, D, generator=g))
    return c


def ln_x_pred(c, mut=None):
    """the row ln_rows_fwd normalises, bit for bit: x itself, or (bias + resid) + s_0 + s_1 + ... in fp32"""
    if "x" in c:
        return c["x"].to(F32)
    return slab_sum_f32(c["bias"][None].to(F32) + c["resid"].to(F32), c["slabs"], mut)


def ln_fwd_ref(x, gamma, beta, eps=LN_EPS):
    """fp64 LayerNorm of x [rows][D] (an fp32-exact input) with its bounds: dict y, mean, rstd, E_y, E_mean, E_rstd.
    mean:  LN_TREE u mean|x| (the kernel's summation tree; a D-term chain is not assumed).
    rstd:  an error d of the mean adds exactly d^2 to the two-pass variance (0.5 rstd^3 d^2); the squares, their tree, the division,
           + eps and a 1-ulp rsqrt: 16 u rstd.
    y:     ((x - mean) rstd gamma + beta) in fp32: |gamma| (rstd (E_mean + u |x - mean|) + |x - mean| E_rstd) + 3 u |(x - mean) rstd gamma|
           + u |y| = e, then bf16: e + UBF (|y| + e)."""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    mean = x.mean(1, keepdim=True)
    xc = x - mean
    rstd = ((xc * xc).mean(1, keepdim=True) + eps).rsqrt()
    y = xc * rstd * gamma + beta
    E_mean = LN_TREE * U32 * x.abs().mean(1, keepdim=True)
    E_rstd = 16 * U32 * rstd + 0.5 * rstd ** 3 * E_mean ** 2
    e = gamma.abs() * (rstd * (E_mean + U32 * xc.abs()) + xc.abs() * E_rstd) + 3 * U32 * (xc * rstd * gamma).abs() + U32 * y.abs()
    return dict(y=y, mean=mean[:, 0], rstd=rstd[:, 0], E_y=e + UBF * (y.abs() + e), E_mean=E_mean[:, 0], E_rstd=E_rstd[:, 0])


def _row_sum_emulate(v):
    """sum over the columns of v [rows][D] as one workgroup per row forms it: thread t adds columns t, t + 256, t + 512, then block_sum256"""
    return _block_sum256(_strided_thread_sums(v, v.shape[1]))


def ln_fwd_emulate(c, eps=LN_EPS, mut=None):
    """ln_rows_fwd_kernel in torch fp32: (x [rows][D] as stored, y bf16-exact, mean, rstd).
    mut: 'skip_last_slab' | 'reverse_slabs' | 'ln_mean_short' (the mean's sum stops one column early)."""
    x = ln_x_pred(c, mut)
    D = x.shape[1]
    Df = torch.tensor(float(D), dtype=F32)
    mean = _row_sum_emulate(x[:, :D - 1] if mut == "ln_mean_short" else x) / Df
    d = x - mean[:, None]
    rstd = torch.rsqrt(_row_sum_emulate(d * d) / Df + torch.tensor(eps, dtype=F32))
    y = bf16_round(d * rstd[:, None] * c["gamma"].to(F32) + c["beta"].to(F32))
    return x, y, mean, rstd


def ln_bwd_case(rows, D, n_slabs, seed=1):
    """Backward operands: x, gamma, dy slabs [n][rows][D], a non-zero g on entry; mean / rstd are the fp64 reference's rounded to fp32, so the
    backward is checked independently of the forward"""
    g = _gen("lnb", rows, D, n_slabs, seed)
    x = 0.5 + 3.0 * torch.randn(rows, D, generator=g)
    f = ln_fwd_ref(x, torch.ones(D), torch.zeros(D))
    return dict(x=x, gamma=1 + 0.1 * torch.randn(D, generator=g), slabs=torch.randn(n_slabs, rows, D, generator=g) / math.sqrt(n_slabs),
                g0=torch.randn(rows, D, generator=g), mean=f["mean"].float(), rstd=f["rstd"].float())


def ln_dy_pred(c, mut=None):
    """slab 0 after ln_rows_bwd: s_0 + s_1 + ... in fp32 (the kernel starts from slab 0)"""
    return slab_sum_f32(c["slabs"][0], c["slabs"][1:], mut) if c["slabs"].shape[0] > 1 else c["slabs"][0].to(F32)


def ln_bwd_ref(c, dy):
    """fp64 g = g0 + rstd (dh - mean(dh) - xh mean(dh xh)), dh = dy gamma, xh = (x - mean) rstd, for the fp32 dy / mean / rstd given, and its
    bound: s1 = mean(dh): LN_TREE u mean|dh| + u of each product; s2 = mean(dh xh): (LN_TREE + 4) u mean|dh xh|; the bracket: the errors of
    its terms and two subtractions; the product with rstd and the add of g0: one rounding each."""
    x, gamma, dy, g0 = c["x"].double(), c["gamma"].double(), dy.double(), c["g0"].double()
    mean, rstd = c["mean"].double()[:, None], c["rstd"].double()[:, None]
    xh, dh = (x - mean) * rstd, dy * gamma
    s1, s2 = dh.mean(1, keepdim=True), (dh * xh).mean(1, keepdim=True)
    t = dh - s1 - xh * s2
    g = g0 + rstd * t
    E_s1 = (LN_TREE + 1) * U32 * dh.abs().mean(1, keepdim=True)
    E_s2 = (LN_TREE + 4) * U32 * (dh * xh).abs().mean(1, keepdim=True)
    E_t = E_s1 + xh.abs() * E_s2 + 3 * U32 * dh.abs() + 2 * U32 * s1.abs() + 5 * U32 * (xh * s2).abs()
    return g, rstd * E_t + U32 * (rstd * t).abs() + U32 * g.abs()


def ln_bwd_emulate(c, mut=None):
    """ln_rows_bwd_kernel in torch fp32: (slab 0 after the call, g, g_bf)"""
    dy = ln_dy_pred(c, mut)
    x, gamma = c["x"].to(F32), c["gamma"].to(F32)
    D = x.shape[1]
    Df = torch.tensor(float(D), dtype=F32)
    dh, xh = dy * gamma, (x - c["mean"][:, None]) * c["rstd"][:, None]
    s1 = _row_sum_emulate(dh) / Df
    s2 = _row_sum_emulate(dh * xh) / Df
    g = c["g0"].to(F32) + c["rstd"][:, None] * (dh - s1[:, None] - xh * s2[:, None])
    return dy, g, bf16_round(g)


# ------------------------------------------------------------------------------------------------ finisher of the split-K row GEMMs
def gelu64(x):
    return x * 0.5 * (1 + torch.erf(x / math.sqrt(2.0)))


def gelu_grad64(x):
    return 0.5 * (1 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)


def fin_case(rows, N, n_slabs, seed=1):
    """slabs [n][rows][N], bias [N], resid [rows][N], aux: bf16-exact pre-activations spanning [-6, 6] (both saturated branches of
    gelu_grad_f) in a fixed shuffle"""
    g = _gen("fin", rows, N, n_slabs, seed)
    aux = torch.linspace(-6, 6, rows * N)[torch.randperm(rows * N, generator=g)].reshape(rows, N)
    return dict(slabs=torch.randn(n_slabs, rows, N, generator=g), bias=torch.randn(N, generator=g), resid=torch.randn(rows, N, generator=g),
                aux=bf16_round(aux))


def fin_v_pred(c, mode, mut=None):
    """(bias + s_0) + s_1 + ... in fp32; mode 2 starts from 0"""
    start = torch.zeros_like(c["slabs"][0]) if mode == 2 else c["bias"][None].to(F32).expand_as(c["slabs"][0])
    return slab_sum_f32(start, c["slabs"], mut)


def fin_ref(c, mode, mut=None):
    """mode 0: the fp32 output predicted bit for bit.  mode 1: (gelu reference fp64, its bar, pre = bf16(v) bit for bit).  mode 2:
    (v gelu'(aux) fp64, its bar).  The bars are common.h's own for gelu_f / gelu_grad_f plus the bf16 rounding of the output."""
    v = fin_v_pred(c, mode, mut)
    if mode == 0:
        return v + c["resid"].to(F32)
    if mode == 1:
        ref = gelu64(v.double())
        return ref, GELU_ABS + UBF * ref.abs(), bf16_round(v)
    ref = v.double() * gelu_grad64(c["aux"].double())
    return ref, GELU_GRAD_REL * v.double().abs() + UBF * ref.abs()


def _cdf_poly_f32(xc):
    u = xc * xc
    p = torch.full_like(xc, 7.804400182e-11)
    for coef in (-6.827484800e-09, 2.666929504e-07, -6.221946023e-06, 9.829076589e-05, -1.130963792e-03, 9.869961999e-03, -6.640202552e-02,
                 3.989198506e-01):
        p = p * u + coef
    return xc * p + 0.5


def _gelu_grad_f32(x):
    xc = x.clamp(-4.0, 4.0)
    u = xc * xc
    p = torch.full_like(xc, -5.066447262e-11)
    for coef in (4.789254326e-09, -2.026289394e-07, 5.107016932e-06, -8.623141184e-05, 1.038558665e-03, -9.190188721e-03, 5.937872082e-02,
                 -2.656380534e-01, 7.978171706e-01):
        p = p * u + coef
    d = xc * p + 0.5
    return torch.where(x < -4.0, torch.zeros_like(x), torch.where(x > 4.0, torch.full_like(x, 0.99997), d))


def fin_emulate(c, mode, pre_lo=0, sentinel=-7.0, mut=None):
    """rows_finish_kernel in torch fp32 (common.h's polynomials without the fused multiply-adds).  mode 0: out_f32.  mode 1: (out_bf,
    pre_bf with `sentinel` in the rows the gate leaves alone).  mode 2: out_bf.
    mut: 'skip_last_slab' | 'reverse_slabs' | 'pre_lo_off_by_one' (the gate takes rows > pre_lo)."""
    v = fin_v_pred(c, mode, mut)
    if mode == 0:
        return v + c["resid"].to(F32)
    if mode == 1:
        m = v.clamp(min=-4.0)
        out = bf16_round(m * _cdf_poly_f32(m.clamp(max=4.0)))
        lo = pre_lo + 1 if mut == "pre_lo_off_by_one" else pre_lo
        pre = torch.full_like(v, sentinel)
        pre[lo:] = bf16_round(v)[lo:]
        return out, pre
    return bf16_round(v * _gelu_grad_f32(c["aux"].to(F32)))
