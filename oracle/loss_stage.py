"""fp64 references, closed forms, worst-case error bounds and an fp32 rounding emulation of the LOSS STAGE of the fused step
(test infrastructure only, torch-CPU): the structure term (``selfsim_tgt/loss/dk_kernel``), the batched MSE
(``mse_batched_kernel``) and the total (``total_loss_kernel``), as ``util/losses.py:74-105`` defines them.

The bounds are derived from the reference alone -- the precision of the number formats and the element bar ``DELTA`` that
``tests/test_ops_gpu.py::test_selfsim_fwd_bwd`` already holds S to -- never from what a kernel returns.  ``tests/test_loss_stage_cpu.py``
checks on a machine without a GPU that an fp32 emulation of the kernels' roundings stays inside them and that they sit well below the
signal; ``tests/test_loss_stage_gpu.py`` holds the kernels to them.
"""
import torch

from .extractor import attn_cosine_sim

DELTA = 2e-5          # element error of a cosine similarity from bf16 keys with fp32 accumulation
U32 = 2.0 ** -24      # unit roundoff of fp32
UBF = 2.0 ** -8       # generous for a bf16 round to nearest (2^-9)
EPS = 1e-8            # attn_cosine_sim's clamp

# the shapes and regimes of the GPU tests (the CPU test walks the same list)
STRUCT_SHAPES = [(64, 64), (65, 384), (129, 128), (197, 384)]
STRUCT_REGIMES = ["independent", "near_target"]
FP8_SHAPES = [(65, 128), (197, 384)]
LAMBDA = 10.0         # the reference's lambda_global_ssim


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def tld(T):
    """Row pitch of a pass in the ViT engine's token matrices."""
    return (T + 31) // 32 * 32


# ------------------------------------------------------------------------------------------------ cases
def structure_case(T, D, regime, seed, zero_row=True):
    """(Kt, Kx): bf16-exact fp32 [T][D] target / generated keys.  independent: two draws with per-row scale 1 + |N(0,1)|;
    near_target: Kx = bf16(Kt + 0.05 N), the cancellation the real step lives in.  T > 64: one all-zero row in Kx."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * T + D)
    Kt = bf16_round(torch.randn(T, D, generator=g) * (1 + torch.randn(T, 1, generator=g).abs()))
    if regime == "independent":
        Kx = bf16_round(torch.randn(T, D, generator=g) * (1 + torch.randn(T, 1, generator=g).abs()))
    elif regime == "near_target":
        Kx = bf16_round(Kt + 0.05 * torch.randn(T, D, generator=g))
    else:
        raise ValueError(regime)
    if zero_row and T > 64:
        Kx[T // 3] = 0
    return Kt, Kx


def _e4m3_values():
    """the normal e4m3fn magnitudes in [16, 448]"""
    return torch.tensor([(8 + m) / 8 * 2.0 ** e for e in range(4, 9) for m in range(8) if (8 + m) / 8 * 2.0 ** e <= 448.0])


def fp8_case(T, D, seed):
    """(Kt, Kx) whose per-row e4m3 quantisation is exact: every entry is an e4m3 value times the row's 2^k (k in -3..3), one entry
    per row is +-448 * 2^k -- so amax = 448 * 2^k, the quantiser's 448 / amax = 2^-k and x * 2^-k is the e4m3 value itself.  Kx is Kt
    with a quarter of the entries and every row scale redrawn (no zero row: the quantiser at amax = 0 is not this module's subject)."""
    g = torch.Generator().manual_seed(2000 * seed + 7 * T + D)
    vals = _e4m3_values()

    def draw():
        v = vals[torch.randint(len(vals), (T, D), generator=g)]
        return v * (torch.randint(2, (T, D), generator=g) * 2 - 1).float()

    def finish(q):
        q = q.clone()
        col = torch.randint(D, (T,), generator=g)
        sign = (torch.randint(2, (T,), generator=g) * 2 - 1).float()
        q[torch.arange(T), col] = 448.0 * sign
        k = torch.randint(-3, 4, (T, 1), generator=g).float()
        out = q * 2.0 ** k
        assert torch.equal(bf16_round(out), out)
        return out

    qt = draw()
    qx = torch.where(torch.rand(T, D, generator=g) < 0.25, draw(), qt)
    return finish(qt), finish(qx)


# ------------------------------------------------------------------------------------------------ structure term
def _cos(K, eps):
    return attn_cosine_sim(K[None, None], eps)[0]


def structure_ref(Kx, Kt, lam=LAMBDA, eps=EPS):
    """fp64 autograd of ``lam * mean((cos(Kx) - cos(Kt))^2)`` (util/losses.py:74-83).  Returns (loss, dKx)."""
    leaf = Kx.double().clone().requires_grad_(True)
    St = _cos(Kt.double(), eps)
    loss = lam * ((_cos(leaf, eps) - St) ** 2).mean()
    loss.backward()
    return loss.item(), leaf.grad


def structure_closed_form(Kx, Kt, lam=LAMBDA, eps=EPS):
    """What the kernels compute, in fp64: with d = S - S*, E = dS + dS^T = 4 lam d / T^2, c = max(n_i n_j, eps):
    W = E / c, r_i = sum_j [n_i n_j > eps] E_ij S_ij / max(n_i^2, 1e-30), dK = W K - diag(r) K.  Returns a dict."""
    K = Kx.double()
    T = K.shape[0]
    n = K.norm(dim=1)
    nn = n[:, None] * n[None, :]
    c = nn.clamp(min=eps)
    S = (K @ K.T) / c
    d = S - _cos(Kt.double(), eps)
    E = 4.0 * lam * d / (T * T)
    W = E / c
    r = ((nn > eps) * E * S).sum(1) / (n * n).clamp(min=1e-30)
    return dict(loss=lam * (d * d).mean().item(), dK=W @ K - r[:, None] * K, W=W, r=r, d=d, c=c, nn=nn, n=n, S=S)


def dk_bound(K, W, We_w, We_r, nn, n):
    """Element bound of dK = W K - diag(r) K: bf16 storage of W; an error We_w of W itself; an error sum_j (We_r * nn)_ij / n_i^2 of r."""
    Ka = K.double().abs()
    return UBF * (W.abs() @ Ka) + We_w @ Ka + ((We_r * nn).sum(1) / (n * n).clamp(min=1e-30))[:, None] * Ka


def structure_bounds(Kx, Kt, lam=LAMBDA, eps=EPS, delta=DELTA):
    """(loss bound, dK element bound [T][D]) for S and S* each known to `delta`:
    loss: lam / T^2 * sum(2 |d| delta + delta^2);
    dK_ij: 2^-8 (|W| |K|)_ij + (We |K|)_ij + 2 sum_j (We nn)_i / max(n_i^2, 1e-30) |K_ij|, We = 4 lam delta / (T^2 c)."""
    cf = structure_closed_form(Kx, Kt, lam, eps)
    T = Kx.shape[0]
    loss_b = lam / (T * T) * (2 * cf["d"].abs() * delta + delta * delta).sum().item()
    We = 4.0 * lam * delta / (T * T * cf["c"])
    return loss_b, dk_bound(Kx, cf["W"], We, 2 * We, cf["nn"], cf["n"])


def selfsim_bwd_closed_form(K, dS, eps=EPS, delta=DELTA):
    """The unfused public op (splice_keys_selfsim_bwd) for a GIVEN dS: (S, dK, dK element bound), fp64.  W = (dS + dS^T) / c carries
    no S error here; r does: |E_ij| delta per term."""
    K = K.double()
    n = K.norm(dim=1)
    nn = n[:, None] * n[None, :]
    c = nn.clamp(min=eps)
    S = (K @ K.T) / c
    E = dS.double() + dS.double().T
    W = E / c
    r = ((nn > eps) * E * S).sum(1) / (n * n).clamp(min=1e-30)
    return S, W @ K - r[:, None] * K, dk_bound(K, W, torch.zeros_like(W), delta * W.abs(), nn, n)


def structure_emulate_fp32(Kx, Kt, lam=LAMBDA, eps=EPS):
    """The kernels' roundings restated in fp32 torch-CPU: fp32 Gram and norms, S = G / max(nn, eps), e = e_scale * d with the step's
    fp32 e_scale, W stored in bf16, r gated by nn > eps, dK = W K - r K in fp32.  Returns (loss [lam applied in fp64], dK)."""
    f = torch.float32
    K, Kt = Kx.to(f), Kt.to(f)
    T = K.shape[0]

    def cos(M):
        n = (M * M).sum(1).sqrt()
        nn = n[:, None] * n[None, :]
        return (M @ M.T) / nn.clamp(min=eps), nn, n

    S, nn, n = cos(K)
    St = cos(Kt)[0]
    loss_scale = torch.tensor(1.0, dtype=f) / (torch.tensor(float(T), dtype=f) * torch.tensor(float(T), dtype=f))
    e_scale = torch.tensor(4.0, dtype=f) * torch.tensor(lam, dtype=f) * loss_scale
    d = S - St
    loss = ((d * d).sum() * loss_scale).double().item() * lam
    e = e_scale * d
    W = bf16_round(e / nn.clamp(min=eps))
    r = torch.where(nn > eps, e * S, torch.zeros_like(S)).sum(1) / (n * n).clamp(min=1e-30)
    return loss, (W @ K - r[:, None] * K).double()


# ------------------------------------------------------------------------------------------------ batched MSE
MSE_GRAD_REL = 4 * U32    # d = a - b, 2 * gmean, times d: three fp32 roundings (and gmean's own division)
MSE_LOSS_REL = 16 * U32   # non-negative terms: 3 roundings per term + the longest add chain (2 per thread, 6 in the wave, 2 across waves)
MSE_MAX_WG = 1024         # SPLICE_MSE_PARTIALS


def mse_ref(a, b, loss_weight, gmean):
    """fp64: per-workgroup loss partials as the header documents them -- workgroup w of g = min(ceil(n / 256), 1024) owns the flat
    elements i with (i // 256) % g == w; partial = loss_weight / n * sum d^2 -- and grad = 2 gmean d.  a, b: [rows][cols] views."""
    d = a.double() - b.double()
    n = d.numel()
    g = min((n + 255) // 256, MSE_MAX_WG)
    flat = torch.zeros(-(-n // (256 * g)) * 256 * g, dtype=torch.float64)
    flat[:n] = (d * d).reshape(-1)
    part = flat.reshape(-1, g, 256).sum((0, 2)) * (loss_weight / n)
    return part, 2.0 * gmean * d


def mse_emulate_fp32(a, b, loss_weight, gmean):
    f = torch.float32
    d = a.to(f) - b.to(f)
    n = d.numel()
    g = min((n + 255) // 256, MSE_MAX_WG)
    flat = torch.zeros(-(-n // (256 * g)) * 256 * g, dtype=f)
    flat[:n] = (d * d).reshape(-1)
    wmean = torch.tensor(loss_weight, dtype=f) / torch.tensor(float(n), dtype=f)
    part = flat.reshape(-1, g, 256).sum((0, 2)) * wmean
    return part.double(), (torch.tensor(2.0, dtype=f) * torch.tensor(gmean, dtype=f) * d).double()


# ------------------------------------------------------------------------------------------------ total
# term k of the slot layout -> (index of its weight in (w_ssim, w_essim, w_ecls, w_cls, w_id), which slot count it uses)
TOTAL_TERMS = {1: (0, "a"), 2: (1, "e"), 3: (2, "e"), 4: (3, "c"), 5: (4, "b")}


def total_weights(pair, weights, wtab, ssim_on, entire):
    """the five weights (w_ssim, w_essim, w_ecls, w_cls, w_id) of a pair; wtab rows are {cls, ssim, id, ecls, essim}"""
    if wtab is None:
        return [float(w) for w in weights]
    w = [float(x) for x in wtab[pair]]
    return [w[1] if ssim_on else 0.0, w[4] if entire else 0.0, w[3] if entire else 0.0, w[0], w[2] if ssim_on else 0.0]


def total_ref(buf, lstride, lp, pairs, n, weights, wtab=None, ssim_on=1, entire=1):
    """fp64 reference of total_loss_kernel on a flat partials buffer: term k's partials of a slot start at 8 + k * lp, pair p's slots of
    a term are the n[...] consecutive slots from p * n[...].  n = dict(a=, b=, c=, e=).  Returns (out8 [pairs][8], bound [pairs][8]):
    |err raw_k| <= lp * 2^-24 * sum|partials| (the add chain is ceil(lp / 64) + 6 + slots <= lp long), and the total adds
    sum |w_k| bound_k + 6 * 2^-24 * sum |w_k raw_k| (one product and four adds per term)."""
    buf = buf.double()
    out = torch.zeros(pairs, 8, dtype=torch.float64)
    bound = torch.zeros(pairs, 8, dtype=torch.float64)
    for p in range(pairs):
        w = total_weights(p, weights, wtab, ssim_on, entire)
        for k, (wi, which) in TOTAL_TERMS.items():
            ns = n[which]
            parts = torch.cat([buf[(p * ns + s) * lstride + 8 + k * lp:(p * ns + s) * lstride + 8 + (k + 1) * lp] for s in range(ns)])
            out[p, k] = parts.sum()
            bound[p, k] = lp * U32 * parts.abs().sum()
            out[p, 0] += w[wi] * out[p, k]
            bound[p, 0] += abs(w[wi]) * bound[p, k] + 6 * U32 * abs(w[wi] * out[p, k])
    return out, bound


def total_emulate_fp32(buf, lstride, lp, pairs, n, weights, wtab=None, ssim_on=1, entire=1):
    """the kernel's sums in fp32: 64 strided lane sums, a butterfly over the lanes, slots added in order, the total left to right"""
    f = torch.float32
    buf = buf.to(f)
    out = torch.zeros(pairs, 8, dtype=f)
    for p in range(pairs):
        w = [torch.tensor(x, dtype=f) for x in total_weights(p, weights, wtab, ssim_on, entire)]
        for k, (wi, which) in TOTAL_TERMS.items():
            ns = n[which]
            tot = torch.tensor(0.0, dtype=f)
            for s in range(ns):
                part = buf[(p * ns + s) * lstride + 8 + k * lp:(p * ns + s) * lstride + 8 + (k + 1) * lp]
                lanes = torch.zeros(-(-lp // 64) * 64, dtype=f)
                lanes[:lp] = part
                acc = torch.zeros(64, dtype=f)
                for row in lanes.reshape(-1, 64):
                    acc = acc + row
                while acc.numel() > 1:
                    acc = acc[:acc.numel() // 2] + acc[acc.numel() // 2:]
                tot = tot + acc[0]
            out[p, k] = tot
        out[p, 0] = (((w[0] * out[p, 1] + w[1] * out[p, 2]) + w[2] * out[p, 3]) + w[3] * out[p, 4]) + w[4] * out[p, 5]
    return out.double()
