"""CPU: the references, predictions and derived bounds of oracle/cls_tail.py, which tests/test_cls_tail_gpu.py holds the [CLS]-tail kernels
of the top ViT block to (splice_amd/csrc/vit_cls.hip).  At every case of the GPU test, without a GPU:
  1. the unmodified fp32 emulation of the kernels' roundings stays inside every bound and meets every bit-exact prediction;
  2. every bound is small against the signal: norm-wise under 1e-2 of the reference (the figure tests/test_loss_stage_gpu.py holds dK to);
  3. each deliberate small error of the emulation -- key T-1 dropped from the softmax, a probability of 1e-3 at column T, slab n-1 left out,
     slabs added in reverse order, dO not rounded to bf16, delta without its last term, the LayerNorm mean over D-1 columns, the pre_lo
     gate off by one row -- pushes at least one element outside its bound or breaks a bit-exact prediction.
The closed forms the bounds are built on are checked against fp64 autograd on the way.
"""
import pytest
import torch

from oracle import cls_tail as ct

NORMWISE = 1e-2


def _ratio(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


def _normwise(bound, ref):
    return (bound.norm() / ref.norm()).item()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ single-query attention
@pytest.mark.parametrize("T,Tld,D,H,B,regime", ct.ATTN_CASES)
def test_attention_emulation_bounds_and_mutations(T, Tld, D, H, B, regime):
    qkv_all = ct.attn_case(T, D, H, B, regime)
    assert torch.equal(ct.bf16_round(qkv_all), qkv_all)
    for b in range(B):
        qkv = qkv_all[b]
        p, out = ct.attn_ref(qkv, H)
        if regime == "sharp" and T > 1:
            assert ((p.max(1).values - 0.9).abs() < 0.05).all(), p.max(1).values      # "about 0.9", after q went to bf16
            assert p[0].argmax().item() == T - 1
        Ep, Eout = ct.attn_fwd_bounds(qkv, H, Tld)
        probs, o = ct.attn_fwd_emulate(qkv, H, Tld)
        # 1. the emulation inside the bounds
        assert (probs[:, T:] == 0).all()
        r_p, r_o = _ratio((probs[:, :T].double() - p).abs(), Ep), _ratio((o.double() - out).abs(), Eout)
        assert r_p <= 1.0 and r_o <= 1.0, (r_p, r_o)
        # 2. the bounds against the signal
        assert _normwise(Ep, p) < NORMWISE and _normwise(Eout, out) < NORMWISE, (_normwise(Ep, p), _normwise(Eout, out))
        if T == 1:
            assert torch.equal(probs[:, 0], torch.ones(H)) and torch.equal(o, qkv[0, 2 * D:])   # exact: p = 1, out = v_0
        else:
            # 3. forward mutations
            pm, om = ct.attn_fwd_emulate(qkv, H, Tld, mut="drop_last_key")
            assert _ratio((pm[:, :T].double() - p).abs(), Ep) > 1.0
            pm, om = ct.attn_fwd_emulate(qkv, H, Tld, mut="pad_prob")
            assert (pm[:, T:] != 0).any()
        # backward: the probabilities handed over are the reference's, rounded to fp32 (independent of the forward)
        p32 = torch.zeros(H, Tld)
        p32[:, :T] = p.float()
        for n in ct.ATTN_SLABS:   # the slab sum alone decides dO: predicted for every slab count, the rest of the backward at n = 6
            slabs = ct.dout_slabs(B, D, n)[:, b]
            dO = ct.attn_dO(slabs)
            assert torch.equal(ct.bf16_round(dO), dO)
            assert not torch.equal(ct.attn_dO(slabs, "skip_last_slab"), dO) and not torch.equal(ct.attn_dO(slabs, "dO_unrounded"), dO)
        slabs = ct.dout_slabs(B, D, 6)[:, b]
        dO = ct.attn_dO(slabs)
        r = ct.attn_bwd_ref(qkv, H, dO)
        E_dk, E_dq, E_ds = ct.attn_bwd_bounds(qkv, H, Tld, dO, ct.U32 * p)
        # the closed form is fp64 autograd; the bf16 ds of dq stays inside its plain worst case
        grad = ct.attn_bwd_autograd(qkv, H, dO)
        scale = grad.abs().max().item() + 1e-300
        assert (grad[:, D:2 * D] - r["dk"]).abs().max().item() <= 1e-12 * scale
        assert (grad[0, :D] - r["dq_plain"]).abs().max().item() <= 1e-12 * scale
        assert (grad[1:, :D] == 0).all()
        dv64 = (p[:, :, None] * dO.double().reshape(H, 1, 64)).transpose(0, 1).reshape(T, D)
        assert (grad[:, 2 * D:] - dv64).abs().max().item() <= 1e-12 * scale
        _, k, _ = ct.split_heads(qkv.double(), H)
        coarse = ct.UBF * torch.einsum("ht,htd->hd", r["ds"].abs(), k.abs()).reshape(-1)
        assert ((r["dq"] - r["dq_plain"]).abs() <= coarse + 1e-300).all()
        e = ct.attn_bwd_emulate(qkv, H, Tld, p32, slabs)
        assert torch.equal(e["dO"], dO)
        assert torch.equal(_bits(e["dv"]), _bits(ct.attn_dv_pred(p32, dO, T)))
        r_dk, r_dq = _ratio((e["dk"].double() - r["dk"]).abs(), E_dk), _ratio((e["dq"].double() - r["dq"]).abs(), E_dq)
        assert r_dk <= 1.0 and r_dq <= 1.0, (r_dk, r_dq)
        if T == 1:
            assert (e["dk"] == 0).all() and (e["dq"] == 0).all() and torch.equal(e["dv"][0], dO)   # exact: dk = 0, dq = 0, dv_0 = dO
            continue
        assert _normwise(E_dk, r["dk"]) < NORMWISE and _normwise(E_dq, r["dq"]) < NORMWISE, (_normwise(E_dk, r["dk"]), _normwise(E_dq, r["dq"]))
        # 3. backward mutations
        m = ct.attn_bwd_emulate(qkv, H, Tld, p32, slabs, mut="dO_unrounded")
        assert not torch.equal(_bits(m["dv"]), _bits(ct.attn_dv_pred(p32, dO, T)))
        m = ct.attn_bwd_emulate(qkv, H, Tld, p32, slabs, mut="delta_short")
        assert max(_ratio((m["dk"].double() - r["dk"]).abs(), E_dk), _ratio((m["dq"].double() - r["dq"]).abs(), E_dq)) > 1.0


# ------------------------------------------------------------------------------------------------ LayerNorm of strided rows
def _ln_fwd_inside(c, mut=None):
    """(worst err / bound over mean, rstd, y; x prediction met) of the emulation with `mut` against the unmutated reference"""
    x_pred = ct.ln_x_pred(c)
    f = ct.ln_fwd_ref(x_pred, c["gamma"], c["beta"])
    x, y, mean, rstd = ct.ln_fwd_emulate(c, mut=mut)
    worst = max(_ratio((mean.double() - f["mean"]).abs(), f["E_mean"]), _ratio((rstd.double() - f["rstd"]).abs(), f["E_rstd"]),
                _ratio((y.double() - f["y"]).abs(), f["E_y"]))
    return worst, torch.equal(_bits(x), _bits(x_pred)), f


@pytest.mark.parametrize("n_slabs", ct.LN_FWD_SLABS)
@pytest.mark.parametrize("rows", ct.LN_ROWS)
@pytest.mark.parametrize("D", ct.LN_DIMS)
def test_ln_rows_fwd_emulation_bounds_and_mutations(D, rows, n_slabs):
    c = ct.ln_case(rows, D, n_slabs)
    worst, x_ok, f = _ln_fwd_inside(c)
    assert worst <= 1.0 and x_ok, worst
    assert _normwise(f["E_y"], f["y"]) < NORMWISE and _normwise(f["E_mean"], ct.ln_x_pred(c).double().abs().mean(1)) < NORMWISE
    assert _normwise(f["E_rstd"], f["rstd"]) < NORMWISE
    assert _ln_fwd_inside(c, "ln_mean_short")[0] > 1.0
    if n_slabs:
        assert not _ln_fwd_inside(c, "skip_last_slab")[1]
    if n_slabs >= 6 and rows * D >= 100:
        assert not _ln_fwd_inside(c, "reverse_slabs")[1]


@pytest.mark.parametrize("D", ct.LN_DIMS)
def test_ln_rows_fwd_edge_rows(D):
    """a zero-variance row (y = bf16(beta) exactly, rstd = eps^-1/2) and a row with mean 1e3 meet the same bounds, and those stay small"""
    c = ct.ln_case(3, D, 0, edge=True)
    worst, _, f = _ln_fwd_inside(c)
    assert worst <= 1.0, worst
    _, y, _, rstd = ct.ln_fwd_emulate(c)
    assert torch.equal(y[0], ct.bf16_round(c["beta"])) and abs(rstd[0].item() - 1000.0) < 1e-3
    assert _normwise(f["E_y"][1:], f["y"][1:]) < NORMWISE
    assert _ln_fwd_inside(c, "ln_mean_short")[0] > 1.0


@pytest.mark.parametrize("n_slabs", ct.LN_BWD_SLABS)
@pytest.mark.parametrize("rows", ct.LN_ROWS)
@pytest.mark.parametrize("D", ct.LN_DIMS)
def test_ln_rows_bwd_emulation_bounds_and_mutations(D, rows, n_slabs):
    c = ct.ln_bwd_case(rows, D, n_slabs)
    dy_pred = ct.ln_dy_pred(c)
    g_ref, E_g = ct.ln_bwd_ref(c, dy_pred)
    # the closed form is fp64 autograd of the LayerNorm (gamma only: beta does not reach the input gradient)
    leaf = c["x"].double().clone().requires_grad_(True)
    xc = leaf - leaf.mean(1, keepdim=True)
    yy = xc * ((xc * xc).mean(1, keepdim=True) + ct.LN_EPS).rsqrt() * c["gamma"].double()
    yy.backward(dy_pred.double())
    # (mean / rstd are handed over rounded to fp32: 2^-24 relative on them, amplified by |x - mean| rstd <= a few)
    assert ((leaf.grad + c["g0"].double()) - g_ref).abs().max().item() <= 1e-5 * g_ref.abs().max().item()
    dy, g, g_bf = ct.ln_bwd_emulate(c)
    assert torch.equal(_bits(dy), _bits(dy_pred)) and torch.equal(g_bf, ct.bf16_round(g))
    assert _ratio((g.double() - g_ref).abs(), E_g) <= 1.0
    assert _normwise(E_g, g_ref) < NORMWISE
    if n_slabs > 1:
        assert not torch.equal(_bits(ct.ln_bwd_emulate(c, "skip_last_slab")[0]), _bits(dy_pred))
    if n_slabs >= 6 and rows * D >= 100:
        assert not torch.equal(_bits(ct.ln_bwd_emulate(c, "reverse_slabs")[0]), _bits(dy_pred))


# ------------------------------------------------------------------------------------------------ finisher of the split-K row GEMMs
@pytest.mark.parametrize("n_slabs", ct.FIN_SLABS)
@pytest.mark.parametrize("rows,N", ct.FIN_SHAPES)
def test_rows_finish_emulation_bounds_and_mutations(rows, N, n_slabs):
    c = ct.fin_case(rows, N, n_slabs)
    assert c["aux"].min().item() < -4.0 and c["aux"].max().item() > 4.0
    # mode 0: bit for bit
    want = ct.fin_ref(c, 0)
    assert torch.equal(_bits(ct.fin_emulate(c, 0)), _bits(want))
    assert not torch.equal(_bits(ct.fin_emulate(c, 0, mut="skip_last_slab")), _bits(want))
    if n_slabs >= 8:
        assert not torch.equal(_bits(ct.fin_emulate(c, 0, mut="reverse_slabs")), _bits(want))
    # mode 1: GELU inside common.h's bar, the pre-activation bit for bit, the gate
    ref, bar, pre = ct.fin_ref(c, 1)
    assert _normwise(bar, ref) < NORMWISE
    for pre_lo in (0, 1, rows):
        out, pre_e = ct.fin_emulate(c, 1, pre_lo=pre_lo)
        assert _ratio((out.double() - ref).abs(), bar) <= 1.0
        assert torch.equal(pre_e[pre_lo:], pre[pre_lo:]) and (pre_e[:pre_lo] == -7.0).all()
        if pre_lo < rows:
            _, pre_m = ct.fin_emulate(c, 1, pre_lo=pre_lo, mut="pre_lo_off_by_one")
            assert not torch.equal(pre_m, pre_e)
    out_m, pre_m = ct.fin_emulate(c, 1, mut="skip_last_slab")
    assert not torch.equal(pre_m, pre) and _ratio((out_m.double() - ref).abs(), bar) > 1.0
    # mode 2
    ref, bar = ct.fin_ref(c, 2)
    assert _normwise(bar, ref) < NORMWISE
    assert _ratio((ct.fin_emulate(c, 2).double() - ref).abs(), bar) <= 1.0
    assert _ratio((ct.fin_emulate(c, 2, mut="skip_last_slab").double() - ref).abs(), bar) > 1.0
