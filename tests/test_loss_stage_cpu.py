"""CPU: the references and the derived bounds of oracle/loss_stage.py, which tests/test_loss_stage_gpu.py and the self-similarity
cases of tests/test_ops_gpu.py hold the HIP kernels to.  Three things, at every shape the GPU tests use:
  * the closed form the kernels restate (dK = W K - diag(r) K with the nn > eps gate) equals fp64 autograd, zero row included;
  * an fp32 emulation of the kernels' roundings (W in bf16 included) stays inside every bound;
  * the bounds bite: the median |dK| / bound is above 2, so a structural mistake (O(1) on the elements it touches) fails.
"""
import pytest
import torch

from oracle import loss_stage as ls

STRUCT_CASES = [(T, D, regime) for T, D in ls.STRUCT_SHAPES for regime in ls.STRUCT_REGIMES]


def _struct_keys(T, D, regime):
    return ls.fp8_case(T, D, 1) if regime == "fp8" else ls.structure_case(T, D, regime, 1)


@pytest.mark.parametrize("T,D,regime", STRUCT_CASES + [(T, D, "fp8") for T, D in ls.FP8_SHAPES])
def test_structure_closed_form_emulation_and_bounds(T, D, regime):
    Kt, Kx = _struct_keys(T, D, regime)
    if regime != "fp8" and T > 64:
        assert (Kx == 0).all(1).sum().item() == 1          # the zero row is there
    loss, dK = ls.structure_ref(Kx, Kt)
    cf = ls.structure_closed_form(Kx, Kt)
    assert abs(cf["loss"] - loss) <= 1e-12 * abs(loss)
    assert (cf["dK"] - dK).abs().max().item() <= 1e-10 * dK.abs().max().item()
    assert torch.isfinite(dK).all()
    loss_b, dk_b = ls.structure_bounds(Kx, Kt)
    e_loss, e_dK = ls.structure_emulate_fp32(Kx, Kt)
    assert abs(e_loss - loss) <= loss_b, (abs(e_loss - loss), loss_b)
    ratio = ((e_dK - dK).abs() / dk_b.clamp(min=1e-300)).max().item()
    signal = (dK.abs() / dk_b.clamp(min=1e-300)).median().item()
    normwise = ((e_dK - dK).norm() / dK.norm()).item()
    print(f"T={T} D={D} {regime}: emulation err/bound {ratio:.3f}, median |dK|/bound {signal:.2f}, norm-wise {normwise:.2e}, "
          f"loss err/bound {abs(e_loss - loss) / loss_b:.3f}")
    assert ratio <= 1.0, ratio
    assert signal > 2.0, signal
    assert normwise < 1e-2, normwise
    # the loss bound bites too: one of the (at most 10) tiles lost or doubled moves the loss by far more
    assert loss_b < 0.01 * loss, (loss_b, loss)


@pytest.mark.parametrize("T,D", [(64, 64), (65, 384)])
def test_unfused_backward_closed_form_and_bound(T, D):
    """the form tests/test_ops_gpu.py uses for splice_keys_selfsim_bwd: a given, non-symmetric dS and a zero row"""
    from oracle.extractor import attn_cosine_sim
    g = torch.Generator().manual_seed(5 + T)
    K = ls.bf16_round(torch.randn(T, D, generator=g) * (1 + torch.randn(T, 1, generator=g).abs()))
    K[T // 3] = 0
    dS = torch.randn(T, T, generator=g)
    leaf = K.double().clone().requires_grad_(True)
    S_ref = attn_cosine_sim(leaf[None, None])[0]
    S_ref.backward(dS.double())
    S, dK, bound = ls.selfsim_bwd_closed_form(K, dS)
    assert (S - S_ref).abs().max().item() < 1e-12
    assert (dK - leaf.grad).abs().max().item() <= 1e-10 * leaf.grad.abs().max().item()
    assert (leaf.grad.abs() / bound.clamp(min=1e-300)).median().item() > 2.0


MSE_CASES = [(1, 384), (65, 384), (700, 384)]


@pytest.mark.parametrize("rows,cols", MSE_CASES)
def test_mse_emulation_inside_bounds(rows, cols):
    g = torch.Generator().manual_seed(rows)
    a, b = torch.randn(rows, cols, generator=g), torch.randn(rows, cols, generator=g)
    gmean = float(torch.tensor(10.0) / torch.tensor(float(rows * cols)))
    part, grad = ls.mse_ref(a, b, 1.0, gmean)
    e_part, e_grad = ls.mse_emulate_fp32(a, b, 1.0, gmean)
    assert part.numel() == min(-(-rows * cols // 256), 1024)
    assert abs(part.sum().item() - ((a.double() - b.double()) ** 2).mean().item()) < 1e-12
    assert ((e_part - part).abs() <= ls.MSE_LOSS_REL * part).all()
    assert ((e_grad - grad).abs() <= ls.MSE_GRAD_REL * grad.abs()).all()


@pytest.mark.parametrize("lp", [70, 1024])
@pytest.mark.parametrize("mixed", [False, True])
def test_total_emulation_inside_bounds(lp, mixed):
    g = torch.Generator().manual_seed(lp)
    n = dict(a=3, b=2, c=2, e=1)
    lstride = 8 + 6 * lp + 5
    buf = torch.rand(2 * 3 * lstride, generator=g)
    if mixed:
        buf = buf - 0.5
    w = [float(torch.tensor(x)) for x in (10.0, 0.1, 3.0, 0.25, 1.0)]
    ref, bound = ls.total_ref(buf, lstride, lp, 2, n, w)
    emu = ls.total_emulate_fp32(buf, lstride, lp, 2, n, w)
    assert ((emu - ref).abs() <= bound).all(), ((emu - ref).abs() / bound.clamp(min=1e-300)).max()
    assert (ref[:, 6:] == 0).all()
    # a gate switches a term's weight off, the raw sums stay
    wtab = torch.tensor([[1.0, 10.0, 2.0, 0.5, 0.25], [0.0, 1.0, 0.0, 1.0, 1.0]])
    gated, _ = ls.total_ref(buf, lstride, lp, 2, n, w, wtab=wtab, ssim_on=0, entire=1)
    assert torch.equal(gated[:, 1:6], ref[:, 1:6])
    assert abs(gated[0, 0].item() - (0.25 * ref[0, 2] + 0.5 * ref[0, 3] + 1.0 * ref[0, 4]).item()) < 1e-9
