"""splice_vit_backward with `d_block == NULL` against the same call with an all-zero block-output seed plane, the top block's
[CLS]-only tail on.  The zero plane runs grad_stream, the three split-K [CLS]-row GEMMs of the tail with their finishing kernels and the
single-query attention backward -- all on zero gradient; NULL starts at the key gradient of the top block.  The two calls must give
the same image gradient: every finite non-zero value bit for bit; exact zeros may differ in sign (0 + (-0) = +0), which `==` does
not see.  (The fused step hands the y' chain the zero plane: dropping it there was measured slower, DESIGN.md section 8.  This
pins the equivalence the experiment rests on.)
"""
import pytest
import torch

from splice_amd import _lib, synth
from splice_amd.vit import VitContext, VitEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_null_block_seeds_equal_zero_block_seeds():
    """Depth 2, width 64, one head (the smallest the engine accepts), 32 x 32, three passes of which [1, 3) carry gradients; backward of pass 1
    with the same non-zero d_keys, once with an all-zero d_block[L-1] and once with d_block == NULL."""
    patch, dim, depth, heads, B, H = 8, 64, 2, 1, 3, 32
    sd = synth.vit_params(11, patch=patch, dim=dim, depth=depth, img_size=H, w_std=0.05)
    eng = VitEngine(patch=patch, dim=dim, depth=depth, heads=heads).load_state_dict(sd)
    ctx = VitContext(eng, B, H, H, True)
    lib = _lib.lib()
    _lib.check(lib.splice_vit_ctx_set_top_cls_only(ctx.handle, 1))
    imgs = torch.from_numpy(synth.uniform(12, "seeds/img", (B, 3, H, H))).to(DEV)
    _lib.check(lib.splice_vit_forward_ex(ctx.handle, _lib.ptr(imgs), 1, 1, _lib.current_stream()), "vit_forward_ex")
    T, Tld = ctx.T, ctx.Tld
    dk = torch.zeros(B, Tld, dim, device=DEV)
    dk[:, :T] = torch.from_numpy(synth.normal(13, "seeds/dk", (B, T, dim))).to(DEV)   # rows of padding tokens carry zero gradient
    zeros = torch.zeros(B, Tld, dim, device=DEV)
    d_zero = ctx.backward(1, 2, {depth - 1: zeros}, None, {depth - 1: dk}, normalize=True)
    d_null = ctx.backward(1, 2, None, None, {depth - 1: dk}, normalize=True)
    torch.cuda.synchronize()
    assert d_zero[1].abs().max().item() > 0.0 and d_null[1].abs().max().item() > 0.0
    assert torch.isfinite(d_zero).all() and torch.isfinite(d_null).all()
    assert bool((d_zero == d_null).all()), (d_zero - d_null).abs().max().item()
    # the other passes are not written by either call
    assert d_zero[0].abs().max().item() == 0.0 and d_zero[2].abs().max().item() == 0.0
    assert d_null[0].abs().max().item() == 0.0 and d_null[2].abs().max().item() == 0.0
