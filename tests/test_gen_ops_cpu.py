"""CPU: the references, emulations and derived bounds of oracle/gen_ops.py, which tests/test_gen_ops_gpu.py holds the generator's kernels to
(splice_amd/csrc/gen_conv.hip, gen_wgrad.hip, gen_bn.hip, gen_pointwise.hip).  At every case of the GPU test, without a GPU:
  1. the form the case is named for is the one the restated launch policy gives;
  2. the fp32 emulation stays inside every bound in two summation orders (one of them the kernels' chunking: split-K slices, segments,
     weight-gradient chunks);
  3. each deliberate error of the emulation -- a dropped border tap, a reflected index off by one, the last ragged chunk / segment / slice
     skipped, rstd from the unbiased variance, a missing mean(dz) term, the adjoint's 3/4 and 1/4 exchanged at a border, a slab added twice,
     accumulate ignored -- pushes at least one element outside its bound (where the error is larger than the bound can be at all: the
     unbiased variance of n values changes rstd by 1 / (2 n), which falls below fp32's own rounding on the largest planes);
  4. the share of BatchNorm pre-activations inside their own forward bound stays under SIGN_SHARE_CAP for the chosen inputs;
  5. the closed forms the bounds are built on are fp64 autograd.
The norm-wise size of every bound relative to its reference is printed (`GEN_OPS_CPU ...`); no bar is set for it.
"""
import pytest
import torch

from oracle import gen_ops as go


def _ratio(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


def _nw(bound, ref):
    return (bound.norm() / ref.norm().clamp(min=1e-300)).item()


# ------------------------------------------------------------------------------------------------ convolutions
@pytest.mark.parametrize("c", go.CONV_CASES + go.ARENA_CASES, ids=repr)
def test_conv_emulation_bounds_and_mutations(c):
    form = go.conv_policy(c)
    assert c.form is None or form == c.form, (c, form, c.form)
    d = go.conv_inputs(c)
    r = go.conv_ref(c, d)
    E = go.conv_bound(c, r, form)
    Ho, Wo = c.out_hw
    pix = go.emu_pixels(Ho * Wo, Wo)
    ref, Ep = r["ref"].reshape(c.N, c.Cout, -1)[:, :, pix], E.reshape(c.N, c.Cout, -1)[:, :, pix]
    if not c.big and not c.act and not c.accumulate:   # the reduction the emulation walks is the reference's (fp64 matrix product of the same columns)
        cols, wmat = go.conv_cols(c, d["inp"])
        for n in range(c.N):
            mm = wmat(d["w"][c.arena_of(n)]).double() @ cols[n].double()
            if d["bias"] is not None:
                mm = mm + d["bias"][c.arena_of(n)].double()[:, None]
            assert (mm - r["ref"][n].reshape(c.Cout, -1)).abs().max() < 1e-11
    worst = [_ratio((go.conv_emulate(c, d, form, order) - ref).abs(), Ep) for order in ("kernel", "reverse")]
    assert max(worst) <= 1.0, (c, worst)
    caught = {m: _ratio((go.conv_emulate(c, d, form, "kernel", m) - ref).abs(), Ep) for m in go.conv_mutations(c, form)}
    print(f"GEN_OPS_CPU conv {c}: form {form}, emulation err/bound {worst[0]:.3f} / {worst[1]:.3f}, bound/ref {_nw(E, r['ref']):.2e}, mutations {caught}")
    assert all(v > 1.0 for v in caught.values()), (c, caught)


@pytest.mark.parametrize("c", go.REFLECT_DGRAD_CASES, ids=repr)
def test_reflect_dgrad_emulation_bounds_and_mutations(c):
    d = go.conv_inputs(c)
    r = go.conv_ref(c, d)
    E = go.conv_bound(c, r, (0, 4, 1, 1, 1), fold=True)
    worst = [_ratio((go.reflect_dgrad_emulate(c, d, order) - r["ref"]).abs(), E) for order in ("kernel", "reverse")]
    assert max(worst) <= 1.0, (c, worst)
    muts = ["drop_border_tap", "skip_last_chunk", "reflect_off_by_one"] + (["accumulate_ignored"] if c.accumulate else [])
    caught = {m: _ratio((go.reflect_dgrad_emulate(c, d, "kernel", m) - r["ref"]).abs(), E) for m in muts}
    print(f"GEN_OPS_CPU reflect_dgrad {c}: emulation err/bound {worst[0]:.3f} / {worst[1]:.3f}, bound/ref {_nw(E, r['ref']):.2e}, mutations {caught}")
    assert all(v > 1.0 for v in caught.values()), (c, caught)


# ------------------------------------------------------------------------------------------------ weight gradients
@pytest.mark.parametrize("c", go.WGRAD_CASES, ids=repr)
def test_wgrad_emulation_bounds_and_mutations(c):
    assert go.wgrad_form(c) == c.wform, (c, go.wgrad_form(c), c.wform)
    d = go.wgrad_inputs(c)
    r = go.wgrad_ref(c, d)
    worst = [_ratio((go.wgrad_emulate(c, d, order).double() - r["ref"]).abs(), r["E"]) for order in ("chunks", "flat")]
    assert max(worst) <= 1.0, (c, worst)
    caught = {m: _ratio((go.wgrad_emulate(c, d, "chunks", m).double() - r["ref"]).abs(), r["E"]) for m in go.wgrad_mutations(c)}
    print(f"GEN_OPS_CPU wgrad {c}: form {c.wform}, emulation err/bound {worst[0]:.3f} / {worst[1]:.3f}, bound/ref {_nw(r['E'], r['ref']):.2e}, mutations {caught}")
    assert all(v > 1.0 for v in caught.values()), (c, caught)


# ------------------------------------------------------------------------------------------------ BatchNorm
def _fwd_worst(f, m, r, o):
    return max(_ratio((m.double() - f["mean"]).abs(), f["E_mean"]), _ratio((r.double() - f["rstd"]).abs(), f["E_rstd"]), _ratio((o.double() - f["out"]).abs(), f["E_out"]))


def _bwd_worst(b, dy, dg, db, amb=None):
    return max(go.bn_dy_ratio(dy, b, amb), _ratio((dg.double() - b["dgamma"]).abs(), b["E_dgamma"]), _ratio((db.double() - b["dbeta"]).abs(), b["E_dbeta"]))


@pytest.mark.parametrize("c", go.BN_CASES, ids=repr)
def test_bn_emulation_bounds_and_mutations(c):
    assert c.form[0] == c.kind, (c, c.form)
    d = go.bn_inputs(c)
    p = go.bn_problem(c, d)
    f, y32 = p["fwd"], p["y32"]
    share = (f["t"].abs() < f["E_t"]).double().mean(2).max().item()
    assert share <= go.SIGN_SHARE_CAP, (c, share)
    worst = [_fwd_worst(f, *go.bn_fwd_emulate(c, y32, d["gamma"], d["beta"], order=o)) for o in ("segments", "flat")]
    assert max(worst) <= 1.0, (c, worst)
    caught = {}
    n = len(c.groups[0]) * c.HW
    if n > 1 and 1.0 / (2 * (n - 1)) > 2 * (f["E_rstd"] / f["rstd"]).max().item():
        caught["unbiased_var"] = _fwd_worst(f, *go.bn_fwd_emulate(c, y32, d["gamma"], d["beta"], mut="unbiased_var"))
    if go.bn_skip_tail(c, c.HW) is not None:
        caught["skip_tail"] = _fwd_worst(f, *go.bn_fwd_emulate(c, y32, d["gamma"], d["beta"], mut="skip_tail"))
    if c.slabs:
        y2 = go.slab_sum_f32(p["slab_start"], d["slabs"], twice=True)
        caught["slab_twice"] = _fwd_worst(f, *go.bn_fwd_emulate(c, y2, d["gamma"], d["beta"]))
    # backward on the saved fp32 statistics and the stored activation of the reference forward
    b, amb, prev = p["bwd"], p["amb"], p["prev"]
    args = (p["da32"], p["pos"], p["y_in"], p["m32"], p["r32"], d["gamma"])
    wb = [_bwd_worst(b, *go.bn_bwd_emulate(c, *args, order=o, prev=prev), amb) for o in ("segments", "flat")]
    assert max(wb) <= 1.0, (c, wb)
    bc = {"missing_mean_dz": _bwd_worst(b, *go.bn_bwd_emulate(c, *args, mut="missing_mean_dz", prev=prev), amb)}
    if go.bn_skip_tail(c, c.HW) is not None:
        bc["skip_tail"] = _bwd_worst(b, *go.bn_bwd_emulate(c, *args, mut="skip_tail", prev=prev), amb)
    if c.acc:
        bc["accumulate_ignored"] = _bwd_worst(b, *go.bn_bwd_emulate(c, *args, mut="accumulate_ignored", prev=prev), amb)
    if c.da_slabs:
        k, acc = c.da_slabs
        da2 = go.slab_sum_f32(torch.zeros_like(d["da"]), d["da_slabs"], twice=True)
        da2 = d["da"] + da2 if acc else da2
        bc["slab_twice"] = _bwd_worst(b, *go.bn_bwd_emulate(c, da2, *args[1:], prev=prev), amb)
        if acc:
            da3 = go.slab_sum_f32(torch.zeros_like(d["da"]), d["da_slabs"])
            bc["accumulate_ignored_slabs"] = _bwd_worst(b, *go.bn_bwd_emulate(c, da3, *args[1:], prev=prev), amb)
    print(f"GEN_OPS_CPU bn {c}: form {c.form}, forward emulation err/bound {worst[0]:.3f} / {worst[1]:.3f}, bound/ref out {_nw(f['E_out'], f['out']):.2e}, "
          f"mutations {caught}; backward {wb[0]:.3f} / {wb[1]:.3f}, bound/ref dy {_nw(b['E_dy'], b['dy']):.2e}, mutations {bc}; sign-ambiguous share {share:.1e}")
    assert all(v > 1.0 for v in caught.values()) and all(v > 1.0 for v in bc.values()), (c, caught, bc)


@pytest.mark.parametrize("name", ["small_257_batch2_N4_arenas", "small_4_N2_shared", "mid_4097"])
def test_bn_closed_form_is_autograd(name):
    c = {c.name: c for c in go.BN_CASES}[name]
    d = go.bn_inputs(c)
    y = d["y"].double().requires_grad_(True)
    ga, be = d["gamma"].double().requires_grad_(True), d["beta"].double().requires_grad_(True)
    f = go.bn_fwd_ref(c, y, ga, be)
    gy, gg, gb = torch.autograd.grad(f["out"], (y, ga, be), d["da"].double())
    b = go.bn_bwd_ref(c, d["da"], f["out"].detach() > 0, d["y"], f["mean"].detach(), f["rstd"].detach(), d["gamma"])
    assert (gy - b["dy"]).abs().max() < 1e-10 * gy.abs().max()
    assert (gg.reshape(b["dgamma"].shape) - b["dgamma"]).abs().max() < 1e-10 * gg.abs().max()
    assert (gb.reshape(b["dbeta"].shape) - b["dbeta"]).abs().max() < 1e-10 * gb.abs().max()


# ------------------------------------------------------------------------------------------------ pointwise
@pytest.mark.parametrize("h,w,Ho,Wo", go.UP_CASES)
def test_upsample_emulation_bounds_and_mutations(h, w, Ho, Wo):
    x, dout = go.up_inputs(h, w, Ho, Wo)
    ref, E = go.up_ref(x.double(), Ho, Wo), go.up_bound(x, Ho, Wo)
    worst = [_ratio((go.up_emulate(x, Ho, Wo, o).double() - ref).abs(), E) for o in ("kernel", "columns")]
    aref, AE = go.up_adjoint_ref(dout, h, w), go.up_adjoint_bound(dout, h, w)
    wa = [_ratio((go.up_adjoint_emulate(dout, h, w, o).double() - aref).abs(), AE) for o in ("kernel", "autograd")]
    assert max(worst) <= 1.0 and max(wa) <= 1.0, (worst, wa)
    caught = None
    if h * w > 1:   # (a 1 x 1 source has no 1/4 tap to exchange)
        caught = _ratio((go.up_adjoint_emulate(dout, h, w, "kernel", "swap_border_weights").double() - aref).abs(), AE)
        assert caught > 1.0
    print(f"GEN_OPS_CPU upsample2x {h}x{w} -> {Ho}x{Wo}: forward {worst[0]:.3f} / {worst[1]:.3f}, bound/ref {_nw(E, ref):.2e}; adjoint {wa[0]:.3f} / {wa[1]:.3f}, "
          f"bound/ref {_nw(AE, aref):.2e}, swapped border weights {caught}")


@pytest.mark.parametrize("HW,N,group", [(HW, N, grp) for HW in go.SIGMOID_HW for N, grp in go.SIGMOID_BATCHES])
def test_sigmoid_bwd_emulation_bounds_and_mutations(HW, N, group):
    dout, s = go.sigmoid_inputs(HW, N, group)
    segs = go.sigmoid_bias_segments(N, HW, group)
    ref, E = go.sigmoid_bwd_ref(dout, s)
    pref, PE = go.sigmoid_bias_ref(ref, segs)
    for order in ("kernel", "flat"):
        dpre, parts = go.sigmoid_bwd_emulate(dout, s, segs, order)
        assert _ratio((dpre.double() - ref).abs(), E) <= 1.0 and _ratio((parts.double() - pref).abs(), PE) <= 1.0
    if len(segs) > (N // group if group else 1):
        _, parts = go.sigmoid_bwd_emulate(dout, s, segs, "kernel", "skip_last_segment")
        assert _ratio((parts.double() - pref).abs(), PE) > 1.0
    print(f"GEN_OPS_CPU sigmoid_bwd_bias HW {HW} N {N} group {group}: bound/ref dpre {_nw(E, ref):.2e}, partials {_nw(PE, pref):.2e}")
