"""GPU: the generator's kernels ONE LAUNCHER AT A TIME -- conv_launch (implicit GEMM at every channel-tile depth, fragment count and wave-group
form, split-K with and without the deferred reduction, the LDS-halo tile kernel, 5x5 / 7x7), conv_pair_launch, conv_reflect_dgrad_launch,
the weight gradients (small / big / tile class, every chunk rule, the vector and the scalar reduction), bn_fwd_launch / bn_bwd_launch in
every form of bn_form (with fused upsampling, split-K slabs in either direction, a chained skip BatchNorm, batch statistics, parameter
arenas) and the three pointwise launchers -- through the splice_gen_* test hooks, which call the engine's own launchers on the caller's
buffers.  References and every bound come from oracle/gen_ops.py: fp64 torch-CPU, worst-case element bounds derived from the reference and
fp32's unit roundoff alone (tests/test_gen_ops_cpu.py checks them, and that they bite, without a GPU).  The conditioning is that of one
operation, so the bars are ~1e-5 of the signal instead of the 1e-1 per tensor of the whole-net gradient tests.

Every output and scratch buffer is prefilled with a NaN payload and has guard floats in front, behind and in the gaps of strided layouts;
they are asserted untouched.  rc == 0 and the REPORTED form are asserted: a case that silently runs another instantiation fails.  Every
case prints `GEN_OPS <case> ... err/bound`.

The two measured allowances (oracle/gen_ops.py):
  * sigmoid head (__expf, division): measured on the MI355X, worst |out - fp64| of `head_sigmoid` 8.06e-8 -- all of it inside the
    propagated pre-activation bound (excess -1.5e-7); the allowance on top of that bound is SIGMOID_ALLOW = 4 x 8.06e-8 = 3.2e-7
    (2e-5 is what the whole-net test holds the output to);
  * LeakyReLU sign of the BatchNorm backward forms that re-form the pre-activation (sign_from_y): elements inside their own forward bound
    are compared against both slopes; measured worst share of a plane 3.1e-5 (vec_65537_N2_*), cap SIGN_SHARE_CAP = 1e-3.
"""
import ctypes as C
import functools

import pytest
import torch

from oracle import gen_ops as go
from splice_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_BITS = 0x7FC0DEAD      # a quiet NaN with a payload: what the kernels must leave alone
ERR_ARG = -1               # SPLICE_ERR_ARG
GUARD = 64                 # floats in front of and behind every buffer
GAP = 7                    # floats between the channel planes of a strided (concat-style) layout
CH_OFF = 3                 # channel offset of a strided layout inside its wider buffer


def _st():
    return _lib.current_stream()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ratio(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


class Buf:
    """A device fp32 buffer of NaN payloads holding an [N][C][HW] tensor at (nstride, cstride) behind GUARD floats; everything that is not
    an element of the tensor must still be the payload after a launch."""

    def __init__(self, N, C, HW, strided=False, values=None, extra=0):
        self.N, self.C, self.HW = N, C, HW
        self.cs = HW + GAP if strided else HW
        self.ns = (C + CH_OFF + 2) * self.cs if strided else C * HW
        self.off = GUARD + (CH_OFF * self.cs if strided else 0)
        self.t = torch.full((GUARD + N * self.ns + GUARD + extra,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
        idx = (torch.arange(N)[:, None, None] * self.ns + torch.arange(C)[None, :, None] * self.cs + torch.arange(HW)[None, None, :] + self.off)
        self.idx = idx.reshape(-1).to(DEV)
        if values is not None:
            self.t[self.idx] = values.reshape(-1).to(torch.float32).to(DEV)

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr() + 4 * self.off)

    def get(self):
        return self.t[self.idx].reshape(self.N, self.C, self.HW).cpu()

    def untouched_outside(self):
        b = _bits(self.t).clone()
        b[self.idx] = NAN_BITS
        return bool((b == NAN_BITS).all())

    def all_untouched(self):
        return bool((_bits(self.t) == NAN_BITS).all())


def _flat(values=None, n=None):
    """a compact device buffer with guards: (tensor, pointer, view of the payload)"""
    n = values.numel() if values is not None else n
    t = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    if values is not None:
        t[GUARD:GUARD + n] = values.reshape(-1).to(torch.float32).to(DEV)
    return t, C.c_void_p(t.data_ptr() + 4 * GUARD), t[GUARD:GUARD + n]


def _guards_ok(t, n):
    b = _bits(t)
    return bool((b[:GUARD] == NAN_BITS).all() and (b[GUARD + n:] == NAN_BITS).all())


# ================================================================================================ convolutions
@functools.lru_cache(maxsize=None)
def _conv_ref(name):
    """inputs, fp64 reference and magnitudes of a case: computed once, shared, never modified"""
    c = {c.name: c for c in go.CONV_CASES + go.REFLECT_DGRAD_CASES + go.ARENA_CASES + PAIR_PARTS}[name]
    d = go.conv_inputs(c)
    return c, d, go.conv_ref(c, d)


def _params(c, d):
    """the parameter arenas on the device: arena a = [weights | bias | slack]; returns (tensor, w pointer, bias pointer, p_nstride)"""
    nw = d["w"][0].numel()
    pn = (nw + c.Co + 5 + 3) // 4 * 4
    host = torch.full((c.arenas, pn), float("nan"))
    host[:, :nw] = d["w"].reshape(c.arenas, -1)
    if d["bias"] is not None:
        host[:, nw:nw + c.Co] = d["bias"]
    t, p, _ = _flat(host)
    return t, p, (C.c_void_p(p.value + 4 * nw) if d["bias"] is not None else None), pn


def _conv_args(c, d, inb, outb, wp, bp, pn, ws=None, ws_floats=0, defer=0, N=None, img0=0):
    T = c.ks * c.ks
    a = _lib.GenConvArgs()
    setattr(a, "in", C.c_void_p(inb.ptr.value + 4 * img0 * inb.ns))
    a.out = C.c_void_p(outb.ptr.value + 4 * img0 * outb.ns)
    a.w, a.bias = wp, bp
    a.in_nstride, a.in_cstride, a.out_nstride, a.out_cstride = inb.ns, inb.cs, outb.ns, outb.cs
    a.w_jstride, a.w_cstride = (T, c.Ci * T) if c.transposed else (c.Ci * T, T)
    a.p_nstride = pn if c.arenas > 1 else 0
    a.p_group = c.group if c.arenas > 1 else 0
    a.N = c.N if N is None else N
    a.Cin, a.Cout = c.Cin, c.Cout
    (a.Hi, a.Wi), (a.Ho, a.Wo) = c.in_hw, c.out_hw
    a.ks, a.stride, a.pad = c.ks, c.stride, c.pad
    a.reflect, a.act, a.transposed, a.accumulate = c.reflect, c.act, c.transposed, c.accumulate
    a.ws, a.ws_floats, a.defer_reduce = ws, ws_floats, defer
    return a


def _run_conv(c, d, defer=0, reflect_dgrad=False):
    """one launch of the case on guarded buffers -> (out [N][Cout][Ho][Wo] fp32 on the host, reported form, slabs or None)"""
    (Hi, Wi), (Ho, Wo) = c.in_hw, c.out_hw
    inb = Buf(c.N, c.Cin, Hi * Wi, c.concat, d["inp"])
    outb = Buf(c.N, c.Cout, Ho * Wo, c.concat, d["prev"])
    pt, wp, bp, pn = _params(c, d)
    per = c.N * c.Cout * Ho * Wo
    ws_t = ws_p = None
    ws_floats = 0
    if c.ws:
        ws_floats = per * 16
        ws_t, ws_p, _ = _flat(n=ws_floats)
    a = _conv_args(c, d, inb, outb, wp, bp, pn, ws_p, ws_floats, defer)
    form = (C.c_int * _lib.GEN_CONV_FORM_INTS)()
    if reflect_dgrad:
        Hp, Wp = Ho + 2 * c.pad, Wo + 2 * c.pad
        sc_t, sc_p, _ = _flat(n=c.N * c.Cout * Hp * Wp)
        rc = _lib.lib().splice_gen_conv_reflect_dgrad(C.byref(a), sc_p, c.N * c.Cout * Hp * Wp, _st())
    else:
        rc = _lib.lib().splice_gen_conv(C.byref(a), form, _st())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().splice_last_error()
    assert outb.untouched_outside(), f"{c}: written outside the output planes"
    assert inb.untouched_outside() and _guards_ok(pt, c.arenas * pn)
    slabs = None
    if reflect_dgrad:
        assert _guards_ok(sc_t, c.N * c.Cout * Hp * Wp)
    if c.ws:
        k = form[4]
        assert _guards_ok(ws_t, ws_floats)
        body = _bits(ws_t[GUARD:GUARD + ws_floats])
        assert (body[k * per if k > 1 else 0:] == NAN_BITS).all(), f"{c}: split-K scratch written beyond its {k} slices"
        if k > 1:
            slabs = ws_t[GUARD:GUARD + k * per].reshape(k, c.N, c.Cout, Ho * Wo).cpu()
    out = outb.get().reshape(c.N, c.Cout, Ho, Wo)
    if defer and form[4] > 1:
        pv = d["prev"].reshape(c.N, c.Cout, Ho, Wo) if c.accumulate else None
        assert (torch.equal(out, pv) if pv is not None else outb.all_untouched()), f"{c}: the deferred reduction touched the output"
    return out, tuple(form), slabs


def _check_conv(c, d, r, out, form, fold=False, tag=""):
    assert torch.isfinite(out).all()
    E = go.conv_bound(c, r, form, fold)
    err = (out.double() - r["ref"]).abs()
    q = _ratio(err, E)
    extra = ""
    if c.act:
        s = torch.sigmoid(r["pre"])
        excess = (err - go.g(go.conv_roundings(c, form)) * r["S"] * s * (1 - s) - go.U * s).max().item()
        extra = f", sigmoid excess over the propagated bound {excess:.3e} (allowance {go.SIGMOID_ALLOW:.3e}), worst abs err {err.max().item():.3e}"
        assert go.SIGMOID_ALLOW < 2e-5
    print(f"GEN_OPS conv {c}{tag}: form (tile, CK, fn, ng, ksplit) = {form}, err/bound {q:.3f}, bound/ref {(E.norm() / r['ref'].norm()).item():.2e}{extra}")
    assert q <= 1.0, (c, q)


@pytest.mark.parametrize("name", [c.name for c in go.CONV_CASES])
def test_conv(name):
    c, d, r = _conv_ref(name)
    out, form, _ = _run_conv(c, d)
    assert form == go.conv_policy(c), (c, form, go.conv_policy(c))
    assert c.form is None or form == c.form, f"{c}: ran {form}, the case is named for {c.form}"
    _check_conv(c, d, r, out, form)


@pytest.mark.parametrize("name", [c.name for c in go.CONV_CASES if c.ws])
def test_conv_deferred_reduction_is_the_reduce_kernel_bit_for_bit(name):
    """defer_reduce leaves the raw slices; bias + slices in slice order (+ the previous value under accumulate) is the non-deferred output"""
    c, d, r = _conv_ref(name)
    out, form, _ = _run_conv(c, d)
    out_d, form_d, slabs = _run_conv(c, d, defer=1)
    assert form_d == form and form[4] > 1 and slabs is not None
    (Ho, Wo) = c.out_hw
    v = (d["bias"][0][None, :, None].expand(c.N, c.Cout, Ho * Wo).clone() if d["bias"] is not None else torch.zeros(c.N, c.Cout, Ho * Wo))
    for k in range(form[4]):
        v = v + slabs[k]
    if c.accumulate:
        v = d["prev"].reshape(c.N, c.Cout, -1) + v
    assert torch.equal(_bits(v.reshape(out.shape)), _bits(out)), f"{c}: bias + slabs in slice order is not the reduced output"
    print(f"GEN_OPS conv {c} defer_reduce: {form[4]} slices, bias + slabs in slice order == the reduced output bit for bit")


@pytest.mark.parametrize("name", [c.name for c in go.REFLECT_DGRAD_CASES])
def test_conv_reflect_dgrad(name):
    c, d, r = _conv_ref(name)
    out, _, _ = _run_conv(c, d, reflect_dgrad=True)
    _check_conv(c, d, r, out, (0, 4, 1, 1, 1), fold=True, tag=" reflect_dgrad")


@pytest.mark.parametrize("name", [c.name for c in go.ARENA_CASES])
def test_conv_independent_arenas_match_their_own_single_calls(name):
    """p_nstride (and p_group): every image against the fp64 reference of ITS arena, and bit-identical to an N = 1 call with that arena"""
    c, d, r = _conv_ref(name)
    out, form, _ = _run_conv(c, d)
    assert form == go.conv_policy(c)
    _check_conv(c, d, r, out, form)
    for n in range(c.N):
        a = c.arena_of(n)
        c1 = go.ConvCase(f"{c.name}_img{n}", c.Ci, c.Co, c.H, c.W, c.ks, c.stride, transposed=c.transposed, ws=c.ws)
        d1 = dict(inp=d["inp"][n:n + 1], w=d["w"][a:a + 1], bias=d["bias"][a:a + 1] if d["bias"] is not None else None, prev=None)
        out1, form1, _ = _run_conv(c1, d1)
        assert form1 == form, (form1, form)
        assert torch.equal(_bits(out1[0]), _bits(out[n])), f"{c}: image {n} differs from its own N = 1 call"
    print(f"GEN_OPS conv {c}: every image bit-identical to its own N = 1 call")


# the halves of the pair launches (conv_pair_launch): forward, the 1x1 skip convolution beside the 3x3 stride-2 encoder convolution of the
# same input; backward, two 1x1 data gradients; a 5x5 partner is outside the instantiated set and takes two launches
PAIR_PARTS = [go.ConvCase("pair_f_a", 8, 4, 16, 18, 1), go.ConvCase("pair_f_b", 8, 16, 16, 18, 3, 2),
              go.ConvCase("pair_b_a", 8, 4, 9, 11, 1, transposed=1), go.ConvCase("pair_b_b", 24, 20, 9, 11, 1, transposed=1),
              go.ConvCase("pair_x_a", 8, 4, 13, 12, 1), go.ConvCase("pair_x_b", 8, 18, 13, 12, 5)]


@pytest.mark.parametrize("na,nb,shared", [("pair_f_a", "pair_f_b", True), ("pair_b_a", "pair_b_b", False), ("pair_x_a", "pair_x_b", True)])
def test_conv_pair(na, nb, shared):
    ca, da, ra = _conv_ref(na)
    cb, db, rb = _conv_ref(nb)
    if shared:   # both read the same input
        db = dict(db, inp=da["inp"])
        rb = go.conv_ref(cb, db)
    singles = [_run_conv(ca, da), _run_conv(cb, db)]
    bufs = []
    for c, d in ((ca, da), (cb, db)):
        inb = Buf(c.N, c.Cin, c.in_hw[0] * c.in_hw[1], False, d["inp"])
        outb = Buf(c.N, c.Cout, c.out_hw[0] * c.out_hw[1], True)
        bufs.append((inb, outb, _params(c, d)))
    args = [_conv_args(c, d, inb, outb, p[1], p[2], p[3]) for (c, d), (inb, outb, p) in zip(((ca, da), (cb, db)), bufs)]
    forms = (C.c_int * (2 * _lib.GEN_CONV_FORM_INTS))()
    rc = _lib.lib().splice_gen_conv_pair(C.byref(args[0]), C.byref(args[1]), forms, _st())
    torch.cuda.synchronize()
    assert rc == 0
    for i, (c, d, r) in enumerate(((ca, da, ra), (cb, db, rb))):
        inb, outb, _ = bufs[i]
        assert outb.untouched_outside()
        out = outb.get().reshape(singles[i][0].shape)
        form = tuple(forms[5 * i:5 * i + 5])
        assert form == singles[i][1] == go.conv_policy(c)
        _check_conv(c, d, r, out, form, tag=" (pair launch)")
        assert torch.equal(_bits(out), _bits(singles[i][0])), f"{c}: the pair launch differs from conv_launch"
    print(f"GEN_OPS conv_pair {na} + {nb}: both bit-identical to their own conv_launch")


def test_conv_refusals():
    """return codes only: nothing is launched, nothing is written"""
    c, d, _ = _conv_ref("k3_reflect_small")
    (Hi, Wi), (Ho, Wo) = c.in_hw, c.out_hw
    inb, outb = Buf(1, c.Cin, Hi * Wi, False, d["inp"]), Buf(1, c.Cout, Ho * Wo)
    pt, wp, bp, pn = _params(c, d)
    lib = _lib.lib()

    def rc_of(**kw):
        a = _conv_args(c, d, inb, outb, wp, bp, pn)
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.splice_gen_conv(C.byref(a), None, _st())
    assert rc_of() == 0
    torch.cuda.synchronize()
    outb.t.view(torch.int32)[outb.idx] = NAN_BITS
    for kw in (dict(w=None), dict(out=None), {"in": None}, dict(N=0), dict(Cin=0), dict(Ho=-1), dict(ks=2), dict(ks=9), dict(stride=3), dict(stride=0),
               dict(pad=11), dict(pad=Hi), dict(transposed=1), dict(in_cstride=Hi * Wi - 1), dict(out_cstride=Ho * Wo - 1), dict(in_cstride=1 << 29),
               dict(w_jstride=1 << 30), dict(p_group=2), dict(defer_reduce=1), dict(act=2)):
        assert rc_of(**kw) == ERR_ARG, kw
        assert b"invalid argument" in lib.splice_last_error()
    a = _conv_args(c, d, inb, outb, wp, bp, pn)
    sc_t, sc_p, _ = _flat(n=16)
    assert lib.splice_gen_conv_reflect_dgrad(C.byref(a), sc_p, 16, _st()) == ERR_ARG      # scratch too small
    assert lib.splice_gen_conv_reflect_dgrad(C.byref(a), None, 1 << 20, _st()) == ERR_ARG
    assert lib.splice_gen_conv_pair(C.byref(a), None, None, _st()) == ERR_ARG
    torch.cuda.synchronize()
    assert outb.all_untouched() and _guards_ok(sc_t, 16)


# ================================================================================================ pointwise
@pytest.mark.parametrize("h,w,Ho,Wo", go.UP_CASES)
def test_upsample2x_forward_and_adjoint(h, w, Ho, Wo):
    N, Cc = 2, 3
    x, dout = go.up_inputs(h, w, Ho, Wo, N, Cc)
    lib = _lib.lib()
    xin, yout = Buf(N, Cc, h * w, False, x), Buf(N, Cc, Ho * Wo)
    rc = lib.splice_gen_upsample2x_fwd(xin.ptr, xin.ns, yout.ptr, yout.ns, N, Cc, h, w, Ho, Wo, _st())
    torch.cuda.synchronize()
    assert rc == 0 and yout.untouched_outside()
    got = yout.get().reshape(N, Cc, Ho, Wo).double()
    q_f = _ratio((got - go.up_ref(x.double(), Ho, Wo)).abs(), go.up_bound(x, Ho, Wo))
    din, dob = Buf(N, Cc, h * w), Buf(N, Cc, Ho * Wo, False, dout)
    rc = lib.splice_gen_upsample2x_bwd(dob.ptr, dob.ns, din.ptr, din.ns, N, Cc, h, w, Ho, Wo, _st())
    torch.cuda.synchronize()
    assert rc == 0 and din.untouched_outside()
    got = din.get().reshape(N, Cc, h, w).double()
    q_b = _ratio((got - go.up_adjoint_ref(dout, h, w)).abs(), go.up_adjoint_bound(dout, h, w))
    print(f"GEN_OPS upsample2x {h}x{w} -> {Ho}x{Wo}: forward err/bound {q_f:.3f}, adjoint err/bound {q_b:.3f}")
    assert q_f <= 1.0 and q_b <= 1.0
    assert lib.splice_gen_upsample2x_fwd(xin.ptr, xin.ns, yout.ptr, yout.ns, N, Cc, h, w, 2 * h + 1, Wo, _st()) == ERR_ARG
    assert lib.splice_gen_upsample2x_bwd(dob.ptr, dob.ns, None, din.ns, N, Cc, h, w, Ho, Wo, _st()) == ERR_ARG


@pytest.mark.parametrize("HW", go.SIGMOID_HW)
@pytest.mark.parametrize("N,group", go.SIGMOID_BATCHES)
def test_sigmoid_bwd_bias(HW, N, group):
    Cc, indep = 3, group > 0
    dout, s = go.sigmoid_inputs(HW, N, group, Cc)
    lib = _lib.lib()
    pf = lib.splice_gen_sigmoid_bias_part_floats(N, Cc)
    assert pf == N * Cc * 64
    dt, dp, _ = _flat(dout)
    stt, sp, _ = _flat(s)
    ot, op, ov = _flat(n=N * Cc * HW)
    pt, pp, pv = _flat(n=pf)
    chunks = C.c_int(0)
    rc = lib.splice_gen_sigmoid_bwd_bias(dp, sp, op, N, Cc, HW, pp, pf, 4096 if indep else 0, max(group, 1), C.byref(chunks), _st())
    torch.cuda.synchronize()
    assert rc == 0 and _guards_ok(ot, N * Cc * HW) and _guards_ok(pt, pf)
    segs = go.sigmoid_bias_segments(N, HW, group)
    assert chunks.value == len(segs), (chunks.value, len(segs))
    ref, E = go.sigmoid_bwd_ref(dout, s)
    q_e = _ratio((ov.cpu().reshape(N, Cc, HW).double() - ref).abs(), E)
    pref, PE = go.sigmoid_bias_ref(ref, segs)
    parts = pv.cpu()[:len(segs) * Cc].reshape(len(segs), Cc).double()
    assert (_bits(pv.cpu()[len(segs) * Cc:]) == NAN_BITS).all(), "partials written beyond [group][segment][channel]"
    q_p = _ratio((parts - pref).abs(), PE)
    # the partials of a group summed in segment order against the reference's per-channel sum
    ng = len(segs) // go.plane_blocks(HW)
    tot = parts.reshape(ng, -1, Cc).sum(1)
    q_s = _ratio((tot - pref.reshape(ng, -1, Cc).sum(1)).abs(), PE.reshape(ng, -1, Cc).sum(1))
    print(f"GEN_OPS sigmoid_bwd_bias HW {HW} N {N} group {group}: dpre err/bound {q_e:.3f}, partials {q_p:.3f}, channel sums {q_s:.3f}")
    assert q_e <= 1.0 and q_p <= 1.0 and q_s <= 1.0
    assert lib.splice_gen_sigmoid_bwd_bias(dp, sp, op, N, Cc, HW, pp, pf - 1, 0, 1, None, _st()) == ERR_ARG
    assert lib.splice_gen_sigmoid_bwd_bias(dp, sp, op, 3, Cc, HW, pp, pf, 4096, 2, None, _st()) == ERR_ARG


# ================================================================================================ weight gradients
@pytest.mark.parametrize("c", go.WGRAD_CASES, ids=repr)
def test_conv_wgrad(c):
    d = go.wgrad_inputs(c)
    r = go.wgrad_ref(c, d)
    lib = _lib.lib()
    n = c.Co * c.Ci * c.ks * c.ks
    xb, dyb = Buf(c.N, c.Ci, c.H * c.W, c.concat, d["x"]), Buf(c.N, c.Co, c.Ho * c.Wo, c.concat, d["dy"])
    wsf = lib.splice_gen_conv_wgrad_ws_floats(c.N, c.Ci, c.Co, c.ks, c.Ho, c.Wo)
    assert wsf == c.wform[3] * n
    ws_t, ws_p, _ = _flat(n=wsf)
    n_out = c.N if c.indep else 1
    pn = (n + 8 + 3) // 4 * 4 if c.indep else 0           # gradient arenas of the independent images
    host = torch.full((n_out, pn if c.indep else n), float("nan"))
    dw_t, dw_p, dw_v = _flat(host)
    _bits(dw_t)[:] = NAN_BITS
    if c.acc:
        dw_v.reshape(n_out, -1)[:, :n] = d["prev"].reshape(n_out, n).to(DEV)
    a = _lib.GenWgradArgs()
    a.x, a.dy, a.ws, a.ws_floats = xb.ptr, dyb.ptr, ws_p, wsf
    a.x_nstride, a.x_cstride, a.dy_nstride, a.dy_cstride = xb.ns, xb.cs, dyb.ns, dyb.cs
    a.N, a.Cin, a.Hi, a.Wi, a.Cout, a.Ho, a.Wo, a.ks, a.stride, a.pad, a.reflect = c.N, c.Ci, c.H, c.W, c.Co, c.Ho, c.Wo, c.ks, c.stride, c.pad, c.reflect
    form = (C.c_int * _lib.GEN_WGRAD_FORM_INTS)()
    rc = lib.splice_gen_conv_wgrad(C.byref(a), dw_p, c.acc, c.N if c.indep else 1, pn, form, _st())
    torch.cuda.synchronize()
    assert rc == 0, lib.splice_last_error()
    assert tuple(form)[:5] == c.wform == go.wgrad_form(c), f"{c}: ran {tuple(form)}, the case is named for {c.wform}"
    assert _guards_ok(ws_t, wsf) and _guards_ok(dw_t, host.numel()) and xb.untouched_outside() and dyb.untouched_outside()
    got = dw_v.cpu().reshape(n_out, -1)
    assert (_bits(got[:, n:]) == NAN_BITS).all(), "written between the gradient arenas"
    assert torch.isfinite(ws_t[GUARD:GUARD + wsf]).all(), "a chunk partial was not written"
    q = _ratio((got[:, :n].reshape(r["ref"].shape).double() - r["ref"]).abs(), r["E"])
    print(f"GEN_OPS wgrad {c}: form (class, variant, ppc, chunks, vec, workgroups) = {tuple(form)}, err/bound {q:.3f}, bound/ref {(r['E'].norm() / r['ref'].norm()).item():.2e}")
    assert q <= 1.0, (c, q)


def test_conv_wgrad_refusals():
    c = go.WGRAD_CASES[0]
    d = go.wgrad_inputs(c)
    lib = _lib.lib()
    n = c.Co * c.Ci
    xb, dyb = Buf(1, c.Ci, c.H * c.W, False, d["x"]), Buf(1, c.Co, c.Ho * c.Wo, False, d["dy"])
    wsf = lib.splice_gen_conv_wgrad_ws_floats(1, c.Ci, c.Co, 1, c.Ho, c.Wo)
    ws_t, ws_p, _ = _flat(n=wsf)
    dw_t, dw_p, _ = _flat(n=n)

    def rc_of(dw=dw_p, n_img=1, pn=0, **kw):
        a = _lib.GenWgradArgs()
        a.x, a.dy, a.ws, a.ws_floats = xb.ptr, dyb.ptr, ws_p, wsf
        a.x_nstride, a.x_cstride, a.dy_nstride, a.dy_cstride = xb.ns, xb.cs, dyb.ns, dyb.cs
        a.N, a.Cin, a.Hi, a.Wi, a.Cout, a.Ho, a.Wo, a.ks, a.stride, a.pad, a.reflect = 1, c.Ci, c.H, c.W, c.Co, c.Ho, c.Wo, 1, 1, 0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.splice_gen_conv_wgrad(C.byref(a), dw, 0, n_img, pn, None, _st())
    for kw in (dict(x=None), dict(dy=None), dict(ws=None), dict(dw=None), dict(Cout=129), dict(ks=2), dict(ks=4), dict(N=0), dict(Hi=0), dict(stride=3),
               dict(ws_floats=wsf - 1), dict(x_cstride=c.H * c.W - 1), dict(x_cstride=1 << 29), dict(Hi=70000), dict(n_img=2), dict(pn=n - 1, n_img=1),
               dict(reflect=1, pad=c.H)):
        assert rc_of(**kw) == ERR_ARG, kw
    torch.cuda.synchronize()
    assert (_bits(ws_t) == NAN_BITS).all() and (_bits(dw_t) == NAN_BITS).all()


# ================================================================================================ BatchNorm
KIND = {go.SMALL: "SMALL", go.MID: "MID", go.TWO_STAGE: "TWO_STAGE", go.TWO_STAGE_VEC: "TWO_STAGE_VEC"}


@functools.lru_cache(maxsize=None)
def _bn_problem(name):
    c = {c.name: c for c in go.BN_CASES}[name]
    d = go.bn_inputs(c)
    return c, d, go.bn_problem(c, d)


def _bn_params(c, *tensors):
    """parameter arenas [n_par][p_nstride] holding the given [n_par][k] tensors back to back; returns (buffer, pointers, p_nstride, offsets)"""
    widths = [t.shape[1] for t in tensors]
    pn = (sum(widths) + 6 + 3) // 4 * 4
    host = torch.full((c.n_par, pn), float("nan"))
    offs, o = [], 0
    for t, wd in zip(tensors, widths):
        host[:, o:o + wd] = t
        offs.append(o)
        o += wd
    t, p, v = _flat(host)
    return t, [C.c_void_p(p.value + 4 * o) for o in offs], pn, offs, v


def _bn_common(c, a, par_ptrs, pn):
    a.N, a.C, a.HW, a.batch = c.N, c.C, c.HW, c.batch
    a.eps, a.slope = go.BN_EPS, c.slope
    a.p_nstride = pn if c.arenas else 0
    a.gamma, a.beta = par_ptrs[0], par_ptrs[1]
    if c.up:
        a.up_h, a.up_w, a.up_Ho, a.up_Wo, a.up_c0 = c.up
    if c.pre:
        a.pre_C, a.pre_slope = c.pre[0], go.PRE_SLOPE
        a.pre_gamma, a.pre_beta = par_ptrs[2], par_ptrs[3]


def _reported_form(c):
    out = (C.c_int * _lib.GEN_BN_FORM_INTS)()
    assert _lib.lib().splice_gen_bn_form(c.HW, c.N, 4 if c.arenas else 0, c.batch, out) == 0
    assert tuple(out) == c.form and out[0] == c.kind, f"{c}: runs as {tuple(out)}, the case is named for {KIND[c.kind]} {c.form}"
    return tuple(out)


@pytest.mark.parametrize("name", [c.name for c in go.BN_CASES])
def test_bn_forward(name):
    c, d, p = _bn_problem(name)
    form = _reported_form(c)
    lib = _lib.lib()
    N, Cc, HW = c.N, c.C, c.HW
    f = p["fwd"]
    pars = [d["gamma"], d["beta"]] + ([d["pre_gamma"], d["pre_beta"]] if c.pre else []) + ([d["bias"]] if c.slabs else []) + \
           ([d["pre_bias"]] if c.pre and c.pre[1] else [])
    par_t, pp, pn, _, _ = _bn_params(c, *pars)
    # y: what the kernel forms itself (slab sums, upsampled channels, the chained skip BatchNorm's output) starts as NaN payload
    formed = torch.zeros(Cc, dtype=torch.bool)
    if c.slabs:
        formed[:] = True
    if c.up:
        formed[c.up[4]:] = True
    if c.pre:
        formed[:c.pre[0]] = True
    yb = Buf(N, Cc, HW, False, d["y"])
    yb_view = yb.t[GUARD:GUARD + N * Cc * HW].view(N, Cc, HW)
    _bits(yb_view)[:, formed] = NAN_BITS
    outb = Buf(N, Cc, HW)
    part_f = lib.splice_gen_bn_part_floats(N, Cc)
    part_t, part_p, _ = _flat(n=part_f)
    st_t, st_p, st_v = _flat(n=2 * N * Cc)
    a = _lib.GenBnArgs()
    _bn_common(c, a, pp, pn)
    a.y, a.out, a.y_nstride, a.out_nstride = yb.ptr, outb.ptr, yb.ns, outb.ns
    a.part, a.part_floats = part_p, part_f
    a.mean, a.rstd = st_p, C.c_void_p(st_p.value + 4 * N * Cc)
    keep = [par_t, part_t, st_t]
    if c.up:
        srcb = Buf(N, Cc - c.up[4], c.up[0] * c.up[1], False, d["src"])
        a.up_src, a.up_src_ns = srcb.ptr, srcb.ns
    if c.slabs:
        sl_t, sl_p, _ = _flat(d["slabs"])
        a.slabs, a.ksplit, a.bias = sl_p, c.slabs, pp[-1 - (1 if c.pre and c.pre[1] else 0)]
        keep.append(sl_t)
    if c.pre:
        pc, ps = c.pre
        y1b = Buf(N, pc, HW, False, None if ps else d["pre_y"])
        pst_t, pst_p, pst_v = _flat(n=2 * N * pc)
        a.pre_y, a.pre_y_ns, a.pre_mean, a.pre_rstd = y1b.ptr, y1b.ns, pst_p, C.c_void_p(pst_p.value + 4 * N * pc)
        if ps:
            psl_t, psl_p, _ = _flat(d["pre_slabs"])
            a.pre_slabs, a.pre_ksplit, a.pre_bias = psl_p, ps, pp[-1]
            keep.append(psl_t)
    rc = lib.splice_gen_bn_fwd(C.byref(a), _st())
    torch.cuda.synchronize()
    assert rc == 0, lib.splice_last_error()
    assert outb.untouched_outside() and yb.untouched_outside() and _guards_ok(st_t, 2 * N * Cc) and _guards_ok(part_t, part_f) and _guards_ok(par_t, c.n_par * pn)
    if c.kind < go.TWO_STAGE and not (c.up and not form[4]):
        assert (_bits(part_t) == NAN_BITS).all(), "a one-launch form wrote the two-stage scratch"
    y_got = yb.get()
    assert torch.equal(_bits(y_got[:, ~formed]), _bits(d["y"][:, ~formed])), "y was rewritten where the kernel forms nothing"
    qs = {}
    if c.slabs:   # bit-exact: bias + slabs in slab order
        assert torch.equal(_bits(y_got), _bits(p["y32"])), f"{c}: the stored y is not bias + slabs in slab order"
        qs["y"] = "bit-exact"
    elif formed.any():
        qs["y"] = _ratio((y_got[:, formed].double() - p["y_ref"][:, formed]).abs(), p["E_y"][:, formed].clamp(min=1e-300))
    if c.pre:
        pc, ps = c.pre
        f1 = p["pre"]["fwd"]
        if ps:
            assert torch.equal(_bits(y1b.get()), _bits(p["pre"]["y1"])), f"{c}: the skip plane is not bias + slabs in slab order"
        else:
            assert torch.equal(_bits(y1b.get()), _bits(d["pre_y"]))
        assert y1b.untouched_outside() and _guards_ok(pst_t, 2 * N * pc)
        pst = pst_v.cpu().double().reshape(2, N, pc)
        qs["pre_mean"], qs["pre_rstd"] = _ratio((pst[0] - f1["mean"]).abs(), f1["E_mean"]), _ratio((pst[1] - f1["rstd"]).abs(), f1["E_rstd"])
    st = st_v.cpu().double().reshape(2, N, Cc)
    qs["mean"], qs["rstd"] = _ratio((st[0] - f["mean"]).abs(), f["E_mean"]), _ratio((st[1] - f["rstd"]).abs(), f["E_rstd"])
    out = outb.get()
    assert torch.isfinite(out).all()
    qs["out"] = _ratio((out.double() - f["out"]).abs(), f["E_out"])
    print(f"GEN_OPS bn_fwd {c}: form {KIND[form[0]]} {form[1:]}, err/bound " + ", ".join(f"{k} {v if isinstance(v, str) else format(v, '.3f')}" for k, v in qs.items()) +
          f", bound/ref out {(f['E_out'].norm() / f['out'].norm()).item():.2e}")
    assert all(isinstance(v, str) or v <= 1.0 for v in qs.values()), (c, qs)


@pytest.mark.parametrize("name", [c.name for c in go.BN_CASES if not c.slabs])
def test_bn_backward(name):
    c, d, p = _bn_problem(name)
    form = _reported_form(c)
    lib = _lib.lib()
    N, Cc, HW = c.N, c.C, c.HW
    b = p["bwd"]
    zeros = torch.zeros(c.n_par, Cc)
    prev = p["prev"] if c.acc else None
    pars = [d["gamma"], d["beta"]] + ([d["pre_gamma"], d["pre_beta"]] if c.pre else [])
    par_t, pp, pn, offs, _ = _bn_params(c, *pars)
    # gradient arenas with the layout of the parameter arenas
    g_host = [torch.full((c.n_par, Cc), float("nan")), torch.full((c.n_par, Cc), float("nan"))]
    if c.pre:
        g_host += [torch.full((c.n_par, c.pre[0]), float("nan"))] * 2
    g_t, gp, gpn, _, g_v = _bn_params(c, *g_host)
    assert gpn == pn
    _bits(g_t)[:] = NAN_BITS
    gv = g_v.view(c.n_par, pn)
    if c.acc:
        gv[:, offs[0]:offs[0] + Cc], gv[:, offs[1]:offs[1] + Cc] = prev[0].to(DEV), prev[1].to(DEV)
        if c.pre:
            q = p["pre"]
            gv[:, offs[2]:offs[2] + c.pre[0]], gv[:, offs[3]:offs[3] + c.pre[0]] = q["prev"][0].to(DEV), q["prev"][1].to(DEV)
    yb, outb = Buf(N, Cc, HW, False, p["y_in"]), Buf(N, Cc, HW, False, p["out32"])
    dab = Buf(N, Cc, HW, False, d["da"] if (not c.da_slabs or c.da_slabs[1]) else None)
    dyb = Buf(N, Cc, HW)
    part_f = lib.splice_gen_bn_part_floats(N, Cc)
    part_t, part_p, _ = _flat(n=part_f)
    st_t, st_p, _ = _flat(torch.stack([p["m32"], p["r32"]]))
    a = _lib.GenBnArgs()
    _bn_common(c, a, pp, pn)
    a.y, a.out, a.y_nstride, a.out_nstride = yb.ptr, outb.ptr, yb.ns, outb.ns
    a.part, a.part_floats = part_p, part_f
    a.mean, a.rstd = st_p, C.c_void_p(st_p.value + 4 * N * Cc)
    a.da, a.dy, a.da_nstride, a.dy_nstride = dab.ptr, dyb.ptr, dab.ns, dyb.ns
    a.dgamma, a.dbeta, a.accumulate = gp[0], gp[1], c.acc
    written = torch.ones(Cc, dtype=torch.bool)   # channels whose dy the launch writes
    if c.up:
        srcb = Buf(N, Cc - c.up[4], c.up[0] * c.up[1])
        a.up_d_src, a.up_d_src_ns = srcb.ptr, srcb.ns
        if form[5]:
            written[c.up[4]:] = False   # fused: the gradient of an upsampled channel goes straight through the adjoint
    if c.da_slabs:
        sl_t, sl_p, _ = _flat(d["da_slabs"])
        a.da_slabs, a.da_ksplit, a.da_accumulate = sl_p, c.da_slabs[0], c.da_slabs[1]
    if c.pre:
        pc = c.pre[0]
        q = p["pre"]
        y1b, dy1b = Buf(N, pc, HW, False, q["y1_in"]), Buf(N, pc, HW)
        pst_t, pst_p, _ = _flat(torch.stack([q["m32"], q["r32"]]))
        a.pre_y, a.pre_y_ns, a.pre_mean, a.pre_rstd = y1b.ptr, y1b.ns, pst_p, C.c_void_p(pst_p.value + 4 * N * pc)
        a.pre_dy, a.pre_dgamma, a.pre_dbeta = dy1b.ptr, gp[2], gp[3]
        written[:pc] = False            # chained: the gradient of a skip channel goes on into the skip BatchNorm's adjoint
    rc = lib.splice_gen_bn_bwd(C.byref(a), _st())
    torch.cuda.synchronize()
    assert rc == 0, lib.splice_last_error()
    assert dyb.untouched_outside() and _guards_ok(part_t, part_f) and yb.untouched_outside() and outb.untouched_outside()
    dy = dyb.get()
    assert (_bits(dy[:, ~written]) == NAN_BITS).all(), "dy written for a channel whose gradient goes on inside the launch"
    assert torch.isfinite(dy[:, written]).all()
    sub = dict(dy=b["dy"][:, written], dy_alt=b["dy_alt"][:, written], E_dy=b["E_dy"][:, written])
    amb = p["amb"][:, written] if p["amb"] is not None else None
    qs = {"dy": go.bn_dy_ratio(dy[:, written], sub, amb)}
    gh = gv.cpu().double()
    assert (_bits(gv.cpu()[:, sum(t.shape[1] for t in g_host):]) == NAN_BITS).all() and _guards_ok(g_t, c.n_par * pn)
    dg, db = gh[:, offs[0]:offs[0] + Cc], gh[:, offs[1]:offs[1] + Cc]
    qs["dgamma"], qs["dbeta"] = _ratio((dg - b["dgamma"]).abs(), b["E_dgamma"]), _ratio((db - b["dbeta"]).abs(), b["E_dbeta"])
    if c.up:
        assert srcb.untouched_outside()
        qs["d_src"] = _ratio((srcb.get().reshape(p["d_src"].shape).double() - p["d_src"]).abs(), p["E_d_src"])
    if c.pre:
        b1 = q["bwd"]
        assert dy1b.untouched_outside()
        qs["pre_dy"] = go.bn_dy_ratio(dy1b.get(), b1)
        qs["pre_dgamma"] = _ratio((gh[:, offs[2]:offs[2] + pc] - b1["dgamma"]).abs(), b1["E_dgamma"])
        qs["pre_dbeta"] = _ratio((gh[:, offs[3]:offs[3] + pc] - b1["dbeta"]).abs(), b1["E_dbeta"])
    share = p["amb"].double().mean(2).max().item() if p["amb"] is not None else 0.0
    assert share <= go.SIGN_SHARE_CAP
    print(f"GEN_OPS bn_bwd {c}: form {KIND[form[0]]} {form[1:]}, err/bound " + ", ".join(f"{k} {v:.3f}" for k, v in qs.items()) +
          f", bound/ref dy {(b['E_dy'].norm() / b['dy'].norm()).item():.2e}, sign-ambiguous share {share:.1e}")
    assert all(v <= 1.0 for v in qs.values()), (c, qs)


def test_bn_refusals():
    """what bn_args_ok and the hook refuse: return codes only, nothing written"""
    lib = _lib.lib()
    N, Cc, HW = 2, 2, 5000
    buf = Buf(N, Cc, HW)
    par_t, par_p, _ = _flat(torch.ones(4 * Cc + 64))
    sc_t, sc_p, _ = _flat(n=lib.splice_gen_bn_part_floats(N, Cc) + 4 * N * Cc)

    def rc_of(bwd=False, **kw):
        a = _lib.GenBnArgs()
        a.y = a.out = a.da = a.dy = buf.ptr
        a.y_nstride = a.out_nstride = a.da_nstride = a.dy_nstride = buf.ns
        a.N, a.C, a.HW, a.eps, a.slope = N, Cc, HW, go.BN_EPS, 0.2
        a.gamma = a.beta = a.dgamma = a.dbeta = par_p
        a.part, a.part_floats = sc_p, lib.splice_gen_bn_part_floats(N, Cc)
        a.mean = a.rstd = C.c_void_p(sc_p.value + 4 * a.part_floats)
        for k, v in kw.items():
            setattr(a, k, v)
        return (lib.splice_gen_bn_bwd if bwd else lib.splice_gen_bn_fwd)(C.byref(a), _st())
    some = par_p
    cases = [dict(y=None), dict(gamma=None), dict(beta=None), dict(mean=None), dict(N=0), dict(HW=0), dict(batch=9), dict(batch=3), dict(N=4, batch=2),
             dict(part=None), dict(part_floats=8), dict(y_nstride=Cc * HW - 1),
             dict(slabs=some, ksplit=4),                                  # TWO_STAGE (shared parameters, N 2) takes no forward slabs
             dict(HW=196, slabs=some, ksplit=1), dict(HW=196, batch=2, slabs=some, ksplit=4),
             dict(pre_y=some, pre_C=1, pre_gamma=some, pre_beta=some, pre_mean=some, pre_rstd=some),   # no own plane: cannot host a BnPre
             dict(HW=196, up_src=some, up_c0=1, up_h=7, up_w=7, up_Ho=14, up_Wo=15), dict(HW=196, up_src=some, up_c0=2, up_h=7, up_w=7, up_Ho=14, up_Wo=14),
             dict(HW=196, up_src=some, up_c0=1, up_h=6, up_w=7, up_Ho=14, up_Wo=14),
             dict(p_nstride=8, pre_y=some, pre_C=1, pre_gamma=some, pre_beta=some, pre_mean=some, pre_rstd=some, pre_slabs=some, pre_ksplit=4)]  # MID: no skip slabs
    for kw in cases:
        assert rc_of(**kw) == ERR_ARG, kw
    for kw in (dict(da=None), dict(dgamma=None), dict(HW=196, da_slabs=some, da_ksplit=4),   # shared parameters, N 2: the backward takes no slabs
               dict(p_nstride=8, pre_y=some, pre_C=1, pre_gamma=some, pre_beta=some, pre_mean=some, pre_rstd=some),      # backward BnPre without pre_dy
               dict(HW=196, up_d_src=None, up_src=some, up_c0=1, up_h=7, up_w=7, up_Ho=14, up_Wo=14)):
        assert rc_of(True, **kw) == ERR_ARG, kw
    out = (C.c_int * _lib.GEN_BN_FORM_INTS)()
    assert lib.splice_gen_bn_form(0, 1, 0, 0, out) == ERR_ARG and lib.splice_gen_bn_form(16, 1, 0, 0, None) == ERR_ARG
    torch.cuda.synchronize()
    assert buf.all_untouched() and (_bits(sc_t) == NAN_BITS).all()
