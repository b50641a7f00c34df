"""fp64 references, worst-case element bounds and fp32 rounding emulations of the GENERATOR's kernels, one launcher at a time (test
infrastructure only, torch-CPU): the convolutions of ``splice_amd/csrc/gen_conv.hip`` (implicit GEMM, LDS-halo tile kernel, split-K, pair
launch, reflect fold), the weight gradients of ``gen_wgrad.hip``, the BatchNorm forms of ``gen_bn.hip`` and the pointwise kernels of
``gen_pointwise.hip``.  ``tests/test_gen_ops_gpu.py`` drives the launchers through the ``splice_gen_*`` test hooks and holds every output
element to the bounds below; ``tests/test_gen_ops_cpu.py`` checks without a GPU that the emulations stay inside the bounds and that each
deliberate error (the ``mut`` switches) leaves them.

How the bounds are derived.  ``U = 2^-24`` is fp32's unit roundoff, ``g(k) = k U / (1 - k U)``.  The kernels read fp32 operands exactly,
multiply exactly inside the fp32 MFMA (``v_mfma_f32_16x16x4_f32``: an fma chain) and round once per addition, so

  * a sum of products that passes through at most ``k`` roundings on any path -- in ANY order -- is within ``g(k) * sum_i |a_i b_i|`` of the
    exact sum (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  For a convolution ``k = n + c``: ``n`` reduction
    elements (channels x taps) and ``c`` extra roundings of the form: the bias add, one add per split-K slice, the 8-wave exchange,
    ``accumulate`` (whose previous value joins the sum of magnitudes), the reflect fold's nine adds;
  * a weight gradient sums ``N * Ho * Wo`` products; its chunks (``wgrad_chunks``, restated here) are independent chains of at most
    ``pix_per_chunk`` roundings, summed by four interleaved chains and one final tree: ``k = pix_per_chunk + ceil(chunks / 4) + 3``;
  * the BatchNorm reductions are trees, not chains.  The contract the kernels are held to is a depth of at most ``BN_DEPTH = 64`` additions
    for a plain plane sum (a thread's run of at most 20 elements, 6 shuffle levels, at most 16 wave partials, the images of a batch) and
    ``BN_CHAN = 48`` further roundings where segment statistics are merged pairwise (Chan et al.: at most 8 levels of 6 operations).  Mean,
    variance and the two backward sums get these reduction bounds, and they are propagated to first order through the normalisation --
    every elementary operation of the per-element arithmetic adds its own ``U |value|`` (the derivations stand with the functions);
  * the x2 bilinear upsampling has exact weights (1/4, 3/4, 1): 4 roundings on a path forward, 10 through the adjoint's 16 taps.

Nothing here is taken from what a kernel returns, with two exceptions the formats cannot give, both measured against the fp64 reference:
the sigmoid head (``__expf`` and the division; ``SIGMOID_ALLOW``) and the LeakyReLU sign of a BatchNorm backward that re-forms the
pre-activation itself (an element whose fp64 pre-activation is smaller than its own forward bound may take either slope;
``bn_bwd_check`` compares such elements against both branches and ``SIGN_SHARE_CAP`` caps their share of a plane).
"""
import math

import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64
U = 2.0 ** -24


def g(k):
    return k * U / (1.0 - k * U)


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def r32(t):
    """one fp32 rounding of an fp64 tensor, kept in fp64 (the emulations hold fp32 values in fp64 tensors)"""
    return t.to(F32).to(F64)


def cdiv(a, b):
    return (a + b - 1) // b


# ================================================================================================ convolutions
# The sigmoid head: 1 / (1 + __expf(-v)) has no format-derived bound.  Measured against fp64 on the head cases of the GPU test (worst
# |out - sigmoid(v_ref)|: 8.06e-8, all of it inside the propagated pre-activation bound -- the excess over that bound was negative, -1.5e-7;
# inputs seeded and fixed).  The allowance is 4 x the whole measured error, 3.2e-7, and stays far below the 2e-5 the whole-net test holds
# the generator output to.
SIGMOID_MEASURED = 8.06e-8
SIGMOID_ALLOW = 4 * SIGMOID_MEASURED


class ConvCase:
    """One launch.  The LAYER is Ci -> Co channels, ks x ks, stride, pad on an H x W input (output Ho x Wo); `transposed` runs its data
    gradient (in = dy [Co][Ho][Wo], out = dx [Ci][H][W]).  form = (tile kernel, CK, fn_run, ng, ksplit) the case is named for.
    arenas > 1: independent images with a parameter arena each (p_nstride), `group` images per arena.  concat: strided channel layout
    (channel strides larger than the plane, a channel offset inside a wider buffer)."""

    def __init__(self, name, Ci, Co, H, W, ks, stride=1, form=None, N=1, reflect=0, act=0, transposed=0, accumulate=0, ws=0, defer=0,
                 concat=0, arenas=1, group=1, bias=1, big=0):
        self.name, self.Ci, self.Co, self.H, self.W, self.ks, self.stride, self.pad = name, Ci, Co, H, W, ks, stride, ks // 2
        self.N, self.reflect, self.act, self.transposed, self.accumulate, self.ws, self.defer = N, reflect, act, transposed, accumulate, ws, defer
        self.concat, self.arenas, self.group, self.bias, self.form, self.big = concat, arenas, group, bias and not transposed, form, big
        self.Ho = (H + 2 * self.pad - ks) // stride + 1
        self.Wo = (W + 2 * self.pad - ks) // stride + 1
        # the launcher's view: reduction channels, output columns, input / output planes
        self.Cin, self.Cout = (Co, Ci) if transposed else (Ci, Co)
        self.in_hw, self.out_hw = ((self.Ho, self.Wo), (H, W)) if transposed else ((H, W), (self.Ho, self.Wo))

    def __repr__(self):
        return self.name

    def arena_of(self, img):
        return 0 if self.arenas == 1 else img // self.group


def conv_ck(ks, Cin):
    return (8 if Cin >= 32 else 4) if ks == 3 else (32 if Cin >= 64 else 16) if ks == 1 else 4


def conv_policy(c, ws_floats=None):
    """conv_tile_ok / conv_ck / conv_policy of gen_conv.hip restated (environment switches unset): the form a shape is expected to run in.
    The GPU test compares this, and the form each case names, with what the launcher reports."""
    Ho, Wo = c.out_hw
    HWo = Ho * Wo
    CK = conv_ck(c.ks, c.Cin)
    if c.ks == 3 and c.stride == 1 and not c.act and Wo >= 64 and HWo > 40000 and not (c.reflect and c.transposed):
        return (1, CK, 1 if c.Cout <= 16 else 2, 1, 1)
    mt = cdiv(HWo, 64)
    fn = 2 if (c.ks < 5 and 16 < c.Cout <= 32) else 1
    nt = cdiv(c.Cout, 16 * fn)
    fn_run = 2 if (c.ks < 5 and fn == 1 and c.Cout >= 64 and c.N >= 4) else fn
    if c.ks < 5 and mt >= 512 and c.Cout > 16:
        fn_run = max(fn_run, 4 if c.Cout > 32 else 2)
    npol = (c.group if c.group > 1 else 1) if c.arenas > 1 else c.N
    wgs = mt * nt * npol
    ksplit, ktiles = 1, cdiv(c.Cin, CK)
    if c.ws and wgs < 128 and ktiles >= 4:
        ksplit = min(cdiv(256, wgs), ktiles, 16)
        ksplit = 1 if ksplit < 2 else ksplit
    ng = 2 if (c.ks == 3 and CK == 8 and mt * nt * ksplit * npol <= 2048 and ktiles >= 2) else 1
    return (0, CK, 1 if c.ks >= 5 else fn_run, ng, ksplit)


def conv_inputs(c):
    """fp32 operands of a case, seeded: x (or dy for the data gradient) ~ N(0, 1) on a smooth offset, weights ~ N(0, 1) / sqrt(n), bias,
    and the previous contents of the output for `accumulate`"""
    gen = _gen("conv", c.name)
    Hi, Wi = c.in_hw
    Ho, Wo = c.out_hw
    inp = torch.randn(c.N, c.Cin, Hi, Wi, generator=gen) + 0.5
    w = torch.randn(c.arenas, c.Co, c.Ci, c.ks, c.ks, generator=gen) / math.sqrt(c.Cin * c.ks * c.ks)
    b = torch.randn(c.arenas, c.Co, generator=gen) * 0.5 if c.bias else None
    prev = torch.randn(c.N, c.Cout, Ho, Wo, generator=gen) if c.accumulate else None
    return dict(inp=inp, w=w, bias=b, prev=prev)


def _reflect_index(n, p, off=0):
    """source index of every position of the reflection-padded axis (nn.ReflectionPad2d: the mirror without the edge); off = 1: the
    deliberate error, a mirror that includes the edge"""
    idx = []
    for t in range(-p, n + p):
        s = -t - off if t < 0 else (2 * (n - 1) - t + off if t >= n else t)
        idx.append(min(max(s, 0), n - 1))
    return torch.tensor(idx)


def _pad_input(c, x, mut=None):
    """the forward's padded input [N][Ci][H + 2p][W + 2p]"""
    p = c.pad
    if not c.reflect:
        return F.pad(x, (p, p, p, p))
    off = 1 if mut == "reflect_off_by_one" else 0
    return x[:, :, _reflect_index(c.H, p, off)][:, :, :, _reflect_index(c.W, p, off)]


def conv_cols(c, inp, mut=None):
    """The reduction as the kernels see it: cols [N][K][L] and, per arena, the weight matrix [Cout][K], k = (reduction channel, ky, kx)
    in the weight's own order, L = output pixels.  Forward: im2col of the padded input.  Data gradient: the gather
    out[iy][ix] += dy[(iy + pad - ky) / s][(ix + pad - kx) / s] w[ky][kx] as im2col of the zero-stuffed dy with the taps flipped."""
    T = c.ks * c.ks
    if not c.transposed:
        cols = F.unfold(_pad_input(c, inp, mut), c.ks, stride=c.stride)

        def wmat(w):
            return w.reshape(c.Co, c.Ci * T)
    else:
        s, p, ks = c.stride, c.pad, c.ks
        N, Co, Ho, Wo = inp.shape
        st = inp.new_zeros(N, Co, (Ho - 1) * s + 1, (Wo - 1) * s + 1)
        st[:, :, ::s, ::s] = inp
        lo = ks - 1 - p
        hy, hx = c.H + ks - 1 - lo - st.shape[2], c.W + ks - 1 - lo - st.shape[3]
        assert lo >= 0 and hy >= 0 and hx >= 0
        cols = F.unfold(F.pad(st, (lo, hx, lo, hy)), ks)
        cols = cols.reshape(N, Co, T, -1).flip(2).reshape(N, Co * T, -1)   # unfold's tap (a, b) is the kernel's (ks-1-a, ks-1-b)

        def wmat(w):
            return w.permute(1, 0, 2, 3).reshape(c.Ci, c.Co * T)
    return cols, wmat


def conv_ref(c, d):
    """fp64: the reference (F.conv2d, reflection by F.pad, the data gradient by autograd of that forward), the sum of magnitudes S of
    every output element and the pre-activation.  Returns dict(ref, S, pre)."""
    x, w = d["inp"].double(), d["w"].double()
    Ho, Wo = c.out_hw
    outs, mags = [], []
    for n in range(c.N):
        wa = w[c.arena_of(n)]
        ba = d["bias"][c.arena_of(n)].double() if d["bias"] is not None else None

        def fwd(xin, wt, bt):
            if c.reflect:
                return F.conv2d(F.pad(xin, (c.pad,) * 4, mode="reflect"), wt, bt, stride=c.stride)
            return F.conv2d(xin, wt, bt, stride=c.stride, padding=c.pad)
        if not c.transposed:
            outs.append(fwd(x[n:n + 1], wa, ba))
            mags.append(fwd(x[n:n + 1].abs(), wa.abs(), ba.abs() if ba is not None else None))
        else:
            for xin, wt, acc in ((x[n:n + 1], wa, outs), (x[n:n + 1].abs(), wa.abs(), mags)):
                z = torch.zeros(1, c.Ci, c.H, c.W, dtype=F64, requires_grad=True)
                acc.append(torch.autograd.grad(fwd(z, wt, None), z, xin)[0])
    pre, S = torch.cat(outs), torch.cat(mags)
    ref = torch.sigmoid(pre) if c.act else pre
    if c.accumulate:
        ref = d["prev"].double() + ref
        S = S + d["prev"].double().abs()
    assert ref.shape == (c.N, c.Cout, Ho, Wo)
    return dict(ref=ref, S=S, pre=pre)


def conv_roundings(c, form, fold=False):
    """k of the bound: reduction length + the extra roundings of the form"""
    _, _, _, ng, ksplit = form
    return c.Cin * c.ks * c.ks + (1 if c.bias else 0) + (ksplit if ksplit > 1 else 0) + (1 if ng == 2 else 0) + (1 if c.accumulate else 0) + (9 if fold else 0)


def conv_bound(c, r, form, fold=False):
    """element bound of the output.  Behind the sigmoid the pre-activation bound goes through the derivative s (1 - s) <= 1/4 (first order) and
    SIGMOID_ALLOW is added."""
    E = g(conv_roundings(c, form, fold)) * r["S"]
    if c.act:
        s = torch.sigmoid(r["pre"])
        E = E * s * (1 - s) + SIGMOID_ALLOW + U * s
    return E.clamp(min=1e-300)


def emu_pixels(L, Wo):
    """output pixels the emulation is run on: all of a small plane; of a big one the two outermost rows and columns and every 41st pixel"""
    if L <= 4096:
        return torch.arange(L)
    i = torch.arange(L)
    y, x = i // Wo, i % Wo
    Ho = L // Wo
    return i[(y < 2) | (y >= Ho - 2) | (x < 2) | (x >= Wo - 2) | (i % 41 == 0)]


def _chain(cols, wm, ks_order, start=None):
    """acc = fp32(acc + w_k * col_k) over k in ks_order, from `start` (or 0): the fma chain of the matrix cores.  cols [K][L], wm [Cout][K],
    fp64 tensors holding fp32 values; the product is exact in fp64"""
    acc = torch.zeros(wm.shape[0], cols.shape[1], dtype=F64) if start is None else start.clone()
    for k in ks_order:
        acc = r32(acc + wm[:, k, None] * cols[None, k])
    return acc


def conv_emulate(c, d, form, order="kernel", mut=None, pix=None):
    """fp32 emulation of the launch on the output pixels `pix` (emu_pixels) -> [N][Cout][len(pix)] fp64.
    order 'kernel': channel tiles ascending, split-K slices of whole channel tiles summed in slice order behind the bias (gen_conv.hip);
    order 'reverse': one chain over k descending that starts from the bias.
    mut: drop_border_tap (every pixel of the first output row loses the tap with the largest product of output column 0),
    reflect_off_by_one, skip_last_chunk (the last split-K slice, or the last channel tile), slab_twice, accumulate_ignored."""
    _, CK, _, _, ksplit = form
    T = c.ks * c.ks
    Ho, Wo = c.out_hw
    cols, wmat = conv_cols(c, d["inp"], mut)
    pix = emu_pixels(Ho * Wo, Wo) if pix is None else pix
    cols = cols[:, :, pix].double()
    out = []
    for n in range(c.N):
        wm = wmat(d["w"][c.arena_of(n)]).double()
        cn = cols[n]
        if mut == "drop_border_tap":
            row0 = (pix < Wo).nonzero().flatten()
            kmax = (wm[0, :, None] * cn[:, row0]).abs().argmax(0)
            cn = cn.clone()
            cn[kmax, row0] = 0.0
        b = d["bias"][c.arena_of(n)].double()[:, None] if d["bias"] is not None else None
        if order == "kernel":
            cper = cdiv(cdiv(c.Cin, ksplit), CK) * CK
            slabs = []
            for s in range(ksplit):
                lo, hi = s * cper, min(c.Cin, (s + 1) * cper)
                if mut == "skip_last_chunk" and ksplit == 1:
                    hi = (cdiv(c.Cin, CK) - 1) * CK
                slabs.append(_chain(cn, wm, range(lo * T, hi * T)))
            if mut == "skip_last_chunk" and ksplit > 1:
                slabs = slabs[:-1]
            if mut == "slab_twice":
                slabs = [slabs[0]] + slabs
            if ksplit > 1:
                v = b.expand_as(slabs[0]).clone() if b is not None else torch.zeros_like(slabs[0])
                for sl in slabs:
                    v = r32(v + sl)
            else:
                v = r32(slabs[0] + b) if b is not None else slabs[0]
        else:
            assert mut is None
            start = b.expand(c.Cout, cn.shape[1]) if b is not None else None
            v = _chain(cn, wm, range(c.Cin * T - 1, -1, -1), start)
        if c.act:
            v = torch.sigmoid(v.to(F32)).double()
        if c.accumulate and mut != "accumulate_ignored":
            v = r32(d["prev"][n].reshape(c.Cout, -1)[:, pix].double() + v)
        out.append(v)
    return torch.stack(out)


def conv_mutations(c, form):
    m = ["drop_border_tap", "skip_last_chunk"]
    if c.reflect:
        m.append("reflect_off_by_one")
    if form[4] > 1:
        m.append("slab_twice")
    if c.accumulate:
        m.append("accumulate_ignored")
    return m


def _both(name, *a, **k):
    return [ConvCase(name, *a, **k), ConvCase(name + "_T", *a, transposed=1, **k)]


CONV_CASES = (
    _both("k1_ck16", 20, 4, 9, 11, 1, form=None) + [ConvCase("k1_ck16_fwd_form", 20, 4, 9, 11, 1, form=(0, 16, 1, 1, 1))] +
    _both("k1_ck16_concat", 20, 4, 9, 11, 1, concat=1) +
    _both("k1_ck32_concat", 67, 19, 17, 13, 1, concat=1) + [ConvCase("k1_ck32", 67, 19, 17, 13, 1, form=(0, 32, 2, 1, 1))] +
    [ConvCase("head_sigmoid", 16, 3, 15, 17, 1, act=1, form=(0, 16, 1, 1, 1))] +
    _both("k3_ck4_s2_odd", 3, 16, 31, 29, 3, 2, form=(0, 4, 1, 1, 1)) + _both("k3_ck4_s2_even", 3, 16, 32, 30, 3, 2, form=(0, 4, 1, 1, 1), concat=1) +
    [ConvCase("k3_ck8_splitk4_ng2", 32, 16, 14, 14, 3, ws=1, form=(0, 8, 1, 2, 4)), ConvCase("k3_ck8_nosplit_ng2", 32, 16, 14, 14, 3, form=(0, 8, 1, 2, 1)),
     ConvCase("k3_ck8_splitk4_acc", 32, 16, 14, 14, 3, ws=1, accumulate=1, concat=1, form=(0, 8, 1, 2, 4)),
     ConvCase("k3_ck8_nosplit_acc", 32, 16, 14, 14, 3, accumulate=1, form=(0, 8, 1, 2, 1)),
     ConvCase("k3_ck8_T_splitk", 32, 16, 14, 14, 3, ws=1, transposed=1, form=(0, 4, 2, 1, 4)),
     ConvCase("k3_ck8_T_red32_splitk_acc", 16, 32, 14, 14, 3, ws=1, transposed=1, accumulate=1, form=(0, 8, 1, 2, 4)),
     ConvCase("k3_ck8_fn2_splitk", 32, 24, 14, 14, 3, ws=1, form=(0, 8, 2, 2, 4)),
     ConvCase("k3_ck4_batched_fn2", 8, 64, 8, 8, 3, N=4, form=(0, 4, 2, 1, 1))] +
    _both("k3_big_fn2", 4, 20, 600, 60, 3, big=1) + _both("k3_big_fn4", 4, 33, 600, 60, 3, big=1) +
    [ConvCase("k3_big_fn2_form", 4, 20, 600, 60, 3, form=(0, 4, 2, 1, 1), big=1, accumulate=1),
     ConvCase("k3_big_ck8_ng1", 32, 64, 600, 60, 3, form=(0, 8, 4, 1, 1), big=1)] +
    [ConvCase("tile_ck4_fn2", 5, 19, 157, 257, 3, form=(1, 4, 2, 1, 1), big=1), ConvCase("tile_ck4_fn2_reflect", 5, 19, 157, 257, 3, reflect=1, form=(1, 4, 2, 1, 1), big=1),
     ConvCase("tile_ck4_fn2_T", 5, 19, 157, 257, 3, transposed=1, form=(1, 4, 1, 1, 1), big=1),
     ConvCase("tile_ck4_fn2_acc_concat", 5, 19, 157, 257, 3, accumulate=1, concat=1, form=(1, 4, 2, 1, 1), big=1),
     ConvCase("tile_ck4_fn2_N2", 5, 19, 157, 257, 3, N=2, form=(1, 4, 2, 1, 1), big=1),
     ConvCase("tile_ck8_fn1", 33, 7, 157, 257, 3, form=(1, 8, 1, 1, 1), big=1), ConvCase("tile_ck8_fn1_reflect", 33, 7, 157, 257, 3, reflect=1, form=(1, 8, 1, 1, 1), big=1),
     ConvCase("tile_ck8_fn1_acc_N2", 33, 7, 157, 257, 3, accumulate=1, N=2, form=(1, 8, 1, 1, 1), big=1),
     ConvCase("tile_ck8_fn1_T", 33, 7, 157, 257, 3, transposed=1, form=(1, 4, 2, 1, 1), big=1),
     ConvCase("tile_ck8_T_red33_acc", 7, 33, 157, 257, 3, transposed=1, accumulate=1, form=(1, 8, 1, 1, 1), big=1)] +
    _both("k5", 5, 18, 13, 12, 5, form=(0, 4, 1, 1, 1)) + [ConvCase("k5_reflect", 5, 18, 13, 12, 5, reflect=1, form=(0, 4, 1, 1, 1))] +
    _both("k7", 5, 18, 13, 12, 7, form=(0, 4, 1, 1, 1)) + [ConvCase("k7_reflect", 5, 18, 13, 12, 7, reflect=1, concat=1, form=(0, 4, 1, 1, 1))] +
    [ConvCase("k3_reflect_small", 6, 9, 11, 10, 3, reflect=1, form=(0, 4, 1, 1, 1)),
     ConvCase("k3_s2_reflect_odd", 3, 16, 31, 29, 3, 2, reflect=1, form=(0, 4, 1, 1, 1)), ConvCase("k3_s2_reflect_even_ck8", 32, 16, 14, 16, 3, 2, reflect=1, ws=1, form=(0, 8, 1, 2, 4))]
)
# conv_reflect_dgrad_launch: reflect + transposed; 4 x 5 at 7 x 7: the top and the bottom mirror of a row land on the same pixels
REFLECT_DGRAD_CASES = [ConvCase("rd_k3", 5, 6, 13, 12, 3, reflect=1, transposed=1), ConvCase("rd_k5", 5, 6, 13, 12, 5, reflect=1, transposed=1),
                       ConvCase("rd_k7", 5, 6, 13, 12, 7, reflect=1, transposed=1), ConvCase("rd_k7_4x5", 3, 4, 4, 5, 7, reflect=1, transposed=1),
                       ConvCase("rd_k3_acc_concat", 5, 6, 13, 12, 3, reflect=1, transposed=1, accumulate=1, concat=1),
                       ConvCase("rd_k7_4x5_acc_N2", 3, 4, 4, 5, 7, reflect=1, transposed=1, accumulate=1, N=2),
                       ConvCase("rd_k3_s2_odd", 5, 6, 13, 11, 3, 2, reflect=1, transposed=1), ConvCase("rd_k3_s2_even", 5, 6, 14, 12, 3, 2, reflect=1, transposed=1)]
# independent parameter arenas: every image against its own N = 1 call, bit for bit
ARENA_CASES = [ConvCase(f"{n}_{tag}", *a, N=N, arenas=2, group=grp, **k)
               for n, a, k in (("ar_k1", (20, 4, 9, 11, 1), {}), ("ar_k3_splitk", (32, 16, 14, 14, 3), dict(ws=1)), ("ar_k5", (5, 18, 13, 12, 5), {}),
                               ("ar_k3_T", (32, 16, 14, 14, 3), dict(transposed=1)), ("ar_tile", (5, 19, 157, 257, 3), dict(big=1)))
               for tag, N, grp in (("N2", 2, 1), ("N4_group2", 4, 2))]


# ---- the data gradient of a reflection-padded convolution: transposed convolution on the padded domain + mirror fold
def fold_rows(n, p, off=0):
    """padded rows that fold into interior row y (reflect_fold_kernel): itself, its top mirror, its bottom mirror"""
    rows = []
    for y in range(n):
        r = [y + p]
        if 1 <= y <= p:
            r.append(p - y + off)
        if n - 1 - p <= y <= n - 2:
            r.append(p + 2 * (n - 1) - y)
        rows.append(r)
    return rows


def reflect_dgrad_emulate(c, d, order="kernel", mut=None):
    """c: a reflect + transposed case.  The padded-domain data gradient as conv_emulate runs it (pad 0, plane (H + 2p) x (W + 2p)), then
    the fold: up to 3 x 3 sources per pixel added in the kernel's order ('reverse': rows and columns descending).  -> [N][Ci][H][W]"""
    p = c.pad
    cp = ConvCase(c.name, c.Ci, c.Co, c.H + 2 * p, c.W + 2 * p, c.ks, c.stride, transposed=1, N=c.N, arenas=c.arenas, group=c.group)
    cp.pad = 0
    cp.Ho, cp.Wo = c.Ho, c.Wo
    cp.in_hw = (c.Ho, c.Wo)
    form = conv_policy(cp)
    Hp, Wp = cp.out_hw
    inner_mut = mut if mut in ("drop_border_tap", "skip_last_chunk") else None
    dpad = conv_emulate(cp, dict(inp=d["inp"], w=d["w"], bias=None, prev=None), form, order, inner_mut, pix=torch.arange(Hp * Wp)).reshape(c.N, c.Ci, Hp, Wp)
    off = 1 if mut == "reflect_off_by_one" else 0
    ry, rx = fold_rows(c.H, p, off), fold_rows(c.W, p, off)
    out = torch.zeros(c.N, c.Ci, c.H, c.W, dtype=F64)
    for y in range(c.H):
        for x in range(c.W):
            ys, xs = (ry[y], rx[x]) if order == "kernel" else (ry[y][::-1], rx[x][::-1])
            acc = torch.zeros(c.N, c.Ci, dtype=F64)
            for a in ys:
                for b in xs:
                    acc = r32(acc + dpad[:, :, a, b])
            out[:, :, y, x] = acc
    if c.accumulate and mut != "accumulate_ignored":
        out = r32(d["prev"].double() + out)
    return out


# ================================================================================================ pointwise
def up_ref(x, Ho, Wo):
    """x2 bilinear, align_corners=False, the top-left Ho x Wo window"""
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)[..., :Ho, :Wo]


def up_bound(x, Ho, Wo):
    """product, add, product, add on every path, weights exact and positive"""
    return (g(4) * up_ref(x.double().abs(), Ho, Wo)).clamp(min=1e-300)


def up_adjoint_ref(dout, h, w):
    z = torch.zeros(dout.shape[0], dout.shape[1], h, w, dtype=F64, requires_grad=True)
    return torch.autograd.grad(up_ref(z, dout.shape[2], dout.shape[3]), z, dout.double())[0]


def up_adjoint_bound(dout, h, w):
    """two products and at most 4 + 4 adds on a path (row sums of 4 taps, then 4 rows)"""
    return (g(10) * up_adjoint_ref(dout.double().abs(), h, w)).clamp(min=1e-300)


def _up_coord(o, n):
    src = ((o.to(F32) + 0.5) * 0.5 - 0.5).clamp(min=0)
    i0 = src.to(torch.int64)
    return i0, (i0 + 1).clamp(max=n - 1), (src - i0.to(F32))


def up_emulate(x, Ho, Wo, order="kernel"):
    """fp32, every operation rounded.  'kernel': rows of columns, top (1 - ly) + bot ly (up_value); 'columns': columns of rows"""
    x = x.to(F32)
    h, w = x.shape[-2:]
    y0, y1, ly = _up_coord(torch.arange(Ho), h)
    x0, x1, lx = _up_coord(torch.arange(Wo), w)
    ly = ly[:, None]
    if order == "kernel":
        top = x[..., y0, :][..., x0] * (1 - lx) + x[..., y0, :][..., x1] * lx
        bot = x[..., y1, :][..., x0] * (1 - lx) + x[..., y1, :][..., x1] * lx
        return top * (1 - ly) + bot * ly
    left = x[..., y0, :][..., x0] * (1 - ly) + x[..., y1, :][..., x0] * ly
    right = x[..., y0, :][..., x1] * (1 - ly) + x[..., y1, :][..., x1] * ly
    return left * (1 - lx) + right * lx


def _adj_w(m, n, No, swap=False):
    wt = [0.25 if m > 0 else 0.0, 0.75 if m > 0 else 1.0, 0.75 if m < n - 1 else 1.0, 0.25 if m < n - 1 else 0.0]
    if swap and m == n - 1:   # the deliberate error: 1/4 and 3/4 exchanged at the far border
        wt[0], wt[1] = wt[1], wt[0]
    return [0.0 if 2 * m - 1 + t >= No else wt[t] for t in range(4)]


def up_adjoint_emulate(dout, h, w, order="kernel", mut=None):
    """'kernel': up_adjoint_value's 16 clamped taps, row sums first, fp32 throughout; 'autograd': fp32 autograd of up_emulate.
    mut 'swap_border_weights'"""
    dout = dout.to(F32)
    Ho, Wo = dout.shape[-2:]
    if order != "kernel":
        z = torch.zeros(*dout.shape[:2], h, w, requires_grad=True)
        return torch.autograd.grad(up_emulate(z, Ho, Wo), z, dout)[0]
    out = torch.zeros(*dout.shape[:2], h, w)
    swap = mut == "swap_border_weights"
    for my in range(h):
        wy = _adj_w(my, h, Ho, swap)
        for mx in range(w):
            wx = _adj_w(mx, w, Wo, swap)
            acc = torch.zeros(dout.shape[:2])
            for ty in range(4):
                oy = min(max(2 * my - 1 + ty, 0), Ho - 1)
                row = torch.zeros(dout.shape[:2])
                for tx in range(4):
                    if wx[tx] != 0.0:
                        row = row + wx[tx] * dout[..., oy, min(max(2 * mx - 1 + tx, 0), Wo - 1)]
                if wy[ty] != 0.0:
                    acc = acc + wy[ty] * row
            out[..., my, mx] = acc
    return out


def plane_blocks(HW):
    return max(1, min(64, cdiv(HW, 512)))


def sigmoid_bwd_ref(dout, s):
    """dpre = dout s (1 - s) and its bound: the rounding of 1 - s and two products"""
    dpre = dout.double() * s.double() * (1 - s.double())
    return dpre, (g(3) * dpre.abs()).clamp(min=1e-300)


def sigmoid_bias_segments(N, HW, group):
    """(first image, images, lo, hi) of every partial in the launcher's order [image group][segment]; group = 0: one group of all N"""
    per = N if group == 0 else group
    PB = plane_blocks(HW)
    seg = cdiv(HW, PB)
    return [(n0, per, pb * seg, min((pb + 1) * seg, HW)) for n0 in range(0, N, per) for pb in range(PB)]


def sigmoid_bias_ref(dpre, segs):
    """per-partial fp64 sums [len(segs)][C] and bounds: a segment's n values in any order, behind the 3 roundings of each value"""
    ref = torch.stack([dpre[n0:n0 + per, :, lo:hi].sum((0, 2)) for n0, per, lo, hi in segs])
    mag = torch.stack([dpre[n0:n0 + per, :, lo:hi].abs().sum((0, 2)) for n0, per, lo, hi in segs])
    k = max(per * (hi - lo) for _, per, lo, hi in segs) + 3
    return ref, (g(k) * mag).clamp(min=1e-300)


def sigmoid_bwd_emulate(dout, s, segs, order="kernel", mut=None):
    """fp32 dpre and partials.  'kernel': a thread's strided run, then the tree (here: 256 strided chains, then torch's fp32 sum);
    'flat': torch's fp32 sum over the segment.  mut 'skip_last_segment': the ragged last segment of every group is not summed"""
    dout, s = dout.to(F32), s.to(F32)
    dpre = dout * s * (1 - s)
    parts = []
    last_lo = max(lo for _, _, lo, _ in segs)
    for n0, per, lo, hi in segs:
        v = dpre[n0:n0 + per, :, lo:hi]
        if mut == "skip_last_segment" and lo == last_lo:
            v = v[:, :, :0]
        if order == "kernel":
            acc = torch.zeros(v.shape[1], 256)
            for n in range(v.shape[0]):
                for i in range(0, v.shape[2], 256):
                    blk = v[n, :, i:i + 256]
                    acc[:, :blk.shape[1]] += blk
            parts.append(acc.sum(1))
        else:
            parts.append(v.sum((0, 2)))
    return dpre, torch.stack(parts)


# ================================================================================================ BatchNorm (+ LeakyReLU)
BN_DEPTH = 64          # additions on any path of a plain plane sum (see the module docstring)
BN_CHAN = 48           # roundings of the pairwise merges of segment statistics
BN_EPS = 1e-5
SIGN_SHARE_CAP = 1e-3  # share of a plane whose pre-activation may lie inside its own forward bound
SMALL, MID, TWO_STAGE, TWO_STAGE_VEC = 0, 1, 2, 3


def bn_plane_blocks(HW):
    """segments of a two-stage plane (bn_plane_blocks / plane_blocks of the kernels)"""
    if not (HW > 64 * 1024 and HW <= 256 * 5 * 1024):
        return plane_blocks(HW)
    b = cdiv(HW, 4096)
    return 65 if b <= 64 else min(b, 256)


def bn_seg_len(HW, PB):
    s = cdiv(HW, PB)
    return (s + 3) // 4 * 4 if PB > 64 else s


def bn_form(HW, N, p_nstride, batch):
    """bn_form of gen_bn.hip restated (environment switches unset): (kind, hosts_pre, fwd_takes_slabs, bwd_takes_slabs, fwd_fuses_upsample,
    bwd_fuses_upsample, sign_from_y)"""
    own = (not batch) and (N == 1 or p_nstride > 0)
    kind = SMALL if HW <= 4096 else MID if (HW <= 16384 and own) else TWO_STAGE_VEC if bn_plane_blocks(HW) > 64 else TWO_STAGE
    one = kind in (SMALL, MID)
    return (kind, int(own and one), int(kind == SMALL and not batch), int(kind == SMALL and own), int(not batch), int((not batch) and one),
            int((not batch) and kind == TWO_STAGE_VEC))


class BnCase:
    """One BatchNorm launch pair (forward, backward) on [N][C][HW].  batch: images per statistics group (0: per image); arenas: 1 = every
    image / group has its own gamma / beta (p_nstride); up = (h, w, Ho, Wo, c0): channels >= c0 are an upsampling; slabs: forward split-K
    slices; da_slabs = (slices, accumulate); pre = (channels, slices of the skip convolution or 0); acc: dgamma / dbeta accumulate."""

    def __init__(self, name, C, HW, kind, N=1, batch=0, arenas=0, slope=0.2, up=None, slabs=0, da_slabs=None, pre=None, acc=0):
        self.name, self.C, self.HW, self.kind, self.N, self.batch, self.arenas, self.slope = name, C, HW, kind, N, batch, arenas, slope
        self.up, self.slabs, self.da_slabs, self.pre, self.acc = up, slabs, da_slabs, pre, acc
        self.groups = [list(range(n0, n0 + batch)) for n0 in range(0, N, batch)] if batch else [[n] for n in range(N)]
        # parameter sets: one per group / image with arenas, else one
        self.n_par = len(self.groups) if arenas else 1

    def __repr__(self):
        return self.name

    def par_of(self, img):
        return (img // self.batch if self.batch else img) if self.arenas else 0

    @property
    def form(self):
        return bn_form(self.HW, self.N, 1 if self.arenas else 0, self.batch)


def bn_inputs(c):
    """fp32 operands, seeded: continuous inputs (noise on a per-channel offset and a ramp along the plane, so that every part of a plane
    matters to its statistics), |gamma| in [0.5, 1.5], |beta| in [0.1, 0.6] with both signs, da with a non-zero mean"""
    gen = _gen("bn", c.name)
    ramp = torch.linspace(0, 1, c.HW)
    y = torch.randn(c.N, c.C, c.HW, generator=gen) * (0.5 + torch.rand(1, c.C, 1, generator=gen)) + torch.randn(1, c.C, 1, generator=gen) + 0.7 * ramp
    sg = lambda *s: (torch.randint(2, s, generator=gen) * 2 - 1).float()
    gamma = sg(c.n_par, c.C) * (0.5 + torch.rand(c.n_par, c.C, generator=gen))
    beta = sg(c.n_par, c.C) * (0.1 + 0.5 * torch.rand(c.n_par, c.C, generator=gen))
    da = torch.randn(c.N, c.C, c.HW, generator=gen) + 0.3 - 0.5 * ramp
    d = dict(y=y, gamma=gamma, beta=beta, da=da, prev_dg=torch.randn(c.n_par, c.C, generator=gen), prev_db=torch.randn(c.n_par, c.C, generator=gen))
    if c.up:
        h, w, Ho, Wo, c0 = c.up
        d["src"] = torch.randn(c.N, c.C - c0, h, w, generator=gen) + 0.4
    if c.slabs:
        d["slabs"] = torch.randn(c.slabs, c.N, c.C, c.HW, generator=gen) / math.sqrt(c.slabs) + (0.7 * ramp + 0.2) / c.slabs
        d["bias"] = torch.randn(c.n_par, c.C, generator=gen) * 0.5
    if c.da_slabs:
        d["da_slabs"] = torch.randn(c.da_slabs[0], c.N, c.C, c.HW, generator=gen) / math.sqrt(c.da_slabs[0]) + 0.1
    if c.pre:
        pc, ps = c.pre
        d["pre_y"] = torch.randn(c.N, pc, c.HW, generator=gen) * 0.8 + 0.3 + 0.7 * ramp
        d["pre_gamma"] = sg(c.n_par, pc) * (0.5 + torch.rand(c.n_par, pc, generator=gen))
        d["pre_beta"] = sg(c.n_par, pc) * (0.1 + 0.5 * torch.rand(c.n_par, pc, generator=gen))
        if ps:
            d["pre_slabs"] = torch.randn(ps, c.N, pc, c.HW, generator=gen) / math.sqrt(ps) + (0.7 * ramp + 0.1) / ps
            d["pre_bias"] = torch.randn(c.n_par, pc, generator=gen) * 0.5
    return d


def slab_sum_f32(start, slabs, twice=False):
    """((start + s_0) + s_1) + ... in fp32: the order of every slab sum of the generator (bit-exact prediction)"""
    v = start.to(F32).clone()
    for k in range(slabs.shape[0]):
        v = v + slabs[k].to(F32)
        if twice and k == 0:
            v = v + slabs[k].to(F32)
    return v


def lrelu(t, slope):
    return torch.where(t > 0, t, t * slope)


def _per_img(c, p):
    """parameters [n_par][C] -> [N][C][1] by image"""
    return torch.stack([p[c.par_of(n)] for n in range(c.N)])[:, :, None]


def bn_fwd_ref(c, y, gamma, beta, slope=None, E_y=None):
    """fp64 forward of the groups of case c on input y [N][C'][HW] (+ its element bound).  y may carry an input error E_y (an upsampled or
    pre-normalised channel the kernel forms itself).  Derivation, per statistics group of n values, A = mean |y|:
        mean   E_m = g(BN_DEPTH + BN_CHAN / 2 + 1) A + mean(E_y)
        var    E_v = g(BN_DEPTH + BN_CHAN + 3) v + 2 mean(|y - m| E_y) + E_m^2     (d = y - m rounds once, d^2 twice more, then the tree)
        rstd   r = (v + eps)^-1/2, dr/dv = -r^3 / 2:  E_r = r^3 / 2 (E_v + 2 U (v + eps)) + 2 U r    (division, add; rsqrt and its store)
        t      = y sc + sh, sc = gamma r, sh = beta - m sc:
               E_t = |gamma| r (E_m + E_y) + |y - m| |gamma| E_r + U (2 |y sc| + 2 |m sc| + |sh| + |t|)
        out    = LeakyReLU(t), Lipschitz 1 and continuous across the kink: E_out = E_t + U |out|"""
    slope = c.slope if slope is None else slope
    y = y.double()
    E_y = torch.zeros_like(y) if E_y is None else E_y
    Cc = y.shape[1]
    m, v, E_m, E_v = (torch.zeros(c.N, Cc, dtype=F64) for _ in range(4))
    for grp in c.groups:
        yg, eg = y[grp], E_y[grp]
        mg = yg.mean((0, 2))
        vg = ((yg - mg[None, :, None]) ** 2).mean((0, 2))
        Em = g(BN_DEPTH + BN_CHAN // 2 + 1) * yg.abs().mean((0, 2)) + eg.mean((0, 2))
        Ev = g(BN_DEPTH + BN_CHAN + 3) * vg + 2 * ((yg - mg[None, :, None]).abs() * eg).mean((0, 2)) + Em ** 2
        m[grp], v[grp], E_m[grp], E_v[grp] = mg, vg, Em, Ev
    r = (v + BN_EPS) ** -0.5
    E_r = r ** 3 / 2 * (E_v + 2 * U * (v + BN_EPS)) + 2 * U * r
    ga, be = _per_img(c, gamma.double()), _per_img(c, beta.double())
    M, R = m[:, :, None], r[:, :, None]
    sc = ga * R
    sh = be - M * sc
    t = (y - M) * sc + be
    out = lrelu(t, slope)
    E_t = ga.abs() * R * (E_m[:, :, None] + E_y) + (y - M).abs() * ga.abs() * E_r[:, :, None] + U * (2 * (y * sc).abs() + 2 * (M * sc).abs() + sh.abs() + t.abs())
    E_out = E_t + U * out.abs()
    tiny = 1e-300
    return dict(mean=m, rstd=r, t=t, out=out, E_mean=E_m.clamp(min=tiny), E_rstd=E_r.clamp(min=tiny), E_t=E_t.clamp(min=tiny), E_out=E_out.clamp(min=tiny))


def bn_bwd_ref(c, da, pos, y, m, r, gamma, slope=None, E_da=None, amb=None, prev=None, par_groups=True):
    """fp64 closed form of the backward on the kernel's own inputs -- da, the sign of the stored activation (pos), y, the saved fp32 mean /
    rstd -- and the element bounds (tests/test_gen_ops_cpu.py checks the closed form against autograd):
        dz = da (pos ? 1 : slope);  xh = (y - m) r;  s1 = sum dz;  s2 = sum dz xh  (over the statistics group, n values)
        dy = gamma r (dz - s1 / n - xh s2 / n);  dgamma = sum s2;  dbeta = sum s1  (over the groups that share the parameters)
    Derivation: e_dz = U |dz| (the slope product) + E_da;  e_xh = 2 U |xh|;
        E_s1 = g(BN_DEPTH + 2) sum |dz| + sum e_dz;    E_s2 = g(BN_DEPTH + 3) sum |dz xh| + sum (e_dz |xh| + |dz| e_xh)
        k = s / n:  E_k = E_s / n + U |k|
        E_dy = |gamma r| (e_dz + E_k1 + U |dz - k1| + |k2| e_xh + |xh| E_k2 + U |xh k2| + U |dz - k1 - xh k2|) + 2 U |dy|
        E_dgamma = sum E_s2 + g(groups + 1) (sum |s2| + |prev|), dbeta alike.
    amb [N][C][HW] bool: elements whose sign the kernel decides itself and may decide either way; each adds |da| (1 - slope) to E_s1 and
    |da xh| (1 - slope) to E_s2, and dy_alt holds their other branch.  prev = (dgamma, dbeta) [n_par][C] under accumulate."""
    slope = c.slope if slope is None else slope
    da, y = da.double(), y.double()
    Cc = y.shape[1]
    E_da = torch.zeros_like(da) if E_da is None else E_da
    ga = _per_img(c, gamma.double())
    M, R = m.double()[:, :, None], r.double()[:, :, None]
    fac = torch.where(pos, torch.ones_like(da), torch.full_like(da, slope))
    dz, xh = da * fac, (y - M) * R
    e_dz = (U * dz.abs() if slope != 1 else 0) + E_da
    e_xh = 2 * U * xh.abs()
    flip = (da * (1 - slope)).abs() * amb if amb is not None else torch.zeros_like(da)
    k1, k2, E_k1, E_k2 = (torch.zeros(c.N, Cc, 1, dtype=F64) for _ in range(4))
    s1g, s2g, E1g, E2g = [], [], [], []
    for grp in c.groups:
        n = len(grp) * y.shape[2]
        s1, s2 = dz[grp].sum((0, 2)), (dz[grp] * xh[grp]).sum((0, 2))
        E1 = g(BN_DEPTH + 2) * dz[grp].abs().sum((0, 2)) + (e_dz[grp] + flip[grp]).sum((0, 2))
        E2 = g(BN_DEPTH + 3) * (dz[grp] * xh[grp]).abs().sum((0, 2)) + ((e_dz[grp] + flip[grp]) * xh[grp].abs() + dz[grp].abs() * e_xh[grp]).sum((0, 2))
        k1[grp], k2[grp] = (s1 / n)[None, :, None], (s2 / n)[None, :, None]
        E_k1[grp], E_k2[grp] = (E1 / n + U * (s1 / n).abs())[None, :, None], (E2 / n + U * (s2 / n).abs())[None, :, None]
        s1g.append(s1); s2g.append(s2); E1g.append(E1); E2g.append(E2)
    gr = ga * R
    dy = gr * (dz - k1 - xh * k2)
    E_dy = gr.abs() * (e_dz + E_k1 + U * (dz - k1).abs() + k2.abs() * e_xh + xh.abs() * E_k2 + U * (xh * k2).abs() + U * (dz - k1 - xh * k2).abs()) + 2 * U * dy.abs()
    dy_alt = gr * (da * (1 + slope - fac) - k1 - xh * k2)
    # parameter gradients: the groups that share a parameter set, in group order
    s1g, s2g, E1g, E2g = (torch.stack(t) for t in (s1g, s2g, E1g, E2g))
    if c.arenas and par_groups:
        dg, db, E_dg, E_db, cnt = s2g, s1g, E2g, E1g, 1
        mg, mb = s2g.abs(), s1g.abs()
    else:
        dg, db, E_dg, E_db, cnt = s2g.sum(0, keepdim=True), s1g.sum(0, keepdim=True), E2g.sum(0, keepdim=True), E1g.sum(0, keepdim=True), len(c.groups)
        mg, mb = s2g.abs().sum(0, keepdim=True), s1g.abs().sum(0, keepdim=True)
    if prev is not None:
        dg, db, mg, mb = prev[0].double() + dg, prev[1].double() + db, mg + prev[0].double().abs(), mb + prev[1].double().abs()
    E_dg, E_db = E_dg + g(cnt + 1) * mg, E_db + g(cnt + 1) * mb
    tiny = 1e-300
    return dict(dy=dy, dy_alt=dy_alt, dgamma=dg, dbeta=db, E_dy=E_dy.clamp(min=tiny), E_dgamma=E_dg.clamp(min=tiny), E_dbeta=E_db.clamp(min=tiny))


def bn_dy_ratio(got, b, amb=None):
    """worst err / bound of dy; ambiguous elements against the nearer of their two branches"""
    err = (got.double() - b["dy"]).abs()
    if amb is not None:
        err = torch.where(amb, torch.minimum(err, (got.double() - b["dy_alt"]).abs()), err)
    return (err / b["E_dy"]).max().item()


def _tree_sum(parts):
    """adjacent pairs, level by level, fp32"""
    parts = list(parts)
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
    return parts[0]


def _segments(c, HW):
    PB = bn_plane_blocks(HW) if c.kind >= TWO_STAGE else 1
    seg = bn_seg_len(HW, PB)
    return [(lo, min(lo + seg, HW)) for lo in range(0, HW, seg)]


def bn_skip_tail(c, HW):
    """what the 'skip_tail' error leaves out of every reduction: the last (ragged) segment of a two-stage plane, else the plane's last
    ragged run of 256 (None: the plane has no such piece)"""
    segs = _segments(c, HW)
    if len(segs) > 1:
        return segs[-1][0]
    if HW > 256 and HW % 256:
        return HW - HW % 256
    return HW - 1 if HW > 1 else None


def bn_fwd_emulate(c, y, gamma, beta, slope=None, order="segments", mut=None):
    """fp32 forward on the fp32 input y [N][C'][HW] -> (mean, rstd, out).  'segments': per-segment mean and M2 (two-pass inside the segment),
    merged pairwise (Chan), the images of a batch in order; 'flat': torch's fp32 mean / two-pass variance over the whole group.
    mut: unbiased_var, skip_tail"""
    slope = c.slope if slope is None else slope
    y = y.to(F32)
    HW, Cc = y.shape[2], y.shape[1]
    cut = bn_skip_tail(c, HW) if mut == "skip_tail" else None
    m, r = torch.zeros(c.N, Cc), torch.zeros(c.N, Cc)
    for grp in c.groups:
        yg = y[grp] if cut is None else y[grp][:, :, :cut]
        n = yg.shape[0] * yg.shape[2]
        if order == "flat":
            mg = yg.sum((0, 2)) / n
            M2 = ((yg - mg[None, :, None]) ** 2).sum((0, 2))
        else:
            stats = []
            for i in range(yg.shape[0]):
                for lo, hi in _segments(c, HW):
                    s = yg[i, :, lo:hi]
                    if s.shape[1]:
                        ms = s.sum(1) / s.shape[1]
                        stats.append((float(s.shape[1]), ms, ((s - ms[:, None]) ** 2).sum(1)))
            while len(stats) > 1:
                nxt = []
                for i in range(0, len(stats), 2):
                    if i + 1 == len(stats):
                        nxt.append(stats[i])
                        continue
                    (na, ma, Ma), (nb, mb, Mb) = stats[i], stats[i + 1]
                    d, w = mb - ma, nb / (na + nb)
                    nxt.append((na + nb, ma + d * w, Ma + (Mb + d * d * (na * w))))
                stats = nxt
            _, mg, M2 = stats[0]
        var = M2 / ((n - 1) if mut == "unbiased_var" else n)
        m[grp], r[grp] = mg, torch.rsqrt(var + BN_EPS)
    ga, be = _per_img(c, gamma.to(F32)), _per_img(c, beta.to(F32))
    sc = ga * r[:, :, None]
    sh = be - m[:, :, None] * sc
    return m, r, lrelu(y * sc + sh, slope)


def bn_bwd_emulate(c, da, pos, y, m, r, gamma, slope=None, order="segments", mut=None, prev=None, par_groups=True):
    """fp32 backward -> (dy, dgamma, dbeta).  'segments': per-segment sums, then the segments and the images in order; 'flat': torch's sums.
    mut: skip_tail, missing_mean_dz, accumulate_ignored"""
    slope = c.slope if slope is None else slope
    da, y, m, r = da.to(F32), y.to(F32), m.to(F32)[:, :, None], r.to(F32)[:, :, None]
    HW, Cc = y.shape[2], y.shape[1]
    dz = torch.where(pos, da, da * slope) if slope != 1 else da
    xh = (y - m) * r
    cut = bn_skip_tail(c, HW) if mut == "skip_tail" else HW
    k1, k2 = torch.zeros(c.N, Cc, 1), torch.zeros(c.N, Cc, 1)
    s1g, s2g = [], []
    for grp in c.groups:
        a, b = dz[grp][:, :, :cut], (dz[grp] * xh[grp])[:, :, :cut]
        if order == "flat":
            s1, s2 = a.sum((0, 2)), b.sum((0, 2))
        else:
            s1 = _tree_sum([_tree_sum([a[i, :, lo:hi].sum(1) for lo, hi in _segments(c, HW) if lo < cut]) for i in range(len(grp))])
            s2 = _tree_sum([_tree_sum([b[i, :, lo:hi].sum(1) for lo, hi in _segments(c, HW) if lo < cut]) for i in range(len(grp))])
        n = float(len(grp) * HW)
        k1[grp], k2[grp] = (torch.zeros_like(s1) if mut == "missing_mean_dz" else s1 / n)[None, :, None], (s2 / n)[None, :, None]
        s1g.append(s1); s2g.append(s2)
    gr = _per_img(c, gamma.to(F32)) * r
    dy = gr * ((dz - k1) - xh * k2)
    s1g, s2g = torch.stack(s1g), torch.stack(s2g)
    if not (c.arenas and par_groups):
        acc1, acc2 = torch.zeros(Cc), torch.zeros(Cc)
        for i in range(s1g.shape[0]):
            acc1, acc2 = acc1 + s1g[i], acc2 + s2g[i]
        s1g, s2g = acc1[None], acc2[None]
    if prev is not None and mut != "accumulate_ignored":
        s2g, s1g = prev[0].to(F32) + s2g, prev[1].to(F32) + s1g
    return dy, s2g, s1g


_SMALL_HW = [1, 4, 255, 256, 257, 1024, 1025, 4095, 4096]
BN_CASES = (
    [BnCase(f"small_{HW}", 2 + i % 4, HW, SMALL, slope=0.2 if i % 2 == 0 else 1.0) for i, HW in enumerate(_SMALL_HW)] +
    [BnCase(f"small_{HW}_{tag}", 3, HW, SMALL, **k) for HW in (4, 257, 4096)
     for tag, k in (("N2_shared", dict(N=2)), ("N2_arenas", dict(N=2, arenas=1)), ("batch2", dict(N=2, batch=2)), ("batch2_N4_arenas", dict(N=4, batch=2, arenas=1)))] +
    [BnCase(f"mid_{HW}", 2 + i, HW, MID, slope=0.2 if i != 1 else 1.0) for i, HW in enumerate((4097, 16383, 16384))] +
    [BnCase(f"mid_{HW}_N2_arenas", 2, HW, MID, N=2, arenas=1) for HW in (4097, 16384)] +
    [BnCase("two_4097_N2_shared", 3, 4097, TWO_STAGE, N=2), BnCase("two_16385", 2, 16385, TWO_STAGE), BnCase("two_33001_64seg", 2, 33001, TWO_STAGE),
     BnCase("two_33001_slope1", 2, 33001, TWO_STAGE, slope=1.0), BnCase("two_4097_batch2", 2, 4097, TWO_STAGE, N=2, batch=2),
     BnCase("two_4097_batch2_N4_arenas", 2, 4097, TWO_STAGE, N=4, batch=2, arenas=1), BnCase("mid_5000_N2_arenas_acc", 2, 5000, MID, N=2, arenas=1, acc=1)] +
    [BnCase("vec_65537_65seg", 3, 65537, TWO_STAGE_VEC), BnCase("vec_65537_slope1", 2, 65537, TWO_STAGE_VEC, slope=1.0),
     BnCase("vec_65537_N2_shared_acc", 2, 65537, TWO_STAGE_VEC, N=2, acc=1), BnCase("vec_65537_N2_arenas", 2, 65537, TWO_STAGE_VEC, N=2, arenas=1),
     BnCase("vec_262147_odd", 2, 262147, TWO_STAGE_VEC), BnCase("vec_266243_66seg", 2, 266243, TWO_STAGE_VEC),
     BnCase("vec_70001_batch2", 2, 70001, TWO_STAGE_VEC, N=2, batch=2)] +
    [BnCase("up_small_even", 4, 120, SMALL, up=(5, 6, 10, 12, 2)), BnCase("up_small_odd", 4, 99, SMALL, up=(5, 6, 9, 11, 2)),
     BnCase("up_small_bigsrc", 3, 4096, SMALL, up=(32, 64, 64, 64, 1)), BnCase("up_small_N2_shared", 3, 120, SMALL, N=2, up=(5, 6, 10, 12, 1)),
     BnCase("up_mid_even", 3, 8208, MID, up=(36, 57, 72, 114, 1)), BnCase("up_mid_odd_bigsrc", 3, 16383, MID, up=(64, 65, 127, 129, 2)),
     BnCase("up_two_even", 3, 16640, TWO_STAGE, up=(65, 64, 130, 128, 1)), BnCase("up_two_N2_shared_odd", 3, 4623, TWO_STAGE, N=2, up=(35, 34, 69, 67, 2)),
     BnCase("up_vec_even", 2, 66564, TWO_STAGE_VEC, up=(129, 129, 258, 258, 1)), BnCase("up_vec_odd_N2_shared", 2, 66049, TWO_STAGE_VEC, N=2, up=(129, 129, 257, 257, 1)),
     BnCase("up_small_batch2", 4, 120, SMALL, N=2, batch=2, up=(5, 6, 10, 12, 2)), BnCase("up_two_batch2_odd", 3, 4623, TWO_STAGE, N=2, batch=2, up=(35, 34, 69, 67, 1))] +
    [BnCase(f"slabs_k{k}", 3, 196, SMALL, slabs=k) for k in (2, 4, 5)] + [BnCase("slabs_k4_N2_arenas", 2, 1025, SMALL, N=2, arenas=1, slabs=4)] +
    [BnCase("daslabs_k4", 3, 196, SMALL, da_slabs=(4, 0)), BnCase("daslabs_k5_acc", 3, 196, SMALL, da_slabs=(5, 1)),
     BnCase("daslabs_k9_acc_N2_arenas", 2, 1025, SMALL, N=2, arenas=1, da_slabs=(9, 1), acc=1)] +
    [BnCase("pre_small", 4, 196, SMALL, pre=(2, 0)), BnCase("pre_small_slabs", 4, 196, SMALL, pre=(2, 4)), BnCase("pre_small_up_N2_arenas_acc", 5, 120, SMALL, N=2, arenas=1, pre=(2, 5), up=(5, 6, 10, 12, 3), acc=1),
     BnCase("pre_mid", 3, 4225, MID, pre=(2, 0)), BnCase("pre_mid_up_N2_arenas", 4, 8208, MID, N=2, arenas=1, pre=(2, 0), up=(36, 57, 72, 114, 3))]
)


# ================================================================================================ weight gradients
class WgradCase(ConvCase):
    """dW [Co][Ci][ks][ks] of the layer of ConvCase from x [N][Ci][H][W] and dy [N][Co][Ho][Wo].  indep: the N images are independent (a
    gradient arena each, p_nstride); acc: dW accumulates.  form = (class 0 small / 1 big / 2 tile, kernel variant, pixels per chunk, chunks,
    vectorised reduce) the case is named for."""

    def __init__(self, name, Ci, Co, H, W, ks, stride=1, wform=None, N=1, reflect=0, concat=0, indep=0, acc=0):
        super().__init__(name, Ci, Co, H, W, ks, stride, N=N, reflect=reflect, concat=concat)
        self.indep, self.acc, self.wform = indep, acc, wform


def wgrad_chunks(N, Ho, Wo):
    """wgrad_chunks of gen_wgrad.hip: (pixels per chunk, chunks per image)"""
    HWo = Ho * Wo
    ppc = 64 if HWo <= 256 else 256 if HWo <= 1024 else 512
    if HWo > 128 * 512:
        ppc = (cdiv(HWo, 128) + 63) // 64 * 64
    return ppc, cdiv(HWo, ppc)


def wgrad_tile_ok(c):
    return c.ks == 3 and c.stride == 1 and c.Wo >= 64 and c.Ho * c.Wo > 40000 and c.H == c.Ho and c.W == c.Wo and c.pad == 1


def wgrad_form(c):
    """(class, variant, pixels per chunk, chunks, vectorised reduce) as conv_wgrad_add / wgrad_reduce_all_launch decide them (buffers 16-byte
    aligned, arena stride a multiple of 4)"""
    ppc, cpi = wgrad_chunks(c.N, c.Ho, c.Wo)
    ni = cdiv(c.Co, 16)
    if wgrad_tile_ok(c):
        cls, var = 2, 1 if ni < 2 else 2
    else:
        cls = 1 if c.Co > 32 else 0
        var = {1: 0, 3: 4, 5: 8, 7: 12}[c.ks] + (0 if ni <= 1 else 1 if ni <= 2 else 2 if ni <= 4 else 3)
    return (cls, var, ppc, c.N * cpi, int((c.Co * c.Ci * c.ks * c.ks) % 4 == 0))


def wgrad_chunk_ranges(c):
    """pixel ranges [lo, hi) of an image's chunks.  Batched kernels: pix_per_chunk consecutive pixels.  Tile kernel: strips of whole
    4 x 64-pixel tiles, tile t of strip s when s T / chunks <= t < (s + 1) T / chunks -- returned as index tensors"""
    ppc, cpi = wgrad_chunks(c.N, c.Ho, c.Wo)
    L = c.Ho * c.Wo
    if not wgrad_tile_ok(c):
        return [torch.arange(lo, min(lo + ppc, L)) for lo in range(0, L, ppc)]
    tx, ty = cdiv(c.Wo, 64), cdiv(c.Ho, 4)
    T = tx * ty
    i = torch.arange(L)
    tile = (i // c.Wo // 4) * tx + (i % c.Wo) // 64
    return [i[(tile >= s * T // cpi) & (tile < (s + 1) * T // cpi)] for s in range(cpi)]


def wgrad_inputs(c):
    gen = _gen("wgrad", c.name)
    x = torch.randn(c.N, c.Ci, c.H, c.W, generator=gen) + 0.5
    dy = torch.randn(c.N, c.Co, c.Ho, c.Wo, generator=gen) + 0.25
    n_out = c.N if c.indep else 1
    prev = torch.randn(n_out, c.Co, c.Ci, c.ks, c.ks, generator=gen) * 30 if c.acc else None
    return dict(x=x, dy=dy, prev=prev)


def wgrad_ref(c, d):
    """fp64 weight gradient by autograd of the forward ([n_out][Co][Ci][ks][ks], n_out = N for independent images, else 1: the sum over the
    images), the magnitudes, and the bound: a chunk is a chain of at most its pixel count, the chunks are summed by four interleaved chains
    and one (s0 + s1) + (s2 + s3) tree; accumulate adds one rounding and |prev|"""
    x, dy = d["x"].double(), d["dy"].double()
    res = []
    for xa, da in ((x, dy), (x.abs(), dy.abs())):
        per = []
        for n in range(c.N):
            w = torch.zeros(c.Co, c.Ci, c.ks, c.ks, dtype=F64, requires_grad=True)
            xin = F.pad(xa[n:n + 1], (c.pad,) * 4, mode="reflect") if c.reflect else xa[n:n + 1]
            out = F.conv2d(xin, w, None, stride=c.stride, padding=0 if c.reflect else c.pad)
            per.append(torch.autograd.grad(out, w, da[n:n + 1])[0])
        per = torch.stack(per)
        res.append(per if c.indep else per.sum(0, keepdim=True))
    ref, S = res
    chunks = len(wgrad_chunk_ranges(c)) * (1 if c.indep else c.N)
    k = max(len(r) for r in wgrad_chunk_ranges(c)) + cdiv(chunks, 4) + 3 + (1 if c.acc else 0)
    if c.acc:
        ref, S = d["prev"].double() + ref, S + d["prev"].double().abs()
    return dict(ref=ref, E=(g(k) * S).clamp(min=1e-300))


def wgrad_emulate(c, d, order="chunks", mut=None):
    """fp32 weight gradient.  'chunks': every chunk of every image as one fp32 matrix product over its pixels, the chunks summed as
    wgrad_chunk_sum does (chains c mod 4, then (s0 + s1) + (s2 + s3)); 'flat': one fp32 matrix product over all pixels of all images.
    mut: skip_last_chunk (every image's last chunk), drop_border_tap (the first output row loses tap (ks - 1, 0)), reflect_off_by_one,
    accumulate_ignored"""
    T = c.ks * c.ks
    cols, _ = conv_cols(c, d["x"], mut)                       # [N][Ci T][L]
    if mut == "drop_border_tap":
        cols = cols.clone()
        cols[:, (c.ks - 1) * c.ks::T, :c.Wo] = 0.0
    dy = d["dy"].reshape(c.N, c.Co, -1)
    outs = []
    for imgs in ([[n] for n in range(c.N)] if c.indep else [list(range(c.N))]):
        if order == "flat":
            assert mut is None
            s = sum(dy[n] @ cols[n].T for n in imgs)
        else:
            parts = []
            for n in imgs:
                rng = wgrad_chunk_ranges(c)
                for r in (rng[:-1] if mut == "skip_last_chunk" else rng):
                    parts.append(dy[n][:, r] @ cols[n][:, r].T)
            ch = [torch.zeros(c.Co, c.Ci * T) for _ in range(4)]
            for i, p in enumerate(parts):
                ch[i % 4] = ch[i % 4] + p
            s = (ch[0] + ch[1]) + (ch[2] + ch[3])
        outs.append(s.reshape(c.Co, c.Ci, c.ks, c.ks))
    out = torch.stack(outs)
    if c.acc and mut != "accumulate_ignored":
        out = d["prev"] + out
    return out


def wgrad_mutations(c):
    return ["skip_last_chunk", "drop_border_tap"] + (["reflect_off_by_one"] if c.reflect else []) + (["accumulate_ignored"] if c.acc else [])


WGRAD_CASES = [
    WgradCase("w_k1_co4_15x17", 20, 4, 15, 17, 1, wform=(0, 0, 64, 4, 1)), WgradCase("w_k1_co24_31x33", 20, 24, 31, 33, 1, wform=(0, 1, 256, 4, 1)),
    WgradCase("w_k1_co64_15x17", 20, 64, 15, 17, 1, wform=(1, 2, 64, 4, 1)), WgradCase("w_k1_co128_31x33_concat", 20, 128, 31, 33, 1, concat=1, wform=(1, 3, 256, 4, 1)),
    WgradCase("w_k3_co16_31x33", 5, 16, 31, 33, 3, wform=(0, 4, 256, 4, 1)), WgradCase("w_k3_co24_45x47_ragged", 6, 24, 45, 47, 3, wform=(0, 5, 512, 5, 1)),
    WgradCase("w_k3_co64_15x17", 8, 64, 15, 17, 3, wform=(1, 6, 64, 4, 1)), WgradCase("w_k3_co128_15x17", 4, 128, 15, 17, 3, wform=(1, 7, 64, 4, 1)),
    WgradCase("w_k5_co4_15x17", 5, 4, 15, 17, 5, wform=(0, 8, 64, 4, 1)), WgradCase("w_k5_co24_15x17", 5, 24, 15, 17, 5, wform=(0, 9, 64, 4, 1)),
    WgradCase("w_k5_co64_31x33", 5, 64, 31, 33, 5, wform=(1, 10, 256, 4, 1)), WgradCase("w_k5_co128_15x17", 4, 128, 15, 17, 5, wform=(1, 11, 64, 4, 1)),
    WgradCase("w_k7_co16_15x17", 5, 16, 15, 17, 7, wform=(0, 12, 64, 4, 1)), WgradCase("w_k7_co24_15x17", 4, 24, 15, 17, 7, wform=(0, 13, 64, 4, 1)),
    WgradCase("w_k7_co64_15x17", 4, 64, 15, 17, 7, wform=(1, 14, 64, 4, 1)), WgradCase("w_k7_co128_45x47_ragged", 4, 128, 45, 47, 7, wform=(1, 15, 512, 5, 1)),
    WgradCase("w_k3_s2_co16_31x33", 5, 16, 31, 33, 3, 2, wform=(0, 4, 256, 2, 1)), WgradCase("w_k3_s2_even_32x30_concat", 5, 16, 32, 30, 3, 2, concat=1, wform=(0, 4, 64, 4, 1)),
    WgradCase("w_k3_reflect_co16_15x17", 5, 16, 15, 17, 3, reflect=1, wform=(0, 4, 64, 4, 1)), WgradCase("w_k5_reflect_co4_15x17", 5, 4, 15, 17, 5, reflect=1, wform=(0, 8, 64, 4, 1)),
    WgradCase("w_k7_reflect_co16_45x47", 4, 16, 45, 47, 7, reflect=1, wform=(0, 12, 512, 5, 1)),
    WgradCase("w_k3_s2_reflect_31x33", 5, 16, 31, 33, 3, 2, reflect=1, wform=(0, 4, 256, 2, 1)),
    WgradCase("w_k3_N2_sum", 5, 16, 31, 33, 3, N=2, wform=(0, 4, 256, 8, 1)), WgradCase("w_k3_N2_sum_acc", 5, 16, 45, 47, 3, N=2, acc=1, wform=(0, 4, 512, 10, 1)),
    WgradCase("w_k3_scalar_81", 3, 3, 15, 17, 3, wform=(0, 4, 64, 4, 0)), WgradCase("w_k3_scalar_81_acc", 3, 3, 45, 47, 3, acc=1, wform=(0, 4, 512, 5, 0)),
    WgradCase("w_k3_indep_N2", 5, 16, 45, 47, 3, N=2, indep=1, wform=(0, 4, 512, 10, 1)), WgradCase("w_k1_indep_N2_acc", 20, 64, 15, 17, 1, N=2, indep=1, acc=1, wform=(1, 2, 64, 8, 1)),
    WgradCase("w_tile_co19_ci9", 9, 19, 157, 257, 3, wform=(2, 2, 512, 79, 0)), WgradCase("w_tile_co40_ci5", 5, 40, 157, 257, 3, wform=(2, 2, 512, 79, 1)),
    WgradCase("w_tile_co7_reflect", 5, 7, 157, 257, 3, reflect=1, wform=(2, 1, 512, 79, 0)), WgradCase("w_tile_co16_N2_acc", 4, 16, 157, 257, 3, N=2, acc=1, wform=(2, 1, 512, 158, 1)),
    WgradCase("w_tile_258x257_chunk_rule", 4, 19, 258, 257, 3, wform=(2, 2, 576, 116, 1)), WgradCase("w_k1_258x257_chunk_rule", 4, 4, 258, 257, 1, wform=(0, 0, 576, 116, 1)),
]


PRE_SLOPE = 0.1   # LeakyReLU of the chained skip BatchNorm (different from the concat's, so that a mix-up shows)


def bn_problem(c, d):
    """Everything a BatchNorm case is checked against, built once: the input as the reference sees it (y_ref fp64 + the element bound E_y of
    the parts the kernel forms itself: upsampled channels, the chained skip BatchNorm's activation), the same input as an fp32 emulation
    forms it (y32), the forward reference, and the backward's own inputs -- fp32 roundings of the reference's y, out, mean, rstd, so that
    the backward is judged independently of the forward kernel -- with its reference.  Slab sums are bit-exact predictions (slab order)."""
    N, C, HW = c.N, c.C, c.HW
    y32 = d["y"].clone()
    p = dict(slab_start=None, pre=None)
    if c.slabs:
        p["slab_start"] = _per_img(c, d["bias"]).expand(N, C, HW)
        y32 = slab_sum_f32(p["slab_start"], d["slabs"])
    y_ref, E_y = y32.double(), torch.zeros(N, C, HW, dtype=F64)
    if c.pre:
        pc, ps = c.pre
        c1 = BnCase(c.name + "_pre", pc, HW, c.kind, N=N, arenas=c.arenas, slope=PRE_SLOPE)
        y1 = slab_sum_f32(_per_img(c, d["pre_bias"]).expand(N, pc, HW), d["pre_slabs"]) if ps else d["pre_y"]
        f1 = bn_fwd_ref(c1, y1, d["pre_gamma"], d["pre_beta"])
        y_ref[:, :pc], E_y[:, :pc] = f1["out"], f1["E_out"]
        y32[:, :pc] = bn_fwd_emulate(c1, y1, d["pre_gamma"], d["pre_beta"])[2]
        p["pre"] = dict(c=c1, y1=y1, fwd=f1)
    if c.up:
        h, w, Ho, Wo, c0 = c.up
        y_ref[:, c0:] = up_ref(d["src"].double(), Ho, Wo).reshape(N, C - c0, HW)
        E_y[:, c0:] = up_bound(d["src"], Ho, Wo).reshape(N, C - c0, HW)
        y32[:, c0:] = up_emulate(d["src"], Ho, Wo).reshape(N, C - c0, HW)
    f = bn_fwd_ref(c, y_ref, d["gamma"], d["beta"], E_y=E_y)
    p.update(y_ref=y_ref, E_y=E_y, y32=y32, fwd=f)
    # ---- backward
    y_in, m32, r32, out32 = y_ref.to(F32), f["mean"].to(F32), f["rstd"].to(F32), f["out"].to(F32)
    da32 = d["da"]
    if c.da_slabs:
        s = slab_sum_f32(torch.zeros(N, C, HW), d["da_slabs"])
        da32 = d["da"] + s if c.da_slabs[1] else s
    amb, pos = None, out32 > 0
    if c.form[6] and c.slope != 1:   # the kernel re-forms the pre-activation from y: its sign is the kernel's own decision
        t_b = (y_in.double() - m32.double()[:, :, None]) * r32.double()[:, :, None] * _per_img(c, d["gamma"].double()) + _per_img(c, d["beta"].double())
        pos, amb = t_b > 0, t_b.abs() < f["E_t"]
    prev = (d["prev_dg"], d["prev_db"]) if c.acc else None
    b = bn_bwd_ref(c, da32, pos, y_in, m32, r32, d["gamma"], amb=amb, prev=prev)
    p.update(y_in=y_in, m32=m32, r32=r32, out32=out32, da32=da32, pos=pos, amb=amb, prev=prev, bwd=b)
    if c.up:
        h, w, Ho, Wo, c0 = c.up
        dyu, Eu = b["dy"][:, c0:].reshape(N, C - c0, Ho, Wo), b["E_dy"][:, c0:].reshape(N, C - c0, Ho, Wo)
        p["d_src"] = up_adjoint_ref(dyu, h, w)
        p["E_d_src"] = up_adjoint_ref(Eu, h, w) + up_adjoint_bound(dyu, h, w)
    if c.pre:
        pc, ps = c.pre
        q = p["pre"]
        q["m32"], q["r32"], q["y1_in"] = q["fwd"]["mean"].to(F32), q["fwd"]["rstd"].to(F32), q["y1"].to(F32)
        q["prev"] = (d["prev_dg"][:, :pc] * 0.5, d["prev_db"][:, :pc] * 0.5) if c.acc else None
        q["bwd"] = bn_bwd_ref(q["c"], b["dy"][:, :pc], y_in[:, :pc] > 0, q["y1_in"], q["m32"], q["r32"], d["pre_gamma"], E_da=b["E_dy"][:, :pc], prev=q["prev"])
    return p


UP_CASES = [(h, w, Ho, Wo) for h, w in ((1, 1), (1, 7), (5, 6)) for Ho, Wo in ((2 * h, 2 * w), (2 * h - 1, 2 * w - 1))]
SIGMOID_HW = [100, 513, 40000]
SIGMOID_BATCHES = [(1, 0), (2, 0), (4, 2)]   # (N, group): group 0 = one parameter set, the partials run over all N images


def up_inputs(h, w, Ho, Wo, N=2, C=3):
    gen = _gen("up", h, w, Ho, Wo)
    return torch.randn(N, C, h, w, generator=gen), torch.randn(N, C, Ho, Wo, generator=gen)


def sigmoid_inputs(HW, N, group, C=3):
    gen = _gen("sig", HW, N, group)
    return torch.randn(N, C, HW, generator=gen) + 0.3, torch.sigmoid(torch.randn(N, C, HW, generator=gen) * 2)
