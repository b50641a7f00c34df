"""GPU: the small-plane BatchNorm kernels (form SMALL, planes of <= 4096 pixels) exist in instances that compile only the features a launch
needs (gen_bn.hip: batch statistics 1, shared-parameter tail 2, slabs 4, a pre BatchNorm 8, a fused upsampling 16).  Every instance that covers a
call must give the bits of the fully general instance (mask 31) of the same register tile: the same call runs under the automatic choice, under
the exact instance where one exists, and under mask 31 (splice_gen_bn_small_instance), and EVERY buffer of the call -- outputs, the y the
forward forms, statistics, parameter gradients, the low-resolution gradient, the pre BatchNorm's outputs, inputs, and the NaN-payload guards
around all of them -- is compared bit for bit.  An instance that lacks a feature the call needs must refuse the call and write nothing.

The numerical checks of these kernels against fp64 are tests/test_gen_ops_gpu.py; this file only pins the instances to one another.
Plane sizes: 257 (<4> at its low end), 1024 / 1025 (the <4> / <16> boundary), 3136 (56 x 56) and 4096 (<16> at its top end); 64 and 256 add <1>."""
import ctypes as C

import pytest
import torch

from splice_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_BITS = 0x7FC0DEAD
ERR_ARG = -1
GUARD = 64
EPS = 1e-5
PN = 16                     # p_nstride of the parameter arenas (floats)
F_BATCH, F_TAIL, F_SLABS, F_PRE, F_UP, F_ALL = 1, 2, 4, 8, 16, 31
INSTANCES = [0, F_SLABS, F_UP, F_PRE | F_UP, F_PRE | F_UP | F_SLABS, F_BATCH, F_TAIL, F_ALL]   # the launcher's list, in its order

# Ho x Wo = HW window of the x2 upsampling of an h x w source: (h, w, Ho, Wo)
UPS = {64: (4, 4, 8, 8), 256: (8, 8, 16, 16), 257: (1, 129, 1, 257), 1024: (16, 16, 32, 32), 1025: (13, 21, 25, 41), 3136: (28, 28, 56, 56),
       4096: (32, 32, 64, 64)}
HWS = [257, 1024, 1025, 3136, 4096]


def case(HW, C_=3, N=1, arenas=False, batch=0, slope=0.2, up=False, pre=0, pre_slabs=0, slabs=0, da_slabs=None, acc=0, up_src=None):
    return dict(HW=HW, C=C_, N=N, arenas=arenas, batch=batch, slope=slope, up=(up_src or UPS[HW]) if up else None, pre=pre, pre_slabs=pre_slabs,
                slabs=slabs, da_slabs=da_slabs, acc=acc)


def _cases():
    out = []
    for HW in HWS + [64, 256]:
        out += [case(HW), case(HW, slope=1.0), case(HW, C_=5, acc=1),
                case(HW, up=True),                                        # odd sources at 257 and 1025, even ones elsewhere
                case(HW, C_=4, up=True, pre=2), case(HW, C_=4, up=True, pre=2, acc=1),   # the concat unit as the engine issues it
                case(HW, pre=2),                                          # BnPre alone (SPLICE_BN_CHAIN on a unit without upsampling)
                case(HW, C_=4, up=True, pre=2, pre_slabs=4, da_slabs=(4, 0)),            # ... with slabs: the skip conv's (fwd), the data gradient's (bwd)
                case(HW, slabs=4, da_slabs=(4, 0)), case(HW, slabs=9, da_slabs=(9, 0)),
                case(HW, slabs=2, da_slabs=(4, 1)), case(HW, slabs=16, da_slabs=(9, 1)),
                case(HW, N=2), case(HW, N=2, acc=1),                      # shared parameters: the backward's tail loop
                case(HW, N=2, arenas=True), case(HW, N=2, arenas=True, C_=4, up=True, pre=2, da_slabs=(4, 1)),
                case(HW, N=2, batch=2), case(HW, N=2, batch=2, slope=1.0)]
    out.append(case(4096, up=True, up_src=(40, 40, 64, 64)))              # a source too big for the LDS stage: read from global memory
    return out


CASES = _cases()


def _id(c):
    return "-".join(f"{k}{v}" for k, v in c.items() if v not in (None, 0, False) or k == "HW").replace(" ", "")


def need(c, bwd):
    m = F_BATCH if c["batch"] else 0
    if bwd:
        m |= F_TAIL if (not c["batch"] and not c["arenas"] and c["N"] > 1) else 0
        m |= F_SLABS if c["da_slabs"] else 0
    else:
        m |= F_SLABS if (c["slabs"] or c["pre_slabs"]) else 0
    m |= F_PRE if c["pre"] else 0
    m |= F_UP if c["up"] else 0
    return m


def _bits(t):
    return t.contiguous().view(torch.int32)


class Arena:
    """every device buffer of one call: NaN-payload guards around each, all of them compared afterwards"""

    def __init__(self, seed):
        self.g = torch.Generator().manual_seed(seed)
        self.bufs = []

    def buf(self, n, fill=None, positive=False):
        """n floats: random (fill='rand'), or NaN payload (an output)"""
        t = torch.full((GUARD + n + GUARD,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
        if fill == "rand":
            v = torch.randn(n, generator=self.g)
            t[GUARD:GUARD + n] = (v.abs() + 0.5 if positive else v).to(DEV)
        self.bufs.append((t, n))
        return C.c_void_p(t.data_ptr() + 4 * GUARD)

    def guards_ok(self):
        return all(bool((_bits(t)[:GUARD] == NAN_BITS).all() and (_bits(t)[GUARD + n:] == NAN_BITS).all()) for t, n in self.bufs)

    def snapshot(self):
        return [_bits(t).clone() for t, _ in self.bufs]


def _run(c, bwd, mask, seed=5):
    """one call under the instance `mask` (-1: automatic) on fresh, identically filled buffers: (rc, every buffer's bits, guards intact, untouched outputs)"""
    lib = _lib.lib()
    N, Cc, HW = c["N"], c["C"], c["HW"]
    A = Arena(seed)
    a = _lib.GenBnArgs()
    a.N, a.C, a.HW, a.batch, a.eps, a.slope = N, Cc, HW, c["batch"], EPS, c["slope"]
    a.p_nstride = PN if c["arenas"] else 0
    a.y_nstride = a.out_nstride = a.da_nstride = a.dy_nstride = Cc * HW
    n_par = N * PN
    a.gamma, a.beta = A.buf(n_par, "rand"), A.buf(n_par, "rand")
    a.y = A.buf(N * Cc * HW, "rand")                 # forward: the channels the kernel forms are overwritten
    a.out = A.buf(N * Cc * HW, "rand" if bwd else None)
    a.mean, a.rstd = A.buf(N * Cc, "rand" if bwd else None), A.buf(N * Cc, "rand" if bwd else None, positive=True)
    if c["up"]:
        h, w, Ho, Wo = c["up"]
        c0 = Cc - 1 if not c["pre"] else c["pre"]
        a.up_h, a.up_w, a.up_Ho, a.up_Wo, a.up_c0 = h, w, Ho, Wo, c0
        a.up_src_ns = a.up_d_src_ns = (Cc - c0) * h * w
        if bwd:
            a.up_d_src = A.buf(N * (Cc - c0) * h * w)
        else:
            a.up_src = A.buf(N * (Cc - c0) * h * w, "rand")
    if c["pre"]:
        pc = c["pre"]
        a.pre_C, a.pre_slope, a.pre_y_ns = pc, 0.2, pc * HW
        a.pre_gamma, a.pre_beta = A.buf(n_par, "rand"), A.buf(n_par, "rand")
        a.pre_y = A.buf(N * pc * HW, None if (c["pre_slabs"] and not bwd) else "rand")
        a.pre_mean, a.pre_rstd = A.buf(N * pc, "rand" if bwd else None), A.buf(N * pc, "rand" if bwd else None, positive=True)
        if c["pre_slabs"] and not bwd:
            a.pre_slabs, a.pre_ksplit, a.pre_bias = A.buf(c["pre_slabs"] * N * pc * HW, "rand"), c["pre_slabs"], A.buf(n_par, "rand")
        if bwd:
            a.pre_dy = A.buf(N * pc * HW)
            a.pre_dgamma, a.pre_dbeta = A.buf(n_par, "rand" if c["acc"] else None), A.buf(n_par, "rand" if c["acc"] else None)
    if not bwd and c["slabs"] and not c["up"] and not c["pre"]:
        a.slabs, a.ksplit, a.bias = A.buf(c["slabs"] * N * Cc * HW, "rand"), c["slabs"], A.buf(n_par, "rand")
    if bwd:
        a.da, a.dy = A.buf(N * Cc * HW, "rand"), A.buf(N * Cc * HW)
        a.dgamma, a.dbeta, a.accumulate = A.buf(n_par, "rand" if c["acc"] else None), A.buf(n_par, "rand" if c["acc"] else None), c["acc"]
        if c["da_slabs"]:
            k, sacc = c["da_slabs"]
            a.da_slabs, a.da_ksplit, a.da_accumulate = A.buf(k * N * Cc * HW, "rand"), k, sacc
    before = A.snapshot()
    assert lib.splice_gen_bn_small_instance(mask) == 0
    try:
        rc = (lib.splice_gen_bn_bwd if bwd else lib.splice_gen_bn_fwd)(C.byref(a), _lib.current_stream())
        torch.cuda.synchronize()
    finally:
        assert lib.splice_gen_bn_small_instance(-1) == 0
    after = A.snapshot()
    return rc, after, A.guards_ok(), all(torch.equal(x, y) for x, y in zip(before, after))


def _check(c, bwd):
    m = need(c, bwd)
    rc, ref, guards, untouched = _run(c, bwd, F_ALL)
    assert rc == 0 and guards and not untouched, (_lib.lib().splice_last_error(), guards, untouched)
    modes = [-1] + ([m] if m in INSTANCES and m != F_ALL else [])
    for mode in modes:
        rc, got, guards, _ = _run(c, bwd, mode)
        assert rc == 0 and guards, (mode, _lib.lib().splice_last_error(), guards)
        for i, (g, r) in enumerate(zip(got, ref)):
            assert torch.equal(g, r), f"instance {mode}: buffer {i} differs from the general instance in {(g != r).sum().item()} words"
    # an instance without a feature the call needs refuses it and writes nothing
    for lacking in [i for i in INSTANCES if m & ~i][:3]:
        rc, _, guards, untouched = _run(c, bwd, lacking)
        assert rc == ERR_ARG and guards and untouched, (lacking, rc)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_forward_instances_give_the_general_instance_bit_for_bit(c):
    _check(c, False)


@pytest.mark.parametrize("c", CASES, ids=_id)
def test_backward_instances_give_the_general_instance_bit_for_bit(c):
    _check(c, True)


def test_selector_takes_only_existing_instances():
    lib = _lib.lib()
    for bad in (3, 8, 12, 20, 32, 255, -2 ** 31):
        rc = lib.splice_gen_bn_small_instance(bad)
        if bad < 0:
            assert rc == 0   # any negative value: automatic
        else:
            assert rc == ERR_ARG, bad
    for ok in INSTANCES:
        assert lib.splice_gen_bn_small_instance(ok) == 0
    assert lib.splice_gen_bn_small_instance(-1) == 0
