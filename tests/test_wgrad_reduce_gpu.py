"""GPU: wgrad_reduce_all_kernel alone, through splice_gen_wgrad_reduce, on random fp32 partials against a CPU emulation of its summation
order in torch float32 -- EXACT under ==.  The order (gen_wgrad.hip, include/splice_hip.h): the chunks are walked in groups of four, chunk c of a
full group joins chain c mod 4, the chunks of the last, partial group all join chain 0, each chain in increasing c starting from +0; then
(a0 + a1) + (a2 + a3); then the optional += into the destination.  How many loads the kernel keeps in flight (groups of 32, 8 / 16, 4, 1) must
not show: the chunk counts sit on both sides of every group size, and 98 is the walk of the 224 x 224 layers.  fp32 addition on the CPU and on
the GPU is the same IEEE operation, so the bound is zero.

The 16-byte path needs n % 4 == 0 and 16-byte aligned buffers; n = 3 and a destination moved by one float drive the scalar path
(wgrad_chunk_sum).  NaN-payload guards sit around every buffer."""
import ctypes as C

import pytest
import torch

from splice_amd import _lib

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN_BITS = 0x7FC0DEAD
ERR_ARG = -1
GUARD = 64
CHUNKS = [1, 3, 4, 7, 8, 9, 31, 32, 33, 98, 128]


def _bits(t):
    return t.contiguous().view(torch.int32)


def emulate(part, prev):
    """part [chunks][n] fp32 (CPU), prev [n] or None -> the kernel's sum, in its order, in fp32"""
    chunks, n = part.shape
    a = [torch.zeros(n, dtype=torch.float32) for _ in range(4)]
    full = chunks // 4 * 4
    for c in range(chunks):
        j = c % 4 if c < full else 0
        a[j] = a[j] + part[c]
    s = (a[0] + a[1]) + (a[2] + a[3])
    return prev + s if prev is not None else s


def _buf(values=None, n=None, shift=0):
    n = values.numel() if values is not None else n
    t = torch.full((GUARD + shift + n + GUARD,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
    if values is not None:
        t[GUARD + shift:GUARD + shift + n] = values.reshape(-1).to(DEV)
    return t, C.c_void_p(t.data_ptr() + 4 * (GUARD + shift)), t[GUARD + shift:GUARD + shift + n]


def _guards_ok(t, n, shift=0):
    b = _bits(t)
    return bool((b[:GUARD + shift] == NAN_BITS).all() and (b[GUARD + shift + n:] == NAN_BITS).all())


def _check(n, chunks, acc, n_img=1, pn=0, shift=0, seed=0):
    g = torch.Generator().manual_seed(1000 * n + 10 * chunks + acc + seed)
    # magnitudes spread over a few binades, so that a different association order shows in the last bits
    part = torch.randn(chunks, n, generator=g) * torch.exp2(torch.randint(-3, 4, (chunks, n), generator=g).float())
    width = pn * n_img if pn else n
    prev = torch.randn(width, generator=g)
    p_t, p_p, _ = _buf(part)
    d_t, d_p, d_v = _buf(prev if acc else None, n=width, shift=shift)
    rc = _lib.lib().splice_gen_wgrad_reduce(p_p, n, chunks, d_p, acc, n_img, pn, _lib.current_stream())
    torch.cuda.synchronize()
    assert rc == 0, _lib.lib().splice_last_error()
    assert _guards_ok(p_t, chunks * n) and _guards_ok(d_t, width, shift)
    assert torch.equal(p_t[GUARD:GUARD + chunks * n].cpu().view(chunks, n), part), "the partials were written"
    got = d_v.cpu()
    cpi = chunks // n_img
    for i in range(n_img):
        lo = i * pn
        want = emulate(part[i * cpi:(i + 1) * cpi], prev[lo:lo + n] if acc else None)
        diff = (_bits(got[lo:lo + n]) != _bits(want)).sum().item()
        assert diff == 0, f"n {n} chunks {chunks} acc {acc} image {i}: {diff} of {n} elements differ from the documented order"
        rest = _bits(got[lo + n:lo + pn]) if pn else None   # the rest of an arena is not the layer's: untouched
        if rest is not None and rest.numel():
            assert torch.equal(rest, _bits(prev[lo + n:lo + pn])) if acc else bool((rest == NAN_BITS).all())


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n", [4, 12, 48, 256])
@pytest.mark.parametrize("chunks", CHUNKS)
def test_vector_path_sums_in_the_documented_order(chunks, n, acc):
    _check(n, chunks, acc)


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("chunks", CHUNKS)
def test_scalar_path_sums_in_the_documented_order(chunks, acc):
    _check(3, chunks, acc)
    _check(12, chunks, acc, shift=1)   # a destination that is not 16-byte aligned: the scalar path on a vector-sized layer


@pytest.mark.parametrize("acc", [0, 1])
@pytest.mark.parametrize("n,chunks,pn", [(12, 2 * 98, 16), (48, 2 * 33, 48), (3, 2 * 98, 8), (12, 2 * 7, 14), (256, 2 * 1, 260)])
def test_independent_images_sum_their_own_chunks(n, chunks, pn, acc):
    _check(n, chunks, acc, n_img=2, pn=pn)


def test_zero_chunks_is_an_exact_zero_and_bad_arguments_are_refused():
    lib = _lib.lib()
    d_t, d_p, d_v = _buf(n=8)
    p_t, p_p, _ = _buf(torch.ones(8))
    assert lib.splice_gen_wgrad_reduce(p_p, 8, 0, d_p, 0, 1, 0, _lib.current_stream()) == 0
    torch.cuda.synchronize()
    assert bool((_bits(d_v.cpu()) == 0).all()) and _guards_ok(d_t, 8)
    st = _lib.current_stream()
    for args in [(None, 8, 1, d_p, 0, 1, 0), (p_p, 8, 1, None, 0, 1, 0), (p_p, 0, 1, d_p, 0, 1, 0), (p_p, 8, -1, d_p, 0, 1, 0), (p_p, 8, 1, d_p, 0, 2, 0),
                 (p_p, 4, 2, d_p, 0, 0, 4), (p_p, 4, 3, d_p, 0, 2, 4), (p_p, 4, 2, d_p, 0, 2, 3)]:
        assert lib.splice_gen_wgrad_reduce(*args, st) == ERR_ARG, args
