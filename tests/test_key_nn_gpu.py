"""GPU: the nearest-neighbour key appearance term (``lambda_global_key_nn`` / ``dino_nn_layer``), op level: the four
launches on caller buffers (splice_key_nn_pairs) against float64 on the same bf16 values under bounds derived from the arithmetic
include/splice_hip.h states -- the assignment on planted and on iid inputs, cosines, value and every key-gradient element, masking of the
rows >= T, ties, the all-zero row, add versus store, guard bands, partial slots, batch independence, equal keys, refusals.  The step-level
tests are in tests/test_key_nn_step_gpu.py."""
import ctypes as C

import numpy as np
import pytest
import torch

from splice_amd import _lib
from splice_amd.engine import np_key_nn
from test_key_nn_cpu import EPS, IID_SHAPE, OP_SHAPES, U24, cosine_reference, iid_exempt_rows, iid_keys, planted_keys

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
NAN_BITS = 0x7FC0DEAD      # a quiet NaN with a payload: what the kernels must leave alone
PART_FILL = -123.0         # prefill of partial slots, values and cosines
MATCH_FILL = -77           # prefill of the assignment
GUARD = 64                 # elements of guard band on either side of every output buffer
OP_LAM = 0.37
DK_GAP = 8                 # a key-gradient row is D + 8 floats long
PART_EXTRA = 3             # a pair's partial row is ceil(T / 4) + 3 slots long
ERR_ARG = -1               # SPLICE_ERR_ARG
SLACK = 1 + 1e-5           # the products of the first-order terms of a bound


def _st():
    return _lib.current_stream()


def _at(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _parts(T):
    return -(-T // 4)


def _scale(T):
    return float(f32(OP_LAM / T))


def _run(kx, kb, pad="ones", pattern=False, first_pair=0, n_pairs=None, D_arg=None, T_arg=None, null=None, ld_off=None):
    """One splice_key_nn_pairs call on the bf16 keys kx, kb ([pairs][T][D]).  Laid out as tests/test_key_gram_gpu.py lays its buffers out:
    the keys sit in a [pairs][T + 5][3 D] array at column offset D (the qkv layout), so pairs are a gap apart; rows >= T of both arrays and
    every other column hold `pad` ("zeros", "ones": 1e4, "nan": a payload NaN); a key-gradient row is D + 8 floats, a pair has T + 7 of them;
    every output has 64-element guard bands.  The key-gradient buffer is prefilled with a seeded pattern everywhere (`pattern`) or with that
    pattern outside rows < T, columns < D and zeros inside.  first_pair / n_pairs: launch on a sub-range of the pairs (pointers moved)."""
    L = _lib.lib()
    pairs, T, D = kx.shape
    n = pairs - first_pair if n_pairs is None else n_pairs
    Rk, Rd, ldk, lddk = T + 5, T + 7, 3 * D, D + DK_GAP
    fill = {"zeros": 0.0, "ones": 1e4, "nan": float("nan")}[pad]
    arrs = []
    for k in (kx, kb):
        a = torch.full((pairs, Rk, ldk), fill, dtype=torch.bfloat16)
        if pad == "nan":
            a.view(torch.int16)[:] = 0x7FC1   # (a bf16 NaN with a payload)
        a[:, :T, D:2 * D] = k
        arrs.append(a.to(DEV))
    ax, ab = arrs
    parts = _parts(T)
    part_ps = parts + PART_EXTRA
    match = torch.full((GUARD + n * T + GUARD,), MATCH_FILL, dtype=torch.int32, device=DEV)
    cos = torch.full((GUARD + n * T + GUARD,), PART_FILL, device=DEV)
    part = torch.full((GUARD + n * part_ps + GUARD,), PART_FILL, device=DEV)
    value = torch.full((GUARD + n + GUARD,), PART_FILL, device=DEV)
    ws_bytes = int(L.splice_key_nn_ws_bytes(T, D, max(n, 1)))
    ws = torch.full((GUARD + ws_bytes // 4 + GUARD,), NAN_BITS, dtype=torch.int32, device=DEV)   # (scratch arrives dirty)
    g = torch.Generator().manual_seed(11 + T + D)
    dk0 = 1e-4 * torch.randn(GUARD + n * Rd * lddk + GUARD, generator=g)
    if not pattern:
        dk0[GUARD:-GUARD].view(n, Rd, lddk)[:, :T, :D] = 0.0
    dk = dk0.to(DEV)
    ptr = dict(k_x=_at(ax, first_pair * Rk * ldk + D), k_b=_at(ab, first_pair * Rk * ldk + D), match=_at(match, GUARD), cos=_at(cos, GUARD), part=_at(part, GUARD),
               value=_at(value, GUARD), dk=_at(dk, GUARD), ws=_at(ws, GUARD))
    if null:
        ptr[null] = C.c_void_p(0)
    ld = dict(ldk=ldk, lddk=lddk)
    if ld_off:
        ld[ld_off[0]] += ld_off[1]
    rc = L.splice_key_nn_pairs(ptr["k_x"], ptr["k_b"], ld["ldk"], Rk * ldk, Rk * ldk, T if T_arg is None else T_arg, D if D_arg is None else D_arg, n, _scale(T), EPS,
                               ptr["match"], ptr["cos"], ptr["part"], part_ps, ptr["value"], ptr["dk"], ld["lddk"], Rd * lddk, ptr["ws"], _st())
    torch.cuda.synchronize()
    guards = bool((match[:GUARD] == MATCH_FILL).all() and (match[-GUARD:] == MATCH_FILL).all() and (ws[:GUARD] == NAN_BITS).all() and (ws[-GUARD:] == NAN_BITS).all())
    for b in (cos, part, value):
        guards = guards and bool((b[:GUARD] == PART_FILL).all() and (b[-GUARD:] == PART_FILL).all())
    dkc = dk.cpu()
    guards = guards and torch.equal(_bits(dkc[:GUARD]), _bits(dk0[:GUARD])) and torch.equal(_bits(dkc[-GUARD:]), _bits(dk0[-GUARD:]))
    return dict(rc=rc, match=match[GUARD:-GUARD].view(n, T).cpu(), cos=cos[GUARD:-GUARD].view(n, T).cpu(), part=part[GUARD:-GUARD].view(n, part_ps).cpu(),
                value=value[GUARD:-GUARD].cpu(), dk=dkc[GUARD:-GUARD].view(n, Rd, lddk), dk0=dk0[GUARD:-GUARD].view(n, Rd, lddk), guards=guards)


def _same_bits(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in ("match", "cos", "part", "value", "dk"))


def _untouched(r):
    fill = int(np.array(PART_FILL, dtype=f32).view(np.int32))
    return bool((r["match"] == MATCH_FILL).all() and (_bits(r["cos"]) == fill).all() and (_bits(r["part"]) == fill).all() and (_bits(r["value"]) == fill).all()
                and torch.equal(_bits(r["dk"]), _bits(r["dk0"])))


def _check_values(r, kx, kb, p, tag):
    """Pair p of run r against float64 on the same bf16 values with the kernel's own assignment: the cosines, the value and every
    key-gradient element, under bounds derived from the arithmetic of splice_key_nn_pairs (include/splice_hip.h).
      cos_t: E_tj of cosine_reference at j = match[t].
      value: r_t = fl(1 - c_t) carries E_t + 2^-24 |r_t|; the sum passes 2 adds in the workgroup, ceil(parts / 64) lane-strided adds, 6 tree
          levels, the crop add, then the rounded 1 / T and its product: R = ceil(parts / 64) + 11 roundings on addends taken by absolute value:
          bound_v = mean(E_t + 2^-24 |r_t|) (1 + R 2^-24) + R 2^-24 mean|r_t|
      dK_td = fma(wb, b_jd, fma(wk, k_td, pre)):  q = fl(n_t m_j) carries eps_q = 2 eps_n + 2^-24 (exact where clamped to eps);
          wb = fl(-scale / f): relative eps_q + 2^-24;  wk = fl(fl(scale c) / fl(n_t n_t)): |error| <= scale E_t / n_t^2 + |wk| (2 eps_n + 3 2^-24);
          two fused multiply-adds, one rounding each:
          bound_g = |b_jd| |wb| (eps_q + 2^-24) + |k_td| dwk + 2^-24 (|pre + wk k_td| + |pre + dK_td|)   (times SLACK)
    scale is lambda / T as the caller rounded it: the reference takes lambda = scale * T."""
    T, D = kx.shape[1:]
    x, b = kx[p].double().numpy(), kb[p].double().numpy()
    m = r["match"][p].numpy().astype(np.int64)
    assert ((m >= 0) & (m < T)).all()
    c, E = cosine_reference(kx[p], kb[p])
    rows = np.arange(T)
    Et = E[rows, m]
    raw, _, cos, dk = np_key_nn(x, b, _scale(T) * T, eps=EPS, match=m)
    got_c = r["cos"][p].double().numpy()
    frac_c = float((np.abs(got_c - cos) / Et.clip(1e-300)).max()) if Et.max() > 0 else float(np.abs(got_c - cos).max())
    R = -(-_parts(T) // 64) + 11
    rt = 1.0 - cos
    bound_v = np.mean(Et + U24 * np.abs(rt)) * (1 + R * U24) * SLACK + R * U24 * np.mean(np.abs(rt))
    got_v = float(r["value"][p])
    nx, nb = np.sqrt((x * x).sum(1)), np.sqrt((b * b).sum(1))
    eps_n = ((D / 64 + 6) / 2 + 1) * U24
    q = nx * nb[m]
    live = q > EPS
    eps_q = np.where(live, 2 * eps_n + U24, 0.0)
    sc = _scale(T)
    wb = sc / np.maximum(q, EPS)
    wk = np.where(live, sc * cos / np.where(nx > 0, nx * nx, 1.0), 0.0)
    dwk = np.where(live, sc * Et / np.where(nx > 0, nx * nx, 1.0) + np.abs(wk) * (2 * eps_n + 3 * U24), 0.0)
    pre = r["dk0"][p, :T, :D].double().numpy()
    want = pre + dk
    bound_g = (np.abs(b[m]) * (wb * (eps_q + U24))[:, None] + np.abs(x) * dwk[:, None] + U24 * (np.abs(pre + wk[:, None] * x) + np.abs(want))) * SLACK
    got_g = r["dk"][p, :T, :D].double().numpy()
    bad = bound_g <= 0
    frac_g = float((np.abs(got_g - want)[~bad] / bound_g[~bad]).max()) if (~bad).any() else 0.0
    assert (got_g[bad] == want[bad]).all()
    print(f"KEY_NN op {tag} T={T} D={D} pair {p}: value {got_v:.7g} ref {raw:.7g} err/bound {abs(got_v - raw) / bound_v:.4f}; cos worst err/bound {frac_c:.4f} "
          f"(largest bound {Et.max():.2e}); dK worst err/bound {frac_g:.4f}, norm-wise rel {np.linalg.norm(got_g - want) / max(np.linalg.norm(dk), 1e-300):.3e}")
    assert (np.abs(got_c - cos) <= Et).all(), (p, frac_c)
    assert abs(got_v - raw) <= bound_v, (p, got_v, raw, bound_v)
    assert frac_g <= 1.0, (p, frac_g)
    return raw, cos, dk


@pytest.fixture(scope="module")
def op_runs():
    cache = {}

    def get(kind, T, D, pairs, **kw):
        key = (kind, T, D, pairs, tuple(sorted(kw.items())))
        if key not in cache:
            kx, kb = planted_keys(T, D, pairs)[:2] if kind == "planted" else iid_keys(pairs)
            cache[key] = _run(kx, kb, **kw)
        return cache[key]
    return get


@pytest.mark.parametrize("T,D", OP_SHAPES)
@pytest.mark.parametrize("pairs", [1, 3])
@pytest.mark.parametrize("pattern", [False, True], ids=["store", "add"])
def test_planted_match_and_values_against_fp64(op_runs, T, D, pairs, pattern):
    """match == pi on EVERY row; cosines, value and every key-gradient element inside the derived bounds; with the buffer prefilled by a
    seeded pattern the result is pattern + dK (the prefill is the addend).  Rows >= T of dK, the gap behind a row, the partial slots beyond
    ceil(T / 4) and the guard bands keep their bits; every partial slot below is written."""
    kx, kb, pi = planted_keys(T, D, pairs)
    r = op_runs("planted", T, D, pairs, pattern=pattern)
    assert r["rc"] == 0 and r["guards"]
    assert np.array_equal(r["match"].numpy(), pi), np.nonzero(r["match"].numpy() != pi)
    parts = _parts(T)
    fill = int(np.array(PART_FILL, dtype=f32).view(np.int32))
    assert (_bits(r["part"][:, parts:]) == fill).all(), "partial slots beyond ceil(T / 4) were written"
    assert (_bits(r["part"][:, :parts]) != fill).all(), "a partial slot was not written"
    assert torch.equal(_bits(r["dk"][:, T:]), _bits(r["dk0"][:, T:])), "a padding row of the key gradient moved"
    assert torch.equal(_bits(r["dk"][:, :, D:]), _bits(r["dk0"][:, :, D:])), "the gap behind a key-gradient row moved"
    for p in range(pairs):
        raw, cos, dk = _check_values(r, kx, kb, p, f"planted prefill={'pattern' if pattern else 'zeros'}")
        # the partials: slot g is (r0 + r1) + (r2 + r3) of the reported cosines of rows 4 g .. 4 g + 3, exactly (a row >= T adds 0)
        rr = np.zeros(parts * 4, dtype=f32)
        rr[:T] = f32(1.0) - r["cos"][p].numpy()
        rr = rr.reshape(parts, 4)
        want_part = (rr[:, 0] + rr[:, 1]) + (rr[:, 2] + rr[:, 3])
        assert r["part"][p, :parts].numpy().tobytes() == want_part.astype(f32).tobytes()
        assert np.abs(dk).max() > 0 and raw > 0.01


@pytest.mark.parametrize("pairs", [1, 3])
def test_iid_match_against_fp64(op_runs, pairs):
    """independent keys: the reference's top-two gaps come down to the size of the error bound.  A row whose reference gap is below twice
    its derived cosine bound is exempt from index equality -- at most 1 % of the rows -- and its chosen column must still have a reference
    cosine within that bound of the row maximum; every other row matches the reference's arg-max.  Values as in the planted test."""
    T, D = IID_SHAPE
    kx, kb = iid_keys(pairs)
    r = op_runs("iid", T, D, pairs)
    assert r["rc"] == 0 and r["guards"]
    for p in range(pairs):
        exempt, c, E = iid_exempt_rows(kx[p], kb[p])
        assert len(exempt) <= T // 100
        m = r["match"][p].numpy()
        want = np.argmax(c, axis=1)
        strict = np.setdiff1d(np.arange(T), exempt)
        assert np.array_equal(m[strict], want[strict]), np.nonzero(m != want)
        for t in exempt:
            print(f"KEY_NN op iid pair {p} exempt row {t}: chose {m[t]} (reference {want[t]}), reference cosine {c[t, m[t]]:.8f} against the maximum {c[t].max():.8f}, bound {E[t].max():.2e}")
            assert c[t].max() - c[t, m[t]] <= E[t].max()
        _check_values(r, kx, kb, p, "iid")


@pytest.mark.parametrize("T,D", OP_SHAPES)
def test_rows_beyond_T_reach_no_output_bit(op_runs, T, D):
    """rows >= T of both key arrays (and every other element of the qkv-shaped buffers) hold 1e4 in one run and a payload NaN in another:
    every output bit equals the run with zeros there -- an unmasked 1e4 target row would win every arg-max"""
    base = op_runs("planted", T, D, 3, pattern=True, pad="zeros")
    assert base["rc"] == 0 and base["guards"]
    for pad in ("ones", "nan"):
        r = op_runs("planted", T, D, 3, pattern=True, pad=pad)
        assert r["rc"] == 0 and r["guards"] and _same_bits(base, r), pad
        assert bool(torch.isfinite(r["dk"]).all()) and bool(torch.isfinite(r["cos"]).all())


def test_ties_go_to_the_lowest_index():
    """T = 197: target rows 3 and 130 (another column tile) are bit-equal, and so are rows 19 (the same lane, the other fragment) and 40
    (another lane group of the same tile); rows planted on any of them report 3"""
    T, D = 197, 192
    kx, kb, pi = planted_keys(T, D, 1)
    kb = kb.clone()
    kx = kx.clone()
    for j in (19, 40, 130):
        kb[0, j] = kb[0, 3]
    planted_on = np.nonzero(np.isin(pi[0], (3, 19, 40)))[0]
    g = torch.Generator().manual_seed(77)
    for t in planted_on:                      # (the rows planted on the old rows 19 and 40 are planted on the shared row again)
        if pi[0][t] != 3:
            kx[0, t] = (0.9 * kb[0, 3].float() + 0.3 * torch.randn(D, generator=g)).to(torch.bfloat16)
    extra = [150, 151, 190, 196]              # and a few rows that are a multiple of the shared row: cosine 1 with all four
    for t in extra:
        kx[0, t] = (1.3 * kb[0, 130].float()).to(torch.bfloat16)
    assert len(planted_on) >= 3
    r = _run(kx, kb)
    assert r["rc"] == 0 and r["guards"]
    m = r["match"][0].numpy()
    want = pi[0].copy()
    want[np.isin(want, (19, 40))] = 3
    want[extra] = 3
    assert np.array_equal(m, want), np.nonzero(m != want)
    assert (m[planted_on] == 3).all() and (m[extra] == 3).all()
    _check_values(r, kx, kb, 0, "ties")


def test_an_all_zero_row_takes_the_clamped_branch():
    """an all-zero x' row: cos 0, match 0, and the gradient -scale b_0 / eps within its bound"""
    T, D = 65, 128
    kx, kb, pi = planted_keys(T, D, 1)
    kx = kx.clone()
    for t in (0, 33, 64):
        kx[0, t] = 0.0
    r = _run(kx, kb)
    assert r["rc"] == 0 and r["guards"]
    for t in (0, 33, 64):
        assert int(r["match"][0, t]) == 0 and float(r["cos"][0, t]) == 0.0
        want = -_scale(T) * kb[0, 0].double().numpy() / EPS
        got = r["dk"][0, t, :D].double().numpy()
        assert (np.abs(got - want) <= 2 * U24 * np.abs(want) * SLACK).all() and np.abs(want).max() > 1e3   # (the division and the fused multiply-add: one rounding each)
    keep = np.setdiff1d(np.arange(T), (0, 33, 64))
    assert np.array_equal(r["match"][0].numpy()[keep], pi[0][keep])
    _check_values(r, kx, kb, 0, "zero rows")


def test_a_pair_of_a_batched_launch_equals_its_own_launch(op_runs):
    """pair p of the three-pair launch against the one-pair launch on its operands: every output bit for bit"""
    for T, D in ((197, 192), (65, 128)):
        kx, kb, _ = planted_keys(T, D, 3)
        three = op_runs("planted", T, D, 3, pattern=False)   # (zeros under the rows < T: a pair's prefill is the same in both launches)
        for p in range(3):
            one = _run(kx, kb, pattern=False, first_pair=p, n_pairs=1)
            assert one["rc"] == 0 and one["guards"]
            assert torch.equal(three["match"][p], one["match"][0]) and torch.equal(_bits(three["cos"][p]), _bits(one["cos"][0]))
            assert torch.equal(_bits(three["part"][p]), _bits(one["part"][0])) and torch.equal(_bits(three["value"][p:p + 1]), _bits(one["value"][0:1]))
            assert torch.equal(_bits(three["dk"][p, :T, :D]), _bits(one["dk"][0, :T, :D]))
        assert not torch.equal(three["value"][0:1], three["value"][1:2])


@pytest.mark.parametrize("T,D", [(65, 128), (197, 192)])
def test_equal_keys_match_themselves(T, D):
    """K_x' == K_B' with distinct rows: match[i] == i, and the value and every key-gradient element lie within their bounds of 0"""
    kb = planted_keys(T, D, 1)[1]
    r = _run(kb, kb)
    assert r["rc"] == 0 and r["guards"]
    assert np.array_equal(r["match"][0].numpy(), np.arange(T))
    raw, cos, dk = _check_values(r, kb, kb, 0, "equal keys")
    assert abs(raw) < 1e-12 and np.abs(dk).max() < 1e-12 * _scale(T)
    print(f"KEY_NN op equal keys T={T} D={D}: value {float(r['value'][0]):.3e}, max |dK| {float(r['dk'][0, :T, :D].abs().max()):.3e}")


def test_op_refusals_launch_nothing():
    T, D = 65, 128
    kx, kb, _ = planted_keys(T, D, 3)
    cases = [dict(D_arg=96), dict(D_arg=0), dict(T_arg=0), dict(T_arg=-3), dict(n_pairs=0)] + \
            [dict(null=k) for k in ("k_x", "k_b", "match", "cos", "part", "value", "dk", "ws")] + \
            [dict(ld_off=("ldk", -3 * D + D - 8)), dict(ld_off=("ldk", 4)), dict(ld_off=("lddk", -16))]
    for kw in cases:
        r = _run(kx, kb, pattern=True, **kw)
        assert r["rc"] == ERR_ARG and r["guards"] and _untouched(r), kw
