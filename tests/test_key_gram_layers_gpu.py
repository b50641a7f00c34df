"""GPU: the key second-moment term over several ViT blocks and its centred form (``dino_gram_layers`` / ``dino_gram_layer_weights`` /
``dino_gram_centered``).
Op level: the launches on caller buffers (splice_key_gram_layers_pairs) against float64 on the same bf16 values under a bound derived from
the arithmetic the header states, padding columns, guard bands, batch independence, entry i against the one-block hook bit for bit, equal
and token-constant keys, refusals.  Step level: the per-layer addends, their sum and word 0, the generator gradient against the oracle's
autograd through the same plan, and bit-identity where the step promises it."""
import ctypes as C
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dino_vit
from oracle import extractor as oex
from oracle import losses as olosses
from splice_amd import _lib, synth
from splice_amd.engine import (DEFAULT_CFG, KEY_GRAM_LAYER_KEYS, KEY_GRAM_LOSS_KEY, MultiPairEngine, SpliceEngine, np_key_gram_layers)
from splice_amd.generator import GeneratorPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
U24 = 2.0 ** -24           # unit roundoff of float32
U23 = 2.0 ** -23           # per-term unit of an fp32 MFMA accumulation whose internal order and rounding are not specified
UBF = 2.0 ** -9            # unit roundoff of bf16
SLACK = 1.0 + 1e-5         # the second-order terms of the bounds below
PART_FILL = -123.0         # prefill of partial slots, values and means
FILL_BITS = int(np.array(PART_FILL, dtype=f32).view(np.int32))
GUARD = 64                 # elements of guard band on either side of every output buffer
LAM, LAYER = "lambda_global_key_gram", "dino_gram_layer"
LAYERS, WEIGHTS, CENTERED = KEY_GRAM_LAYER_KEYS
S_LAYERS = "dino_ssim_layers"
ERR_ARG = -1               # SPLICE_ERR_ARG


def _st():
    return _lib.current_stream()


def _at(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bits16(t):
    return t.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ op level
OP_LAM = 0.37
GAP_T = 40       # token columns between the pairs' blocks of a transposed copy beyond round_up(T, 8), and behind the last
DK_GAP = 8       # a key-gradient row is D + 8 floats long
PART_EXTRA = 3   # a pair's partial row is the tiles + 3 slots long
OP_WEIGHTS = {1: [1.0], 3: [0.5, 1.0, 3.0], 12: [0.25 * (i + 1) for i in range(12)]}


def _tiles(D):
    nt = D // 64
    return nt * (nt + 1) // 2


@functools.lru_cache(maxsize=None)
def _op_keys(T, D, pairs, layer, mode="mean"):
    """seeded bf16 keys of `pairs` pairs of table entry `layer`, generated and target, [pairs][T][D]; never modified.
    "mean": a per-feature mean mu of order 1 on unit-variance keys, the target's mean 0.8 mu + 0.3 randn; "equal": the target is the
    generated pass; "const": both sides constant along the tokens, with different per-feature constants of order 1."""
    g = torch.Generator().manual_seed(9000 + 10 * T + D + pairs + 1000 * layer)
    mu = torch.randn(D, generator=g)
    if mode == "const":
        kx = (mu + 0.5).expand(pairs, T, D).contiguous().to(torch.bfloat16)
        kb = (0.8 * mu + 0.3 * torch.randn(D, generator=g)).expand(pairs, T, D).contiguous().to(torch.bfloat16)
        return kx, kb
    z = torch.randn(pairs, T, D, generator=g)
    kx = (z + mu).to(torch.bfloat16)
    if mode == "equal":
        return kx, kx.clone()
    kb = (0.9 * z + 0.5 * torch.randn(pairs, T, D, generator=g) + 0.8 * mu + 0.3 * torch.randn(D, generator=g)).to(torch.bfloat16)
    return kx, kb


def _scale(T, D, w):
    """the entry's scale as the step forms it: the one-block scale in float32, times the weight, one rounding more"""
    return float(f32(f32(4.0 * OP_LAM / (T * D * D)) * f32(w)))


def _layer_buffers(T, D, pairs, layer, mode, pad, pattern, first_pair, n):
    """device buffers of one table entry, laid out as tests/test_key_gram_gpu.py lays out its one block: gaps between the pairs' token
    columns, 1e4 in the rows >= T of the row-major keys, NaN-pattern / fill prefills and guard bands around every output"""
    kx, kb = _op_keys(T, D, pairs, layer, mode)
    t8 = -(-T // 8) * 8
    Tp, Rk, Rd = t8 + GAP_T, T + 5, T + 7
    ldt_x, ldt_b, ldk, lddk = pairs * Tp + 8, pairs * Tp + 24, 3 * D, D + DK_GAP
    krow = torch.full((pairs, Rk, ldk), 1e4, dtype=torch.bfloat16)
    krow[:, :T, D:2 * D] = kx
    tx = torch.full((D, ldt_x), pad, dtype=torch.bfloat16)
    tb = torch.full((D, ldt_b), pad, dtype=torch.bfloat16)
    for p in range(pairs):
        tx[:, p * Tp:p * Tp + T] = kx[p].T
        tb[:, p * Tp:p * Tp + T] = kb[p].T
    part_ps = _tiles(D) + PART_EXTRA
    g = torch.Generator().manual_seed(11 + T + D + layer)
    dk0 = 1e-4 * torch.randn(GUARD + n * Rd * lddk + GUARD, generator=g)
    if not pattern:
        dk0[GUARD:-GUARD].view(n, Rd, lddk)[:, :T, :D] = 0.0
    b = dict(krow=krow.to(DEV), tx=tx.to(DEV), tb=tb.to(DEV), dk0=dk0, dk=dk0.to(DEV),
             delta=torch.full((GUARD + n * D * D + GUARD,), 0x7FC1, dtype=torch.int16, device=DEV),
             part=torch.full((GUARD + n * part_ps + GUARD,), PART_FILL, device=DEV))
    b["ptr"] = dict(k_x=_at(b["krow"], first_pair * Rk * ldk + D), kT_x=_at(b["tx"], first_pair * Tp), kT_b=_at(b["tb"], first_pair * Tp),
                    delta=_at(b["delta"], GUARD), part=_at(b["part"], GUARD), dk=_at(b["dk"], GUARD))
    b["geo"] = dict(Tp=Tp, Rk=Rk, Rd=Rd, ldt_x=ldt_x, ldt_b=ldt_b, ldk=ldk, lddk=lddk, part_ps=part_ps)
    return b


def _collect(b, T, D, n):
    """an entry's outputs on the host, and whether its guard bands kept their bits"""
    geo = b["geo"]
    ok = bool((b["delta"][:GUARD] == 0x7FC1).all() and (b["delta"][-GUARD:] == 0x7FC1).all())
    ok = ok and bool((b["part"][:GUARD] == PART_FILL).all() and (b["part"][-GUARD:] == PART_FILL).all())
    dkc = b["dk"].cpu()
    ok = ok and torch.equal(_bits(dkc[:GUARD]), _bits(b["dk0"][:GUARD])) and torch.equal(_bits(dkc[-GUARD:]), _bits(b["dk0"][-GUARD:]))
    return dict(delta=b["delta"][GUARD:-GUARD].view(n, D, D).cpu(), part=_bits(b["part"][GUARD:-GUARD]).view(n, geo["part_ps"]).cpu(),
                dk=dkc[GUARD:-GUARD].view(n, geo["Rd"], geo["lddk"]), dk0=b["dk0"][GUARD:-GUARD].view(n, geo["Rd"], geo["lddk"])), ok


def _run(T, D, pairs, n_layers, centered, mode="mean", pad=0.0, pattern=True, first_pair=0, n_pairs=None, D_arg=None, n_arg=None, null=None, ld_off=None,
         share_dk=False):
    """One splice_key_gram_layers_pairs call on `n_layers` entries with the weights OP_WEIGHTS[n_layers].  The token columns >= T of both
    transposed copies (and every gap column) hold `pad`.  null: ("table", name) passes a null table, (i, name) a null entry pointer;
    ld_off: (name, delta) on a shared leading dimension; share_dk: entry 1 is given entry 0's dk.  Returns dict(rc, layers [per entry:
    delta, part, dk, dk0], values bits [n][n_layers], value bits [n], mu bits, guards)."""
    L = _lib.lib()
    n = pairs - first_pair if n_pairs is None else n_pairs
    weights = OP_WEIGHTS[n_layers]
    bufs = [_layer_buffers(T, D, pairs, i, mode, pad, pattern, first_pair, n) for i in range(n_layers)]
    geo = dict(bufs[0]["geo"])
    values = torch.full((GUARD + n * n_layers + GUARD,), PART_FILL, device=DEV)
    value = torch.full((GUARD + n + GUARD,), PART_FILL, device=DEV)
    mu = torch.full((GUARD + n_layers * n * 2 * D + GUARD,), PART_FILL, device=DEV)
    arr = {}
    for name in ("k_x", "kT_x", "kT_b", "delta", "part", "dk"):
        ptrs = [b["ptr"][name].value for b in bufs]
        if share_dk and name == "dk":
            ptrs[1] = ptrs[0]
        if null and null[0] != "table" and null[1] == name:
            ptrs[null[0]] = None
        arr[name] = None if null and null[0] == "table" and null[1] == name else (C.c_void_p * n_layers)(*ptrs)
    if ld_off:
        geo[ld_off[0]] += ld_off[1]
    wv, sv = (C.c_float * n_layers)(*weights), (C.c_float * n_layers)(*[_scale(T, D, w) for w in weights])
    rc = L.splice_key_gram_layers_pairs(n_layers if n_arg is None else n_arg, arr["k_x"], arr["kT_x"], arr["kT_b"], arr["delta"], arr["part"], arr["dk"], wv, sv,
                                        geo["ldk"], geo["Rk"] * bufs[0]["geo"]["ldk"], geo["ldt_x"], geo["Tp"], geo["ldt_b"], geo["Tp"], T, D if D_arg is None else D_arg, n,
                                        int(centered), geo["part_ps"], _at(values, GUARD), _at(value, GUARD), _at(mu, GUARD), geo["lddk"],
                                        geo["Rd"] * bufs[0]["geo"]["lddk"], _st())
    torch.cuda.synchronize()
    guards = True
    for b_ in (values, value, mu):
        guards = guards and bool((b_[:GUARD] == PART_FILL).all() and (b_[-GUARD:] == PART_FILL).all())
    layers = []
    for b in bufs:
        out, ok = _collect(b, T, D, n)
        guards = guards and ok
        layers.append(out)
    return dict(rc=rc, layers=layers, values=_bits(values[GUARD:-GUARD]).view(n, n_layers).cpu(), value=_bits(value[GUARD:-GUARD]).cpu(),
                mu=_bits(mu[GUARD:-GUARD]).cpu(), guards=guards, weights=weights)


def _untouched(r):
    ok = bool((r["values"] == FILL_BITS).all() and (r["value"] == FILL_BITS).all() and (r["mu"] == FILL_BITS).all())
    for l in r["layers"]:
        ok = ok and bool((l["part"] == FILL_BITS).all() and (_bits16(l["delta"]) == 0x7FC1).all()) and torch.equal(_bits(l["dk"]), _bits(l["dk0"]))
    return ok


def _run_one_block(T, D, pairs, layer, scale, mode="mean", pattern=True):
    """the existing one-block hook, splice_key_gram_pairs, on table entry `layer`'s operands and prefills"""
    b = _layer_buffers(T, D, pairs, layer, mode, 0.0, pattern, 0, pairs)
    geo, ptr = b["geo"], b["ptr"]
    value = torch.full((pairs,), PART_FILL, device=DEV)
    rc = _lib.lib().splice_key_gram_pairs(ptr["k_x"], geo["ldk"], geo["Rk"] * geo["ldk"], ptr["kT_x"], geo["ldt_x"], geo["Tp"], ptr["kT_b"], geo["ldt_b"], geo["Tp"], T, D, pairs,
                                          scale, ptr["delta"], ptr["part"], geo["part_ps"], _at(value), ptr["dk"], geo["lddk"], geo["Rd"] * geo["lddk"], _st())
    torch.cuda.synchronize()
    out, ok = _collect(b, T, D, pairs)
    assert rc == 0 and ok
    out["value"] = value.cpu()
    return out


def _reference(T, D, pairs, p, n_layers, centered, mode="mean"):
    """np_key_gram_layers on pair p's bf16 values in float64, and per entry the bounds of its addend and of every key-gradient element,
    derived from the arithmetic include/splice_hip.h states for splice_key_gram_layers_pairs, with the reference's absolute-value sums.
    Uncentred (tests/test_key_gram_gpu.py::_reference, with the entry's weight):
      Delta_ij: one fp32 accumulator over the 2 T exact bf16 x bf16 products, then the rounded 1 / T and one product:
          E_ij = 2 T 2^-23 A_ij + 3 2^-24 |Delta_ij|,   A = (|K_x|^T |K_x| + |K_B|^T |K_B|) / T
    Centred:
      mu_f = fl(S fl(1 / T)), S a sum of exact bf16 values through at most ceil(T / 64) lane-strided additions and 6 tree levels:
          e_f = (ceil(T / 64) + 6 + 2) 2^-24 mean_t |K_tf|                      (the fp32 mean tree, the rounded 1 / T, the product)
      m_ij = fl(mu_x,i mu_x,j - fl(mu_b,i mu_b,j)), fused:
          Em_ij = (|mu_i| e_j + e_i |mu_j| + e_i e_j) for x' and for the target, + 2^-24 (|mu_b,i mu_b,j| + |m_ij|)
      Delta_ij = fl(acc fl(1 / T) - m_ij), fused, G = the uncentred difference:
          E_ij = 2 T 2^-23 A_ij + 2^-24 |G_ij| + Em_ij + 2^-24 |Delta_ij|
    Addend: every d^2 enters as (Delta + e)^2, |e| <= E, through at most 41 fp32 roundings (the 40 of the one-block term, and the product
    with the weight), all addends non-negative:  bound_a = w ((mean(2 |Delta| E + E^2)) (1 + 41 2^-24) + 41 2^-24 raw).
    The value adds the n addends ascending from 0: bound_v = sum of bound_a + n 2^-24 (sum of the addends + sum of bound_a).
    Key gradient.  Db = bf16(Delta + e): |Db - Delta| <= F = E + 2^-9 (|Delta| + E).  (K Db)_tj is an fp32 accumulation of D exact
    products.  Centred, r_j = sum_i Db_ji mu_x,i in four chains of D / 4 fused multiply-adds and two additions:
          R_j = (F |mu_x|)_j + ((|Delta| + F) e)_j + (D / 4 + 2) 2^-24 ((|Delta| + F) (|mu_x| + e))_j
    then fl(acc - r_j), one rounding, and fma(c32, that, prefill) with c32 the scale after two roundings:
          core_tj = c (D 2^-23 (|K| (|Delta| + F)) + |K| F + R_j + 2^-24 |K Delta - r|)_tj + 2 2^-24 |dK|_tj
          bound_g = core + 2^-24 (|prefill| + |dK| + core)"""
    weights = OP_WEIGHTS[n_layers]
    xs, bs = [], []
    for i in range(n_layers):
        kx, kb = _op_keys(T, D, pairs, i, mode)
        xs.append(kx[p].double().numpy())
        bs.append(kb[p].double().numpy())
    raw, addends, dks = np_key_gram_layers(xs, bs, OP_LAM, weights, centered)
    out = []
    for i, (x, b, w) in enumerate(zip(xs, bs, weights)):
        G = (x.T @ x - b.T @ b) / T
        A = (np.abs(x).T @ np.abs(x) + np.abs(b).T @ np.abs(b)) / T
        ax = np.abs(x)
        if centered:
            mx, mb = x.mean(0), b.mean(0)
            depth = -(-T // 64) + 6 + 2
            ex, eb = depth * U24 * ax.mean(0), depth * U24 * np.abs(b).mean(0)
            delta = G - (np.outer(mx, mx) - np.outer(mb, mb))
            Em = sum(np.outer(np.abs(m), e) + np.outer(e, np.abs(m)) + np.outer(e, e) for m, e in ((mx, ex), (mb, eb)))
            Em = Em + U24 * (np.abs(np.outer(mb, mb)) + np.abs(np.outer(mx, mx) - np.outer(mb, mb)))
            E = (2 * T * U23 * A + U24 * np.abs(G) + Em + U24 * np.abs(delta)) * SLACK
        else:
            delta = G
            E = (2 * T * U23 * A + 3 * U24 * np.abs(delta)) * SLACK
        raw_i = float(np.mean(delta * delta))
        bound_a = w * (np.mean(2 * np.abs(delta) * E + E * E) * (1 + 41 * U24) + 41 * U24 * raw_i)
        Fm = E + UBF * (np.abs(delta) + E)
        c = 4.0 * OP_LAM * w / (T * D * D)
        core = D * U23 * (ax @ (np.abs(delta) + Fm).T) + ax @ Fm.T
        g = x @ delta
        if centered:
            R = Fm @ np.abs(mx) + (np.abs(delta) + Fm) @ ex + (D / 4 + 2) * U24 * ((np.abs(delta) + Fm) @ (np.abs(mx) + ex))
            g = g - np.outer(np.ones(T), delta @ mx)
            core = core + R[None, :] + U24 * np.abs(g)
        core = c * core * SLACK + 2 * U24 * np.abs(dks[i])
        out.append(dict(addend=addends[i], bound_a=bound_a, dk=dks[i], core=core, delta=delta))
    bound_v = sum(o["bound_a"] for o in out) + n_layers * U24 * (sum(addends) + sum(o["bound_a"] for o in out))
    return raw, bound_v, out


OP_SHAPES = [(9, 64, 1), (65, 384, 2), (130, 384, 2), (65, 768, 1)]


@pytest.fixture(scope="module")
def op_runs():
    cache = {}

    def get(T, D, pairs, n_layers, centered, **kw):
        key = (T, D, pairs, n_layers, centered, tuple(sorted(kw.items())))
        if key not in cache:
            cache[key] = _run(T, D, pairs, n_layers, centered, **kw)
        return cache[key]
    return get


def _check_against_fp64(r, T, D, pairs, n_layers, centered, mode="mean", tag=""):
    """value, per-layer addends and every key-gradient element inside the derived bounds; rows >= T, the gap behind a row and the unused
    partial slots keep their bits; returns the worst fractions of the bounds (value, addend, dK)"""
    assert r["rc"] == 0 and r["guards"]
    tiles = _tiles(D)
    if not centered:
        assert (r["mu"] == FILL_BITS).all(), "the uncentred form wrote means"
    worst = [0.0, 0.0, 0.0]
    for i, l in enumerate(r["layers"]):
        assert (l["part"][:, tiles:] == FILL_BITS).all(), "partial slots beyond the tiles were written"
        assert torch.equal(_bits(l["dk"][:, T:]), _bits(l["dk0"][:, T:])), "a padding row of the key gradient moved"
        assert torch.equal(_bits(l["dk"][:, :, D:]), _bits(l["dk0"][:, :, D:])), "the gap behind a key-gradient row moved"
    for p in range(pairs):
        raw, bound_v, ref = _reference(T, D, pairs, p, n_layers, centered, mode)
        got_v = float(r["value"][p:p + 1].view(torch.float32).item())
        got_a = r["values"][p].view(torch.float32).double().numpy()
        acc = f32(0)
        for a in r["values"][p].view(torch.float32).numpy():
            acc = f32(acc + a)
        assert acc.tobytes() == f32(got_v).tobytes(), "value is not the fp32 sum of the addends, ascending from 0"
        worst[0] = max(worst[0], abs(got_v - raw) / bound_v)
        for i, (o, l) in enumerate(zip(ref, r["layers"])):
            pre = l["dk0"][p, :T, :D].double().numpy()
            got_g = l["dk"][p, :T, :D].double().numpy()
            bound_g = o["core"] + U24 * (np.abs(pre) + np.abs(o["dk"]) + o["core"])
            frac_g = float((np.abs(got_g - (pre + o["dk"])) / bound_g).max())
            frac_a = abs(got_a[i] - o["addend"]) / o["bound_a"]
            got_d = l["delta"][p].view(torch.bfloat16).double().numpy()
            assert np.isfinite(got_d).all() and np.isfinite(got_g).all()
            worst[1], worst[2] = max(worst[1], frac_a), max(worst[2], frac_g)
            print(f"KEY_GRAM_LAYERS op{tag} T={T} D={D} n={n_layers} {'centred' if centered else 'uncentred'} pair {p} entry {i} (w {r['weights'][i]}): addend {got_a[i]:.7g} "
                  f"ref {o['addend']:.7g} err/bound {frac_a:.4f}; dK worst err/bound {frac_g:.4f}, norm-wise rel {np.linalg.norm(got_g - pre - o['dk']) / max(np.linalg.norm(o['dk']), 1e-300):.3e}")
            assert frac_a <= 1.0, (p, i, got_a[i], o["addend"], o["bound_a"])
            assert frac_g <= 1.0, (p, i, frac_g)
        print(f"KEY_GRAM_LAYERS op{tag} T={T} D={D} n={n_layers} {'centred' if centered else 'uncentred'} pair {p}: value {got_v:.7g} ref {raw:.7g} err/bound {abs(got_v - raw) / bound_v:.4f}")
        assert abs(got_v - raw) <= bound_v, (p, got_v, raw, bound_v)
        if centered and mode == "mean":   # the other form's reference lies outside this form's bound: a kernel that ignores the flag fails
            other = np_key_gram_layers([_op_keys(T, D, pairs, i, mode)[0][p].double().numpy() for i in range(n_layers)],
                                       [_op_keys(T, D, pairs, i, mode)[1][p].double().numpy() for i in range(n_layers)], OP_LAM, r["weights"], False)[0]
            assert abs(other - raw) > bound_v, (other, raw, bound_v)
    print(f"KEY_GRAM_LAYERS op{tag} T={T} D={D} n={n_layers} {'centred' if centered else 'uncentred'}: worst err/bound value {worst[0]:.4f} addend {worst[1]:.4f} dK {worst[2]:.4f}")
    return worst


@pytest.mark.parametrize("T,D,pairs", OP_SHAPES)
@pytest.mark.parametrize("n_layers", [1, 3])
@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_values_and_key_gradients_against_fp64(op_runs, T, D, pairs, n_layers, centered):
    """On the same bf16 values; one entry: the key-gradient buffers zero inside, three: prefilled with a seeded pattern (the result is
    pattern + dK, one fp32 rounding more: the bound's last term)."""
    _check_against_fp64(op_runs(T, D, pairs, n_layers, centered, pattern=n_layers == 3), T, D, pairs, n_layers, centered)


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_a_full_table_of_twelve_entries(centered):
    r = _run(65, 384, 1, 12, centered)
    _check_against_fp64(r, 65, 384, 1, 12, centered, tag=" full table")
    assert len({int(v) for v in r["values"][0]}) == 12   # (twelve entries, twelve different addends)


@pytest.mark.parametrize("T,D,pairs", OP_SHAPES)
@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_padding_columns_reach_no_output_bit(op_runs, T, D, pairs, centered):
    """the token columns >= T of both transposed copies filled with 1e4 against zeros there: every output has the same bits, the means
    included"""
    a, b = op_runs(T, D, pairs, 3, centered, pattern=True), op_runs(T, D, pairs, 3, centered, pattern=True, pad=1e4)
    assert a["rc"] == 0 and b["rc"] == 0 and b["guards"]
    assert torch.equal(a["value"], b["value"]) and torch.equal(a["values"], b["values"]) and torch.equal(a["mu"], b["mu"])
    for la, lb in zip(a["layers"], b["layers"]):
        assert torch.equal(la["part"], lb["part"]) and torch.equal(_bits16(la["delta"]), _bits16(lb["delta"])) and torch.equal(_bits(la["dk"]), _bits(lb["dk"]))
        assert bool(torch.isfinite(lb["dk"]).all())


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_a_pair_of_a_batched_launch_equals_its_own_launch(op_runs, centered):
    """pair 1 of the two-pair launch against the one-pair launch on its operands: every output bit for bit"""
    for T in (65, 130):
        two = op_runs(T, 384, 2, 3, centered, pattern=False)
        one = _run(T, 384, 2, 3, centered, pattern=False, first_pair=1)
        assert one["rc"] == 0 and one["guards"]
        assert torch.equal(two["values"][1], one["values"][0]) and torch.equal(two["value"][1:2], one["value"][0:1])
        if centered:
            assert torch.equal(two["mu"].view(3, 2, -1)[:, 1], one["mu"].view(3, 1, -1)[:, 0])
        for l2, l1 in zip(two["layers"], one["layers"]):
            assert torch.equal(l2["part"][1], l1["part"][0]) and torch.equal(_bits16(l2["delta"][1]), _bits16(l1["delta"][0]))
            assert torch.equal(_bits(l2["dk"][1, :T, :384]), _bits(l1["dk"][0, :T, :384]))
        assert not torch.equal(two["value"][0:1], two["value"][1:2])


@pytest.mark.parametrize("T,D,pairs", [(9, 64, 1), (65, 384, 2), (130, 384, 2)])
def test_an_entry_of_the_uncentred_launch_equals_the_one_block_hook(op_runs, T, D, pairs):
    """entry i (weights 0.5, 1, 3) against splice_key_gram_pairs on its operands with the entry's scale: delta, partials and key gradient
    bit for bit, and the addend is fl(w * its value)"""
    r = op_runs(T, D, pairs, 3, False, pattern=True)
    assert r["rc"] == 0
    for i, w in enumerate(OP_WEIGHTS[3]):
        one = _run_one_block(T, D, pairs, i, _scale(T, D, w))
        l = r["layers"][i]
        assert torch.equal(_bits16(l["delta"]), _bits16(one["delta"])) and torch.equal(l["part"], one["part"]), i
        assert torch.equal(_bits(l["dk"]), _bits(one["dk"])), i
        want = (f32(w) * one["value"].numpy()).astype(f32)
        assert want.tobytes() == r["values"][:, i].view(torch.float32).numpy().tobytes(), (i, w)
    if T == 65:   # weight 1: the scale has the bits of the one-block scale
        assert f32(_scale(T, D, 1.0)).tobytes() == f32(4.0 * OP_LAM / (T * D * D)).tobytes()


def test_two_entries_on_one_key_gradient_buffer_are_refused():
    """the choice DESIGN.md section 9o states: refused, nothing launched (the step never builds such a table: a block is listed once)"""
    r = _run(65, 384, 1, 3, False, share_dk=True)
    assert r["rc"] == ERR_ARG and r["guards"] and _untouched(r)


@pytest.mark.parametrize("T,D,pairs", [(65, 384, 2), (65, 768, 1)])
def test_equal_keys_centred_give_zero_within_the_bound(T, D, pairs):
    r = _run(T, D, pairs, 3, True, mode="equal", pattern=False)
    assert r["rc"] == 0 and r["guards"]
    for p in range(pairs):
        raw, bound_v, ref = _reference(T, D, pairs, p, 3, True, "equal")
        assert raw == 0.0 and not any(o["dk"].any() for o in ref)
        got_v = float(r["value"][p:p + 1].view(torch.float32).item())
        worst = max(float((np.abs(l["dk"][p, :T, :D].double().numpy()) / (o["core"] * (1 + U24))).max()) for o, l in zip(ref, r["layers"]))
        print(f"KEY_GRAM_LAYERS op equal keys centred T={T} D={D} pair {p}: value {got_v:.3e} (bound {bound_v:.3e}), worst |dK| / bound {worst:.4f}")
        assert abs(got_v) <= bound_v and worst <= 1.0


@pytest.mark.parametrize("T,D,pairs", [(65, 384, 2), (130, 384, 2)])
def test_token_constant_keys_centred_cancel_within_the_bound(T, D, pairs):
    """keys constant along the tokens on both sides, with different constants: every M is zero in exact arithmetic -- the cancellation case
    of acc / T - m -- so value and key gradient lie within the bound of zero; the uncentred reference lies far outside it"""
    r = _run(T, D, pairs, 3, True, mode="const", pattern=False)
    assert r["rc"] == 0 and r["guards"]
    for p in range(pairs):
        raw, bound_v, ref = _reference(T, D, pairs, p, 3, True, "const")
        assert raw <= 1e-25
        got_v = float(r["value"][p:p + 1].view(torch.float32).item())
        worst = max(float((np.abs(l["dk"][p, :T, :D].double().numpy() - o["dk"]) / (o["core"] * (1 + U24))).max()) for o, l in zip(ref, r["layers"]))
        unc = _reference(T, D, pairs, p, 3, False, "const")[0]
        print(f"KEY_GRAM_LAYERS op token-constant keys centred T={T} D={D} pair {p}: value {got_v:.3e} (bound {bound_v:.3e}; uncentred reference {unc:.3e}), worst |dK| / bound {worst:.4f}")
        assert abs(got_v - raw) <= bound_v and worst <= 1.0
        assert unc > bound_v


def test_op_refusals_launch_nothing():
    T, D = 65, 384
    cases = [dict(n_arg=0), dict(n_arg=13), dict(n_arg=-1), dict(D_arg=96), dict(D_arg=0), dict(ld_off=("ldt_x", 4)), dict(ld_off=("ldt_b", 2)), dict(ld_off=("ldk", 4)),
             dict(ld_off=("lddk", -16))] + [dict(null=(1, k)) for k in ("k_x", "kT_x", "kT_b", "delta", "part", "dk")] + [dict(null=("table", k)) for k in ("k_x", "dk")]
    for centered in (False, True):
        for kw in cases:
            r = _run(T, D, 2, 3, centered, **kw)
            assert r["rc"] == ERR_ARG and r["guards"] and _untouched(r), (centered, kw)
    assert _run(T, D, 2, 3, False, n_pairs=0)["rc"] == ERR_ARG


# ------------------------------------------------------------------------------------------------ step level
GEN_SEED = 41
VALUE_BAR = 1e-2            # what the teacher-forced test and the sibling layer tests hold a reported loss to
TEACHER_FORCED_BAR = 3e-2   # tests/test_step_gpu.py::test_step_gradients_vs_oracle_teacher_forced
KG_LAM = 2.0
KG_LAYERS, KG_WEIGHTS = [2, 5, 11], [0.5, 1.0, 2.0]


@pytest.fixture(scope="module")
def vit_state():
    return synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)


@pytest.fixture(scope="module")
def vit(vit_state):
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(vit_state)


def _cfg(**over):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed=40, pair=2):   # (tests/test_key_gram_gpu.py::_pair)
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _engine(vit, entire=True, **over):
    return SpliceEngine(_cfg(**over), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64) if entire else None, vit_engine=vit)


def _keys(centered=False, layers=KG_LAYERS, weights=KG_WEIGHTS, lam=KG_LAM):
    return {LAM: lam, LAYERS: list(layers), WEIGHTS: None if weights is None else list(weights), CENTERED: centered}


@pytest.fixture(scope="module")
def oracle_vit(vit_state):
    m = dino_vit.VisionTransformer(8, 384, 12, 6, img_size=64).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vit_state.items()})
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _oracle_keys(m, img, layers):
    """the [T][D] fp32 keys of the blocks `layers` of the oracle ViT, every token, the heads concatenated"""
    qkv = dino_vit.forward_features(m, olosses.normalize(img).unsqueeze(0))["qkv"]
    D = qkv[0].shape[-1] // 3
    return [qkv[l].reshape(-1, 3 * D)[:, D:2 * D] for l in layers]


def _moment(k, centered):
    g = k.T @ k / k.shape[0]
    if centered:
        mu = k.mean(0)
        g = g - torch.outer(mu, mu)
    return g


def _oracle_loss(m, x, b, layers, weights, centered):
    with torch.no_grad():
        want = [_moment(k, centered) for k in _oracle_keys(m, b, layers)]
    return sum(w * F.mse_loss(_moment(k, centered), g) for k, g, w in zip(_oracle_keys(m, x, layers), want, weights))


def _fmaf32(a, b, c):
    """fl32(a * b + c) with one rounding, from exact rationals (ties to even)"""
    exact = Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c))
    g = f32(float(exact))
    cands = [np.nextafter(g, f32(-np.inf)), g, np.nextafter(g, f32(np.inf))]
    return min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.int32)) & 1))


def _word0(row, cfg, entire, kg):
    """the total-loss kernel's chain on the reported words, in float32: one product, four fused multiply-adds, then this term's fused
    multiply-add (the steps compared lie behind cls_warmup)"""
    w = {k: f32(cfg[k]) for k in ("lambda_global_ssim", "lambda_entire_ssim", "lambda_entire_cls", "lambda_global_cls", "lambda_global_identity")}
    w_essim, w_ecls = (w["lambda_entire_ssim"], w["lambda_entire_cls"]) if entire else (f32(0), f32(0))
    t = f32(w_essim * f32(row[2]))
    t = _fmaf32(w["lambda_global_ssim"], row[1], t)
    t = _fmaf32(w_ecls, row[3], t)
    t = _fmaf32(w["lambda_global_cls"], row[4], t)
    t = _fmaf32(w["lambda_global_identity"], row[5], t)
    return _fmaf32(f32(cfg[LAM]), f32(kg), t)


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_step_reports_the_addends_their_sum_and_word_0(vit, oracle_vit, centered):
    """[2, 5, 11] with weights [0.5, 1, 2]; lr 0, cls_warmup 0, entire_A_every 2: step 0 is an entire-image step, step 1 an ordinary one.
    Every per-layer addend against np_key_gram_layers of the oracle ViT's fp32 keys on the plan's own forward output and on the B crop,
    1e-2 relative; their fp32 ascending sum is the reported value exactly; word 0 is the kernel's fused multiply-add chain on the
    reported words, exactly; the parameters do not move."""
    A, B = _pair()
    eng = _engine(vit, lr=0.0, cls_warmup=0, entire_A_every=2, **_keys(centered))
    assert eng.key_gram_layers == (KG_LAM, KG_LAYERS, KG_WEIGHTS, centered) and eng.key_gram is not None
    assert eng.cfg[LAYERS] == KG_LAYERS and eng.cfg[LAYER] is None and eng.cfg[CENTERED] is centered
    p0 = eng.params.clone()
    x = GeneratorPlan(eng.gen, 1, 64, 64, True, 0).forward(eng.params, A[None])[0].cpu()
    raw, addends, _ = np_key_gram_layers([k.numpy() for k in _oracle_keys(oracle_vit, x, KG_LAYERS)], [k.numpy() for k in _oracle_keys(oracle_vit, B.cpu(), KG_LAYERS)],
                                         KG_LAM, KG_WEIGHTS, centered)
    for step in range(2):
        eng.step(A, B, A)
        entire = step % 2 == 0
        row = eng.losses_dev[0].cpu().numpy()
        got, per = eng.key_gram_value(), eng.key_gram_layer_values()
        losses = eng.losses()
        rel = [abs(float(per[i]) - addends[i]) / addends[i] for i in range(3)]
        print(f"KEY_GRAM_LAYERS step {step} ({'entire-image' if entire else 'ordinary'}) {'centred' if centered else 'uncentred'}: addends {[float(v) for v in per]}, oracle "
              f"{addends}, rel {['%.2e' % r for r in rel]}; value {got:.7g}, oracle {raw:.7g}, rel {abs(got - raw) / raw:.2e}; bar {VALUE_BAR:.0e}")
        assert per.dtype == f32 and per.shape == (3,)
        acc = f32(0)
        for v in per:
            acc = f32(acc + v)
        assert acc.tobytes() == f32(got).tobytes()
        assert max(rel) <= VALUE_BAR and abs(got - raw) / raw <= VALUE_BAR, (step, rel, got, raw)
        assert losses[KEY_GRAM_LOSS_KEY] == got and losses["loss"] == float(row[0])
        assert row[0].tobytes() == _word0(row, eng.cfg, entire, got).tobytes(), (step, row, got)
    assert torch.equal(eng.params, p0)


@pytest.fixture(scope="module")
def grad_errs(vit, oracle_vit):
    """per term ("ssim": the structure term alone at the default layer, what the parent commit computes too; False / True: this term alone
    on [2, 5, 11], uncentred / centred): whole-arena relative L2 of the step's generator gradient against plan.backward of the oracle's
    autograd image gradient on the plan's own forward output, and the relative error of word 0.  Conv biases in front of a BatchNorm left
    out."""
    cache = {}

    def get(name):
        if name not in cache:
            A, B = _pair()
            off = dict(lambda_global_cls=0.0, lambda_global_identity=0.0, lambda_entire_cls=0.0, lambda_entire_ssim=0.0, cls_warmup=0, lr=0.0)
            if name == "ssim":
                eng = _engine(vit, entire=False, **off)
            else:
                eng = _engine(vit, entire=False, **off, lambda_global_ssim=0.0, **_keys(name))
            p0 = eng.params.clone()
            eng.step(A, B)
            assert torch.equal(eng.params, p0)
            plan = GeneratorPlan(eng.gen, 1, 64, 64, True, 0)
            x = plan.forward(eng.params, A[None])[0].cpu().clone().requires_grad_(True)
            if name == "ssim":
                with torch.no_grad():
                    target = oex.keys_self_sim_from_input(oracle_vit, olosses.normalize(A.cpu()).unsqueeze(0), layer=11)
                loss = F.mse_loss(oex.keys_self_sim_from_input(oracle_vit, olosses.normalize(x).unsqueeze(0), layer=11), target) * eng.cfg["lambda_global_ssim"]
            else:
                loss = KG_LAM * _oracle_loss(oracle_vit, x, B.cpu(), KG_LAYERS, KG_WEIGHTS, name)
            dx, = torch.autograd.grad(loss, x)
            g_ref = plan.backward(eng.params, dx[None].to(DEV).contiguous())
            num = den = 0.0
            for (pname, g), r in zip(eng.gen.unflatten(eng.grads).items(), eng.gen.unflatten(g_ref).values()):
                if pname.endswith("0.bias") and pname != "9.0.bias":
                    continue   # zero-gradient conv biases (feed a BatchNorm)
                num += (g.double() - r.double()).pow(2).sum().item()
                den += r.double().pow(2).sum().item()
            cache[name] = ((num / den) ** 0.5, abs(eng.losses_dev[0, 0].item() - loss.item()) / loss.item(), eng.grads.clone())
        return cache[name]
    return get


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_step_gradient_against_the_oracle_through_the_same_plan(grad_errs, centered):
    """Only this term on, [2, 5, 11] with weights [0.5, 1, 2].  The yardstick is the identical comparison for the structure term alone at
    the default layer; the term is held to the larger of three times that figure and the teacher-forced bar."""
    yard, yard_loss, _ = grad_errs("ssim")
    err, loss_err, _ = grad_errs(centered)
    bar = max(3 * yard, TEACHER_FORCED_BAR)
    print(f"KEY_GRAM_LAYERS gradient {'centred' if centered else 'uncentred'} [2, 5, 11]: rel L2 {err:.3e} (total rel {loss_err:.2e}); structure term, default layer {yard:.3e} "
          f"(total rel {yard_loss:.2e}); bar {bar:.3e}")
    assert err <= bar and loss_err < 1e-2 and yard_loss < 1e-2


def _arenas(eng, pair=0):
    n, st = eng.gen.numel, eng.stride
    sl = slice(pair * st, pair * st + n)
    return dict(params=eng.params[sl].clone(), m=eng.m[sl].clone(), v=eng.v[sl].clone(), running=eng.running[pair].clone(), losses=eng.losses_dev[pair].clone())


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


def _walk(eng, twin, A, B, check_value=False):
    """6 steps over the regimes -- [CLS] warm-up (steps 0-1), entire-image steps (0, 4), an unequal crop (step 3) --, the same bytes everywhere"""
    A2 = A[:, :60, :60].contiguous()
    for i in range(6):
        for e in (eng, twin):
            e.step(A2 if i == 3 else A, B, A)
        assert torch.equal(_bits(eng.losses_dev), _bits(twin.losses_dev)) and torch.equal(_bits(eng.grads), _bits(twin.grads)), i
        if check_value:
            assert f32(eng.key_gram_value()).tobytes() == f32(twin.key_gram_value()).tobytes(), i
    assert _same(_arenas(eng), _arenas(twin))


@pytest.mark.parametrize("spelling", [{LAYERS: [5]}, {LAYERS: [5], WEIGHTS: [1.0], CENTERED: False}], ids=["list", "list-weights-flag"])
def test_a_one_entry_list_is_the_one_block_configuration(vit, spelling):
    """dino_gram_layers [5], weight 1, not centred, against dino_gram_layer 5: the old setter, the old launches, the same bytes over the
    six-step regime walk"""
    A, B = _pair()
    eng = _engine(vit, cls_warmup=2, entire_A_every=4, **{LAM: KG_LAM}, **spelling)
    twin = _engine(vit, cls_warmup=2, entire_A_every=4, **{LAM: KG_LAM, LAYER: 5})
    assert eng.key_gram == (KG_LAM, 5) and eng.key_gram_layers is None and eng.cfg[LAYER] == 5 and eng.cfg[LAYERS] is None
    _walk(eng, twin, A, B, check_value=True)
    assert eng.key_gram_value() > 0
    with pytest.raises(RuntimeError, match="dino_gram_layers"):
        eng.key_gram_layer_values()
    out = (C.c_float * 8)()
    assert _lib.lib().splice_step_key_gram_layer_values(eng.handle, out) != 0 and b"no key second-moment layers" in _lib.lib().splice_last_error()


def test_the_new_keys_at_their_defaults_are_the_engine_without_them(vit):
    A, B = _pair()
    cfg = {k: v for k, v in _cfg(cls_warmup=2, entire_A_every=4).items() if k not in KEY_GRAM_LAYER_KEYS}
    twin = SpliceEngine(cfg, None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64), vit_engine=vit)
    eng = _engine(vit, cls_warmup=2, entire_A_every=4, **{LAYERS: None, WEIGHTS: None, CENTERED: False})
    assert eng.key_gram is None and eng.key_gram_layers is None
    _walk(eng, twin, A, B)
    assert KEY_GRAM_LOSS_KEY not in eng.losses()
    # ... and beside the one-block term
    on = _engine(vit, cls_warmup=2, entire_A_every=4, **{LAM: KG_LAM, LAYER: 5, LAYERS: None, WEIGHTS: None, CENTERED: False})
    cfg_on = {k: v for k, v in _cfg(cls_warmup=2, entire_A_every=4, **{LAM: KG_LAM, LAYER: 5}).items() if k not in KEY_GRAM_LAYER_KEYS}
    _walk(on, SpliceEngine(cfg_on, None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64), vit_engine=vit), A, B, check_value=True)


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_batch_independence_two_pairs(vit, centered):
    """default lr, 3 steps behind the warm-up: each pair of a two-pair engine is, bit for bit, its own SpliceEngine run, addends included"""
    keys = _keys(centered)
    pairs = [_pair(40, 2), _pair(62, 0)]
    gens = [synth.generator_params(41, 0.02), synth.generator_params(61, 0.02)]
    multi = MultiPairEngine(_cfg(cls_warmup=1, **keys), None, gens, (64, 64), (64, 64), vit_engine=vit)
    A2, B2 = torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()
    rows, vals, pers = [], [], []
    for _ in range(3):
        multi.step(A2, B2, A2)
        rows.append(multi.losses_dev.clone())
        vals.append(multi.key_gram_value())
        pers.append(multi.key_gram_layer_values())
    for p in range(2):
        single = SpliceEngine(_cfg(cls_warmup=1, **keys), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for k in range(3):
            single.step(pairs[p][0], pairs[p][1], pairs[p][0])
            assert torch.equal(_bits(single.losses_dev[0]), _bits(rows[k][p])), (p, k)
            assert f32(single.key_gram_value()).tobytes() == f32(vals[k][p]).tobytes(), (p, k)
            assert single.key_gram_layer_values().tobytes() == pers[k][p].tobytes(), (p, k)
        assert multi.key_gram_layer_values(p).tobytes() == pers[2][p].tobytes()
        assert _same(_arenas(multi, p), _arenas(single)), p
        assert vals[2][p] > 0 and vals[0][p] == 0 and not pers[0][p].any()   # (step 0 lies before the warm-up step: the term has not run)


def test_graph_replay_equals_eager(vit):
    """Four steps on fixed crops with lr 0: step 1 is launched eagerly, step 2 captures the graph, step 3 replays it; then an engine that
    never captures.  Behind it other settings in the same process -- another list, another weight, the other flag --: their own graphs,
    their own numbers (the pool's salt carries all three)."""
    A, B = _pair()
    keys = _keys(True)
    eng = _engine(vit, lr=0.0, cls_warmup=0, **keys)
    seen = []
    for _ in range(4):
        eng.step(A, B, A)
        seen.append((eng.grads.clone(), eng.m.clone(), eng.losses_dev.clone()))
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    assert stats[0] + stats[2] >= 1                                     # a graph was in use
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(seen[3], seen[1]))   # (both ordinary steps; steps 0 and 2 are entire-image steps)
    val, per = eng.key_gram_value(), eng.key_gram_layer_values()
    eager = _engine(vit, lr=0.0, cls_warmup=0, **keys)
    _lib.check(_lib.lib().splice_step_use_graph(eager.handle, 0), "use_graph")
    for _ in range(4):
        eager.step(A, B, A)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((eager.grads, eager.m, eager.losses_dev), seen[3]))
    assert eager.key_gram_value() == val and val > 0 and eager.key_gram_layer_values().tobytes() == per.tobytes()
    for other_keys in (_keys(True, layers=[2, 7, 11]), _keys(True, weights=[0.5, 1.0, 3.0]), _keys(False)):
        other = _engine(vit, lr=0.0, cls_warmup=0, **other_keys)
        other_eager = _engine(vit, lr=0.0, cls_warmup=0, **other_keys)
        _lib.check(_lib.lib().splice_step_use_graph(other_eager.handle, 0), "use_graph")
        for _ in range(4):
            other.step(A, B, A)
            other_eager.step(A, B, A)
        assert torch.equal(_bits(other.m), _bits(other_eager.m)) and torch.equal(_bits(other.losses_dev), _bits(other_eager.losses_dev))
        assert not torch.equal(_bits(other.losses_dev), _bits(seen[3][2]))


@pytest.mark.parametrize("centered", [False, True], ids=["uncentred", "centred"])
def test_together_with_structure_layers_sharing_one_block(vit, grad_errs, centered):
    """dino_ssim_layers [5, 11] and dino_gram_layers [2, 5]: block 5's key-gradient buffer is shared -- the structure term stores, this term
    adds -- and block 2's is this term's own, zeroed each step.  lr 0, only these two terms on.  The generator gradient equals the sum of
    the two single-term gradients within the gradient bar; each term's values have the bits of the engine that carries it alone."""
    A, B = _pair()
    sk, gk = {S_LAYERS: [5, 11]}, _keys(centered, layers=[2, 5], weights=[0.5, 2.0])
    base = dict(lr=0.0, cls_warmup=0, lambda_global_cls=0.0, lambda_global_identity=0.0)
    both = _engine(vit, entire=False, **base, **sk, **gk)
    only_s = _engine(vit, entire=False, **base, **sk)
    only_g = _engine(vit, entire=False, **base, **gk, lambda_global_ssim=0.0)
    first = None
    for _ in range(2):   # (twice: the second step meets the buffers the first one left, block 2's own among them)
        for e in (both, only_s, only_g):
            e.step(A, B)
        if first is None:
            first = (both.grads.clone(), only_g.grads.clone())
    assert torch.equal(_bits(first[0]), _bits(both.grads)) and torch.equal(_bits(first[1]), _bits(only_g.grads))
    assert both.key_gram_layer_values().tobytes() == only_g.key_gram_layer_values().tobytes() and both.key_gram_value() > 0
    assert f32(both.key_gram_value()).tobytes() == f32(only_g.key_gram_value()).tobytes()
    assert both.ssim_layer_values().tobytes() == only_s.ssim_layer_values().tobytes()
    want = only_s.grads.double() + only_g.grads.double()
    assert bool(only_s.grads.abs().max() > 0) and bool(only_g.grads.abs().max() > 0)
    rel = ((both.grads.double() - want).norm() / want.norm()).item()
    share = (only_g.grads.double().norm() / want.norm()).item()
    bar = max(3 * grad_errs("ssim")[0], TEACHER_FORCED_BAR)
    print(f"KEY_GRAM_LAYERS {'centred' if centered else 'uncentred'} [2, 5] with structure layers [5, 11]: combined gradient against the sum of the single-term gradients rel L2 "
          f"{rel:.3e} (this term's share of the norm {share:.2e}); bar {bar:.3e}")
    assert rel <= bar and share > 1e-3


def test_snapshot_is_refused_under_another_list_weight_or_flag(vit):
    A, B = _pair()
    eng = _engine(vit, **_keys(True))
    eng.step(A, B, A)
    state = eng.snapshot(0)
    for other, key in ((_keys(True, layers=[2, 7, 11]), LAYERS), (_keys(True, weights=[0.5, 1.0, 3.0]), WEIGHTS), (_keys(False), CENTERED)):
        with pytest.raises(ValueError, match="'" + key + "'"):
            _engine(vit, **other).restore([state])
    with pytest.raises(ValueError, match="dino_gram"):
        _engine(vit, **{LAM: KG_LAM, LAYER: 5}).restore([state])
    same = _engine(vit, **_keys(True))
    same.restore([state])
    eng.step(A, B, A)
    same.step(A, B, A)
    assert torch.equal(_bits(same.params), _bits(eng.params)) and torch.equal(_bits(same.losses_dev), _bits(eng.losses_dev))
    assert same.key_gram_layer_values().tobytes() == eng.key_gram_layer_values().tobytes()


def test_setter_refusals(vit, vit_state):
    L = _lib.lib()
    A, B = _pair()
    eng = _engine(vit)

    def call(handle, lam, layers, weights, centered=0):
        n = len(layers)
        return L.splice_step_set_key_gram_layers(handle, lam, n, (C.c_int * max(n, 1))(*layers), (C.c_float * max(n, 1))(*weights), centered)
    for lam in (0.0, -1.0, float("nan"), float("inf")):
        assert call(eng.handle, lam, [2, 5], [1.0, 1.0]) != 0 and b"finite and > 0" in L.splice_last_error()
    assert call(eng.handle, 1.0, [], []) != 0 and b"1..12 layers" in L.splice_last_error()
    assert call(eng.handle, 1.0, list(range(12)) + [11], [1.0] * 13) != 0 and b"1..12 layers" in L.splice_last_error()
    for layers in ([5, 2], [5, 5], [-1, 5], [5, 12]):
        assert call(eng.handle, 1.0, layers, [1.0, 1.0]) != 0 and b"ascending distinct" in L.splice_last_error()
    for w in (0.0, -1.0, float("nan"), float("inf")):
        assert call(eng.handle, 1.0, [2, 5], [1.0, w]) != 0 and b"weights must be finite" in L.splice_last_error()
    assert call(eng.handle, 1.0, [2, 5], [1.0, 1.0], 2) != 0 and b"centered" in L.splice_last_error()
    assert L.splice_step_set_key_gram_layers(eng.handle, 1.0, 2, None, None, 0) != 0
    out = (C.c_float * 8)()
    assert L.splice_step_key_gram_layer_values(eng.handle, out) != 0 and b"no key second-moment layers" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert call(eng.handle, 1.0, [2, 5], [1.0, 1.0]) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    lead = _engine(vit)
    assert L.splice_step_set_phases(eng.handle, 2, lead.handle) == 0
    assert call(eng.handle, 1.0, [2, 5], [1.0, 1.0]) != 0 and b"phase mode" in L.splice_last_error()
    assert L.splice_step_set_phases(eng.handle, 7, None) == 0
    eng.step(A, B, A)
    assert call(eng.handle, 1.0, [2, 5], [1.0, 1.0]) != 0 and b"before the first step" in L.splice_last_error()
    # the two setters exclude each other, in either order
    on = _engine(vit, **_keys(False))
    assert call(on.handle, 1.0, [2, 5], [1.0, 1.0]) != 0 and b"once" in L.splice_last_error()
    assert L.splice_step_set_key_gram(on.handle, 1.0, 5) != 0 and b"once" in L.splice_last_error()
    old = _engine(vit, **{LAM: 1.0, LAYER: 5})
    assert call(old.handle, 1.0, [2, 5], [1.0, 1.0]) != 0 and b"once" in L.splice_last_error()
    # what the one-block setter's handle refuses behind it, this one's refuses too
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"key second-moment" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 2, lead.handle) != 0 and b"key second-moment" in L.splice_last_error()
    two, w2 = (C.c_int * 2)(3, 11), (C.c_float * 2)(1.0, 1.0)
    assert L.splice_step_set_ssim_layers(on.handle, 2, two, w2) != 0 and b"in front of" in L.splice_last_error()   # (shared buffers: structure layers first)
    assert L.splice_step_key_gram_layer_values(on.handle, out) == 0 and out[0] == 0.0 and out[2] == 0.0   # (no step yet)
    assert L.splice_step_key_gram_values(on.handle, out) == 0 and out[0] == 0.0
    with pytest.raises(ValueError, match="'lambda_global_key_gram'.*crop counts"):
        MultiPairEngine(_cfg(**_keys(True)), None, [synth.generator_params(41, 0.02)] * 2, (64, 64), None, vit_engine=vit, n_crops=(2, 1))
    # fp8: the C setter refuses what the Python engine refuses on the host (an engine of its own: the e4m3 weights stay with it)
    from splice_amd.vit import VitEngine
    vit8 = VitEngine("dino_vits8", device=DEV).load_state_dict(vit_state)
    e8 = SpliceEngine(_cfg(), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit8, fp8=True)
    assert call(e8.handle, 1.0, [2, 5], [1.0, 1.0]) != 0 and b"fp8" in L.splice_last_error()
    with pytest.raises(ValueError, match="fp8"):
        SpliceEngine(_cfg(**_keys(True)), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit8, fp8=True)
