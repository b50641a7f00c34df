"""CPU: the walk classes, references, bounds, rescale prediction and fp32 emulation of oracle/attention.py, which tests/test_attention_gpu.py holds
the full-sequence attention kernels to (attn_x32.h, attn_bwd_x32.h, attention.hip).  Without a GPU:
  1. ATTN_T reaches every value of every component of the three walk-class functions for 2, 4 and 8 waves, of the class of the 16x16x32 halves and
     of the e4m3 forward, and the pairs (remainder class, Tld % 64) and (ring phase, masked last tile); the assertion lists what is missing;
  2. the partner condition: every query's planted key holds a probability in [0.25, 0.9] at every T >= 2 (plain, pre-scaled and e4m3 operands);
  3. the unmodified emulation stays inside every bound at every case, and takes no lazy rescale in the partner and flat regimes;
  4. every bound is small against the signal: norm-wise under 1e-2 of the reference (tests/test_cls_tail_cpu.py's figure); the e4m3 output bound
     carries the format's 2^-4 step and its 2^-16 floor per key and is held under 2^-4 + T 2^-16 + 2e-2 (1e-2 for what the fp8 MFMA drops of a score, 1e-2 for the rest), its lse bound under 2^-5 log2 units;
  5. every deliberate defect of the emulation leaves a bound or breaks an exact statement wherever it is meaningful;
  6. the rescale predictor gives exactly the designed (query, tile) set at every ramp case, 2^4 clear of the threshold on either side.
The closed forms of the backward are checked against fp64 autograd on the way.
"""
import functools

import pytest
import torch

from oracle import attention as at

NORMWISE = 1e-2
D, H, B = at.BASE_GEOM


def _ratio(err, bound):
    return (err / bound.clamp(min=1e-300)).max().item()


def _normwise(bound, ref):
    return (bound.norm() / ref.norm()).item()


# ------------------------------------------------------------------------------------------------ 1. coverage
def _universe(fn, NW=None, fp8=None, limit=4096):
    """every value each component takes over T = 1 .. limit (all of them occur below 1024: the classes saturate)"""
    seen = {}
    for T in range(1, limit + 1):
        c = fn(T, NW) if NW is not None else fn(T, fp8)
        for k, v in c.items():
            seen.setdefault(k, set()).add(v)
    return seen


def test_attn_t_reaches_every_walk_class():
    missing = []
    expect = {  # written out from the loop structure, not only enumerated: a component that stopped varying would show here
        "fwd": dict(prologue={1, 2, 3, 4}, main={0, 1, 2}, tail={1, 2, 3, 4, 5, 6}, phase={0, 1, 2, 3, 4, 5}, rem={"0", "1..31", "32", "33..63"}, tld64={0, 32}),
        "bwd_q": dict(prologue={1, 2, 3}, main={0, 1, 2}, phase={0, 1, 2, 3}, rem={"0", "1..31", "32", "33..63"}, tld64={0, 32}),
        "bwd_kv": dict(prologue={1, 2, 3}, main={0, 1, 2}, phase={0, 1, 2, 3}, rem={"0", "1..31", "32", "33..63"}, tld64={0, 32}, half={False, True},
                       pad={False, True}),
    }
    for name, fn in (("fwd", at.fwd_class), ("bwd_q", at.bwd_q_class), ("bwd_kv", at.bwd_kv_class)):
        for NW in at.NWS:
            uni = _universe(fn, NW=NW)
            want = dict(expect[name], idle=set(range(NW)))
            assert uni == want, (name, NW, uni)
            got = {}
            for T in at.ATTN_T:
                for k, v in fn(T, NW).items():
                    got.setdefault(k, set()).add(v)
            missing += [(name, NW, k, sorted(want[k] - got[k], key=str)) for k in want if want[k] - got[k]]
    for fp8 in (False, True):
        uni = _universe(at.small_class, fp8=fp8)
        # the three components are tied (the remainder class fixes Tld % 64): the product that exists is what must be reached
        combos = {tuple(sorted(at.small_class(T, fp8).items())) for T in range(1, 4097)}
        got = {tuple(sorted(at.small_class(T, fp8).items())) for T in at.ATTN_T}
        assert uni["nt"] == {1, 2, 3, 4} and (not fp8 or uni["odd"] == {0, 1})
        missing += [("small", fp8, c) for c in sorted(combos - got, key=str)]
    # pairs
    for name, fn, period in (("fwd", at.fwd_class, 6), ("bwd_q", at.bwd_q_class, 4), ("bwd_kv", at.bwd_kv_class, 4)):
        pairs = {(fn(T, 4)["phase"], T % 64 != 0) for T in at.ATTN_T}
        missing += [(name, "phase x masked", p) for p in sorted({(ph, mk) for ph in range(period) for mk in (False, True)} - pairs)]
        rt = {(fn(T, 4)["rem"], fn(T, 4)["tld64"]) for T in at.ATTN_T}
        missing += [(name, "rem x tld64", p) for p in sorted({(fn(T, 4)["rem"], fn(T, 4)["tld64"]) for T in range(1, 4097)} - rt)]
    assert not missing, missing
    # what the existing op-level tests left unrun, by name
    assert any(at.fwd_class(T, 4)["tld64"] == 0 and T % 64 for T in at.ATTN_T)                    # full-tile DMA of a masked last tile
    assert {(T + 63) // 64 for T in at.ATTN_T} >= {1, 2, 3, 4, 5, 6, 7, 8, 9}
    assert max(at.ATTN_T) <= 897 and all(T <= 897 for T, *_ in at.WIDE_CASES)


def test_case_lists_are_consistent():
    assert set(at.PROBS_T) and any(T < 64 for T in at.PROBS_T) and any(T % 64 == 0 for T in at.PROBS_T) and any(T % 32 for T in at.PROBS_T)
    assert {at.rem_class(T) for T in at.CHAIN_T} == {"0", "1..31", "32", "33..63"} and set(at.CHAIN_T) <= set(at.ATTN_T)
    assert {T for T, *_ in at.RAMP_CASES} <= set(at.ATTN_T)
    lvl2 = [T for T, _, lv in at.RAMP_CASES if lv == 2]
    assert any(T % 64 == 0 for T in lvl2) and min(lvl2) == 65
    for T, tiles, _ in at.RAMP_CASES:
        assert all(0 < t < (T + 63) // 64 for t in tiles)
        for w in range(0, at.tld(T), 32):
            assert len([q for q in at.ramp_queries(T) if w <= q < w + 32]) < 32


# ------------------------------------------------------------------------------------------------ 2. - 5. forward
CASES = [(T, D, H, B) for T in at.ATTN_T] + at.WIDE_CASES


@functools.lru_cache(maxsize=4)
def _fwd(T, Dm, Hh, Bb, regime, fold, fp8=False):
    qkv = at.make_qkv(T, Dm, Hh, Bb, regime, fold, fp8=fp8)
    return qkv, at.forward_ref(qkv, T, Hh, fold)


def _fwd_worst(f, T, out, lse, E_lse, E_out):
    return max(_ratio((lse[:, :, :T].double() - f["lse"][:, :, :T]).abs(), E_lse), _ratio((out[:, :, :T].double() - f["out"][:, :, :T]).abs(), E_out))


@pytest.mark.parametrize("T,Dm,Hh,Bb", CASES)
def test_partner_condition(T, Dm, Hh, Bb):
    for fold, fp8 in ((False, False), (True, False), (False, True)):
        qkv, f = _fwd(T, Dm, Hh, Bb, "partner", fold, fp8)
        assert torch.equal(at.e4m3_round(qkv) if fp8 else at.bf16_round(qkv), qkv)
        if T >= 2:
            p = f["P"][:, :, torch.arange(T), at.partner_perm(T)]
            assert p.min().item() >= 0.25 and p.max().item() <= 0.9, (fold, fp8, p.min().item(), p.max().item())
    assert sorted(at.partner_perm(T).tolist()) == list(range(T))


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("regime", at.REGIMES)
@pytest.mark.parametrize("T,Dm,Hh,Bb", CASES)
def test_forward_emulation_bounds_and_mutations(T, Dm, Hh, Bb, regime, fold):
    qkv, f = _fwd(T, Dm, Hh, Bb, regime, fold)
    assert torch.equal(at.bf16_round(qkv), qkv) and (qkv[:, T:].abs().sum(-1) > 0).all() and qkv.abs().max() < 64
    E_lse, E_out = at.forward_bounds(f)
    fire, _, exact = at.rescale_plan(f)
    assert not fire.any() and not exact.any()                      # the bounds' premise: the reference point never moves in these regimes
    out, lse, n_resc = at.forward_emulate(qkv, T, Hh, fold)
    assert n_resc == 0
    worst = _fwd_worst(f, T, out, lse, E_lse, E_out)
    assert worst <= 1.0, worst
    assert _normwise(E_out, f["out"][:, :, :T]) < NORMWISE and E_lse.max().item() < 1e-3, (_normwise(E_out, f["out"][:, :, :T]), E_lse.max().item())
    # padding independence of the unmodified emulation, bit for bit
    qkv2 = at.make_qkv(T, Dm, Hh, Bb, regime, fold, pad_seed=1)
    assert torch.equal(qkv2[:, :T], qkv[:, :T]) and (T == at.tld(T) or not torch.equal(qkv2[:, T:], qkv[:, T:]))
    out2, lse2, _ = at.forward_emulate(qkv2, T, Hh, fold)
    assert torch.equal(out2[:, :, :T], out[:, :, :T]) and torch.equal(lse2[:, :, :T], lse[:, :, :T])
    for mut in at.FWD_MUTS:
        meaningful = dict(drop_last_key=T >= 2, admit_pad_key=T < at.tld(T), stale_tile=T > 64, skip_subtile=T % 64 != 0 and T >= 2,
                          heads_swapped=True, lse_missing_tile=True)[mut]
        if not meaningful:
            continue
        om, lm, _ = at.forward_emulate(qkv, T, Hh, fold, mut=mut)
        caught = not _fwd_worst(f, T, om, lm, E_lse, E_out) <= 1.0
        if mut == "admit_pad_key" and not caught:   # the exact statement: the bits then depend on what the padding holds
            o2, l2, _ = at.forward_emulate(qkv2, T, Hh, fold, mut=mut)
            caught = not (torch.equal(o2[:, :, :T], om[:, :, :T]) and torch.equal(l2[:, :, :T], lm[:, :, :T]))
        assert caught, mut


@pytest.mark.parametrize("regime", at.REGIMES)
@pytest.mark.parametrize("T", at.ATTN_T)
def test_fp8_forward_emulation_bounds(T, regime):
    qkv, f = _fwd(T, D, H, B, regime, False, True)
    assert torch.equal(at.e4m3_round(qkv), qkv)
    E_lse, E_out = at.forward_bounds(f, fp8=True)
    out, lse, _ = at.forward_emulate(qkv, T, H, fp8=True)
    assert _fwd_worst(f, T, out, lse, E_lse, E_out) <= 1.0
    # the format's own step (2^-4) and floor (2^-16 of the largest probability, at each of T keys) are the kernel's design; the score bits the
    # fp8 MFMA drops and the rest are held to NORMWISE each
    assert _normwise(E_out, f["out"][:, :, :T]) < 2.0 ** -4 + T * 2.0 ** -16 + 2 * NORMWISE and E_lse.max().item() < 2.0 ** -5
    if T >= 2:
        om, lm, _ = at.forward_emulate(qkv, T, H, fp8=True, mut="drop_last_key")
        assert not _fwd_worst(f, T, om, lm, E_lse, E_out) <= 1.0
    if regime == "flat" and T > 128:
        assert at.fp8_limit_hits(f) > 0


# ------------------------------------------------------------------------------------------------ 6. the ramp
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("T,tiles,level", at.RAMP_CASES)
def test_ramp_predictor_and_rescale_mutations(T, tiles, level, fold):
    qkv = at.make_qkv(T, D, H, B, "ramp", fold, ramp=(tiles, level))
    f = at.forward_ref(qkv, T, H, fold)
    fire, ps, exact = at.rescale_plan(f)
    fire, ps, exact = fire[:, :, :T], ps[:, :, :T], exact[:, :, :T]
    nt = (T + 63) // 64
    chosen = torch.zeros(T, dtype=torch.bool)
    chosen[at.ramp_queries(T)] = True
    if level == 1:
        want = torch.zeros(T, nt, dtype=torch.bool)
        want[chosen.nonzero()[:, 0][:, None], torch.tensor(tiles)[None, :]] = True
        assert want.any() and torch.equal(fire, want.expand_as(fire)), "the rescale set is not the designed one"
        assert not exact.any()
        assert (ps[fire] >= 34).all() and (ps[~fire] <= 26).all(), (ps[fire].min().item(), ps[~fire].max().item())
        E_lse, E_out = at.forward_bounds(f, rescales=nt)
        out, lse, n_resc = at.forward_emulate(qkv, T, H, fold)
        assert n_resc >= int(want.sum()) * B * H
        assert _fwd_worst(f, T, out, lse, E_lse, E_out) <= 1.0
        assert _normwise(E_out, f["out"][:, :, :T]) < NORMWISE
        for mut in at.RESCALE_MUTS:
            if mut == "rescale_not_inflight" and max(tiles) == nt - 1 and len(tiles) == 1:
                continue                                        # nothing is in flight behind the last tile
            om, lm, _ = at.forward_emulate(qkv, T, H, fold, mut=mut)
            assert not _fwd_worst(f, T, om, lm, E_lse, E_out) <= 1.0, mut
    else:
        assert torch.equal(exact, chosen.expand_as(exact)), "the exact-walk set is not the designed one"
        E_lse, E_out = at.forward_bounds(f, rescales=nt, exact=True)
        assert _normwise(E_out, f["out"][:, :, :T]) < NORMWISE and torch.isfinite(E_out).all() and torch.isfinite(E_lse).all()


# ------------------------------------------------------------------------------------------------ backward
@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("regime", at.REGIMES)
@pytest.mark.parametrize("T,Dm,Hh,Bb", CASES)
def test_backward_emulation_bounds_and_mutations(T, Dm, Hh, Bb, regime, fold):
    qkv, f = _fwd(T, Dm, Hh, Bb, regime, fold)
    dout = at.make_dout(T, Dm, Bb)
    assert torch.equal(at.bf16_round(dout), dout) and (dout[:, T:] == 0).all()
    out_bf = at.bf16_round(at.join_heads(f["out"]).float())
    lse32 = f["lse"].float()
    r = at.backward_ref(f, dout, out_bf, at.U32 * f["lse"][:, :, :T].abs())
    # the closed form with exact ds and P is fp64 autograd up to the bf16 rounding of the handed output (delta = dO . bf16(out))
    gq, gk, gv = at.backward_autograd(qkv, T, Hh, dout, fold)
    scale = max(gq.abs().max().item(), gk.abs().max().item(), gv.abs().max().item()) + 1e-300
    dO = at.split_heads(dout.double(), Hh)[0][:, :, :T]
    slack = at.UBF * (dO.abs() * f["out"][:, :, :T].abs()).sum(-1).max().item() * max(f["k"].abs().max().item(), f["qe"][:, :, :T].abs().max().item())
    assert (gq - r["dq_plain"]).abs().max().item() <= slack + 1e-12 * scale and (gk - r["dk_plain"]).abs().max().item() <= slack + 1e-12 * scale
    assert (gv - r["dv_plain"]).abs().max().item() <= 1e-12 * scale
    e = at.backward_emulate(qkv, T, Hh, dout, out_bf, lse32, fold)
    keys = ("dq", "dk", "dv")

    def worst(em):
        w = [_ratio((em[k][:, :, :T].double() - r[k]).abs(), r["E_" + k]) for k in keys]
        return max(w + [_ratio((em["delta"][:, :, :T].double() - r["delta"]).abs(), r["E_delta"])])

    assert worst(e) <= 1.0, worst(e)
    assert all((e[k][:, :, T:] == 0).all() for k in ("dk", "dv"))
    if T >= 2:
        assert all(_normwise(r["E_" + k], r[k]) < NORMWISE for k in keys), [_normwise(r["E_" + k], r[k]) for k in keys]
    qkv2 = at.make_qkv(T, Dm, Hh, Bb, regime, fold, pad_seed=1)
    for mut in at.BWD_MUTS:
        meaningful = dict(drop_last_key=T >= 2, admit_pad_key=T < at.tld(T), delta_other_head=T >= 2, dk_sign=T >= 2, dk_scale=T >= 2,
                          pad_dk_kept=T < at.tld(T))[mut]
        if not meaningful:
            continue
        m = at.backward_emulate(qkv, T, Hh, dout, out_bf, lse32, fold, mut=mut)
        if mut == "pad_dk_kept":
            caught = bool((m["dk"][:, :, T:] != 0).any() or (m["dv"][:, :, T:] != 0).any())
        else:
            caught = not worst(m) <= 1.0
            if mut == "admit_pad_key" and not caught:
                m2 = at.backward_emulate(qkv2, T, Hh, dout, out_bf, lse32, fold, mut=mut)
                caught = not all(torch.equal(m2[k][:, :, :T], m[k][:, :, :T]) for k in keys)
        assert caught, mut


@pytest.mark.parametrize("T", at.PROBS_T)
def test_probs_bound_is_small(T):
    _, f = _fwd(T, D, H, B, "partner", False)
    E = at.probs_bounds(f, at.U32 * f["lse"][:, :, :T].abs())
    assert _normwise(E, f["P"][:, :, :T]) < 1e-3
