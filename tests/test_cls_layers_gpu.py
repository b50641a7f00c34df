"""GPU: the [CLS] appearance loss over several ViT blocks (``dino_cls_layers`` / ``dino_cls_layer_weights``).
Op level: the layered launch on caller buffers (splice_cls_loss_layers) -- every layer against its own single-layer launch bit for bit,
against float64 under bounds from the standard rounding model, guard bands, refusals.  ViT level: a backward seeded through
splice_vit_ctx_set_cls_seeds against the same gradient handed over in full d_block buffers.  Step level: per-layer values and the reported
word, the generator gradient against the oracle's autograd through the same plan, and bit-identity where the step promises it."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dino_vit
from oracle import losses as olosses
from splice_amd import _lib, synth
from splice_amd.engine import DEFAULT_CFG, MultiPairEngine, SpliceEngine, np_cls_layers, np_plateau, stop_window_closes
from splice_amd.generator import GeneratorPlan

pytestmark = pytest.mark.gpu
DEV = "cuda"
f32 = np.float32
U = 2.0 ** -24             # unit roundoff of float32
NAN_BITS = 0x7FC0DEAD      # a quiet NaN with a payload: what the kernel must leave alone
PART_FILL = -123.0         # prefill of partial slots and values
GUARD = 64                 # elements of guard band on either side of every output buffer
LAYERS, WEIGHTS = "dino_cls_layers", "dino_cls_layer_weights"
S_LAYERS, S_WEIGHTS = "dino_ssim_layers", "dino_ssim_layer_weights"


def _st():
    return _lib.current_stream()


def _at(t, elems=0):
    return C.c_void_p(t.data_ptr() + elems * t.element_size())


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ op level
OP_LAM = float(f32(0.37))
OP_WEIGHTS = (0.3, 1.7, 1.0)
X_ROWS, T_ROWS = 96, 80    # the slot stride on the generated side is 96 * D floats (a pass of Tld = 96 rows), another on the target side
SEED_GAP, PART_PS = 5, 7   # the seed rows of consecutive slots are D + 5 floats apart; a slot's partial row has 7 slots


@functools.lru_cache(maxsize=None)
def _op_case(D, layer, slots=2):
    """the operands of `layer`: fp32 [slots][rows][D] on both sides, rows 1.. hold a sentinel; the target near the generated row (the
    cancellation the step lives in) for layers >= 1, independent of it for layer 0; no difference is exactly zero; never modified"""
    g = torch.Generator().manual_seed(100 * layer + D)
    x = torch.full((slots, X_ROWS, D), 1e3)
    t = torch.full((slots, T_ROWS, D), -7e5)
    x[:, 0] = torch.randn(slots, D, generator=g)
    t[:, 0] = torch.randn(slots, D, generator=g) if layer == 0 else x[:, 0] + 0.05 * torch.randn(slots, D, generator=g)
    assert ((x[:, 0] - t[:, 0]) != 0).all()
    return x.to(DEV), t.to(DEV)


def _run_cls(D, layers, weights, slots=2, gtab=None, n_arg=None, break_ptr=False, seed_gap=SEED_GAP):
    """One splice_cls_loss_layers call on the operands of `layers`.  Returns (rc, values [slots][n] bits, partials [slots][PART_PS] bits,
    seeds: list of [slots][D + gap] bit patterns, guards_intact)."""
    L, n = _lib.lib(), len(layers)
    ops = [_op_case(D, l, slots) for l in layers]
    sps = D + seed_gap
    vals = torch.full((GUARD + slots * n + GUARD,), PART_FILL, device=DEV)
    part = torch.full((GUARD + slots * PART_PS + GUARD,), PART_FILL, device=DEV)
    seeds = [torch.full((GUARD + slots * max(sps, D) + GUARD,), NAN_BITS, dtype=torch.int32, device=DEV).view(torch.float32) for _ in layers]
    arr = lambda ptrs: (C.c_void_p * n)(*[p.value for p in ptrs])
    xs = [_at(o[0]) for o in ops]
    if break_ptr:
        xs[-1] = C.c_void_p(0)
    tab = None if gtab is None else torch.tensor(gtab, dtype=torch.float32, device=DEV)
    rc = L.splice_cls_loss_layers(n if n_arg is None else n_arg, arr(xs), arr([_at(o[1]) for o in ops]), (C.c_float * n)(*weights), X_ROWS * D, T_ROWS * D, D, slots,
                                  OP_LAM, None if tab is None else _lib.ptr(tab), _at(part, GUARD), PART_PS, arr([_at(s, GUARD) for s in seeds]), sps, _at(vals, GUARD), _st())
    torch.cuda.synchronize()
    guards = bool((vals[:GUARD] == PART_FILL).all() and (vals[-GUARD:] == PART_FILL).all() and (part[:GUARD] == PART_FILL).all() and (part[-GUARD:] == PART_FILL).all())
    for s in seeds:
        b = _bits(s)
        guards = guards and bool((b[:GUARD] == NAN_BITS).all() and (b[-GUARD:] == NAN_BITS).all())
    return (rc, _bits(vals[GUARD:-GUARD]).view(slots, n).cpu(), _bits(part[GUARD:-GUARD]).view(slots, PART_PS).cpu(),
            [_bits(s)[GUARD:-GUARD].view(slots, -1).cpu() for s in seeds], guards)


def _as_f32(bits):
    return bits.contiguous().view(torch.float32)


PART_FILL_BITS = int(np.array(PART_FILL, dtype=f32).view(np.int32))
OP_CASES = [(D, n) for D in (384, 768) for n in (1, 2, 3)]


@pytest.mark.parametrize("D,n", OP_CASES)
def test_layer_of_a_batched_launch_equals_its_own_launch(D, n):
    """Layer i of the batched launch -- its column of the values buffer and its own seed buffer -- has the bits of its own L = 1 launch with
    the same weight; partial slot 0 is the float32 ascending sum of the slot's values, exactly; the other partial slots, the gaps between
    the seed rows and the guard bands keep their prefill."""
    layers, weights = list(range(n)), OP_WEIGHTS[:n]
    rc, vals, part, seeds, guards = _run_cls(D, layers, weights)
    assert rc == 0 and guards
    assert (part[:, 1:] == PART_FILL_BITS).all(), "partial slots other than 0 were written"
    for s in range(2):
        assert _as_f32(part)[s, 0].numpy().tobytes() == np_cls_layers(_as_f32(vals)[s].numpy()).tobytes(), s
    for i, l in enumerate(layers):
        assert (seeds[i][:, D:] == NAN_BITS).all(), "the gap behind a seed row was written"
        rc1, vals1, part1, seeds1, guards1 = _run_cls(D, [l], [weights[i]])
        assert rc1 == 0 and guards1
        assert torch.equal(vals[:, i], vals1[:, 0]) and torch.equal(seeds[i], seeds1[0]), i
        assert torch.equal(part1[:, 0], _bits(_as_f32(vals1)[:, 0] + 0.0)), i   # one layer: the partial is its value (0 + v)


@pytest.mark.parametrize("D,n", OP_CASES)
def test_layers_against_fp64(D, n):
    """On the same fp32 inputs.  A value is a sum of D non-negative addends, each with three roundings (d, its square, its addition --
    fewer where the compiler contracts), times one rounded factor w / D, and one more product: relative error <= (D + 4) 2^-24 in the
    standard model.  A seed element 2 (g w) d has one rounding in d, two in the products and those of g = lambda / D: <= 8 2^-24."""
    layers, weights = list(range(n)), OP_WEIGHTS[:n]
    rc, vals, part, seeds, guards = _run_cls(D, layers, weights)
    assert rc == 0 and guards
    worst_v = worst_s = 0.0
    for i, l in enumerate(layers):
        x, t = (o[:, 0].cpu().double() for o in _op_case(D, l))
        d = x - t
        w = float(f32(weights[i]))
        want_v = (d * d).sum(1) * (w / D)
        want_s = 2.0 * (OP_LAM / D) * w * d
        rel_v = ((_as_f32(vals)[:, i].double() - want_v).abs() / want_v).max().item()
        rel_s = ((_as_f32(seeds[i])[:, :D].double() - want_s).abs() / want_s.abs()).max().item()
        worst_v, worst_s = max(worst_v, rel_v / ((D + 4) * U)), max(worst_s, rel_s / (8 * U))
        assert rel_v <= (D + 4) * U, (i, rel_v)
        assert rel_s <= 8 * U, (i, rel_s)
    print(f"CLS_LAYERS op D={D} n={n}: value worst err/bound {worst_v:.4f}, seed worst err/bound {worst_s:.4f}")


def test_a_slot_whose_table_entry_is_zero_takes_no_part():
    """the per-slot gradient weight (a sweep's PW_CLS row): slot 0 with its own weight, slot 1 with 0 -- nothing of slot 1 is written"""
    D, n = 384, 2
    g0 = float(f32(0.011))
    rc, vals, part, seeds, guards = _run_cls(D, [0, 1], OP_WEIGHTS[:n], gtab=[g0, 0.0])
    assert rc == 0 and guards
    assert (vals[1] == PART_FILL_BITS).all() and (part[1] == PART_FILL_BITS).all() and all((s[1] == NAN_BITS).all() for s in seeds)
    rc, vals_s, part_s, seeds_s, _ = _run_cls(D, [0, 1], OP_WEIGHTS[:n])
    assert torch.equal(vals[0], vals_s[0]) and torch.equal(part[0], part_s[0])   # (the value does not depend on the gradient weight)
    for i in range(n):
        x, t = (o[0, 0].cpu().double() for o in _op_case(D, i))
        want = 2.0 * g0 * float(f32(OP_WEIGHTS[i])) * (x - t)
        assert ((_as_f32(seeds[i])[0, :D].double() - want).abs() / want.abs()).max().item() <= 8 * U


def test_op_refusals_launch_nothing():
    D = 384
    for kw in (dict(layers=[0, 1], weights=[1.0, 0.0]), dict(layers=[0, 1], weights=[float("nan"), 1.0]), dict(layers=[0, 1], weights=[1.0, float("inf")]),
               dict(layers=[0, 1], weights=[1.0, -1.0]), dict(layers=[0, 1], weights=[1.0, 1.0], break_ptr=True), dict(layers=[0, 1], weights=[1.0, 1.0], n_arg=0),
               dict(layers=[0, 1], weights=[1.0, 1.0], n_arg=13), dict(layers=[0, 1], weights=[1.0, 1.0], seed_gap=-1)):   # (seed rows that would overlap)
        rc, vals, part, seeds, guards = _run_cls(D, **kw)
        assert rc != 0 and guards, kw
        assert (vals == PART_FILL_BITS).all() and (part == PART_FILL_BITS).all() and all((s == NAN_BITS).all() for s in seeds), kw
    L = _lib.lib()
    assert L.splice_cls_loss_layers(1, None, None, None, 96 * D, 96 * D, D, 2, OP_LAM, None, None, 8, None, D, None, _st()) != 0


# ------------------------------------------------------------------------------------------------ ViT level
@pytest.fixture(scope="module")
def vit_state():
    return synth.vit_params(7, "dino_vits8", img_size=64, w_std=0.05)


@pytest.fixture(scope="module")
def vit(vit_state):
    from splice_amd.vit import VitEngine
    return VitEngine("dino_vits8", device=DEV).load_state_dict(vit_state)


def _arm(ctx, seeds, p0, p1):
    """seeds: dict layer -> [B][D] fp32 tensor, or None to disarm"""
    if seeds is None:
        return _lib.lib().splice_vit_ctx_set_cls_seeds(ctx.handle, None, 0, 0)
    a = (C.c_void_p * ctx.engine.depth)()
    for l, t in seeds.items():
        a[l] = t.data_ptr()
    return _lib.lib().splice_vit_ctx_set_cls_seeds(ctx.handle, a, p0, p1)


def _full(ctx, seed, p0=0, p1=None):
    """the [B][Tld][D] d_block buffer that is zero outside row 0 of the passes [p0, p1), where it holds the seed rows"""
    d = torch.zeros(ctx.B, ctx.Tld, ctx.engine.dim, device=DEV)
    d[p0:p1, 0] = seed[p0:p1]
    return d


@pytest.mark.parametrize("top_cls_only", [False, True], ids=["full-top", "cls-only-top"])
def test_seeded_backward_equals_the_same_gradient_in_full_buffers(vit, top_cls_only):
    """dino_vits8, 64 x 64, T = 65, three passes, seeds at blocks {2, 7}: d_img element for element as numbers (==).  Once with the top
    block's key gradient live in front of them (cls-only-top: also a [CLS] row at the top block through d_block, the step's layout), once
    with the seeds as the only gradient (the stream starts at block 7), once armed for a part of the range; and a range the armed one does
    not meet has the bits of a context without the call."""
    from splice_amd.vit import VitContext
    L = _lib.lib()
    B, D = 3, vit.dim
    g = torch.Generator().manual_seed(11)
    img = torch.rand(B, 3, 64, 64, generator=g).to(DEV)
    seeded, plain = VitContext(vit, B, 64, 64, True), VitContext(vit, B, 64, 64, True)
    for c in (seeded, plain):
        _lib.check(L.splice_vit_ctx_set_top_cls_only(c.handle, int(top_cls_only)), "top_cls_only")
        c.forward(img, True)
    assert (seeded.T, seeded.B) == (65, 3)
    seeds = {l: (1e-3 * torch.randn(B, D, generator=g)).to(DEV) for l in (2, 7)}
    dk = torch.zeros(B, seeded.Tld, D)
    dk[:, :seeded.T] = 1e-3 * torch.randn(B, seeded.T, D, generator=g)
    dk = {11: dk.to(DEV)}
    top = {11: _full(plain, (1e-3 * torch.randn(B, D, generator=g)).to(DEV))} if top_cls_only else {}

    def same(a, b):
        return bool((a == b).all()) and bool(torch.isfinite(a).all()) and bool(a.abs().max() > 0)
    # (a) the key gradient of the top block live in front of the seeds
    want = plain.backward(0, B, d_block={**top, **{l: _full(plain, s) for l, s in seeds.items()}}, d_keys=dk, normalize=True)
    assert _arm(seeded, seeds, 0, B) == 0
    got = seeded.backward(0, B, d_block=top or None, d_keys=dk, normalize=True)
    assert same(got, want)
    # (b) the seeds as the only gradient
    want = plain.backward(0, B, d_block={l: _full(plain, s) for l, s in seeds.items()}, normalize=True)
    got = seeded.backward(0, B, normalize=True)
    assert same(got, want)
    # (c) armed for pass 1 alone, backward over all three: with a live stream, and as the only gradient
    assert _arm(seeded, seeds, 1, 2) == 0
    want = plain.backward(0, B, d_block={l: _full(plain, s, 1, 2) for l, s in seeds.items()}, d_keys=dk, normalize=True)
    assert same(seeded.backward(0, B, d_keys=dk, normalize=True), want)
    want = plain.backward(0, B, d_block={l: _full(plain, s, 1, 2) for l, s in seeds.items()}, normalize=True)
    got = seeded.backward(0, B, normalize=True)
    assert same(got, want) and not got[0].any() and not got[2].any()
    # (d) a range the armed one does not meet: the bits of a context without the call
    assert _arm(seeded, seeds, 0, 1) == 0
    want = plain.backward(1, B, d_keys=dk, normalize=True)
    got = seeded.backward(1, B, d_keys=dk, normalize=True)
    assert torch.equal(_bits(got), _bits(want)) and bool(got.abs().max() > 0)
    # disarmed: likewise over the whole range
    assert _arm(seeded, None, 0, 0) == 0
    assert torch.equal(_bits(seeded.backward(0, B, d_keys=dk, normalize=True)), _bits(plain.backward(0, B, d_keys=dk, normalize=True)))
    # refusals
    assert _arm(seeded, seeds, 2, B + 1) != 0 and _arm(seeded, seeds, -1, 2) != 0 and _arm(seeded, seeds, 2, 1) != 0
    nograd = VitContext(vit, B, 64, 64, False)
    assert _arm(nograd, seeds, 0, B) != 0 and b"need_grad" in L.splice_last_error()


# ------------------------------------------------------------------------------------------------ step level
GEN_SEED = 41


def _cfg(**over):
    return dict(DEFAULT_CFG, dino_model_name="dino_vits8", dino_global_patch_size=64, **over)


def _pair(seed=40, pair=2):   # (the pair and generator of tests/test_step_gpu.py::test_step_gradients_vs_oracle_teacher_forced)
    A, B = synth.smooth_image_pair(seed, pair, 64, 64)
    return torch.from_numpy(A).to(DEV), torch.from_numpy(B).to(DEV)


def _engine(vit, entire=True, **over):
    return SpliceEngine(_cfg(**over), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64) if entire else None, vit_engine=vit)


@pytest.fixture(scope="module")
def oracle_vit(vit_state):
    m = dino_vit.VisionTransformer(8, 384, 12, 6, img_size=64).eval()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in vit_state.items()})
    for p in m.parameters():
        p.requires_grad_(False)
    return m


def _cls_rows(m, img):
    """row 0 of every block's output for the image [3][64][64] (fp32, CPU), before the final LayerNorm: prepare_tokens, then the blocks"""
    x = m.prepare_tokens(olosses.normalize(img).unsqueeze(0))
    rows = []
    for blk in m.blocks:
        x = blk(x)
        rows.append(x[0, 0, :])
    return rows


def _oracle_terms(m, x, b, layers, weights):
    """[w_l * mse(cls_l(x), cls_l(b))] over the layers, the target side without gradient"""
    with torch.no_grad():
        want = _cls_rows(m, b)
    got = _cls_rows(m, x)
    return [float(w) * F.mse_loss(got[l], want[l]) for l, w in zip(layers, weights)]


SETS = {"5": ([5], None), "0-11": ([0, 11], [0.5, 2.0]), "2-7-11": ([2, 7, 11], [1.5, 0.25, 1.0])}


def _keys(name):
    layers, weights = SETS[name]
    return {LAYERS: layers} if weights is None else {LAYERS: layers, WEIGHTS: weights}


@pytest.mark.parametrize("name", sorted(SETS))
def test_step_reports_the_layers_and_their_ordered_sum(vit, oracle_vit, name):
    """Step 0 (entire-image: word 3, and word 4 beside it) and step 1 (ordinary: word 4) with lr 0.  Every per-layer value against the
    oracle's block outputs on the plan's own forward output, within the 1e-2 the teacher-forced test of tests/test_step_gpu.py holds every
    reported loss to; the reported word is the float32 sum of the per-layer values in ascending order, exactly."""
    layers, weights = SETS[name]
    weights = weights or [1.0] * len(layers)
    A, B = _pair()
    eng = _engine(vit, lr=0.0, **_keys(name))
    assert eng.cls_layers == (layers, weights)
    p0 = eng.params.clone()
    x = GeneratorPlan(eng.gen, 1, 64, 64, True, 0).forward(eng.params, A[None])[0].cpu()
    want = [t.item() for t in _oracle_terms(oracle_vit, x, B.cpu(), layers, weights)]
    for step, words in enumerate((((3, True), (4, False)), ((4, False),))):
        eng.step(A, B, A)
        row = eng.losses_dev[0].cpu().numpy()
        for word, entire in words:
            vals = eng.cls_layer_values(entire=entire)
            assert vals.dtype == np.float32 and vals.shape == (len(layers),)
            for l, v, w in zip(layers, vals, want):
                print(f"CLS_LAYERS step {step} word {word} set {name} layer {l}: w * mse {v:.7g}, oracle {w:.7g}, rel {abs(v - w) / w:.2e}")
                assert abs(v - w) / w < 1e-2, (step, word, l, v, w)
            assert row[word].tobytes() == np_cls_layers(vals).tobytes(), (step, word, row[word], vals)
            assert eng.losses()["loss_entire_cls" if entire else "loss_global_cls"] == float(row[word])
        if step == 1:
            assert row[3] == 0   # the entire-image term did not run at this step
    assert torch.equal(eng.params, p0)


def test_step_word_over_two_crops(vit, oracle_vit):
    """n_crops = 2: the word is the sum over the pair's crops of the layered term, against the oracle on the plan's own output"""
    layers, weights = SETS["2-7-11"]
    A, B = _pair()
    A2 = torch.stack([A, A.flip(-1)]).contiguous()
    B2 = torch.stack([B, B.flip(-2)]).contiguous()
    eng = SpliceEngine(_cfg(lr=0.0, **_keys("2-7-11")), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit, n_crops=2)
    x = GeneratorPlan(eng.gen, 2, 64, 64, True, 0, batch_stats=True).forward(eng.params, A2).cpu()
    per_crop = [[t.item() for t in _oracle_terms(oracle_vit, x[i], B2[i].cpu(), layers, weights)] for i in range(2)]
    want = sum(sum(c) for c in per_crop)
    eng.step(A2, B2)
    got = float(eng.losses_dev[0, 4].item())
    vals = eng.cls_layer_values()
    print(f"CLS_LAYERS two crops: word {got:.7g}, oracle {want:.7g}, rel {abs(got - want) / want:.2e}")
    assert abs(got - want) / want < 1e-2
    for i, v in enumerate(vals):   # per layer, the pair's crops added in crop order
        w = per_crop[0][i] + per_crop[1][i]
        assert abs(v - w) / w < 1e-2, (i, v, w)


@pytest.fixture(scope="module")
def grad_errs(vit, oracle_vit):
    """per layer set (None: the keys absent, what the parent commit computes too): whole-arena relative L2 of the step's generator
    gradient against plan.backward of the oracle's autograd image gradient on the plan's own forward output, only the appearance term on"""
    cache = {}

    def get(name):
        if name not in cache:
            A, B = _pair()
            only = dict(lambda_global_ssim=0.0, lambda_global_identity=0.0, lambda_entire_cls=0.0, lambda_entire_ssim=0.0, cls_warmup=0, lr=0.0)
            eng = _engine(vit, entire=False, **only, **({} if name is None else _keys(name)))
            layers, weights = ([11], [1.0]) if name is None else (SETS[name][0], SETS[name][1] or [1.0] * len(SETS[name][0]))
            p0 = eng.params.clone()
            eng.step(A, B)
            assert torch.equal(eng.params, p0)
            plan = GeneratorPlan(eng.gen, 1, 64, 64, True, 0)
            x = plan.forward(eng.params, A[None])[0].cpu().clone().requires_grad_(True)
            loss = sum(_oracle_terms(oracle_vit, x, B.cpu(), layers, weights)) * eng.cfg["lambda_global_cls"]
            dx, = torch.autograd.grad(loss, x)
            g_ref = plan.backward(eng.params, dx[None].to(DEV).contiguous())
            num = den = 0.0
            for (pname, g), r in zip(eng.gen.unflatten(eng.grads).items(), eng.gen.unflatten(g_ref).values()):
                if pname.endswith("0.bias") and pname != "9.0.bias":
                    continue   # zero-gradient conv biases (feed a BatchNorm)
                num += (g.double() - r.double()).pow(2).sum().item()
                den += r.double().pow(2).sum().item()
            cache[name] = ((num / den) ** 0.5, abs(eng.losses_dev[0, 0].item() - loss.item()) / loss.item())
        return cache[name]
    return get


TEACHER_FORCED_BAR = 3e-2   # tests/test_step_gpu.py::test_step_gradients_vs_oracle_teacher_forced


@pytest.mark.parametrize("name", sorted(SETS))
def test_step_gradient_against_the_oracle_through_the_same_plan(grad_errs, name):
    """The yardstick is the identical comparison at the default layer, which needs nothing of this feature; a layer set is held to the
    larger of three times that figure and the teacher-forced bar (DESIGN.md section 9l has the measured table)."""
    yard, yard_loss = grad_errs(None)
    err, loss_err = grad_errs(name)
    bar = max(3 * yard, TEACHER_FORCED_BAR)
    print(f"CLS_LAYERS gradient set {name}: rel L2 {err:.3e} (total rel {loss_err:.2e}); default layer {yard:.3e} (total rel {yard_loss:.2e}); bar {bar:.3e}")
    assert err <= bar and loss_err < 1e-2 and yard_loss < 1e-2


def _arenas(eng, pair=0):
    n, st = eng.gen.numel, eng.stride
    sl = slice(pair * st, pair * st + n)
    return dict(params=eng.params[sl].clone(), m=eng.m[sl].clone(), v=eng.v[sl].clone(), running=eng.running[pair].clone(), losses=eng.losses_dev[pair].clone())


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a)


@pytest.mark.parametrize("keys", [{LAYERS: [11]}, {LAYERS: [11], WEIGHTS: [1.0]}, {LAYERS: None, WEIGHTS: None}], ids=["top", "top-w1", "null"])
def test_default_layer_is_the_engine_without_the_keys(vit, keys):
    """6 steps over the regimes -- [CLS] warm-up (steps 0-1), entire-image steps (0, 4), an unequal crop (step 3) --: the default spelled
    out launches what a config without the keys launches, the same bytes everywhere"""
    A, B = _pair()
    A2 = A[:, :60, :60].contiguous()
    cfg = {k: v for k, v in _cfg(cls_warmup=2, entire_A_every=4).items() if k not in (LAYERS, WEIGHTS)}
    twin = SpliceEngine(cfg, None, synth.generator_params(GEN_SEED, 0.02), (64, 64), (64, 64), vit_engine=vit)
    eng = _engine(vit, cls_warmup=2, entire_A_every=4, **keys)
    assert eng.cls_layers is None
    for i in range(6):
        for e in (eng, twin):
            e.step(A2 if i == 3 else A, B, A)
        assert torch.equal(_bits(eng.losses_dev), _bits(twin.losses_dev)) and torch.equal(_bits(eng.grads), _bits(twin.grads)), i
    assert _same(_arenas(eng), _arenas(twin))
    with pytest.raises(RuntimeError, match="dino_cls_layers"):
        eng.cls_layer_values()


def test_batch_independence_two_pairs(vit):
    """default lr, 3 steps, layers [3, 11]: each pair of a two-pair engine is, bit for bit, its own SpliceEngine run, values included"""
    keys = {LAYERS: [3, 11], WEIGHTS: [0.75, 1.25]}
    pairs = [_pair(40, 2), _pair(62, 0)]
    gens = [synth.generator_params(41, 0.02), synth.generator_params(61, 0.02)]
    multi = MultiPairEngine(_cfg(**keys), None, gens, (64, 64), (64, 64), vit_engine=vit)
    A2, B2 = torch.stack([p[0] for p in pairs]).contiguous(), torch.stack([p[1] for p in pairs]).contiguous()
    rows, vals, evals = [], [], []
    for _ in range(3):
        multi.step(A2, B2, A2)
        rows.append(multi.losses_dev.clone())
        vals.append(multi.cls_layer_values())
        evals.append(multi.cls_layer_values(entire=True))
    for p in range(2):
        single = SpliceEngine(_cfg(**keys), None, gens[p], (64, 64), (64, 64), vit_engine=vit)
        for k in range(3):
            single.step(pairs[p][0], pairs[p][1], pairs[p][0])
            assert torch.equal(_bits(single.losses_dev[0]), _bits(rows[k][p])), (p, k)
            assert single.cls_layer_values().tobytes() == vals[k][p].tobytes(), (p, k)
            assert single.cls_layer_values(entire=True).tobytes() == evals[k][p].tobytes(), (p, k)
        assert multi.cls_layer_values(p).tobytes() == vals[2][p].tobytes()
        assert _same(_arenas(multi, p), _arenas(single)), p
        assert rows[2][p][4] > 0 and vals[2][p].all() and evals[2][p].all()


def test_graph_replay_equals_eager(vit):
    """Four steps on fixed crops with lr 0: step 1 is launched eagerly, step 2 captures the graph, step 3 replays it; then an engine that
    never captures.  Gradient arena, first moment and losses row agree bit for bit."""
    A, B = _pair()
    keys = _keys("2-7-11")
    eng = _engine(vit, lr=0.0, **keys)
    seen = []
    for _ in range(4):
        eng.step(A, B, A)
        seen.append((eng.grads.clone(), eng.m.clone(), eng.losses_dev.clone()))
    stats = (C.c_longlong * 3)()
    _lib.check(_lib.lib().splice_step_graph_stats(eng.handle, stats), "graph_stats")
    assert stats[0] + stats[2] >= 1                                     # a graph was in use
    for k in (2, 3):
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(seen[k], seen[1])), k
    vals = eng.cls_layer_values()
    eager = _engine(vit, lr=0.0, **keys)
    _lib.check(_lib.lib().splice_step_use_graph(eager.handle, 0), "use_graph")
    for _ in range(4):
        eager.step(A, B, A)
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip((eager.grads, eager.m, eager.losses_dev), seen[3]))
    assert eager.cls_layer_values().tobytes() == vals.tobytes() and vals.all()
    # another layer set behind it in the same process: its own graphs, its own numbers (the pool's salt carries the set)
    other = _engine(vit, lr=0.0, **_keys("0-11"))
    other_eager = _engine(vit, lr=0.0, **_keys("0-11"))
    _lib.check(_lib.lib().splice_step_use_graph(other_eager.handle, 0), "use_graph")
    for _ in range(4):
        other.step(A, B, A)
        other_eager.step(A, B, A)
    assert torch.equal(_bits(other.grads), _bits(other_eager.grads)) and torch.equal(_bits(other.losses_dev), _bits(other_eager.losses_dev))
    assert not torch.equal(_bits(other.losses_dev), _bits(seen[3][2]))


def test_sweep_with_shared_layers_equals_an_engine_per_slot(vit):
    """per-slot lambda_global_cls (the PW_CLS table, one factor more per layer), one of them 0 (that slot takes no part in the launch and
    its seed rows are never written), shared layers: slot p is its SpliceEngine, bit for bit"""
    A, B = _pair()
    keys = {LAYERS: [3, 11], WEIGHTS: [0.5, 2.0]}
    variants = [dict(lambda_global_cls=0.5), dict(lambda_global_cls=0.0), dict(lambda_global_cls=2.0)]
    gen = synth.generator_params(GEN_SEED, 0.02)
    sweep = MultiPairEngine(_cfg(cls_warmup=1, **keys), None, [gen] * 3, (64, 64), (64, 64), vit_engine=vit, pair_cfgs=variants)
    A3, B3 = torch.stack([A] * 3).contiguous(), torch.stack([B] * 3).contiguous()
    rows = []
    for _ in range(3):
        sweep.step(A3, B3, A3)
        rows.append(sweep.losses_dev.clone())
    assert not sweep.cls_layer_values(1).any() and sweep.cls_layer_values(0).all()
    for p, over in enumerate(variants):
        single = _engine(vit, cls_warmup=1, **keys, **over)
        for k in range(3):
            single.step(A, B, A)
            assert torch.equal(_bits(single.losses_dev[0]), _bits(rows[k][p])), (p, k)
        assert _same(_arenas(sweep, p), _arenas(single)), p
    assert not torch.equal(_bits(rows[2][0]), _bits(rows[2][2])) and rows[2][1][4] == 0


def test_both_layer_keys_together(vit):
    """dino_ssim_layers on as well: each accessor returns the bits of the engine that carries only its own key (lr 0; step 0 is an
    entire-image step, step 1 an ordinary one behind cls_warmup)"""
    A, B = _pair()
    ck, sk = _keys("2-7-11"), {S_LAYERS: [2, 7, 11]}
    both, only_c, only_s = (_engine(vit, lr=0.0, cls_warmup=1, **k) for k in ({**ck, **sk}, ck, sk))
    for step in range(2):
        for e in (both, only_c, only_s):
            e.step(A, B, A)
        for entire in ((True, False) if step == 0 else (False,)):
            assert both.cls_layer_values(entire=entire).tobytes() == only_c.cls_layer_values(entire=entire).tobytes() and both.cls_layer_values(entire=entire).all()
            assert both.ssim_layer_values(entire=entire).tobytes() == only_s.ssim_layer_values(entire=entire).tobytes()
        row = both.losses_dev[0].cpu().numpy()
        assert row[4].tobytes() == only_c.losses_dev[0, 4].cpu().numpy().tobytes() and row[1].tobytes() == only_s.losses_dev[0, 1].cpu().numpy().tobytes()
    assert both.ssim_layer_values().all()


def test_stop_rule_sees_the_layered_total(vit):
    """stop_window 2: the stop record's window sums are those of the NumPy rule fed the reported totals"""
    A, B = _pair()
    rule = dict(stop_window=2, stop_rel=0.01, stop_patience=50, stop_min_steps=0)
    eng = _engine(vit, cls_warmup=1, entire_A_every=4, **_keys("2-7-11"), **rule)
    off = _engine(vit, cls_warmup=1, entire_A_every=4, **rule)
    totals = []
    for _ in range(8):
        eng.step(A, B, A)
        off.step(A, B, A)
        totals.append(eng.losses_dev[0, 0].item())
    counted = [stop_window_closes(k, 1, 1, 4) for k in range(8)]
    want = np_plateau(np.array(totals, dtype=f32), counted, 2, 0.01, 50, 0)
    s, count, windows, best, bad, stop_step = eng._stop_records()[0]
    assert (count, windows, bad, stop_step) == (want["count"], want["windows"], want["bad"], want["stop_step"]) and windows == 3
    assert f32(s).tobytes() == want["sum"].tobytes() and f32(best).tobytes() == want["best"].tobytes()
    assert f32(best) != f32(off._stop_records()[0][3])


def test_snapshot_is_refused_under_another_layer_set(vit):
    A, B = _pair()
    eng = _engine(vit, **_keys("2-7-11"))
    eng.step(A, B, A)
    state = eng.snapshot(0)
    with pytest.raises(ValueError, match="dino_cls_layer"):   # (either key: the comparison names the first that differs)
        _engine(vit).restore([state])
    with pytest.raises(ValueError, match="'" + LAYERS + "'"):
        _engine(vit, **{LAYERS: [3, 7, 11], WEIGHTS: [1.5, 0.25, 1.0]}).restore([state])
    with pytest.raises(ValueError, match="'" + WEIGHTS + "'"):
        _engine(vit, **{LAYERS: [2, 7, 11], WEIGHTS: [1.5, 0.25, 2.0]}).restore([state])
    same = _engine(vit, **{LAYERS: [11, 7, 2], WEIGHTS: [1.0, 0.25, 1.5]})   # (the same set in another order: one canonical form)
    same.restore([state])
    eng.step(A, B, A)
    same.step(A, B, A)
    assert torch.equal(_bits(same.params), _bits(eng.params)) and torch.equal(_bits(same.losses_dev), _bits(eng.losses_dev))


def test_setter_refusals(vit, vit_state):
    L = _lib.lib()
    A, B = _pair()
    two, w2 = (C.c_int * 2)(3, 11), (C.c_float * 2)(1.0, 1.0)
    eng = _engine(vit)
    for layers, weights, word in (((C.c_int * 2)(11, 3), w2, b"ascending"), ((C.c_int * 2)(3, 3), w2, b"ascending"), ((C.c_int * 2)(3, 12), w2, b"ascending"),
                                  (two, (C.c_float * 2)(1.0, 0.0), b"finite"), (two, (C.c_float * 2)(float("nan"), 1.0), b"finite")):
        assert L.splice_step_set_cls_layers(eng.handle, 2, layers, weights) != 0 and word in L.splice_last_error()
    for n in (0, 13):
        assert L.splice_step_set_cls_layers(eng.handle, n, two, w2) != 0 and b"needs 1..12 layers" in L.splice_last_error()
    out = (C.c_float * 8)()
    assert L.splice_step_cls_layer_values(eng.handle, 0, out, 8) != 0 and b"no [CLS] layers" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 1, 0) == 0
    assert L.splice_step_set_cls_layers(eng.handle, 2, two, w2) != 0 and b"gradient-only" in L.splice_last_error()
    assert L.splice_step_set_mode(eng.handle, 0, 0) == 0
    lead = _engine(vit)
    assert L.splice_step_set_phases(eng.handle, 2, lead.handle) == 0
    assert L.splice_step_set_cls_layers(eng.handle, 2, two, w2) != 0 and b"phase mode" in L.splice_last_error()
    assert L.splice_step_set_phases(eng.handle, 7, None) == 0
    eng.step(A, B, A)
    assert L.splice_step_set_cls_layers(eng.handle, 2, two, w2) != 0 and b"before the first step" in L.splice_last_error()
    on = _engine(vit, **{LAYERS: [3, 11]})
    assert L.splice_step_set_cls_layers(on.handle, 2, two, w2) != 0 and b"once" in L.splice_last_error()
    assert L.splice_step_set_mode(on.handle, 1, 0) != 0 and b"[CLS] layers" in L.splice_last_error()
    assert L.splice_step_set_phases(on.handle, 2, lead.handle) != 0 and b"[CLS] layers" in L.splice_last_error()
    assert L.splice_step_cls_layer_values(on.handle, 0, out, 1) != 0 and b"holds" in L.splice_last_error()      # two floats needed
    no_entire = _engine(vit, entire=False, **{LAYERS: [3, 11]})
    assert L.splice_step_cls_layer_values(no_entire.handle, 1, out, 8) != 0 and b"entire-image" in L.splice_last_error()
    # fp8: the C setter refuses what the Python engine refuses on the host (an engine of its own: the e4m3 weights stay with it)
    from splice_amd.vit import VitEngine
    vit8 = VitEngine("dino_vits8", device=DEV).load_state_dict(vit_state)
    e8 = SpliceEngine(_cfg(), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit8, fp8=True)
    assert L.splice_step_set_cls_layers(e8.handle, 2, two, w2) != 0 and b"fp8" in L.splice_last_error()
    with pytest.raises(ValueError, match="fp8"):
        SpliceEngine(_cfg(**{LAYERS: [3, 11]}), None, synth.generator_params(GEN_SEED, 0.02), (64, 64), None, vit_engine=vit8, fp8=True)
