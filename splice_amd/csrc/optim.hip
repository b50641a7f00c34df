// Fused multi-tensor optimiser update over the flat parameter arena (K19): torch.optim.Adam / RMSprop / SGD as util/util.py:28-39
// configures them, plus optimizer.zero_grad (train.py:56) when zero_grad != 0.  One walk over the arena (optim_kernel), one element
// rule per optimiser, one launcher that validates and selects the instance.  Beside the three plain rules, torch.optim's further
// arguments (weight decay, momentum / dampening / nesterov, amsgrad, centred RMSprop, AdamW) as extended rules of the same walk.
#include "optim.h"
#include "plateau.h"

// ---- element rules.  Contraction is OFF so that the vector body and the scalar tail of the kernel round alike (an element's result
// must not depend on where in an arena it sits: P pairs per step == P single runs, bit for bit).  USES_M / USES_V: the moment arenas
// the rule reads and writes; the walk does not touch (or alignment-test) the others.
// Adam: no weight decay / amsgrad, eps added after sqrt(v_hat)
struct AdamRule {
    static constexpr bool USES_M = true, USES_V = true, USES_W = false, EXT = false;
    float b1, b2, eps, bc1, bc2_sqrt;
    __device__ __forceinline__ AdamRule(float hp0, float hp1, float eps_, float bc1_, float bc2_sqrt_) : b1(hp0), b2(hp1), eps(eps_), bc1(bc1_), bc2_sqrt(bc2_sqrt_) {}
    __device__ __forceinline__ void update(float& pi, float& gi, float& mi_, float& vi_, float g2i, bool has_g2, float lr, int zero_grad) const {
#pragma clang fp contract(off)
        if (has_g2) gi += g2i;   // second gradient arena (the B-crop plan): g = g + g2, as a separate add would leave it
        const float mi = b1 * mi_ + (1.f - b1) * gi;
        const float vi = b2 * vi_ + (1.f - b2) * gi * gi;
        mi_ = mi;
        vi_ = vi;
        const float denom = sqrtf(vi) / bc2_sqrt + eps;
        pi -= (lr / bc1) * (mi / denom);
        if (zero_grad) gi = 0.f;
    }
};
// RMSprop (alpha 0.99, eps 1e-8; no momentum, not centred, no weight decay): v = alpha v + (1 - alpha) g^2, p -= lr g / (sqrt(v) + eps);
// the v arena holds square_avg
struct RmspropRule {
    static constexpr bool USES_M = false, USES_V = true, USES_W = false, EXT = false;
    float alpha, eps;
    __device__ __forceinline__ RmspropRule(float hp0, float, float eps_, float, float) : alpha(hp0), eps(eps_) {}
    __device__ __forceinline__ void update(float& pi, float& gi, float&, float& vi_, float g2i, bool has_g2, float lr, int zero_grad) const {
#pragma clang fp contract(off)
        if (has_g2) gi += g2i;
        const float vi = alpha * vi_ + (1.f - alpha) * gi * gi;
        vi_ = vi;
        pi -= lr * (gi / (sqrtf(vi) + eps));
        if (zero_grad) gi = 0.f;
    }
};
// SGD (no momentum, dampening, nesterov or weight decay): p -= lr g
struct SgdRule {
    static constexpr bool USES_M = false, USES_V = false, USES_W = false, EXT = false;
    __device__ __forceinline__ SgdRule(float, float, float, float, float) {}
    __device__ __forceinline__ void update(float& pi, float& gi, float&, float&, float g2i, bool has_g2, float lr, int zero_grad) const {
#pragma clang fp contract(off)
        if (has_g2) gi += g2i;
        pi -= lr * gi;
        if (zero_grad) gi = 0.f;
    }
};

// ---- the extended rules (OptimArgs::ext; include/splice_hip.h states them): torch.optim's weight_decay, momentum /
// dampening / nesterov, amsgrad, centered, and AdamW's decoupled decay.  Which arenas a rule walks is a template property (MOM: the m arena
// holds SGD's / RMSprop's momentum buffer; AMS / CEN: the third arena w holds max_exp_avg_sq / grad_avg); the scalar options are wave-uniform
// run-time values, and a zero wd is a BRANCH, never a multiplication by zero: with neutral options a rule computes the plain rule's bits.
// The decay term enters d alone: where g is written back it holds what the plain rules leave there.  t: the update's step count.
struct OptimExtArgs {   // the trailing by-value kernel argument (not preloaded into SGPRs: the plain instances do not read it)
    float* w;
    float wd, mu, damp;
    int nesterov, decoupled;
};
__device__ __forceinline__ float ext_decay(float gi, float pi, float wd) {
#pragma clang fp contract(off)
    return wd != 0.f ? gi + wd * pi : gi;
}
template <bool AMS>
struct AdamExtRule {
    static constexpr bool USES_M = true, USES_V = true, USES_W = AMS, EXT = true;
    float b1, b2, eps, bc1, bc2_sqrt, wd;
    bool decoupled;
    __device__ __forceinline__ AdamExtRule(float hp0, float hp1, float eps_, float bc1_, float bc2_sqrt_, const OptimExtArgs& x, int)
        : b1(hp0), b2(hp1), eps(eps_), bc1(bc1_), bc2_sqrt(bc2_sqrt_), wd(x.wd), decoupled(x.decoupled != 0) {}
    __device__ __forceinline__ void update(float& pi, float& gi, float& mi_, float& vi_, float& wi_, float g2i, bool has_g2, float lr, int zero_grad) const {
#pragma clang fp contract(off)
        if (has_g2) gi += g2i;
        float di = gi;
        if (decoupled) {
            if (wd != 0.f) pi = pi * (1.f - lr * wd);   // AdamW: the decay acts on the weights, the moments see the gradient alone
        } else {
            di = ext_decay(gi, pi, wd);
        }
        const float mi = b1 * mi_ + (1.f - b1) * di;
        const float vi = b2 * vi_ + (1.f - b2) * di * di;
        mi_ = mi;
        vi_ = vi;
        float vh = vi;
        if (AMS) { vh = fmaxf(wi_, vi); wi_ = vh; }
        const float denom = sqrtf(vh) / bc2_sqrt + eps;
        pi -= (lr / bc1) * (mi / denom);
        if (zero_grad) gi = 0.f;
    }
};
// RMSprop: the w arena holds grad_avg (CEN), the m arena the momentum buffer (MOM).  sqrt(v - a a) is not clamped, as torch does not
// clamp it: a gradient that is constant over thousands of steps can round v - a a below 0, and the slot's weights then turn NaN
template <bool MOM, bool CEN>
struct RmspropExtRule {
    static constexpr bool USES_M = MOM, USES_V = true, USES_W = CEN, EXT = true;
    float alpha, eps, wd, mu;
    __device__ __forceinline__ RmspropExtRule(float hp0, float, float eps_, float, float, const OptimExtArgs& x, int) : alpha(hp0), eps(eps_), wd(x.wd), mu(x.mu) {}
    __device__ __forceinline__ void update(float& pi, float& gi, float& mi_, float& vi_, float& wi_, float g2i, bool has_g2, float lr, int zero_grad) const {
#pragma clang fp contract(off)
        if (has_g2) gi += g2i;
        const float di = ext_decay(gi, pi, wd);
        const float vi = alpha * vi_ + (1.f - alpha) * di * di;
        vi_ = vi;
        float avg;
        if (CEN) {
            const float ai = alpha * wi_ + (1.f - alpha) * di;
            wi_ = ai;
            avg = sqrtf(vi - ai * ai) + eps;
        } else {
            avg = sqrtf(vi) + eps;
        }
        if (MOM) {
            const float bi = mu * mi_ + di / avg;
            mi_ = bi;
            pi -= lr * bi;
        } else {
            pi -= lr * (di / avg);
        }
        if (zero_grad) gi = 0.f;
    }
};
// SGD: "first step" is t == 1 (b = d); a slot whose first update the non-finite-norm guard skipped starts from b = 0 at t == 2, where torch's
// "buffer is None" rule would copy d then
template <bool MOM>
struct SgdExtRule {
    static constexpr bool USES_M = MOM, USES_V = false, USES_W = false, EXT = true;
    float wd, mu, damp1;
    bool nesterov, first;
    __device__ __forceinline__ SgdExtRule(float, float, float, float, float, const OptimExtArgs& x, int t)
        : wd(x.wd), mu(x.mu), damp1(1.f - x.damp), nesterov(x.nesterov != 0), first(t == 1) {}
    __device__ __forceinline__ void update(float& pi, float& gi, float& mi_, float&, float&, float g2i, bool has_g2, float lr, int zero_grad) const {
#pragma clang fp contract(off)
        if (has_g2) gi += g2i;
        float di = ext_decay(gi, pi, wd);
        if (MOM) {
            const float bi = first ? di : mu * mi_ + damp1 * di;
            mi_ = bi;
            di = nesterov ? di + mu * bi : bi;
        }
        pi -= lr * di;
        if (zero_grad) gi = 0.f;
    }
};
template <class Rule>
__device__ __forceinline__ Rule make_rule(float hp0, float hp1, float eps, float bc1, float bc2_sqrt, const OptimExtArgs& x, int t) {
    if constexpr (Rule::EXT) return Rule(hp0, hp1, eps, bc1, bc2_sqrt, x, t);
    else return Rule(hp0, hp1, eps, bc1, bc2_sqrt);
}

// The weight average (OptimArgs::ema): e follows the parameter just written.  track: the update's step count is <= ema_start, the average
// still copies the weights.  Afterwards e = d e + (1 - d) p', three roundings like the moment rules.
__device__ __forceinline__ float ema_update(float ei, float pi, float d, bool track) {
#pragma clang fp contract(off)
    return track ? pi : d * ei + (1.f - d) * pi;
}

// Gradient clipping (OptimArgs::clip): the element's gradient is the sum of the two arenas times the pair's coefficient, two roundings.
__device__ __forceinline__ float clip_scale(float gi, float g2i, bool has_g2, float coef) {
#pragma clang fp contract(off)
    if (has_g2) gi += g2i;
    return gi * coef;
}

// ---- the walk.  One float4 per thread and (at the generator's size) ONE pass: the operand vectors of an element group are a single
// memory round trip; the kernel is the last node of the step's critical chain.
// PAIR_LR: every pair of the arena has its own learning rate, lr_ptr[element / lr_stride] (lr_stride = the arena stride, a multiple
// of 4: a float4 never straddles two pairs).
// The argument list is the same for every rule (a rule ignores what it does not use) and keeps Adam's order: the pointers and Adam's
// scalars fill the 16 preloaded kernel-argument SGPRs.  RMSprop and SGD pay for the shared list: their g2 / lr_ptr / zero_grad lie
// behind the preloaded 16 and cost one scalar load at the kernel's head (SGD +0.3 us, RMSprop +0.1 us per launch at one pair, nothing
// measurable at eight).  Argument lists of their own need the walk in an inlined function, which the compiler
// schedules differently (the per-pair-lr instances then take 1-2 VGPRs more than before): not done.
// MASKED (the plateau stop rule): element i belongs to slot i / mask_stride (mask_stride 0: the one arena is slot 0), and the elements
// of a slot that is frozen at this step (stop_frozen; the step index is *mask_step - 1) are SKIPPED: no write to p, m or v, and no
// write-back of g either -- neither the g += g2 sum nor zero_grad.  A frozen slot's gradient arena may therefore hold anything
// (the sum of an earlier step, this step's backward output): nothing reads it, the next step's backward overwrites it.  The three
// arguments lie behind the existing list; the instances without MASKED do not read them and compile to what they were (same
// VGPR / SGPR counts, no scratch).
// EMA (the weight average): a fifth arena e with p's layout, written in the same walk behind the parameter of the element (ema_update).
// The step count is *ema_step_ptr where set (the fused step's device count), else the host's ema_step; every rule reads it here, RMSprop
// and SGD too.  An unaligned e sends the call down the scalar path like any other arena; a frozen slot's e is skipped with the rest of
// it.  The five arguments lie behind the masked ones, and the instances without EMA do not read them.
// CLIP (gradient clipping by the pair's global norm): element i uses the record clip[i / clip_stride] (clip_stride 0: slot 0, read once
// at the kernel's head) that grad_norm_launch wrote for this gradient.  The rule sees gi = fl(fl(g + g2) * coef) -- multiplied when coef is 1 too, which changes no
// bit -- and where g is written back it holds that value.  A slot whose record has skip set (its norm was not finite) is left as it is:
// no write to p, m, v or e; its g is written only as the zeros of zero_grad.  A frozen slot is skipped before its record is read.  The
// two arguments lie behind the EMA ones, and the instances without CLIP do not read them.
// BEST (keep the best window's weights; only with MASKED, whose records and step count it needs): the slot's record best[i / mask_stride]
// (mask_stride 0: slot 0, read once at the kernel's head) was written by this step's loss kernel; where its best_step is this step's index
// -- `take` -- the parameter just written goes to best_p[i] as well, and with EMA the average just written to best_e[i]: copies of the
// registers the ordinary stores hold, no float is computed again.  A frozen slot is skipped before its record is read; a slot skipped by
// the clip guard still takes, its unchanged p (and e).  best_p / best_e take part in the alignment test like every arena.  The three
// arguments lie behind the CLIP ones, and the instances without BEST do not read them.
// Extended rules (Rule::EXT): the options and the third moment arena w (Rule::USES_W; loaded, stored and alignment-tested like m and v,
// and skipped with them where a slot is frozen or skipped by the clip guard) arrive as ONE trailing by-value struct -- a struct is not
// preloaded into SGPRs, so the plain instances, which do not read it, keep their registers and, but for the offset of the hidden grid
// size behind it, their instructions.  An extended rule counts the update's steps as the average does.
template <class Rule, bool PAIR_LR, bool MASKED, bool EMA, bool CLIP, bool BEST = false>
__global__ void optim_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                             float hp0, float hp1, float eps, float bc1, float bc2_sqrt, int zero_grad, const int* __restrict__ step_ptr,
                             const float* __restrict__ g2, const float* __restrict__ lr_ptr, unsigned lr_stride,
                             const splice_stop_state* __restrict__ mask, const int* __restrict__ mask_step, unsigned mask_stride,
                             float* __restrict__ e, float ema_decay, int ema_start, const int* __restrict__ ema_step_ptr, int ema_step,
                             const splice_clip_state* __restrict__ clip, unsigned clip_stride,
                             const splice_best_state* __restrict__ best, float* __restrict__ best_p, float* __restrict__ best_e,
                             const OptimExtArgs ext) {
    static_assert(MASKED || !BEST, "the snapshot needs the stop records and the device step count");
    int step_idx = 0;
    if (MASKED) {
        step_idx = *mask_step - 1;
        if (!mask_stride && stop_frozen(mask, step_idx)) return;
    }
    if (!PAIR_LR && lr_ptr) lr = *lr_ptr;   // learning rate on the device (a schedule under graph replay); null: the argument
    if (step_ptr) {   // Adam's step count lives on the device (graph replay): bias corrections computed here
        const float t = (float)*step_ptr;
        bc1 = 1.0f - powf(hp0, t);
        bc2_sqrt = sqrtf(1.0f - powf(hp1, t));
    }
    bool ema_track = false;
    if (EMA) ema_track = (ema_step_ptr ? *ema_step_ptr : ema_step) <= ema_start;
    // (an extended rule counts the update's steps as the average does)
    const Rule rule = make_rule<Rule>(hp0, hp1, eps, bc1, bc2_sqrt, ext, Rule::EXT ? (ema_step_ptr ? *ema_step_ptr : ema_step) : 0);
    float* const w = Rule::USES_W ? ext.w : nullptr;
    // one arena: its record is read once, at the head, with the step count; several: per element group, behind the group's own loads
    float coef = 1.f;
    int skip = 0;
    if (CLIP && !clip_stride) { coef = clip->coef; skip = clip->skip; }
    bool take = false;
    if (BEST && !mask_stride) take = best->best_step == step_idx;
    auto upd = [&](float& pi, float& gi, float& mi, float& vi, float& wi, float g2i) {
        if constexpr (Rule::EXT) {
            if (CLIP) {
                gi = clip_scale(gi, g2i, g2 != nullptr, coef);
                rule.update(pi, gi, mi, vi, wi, 0.f, false, lr, zero_grad);
            } else {
                rule.update(pi, gi, mi, vi, wi, g2i, g2 != nullptr, lr, zero_grad);
            }
        } else if (CLIP) {
            gi = clip_scale(gi, g2i, g2 != nullptr, coef);
            rule.update(pi, gi, mi, vi, 0.f, false, lr, zero_grad);
        } else {
            rule.update(pi, gi, mi, vi, g2i, g2 != nullptr, lr, zero_grad);
        }
    };
    const unsigned lr_stride4 = lr_stride / 4, mask_stride4 = mask_stride / 4, clip_stride4 = clip_stride / 4;
    const size_t align = reinterpret_cast<size_t>(p) | reinterpret_cast<size_t>(g) | (Rule::USES_M ? reinterpret_cast<size_t>(m) : 0) |
                         (Rule::USES_V ? reinterpret_cast<size_t>(v) : 0) | reinterpret_cast<size_t>(g2) | (EMA ? reinterpret_cast<size_t>(e) : 0) |
                         (BEST ? reinterpret_cast<size_t>(best_p) : 0) | (BEST && EMA ? reinterpret_cast<size_t>(best_e) : 0) |
                         (Rule::USES_W ? reinterpret_cast<size_t>(w) : 0);
    const size_t n4 = (align & 15) ? 0 : n / 4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        if (MASKED && mask_stride && stop_frozen(mask + (unsigned)i / mask_stride4, step_idx)) continue;
        float4 pv = reinterpret_cast<float4*>(p)[i], gv = reinterpret_cast<float4*>(g)[i], mv = {}, vv = {}, wv = {};
        if (Rule::USES_M) mv = reinterpret_cast<float4*>(m)[i];
        if (Rule::USES_V) vv = reinterpret_cast<float4*>(v)[i];
        if (Rule::USES_W) wv = reinterpret_cast<float4*>(w)[i];
        const float4 g2v = g2 ? reinterpret_cast<const float4*>(g2)[i] : float4{0.f, 0.f, 0.f, 0.f};
        if (PAIR_LR) lr = lr_ptr[(unsigned)i / lr_stride4];
        if (BEST && mask_stride4) take = best[(unsigned)i / mask_stride4].best_step == step_idx;
        if (CLIP) {
            if (clip_stride4) {
                const splice_clip_state* cs = clip + (unsigned)i / clip_stride4;
                coef = cs->coef;
                skip = cs->skip;
            }
            if (skip) {
                if (zero_grad) reinterpret_cast<float4*>(g)[i] = float4{0.f, 0.f, 0.f, 0.f};
                if (BEST && take) {   // (the slot is left as it is: its snapshot is the p and e it has)
                    reinterpret_cast<float4*>(best_p)[i] = pv;
                    if (EMA) reinterpret_cast<float4*>(best_e)[i] = reinterpret_cast<float4*>(e)[i];
                }
                continue;
            }
        }
        upd(pv.x, gv.x, mv.x, vv.x, wv.x, g2v.x); upd(pv.y, gv.y, mv.y, vv.y, wv.y, g2v.y); upd(pv.z, gv.z, mv.z, vv.z, wv.z, g2v.z); upd(pv.w, gv.w, mv.w, vv.w, wv.w, g2v.w);
        reinterpret_cast<float4*>(p)[i] = pv;
        if (BEST && take) reinterpret_cast<float4*>(best_p)[i] = pv;
        if (EMA) {
            float4 ev = pv;   // (a tracking average is the parameter: e is not read)
            if (!ema_track) ev = reinterpret_cast<float4*>(e)[i];
            ev.x = ema_update(ev.x, pv.x, ema_decay, ema_track); ev.y = ema_update(ev.y, pv.y, ema_decay, ema_track);
            ev.z = ema_update(ev.z, pv.z, ema_decay, ema_track); ev.w = ema_update(ev.w, pv.w, ema_decay, ema_track);
            reinterpret_cast<float4*>(e)[i] = ev;
            if (BEST && take) reinterpret_cast<float4*>(best_e)[i] = ev;
        }
        if (Rule::USES_M) reinterpret_cast<float4*>(m)[i] = mv;
        if (Rule::USES_V) reinterpret_cast<float4*>(v)[i] = vv;
        if (Rule::USES_W) reinterpret_cast<float4*>(w)[i] = wv;
        if (g2 || zero_grad) reinterpret_cast<float4*>(g)[i] = gv;
    }
    for (size_t i = n4 * 4 + (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        if (MASKED && mask_stride && stop_frozen(mask + (unsigned)i / mask_stride, step_idx)) continue;
        if (BEST && mask_stride) take = best[(unsigned)i / mask_stride].best_step == step_idx;
        if (CLIP) {
            if (clip_stride) {
                const splice_clip_state* cs = clip + (unsigned)i / clip_stride;
                coef = cs->coef;
                skip = cs->skip;
            }
            if (skip) {
                if (zero_grad) g[i] = 0.f;
                if (BEST && take) {
                    best_p[i] = p[i];
                    if (EMA) best_e[i] = e[i];
                }
                continue;
            }
        }
        float pi = p[i], gi = g[i], mi = 0.f, vi = 0.f, wi = 0.f;
        if (Rule::USES_M) mi = m[i];
        if (Rule::USES_V) vi = v[i];
        if (Rule::USES_W) wi = w[i];
        if (PAIR_LR) lr = lr_ptr[(unsigned)i / lr_stride];
        upd(pi, gi, mi, vi, wi, g2 ? g2[i] : 0.f);
        p[i] = pi;
        if (BEST && take) best_p[i] = pi;
        if (EMA) {
            const float ei = ema_update(ema_track ? pi : e[i], pi, ema_decay, ema_track);
            e[i] = ei;
            if (BEST && take) best_e[i] = ei;
        }
        if (Rule::USES_M) m[i] = mi;
        if (Rule::USES_V) v[i] = vi;
        if (Rule::USES_W) w[i] = wi;
        if (g2 || zero_grad) g[i] = gi;
    }
}
static unsigned optim_grid(size_t n) {
    size_t g_ = (n / 4 + 255) / 256 + 1;
    return (unsigned)(g_ > 2048 ? 2048 : g_);
}

int optim_launch(const OptimArgs& a, hipStream_t s) {
#define OPTIM_CLIP(Rule, PAIR_LR, MASKED, EMA) {optim_kernel<Rule, PAIR_LR, MASKED, EMA, false>, optim_kernel<Rule, PAIR_LR, MASKED, EMA, true>}
#define OPTIM_EMA(Rule, PAIR_LR, MASKED) {OPTIM_CLIP(Rule, PAIR_LR, MASKED, false), OPTIM_CLIP(Rule, PAIR_LR, MASKED, true)}
#define OPTIM_INSTANCES(Rule) {{OPTIM_EMA(Rule, false, false), OPTIM_EMA(Rule, false, true)}, {OPTIM_EMA(Rule, true, false), OPTIM_EMA(Rule, true, true)}}
    static constexpr decltype(&optim_kernel<AdamRule, false, false, false, false>) kernels[3][2][2][2][2] = {
        OPTIM_INSTANCES(AdamRule), OPTIM_INSTANCES(RmspropRule), OPTIM_INSTANCES(SgdRule)};   // [kind][PAIR_LR][MASKED][EMA][CLIP]
#undef OPTIM_INSTANCES
#undef OPTIM_EMA
#undef OPTIM_CLIP
    // the snapshot rides in masked updates only: [kind][PAIR_LR][EMA][CLIP], 24 instances beside the 48 above
#define OPTIM_BEST_CLIP(Rule, PAIR_LR, EMA) {optim_kernel<Rule, PAIR_LR, true, EMA, false, true>, optim_kernel<Rule, PAIR_LR, true, EMA, true, true>}
#define OPTIM_BEST(Rule) {{OPTIM_BEST_CLIP(Rule, false, false), OPTIM_BEST_CLIP(Rule, false, true)}, {OPTIM_BEST_CLIP(Rule, true, false), OPTIM_BEST_CLIP(Rule, true, true)}}
    static constexpr decltype(&optim_kernel<AdamRule, false, false, false, false>) best_kernels[3][2][2][2] = {OPTIM_BEST(AdamRule), OPTIM_BEST(RmspropRule), OPTIM_BEST(SgdRule)};
#undef OPTIM_BEST
#undef OPTIM_BEST_CLIP
    // the extended rules: [rule][PAIR_LR][MASKED][EMA][CLIP] and, with the snapshot, [rule][PAIR_LR][EMA][CLIP]; rule = Adam {plain, amsgrad},
    // RMSprop {plain, momentum, centered, both}, SGD {plain, momentum} -- 128 + 64 instances beside the 72 of the plain rules
#define OPTIM_CLIP(Rule, PAIR_LR, MASKED, EMA) {optim_kernel<Rule, PAIR_LR, MASKED, EMA, false>, optim_kernel<Rule, PAIR_LR, MASKED, EMA, true>}
#define OPTIM_EMA(Rule, PAIR_LR, MASKED) {OPTIM_CLIP(Rule, PAIR_LR, MASKED, false), OPTIM_CLIP(Rule, PAIR_LR, MASKED, true)}
#define OPTIM_INSTANCES(Rule) {{OPTIM_EMA(Rule, false, false), OPTIM_EMA(Rule, false, true)}, {OPTIM_EMA(Rule, true, false), OPTIM_EMA(Rule, true, true)}}
#define OPTIM_BEST_CLIP(Rule, PAIR_LR, EMA) {optim_kernel<Rule, PAIR_LR, true, EMA, false, true>, optim_kernel<Rule, PAIR_LR, true, EMA, true, true>}
#define OPTIM_BEST(Rule) {{OPTIM_BEST_CLIP(Rule, false, false), OPTIM_BEST_CLIP(Rule, false, true)}, {OPTIM_BEST_CLIP(Rule, true, false), OPTIM_BEST_CLIP(Rule, true, true)}}
    using RmsExt = RmspropExtRule<false, false>;
    using RmsExtMom = RmspropExtRule<true, false>;
    using RmsExtCen = RmspropExtRule<false, true>;
    using RmsExtMomCen = RmspropExtRule<true, true>;
#define OPTIM_EXT_RULES(M) M(AdamExtRule<false>), M(AdamExtRule<true>), M(RmsExt), M(RmsExtMom), M(RmsExtCen), M(RmsExtMomCen), M(SgdExtRule<false>), M(SgdExtRule<true>)
    static constexpr decltype(&optim_kernel<AdamRule, false, false, false, false>) ext_kernels[8][2][2][2][2] = {OPTIM_EXT_RULES(OPTIM_INSTANCES)};
    static constexpr decltype(&optim_kernel<AdamRule, false, false, false, false>) ext_best_kernels[8][2][2][2] = {OPTIM_EXT_RULES(OPTIM_BEST)};
#undef OPTIM_EXT_RULES
#undef OPTIM_BEST
#undef OPTIM_BEST_CLIP
#undef OPTIM_INSTANCES
#undef OPTIM_EMA
#undef OPTIM_CLIP
    if (a.kind < SPLICE_OPT_ADAM || a.kind > SPLICE_OPT_SGD) {
        splice_set_error("optimiser: unknown optimiser kind %d", a.kind);
        return SPLICE_ERR_ARG;
    }
    const bool adam = a.kind == SPLICE_OPT_ADAM, host_step = adam && !a.step_dev;
    // the extended rules (a.ext): the options are checked as torch.optim checks its arguments, then the arenas the selected rule walks
    int ext_rule = -1;
    OptimExtArgs x = {nullptr, 0.f, 0.f, 0.f, 0, 0};
    if (a.ext) {
        const splice_optim_ext& e = *a.ext;
        const char* names[3] = {"Adam", "RMSprop", "SGD"};
        const bool finite = e.weight_decay <= 3.402823466e+38f && e.momentum <= 3.402823466e+38f && e.dampening >= -3.402823466e+38f && e.dampening <= 3.402823466e+38f;
        if (!(e.weight_decay >= 0.f) || !(e.momentum >= 0.f) || !finite) {
            splice_set_error("optimiser: weight_decay and momentum must be finite and >= 0, dampening finite, got %g, %g, %g", (double)e.weight_decay,
                             (double)e.momentum, (double)e.dampening);
            return SPLICE_ERR_ARG;
        }
        if (e.nesterov && (!(e.momentum > 0.f) || e.dampening != 0.f)) {
            splice_set_error("optimiser: nesterov needs momentum > 0 and dampening == 0, got momentum %g, dampening %g", (double)e.momentum, (double)e.dampening);
            return SPLICE_ERR_ARG;
        }
        const char* alien = (adam && (e.momentum != 0.f || e.dampening != 0.f || e.nesterov)) ? "momentum / dampening / nesterov"
                            : (adam && e.centered) || (a.kind == SPLICE_OPT_SGD && e.centered) ? "centered"
                            : (!adam && e.amsgrad) ? "amsgrad"
                            : (!adam && e.decoupled) ? "decoupled"
                            : (a.kind == SPLICE_OPT_RMSPROP && (e.dampening != 0.f || e.nesterov)) ? "dampening / nesterov" : nullptr;
        if (alien) {
            splice_set_error("optimiser: %s has no %s", names[a.kind], alien);
            return SPLICE_ERR_ARG;
        }
        const bool mom = !adam && e.momentum > 0.f;
        ext_rule = adam ? (e.amsgrad ? 1 : 0) : a.kind == SPLICE_OPT_RMSPROP ? 2 + (mom ? 1 : 0) + (e.centered ? 2 : 0) : 6 + (mom ? 1 : 0);
        const bool needs_w = adam ? e.amsgrad != 0 : e.centered != 0;
        const char* missing = !a.p ? "params" : !a.g ? "grads" : (adam || mom) && !a.m ? "m" : a.kind != SPLICE_OPT_SGD && !a.v ? "v" : needs_w && !a.w ? "w" : nullptr;
        if (missing) {
            splice_set_error("optimiser: the %s rule%s%s%s needs the %s arena, got NULL", names[a.kind], mom ? " with momentum" : "", e.amsgrad ? " with amsgrad" : "",
                             e.centered ? " (centered)" : "", missing);
            return SPLICE_ERR_ARG;
        }
        if (!a.step_dev && !a.mask_step && a.step < 1) {
            splice_set_error("optimiser: an extended rule needs the update's step count (on the device, or step >= 1), got step %d", a.step);
            return SPLICE_ERR_ARG;
        }
        x = OptimExtArgs{needs_w ? a.w : nullptr, e.weight_decay, e.momentum, e.dampening, e.nesterov ? 1 : 0, e.decoupled ? 1 : 0};
    }
    if (!a.p || !a.g || a.n < 1 || (adam && !a.m) || (a.kind != SPLICE_OPT_SGD && !a.v) || (host_step && a.step < 1)) return SPLICE_ERR_ARG;
    // per-pair learning rates index lr_dev with a 32-bit element index
    if (a.lr_stride && (!a.lr_dev || a.lr_stride % 4 || a.n > 0xFFFFFFFFull || a.lr_stride > 0xFFFFFFFFull)) {
        splice_set_error("optimiser: per-pair lr needs a device lr table, an arena stride that is a multiple of 4 and < 2^32 elements");
        return SPLICE_ERR_ARG;
    }
    // a masked update indexes the state records with a 32-bit element index too
    if (a.mask && (!a.mask_step || a.mask_stride % 4 || a.n > 0xFFFFFFFFull || a.mask_stride > 0xFFFFFFFFull || (a.lr_stride && a.mask_stride != a.lr_stride))) {
        splice_set_error("optimiser: a masked update needs the device step count, a slot stride that is a multiple of 4 (the per-pair lr stride where both are set) and < 2^32 elements");
        return SPLICE_ERR_ARG;
    }
    // the weight average counts the update's steps: the device count of the fused step, or the host's
    const int* ema_step_dev = a.step_dev ? a.step_dev : a.mask_step;
    if (a.ema && (!(a.ema_decay > 0.f && a.ema_decay < 1.f) || a.ema_start < 0 || (!ema_step_dev && a.step < 1))) {
        splice_set_error("optimiser: a weight average needs 0 < ema_decay < 1, ema_start >= 0 and a step count (on the device, or step >= 1)");
        return SPLICE_ERR_ARG;
    }
    // the clip records are indexed like the stop records
    if (a.clip && (a.clip_stride % 4 || a.n > 0xFFFFFFFFull || a.clip_stride > 0xFFFFFFFFull || (a.lr_stride && a.clip_stride != a.lr_stride) ||
                   (a.mask && a.clip_stride != a.mask_stride))) {
        splice_set_error("optimiser: a clipped update needs a slot stride that is a multiple of 4 (that of the per-pair lr and of the mask where they are set) and < 2^32 elements");
        return SPLICE_ERR_ARG;
    }
    // the snapshot reads the record of the slot the stop records name: it needs them, its arena and -- exactly with an average -- the best average
    if (a.best && (!a.mask || !a.best_p || (a.best_ema != nullptr) != (a.ema != nullptr))) {
        splice_set_error("optimiser: keeping the best weights needs the stop records, the best arena and a best average exactly when an average is kept");
        return SPLICE_ERR_ARG;
    }
    // a host step count: the bias corrections come from the HOST's powf (host and device powf need not agree to the bit, so a caller
    // stays with the form it has)
    const float bc1 = host_step ? 1.0f - powf(a.hp0, (float)a.step) : 1.f;
    const float bc2_sqrt = host_step ? sqrtf(1.0f - powf(a.hp1, (float)a.step)) : 1.f;
    const auto kernel = ext_rule >= 0 ? (a.best ? ext_best_kernels[ext_rule][a.lr_stride != 0][a.ema != nullptr][a.clip != nullptr]
                                                : ext_kernels[ext_rule][a.lr_stride != 0][a.mask != nullptr][a.ema != nullptr][a.clip != nullptr])
                        : a.best      ? best_kernels[a.kind][a.lr_stride != 0][a.ema != nullptr][a.clip != nullptr]
                                      : kernels[a.kind][a.lr_stride != 0][a.mask != nullptr][a.ema != nullptr][a.clip != nullptr];
    SPLICE_LAUNCH(kernel, dim3(optim_grid(a.n)), dim3(256), 0, s, a.p, a.g, a.m, a.v, a.n, a.lr, a.hp0, a.hp1, a.eps, bc1, bc2_sqrt, a.zero_grad,
                  adam ? a.step_dev : nullptr, a.g2, a.lr_dev, (unsigned)a.lr_stride, a.mask, a.mask_step, (unsigned)a.mask_stride,
                  a.ema, a.ema_decay, a.ema_start, ema_step_dev, a.step, a.clip, (unsigned)a.clip_stride, a.best, a.best_p, a.best_ema, x);
    return SPLICE_OK;
}

// ---- the gradient norm of every pair (include/splice_hip.h states the rule).  No float atomics and a fixed
// assignment of elements to threads and of chunks to partials, counted from the start of the pair's arena: a pair's sum does not depend
// on the other pairs of the launch.
// Stage 1: workgroup (chunk, pair) sums the squares of SPLICE_CLIP_CHUNK floats.  An arena that is not 16-byte aligned (and the float4
// that straddles n) is read element by element into the same thread and component, so the bits are the same.
static_assert(SPLICE_CLIP_CHUNK == 4 * 4 * 256, "a chunk is four float4 rounds of 256 threads");
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* __restrict__ g, const float* __restrict__ g2, size_t stride, size_t n,
                                                         float* __restrict__ partials, const splice_stop_state* __restrict__ stop,
                                                         const int* __restrict__ step_dev) {
#pragma clang fp contract(off)
    __shared__ float sm[256];
    const unsigned pair = blockIdx.y, t = threadIdx.x;
    if (stop && stop_frozen(stop + pair, *step_dev - 1)) return;
    const float* a = g + (size_t)pair * stride;
    const float* b = g2 ? g2 + (size_t)pair * stride : nullptr;
    const bool vec = ((reinterpret_cast<size_t>(a) | reinterpret_cast<size_t>(b)) & 15) == 0;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const size_t e = (size_t)blockIdx.x * SPLICE_CLIP_CHUNK + (size_t)j * 1024 + t * 4;
        float s[4] = {0.f, 0.f, 0.f, 0.f};   // (an element at or beyond n adds +0)
        if (vec && e + 4 <= n) {
            const float4 x = *reinterpret_cast<const float4*>(a + e);
            s[0] = x.x; s[1] = x.y; s[2] = x.z; s[3] = x.w;
            if (b) {
                const float4 y = *reinterpret_cast<const float4*>(b + e);
                s[0] += y.x; s[1] += y.y; s[2] += y.z; s[3] += y.w;
            }
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (e + c < n) {
                    s[c] = a[e + c];
                    if (b) s[c] += b[e + c];
                }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) acc += s[c] * s[c];
    }
    // the halving tree a[t] += a[t + off]: off = 128 and 64 across the waves through LDS, 32 .. 1 inside wave 0 (lane t < off reads t + off)
    sm[t] = acc;
    __syncthreads();
    if (t < 64) {
        float v = (sm[t] + sm[t + 128]) + (sm[t + 64] + sm[t + 192]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (t == 0) partials[(size_t)pair * gridDim.x + blockIdx.x] = v;
    }
}
// Stage 2: workgroup = pair.  The partials in fp64 (their order is fixed, the rounding of 254 of them no longer shows in the fp32 result),
// then the record.  Thread 0 alone writes it.  TRACE (the loss trace): it also stores the norm and the coefficient into
// words 6 and 7 of row *step_dev - 1 of the pair's trace ([capacity][pairs][8]; words 0-5 belong to total_loss_kernel), a row beyond
// capacity left out.  The instance without TRACE does not read the two trailing arguments.  AUTO (clipping against the pair's own running
// norm): the threshold is the smaller of max_norm (0: none) and k times the reference of the step's regime in the
// pair's second record, which thread 0 then moves towards the norm; a frozen pair keeps both records.  The rule lies behind the TRACE
// arguments as ONE by-value struct -- a struct is not preloaded into SGPRs, so the preloaded arguments, and with them the register the
// workgroup index arrives in, are those of the instances without AUTO, which do not read it.
template <bool TRACE, bool AUTO = false>
__global__ __launch_bounds__(256) void grad_clip_coef_kernel(const float* __restrict__ partials, unsigned chunks, float max_norm,
                                                             splice_clip_state* __restrict__ state, const splice_stop_state* __restrict__ stop,
                                                             const int* __restrict__ step_dev, float* __restrict__ trace, int capacity,
                                                             const ClipAutoRule rule) {
#pragma clang fp contract(off)
    __shared__ double sd[256];
    const unsigned pair = blockIdx.x, t = threadIdx.x;
    if (stop && stop_frozen(stop + pair, *step_dev - 1)) return;
    const float* part = partials + (size_t)pair * chunks;
    double acc = 0.0;
    for (unsigned i = t; i < chunks; i += 256) acc += (double)part[i];
    sd[t] = acc;
    __syncthreads();
    if (t < 64) {
        double v = (sd[t] + sd[t + 128]) + (sd[t + 64] + sd[t + 192]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (t == 0) {
            splice_clip_state r = state[pair];
            r.sumsq = (float)v;
            r.norm = sqrtf(r.sumsq);
            float thr = max_norm, thr_auto = __builtin_inff(), ref = 0.f;
            int seen = 0;
            const int regime = rule.regime;
            splice_clip_auto_state* const rec = rule.records + pair;
            if (AUTO) {   // (regime -1: no reference is read or written, the cap alone acts)
                if (regime >= 0) {
                    ref = rec->ref[regime];
                    seen = rec->count[regime];
                    if (seen >= rule.warmup && ref > 0.f) thr_auto = rule.k * ref;
                }
                thr = max_norm > 0.f ? fminf(max_norm, thr_auto) : thr_auto;
            }
            if (r.norm <= 3.402823466e+38f) {   // finite (a NaN compares false)
                r.coef = fminf(1.f, thr / (r.norm + 1e-6f));   // (+inf / x = +inf: coef 1)
                r.skip = 0;
                r.clipped += r.coef < 1.f ? 1 : 0;
                if (AUTO && regime >= 0) {
                    const float x = fminf(r.norm, thr_auto);   // a spike raises the reference by at most the factor k
                    rec->ref[regime] = seen == 0 ? x : rule.beta * ref + (1.f - rule.beta) * x;
                    rec->count[regime] = seen + 1;
                }
            } else {
                r.coef = 0.f;
                r.skip = 1;
                r.skipped += 1;
            }
            state[pair] = r;
            if (AUTO) {
                rec->thr = thr;
                rec->regime = regime;
            }
            if (TRACE) {
                const int row = *step_dev - 1;
                if (row >= 0 && row < capacity) {
                    float* tr = trace + ((size_t)row * gridDim.x + pair) * 8;
                    tr[6] = r.norm;
                    tr[7] = r.coef;
                }
            }
        }
    }
}

int grad_norm_launch(const float* g, const float* g2, int pairs, size_t stride, size_t n, float max_norm, float* partials, splice_clip_state* state,
                     const splice_stop_state* stop, const int* step_dev, hipStream_t s, float* trace, int capacity, const ClipAutoRule* rule) {
    if (rule) {   // the cap is optional beside the running norm
        if (!(max_norm >= 0.f) || !(max_norm <= 3.402823466e+38f)) {
            splice_set_error("gradient clipping: beside the running norm max_norm must be a finite number >= 0 (0: no cap), got %g", (double)max_norm);
            return SPLICE_ERR_ARG;
        }
        if (!(rule->k >= 1.f) || !(rule->k <= 3.402823466e+38f) || !(rule->beta >= 0.f && rule->beta < 1.f) || rule->warmup < 1 || rule->regime < -1 ||
            rule->regime > 1 || !rule->records) {
            splice_set_error("gradient clipping (max_norm %g): the running norm needs a finite k >= 1, 0 <= beta < 1, warmup >= 1, a regime of -1, 0 or 1 and its records, got k %g, beta %g, warmup %d, regime %d",
                             (double)max_norm, (double)rule->k, (double)rule->beta, rule->warmup, rule->regime);
            return SPLICE_ERR_ARG;
        }
    } else if (!(max_norm > 0.f) || !(max_norm <= 3.402823466e+38f)) {
        splice_set_error("gradient clipping: max_norm must be a finite number > 0, got %g", (double)max_norm);
        return SPLICE_ERR_ARG;
    }
    if (!g || !partials || !state || pairs < 1 || n < 1 || (stop && !step_dev)) {
        splice_set_error("gradient clipping (max_norm %g): needs the gradient arena, the partials and the state records, n_pairs >= 1, n >= 1 and the device step count with stop records",
                         (double)max_norm);
        return SPLICE_ERR_ARG;
    }
    if (pairs > 1 && (stride % 4 || stride < n)) {
        splice_set_error("gradient clipping (max_norm %g): more than one pair needs n <= stride with stride a multiple of 4", (double)max_norm);
        return SPLICE_ERR_ARG;
    }
    const size_t chunks = (n + SPLICE_CLIP_CHUNK - 1) / SPLICE_CLIP_CHUNK;
    if (chunks > 0x7FFFFFFFull || pairs > 65535) {
        splice_set_error("gradient clipping (max_norm %g): at most 65535 pairs of < 2^43 floats", (double)max_norm);
        return SPLICE_ERR_ARG;
    }
    if (trace && (!step_dev || capacity < 1)) {
        splice_set_error("gradient clipping (max_norm %g): a loss trace needs the device step count and a capacity >= 1", (double)max_norm);
        return SPLICE_ERR_ARG;
    }
    if (pairs == 1) stride = 0;
    SPLICE_LAUNCH(grad_sumsq_kernel, dim3((unsigned)chunks, (unsigned)pairs), dim3(256), 0, s, g, g2, stride, n, partials, stop, step_dev);
    const ClipAutoRule a = rule ? *rule : ClipAutoRule{0.f, 0.f, 0, 0, nullptr};
    if (!trace) capacity = 0;
    // (the trace and the running norm ride in the launch)
#define CLIP_COEF_LAUNCH(TRACE, AUTO)                                                                                                                   \
    SPLICE_LAUNCH((grad_clip_coef_kernel<TRACE, AUTO>), dim3((unsigned)pairs), dim3(256), 0, s, (const float*)partials, (unsigned)chunks, max_norm, state, \
                  stop, step_dev, trace, capacity, a)
    if (rule) {
        if (trace) CLIP_COEF_LAUNCH(true, true); else CLIP_COEF_LAUNCH(false, true);
    } else {
        if (trace) CLIP_COEF_LAUNCH(true, false); else CLIP_COEF_LAUNCH(false, false);
    }
#undef CLIP_COEF_LAUNCH
    return SPLICE_OK;
}

// ---- exports (include/splice_hip.h): fillers of OptimArgs
static OptimArgs optim_args(int kind, float* params, float* grads, const float* g2, float* m, float* v, long long n, float lr, const float* lr_dev,
                            size_t lr_stride, float hp0, float hp1, float eps, int step, int zero_grad) {
    return OptimArgs{kind, params, grads, g2, m, v, n < 1 ? 0 : (size_t)n, lr, lr_dev, lr_stride, hp0, hp1, eps, step, nullptr, zero_grad, nullptr, nullptr, 0};
}
extern "C" {
int splice_adam_step(float* params, float* grads, float* m, float* v, long long n, float lr, float beta1, float beta2, float eps, int step,
                     int zero_grad, splice_stream_t stream) {
    return optim_launch(optim_args(SPLICE_OPT_ADAM, params, grads, nullptr, m, v, n, lr, nullptr, 0, beta1, beta2, eps, step, zero_grad), (hipStream_t)stream);
}
int splice_optim_step_ex(int kind, float* params, float* grads, const float* g2, float* m, float* v, long long n, float lr, const float* lr_dev,
                         float hp0, float hp1, float eps, int step, int zero_grad, splice_stream_t stream) {
    return optim_launch(optim_args(kind, params, grads, g2, m, v, n, lr, lr_dev, 0, hp0, hp1, eps, step, zero_grad), (hipStream_t)stream);
}
// as splice_optim_step_ex with the weight average `ema` updated in the same walk; step >= 1 for every kind (the average counts it)
int splice_optim_step_ema(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, long long n, float lr,
                          const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad, float ema_decay, int ema_start,
                          splice_stream_t stream) {
    if (!ema) { splice_set_error("splice_optim_step_ema: needs the ema arena"); return SPLICE_ERR_ARG; }
    OptimArgs a = optim_args(kind, params, grads, g2, m, v, n, lr, lr_dev, 0, hp0, hp1, eps, step, zero_grad);
    a.ema = ema; a.ema_decay = ema_decay; a.ema_start = ema_start;
    return optim_launch(a, (hipStream_t)stream);
}
int splice_optim_step(int kind, float* params, float* grads, float* m, float* v, long long n, float lr, float hp0, float hp1, float eps, int step,
                      int zero_grad, splice_stream_t stream) {
    return splice_optim_step_ex(kind, params, grads, nullptr, m, v, n, lr, nullptr, hp0, hp1, eps, step, zero_grad, stream);
}
// The OptimArgs of the pairs forms.  slot: floats between two pairs' arenas and the stride of every per-pair table; the whole range
// n_pairs * slot is updated, the padding floats between two arenas included (they hold zero gradients, so they stay as they are).
// slot 0: a single arena of n floats, slot 0 of every table.  step_dev / stop / ema / clip / best: optional.
static OptimArgs pairs_args(int kind, float* params, float* grads, const float* g2, float* m, float* v, int n_pairs, size_t slot, long long n,
                            const float* lr_dev, float hp0, float hp1, float eps, int step, const int* step_dev, const splice_stop_state* stop,
                            int zero_grad, float* ema, float ema_decay, int ema_start, const splice_clip_state* clip, const splice_best_state* best,
                            float* best_params, float* best_ema) {
    OptimArgs a = optim_args(kind, params, grads, g2, m, v, slot ? (long long)n_pairs * (long long)slot : n, 0.f, lr_dev, slot, hp0, hp1, eps, step, zero_grad);
    a.step_dev = step_dev;
    if (stop) { a.mask = stop; a.mask_step = step_dev; a.mask_stride = slot; }
    if (ema) { a.ema = ema; a.ema_decay = ema_decay; a.ema_start = ema_start; }
    if (clip) { a.clip = clip; a.clip_stride = slot; }
    a.best = best; a.best_p = best_params; a.best_ema = best_ema;
    return a;
}
int splice_optim_step_pairs(int kind, float* params, float* grads, const float* g2, float* m, float* v, int n_pairs, long long stride, long long n,
                            const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad, splice_stream_t stream) {
    if (!params || !grads || !lr_dev || n_pairs < 1 || n < 1 || stride < n || stride % 4) {
        splice_set_error("splice_optim_step_pairs: needs a device lr table, n_pairs >= 1 and 1 <= n <= stride with stride a multiple of 4");
        return SPLICE_ERR_ARG;
    }
    return optim_launch(pairs_args(kind, params, grads, g2, m, v, n_pairs, (size_t)stride, n, lr_dev, hp0, hp1, eps, step, nullptr, nullptr, zero_grad, nullptr, 0.f, 0,
                                   nullptr, nullptr, nullptr, nullptr), (hipStream_t)stream);
}
// as splice_optim_step_pairs with the weight average, the fused step's form of the launch: the step count is read from the device
// (step_dev), and with `stop` ([n_pairs] records) a pair that is frozen at step *step_dev - 1 is skipped -- its ema with the rest of it
int splice_optim_step_pairs_ema(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, int n_pairs, long long stride,
                                long long n, const float* lr_dev, float hp0, float hp1, float eps, const int* step_dev, const splice_stop_state* stop,
                                int zero_grad, float ema_decay, int ema_start, splice_stream_t stream) {
    if (!params || !grads || !ema || !lr_dev || !step_dev || n_pairs < 1 || n < 1 || stride < n || stride % 4) {
        splice_set_error("splice_optim_step_pairs_ema: needs the ema arena, a device lr table and step count, n_pairs >= 1 and 1 <= n <= stride with stride a multiple of 4");
        return SPLICE_ERR_ARG;
    }
    return optim_launch(pairs_args(kind, params, grads, g2, m, v, n_pairs, (size_t)stride, n, lr_dev, hp0, hp1, eps, 0, step_dev, stop, zero_grad, ema, ema_decay, ema_start,
                                   nullptr, nullptr, nullptr, nullptr), (hipStream_t)stream);
}
// as splice_optim_step_ema (ema optional) with the one clip record of this gradient: the host-step form of the clipped update
int splice_optim_step_clip(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, long long n, float lr,
                           const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad, float ema_decay, int ema_start,
                           const splice_clip_state* clip, splice_stream_t stream) {
    if (!clip) { splice_set_error("splice_optim_step_clip: needs the clip record"); return SPLICE_ERR_ARG; }
    OptimArgs a = optim_args(kind, params, grads, g2, m, v, n, lr, lr_dev, 0, hp0, hp1, eps, step, zero_grad);
    if (ema) { a.ema = ema; a.ema_decay = ema_decay; a.ema_start = ema_start; }
    a.clip = clip;
    return optim_launch(a, (hipStream_t)stream);
}
int splice_grad_norm_pairs(const float* grads, const float* g2, int n_pairs, long long stride, long long n, float max_norm, float* partials,
                           splice_clip_state* state, const splice_stop_state* stop, const int* step_dev, splice_stream_t stream) {
    return grad_norm_launch(grads, g2, n_pairs, stride < 0 ? 1 : (size_t)stride, n < 1 ? 0 : (size_t)n, max_norm, partials, state, stop, step_dev,
                            (hipStream_t)stream);
}
int splice_grad_norm_pairs_auto(const float* grads, const float* g2, int n_pairs, long long stride, long long n, float max_norm, float k, float beta,
                                int warmup, int regime, float* partials, splice_clip_state* state, splice_clip_auto_state* auto_state,
                                const splice_stop_state* stop, const int* step_dev, splice_stream_t stream) {
    const ClipAutoRule rule = {k, beta, warmup, regime, auto_state};
    return grad_norm_launch(grads, g2, n_pairs, stride < 0 ? 1 : (size_t)stride, n < 1 ? 0 : (size_t)n, max_norm, partials, state, stop, step_dev,
                            (hipStream_t)stream, nullptr, 0, &rule);
}
// as splice_optim_step_pairs_ema (ema optional) with the clip records of splice_grad_norm_pairs; one pair: a single arena of n floats
int splice_optim_step_pairs_clip(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, int n_pairs, long long stride,
                                 long long n, const float* lr_dev, float hp0, float hp1, float eps, const int* step_dev, const splice_stop_state* stop,
                                 int zero_grad, float ema_decay, int ema_start, const splice_clip_state* clip, splice_stream_t stream) {
    if (!params || !grads || !clip || !lr_dev || !step_dev || n_pairs < 1 || n < 1 || (n_pairs > 1 && (stride < n || stride % 4))) {
        splice_set_error("splice_optim_step_pairs_clip: needs the clip records, a device lr table and step count, n_pairs >= 1, n >= 1 and, for more than one pair, n <= stride with stride a multiple of 4");
        return SPLICE_ERR_ARG;
    }
    return optim_launch(pairs_args(kind, params, grads, g2, m, v, n_pairs, n_pairs > 1 ? (size_t)stride : 0, n, lr_dev, hp0, hp1, eps, 0, step_dev, stop, zero_grad, ema,
                                   ema_decay, ema_start, clip, nullptr, nullptr, nullptr), (hipStream_t)stream);
}
// as splice_optim_step_pairs_clip (stop required; clip and ema optional) with the snapshot of the best window's weights
int splice_optim_step_pairs_best(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, int n_pairs, long long stride,
                                 long long n, const float* lr_dev, float hp0, float hp1, float eps, const int* step_dev, const splice_stop_state* stop,
                                 int zero_grad, float ema_decay, int ema_start, const splice_clip_state* clip, const splice_best_state* best,
                                 float* best_params, float* best_ema, splice_stream_t stream) {
    if (!params || !grads || !stop || !best || !best_params || !lr_dev || !step_dev || n_pairs < 1 || n < 1 || (n_pairs > 1 && (stride < n || stride % 4))) {
        splice_set_error("splice_optim_step_pairs_best: needs the stop and best records, the best arena, a device lr table and step count, n_pairs >= 1, n >= 1 and, for more than one pair, n <= stride with stride a multiple of 4");
        return SPLICE_ERR_ARG;
    }
    return optim_launch(pairs_args(kind, params, grads, g2, m, v, n_pairs, n_pairs > 1 ? (size_t)stride : 0, n, lr_dev, hp0, hp1, eps, 0, step_dev, stop, zero_grad, ema,
                                   ema_decay, ema_start, clip, best, best_params, best_ema), (hipStream_t)stream);
}
// the extended rules for one arena: as splice_optim_step_ex with the option record and the third arena w
int splice_optim_step_ext(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* w, long long n, float lr, const float* lr_dev,
                          float hp0, float hp1, float eps, int step, int zero_grad, const splice_optim_ext* options, splice_stream_t stream) {
    if (!options) { splice_set_error("splice_optim_step_ext: needs the option record"); return SPLICE_ERR_ARG; }
    OptimArgs a = optim_args(kind, params, grads, g2, m, v, n, lr, lr_dev, 0, hp0, hp1, eps, step, zero_grad);
    a.w = w; a.ext = options;
    return optim_launch(a, (hipStream_t)stream);
}
// ... and for n_pairs arenas with per-pair lrs: the step count from the device (step_dev) or, step_dev NULL, the host's `step`; stop, ema, clip
// and best (with its arenas) optional, as the fused step composes them
int splice_optim_step_pairs_ext(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* w, float* ema, int n_pairs, long long stride,
                                long long n, const float* lr_dev, float hp0, float hp1, float eps, int step, const int* step_dev, const splice_stop_state* stop,
                                int zero_grad, float ema_decay, int ema_start, const splice_clip_state* clip, const splice_best_state* best, float* best_params,
                                float* best_ema, const splice_optim_ext* options, splice_stream_t stream) {
    if (!options || !params || !grads || !lr_dev || n_pairs < 1 || n < 1 || (n_pairs > 1 && (stride < n || stride % 4))) {
        splice_set_error("splice_optim_step_pairs_ext: needs the option record, a device lr table, n_pairs >= 1, n >= 1 and, for more than one pair, n <= stride with stride a multiple of 4");
        return SPLICE_ERR_ARG;
    }
    OptimArgs a = pairs_args(kind, params, grads, g2, m, v, n_pairs, n_pairs > 1 ? (size_t)stride : 0, n, lr_dev, hp0, hp1, eps, step, step_dev, stop, zero_grad, ema,
                             ema_decay, ema_start, clip, best, best_params, best_ema);
    a.w = w; a.ext = options;
    return optim_launch(a, (hipStream_t)stream);
}
}
