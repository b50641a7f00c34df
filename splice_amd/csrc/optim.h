// The fused optimiser update over a flat arena (optim.hip; torch.optim as util/util.py:28-39 builds them).
#pragma once
#include "common.h"

enum { SPLICE_OPT_ADAM = 0, SPLICE_OPT_RMSPROP = 1, SPLICE_OPT_SGD = 2 };
struct OptimArgs {
    int kind;              // SPLICE_OPT_*
    float *p, *g;
    const float* g2;       // optional: a second gradient arena folded in as g += g2 (g is written back when g2 or zero_grad is set)
    float *m, *v;          // Adam: m and v; RMSprop: v = square_avg; an arena the kind does not use is never touched (may be null)
    size_t n;
    float lr;
    const float* lr_dev;   // optional: the learning rate is read from device memory when the kernel runs (a schedule under graph replay)
    size_t lr_stride;      // != 0 (a multiple of 4): per-pair learning rates, element i of the arena uses lr_dev[i / lr_stride]
    float hp0, hp1, eps;   // Adam: beta1, beta2; RMSprop: alpha
    int step;              // Adam's step count (>= 1); the bias corrections are then computed on the host ...
    const int* step_dev;   // ... unless this is set: the count is read, and they are computed, on the device (graph replay)
    int zero_grad;
    // optional (the plateau stop rule, plateau.h): [slots] records; a slot that is frozen at step *mask_step - 1 is skipped entirely.
    // Element i belongs to slot i / mask_stride (a multiple of 4); mask_stride 0: the one arena is slot 0.
    const splice_stop_state* mask = nullptr;
    const int* mask_step = nullptr;   // device: step index + 1 (the step's Adam count)
    size_t mask_stride = 0;
    // optional (the weight average): an arena laid out like p, written behind p in the same walk.  t = the update's step count (step_dev,
    // else mask_step, else step -- every kind needs one): t <= ema_start: e = p', later e = ema_decay e + (1 - ema_decay) p'
    float* ema = nullptr;
    float ema_decay = 0.f;
    int ema_start = 0;
    // optional (gradient clipping): [slots] records written by grad_norm_launch for this gradient.  Element i uses clip[i / clip_stride]
    // (a multiple of 4; 0: the one arena is slot 0): its gradient is fl(fl(g + g2) * coef), and with skip set the slot is not written
    // (its g is zeroed under zero_grad)
    const splice_clip_state* clip = nullptr;
    size_t clip_stride = 0;
    // optional (keep the best window's weights; needs mask): [slots] records indexed by mask_stride, written by this step's rule.  A slot
    // that is not frozen and whose best_step is the step index *mask_step - 1 has the p just written copied to best_p, and with ema the
    // average just written to best_ema (given exactly when ema is); both are laid out like p
    const splice_best_state* best = nullptr;
    float* best_p = nullptr;
    float* best_ema = nullptr;
    // optional (the extended rules, include/splice_hip.h): the option record selects them -- also when every option is neutral -- and w is
    // the third moment arena, laid out like m and v: Adam's max_exp_avg_sq (amsgrad) or RMSprop's grad_avg (centered); null where the rule
    // keeps none.  m then also holds the momentum buffer of SGD / RMSprop.  Every extended rule needs the update's step count, as ema does
    float* w = nullptr;
    const splice_optim_ext* ext = nullptr;
};
int optim_launch(const OptimArgs& a, hipStream_t s);
// The per-pair gradient norm and clip coefficient (include/splice_hip.h has the rule): two launches, partials[pairs][ceil(n / 4096)] then
// state[pairs].  stop (optional) with step_dev: a frozen pair is left out of both.  trace (optional, with step_dev; the loss trace,
// [capacity][pairs][8]): the second launch also stores norm and coef into words 6 and 7 of row *step_dev - 1 of every pair it writes.
// rule (optional; clipping against the pair's own running norm, include/splice_hip.h): the second launch is its AUTO instance, which also
// keeps records[pairs]; max_norm is then the absolute cap and may be 0 (none).  Without it max_norm must be finite and > 0.
struct ClipAutoRule {
    float k, beta;                     // threshold = k * running norm; the running norm's decay
    int warmup;                        // observations of a regime before its threshold acts
    int regime;                        // of this step: -1, 0 or 1
    splice_clip_auto_state* records;   // device, [pairs]
};
int grad_norm_launch(const float* g, const float* g2, int pairs, size_t stride, size_t n, float max_norm, float* partials, splice_clip_state* state,
                     const splice_stop_state* stop, const int* step_dev, hipStream_t s, float* trace = nullptr, int capacity = 0,
                     const ClipAutoRule* rule = nullptr);
