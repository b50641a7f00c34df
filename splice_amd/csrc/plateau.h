// The plateau stop rule of a slot: window means of the ordinary-step loss, kept and decided on the device.
// One device function, run by thread 0 of a pair's total_loss_kernel workgroup (step_engine.hip) and by splice_plateau_update /
// splice_plateau_update_best.  The plateau lr rule (section 9f) rides on its verdicts: lr_plateau_step, run by the same thread and by
// splice_plateau_update_lr.
#pragma once
#include "common.h"

struct StopRule { int window; float rel; int patience, min_steps; };   // window 0: the rule is off

// frozen at step t: the slot stopped at an earlier step (the update of the stopping step itself still applies)
__device__ __forceinline__ bool stop_frozen(const splice_stop_state* s, int step_idx) {
    const int stop = s->stop_step;
    return stop >= 0 && step_idx > stop;
}

// One counted step of one slot.  fp32, one rounding per operation (no contraction): a NumPy float32 restatement is exact.
// kb / means (keep-best; both null: off): the slot's record and its row of SPLICE_STOP_HISTORY window means, written
// only while the slot is live -- not stopped on entry -- and holding no arithmetic of their own: the step and window index where `best`
// moves, and every closed window's mean.  The state record evolves as it does without them.
// VERDICT (the plateau lr rule, below): *verdict receives the step's outcome -- PLATEAU_OPEN: no window closed, else PLATEAU_BETTER /
// PLATEAU_NOT_BETTER.  Without the flag the function is, statement for statement, what it was before the lr rule.
enum { PLATEAU_OPEN = 0, PLATEAU_BETTER = 1, PLATEAU_NOT_BETTER = 2 };
template <bool VERDICT = false>
__device__ __forceinline__ void plateau_update(splice_stop_state* s, float loss, const StopRule& r, int step_idx, splice_best_state* kb = nullptr,
                                               float* means = nullptr, int* verdict = nullptr) {
#pragma clang fp contract(off)
    const float sum = s->sum + loss;
    const int count = s->count + 1;
    if (count < r.window) {
        s->sum = sum;
        s->count = count;
        if (VERDICT) *verdict = PLATEAU_OPEN;
        return;
    }
    const float mean = sum / (float)r.window;
    const int windows = s->windows;
    const bool live = s->stop_step < 0;
    int bad = s->bad;
    if (windows == 0 || mean < s->best * (1.0f - r.rel)) {
        s->best = mean;
        bad = 0;
        if (VERDICT) *verdict = PLATEAU_BETTER;
        if (kb && live) {
            kb->best_step = step_idx;
            kb->best_window = windows;
        }
    } else {
        ++bad;
        if (VERDICT) *verdict = PLATEAU_NOT_BETTER;
    }
    if (means && live && windows < SPLICE_STOP_HISTORY) means[windows] = mean;
    s->bad = bad;
    s->windows = windows + 1;
    s->sum = 0.f;
    s->count = 0;
    if (bad >= r.patience && step_idx >= r.min_steps && s->stop_step < 0) s->stop_step = step_idx;
}

// The plateau lr rule of a slot (include/splice_hip.h has the rule): factor in (0, 1), patience >= 1 windows,
// min_scale in [0, 1).  factor 0: the rule is off.
struct LrRule { float factor; int patience; float min_scale; };

// One step of one slot, counted or not.  First the step's effective lr, with the scale as it stands BEFORE this step's rule: a cut first
// acts on the next step's update.  Then, on a counted step, the stop rule (its state evolves as without the lr rule); where that closes
// a window of a slot that was live on entry, the lr record takes the verdict.  fp32, one rounding per operation (no contraction).
__device__ __forceinline__ void lr_plateau_step(splice_stop_state* s, splice_lr_state* ls, int* cut_steps, float loss, bool counted, const StopRule& r,
                                                const LrRule& lr, int step_idx, float lr_in, float* lr_eff, splice_best_state* kb = nullptr,
                                                float* means = nullptr) {
#pragma clang fp contract(off)
    *lr_eff = lr_in * ls->scale;
    if (!counted) return;
    const bool live = s->stop_step < 0;
    int verdict;
    plateau_update<true>(s, loss, r, step_idx, kb, means, &verdict);
    if (verdict == PLATEAU_OPEN || !live) return;   // (a frozen slot's record is never written again)
    if (verdict == PLATEAU_BETTER) {
        ls->bad = 0;
        return;
    }
    const int bad = ls->bad + 1, cuts = ls->cuts;
    const float scale = ls->scale;
    if (bad >= lr.patience && scale > lr.min_scale && cuts < SPLICE_STOP_HISTORY) {
        const float cut = scale * lr.factor;
        ls->scale = cut > lr.min_scale ? cut : lr.min_scale;
        cut_steps[cuts] = step_idx;
        ls->cuts = cuts + 1;
        ls->last_cut_step = step_idx;
        ls->bad = 0;
    } else {
        ls->bad = bad;
    }
}
