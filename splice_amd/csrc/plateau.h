// The plateau stop rule of a slot: window means of the ordinary-step loss, kept and decided on the device.
// One device function, run by thread 0 of a pair's total_loss_kernel workgroup (step_engine.hip) and by splice_plateau_update /
// splice_plateau_update_best.
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
__device__ __forceinline__ void plateau_update(splice_stop_state* s, float loss, const StopRule& r, int step_idx, splice_best_state* kb = nullptr,
                                               float* means = nullptr) {
#pragma clang fp contract(off)
    const float sum = s->sum + loss;
    const int count = s->count + 1;
    if (count < r.window) {
        s->sum = sum;
        s->count = count;
        return;
    }
    const float mean = sum / (float)r.window;
    const int windows = s->windows;
    const bool live = s->stop_step < 0;
    int bad = s->bad;
    if (windows == 0 || mean < s->best * (1.0f - r.rel)) {
        s->best = mean;
        bad = 0;
        if (kb && live) {
            kb->best_step = step_idx;
            kb->best_window = windows;
        }
    } else {
        ++bad;
    }
    if (means && live && windows < SPLICE_STOP_HISTORY) means[windows] = mean;
    s->bad = bad;
    s->windows = windows + 1;
    s->sum = 0.f;
    s->count = 0;
    if (bad >= r.patience && step_idx >= r.min_steps && s->stop_step < 0) s->stop_step = step_idx;
}
