// The plateau stop rule of a slot: window means of the ordinary-step loss, kept and decided on the device.
// One device function, run by thread 0 of a pair's total_loss_kernel workgroup (step_engine.hip) and by splice_plateau_update.
#pragma once
#include "common.h"

struct StopRule { int window; float rel; int patience, min_steps; };   // window 0: the rule is off

// frozen at step t: the slot stopped at an earlier step (the update of the stopping step itself still applies)
__device__ __forceinline__ bool stop_frozen(const splice_stop_state* s, int step_idx) {
    const int stop = s->stop_step;
    return stop >= 0 && step_idx > stop;
}

// One counted step of one slot.  fp32, one rounding per operation (no contraction): a NumPy float32 restatement is exact.
__device__ __forceinline__ void plateau_update(splice_stop_state* s, float loss, const StopRule& r, int step_idx) {
#pragma clang fp contract(off)
    const float sum = s->sum + loss;
    const int count = s->count + 1;
    if (count < r.window) {
        s->sum = sum;
        s->count = count;
        return;
    }
    const float mean = sum / (float)r.window;
    int bad = s->bad;
    if (s->windows == 0 || mean < s->best * (1.0f - r.rel)) {
        s->best = mean;
        bad = 0;
    } else {
        ++bad;
    }
    s->bad = bad;
    s->windows += 1;
    s->sum = 0.f;
    s->count = 0;
    if (bad >= r.patience && step_idx >= r.min_steps && s->stop_step < 0) s->stop_step = step_idx;
}
