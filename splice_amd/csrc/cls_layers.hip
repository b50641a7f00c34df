// The [CLS] appearance term over several ViT blocks: for every slot (a pair, or a pair-crop)
//   raw = sum over the named blocks l, ascending, of w_l * mean((cls_l(generated) - cls_l(target))^2),   cls_l = row 0 of block l's output, D floats
// in ONE launch per term: a workgroup of 256 threads per slot walks the layers of a by-value table (ClsLayers, kernels.h) in ascending
// order.  Per layer, thread t takes columns t, t + 256, ... in that order, the 256 sums meet in the wave tree (wave_sum) and the four
// waves' results are added pairwise -- no float atomics, and nothing of a slot's arithmetic depends on the batch it rides in.  Thread 0
// then forms each layer's addend v_l = S_l * (w_l / D), stores it for splice_step_cls_layer_values, and writes their ascending fp32 sum into
// slot 0 of the slot's term row: the total-loss kernel's wave sum of one value and zeros is that value, so the reported word is exactly the
// float32 sum of the reported addends.  The gradient leaves as one seed row per layer and pass, 2 (g w_l) d, which the ViT backward adds
// into row 0 of its gradient stream in front of the block (splice_vit_ctx_set_cls_seeds) -- or, for the top block, through the row of
// d_block the plain path writes.
#include "kernels.h"

__global__ __launch_bounds__(256) void cls_layers_kernel(ClsLayers tab, float g, const float* __restrict__ gtab, float* __restrict__ part, size_t part_ps,
                                                         float* __restrict__ values, size_t values_ps) {
    const int slot = blockIdx.x;
    if (gtab) {   // per-slot gradient weight; a slot whose weight is 0 does not take part
        g = gtab[slot];
        if (g == 0.f) return;
    }
    __shared__ float red[CLS_MAX_LAYERS][4];
    const int D = tab.D;
    for (int i = 0; i < tab.n; ++i) {
        const ClsLayer& e = tab.e[i];
        const float* x = e.x + (size_t)slot * tab.x_ps;
        const float* t = e.tgt + (size_t)slot * tab.t_ps;
        float* seed = e.seed + (size_t)slot * tab.seed_step * e.seed_ps;
        const float gm = g * e.weight;
        float acc = 0.f;
        for (int c = threadIdx.x; c < D; c += 256) {
            const float d = x[c] - t[c];
            acc = __builtin_fmaf(d, d, acc);
            seed[c] = 2.0f * gm * d;
        }
        acc = wave_sum(acc);
        if ((threadIdx.x & 63) == 0) red[i][threadIdx.x >> 6] = acc;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        // (no contraction here: the sum adds the ROUNDED products it has just stored, not fma(S, w / D, tot) -- the identity with the reported values)
#pragma clang fp contract(off)
        float tot = 0.f;
        for (int i = 0; i < tab.n; ++i) {
            const float v = ((red[i][0] + red[i][1]) + (red[i][2] + red[i][3])) * (tab.e[i].weight / (float)D);
            values[(size_t)slot * values_ps + i] = v;
            tot += v;
        }
        part[(size_t)slot * part_ps] = tot;
    }
}

int cls_layers_launch(const ClsLayers& tab, int slots, float g, const float* grad_tab, float* part, size_t part_ps, float* values,
                      size_t values_ps, hipStream_t s) {
    if (tab.n < 1 || tab.n > CLS_MAX_LAYERS || tab.D < 1 || slots < 1 || !part || !values || values_ps < (size_t)tab.n || tab.seed_step < 1) return SPLICE_ERR_ARG;
    for (int i = 0; i < tab.n; ++i) {
        const ClsLayer& e = tab.e[i];
        if (!e.x || !e.tgt || !e.seed || e.seed_ps < (size_t)tab.D || !(e.weight > 0.f) || !(e.weight <= 3.402823466e+38f)) return SPLICE_ERR_ARG;
    }
    SPLICE_LAUNCH(cls_layers_kernel, dim3(slots), dim3(256), 0, s, tab, g, grad_tab, part, part_ps, values, values_ps);
    return SPLICE_OK;
}
