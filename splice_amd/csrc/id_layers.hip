// The key-identity term over several ViT blocks: for every slot (a B crop)
//   raw = sum over the named blocks l, ascending, of w_l * mean((k_l(G(B_crop)) - k_l(B_crop))^2),   k_l = the T x D fp32 keys of block l
// in TWO launches per step, whatever the number of blocks.
//   id_layers_kernel, grid (G, slots, layers), 256 threads: a (slot, layer)'s T * D / 4 float4s are walked grid-stride by its G workgroups --
//     item i of thread t of workgroup b is float4 number (b + k G) * 256 + t, k ascending.  Per float4 the four d = x - tgt enter the thread's
//     sum as fma(d, d, acc) in column order and leave as the gradient 2 (g w_l) d, one 16-byte store into the block's key-gradient rows.  The
//     256 sums meet in the wave tree (wave_sum), the four waves' results pairwise: the workgroup's partial goes to the term's own scratch,
//     [slots][layers][G].  No float atomics; G follows from T * D alone, so nothing of a slot's arithmetic depends on the batch it rides in.
//   id_layers_finish_kernel, one wave per slot: lane i adds layer i's G partials in index order, forms the addend v_i = S_i * (w_i / (T D)) and
//     stores it for splice_step_id_layer_values; lane 0 writes their ascending fp32 sum into slot 0 of the slot's term row.  The total-loss
//     kernel's wave sum of one value and zeros is that value, so the reported word is exactly the float32 sum of the reported addends.
// The two launches never wait on each other inside a kernel: the second is ordered behind the first by the stream (or the graph edge).
#include "kernels.h"

__global__ __launch_bounds__(256) void id_layers_kernel(IdLayers tab, float g, const float* __restrict__ gtab, float* __restrict__ scratch) {
    const int slot = blockIdx.y, layer = blockIdx.z;
    if (gtab) {   // per-slot gradient weight; a slot whose weight is 0 does not take part
        g = gtab[slot];
        if (g == 0.f) return;
    }
    const IdLayer& e = tab.e[layer];
    const float* x = e.x + (size_t)slot * tab.x_rs * e.ldx;
    const float* t = e.tgt + (size_t)slot * tab.t_rs * e.ldt;
    float* gr = e.grad + (size_t)slot * tab.g_rs * e.ldg;
    const float gm2 = 2.0f * (g * e.weight);
    const unsigned d4 = (unsigned)tab.D >> 2, n4 = (unsigned)tab.T * d4;
    float acc = 0.f;
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < n4; i += gridDim.x * 256u) {
        const unsigned r = i / d4, c = (i - r * d4) << 2;
        const float4 a = *reinterpret_cast<const float4*>(x + (size_t)r * e.ldx + c);
        const float4 b = *reinterpret_cast<const float4*>(t + (size_t)r * e.ldt + c);
        const float4 d = {a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w};
        acc = __builtin_fmaf(d.x, d.x, acc);
        acc = __builtin_fmaf(d.y, d.y, acc);
        acc = __builtin_fmaf(d.z, d.z, acc);
        acc = __builtin_fmaf(d.w, d.w, acc);
        *reinterpret_cast<float4*>(gr + (size_t)r * e.ldg + c) = float4{gm2 * d.x, gm2 * d.y, gm2 * d.z, gm2 * d.w};
    }
    __shared__ float red[4];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) scratch[((size_t)slot * tab.n + layer) * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void id_layers_finish_kernel(IdLayers tab, int G, const float* __restrict__ gtab, const float* __restrict__ scratch,
                                                              float* __restrict__ values, size_t values_ps, float* __restrict__ part, size_t part_ps) {
    // (no contraction: the sum adds the ROUNDED products it has just stored -- the identity with the reported values)
#pragma clang fp contract(off)
    const int slot = blockIdx.x, lane = threadIdx.x;
    if (gtab && gtab[slot] == 0.f) return;
    __shared__ float v[ID_MAX_LAYERS];
    if (lane < tab.n) {
        const float* p = scratch + ((size_t)slot * tab.n + lane) * G;
        float S = 0.f;
        for (int b = 0; b < G; ++b) S += p[b];
        float w = 0.f;   // (a uniform walk of the by-value table: a lane-indexed read would spill it to private memory)
        for (int i = 0; i < tab.n; ++i)
            if (lane == i) w = tab.e[i].weight;
        const float vi = S * (w / (float)((size_t)tab.T * tab.D));
        values[(size_t)slot * values_ps + lane] = vi;
        v[lane] = vi;
    }
    __syncthreads();
    if (lane == 0) {
        float tot = 0.f;
        for (int i = 0; i < tab.n; ++i) tot += v[i];
        part[(size_t)slot * part_ps] = tot;
    }
}

int id_layers_wg(int T, int D, int max_wg) {
    if (T < 1 || D < 4 || max_wg < 0) return 0;
    const size_t need = ((size_t)T * (D >> 2) + 255) / 256;
    const size_t cap = max_wg ? (size_t)max_wg : (size_t)ID_MAX_WG;
    return (int)(need < cap ? need : cap);
}

static bool al16(const void* p) { return ((size_t)p & 15) == 0; }
static int id_layers_check(const IdLayers& tab, int slots, int max_wg) {
    if (tab.n < 1 || tab.n > ID_MAX_LAYERS || tab.T < 1 || tab.D < 4 || (tab.D & 3) || slots < 1 || slots > 65535 || max_wg < 0) return SPLICE_ERR_ARG;
    if ((size_t)tab.T * tab.D >= (1ull << 31)) return SPLICE_ERR_ARG;
    for (int i = 0; i < tab.n; ++i) {
        const IdLayer& e = tab.e[i];
        if (!e.x || !e.tgt || !e.grad || !al16(e.x) || !al16(e.tgt) || !al16(e.grad)) return SPLICE_ERR_ARG;
        if (e.ldx < tab.D || e.ldt < tab.D || e.ldg < tab.D || ((e.ldx | e.ldt | e.ldg) & 3)) return SPLICE_ERR_ARG;
        if (!(e.weight > 0.f) || !(e.weight <= 3.402823466e+38f)) return SPLICE_ERR_ARG;
    }
    return SPLICE_OK;
}

int id_layers_launch(const IdLayers& tab, int slots, float g, const float* grad_tab, float* scratch, int max_wg, hipStream_t s) {
    if (!scratch) return SPLICE_ERR_ARG;
    if (int rc = id_layers_check(tab, slots, max_wg)) return rc;
    const int G = id_layers_wg(tab.T, tab.D, max_wg);
    SPLICE_LAUNCH(id_layers_kernel, dim3(G, slots, tab.n), dim3(256), 0, s, tab, g, grad_tab, scratch);
    return SPLICE_OK;
}

int id_layers_finish_launch(const IdLayers& tab, int slots, const float* grad_tab, const float* scratch, int max_wg, float* values,
                            size_t values_ps, float* part, size_t part_ps, hipStream_t s) {
    if (!scratch || !values || !part || values_ps < (size_t)tab.n) return SPLICE_ERR_ARG;
    if (int rc = id_layers_check(tab, slots, max_wg)) return rc;
    const int G = id_layers_wg(tab.T, tab.D, max_wg);
    SPLICE_LAUNCH(id_layers_finish_kernel, dim3(slots), dim3(64), 0, s, tab, G, grad_tab, scratch, values, values_ps, part, part_ps);
    return SPLICE_OK;
}
