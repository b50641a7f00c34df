// The nearest-neighbour key appearance term: for every slot (a crop pair x' / B' of one block's keys, T tokens, D
// features, heads concatenated; k_i the rows of x', b_j those of B')
//     c_ij = (k_i . b_j) / max(|k_i| |b_j|, eps),    j*(i) = the LOWEST j among those with the largest c_ij,
//     raw = (1 / T) sum_i (1 - c_i,j*(i)),    dK_i += -(lambda / T) (b_j* / f - [n_i m_j* > eps] c_i,j* k_i / n_i^2),  f = max(n_i m_j*, eps)
// in FOUR launches whatever the number of slots (the slot is a grid dimension):
//   key_nn_norm_kernel, grid (ceil(T / 4), slots, 2), one wave per row: the fp32 norm of a bf16 key row of x' (z = 0) or B' (z = 1) --
//     the squares added by fused multiply-adds lane-strided ascending (features lane, lane + 64, ...), the wave tree, the square root.
//   key_nn_match_kernel, grid (row tiles x column tiles, slots): a 64 x 64 tile of K_x' K_B'^T on the 4-stage ring (the call of
//     selfsim_gemm_kernel with two operands; rows >= T are clamped to row T - 1 by the ring and never used), divided by
//     max(n_i m_j, eps); columns >= T are discarded; every row of the tile is reduced to (its maximum, the lowest column of that
//     maximum): the lane's two fragments ascending, the 16 lanes of a row by four shuffles, the two waves of a row through LDS.  One
//     (float, int) partial per row and column tile; S is never stored.
//   key_nn_row_kernel, grid (ceil(T / 4), slots), one wave per row i < T: the column-tile partials ascending with a strict >, so the
//     lowest index wins; match[i], cos[i]; the gradient row added into dK by two fused multiply-adds per element; one partial of
//     sum (1 - c_i) per workgroup: (r0 + r1) + (r2 + r3) over its four rows (a row >= T adds 0).
//   key_nn_finish_kernel, one wave per pair: a slot's partials lane-strided ascending, then the wave tree; the pair's crops in crop
//     order; times the rounded 1 / T.
// No float atomics, every partial slot written exactly once, every sum in a fixed order, no launch policy that looks at the slot count:
// a slot's bits are those of its own launch.  Rows >= T of either key array are never read for their value; rows >= T of dK are not written.
#include "kernels.h"

constexpr int KNN_RING = 4;
constexpr size_t KNN_LDS = (size_t)KNN_RING * GemmTile<64, 64>::LDS_ELEMS * sizeof(bf16_t);
constexpr int KNN_NONE = 0x7fffffff;   // the index of "no column yet"

// workspace of one call: the norms [2][slots][Tp], then the partial maxima [slots][ct][Tp] and their columns, Tp = round_up(T, 64)
struct KeyNnWs {
    float* norm_x;
    float* norm_b;
    float* pmax;
    int* pidx;
    int Tp, ct;
};
static KeyNnWs key_nn_ws(const KeyNn& a, int slots) {
    KeyNnWs w;
    w.Tp = cdiv(a.T, 64) * 64;
    w.ct = cdiv(a.T, 64);
    float* p = (float*)a.ws;
    w.norm_x = p; p += (size_t)slots * w.Tp;
    w.norm_b = p; p += (size_t)slots * w.Tp;
    w.pmax = p; p += (size_t)slots * w.ct * w.Tp;
    w.pidx = (int*)p;
    return w;
}
size_t key_nn_ws_bytes(int T, int D, int slots) {
    if (T < 1 || D < 1 || slots < 1) return 0;
    const size_t Tp = (size_t)cdiv(T, 64) * 64, ct = (size_t)cdiv(T, 64);
    return (size_t)slots * Tp * (2 + 2 * ct) * sizeof(float);
}

__global__ __launch_bounds__(256) void key_nn_norm_kernel(KeyNn a, KeyNnWs w) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6), slot = blockIdx.y;
    if (row >= a.T) return;
    const bf16_t* k = blockIdx.z ? a.k_b + (size_t)slot * a.kb_ps : a.k_x + (size_t)slot * a.kx_ps;
    k += (size_t)row * a.ldk;
    float sq = 0.f;
    for (int d = lane; d < a.D; d += 64) {
        const float f = bf2f(k[d]);
        sq = __builtin_fmaf(f, f, sq);
    }
    sq = wave_sum(sq);
    if (lane == 0) (blockIdx.z ? w.norm_b : w.norm_x)[(size_t)slot * w.Tp + row] = sqrtf(sq);
}

// (v, j) <- the better of (v, j) and (ov, oj): the larger value, the lower column between equal values
__device__ __forceinline__ void knn_take(float& v, int& j, float ov, int oj) {
    const bool t = ov > v || (ov == v && oj < j);
    v = t ? ov : v;
    j = t ? oj : j;
}

__global__ __launch_bounds__(256) void key_nn_match_kernel(KeyNn a, KeyNnWs w) {
    extern __shared__ __attribute__((aligned(16))) bf16_t knn_smem[];
    const int T = a.T, slot = blockIdx.y, ct = w.ct;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = t / ct, tn = t % ct, m0 = tm * 64, n0 = tn * 64;
    const bf16_t* X = a.k_x + (size_t)slot * a.kx_ps;
    const bf16_t* B = a.k_b + (size_t)slot * a.kb_ps;
    const float* nx = w.norm_x + (size_t)slot * w.Tp;
    const float* nb = w.norm_b + (size_t)slot * w.Tp;
    GemmTile<64, 64> tile;
    tile.template run_ring<KNN_RING>(X, a.ldk, B, a.ldk, T, T, a.D, m0, n0, knn_smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, wm = wave >> 1, wn = wave & 1;
    // the accumulator layout (GemmTile::for_each): fragment (i, j), register q of lane l is C[wm * 32 + i * 16 + (l >> 4) * 4 + q]
    // [wn * 32 + j * 16 + (l & 15)]: a row's 64 columns lie in 2 fragments x 16 lanes x 2 waves
    float nbj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int col = n0 + wn * 32 + j * 16 + (lane & 15);
        nbj[j] = col < T ? nb[col] : 0.f;
    }
    float* redv = reinterpret_cast<float*>(knn_smem);   // [2 wn][64] (the K loop is over)
    int* redi = reinterpret_cast<int*>(knn_smem) + 128;
    __syncthreads();   // the red arrays lie in the ring: every wave is done reading it
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int lrow = wm * 32 + i * 16 + (lane >> 4) * 4 + q, row = m0 + lrow;
            const float ni = row < T ? nx[row] : 0.f;
            float bv = -__builtin_inff();
            int bj = KNN_NONE;
#pragma unroll
            for (int j = 0; j < 2; ++j) {   // (ascending columns: a strict > keeps the lower one)
                const int col = n0 + wn * 32 + j * 16 + (lane & 15);
                if (col < T) {
                    const float c = tile.acc[i][j][q] / fmaxf(ni * nbj[j], a.eps);
                    if (c > bv) { bv = c; bj = col; }
                }
            }
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) knn_take(bv, bj, __shfl_xor(bv, o, 64), __shfl_xor(bj, o, 64));
            if ((lane & 15) == 0) { redv[wn * 64 + lrow] = bv; redi[wn * 64 + lrow] = bj; }
        }
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int row = m0 + threadIdx.x;
        if (row < T) {
            float bv = redv[threadIdx.x];
            int bj = redi[threadIdx.x];
            knn_take(bv, bj, redv[64 + threadIdx.x], redi[64 + threadIdx.x]);
            const size_t o = ((size_t)slot * ct + tn) * w.Tp + row;
            w.pmax[o] = bv;
            w.pidx[o] = bj;
        }
    }
}

__global__ __launch_bounds__(256) void key_nn_row_kernel(KeyNn a, KeyNnWs w) {
    __shared__ float red[4];
    const int T = a.T, D = a.D, slot = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = blockIdx.x * 4 + wave;
    float one_minus = 0.f;
    if (row < T) {
        // every lane walks the partials itself (one address per wave: a broadcast)
        float c = -__builtin_inff();
        int j = 0;
        for (int tn = 0; tn < w.ct; ++tn) {
            const size_t o = ((size_t)slot * w.ct + tn) * w.Tp + row;
            const float v = w.pmax[o];
            const int vj = w.pidx[o];
            if (v > c && vj < T) { c = v; j = vj; }
        }
        if (lane == 0) {
            a.match[(size_t)slot * T + row] = j;
            a.cos[(size_t)slot * T + row] = c;
        }
        one_minus = 1.0f - c;
        const float ni = w.norm_x[(size_t)slot * w.Tp + row], mj = w.norm_b[(size_t)slot * w.Tp + j];
        const float p = ni * mj, f = fmaxf(p, a.eps);
        const float wb = -a.scale / f;
        const float wk = p > a.eps ? (a.scale * c) / (ni * ni) : 0.f;
        const bf16_t* k = a.k_x + (size_t)slot * a.kx_ps + (size_t)row * a.ldk;
        const bf16_t* b = a.k_b + (size_t)slot * a.kb_ps + (size_t)j * a.ldk;
        float* dk = a.dk + (size_t)slot * a.dk_ps + (size_t)row * a.lddk;
        for (int d = lane; d < D; d += 64) dk[d] = __builtin_fmaf(wb, bf2f(b[d]), __builtin_fmaf(wk, bf2f(k[d]), dk[d]));
    }
    if (lane == 0) red[wave] = one_minus;
    __syncthreads();
    if (threadIdx.x == 0) a.part[(size_t)slot * a.part_ps + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void key_nn_finish_kernel(const float* __restrict__ part, size_t part_ps, int n, int crops, float inv_t,
                                                           float* __restrict__ value) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    float tot = 0.f;
    for (int i = 0; i < crops; ++i) {
        const float* p = part + ((size_t)pair * crops + i) * part_ps;
        float acc = 0.f;
        for (int j = lane; j < n; j += 64) acc += p[j];
        tot += wave_sum(acc);
    }
    if (lane == 0) value[pair] = tot * inv_t;
}

int key_nn_parts(int T) { return T < 1 ? 0 : cdiv(T, 4); }

static bool knn_al16(const void* p) { return ((size_t)p & 15) == 0; }
int key_nn_check(const KeyNn& a, int pairs, int crops) {
    if (a.T < 1 || a.D < 64 || a.D % 64 || a.D > 8192 || pairs < 1 || crops < 1 || (size_t)pairs * crops > 65535) return SPLICE_ERR_ARG;
    if (!a.k_x || !a.k_b || !a.match || !a.cos || !a.part || !a.value || !a.dk || !a.ws) return SPLICE_ERR_ARG;
    if (!(a.scale == a.scale) || a.scale - a.scale != 0.f || !(a.eps > 0.f) || a.eps - a.eps != 0.f) return SPLICE_ERR_ARG;   // (finite; eps > 0)
    // 16-byte rows and slot strides on the bf16 operands (the LDS-DMA of the ring)
    if (!knn_al16(a.k_x) || !knn_al16(a.k_b) || a.ldk % 8 || (a.kx_ps | a.kb_ps) % 8 || ((size_t)a.ws & 3)) return SPLICE_ERR_ARG;
    if (a.ldk < a.D || a.lddk < a.D) return SPLICE_ERR_ARG;
    if (a.part_ps < (size_t)key_nn_parts(a.T)) return SPLICE_ERR_ARG;
    if ((size_t)a.T * a.ldk >= (1ull << 31)) return SPLICE_ERR_ARG;   // (32-bit lane offsets)
    return SPLICE_OK;
}

int key_nn_launch(const KeyNn& a, int pairs, int crops, hipStream_t s) {
    if (int rc = key_nn_check(a, pairs, crops)) return rc;
    const int slots = pairs * crops, rt = cdiv(a.T, 64);
    const KeyNnWs w = key_nn_ws(a, slots);
    SPLICE_LAUNCH(key_nn_norm_kernel, dim3(cdiv(a.T, 4), slots, 2), dim3(256), 0, s, a, w);
    SPLICE_LAUNCH(key_nn_match_kernel, dim3(rt * rt, slots), dim3(256), KNN_LDS, s, a, w);
    SPLICE_LAUNCH(key_nn_row_kernel, dim3(cdiv(a.T, 4), slots), dim3(256), 0, s, a, w);
    SPLICE_LAUNCH(key_nn_finish_kernel, dim3(pairs), dim3(64), 0, s, (const float*)a.part, a.part_ps, key_nn_parts(a.T), crops, a.inv_t, a.value);
    return SPLICE_OK;
}
