// The key second-moment appearance term: for every slot (a crop pair x' / B' of one block's keys, T tokens, D
// features, heads concatenated)
//     G(K) = K^T K / T,    Delta = G(K_x') - G(K_B'),    raw = mean over the D * D entries of Delta^2,    dK_x' = c * K_x' * Delta
// with c = 4 lambda / (T D^2), in THREE launches whatever the number of slots (the slot is a grid dimension):
//   key_gram_loss_kernel, grid (upper-triangular 64 x 64 tiles of D x D, slots): Delta's tile in ONE fp32 accumulator as
//     [K_x ; K_B]^T [K_x ; -K_B], a contraction over 2 T.  Its operands are the token-contiguous transposed key copies [D][tokens] the
//     QKV epilogue writes.  The contraction runs over the T real tokens and nothing else: a 64-token slice is staged through registers,
//     every element whose token index is >= T is replaced by zero there (and a 16-byte chunk that starts at or beyond T is never
//     loaded), so whatever the padding columns hold reaches no bit.  Order, which the bit-level tests pin: slices ascending; inside a
//     slice the two k-steps of the x' operands, then the two of the target's (the B-side negated by its sign bits, exact).  The
//     epilogue scales by 1 / T, writes Delta and (off the diagonal) its mirror tile in bf16 for the backward GEMM, and one partial per
//     tile: the fixed-tree sum of the fp32 Delta^2 of the tile, twice for an off-diagonal tile, times 1 / D^2.
//   key_gram_finish_kernel, one wave per pair: a slot's partials lane-strided ascending, then the wave tree; the pair's crops in crop
//     order.  value[pair] is the raw term.
//   key_gram_dk_kernel, grid (token tiles x feature tiles, slots): dK[rows < T] += c * K_x' * Delta on the 4-stage ring (contraction D,
//     a multiple of 64; Delta is symmetric, so it is its own K-contiguous operand).  It ADDS: it runs behind whatever stored into the
//     buffer (selfsim_dk_kernel, or the zeroing).  Rows >= T are neither read for their value nor written.
// No float atomics, every partial slot written exactly once, every sum in a fixed order, no launch policy that looks at the slot count:
// a slot's bits are those of its own launch.
//
// Over several blocks, and centred: the same three launches with the block a third grid dimension and a by-value
// table of per-block operands (KeyGramLayers), as kernels of their own -- the three above keep their code -- plus, for the centred form
// M(K) = K^T K / T - mu mu^T alone, one launch in front that forms the fp32 means:
//   key_gram_mean_kernel, grid (D / 4, slots, blocks), one wave per feature: the tokens < T of the feature's row of both transposed copies,
//     lane-strided ascending, the wave tree, times the rounded 1 / T.
//   key_gram_layers_loss_kernel<CENTERED>: key_gram_loss_kernel's walk; the centred epilogue forms fl(acc * (1 / T) - m),
//     m = fl(mu_x[i] mu_x[j] - fl(mu_b[i] mu_b[j])), in fp32 (two fused multiply-adds) before the bf16 rounding and the square.
//   key_gram_layers_finish_kernel: per pair, block i's partials as above, times w_i -> values[pair][i]; value[pair] = their sum, ascending.
//   key_gram_layers_dk_kernel<CENTERED>: key_gram_dk_kernel's ring; centred, the workgroup first forms r = Delta mu_x for its 64 columns
//     from the bf16 Delta (four threads per column, a quarter of the row each, added (q0 + q1) + (q2 + q3) through the ring's LDS) and
//     adds c * fl(acc - r[col]).
// Uncentred, block i's delta, partials and dK have the bits of the one-block launch on its operands with its scale.
#include "kernels.h"

constexpr int KG_RING = 4;
constexpr size_t KG_DK_LDS = (size_t)KG_RING * GemmTile<64, 64>::LDS_ELEMS * sizeof(bf16_t);
constexpr int KG_TILE = 64 * GEMM_BK;   // bf16 elements of one staged 64-row operand tile

__device__ __forceinline__ void kg_tri_tile(int t, int nt, int& tm, int& tn) {
    tm = 0;
#pragma unroll 1
    while (t >= nt - tm) { t -= nt - tm; ++tm; }
    tn = tm + t;
}

// The 16-byte chunk of 8 tokens that starts at token k of one feature row, every token >= T replaced by zero; `flip`: the sign bits of the
// eight values (the negated operand).  A chunk that starts at or beyond T is not loaded.
__device__ __forceinline__ u32x4 kg_chunk(const bf16_t* __restrict__ row, int k, int T, uint32_t flip) {
    u32x4 v = {0u, 0u, 0u, 0u};
    const int nv = T - k;   // valid tokens of the chunk
    if (nv > 0) {
        v = *reinterpret_cast<const u32x4*>(row + k);
        if (nv < 8) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const uint32_t keep = (2 * w < nv ? 0x0000FFFFu : 0u) | (2 * w + 1 < nv ? 0xFFFF0000u : 0u);
                v[w] &= keep;
            }
        }
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) v[w] ^= flip;
    return v;
}

__global__ __launch_bounds__(256) void key_gram_loss_kernel(KeyGram a) {
    // one stage: the A (row features) and B (column features) tiles of x', then of the target
    __shared__ __attribute__((aligned(16))) bf16_t smem[4 * KG_TILE];
    __shared__ float red[4];
    const int T = a.T, D = a.D, nt = D / 64, slot = blockIdx.y;
    const int tile_id = blockIdx.x;
    int tm, tn;
    kg_tri_tile(tile_id, nt, tm, tn);
    const int m0 = tm * 64, n0 = tn * 64;
    const bool offdiag = tm != tn;
    const bf16_t* X = a.kT_x + (size_t)slot * a.tx_ps;
    const bf16_t* B = a.kT_b + (size_t)slot * a.tb_ps;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    // a thread stages two chunks of each of the four tiles: LDS row = feature, position p of a row holds source chunk p ^ (row & 7)
    // (the swizzle GemmTile::slice_mfma reads with)
    int srow[2], schunk[2], sdst[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        srow[i] = idx >> 3;
        schunk[i] = (idx & 7) ^ (srow[i] & 7);
        sdst[i] = srow[i] * GEMM_BK + (idx & 7) * 8;
    }
    GemmTile<64, 64> tile;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) tile.acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 r[4][2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = k0 + schunk[i] * 8;
            r[0][i] = kg_chunk(X + (size_t)(m0 + srow[i]) * a.ldt_x, k, T, 0u);
            r[1][i] = kg_chunk(X + (size_t)(n0 + srow[i]) * a.ldt_x, k, T, 0u);
            r[2][i] = kg_chunk(B + (size_t)(m0 + srow[i]) * a.ldt_b, k, T, 0u);
            r[3][i] = kg_chunk(B + (size_t)(n0 + srow[i]) * a.ldt_b, k, T, 0x80008000u);
        }
    };
    const int frow = lane & 15, fchunk = lane >> 4;
    fetch(0);
    for (int k0 = 0; k0 < T; k0 += GEMM_BK) {
        __syncthreads();   // the MFMAs of the slice before are done with the stage
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(smem + q * KG_TILE + sdst[i]) = r[q][i];
        __syncthreads();
        if (k0 + GEMM_BK < T) fetch(k0 + GEMM_BK);   // the next slice's loads fly under this slice's MFMAs
        tile.slice_mfma(smem, smem + KG_TILE, wm, wn, frow, fchunk);
        tile.slice_mfma(smem + 2 * KG_TILE, smem + 3 * KG_TILE, wm, wn, frow, fchunk);
    }
    const float inv_t = 1.0f / (float)T;
    bf16_t* Dl = a.delta + (size_t)slot * D * D;
    float lsum = 0.f;
    tile.for_each(m0, n0, [&](int row0, int col, f32x4 v) {
        float d4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            d4[q] = v[q] * inv_t;
            lsum = __builtin_fmaf(d4[q], d4[q], lsum);
            Dl[(size_t)(row0 + q) * D + col] = f2bf(d4[q]);
        }
        if (offdiag)   // the mirror tile: Delta[col][row0 .. row0 + 3], 8 contiguous bytes
            *reinterpret_cast<uint2*>(Dl + (size_t)col * D + row0) = uint2{pack2bf(d4[0], d4[1]), pack2bf(d4[2], d4[3])};
    });
    lsum = wave_sum(lsum);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    if (tid == 0)
        a.part[(size_t)slot * a.part_ps + tile_id] = ((red[0] + red[1]) + (red[2] + red[3])) * (offdiag ? 2.0f : 1.0f) * (1.0f / ((float)D * (float)D));
}

// ---- the layered instances are kernels of their own: the three kernels above and below keep their code.
// One tile of one slot of the layered loss launch: key_gram_loss_kernel's walk and epilogue, operation for operation.  CENTERED: mu_x / mu_b are the slot's fp32 means ([D] each), and the
// entry becomes fl(acc * (1 / T) - m), m = fl(mu_x[i] mu_x[j] - fl(mu_b[i] mu_b[j])), both fused: one rounding each.
template <bool CENTERED>
__device__ __forceinline__ void kg_loss_tile(const KeyGram& a, const int slot, const int tile_id, const float* __restrict__ mu_x, const float* __restrict__ mu_b) {
    // one stage: the A (row features) and B (column features) tiles of x', then of the target
    __shared__ __attribute__((aligned(16))) bf16_t smem[4 * KG_TILE];
    __shared__ float red[4];
    const int T = a.T, D = a.D, nt = D / 64;
    int tm, tn;
    kg_tri_tile(tile_id, nt, tm, tn);
    const int m0 = tm * 64, n0 = tn * 64;
    const bool offdiag = tm != tn;
    const bf16_t* X = a.kT_x + (size_t)slot * a.tx_ps;
    const bf16_t* B = a.kT_b + (size_t)slot * a.tb_ps;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    // a thread stages two chunks of each of the four tiles: LDS row = feature, position p of a row holds source chunk p ^ (row & 7)
    // (the swizzle GemmTile::slice_mfma reads with)
    int srow[2], schunk[2], sdst[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i;
        srow[i] = idx >> 3;
        schunk[i] = (idx & 7) ^ (srow[i] & 7);
        sdst[i] = srow[i] * GEMM_BK + (idx & 7) * 8;
    }
    GemmTile<64, 64> tile;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) tile.acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 r[4][2];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int k = k0 + schunk[i] * 8;
            r[0][i] = kg_chunk(X + (size_t)(m0 + srow[i]) * a.ldt_x, k, T, 0u);
            r[1][i] = kg_chunk(X + (size_t)(n0 + srow[i]) * a.ldt_x, k, T, 0u);
            r[2][i] = kg_chunk(B + (size_t)(m0 + srow[i]) * a.ldt_b, k, T, 0u);
            r[3][i] = kg_chunk(B + (size_t)(n0 + srow[i]) * a.ldt_b, k, T, 0x80008000u);
        }
    };
    const int frow = lane & 15, fchunk = lane >> 4;
    fetch(0);
    for (int k0 = 0; k0 < T; k0 += GEMM_BK) {
        __syncthreads();   // the MFMAs of the slice before are done with the stage
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int i = 0; i < 2; ++i) *reinterpret_cast<u32x4*>(smem + q * KG_TILE + sdst[i]) = r[q][i];
        __syncthreads();
        if (k0 + GEMM_BK < T) fetch(k0 + GEMM_BK);   // the next slice's loads fly under this slice's MFMAs
        tile.slice_mfma(smem, smem + KG_TILE, wm, wn, frow, fchunk);
        tile.slice_mfma(smem + 2 * KG_TILE, smem + 3 * KG_TILE, wm, wn, frow, fchunk);
    }
    const float inv_t = 1.0f / (float)T;
    bf16_t* Dl = a.delta + (size_t)slot * D * D;
    float lsum = 0.f;
    tile.for_each(m0, n0, [&](int row0, int col, f32x4 v) {
        float d4[4];
        float mxj = 0.f, mbj = 0.f;
        if constexpr (CENTERED) { mxj = mu_x[col]; mbj = mu_b[col]; }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if constexpr (CENTERED) {
                const float pb = mu_b[row0 + q] * mbj;
                const float m = __builtin_fmaf(mu_x[row0 + q], mxj, -pb);
                d4[q] = __builtin_fmaf(v[q], inv_t, -m);
            } else
                d4[q] = v[q] * inv_t;
            lsum = __builtin_fmaf(d4[q], d4[q], lsum);
            Dl[(size_t)(row0 + q) * D + col] = f2bf(d4[q]);
        }
        if (offdiag)   // the mirror tile: Delta[col][row0 .. row0 + 3], 8 contiguous bytes
            *reinterpret_cast<uint2*>(Dl + (size_t)col * D + row0) = uint2{pack2bf(d4[0], d4[1]), pack2bf(d4[2], d4[3])};
    });
    lsum = wave_sum(lsum);
    if (lane == 0) red[wave] = lsum;
    __syncthreads();
    if (tid == 0)
        a.part[(size_t)slot * a.part_ps + tile_id] = ((red[0] + red[1]) + (red[2] + red[3])) * (offdiag ? 2.0f : 1.0f) * (1.0f / ((float)D * (float)D));
}

__global__ __launch_bounds__(64) void key_gram_finish_kernel(const float* __restrict__ part, size_t part_ps, int tiles, int crops, float* __restrict__ value) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    float tot = 0.f;
    for (int i = 0; i < crops; ++i) {
        const float* p = part + ((size_t)pair * crops + i) * part_ps;
        float acc = 0.f;
        for (int j = lane; j < tiles; j += 64) acc += p[j];
        tot += wave_sum(acc);
    }
    if (lane == 0) value[pair] = tot;
}

__global__ __launch_bounds__(256) void key_gram_dk_kernel(KeyGram a) {
    extern __shared__ __attribute__((aligned(16))) bf16_t kg_smem[];
    const int T = a.T, D = a.D, slot = blockIdx.y;
    const int tiles_n = D / 64;
    const int t = xcd_remap(blockIdx.x, gridDim.x);
    const int m0 = (t / tiles_n) * 64, n0 = (t % tiles_n) * 64;
    const bf16_t* K = a.k_x + (size_t)slot * a.k_ps;
    const bf16_t* Dl = a.delta + (size_t)slot * D * D;
    float* dK = a.dk + (size_t)slot * a.dk_ps;
    const float c = a.scale;
    GemmTile<64, 64> tile;
    tile.template run_ring<KG_RING>(K, a.ldk, Dl, D, T, D, D, m0, n0, kg_smem);   // (rows >= T are clamped to row T - 1 and never stored)
    tile.for_each(m0, n0, [&](int row0, int col, f32x4 v) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = row0 + q;
            if (row < T) {
                float* p = dK + (size_t)row * a.lddk + col;
                *p = __builtin_fmaf(c, v[q], *p);
            }
        }
    });
}

// One output tile of one slot of the layered dK launch (key_gram_dk_kernel's ring and epilogue).  CENTERED: r[col] = (delta mu_x)[col] for the tile's 64 columns first, from the bf16 delta
// rows the ring streams anyway (delta is symmetric: row col is column col) -- four threads per column, each a quarter of the row ascending
// by fused multiply-adds, the quarters added as (q0 + q1) + (q2 + q3) through the ring's LDS before the ring starts -- and the epilogue
// adds c * fl(acc - r[col]).
template <bool CENTERED>
__device__ __forceinline__ void kg_dk_tile(const KeyGram& a, const int slot, const int t, const float* __restrict__ mu_x, bf16_t* kg_smem) {
    const int T = a.T, D = a.D;
    const int tiles_n = D / 64;
    const int m0 = (t / tiles_n) * 64, n0 = (t % tiles_n) * 64;
    const bf16_t* K = a.k_x + (size_t)slot * a.k_ps;
    const bf16_t* Dl = a.delta + (size_t)slot * D * D;
    float* dK = a.dk + (size_t)slot * a.dk_ps;
    const float c = a.scale;
    float rj[2] = {0.f, 0.f};
    if constexpr (CENTERED) {
        float* rs = reinterpret_cast<float*>(kg_smem);
        const int tid = threadIdx.x, qd = D / 4, j0 = (tid & 3) * qd;
        const bf16_t* drow = Dl + (size_t)(n0 + (tid >> 2)) * D + j0;
        float acc = 0.f;
        for (int j = 0; j < qd; j += 8) {
            const u32x4 w = *reinterpret_cast<const u32x4*>(drow + j);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc = __builtin_fmaf(__uint_as_float(w[q] << 16), mu_x[j0 + j + 2 * q], acc);
                acc = __builtin_fmaf(__uint_as_float(w[q] & 0xFFFF0000u), mu_x[j0 + j + 2 * q + 1], acc);
            }
        }
        rs[tid] = acc;
        __syncthreads();
        const int lane = tid & 63, wn = (tid >> 6) & 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float* p = rs + 4 * (wn * 32 + j * 16 + (lane & 15));
            rj[j] = (p[0] + p[1]) + (p[2] + p[3]);
        }
        __syncthreads();   // the ring's DMAs write this LDS next
    }
    GemmTile<64, 64> tile;
    static_assert(sizeof(tile.acc) / sizeof(tile.acc[0]) == 2 && sizeof(tile.acc[0]) / sizeof(tile.acc[0][0]) == 2, "rj: two column fragments per wave");
    tile.template run_ring<KG_RING>(K, a.ldk, Dl, D, T, D, D, m0, n0, kg_smem);   // (rows >= T are clamped to row T - 1 and never stored)
    tile.for_each(m0, n0, [&](int row0, int col, f32x4 v) {
        float r = 0.f;
        if constexpr (CENTERED) r = ((col - n0) & 16) ? rj[1] : rj[0];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int row = row0 + q;
            if (row < T) {
                float* p = dK + (size_t)row * a.lddk + col;
                if constexpr (CENTERED) *p = __builtin_fmaf(c, v[q] - r, *p);
                else *p = __builtin_fmaf(c, v[q], *p);
            }
        }
    });
}

// blockIdx.z = entry of the by-value table, blockIdx.y = slot as before
__device__ __forceinline__ KeyGram kg_entry(const KeyGramLayers& t, int i) {
    const KeyGramLayer& e = t.e[i];
    KeyGram a;
    a.kT_x = e.kT_x; a.kT_b = e.kT_b; a.k_x = e.k_x; a.ldt_x = t.ldt_x; a.ldt_b = t.ldt_b; a.ldk = t.ldk; a.tx_ps = t.tx_ps; a.tb_ps = t.tb_ps; a.k_ps = t.k_ps;
    a.T = t.T; a.D = t.D; a.delta = e.delta; a.part = e.part; a.part_ps = t.part_ps; a.value = t.value; a.dk = e.dk; a.lddk = t.lddk; a.dk_ps = t.dk_ps;
    a.scale = e.scale;
    return a;
}
// the fp32 means of entry z, slot y: [2][D], the x' row then the target's
__device__ __forceinline__ float* kg_mu(const KeyGramLayers& t) { return t.mu + ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * 2 * t.D; }

// grid (D / 4, slots, entries), one wave per feature: mu[f] = fl(S * fl(1 / T)), S the sum over the tokens < T of feature f's row of the
// transposed copy -- lane-strided ascending (tokens lane, lane + 64, ...), then the wave tree.  Tokens >= T are not loaded.
__global__ __launch_bounds__(256) void key_gram_mean_kernel(KeyGramLayers t) {
    const KeyGramLayer& e = t.e[blockIdx.z];
    const int slot = blockIdx.y, lane = threadIdx.x & 63, f = blockIdx.x * 4 + (threadIdx.x >> 6), T = t.T;
    const bf16_t* x = e.kT_x + (size_t)slot * t.tx_ps + (size_t)f * t.ldt_x;
    const bf16_t* b = e.kT_b + (size_t)slot * t.tb_ps + (size_t)f * t.ldt_b;
    float sx = 0.f, sb = 0.f;
    for (int k = lane; k < T; k += 64) { sx += bf2f(x[k]); sb += bf2f(b[k]); }
    sx = wave_sum(sx);
    sb = wave_sum(sb);
    if (lane == 0) {
        const float inv_t = 1.0f / (float)T;
        float* mu = kg_mu(t);
        mu[f] = sx * inv_t;
        mu[t.D + f] = sb * inv_t;
    }
}

template <bool CENTERED>
__global__ __launch_bounds__(256) void key_gram_layers_loss_kernel(KeyGramLayers t) {
    const KeyGram a = kg_entry(t, blockIdx.z);
    const float* mu = CENTERED ? kg_mu(t) : nullptr;
    kg_loss_tile<CENTERED>(a, blockIdx.y, blockIdx.x, mu, CENTERED ? mu + t.D : nullptr);
}

// one wave per pair: entry i's partials as key_gram_finish_kernel adds them, times w_i -> values[pair][i]; value[pair] their sum, ascending from 0
__global__ __launch_bounds__(64) void key_gram_layers_finish_kernel(KeyGramLayers t, int tiles, int crops) {
    const int pair = blockIdx.x, lane = threadIdx.x;
    float sum = 0.f;
    for (int l = 0; l < t.n; ++l) {
        const KeyGramLayer& e = t.e[l];
        float tot = 0.f;
        for (int i = 0; i < crops; ++i) {
            const float* p = e.part + ((size_t)pair * crops + i) * t.part_ps;
            float acc = 0.f;
            for (int j = lane; j < tiles; j += 64) acc += p[j];
            tot += wave_sum(acc);
        }
        const float addend = e.weight * tot;
        sum += addend;
        if (lane == 0) t.values[(size_t)pair * t.n + l] = addend;
    }
    if (lane == 0) t.value[pair] = sum;
}

template <bool CENTERED>
__global__ __launch_bounds__(256) void key_gram_layers_dk_kernel(KeyGramLayers t) {
    extern __shared__ __attribute__((aligned(16))) bf16_t kg_smem[];
    const KeyGram a = kg_entry(t, blockIdx.z);
    kg_dk_tile<CENTERED>(a, blockIdx.y, xcd_remap(blockIdx.x, gridDim.x), CENTERED ? kg_mu(t) : nullptr, kg_smem);
}

int key_gram_tiles(int D) {
    if (D < 64 || D % 64) return 0;
    const int nt = D / 64;
    return nt * (nt + 1) / 2;
}

static bool kg_al16(const void* p) { return ((size_t)p & 15) == 0; }
int key_gram_check(const KeyGram& a, int pairs, int crops) {
    if (a.T < 1 || a.D < 64 || a.D % 64 || a.D > 4096 || pairs < 1 || crops < 1 || (size_t)pairs * crops > 65535) return SPLICE_ERR_ARG;
    if (!a.kT_x || !a.kT_b || !a.k_x || !a.delta || !a.part || !a.value || !a.dk) return SPLICE_ERR_ARG;
    if (!kg_al16(a.kT_x) || !kg_al16(a.kT_b) || !kg_al16(a.k_x) || !kg_al16(a.delta)) return SPLICE_ERR_ARG;
    // 16-byte rows and slot strides on the bf16 operands (the chunk loads and the LDS-DMA); a transposed row holds every chunk that starts below T
    const int T8 = (a.T + 7) / 8 * 8;
    if ((a.ldt_x | a.ldt_b | a.ldk) % 8 || (a.tx_ps | a.tb_ps | a.k_ps) % 8) return SPLICE_ERR_ARG;
    if (a.ldt_x < T8 || a.ldt_b < T8 || a.ldk < a.D || a.lddk < a.D) return SPLICE_ERR_ARG;
    if (a.part_ps < (size_t)key_gram_tiles(a.D)) return SPLICE_ERR_ARG;
    if ((size_t)a.T * a.ldk >= (1ull << 31) || (size_t)a.D * a.ldt_x >= (1ull << 31) || (size_t)a.D * a.ldt_b >= (1ull << 31)) return SPLICE_ERR_ARG;   // (32-bit lane offsets)
    return SPLICE_OK;
}

int key_gram_loss_launch(const KeyGram& a, int pairs, int crops, hipStream_t s) {
    if (int rc = key_gram_check(a, pairs, crops)) return rc;
    const int tiles = key_gram_tiles(a.D);
    SPLICE_LAUNCH(key_gram_loss_kernel, dim3(tiles, pairs * crops), dim3(256), 0, s, a);
    SPLICE_LAUNCH(key_gram_finish_kernel, dim3(pairs), dim3(64), 0, s, (const float*)a.part, a.part_ps, tiles, crops, a.value);
    return SPLICE_OK;
}

int key_gram_dk_launch(const KeyGram& a, int pairs, int crops, hipStream_t s) {
    if (int rc = key_gram_check(a, pairs, crops)) return rc;
    SPLICE_LAUNCH(key_gram_dk_kernel, dim3(cdiv(a.T, 64) * (a.D / 64), pairs * crops), dim3(256), KG_DK_LDS, s, a);
    return SPLICE_OK;
}

int key_gram_layers_check(const KeyGramLayers& t, int pairs, int crops) {
    if (t.n < 1 || t.n > KEY_GRAM_MAX_LAYERS || !t.values || !t.value || (t.centered && !t.mu)) return SPLICE_ERR_ARG;
    for (int i = 0; i < t.n; ++i) {
        const KeyGramLayer& e = t.e[i];
        if (!(e.weight > 0.f) || !(e.weight <= 3.402823466e+38f) || !(e.scale == e.scale) || e.scale - e.scale != 0.f) return SPLICE_ERR_ARG;
        KeyGram a = {};
        a.kT_x = e.kT_x; a.kT_b = e.kT_b; a.k_x = e.k_x; a.ldt_x = t.ldt_x; a.ldt_b = t.ldt_b; a.ldk = t.ldk; a.tx_ps = t.tx_ps; a.tb_ps = t.tb_ps; a.k_ps = t.k_ps;
        a.T = t.T; a.D = t.D; a.delta = e.delta; a.part = e.part; a.part_ps = t.part_ps; a.value = t.value; a.dk = e.dk; a.lddk = t.lddk; a.dk_ps = t.dk_ps;
        if (int rc = key_gram_check(a, pairs, crops)) return rc;
        for (int j = 0; j < i; ++j)   // an entry's outputs are its own: two entries on one buffer would race (dk: two read-modify-writes)
            if (t.e[j].dk == e.dk || t.e[j].delta == e.delta || t.e[j].part == e.part) return SPLICE_ERR_ARG;
    }
    return SPLICE_OK;
}

int key_gram_layers_loss_launch(const KeyGramLayers& t, int pairs, int crops, hipStream_t s) {
    if (int rc = key_gram_layers_check(t, pairs, crops)) return rc;
    const int tiles = key_gram_tiles(t.D);
    const dim3 grid(tiles, pairs * crops, t.n);
    if (t.centered) {
        SPLICE_LAUNCH(key_gram_mean_kernel, dim3(t.D / 4, pairs * crops, t.n), dim3(256), 0, s, t);
        SPLICE_LAUNCH(key_gram_layers_loss_kernel<true>, grid, dim3(256), 0, s, t);
    } else
        SPLICE_LAUNCH(key_gram_layers_loss_kernel<false>, grid, dim3(256), 0, s, t);
    SPLICE_LAUNCH(key_gram_layers_finish_kernel, dim3(pairs), dim3(64), 0, s, t, tiles, crops);
    return SPLICE_OK;
}

int key_gram_layers_dk_launch(const KeyGramLayers& t, int pairs, int crops, hipStream_t s) {
    if (int rc = key_gram_layers_check(t, pairs, crops)) return rc;
    const dim3 grid(cdiv(t.T, 64) * (t.D / 64), pairs * crops, t.n);
    if (t.centered) SPLICE_LAUNCH(key_gram_layers_dk_kernel<true>, grid, dim3(256), KG_DK_LDS, s, t);
    else SPLICE_LAUNCH(key_gram_layers_dk_kernel<false>, grid, dim3(256), KG_DK_LDS, s, t);
    return SPLICE_OK;
}
