// Weight gradients of the generator's convolutions (see gen_conv.hip for the family overview): batched and 3x3-tile partial kernels,
// and the one deterministic reduction of every layer's partials per backward.
#include "gen_device.h"
#include <cstdlib>

// ---------------------------------------------------------------------------------------
// Weight gradient: dW[n][c][tap] = sum_{img,pixel} dy[n][pixel] * x[c][tap-shifted pixel].
// Workgroup = (pixel chunk, 4-or-16-channel K tile); MFMA reduces over pixels (64 per LDS fill, the next
// fill prefetched into registers); the partial tile goes to ws[chunk][n][c][tap] and ONE
// wgrad_reduce_all_kernel per backward sums every layer's chunks in a fixed order (bit-reproducible).
constexpr int WG_PC = 64;                      // pixels per LDS fill
constexpr int WG_LD = WG_PC + 2;               // 66 = 2*33
constexpr int WG_XS_FLOATS = 3 * 16 * WG_LD;   // [k][pixel], largest variant (3x3: 36 -> 48 k rows)
constexpr int WG_DS_FLOATS = 8 * 16 * WG_LD;   // [n][pixel], largest variant (128 output channels)
// ROWS (5x5 / 7x7 filters): a K tile is 4 channels x ONE filter row (KS taps), ktile = channel_tile * KS + ky -- keeps the
// tile at 20 / 28 k-values instead of 100 / 196.
template <int KS, int NI, bool ROWS = false>   // NI = 16-row fragments of output channels
__device__ __forceinline__ void conv_wgrad_body(const WgradArgs& a, int chunk, int ktile_in, float* Xs, float* Ds) {
    constexpr int T = ROWS ? KS : KS * KS;     // taps per channel inside one K tile
    constexpr int CK = (ROWS || KS == 3) ? 4 : 16;
    constexpr int KT = CK * T;                 // 36 / 16 / 20 / 28
    const int ktile = ROWS ? ktile_in / KS : ktile_in;
    const int krow = ROWS ? ktile_in % KS : 0;
    constexpr int NJ = (KT + 15) / 16;         // 3 / 1
    constexpr int PC = WG_PC;
    constexpr int LD = WG_LD;
    constexpr int NQ = (NI * NJ + 3) / 4;      // fragment pairs per wave
    constexpr int NA = KT / 4;                 // gathered x elements per thread per fill
    constexpr int ND = NI * 16 * PC / 256;     // dy elements per thread per fill
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = ktile * CK;
    const int HWo = a.Ho * a.Wo;
    const int chunks_per_img = a.chunks_per_img;
    const int img = chunk / chunks_per_img, ch_in_img = chunk % chunks_per_img;
    const float* x = a.x + (size_t)img * a.x_nstride + (size_t)c0 * a.x_cstride;
    const float* dy = a.dy + (size_t)img * a.dy_nstride;
    f32x4 acc[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int e = tid; e < (NJ * 16 - KT) * LD; e += 256) Xs[KT * LD + e] = 0.f;   // k-padding rows stay zero
    const int pl = tid & 63;
    const int p_begin = ch_in_img * a.pix_per_chunk;
    const int p_end = min(p_begin + a.pix_per_chunk, HWo);
    // per-thread gather descriptors (k = wave + 4*i is wave-uniform): channel + tap displacement
    // The 3x3 body of 128 output channels is the variant that peaks: one VGPR over the 256 of two waves per SIMD, which made the big class the
    // generator's only scratch user (every wave of every launch paid the scratch set-up).  Its descriptors are formed from the wave index as
    // a scalar, so they live in SGPRs: 27 VGPRs less, same values.  The other variants keep their instruction stream.
    const int wave_g = (KS == 3 && NI == 8) ? __builtin_amdgcn_readfirstlane(wave) : wave;
    int g_coff[NA], g_dy[NA], g_dx[NA];
    unsigned g_cok = 0;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int k = wave_g + 4 * i;
        const int cl = k / T, tap = k % T;
        g_coff[i] = (int)(cl * a.x_cstride);
        g_dy[i] = (ROWS ? krow : tap / KS) - a.pad;
        g_dx[i] = (ROWS ? tap : tap % KS) - a.pad;
        if (c0 + cl < a.Cin) g_cok |= 1u << i;
    }
    float xv[NA], dv[ND];
    // raw buffer loads (see conv_igemm_body): an element outside the image / the channel range / the chunk gets an offset with bit 31
    // set and reads as 0 -- no exec-masked block per element.  The output-gradient offsets of a thread are fixed, the fill enters as
    // the scalar offset.
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, 0x7FFFFFFF, 0x00020000);
    int d_vo[ND];
#pragma unroll
    for (int t = 0; t < ND; ++t) {
        const int e = tid + 256 * t;
        const int n = e / PC, q = e % PC;
        d_vo[t] = n < a.Cout ? (int)((n * a.dy_cstride + q) * 4) : (int)0x80000000;
    }
    auto fetch = [&](int pb) {
        const int p = pb + pl;
        const bool pvalid = p < p_end;
        const int oy = pvalid ? p / a.Wo : 0, ox = pvalid ? p % a.Wo : 0;
        const int by = oy * a.stride, bx = ox * a.stride;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            int sy = by + g_dy[i], sx = bx + g_dx[i];
            if (a.reflect) {
                sy = sy < 0 ? -sy : (sy >= a.Hi ? 2 * (a.Hi - 1) - sy : sy);
                sx = sx < 0 ? -sx : (sx >= a.Wi ? 2 * (a.Wi - 1) - sx : sx);
            }
            const bool ok = pvalid && ((g_cok >> i) & 1u) && (unsigned)sy < (unsigned)a.Hi && (unsigned)sx < (unsigned)a.Wi;
            const int vo = ok ? (g_coff[i] + sy * a.Wi + sx) * 4 : (int)0x80000000;
            xv[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, vo, 0, 0));
        }
        if (pb + PC <= p_end) {   // a full fill: fixed per-thread offsets + the fill as the scalar offset
            const int so = __builtin_amdgcn_readfirstlane(pb * 4);
#pragma unroll
            for (int t = 0; t < ND; ++t) dv[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rdy, d_vo[t], so, 0));
        } else {
#pragma unroll
            for (int t = 0; t < ND; ++t) {
                const int e = tid + 256 * t;
                const int n = e / PC, q = e % PC;
                const int pp = pb + q;
                dv[t] = (n < a.Cout && pp < p_end) ? dy[(size_t)n * a.dy_cstride + pp] : 0.f;
            }
        }
    };
    fetch(p_begin);
    // fragment reads in batches of WB pixel steps, the next batch in flight under this one's MFMAs (round 5, as in conv_igemm_body: the compiler's
    // order was read -> wait -> MFMA per step); one LDS base per operand + compile-time offsets, re-defined per fill so that they are not hoisted
    // into a register each.  Same operands, same order, same bits.
    constexpr int WB = 4, NB = PC / 4 / WB;
    [[maybe_unused]] int lds_rd = (lane & 15) * LD + (lane >> 4);
    for (int pb = p_begin; pb < p_end; pb += PC) {
        if constexpr (NI < 4) asm volatile("" : "+v"(lds_rd));
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NA; ++i) Xs[(wave + 4 * i) * LD + pl] = xv[i];
#pragma unroll
        for (int t = 0; t < ND; ++t) {
            const int e = tid + 256 * t;
            Ds[(e / PC) * LD + (e % PC)] = dv[t];
        }
        __syncthreads();
        if (pb + PC < p_end) fetch(pb + PC);
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            const int pair = wave + 4 * q;
            if (pair < NI * NJ) {
                const int fi = pair / NJ, fj = pair % NJ;
                if constexpr (NI >= 4) {   // the 64- and 128-channel bodies sit at the 2-waves-per-SIMD register limit: they keep the plain order
#pragma unroll
                    for (int s4 = 0; s4 < PC / 4; ++s4) {
                        const float av = Ds[(fi * 16 + (lane & 15)) * LD + s4 * 4 + (lane >> 4)];
                        const float bv = Xs[(fj * 16 + (lane & 15)) * LD + s4 * 4 + (lane >> 4)];
                        acc[q] = mfma4(av, bv, acc[q]);
                    }
                } else {
                    const int d_rd = lds_rd + fi * 16 * LD, x_rd = lds_rd + fj * 16 * LD;
                    float af[2][WB], bf[2][WB];
#pragma unroll
                    for (int t = 0; t < WB; ++t) { af[0][t] = Ds[d_rd + t * 4]; bf[0][t] = Xs[x_rd + t * 4]; }
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        if (b + 1 < NB) {
#pragma unroll
                            for (int t = 0; t < WB; ++t) { af[(b + 1) & 1][t] = Ds[d_rd + ((b + 1) * WB + t) * 4]; bf[(b + 1) & 1][t] = Xs[x_rd + ((b + 1) * WB + t) * 4]; }
                        }
                        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                        for (int t = 0; t < WB; ++t) acc[q] = mfma4(af[b & 1][t], bf[b & 1][t], acc[q]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
        }
    }
    // partial[chunk][n][c][tap]: layout identical to the weight tensor
    constexpr int TT = KS * KS;   // taps of the full filter (the layout of the partial = the weight tensor's)
    float* ws = a.ws + (size_t)chunk * a.Cout * a.Cin * TT;
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const int pair = wave + 4 * q;
        if (pair < NI * NJ) {
            const int fi = pair / NJ, fj = pair % NJ;
            const int k = fj * 16 + (lane & 15);
            const int cl = k / T, tap = k % T;
            if (k < KT && c0 + cl < a.Cin) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int n = fi * 16 + (lane >> 4) * 4 + r;
                    if (n < a.Cout) ws[((size_t)n * a.Cin + c0 + cl) * TT + (ROWS ? krow * KS + tap : tap)] = acc[q][r];
                }
            }
        }
    }
}

// dw[layer][i] (+)= sum_chunk ws[layer][chunk][i] for every conv layer of a backward in one launch
// n_img > 1 with p_nstride > 0: independent images -- blockIdx.y = image, which sums only ITS chunks (chunk index = image *
// chunks_per_image + k) into its own gradient arena
// one chain of a layer's chunk sum: 4 independent partial sums in a FIXED association order.  The loads of a group go out before its first
// add, so a walk costs one memory round trip per group: the 224 x 224 layers have 98 chunks and a few hundred weights -- a few dozen
// threads whose dependent trips ARE the kernel's duration -- hence groups of 32 first (98 chunks: 3 groups + 2 single loads)
// a loaded value as the register it arrives in, behind every load issued so far: the adds of a group cannot be scheduled in between its
// loads (left alone the compiler keeps a window of 8 loads in flight, whatever the source order says)
__device__ __forceinline__ void wgrad_loaded(float& x) { asm volatile("" : "+v"(x) : : "memory"); }
template <class Load>
__device__ __forceinline__ float wgrad_chunk_sum(int chunks, Load&& ld) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int c = 0;
#pragma unroll 1
    for (; c + 31 < chunks; c += 32) {
        float v[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) v[u] = ld(c + u);
#pragma unroll
        for (int u = 0; u < 32; ++u) wgrad_loaded(v[u]);
#pragma unroll
        for (int u = 0; u < 32; u += 4) { s0 += v[u]; s1 += v[u + 1]; s2 += v[u + 2]; s3 += v[u + 3]; }
    }
    for (; c + 15 < chunks; c += 16) {   // 16 loads in flight, added in the order of the 4-wide loop below (same bits)
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = ld(c + u);
#pragma unroll
        for (int u = 0; u < 16; u += 4) { s0 += v[u]; s1 += v[u + 1]; s2 += v[u + 2]; s3 += v[u + 3]; }
    }
    for (; c + 3 < chunks; c += 4) {
        s0 += ld(c);
        s1 += ld(c + 1);
        s2 += ld(c + 2);
        s3 += ld(c + 3);
    }
    for (; c < chunks; ++c) s0 += ld(c);
    return (s0 + s1) + (s2 + s3);   // chunks == 0: an exact-zero gradient range (BN-fed conv bias)
}
__global__ __launch_bounds__(256) void wgrad_reduce_all_kernel(WgradReduceAll d, const float* __restrict__ ws, float* __restrict__ grads,
                                                               int accumulate, int n_img, size_t p_nstride) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    // The layer table is read ONCE per wave -- lane j fetches the entries of layer j (count <= 64, the wave) -- and the search for a thread's
    // layer runs on registers.  Walking prefix[] in the kernel arguments was one dependent scalar-memory round trip per layer, on lines no
    // launch has touched before: ~50 of them in the workgroups of the last layers, most of the kernel's 21 us.
    static_assert(WGRAD_MAX_LAYERS <= 64, "one lane per layer");
    const int lj = min((int)(threadIdx.x & 63), d.count - 1);
    const long long hi_j = d.prefix[lj + 1], lo_j = d.prefix[lj], wso_j = d.ws_off[lj], dwo_j = d.dw_off[lj];
    const int n_j = d.n[lj], chunks_j = d.chunks[lj], vec_j = d.vec[lj];
    int l = 0;
    for (int k = 0; k + 1 < d.count; ++k) {   // = while (l + 1 < count && gid >= prefix[l + 1]) ++l: the prefix sums do not decrease
        const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)hi_j, k);
        const int hi = __builtin_amdgcn_readlane((int)(hi_j >> 32), k);
        l += gid >= (long long)(((unsigned long long)(unsigned)hi << 32) | lo) ? 1 : 0;
    }
    const long long first = __shfl(lo_j, l), ws_off = __shfl(wso_j, l), dw_off = __shfl(dwo_j, l);
    const int n = __shfl(n_j, l);
    int chunks = __shfl(chunks_j, l);
    const bool vec = __shfl(vec_j, l) != 0;
    if (gid >= d.total) return;   // (behind the lane exchange: every lane holds a layer)
    const int i = (int)(gid - first) * (vec ? 4 : 1);
    const float* p = ws + ws_off + i;
    if (p_nstride) {
        chunks /= n_img;
        p += (size_t)blockIdx.y * chunks * n;
        grads += (size_t)blockIdx.y * p_nstride;
    }
    float* q = grads + dw_off + i;
    if (vec) {
        // four neighbouring elements per thread through 16-byte loads (round 4: the reduction streams 15 MB of partials per image and
        // was latency-bound on 4-byte accesses); every element still sums its chunks in the order of the scalar path: same bits
        float4 s = {0.f, 0.f, 0.f, 0.f};
        float4 a0 = s, a1 = s, a2 = s, a3 = s;
        int c = 0;
#pragma unroll 1
        for (; c + 31 < chunks; c += 32) {   // (32 x 16 B in flight: the long walks of the 224 x 224 layers, see wgrad_chunk_sum)
            float4 v[32];
#pragma unroll
            for (int u = 0; u < 32; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(c + u) * n);
#pragma unroll
            for (int u = 0; u < 32; ++u) { wgrad_loaded(v[u].x); wgrad_loaded(v[u].y); wgrad_loaded(v[u].z); wgrad_loaded(v[u].w); }
#pragma unroll
            for (int u = 0; u < 32; u += 4) {
                a0.x += v[u].x; a0.y += v[u].y; a0.z += v[u].z; a0.w += v[u].w;
                a1.x += v[u + 1].x; a1.y += v[u + 1].y; a1.z += v[u + 1].z; a1.w += v[u + 1].w;
                a2.x += v[u + 2].x; a2.y += v[u + 2].y; a2.z += v[u + 2].z; a2.w += v[u + 2].w;
                a3.x += v[u + 3].x; a3.y += v[u + 3].y; a3.z += v[u + 3].z; a3.w += v[u + 3].w;
            }
        }
        for (; c + 7 < chunks; c += 8) {   // (8 x 16 B in flight; chains by c mod 4 as in wgrad_chunk_sum)
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = *reinterpret_cast<const float4*>(p + (size_t)(c + u) * n);
#pragma unroll
            for (int u = 0; u < 8; u += 4) {
                a0.x += v[u].x; a0.y += v[u].y; a0.z += v[u].z; a0.w += v[u].w;
                a1.x += v[u + 1].x; a1.y += v[u + 1].y; a1.z += v[u + 1].z; a1.w += v[u + 1].w;
                a2.x += v[u + 2].x; a2.y += v[u + 2].y; a2.z += v[u + 2].z; a2.w += v[u + 2].w;
                a3.x += v[u + 3].x; a3.y += v[u + 3].y; a3.z += v[u + 3].z; a3.w += v[u + 3].w;
            }
        }
        for (; c + 3 < chunks; c += 4) {
            const float4 v0 = *reinterpret_cast<const float4*>(p + (size_t)c * n), v1 = *reinterpret_cast<const float4*>(p + (size_t)(c + 1) * n),
                         v2 = *reinterpret_cast<const float4*>(p + (size_t)(c + 2) * n), v3 = *reinterpret_cast<const float4*>(p + (size_t)(c + 3) * n);
            a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
            a1.x += v1.x; a1.y += v1.y; a1.z += v1.z; a1.w += v1.w;
            a2.x += v2.x; a2.y += v2.y; a2.z += v2.z; a2.w += v2.w;
            a3.x += v3.x; a3.y += v3.y; a3.z += v3.z; a3.w += v3.w;
        }
        for (; c < chunks; ++c) {
            const float4 v0 = *reinterpret_cast<const float4*>(p + (size_t)c * n);
            a0.x += v0.x; a0.y += v0.y; a0.z += v0.z; a0.w += v0.w;
        }
        s.x = (a0.x + a1.x) + (a2.x + a3.x); s.y = (a0.y + a1.y) + (a2.y + a3.y);
        s.z = (a0.z + a1.z) + (a2.z + a3.z); s.w = (a0.w + a1.w) + (a2.w + a3.w);
        float4* q4 = reinterpret_cast<float4*>(q);
        if (accumulate) { const float4 o = *q4; s.x = o.x + s.x; s.y = o.y + s.y; s.z = o.z + s.z; s.w = o.w + s.w; }
        *q4 = s;
        return;
    }
    const float s = wgrad_chunk_sum(chunks, [&](int c) { return p[(size_t)c * n]; });
    *q = accumulate ? *q + s : s;
}

int wgrad_chunks(int N, int Ho, int Wo, int* pix_per_chunk, int* chunks_per_img) {
    const int HWo = Ho * Wo;
    // tuned in-step with alternating runs (512 / 256 / 64; 1024 or 256 for the big planes and 128 or 512 for the middle ones lose 0.2-0.4 %)
    int ppc = 512;
    if (HWo <= 1024) ppc = 256;
    if (HWo <= 256) ppc = 64;
    // big planes (round 5: the reference's default 900 x 900 crops): at 512 pixels a plane of 0.81 MP made 1582 chunks, every one writing a full
    // weight-shaped partial -- 0.84 ms of wgrad_reduce_all per step just to stream them back.  At most 128 chunks per image: a workgroup walks
    // more 64-pixel fills before it writes (planes up to 256 x 256 keep their 512-pixel chunks, so the 224 x 224 configs keep their bits).
    if (HWo > 128 * 512) ppc = (cdiv(HWo, 128) + 63) / 64 * 64;
    *pix_per_chunk = ppc;
    *chunks_per_img = cdiv(HWo, ppc);
    return N * *chunks_per_img;
}

// Every conv layer's weight gradient of a backward in ONE launch: the layers are independent of each other (each needs
// only its own input and output gradient, all in place once the dgrad chain has finished), so instead of ~30 small
// serial kernels the workgroups of all layers fill the chip together.  Workgroup -> (layer, pixel chunk, channel tile)
// through the prefix table of the by-value descriptor array; the (filter size, output-channel fragments) variant is a
// workgroup-uniform switch.
// Two instantiations: BIG = false runs the layers with <= 32 output channels (1 or 2 fragments: ~60 VGPRs, 21 KB of LDS,
// several workgroups per CU -- these are the layers with thousands of workgroups), BIG = true the 64 / 128-channel ones
// (up to 229 VGPRs).  One kernel for everything ran the small layers at the big variant's occupancy.
template <bool BIG>
__global__ __launch_bounds__(256, 2) void conv_wgrad_batched_kernel(WgradBatch b) {
    __shared__ float Xs[WG_XS_FLOATS];
    __shared__ float Ds[(BIG ? 8 : 2) * 16 * WG_LD];
    int l = 0;
#pragma unroll 1
    while (l + 1 < b.count && blockIdx.x >= b.d[l + 1].wg_begin) ++l;
    const WgradDesc& d = b.d[l];
    WgradArgs a;
    a.x = d.x; a.dy = d.dy; a.ws = d.ws;
    a.x_nstride = d.x_nstride; a.x_cstride = d.x_cstride; a.dy_nstride = d.dy_nstride; a.dy_cstride = d.dy_cstride;
    a.N = 0; a.Cin = d.Cin; a.Hi = d.Hi; a.Wi = d.Wi; a.Cout = d.Cout; a.Ho = d.Ho; a.Wo = d.Wo;
    a.ks = d.ks; a.stride = d.stride; a.pad = d.pad; a.pix_per_chunk = d.pix_per_chunk; a.chunks_per_img = d.chunks_per_img;
    a.reflect = (int)d.reflect;
    const int local = blockIdx.x - d.wg_begin;
    const int chunk = local % d.chunks, ktile = local / d.chunks;
    if (BIG) {
        switch (d.variant) {
            case 2: conv_wgrad_body<1, 4>(a, chunk, ktile, Xs, Ds); break;
            case 3: conv_wgrad_body<1, 8>(a, chunk, ktile, Xs, Ds); break;
            case 6: conv_wgrad_body<3, 4>(a, chunk, ktile, Xs, Ds); break;
            case 7: conv_wgrad_body<3, 8>(a, chunk, ktile, Xs, Ds); break;
            case 10: conv_wgrad_body<5, 4, true>(a, chunk, ktile, Xs, Ds); break;
            case 11: conv_wgrad_body<5, 8, true>(a, chunk, ktile, Xs, Ds); break;
            case 14: conv_wgrad_body<7, 4, true>(a, chunk, ktile, Xs, Ds); break;
            default: conv_wgrad_body<7, 8, true>(a, chunk, ktile, Xs, Ds); break;
        }
    } else {
        switch (d.variant) {
            case 0: conv_wgrad_body<1, 1>(a, chunk, ktile, Xs, Ds); break;
            case 1: conv_wgrad_body<1, 2>(a, chunk, ktile, Xs, Ds); break;
            case 4: conv_wgrad_body<3, 1>(a, chunk, ktile, Xs, Ds); break;
            case 5: conv_wgrad_body<3, 2>(a, chunk, ktile, Xs, Ds); break;
            case 8: conv_wgrad_body<5, 1, true>(a, chunk, ktile, Xs, Ds); break;
            case 9: conv_wgrad_body<5, 2, true>(a, chunk, ktile, Xs, Ds); break;
            case 12: conv_wgrad_body<7, 1, true>(a, chunk, ktile, Xs, Ds); break;
            default: conv_wgrad_body<7, 2, true>(a, chunk, ktile, Xs, Ds); break;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Weight gradient of the 3x3 stride-1 layers of BIG planes (round 5), the counterpart of conv3x3_tile_kernel: a workgroup = (strip of 4 x 64-pixel tiles,
// 8-channel K tile).  Per tile the (4 + 2) x (64 + 2) x 8 input patch is staged in LDS once (interior tiles: fixed per-thread offsets + the tile as the
// scalar offset; border tiles resolve padding / reflection per element); a wave owns one pixel row, takes its output-gradient operand STRAIGHT from
// global memory (16-byte loads: lane (n, g) holds dy[n][16 q + 4 g .. + 3], four MFMA steps per load) and its input operand from the patch at
// [per-lane (channel, tap) offset + 4 g] + [compile-time pixel offset]; the 72 (channel, tap) columns are 5 fragments, the accumulators stay in registers
// over the whole strip, the four waves' sums are added in wave order through LDS at the end.  conv_wgrad_body fills LDS with 64 pixels x 36 k-values and
// 64 x Cout gradients for 16 MFMA steps per fragment pair (and leaves one wave idle at 16 output channels).
constexpr int WT_CK = 8, WT_NJ = 5, WT_PH = 6, WT_PLANE = WT_PH * CT_PW, WT_PE = WT_CK * WT_PLANE, WT_NP = (WT_PE + 255) / 256;
template <int NI>
__device__ __forceinline__ void conv_wgrad_tile_body(const WgradDesc& d, int chunk, int ktile, int nb /* first output channel of this workgroup */, float* Ps) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Cin = d.Cin, Cout = d.Cout, Hi = d.Hi, Wi = d.Wi, Ho = d.Ho, Wo = d.Wo, pad = d.pad;
    const int img = chunk / d.chunks_per_img, strip = chunk % d.chunks_per_img;
    const int tiles_x = (Wo + CT_TW - 1) / CT_TW, tiles_y = (Ho + 3) / 4, T = tiles_x * tiles_y;
    const int t_begin = (int)((long long)strip * T / d.chunks_per_img), t_end = (int)((long long)(strip + 1) * T / d.chunks_per_img);
    const int c0 = ktile * WT_CK;
    const float* x = d.x + (size_t)img * d.x_nstride + (size_t)c0 * d.x_cstride;
    const float* dy = d.dy + (size_t)img * d.dy_nstride;
    const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(x), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rdy = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dy), 0, 0x7FFFFFFF, 0x00020000);
    // patch element e = tid + 256 j = (channel, patch row, patch column), relative to the tile's patch origin
    int p_rel[WT_NP];
#pragma unroll
    for (int j = 0; j < WT_NP; ++j) {
        const int e = tid + 256 * j;
        const int c = e / WT_PLANE, rem = e % WT_PLANE, r = rem / CT_PW, xx = rem % CT_PW;
        p_rel[j] = (e < WT_PE && c0 + c < Cin) ? (int)(c * d.x_cstride + (unsigned)(r * Wi + xx)) * 4 : (int)0x80000000;
    }
    // input operand: column j = jf * 16 + (lane & 15) = (channel, tap) -> offset inside the patch (+ this wave's row, + the lane's pixel group)
    int b_base[WT_NJ];
#pragma unroll
    for (int jf = 0; jf < WT_NJ; ++jf) {
        const int j = jf * 16 + (lane & 15);
        const int cl = j / 9, tap = j % 9;
        b_base[jf] = (j < WT_CK * 9 ? cl * WT_PLANE + (tap / 3) * CT_PW + tap % 3 : 0) + wave * CT_PW + 4 * (lane >> 4);
    }
    int dy_off[NI];
#pragma unroll
    for (int fi = 0; fi < NI; ++fi) {
        const int n = nb + fi * 16 + (lane & 15);
        dy_off[fi] = n < Cout ? (int)(n * d.dy_cstride) * 4 : (int)0x80000000;
    }
    f32x4 acc[NI][WT_NJ];
#pragma unroll
    for (int fi = 0; fi < NI; ++fi)
#pragma unroll
        for (int jf = 0; jf < WT_NJ; ++jf) acc[fi][jf] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pv[WT_NP];
    float dyn[NI][4][4], dyc[NI][4][4];
    auto fetch = [&](int t) __attribute__((always_inline)) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y0 = ty * 4, x0 = tx * CT_TW, sy0 = y0 - pad, sx0 = x0 - pad;
        const bool interior = sy0 >= 0 && sx0 >= 0 && sy0 + WT_PH <= Hi && sx0 + CT_PW <= Wi;
        if (interior) {
            const int so = __builtin_amdgcn_readfirstlane((sy0 * Wi + sx0) * 4);
#pragma unroll
            for (int j = 0; j < WT_NP; ++j) pv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, p_rel[j], so, 0));
        } else {
#pragma unroll
            for (int j = 0; j < WT_NP; ++j) {
                const int e = tid + 256 * j;
                const int c = e / WT_PLANE, rem = e % WT_PLANE, r = rem / CT_PW, xx = rem % CT_PW;
                int sy = sy0 + r, sx = sx0 + xx;
                if (d.reflect) {
                    sy = sy < 0 ? -sy : (sy >= Hi ? 2 * (Hi - 1) - sy : sy);
                    sx = sx < 0 ? -sx : (sx >= Wi ? 2 * (Wi - 1) - sx : sx);
                }
                const bool ok = p_rel[j] >= 0 && sy >= 0 && sy < Hi && sx >= 0 && sx < Wi;
                pv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rx, ok ? (int)(c * d.x_cstride + (unsigned)(sy * Wi + sx)) * 4 : (int)0x80000000, 0, 0));
            }
        }
        // this wave's row of the output gradient: 16-byte runs (4-byte aligned); pixels behind the row end / rows behind the plane read as 0
        const int row = y0 + wave;
        const int col0 = x0 + 4 * (lane >> 4);
#pragma unroll
        for (int fi = 0; fi < NI; ++fi)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int col = col0 + 16 * q;
                const bool ok = row < Ho && col < Wo && dy_off[fi] >= 0;
                const u32x4 v = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rdy, ok ? dy_off[fi] + (row * Wo + col) * 4 : (int)0x80000000, 0, 0));
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) dyn[fi][q][tt] = col + tt < Wo ? __uint_as_float(v[tt]) : 0.f;
            }
    };
    if (t_begin < t_end) fetch(t_begin);
    for (int t = t_begin; t < t_end; ++t) {
        asm volatile("" : "+v"(b_base[0]), "+v"(b_base[1]), "+v"(b_base[2]), "+v"(b_base[3]), "+v"(b_base[4]));   // (LDS bases re-defined per trip: base + instruction offset)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < WT_NP; ++j)
            if (tid + 256 * j < WT_PE) Ps[tid + 256 * j] = pv[j];
#pragma unroll
        for (int fi = 0; fi < NI; ++fi)
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) dyc[fi][q][tt] = dyn[fi][q][tt];
        __syncthreads();
        if (t + 1 < t_end) fetch(t + 1);
        float bv[2][WT_NJ];
#pragma unroll
        for (int jf = 0; jf < WT_NJ; ++jf) bv[0][jf] = Ps[b_base[jf]];
#pragma unroll
        for (int st = 0; st < 16; ++st) {   // pixel step: column 16 (st / 4) + 4 g + st % 4 of the wave's row
            if (st + 1 < 16) {
#pragma unroll
                for (int jf = 0; jf < WT_NJ; ++jf) bv[(st + 1) & 1][jf] = Ps[b_base[jf] + 16 * ((st + 1) >> 2) + ((st + 1) & 3)];
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int fi = 0; fi < NI; ++fi)
#pragma unroll
                for (int jf = 0; jf < WT_NJ; ++jf) acc[fi][jf] = mfma4(dyc[fi][st >> 2][st & 3], bv[st & 1][jf], acc[fi][jf]);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---- the four waves' sums, added in wave order (fixed: bit-reproducible), then the partial of this (chunk, K tile): layout of the weight tensor
    __syncthreads();
    constexpr int NV = NI * WT_NJ * 4;
    if (wave > 0) {
#pragma unroll
        for (int fi = 0; fi < NI; ++fi)
#pragma unroll
            for (int jf = 0; jf < WT_NJ; ++jf)
#pragma unroll
                for (int r = 0; r < 4; ++r) Ps[((wave - 1) * NV + (fi * WT_NJ + jf) * 4 + r) * 64 + lane] = acc[fi][jf][r];
    }
    __syncthreads();
    if (wave > 0) return;
    float* ws = d.ws + (size_t)chunk * Cout * Cin * 9;
#pragma unroll
    for (int fi = 0; fi < NI; ++fi)
#pragma unroll
        for (int jf = 0; jf < WT_NJ; ++jf) {
            const int j = jf * 16 + (lane & 15);
            const int cl = j / 9, tap = j % 9;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v = acc[fi][jf][r];
#pragma unroll
                for (int w = 0; w < 3; ++w) v += Ps[(w * NV + (fi * WT_NJ + jf) * 4 + r) * 64 + lane];
                const int n = nb + fi * 16 + (lane >> 4) * 4 + r;
                if (j < WT_CK * 9 && c0 + cl < Cin && n < Cout) ws[((size_t)n * Cin + c0 + cl) * 9 + tap] = v;
            }
        }
}
constexpr int WT_LDS_FLOATS = 3 * 2 * WT_NJ * 4 * 64 > WT_PE ? 3 * 2 * WT_NJ * 4 * 64 : WT_PE;
__global__ __launch_bounds__(256) void conv_wgrad_tile_kernel(WgradBatch b) {
    __shared__ float Ps[WT_LDS_FLOATS];
    int l = 0;
#pragma unroll 1
    while (l + 1 < b.count && blockIdx.x >= b.d[l + 1].wg_begin) ++l;
    const WgradDesc& d = b.d[l];
    const int local = blockIdx.x - d.wg_begin;
    // (chunk, K tile, block of 32 output channels): layers with 64 / 128 output channels are 2 / 4 passes over the same patches
    const int chunk = local % d.chunks, kt_all = local / d.chunks, ktiles_c = (d.Cin + WT_CK - 1) / WT_CK;
    const int ktile = kt_all % ktiles_c, nb = (kt_all / ktiles_c) * 32;
    if (d.variant == 1) conv_wgrad_tile_body<1>(d, chunk, ktile, nb, Ps);
    else conv_wgrad_tile_body<2>(d, chunk, ktile, nb, Ps);
}
static bool wgrad_tile_ok(const WgradArgs& a) {
    static const int on = getenv("SPLICE_WGRAD_TILE") ? atoi(getenv("SPLICE_WGRAD_TILE")) : 1;
    constexpr int min_px = 40000;
    return on && a.ks == 3 && a.stride == 1 && a.Wo >= 64 && (long long)a.Ho * a.Wo > min_px && a.Hi == a.Ho && a.Wi == a.Wo && a.pad == 1 &&
           (size_t)a.Cin * a.x_cstride <= 0x1fffffffULL && (size_t)a.Cout * a.dy_cstride <= 0x1fffffffULL;   // (32-bit byte offsets)
}

// append one layer to a batch (partial sums only: ws gets chunks * Cout*Cin*ks*ks floats); returns the number of chunks
int conv_wgrad_add(WgradBatchPair* pair, WgradArgs a, int* chunks_out) {
    const bool tile = wgrad_tile_ok(a);
    WgradBatch* b = tile ? &pair->tile : a.Cout > 32 ? &pair->big : &pair->small;
    if (a.Cout > 128 || (a.ks != 1 && a.ks != 3 && a.ks != 5 && a.ks != 7) || b->count >= WGRAD_BATCH_MAX) return SPLICE_ERR_ARG;
    if ((size_t)a.Cin * a.x_cstride > 0x7fffffffULL || a.x_nstride > 0xffffffffULL || a.dy_nstride > 0xffffffffULL) return SPLICE_ERR_ARG;
    if (a.Hi > 65535 || a.Wi > 65535 || a.Cin > 65535) return SPLICE_ERR_ARG;
    const int chunks = wgrad_chunks(a.N, a.Ho, a.Wo, &a.pix_per_chunk, &a.chunks_per_img);
    const int CK = tile ? WT_CK : a.ks == 1 ? 16 : 4;
    const int ktiles = cdiv(a.Cin, CK) * (a.ks >= 5 ? a.ks : 1) * (tile ? cdiv(a.Cout, 32) : 1);   // 5x5 / 7x7: one K tile per (channel tile, filter row); tile kernel: x blocks of 32 output channels
    const int ni = cdiv(a.Cout, 16);
    WgradDesc& d = b->d[b->count++];
    d.x = a.x; d.dy = a.dy; d.ws = a.ws;
    d.x_nstride = (uint32_t)a.x_nstride; d.x_cstride = (uint32_t)a.x_cstride; d.dy_nstride = (uint32_t)a.dy_nstride; d.dy_cstride = (uint32_t)a.dy_cstride;
    d.Cin = (uint16_t)a.Cin; d.Cout = (uint16_t)a.Cout; d.Hi = (uint16_t)a.Hi; d.Wi = (uint16_t)a.Wi; d.Ho = (uint16_t)a.Ho; d.Wo = (uint16_t)a.Wo;
    d.ks = (uint8_t)a.ks; d.stride = (uint8_t)a.stride; d.pad = (uint8_t)a.pad;
    d.variant = (uint8_t)((a.ks == 3 ? 4 : a.ks == 5 ? 8 : a.ks == 7 ? 12 : 0) + (ni <= 1 ? 0 : ni <= 2 ? 1 : ni <= 4 ? 2 : 3));
    if (tile) d.variant = (uint8_t)(ni < 2 ? 1 : 2);   // 1 or 2 fragments of output channels per workgroup
    d.reflect = (uint32_t)(a.reflect ? 1 : 0);
    d.pix_per_chunk = (uint16_t)a.pix_per_chunk; d.chunks_per_img = (uint16_t)a.chunks_per_img;
    d.wg_begin = (uint32_t)b->total_wgs; d.chunks = (uint32_t)chunks;
    b->total_wgs += chunks * ktiles;
    if (chunks_out) *chunks_out = chunks;
    return SPLICE_OK;
}
int conv_wgrad_batched_launch(const WgradBatchPair& p, hipStream_t s) {
    if (p.big.count > 0) SPLICE_LAUNCH(conv_wgrad_batched_kernel<true>, dim3((unsigned)p.big.total_wgs), dim3(256), 0, s, p.big);
    if (p.small.count > 0) SPLICE_LAUNCH(conv_wgrad_batched_kernel<false>, dim3((unsigned)p.small.total_wgs), dim3(256), 0, s, p.small);
    if (p.tile.count > 0) SPLICE_LAUNCH(conv_wgrad_tile_kernel, dim3((unsigned)p.tile.total_wgs), dim3(256), 0, s, p.tile);
    return SPLICE_OK;
}

int wgrad_reduce_all_launch(const WgradReduceAll& d0, const float* ws, float* grads, int accumulate, hipStream_t s, int n_img, size_t p_nstride) {
    if (d0.count < 1 || d0.count > WGRAD_MAX_LAYERS) return SPLICE_ERR_ARG;
    // work items: four elements per thread wherever a layer's ranges are 16-byte aligned (every layer but the 3-channel head's bias)
    WgradReduceAll d = d0;
    static const int vec_on = getenv("SPLICE_WGRAD_REDUCE_VEC") ? atoi(getenv("SPLICE_WGRAD_REDUCE_VEC")) : 1;
    const bool base_ok = vec_on && !((reinterpret_cast<size_t>(ws) | reinterpret_cast<size_t>(grads)) & 15) && p_nstride % 4 == 0;
    d.prefix[0] = 0;
    for (int i = 0; i < d.count; ++i) {
        const bool v = base_ok && d.n[i] % 4 == 0 && d.ws_off[i] % 4 == 0 && d.dw_off[i] % 4 == 0;
        d.vec[i] = v ? 1 : 0;
        d.prefix[i + 1] = d.prefix[i] + (v ? d.n[i] / 4 : d.n[i]);
    }
    d.total = d.prefix[d.count];
    SPLICE_LAUNCH(wgrad_reduce_all_kernel, dim3((unsigned)((d.total + 255) / 256), p_nstride ? n_img : 1), dim3(256), 0, s, d, ws, grads, accumulate,
                       n_img, p_nstride);
    return SPLICE_OK;
}
