// Kernels of the skip-U-Net generator (K13-K18 of SURVEY.md; models/unet/skip.py:42-102,
// models/unet/common.py:11-124): fp32 NCHW, convolutions as implicit GEMM on the exact-f32
// matrix cores (v_mfma_f32_16x16x4_f32: bit-equal to an fmaf chain, so generator parity with
// the fp32 oracle is rounding-order only), train-mode BatchNorm with per-instance statistics
// (the reference calls netG once per image with batch 1), LeakyReLU(0.2), bilinear x2
// up-sampling written straight into the concat buffer, sigmoid head.  Every reduction runs
// in a fixed order (no float atomics): replicas are bit-reproducible.
//
// This unit: the convolutions (implicit GEMM forward / data gradient, pair kernel, 3x3 tile kernel, split-K reduce, reflect fold)
// and their launch policies.  gen_wgrad.hip: weight gradients; gen_bn.hip: BatchNorm; gen_pointwise.hip: upsampling, sigmoid head.
#include "gen_device.h"
#ifndef CONV_KB
#define CONV_KB 6   // k steps per LDS fragment batch of conv_igemm_body at one output-channel fragment per workgroup (0: the whole tile at once); 3 at 2 or 4 fragments
#endif
#include <cstdlib>

// ---------------------------------------------------------------------------------------
// Implicit-GEMM convolution.  M = output pixels of one image (64 per workgroup),
// N = output channels (16*FN per workgroup), K = (channel, ky, kx) in the weight's own
// memory order, consumed CK channels at a time.  TRANSPOSED = data-gradient form:
// out[c][iy][ix] = sum_{n,ky,kx} in[n][oy][ox] w[n][c][ky][kx] with oy*stride + ky - pad = iy.
// The gather offsets of a thread do not depend on the channel tile, so they are computed once;
// the next tile's operands are fetched into registers while the current one feeds the MFMAs.
// NG = 2: an 8-wave workgroup -- the second wave group takes the other half of every K tile's MFMA steps (and half of
// the gather), its accumulators are added through LDS at the end.  For the layers with at most ~2 workgroups per CU the
// run time is the serial K walk of one workgroup (fp32 MFMA: 32 cycles per 16x16x4 step), and this halves it.
template <int KS, int FN, int CK>
struct ConvTile {   // LDS geometry of one instantiation (shared by the kernel wrappers that carve the LDS)
    static constexpr int T = KS * KS, KT = CK * T, BM = 64;
    static constexpr int LDA = KS == 7 ? BM + 1 : BM + 16;   // 80: k-rows 16 banks apart -> conflict-free ds_read_b32 (7x7: 65, the 196-row tile must fit 64 KB)
    static constexpr int LDW = KT + 2;                        // 2*odd -> conflict-free
    static constexpr int A_FLOATS = KT * LDA, W_FLOATS = 16 * FN * LDW;
};
// bx / by / bz: the block coordinates of a launch of this convolution alone (m tile, n tile * ksplit + slice, image); As / Ws:
// ConvTile<..>::A_FLOATS / W_FLOATS floats of LDS.  Called from conv_igemm_kernel (one convolution per launch) and from
// conv_pair_kernel (two independent convolutions -- e.g. the 1x1 skip branch and the 3x3 stride-2 encoder convolution of one
// scale, which read the same input -- sharing one launch: a launch less on a latency-bound chain).
// offset of image img's parameter arena: its own (p_nstride > 0), its group's (p_group > 1 images per arena) or the one arena
__device__ __forceinline__ size_t conv_arena(const ConvArgs& a, int img) { return (size_t)(a.p_group > 1 ? img / a.p_group : img) * a.p_nstride; }
template <int KS, bool TRANSPOSED, int FN, int CK, int NG>
__device__ __forceinline__ void conv_igemm_body(const ConvArgs& a, int bx, int by, int bz, float* As, float* Ws) {
    constexpr int T = KS * KS;
    constexpr int KT = CK * T;          // k extent of one LDS tile (multiple of 4)
    constexpr int BM = 64;
    constexpr int LDA = ConvTile<KS, FN, CK>::LDA;
    constexpr int LDW = ConvTile<KS, FN, CK>::LDW;
    constexpr int BN = 16 * FN;
    constexpr int NTH = 256 * NG;
    constexpr int NWV = 4 * NG;                     // waves
    constexpr int NA = KT / NWV;                    // gathered elements per thread per tile
    constexpr int NW = (BN * KT + NTH - 1) / NTH;   // weight elements per thread per tile
    constexpr int KSTEPS = KT / 4 / NG;             // MFMA k steps per wave group per tile
    static_assert(KT % (4 * NG) == 0 && ((LDW / 2) & 1) == 1, "tile shape");
    static_assert(NG == 1 || KT * LDA >= FN * 4 * 256, "accumulator exchange reuses the A tile");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (scalar: what depends only on it stays out of the VGPRs)
    const int pw = wave & 3, grp = wave >> 2;       // pixel fragment / wave group
    const int img = bz;
    const int m0 = bx * BM;
    const int HWo = a.Ho * a.Wo;
    const float* in = a.in + (size_t)img * a.in_nstride;
    // independent images (several pairs optimised side by side): image n convolves with ITS OWN parameter arena (grouped
    // images: the arena of its group)
    const float* wgt = a.w + conv_arena(a, img);
    const float* bias = a.bias ? a.bias + conv_arena(a, img) : nullptr;
    const int pl = tid & 63;
    const int p = m0 + pl;
    const bool pvalid = p < HWo;
    const int oy = pvalid ? p / a.Wo : 0, ox = pvalid ? p % a.Wo : 0;
    // split-K: blockIdx.y = n_tile * ksplit + slice; each slice reduces its own channel range and writes a raw
    // partial tile that conv_splitk_reduce_kernel sums in slice order (tiny deep layers: few tiles, long reductions)
    const int ksplit = a.ksplit > 1 ? a.ksplit : 1;
    const int kslice = by % ksplit;
    const int n0 = (by / ksplit) * BN;
    const int cper = ((a.Cin + ksplit - 1) / ksplit + CK - 1) / CK * CK;
    const int cbeg = kslice * cper;
    const int Kc = min(a.Cin, cbeg + cper);  // reduction channels [cbeg, Kc)
    // ---- per-thread gather descriptors (k = wave + NWV*i is wave-uniform)
    int a_off[NA], a_cl[NA];
    unsigned long long a_ok = 0;   // (7x7: 49 gathered elements per thread)
    static_assert(NA <= 64, "gather mask");
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int k = wave + NWV * i;
        const int cl = k / T, tap = k % T;
        const int ky = tap / KS, kx = tap % KS;
        int sy, sx;
        bool ok;
        if (!TRANSPOSED) {
            sy = oy * a.stride + ky - a.pad;
            sx = ox * a.stride + kx - a.pad;
            if (a.reflect) {   // nn.ReflectionPad2d in front of the convolution (models/unet/common.py:113-118): mirror without the edge
                sy = sy < 0 ? -sy : (sy >= a.Hi ? 2 * (a.Hi - 1) - sy : sy);
                sx = sx < 0 ? -sx : (sx >= a.Wi ? 2 * (a.Wi - 1) - sx : sx);
            }
            ok = sy >= 0 && sy < a.Hi && sx >= 0 && sx < a.Wi;
        } else {
            const int ty = oy + a.pad - ky, tx = ox + a.pad - kx;
            ok = ty >= 0 && tx >= 0;
            if (a.stride == 2) {
                ok = ok && !(ty & 1) && !(tx & 1);
                sy = ty >> 1; sx = tx >> 1;
            } else {
                sy = ty; sx = tx;
            }
            ok = ok && sy < a.Hi && sx < a.Wi;
        }
        ok = ok && pvalid;
        a_cl[i] = cl;
        a_off[i] = ok ? (int)(cl * a.in_cstride) + sy * a.Wi + sx : 0;
        if (ok) a_ok |= 1ull << i;
    }
    static_assert(NW <= 64, "weight mask");
    int w_off[NW], w_cl[NW], w_lds[NW];
    unsigned long long w_ok = 0;
#pragma unroll
    for (int t = 0; t < NW; ++t) {
        const int e = tid + NTH * t;
        const int j = e / KT, k = e % KT;
        const int cl = k / T, tap = k % T;
        const bool ok = e < BN * KT && (n0 + j) < a.Cout;
        w_cl[t] = cl;
        w_off[t] = ok ? (int)((size_t)(n0 + j) * a.w_jstride + (size_t)cl * a.w_cstride + tap) : 0;
        w_lds[t] = e < BN * KT ? j * LDW + k : -1;
        if (ok) w_ok |= 1ull << t;
    }
    float av[NA], wv[NW];
    // Full channel tiles are fetched with RAW BUFFER loads: a thread's byte offsets are fixed for the whole kernel (an element that is
    // padding / out of the image / out of the output-channel range carries bit 31 = out of the descriptor's range, and the hardware
    // returns 0 for it), the channel tile enters as the SCALAR offset -- no predicate, no branch, no address arithmetic per load
    // (the guarded global loads compiled to one exec-masked basic block per element: ~120 instructions and 13 branches per tile in
    // front of 18 MFMAs).  Same values, same order.  The last, partial channel tile of a range keeps the guarded form.
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wgt), 0, 0x7FFFFFFF, 0x00020000);
    int a_vo[NA], w_vo[NW];
#pragma unroll
    for (int i = 0; i < NA; ++i) a_vo[i] = ((a_ok >> i) & 1ull) ? a_off[i] * 4 : (int)0x80000000;
#pragma unroll
    for (int t = 0; t < NW; ++t) w_vo[t] = ((w_ok >> t) & 1ull) ? w_off[t] * 4 : (int)0x80000000;
    auto fetch = [&](int c0) {
        if (c0 + CK <= Kc) {
            const int so_a = __builtin_amdgcn_readfirstlane(c0 * (int)a.in_cstride * 4), so_w = __builtin_amdgcn_readfirstlane(c0 * (int)a.w_cstride * 4);
#pragma unroll
            for (int i = 0; i < NA; ++i) av[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, a_vo[i], so_a, 0));
#pragma unroll
            for (int t = 0; t < NW; ++t) wv[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, w_vo[t], so_w, 0));
            return;
        }
        const float* inc = in + (size_t)c0 * a.in_cstride;
        const float* wc = wgt + (size_t)c0 * a.w_cstride;
#pragma unroll
        for (int i = 0; i < NA; ++i) av[i] = a_vo[i] >= 0 && (c0 + a_cl[i] < Kc) ? inc[a_vo[i] >> 2] : 0.f;
#pragma unroll
        for (int t = 0; t < NW; ++t) wv[t] = w_vo[t] >= 0 && (c0 + w_cl[t] < Kc) ? wc[w_vo[t] >> 2] : 0.f;
    };
    f32x4 acc[FN];
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(cbeg);
    // LDS addresses as ONE base per access family + compile-time offsets (the instruction's offset field).  The bases are re-defined (an empty asm) in
    // every trip: hoisted out of the loop as invariants, the 18 + 18 + 18 sums each sat in a register of their own (167 -> 188 VGPRs with the batches)
    // (integer indices, not pointers: a pointer that went through an asm loses its LDS address space and the accesses become flat)
    int a_wr = wave * LDA + pl;
    int a_rd = (grp * KSTEPS * 4 + (lane >> 4)) * LDA + pw * 16 + (lane & 15);
    int w_rd = (lane & 15) * LDW + grp * KSTEPS * 4 + (lane >> 4);
    for (int c0 = cbeg; c0 < Kc; c0 += CK) {
        asm volatile("" : "+v"(a_wr), "+v"(a_rd), "+v"(w_rd));
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NA; ++i) As[a_wr + NWV * i * LDA] = av[i];
#pragma unroll
        for (int t = 0; t < NW; ++t)
            if (w_lds[t] >= 0) Ws[w_lds[t]] = wv[t];
        __syncthreads();
        if (c0 + CK < Kc) fetch(c0 + CK);
        // The fragments of KB k steps are read from LDS as one batch, and the NEXT batch is on its way while this one feeds the MFMAs (round 5:
        // the compiler's own order was read -> wait -> MFMA per k step, an exposed LDS round trip in front of every one of the 18 MFMAs of a tile;
        // same operands in the same order, same bits).
        constexpr int KB0 = FN == 1 ? CONV_KB : 3;
        constexpr int KB = KB0 > 0 ? (KB0 < KSTEPS ? KB0 : KSTEPS) : KSTEPS;
        float af[2][KB], bf[2][FN][KB];
        auto frag = [&](int buf, int k0) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < KB; ++t) {
                if (k0 + t >= KSTEPS) break;
                af[buf][t] = As[a_rd + (k0 + t) * 4 * LDA];
#pragma unroll
                for (int j = 0; j < FN; ++j) bf[buf][j][t] = Ws[w_rd + j * 16 * LDW + (k0 + t) * 4];
            }
        };
        frag(0, 0);
#pragma unroll
        for (int k0 = 0, cur = 0; k0 < KSTEPS; k0 += KB, cur ^= 1) {
            if (k0 + KB < KSTEPS) frag(cur ^ 1, k0 + KB);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < KB; ++t) {
                if (k0 + t >= KSTEPS) break;
#pragma unroll
                for (int j = 0; j < FN; ++j) {
                    acc[j] = mfma4(af[cur][t], bf[cur][j][t], acc[j]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (NG == 2) {   // second wave group -> first, through the (now idle) A tile
        __syncthreads();
        if (grp == 1) {
#pragma unroll
            for (int j = 0; j < FN; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) As[(j * 4 + r) * 256 + (tid & 255)] = acc[j][r];
        }
        __syncthreads();
        if (grp == 1) return;
#pragma unroll
        for (int j = 0; j < FN; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] += As[(j * 4 + r) * 256 + tid];
    }
    // epilogue: acc[j][r] = out[n = n0 + j*16 + (lane&15)][pixel = m0 + pw*16 + (lane>>4)*4 + r]
    if (ksplit > 1) {
        float* wsp = a.ws + (((size_t)kslice * a.N + img) * a.Cout) * HWo;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
            const int n = n0 + j * 16 + (lane & 15);
            if (n >= a.Cout) continue;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int pp = m0 + pw * 16 + (lane >> 4) * 4 + r;
                if (pp < HWo) wsp[(size_t)n * HWo + pp] = acc[j][r];
            }
        }
        return;
    }
    float* out = a.out + (size_t)img * a.out_nstride;
    // bias and (accumulate) the previous values are loaded up front from clamped addresses: a guarded load per element
    // would be one memory round trip per element
    float bj[FN], prev[FN][4];
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int nc = min(n0 + j * 16 + (lane & 15), a.Cout - 1);
        bj[j] = bias ? bias[nc] : 0.f;
        if (a.accumulate) {
#pragma unroll
            for (int r = 0; r < 4; ++r) prev[j][r] = out[(size_t)nc * a.out_cstride + min(m0 + pw * 16 + (lane >> 4) * 4 + r, HWo - 1)];
        }
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (n >= a.Cout) continue;
        const float b = bj[j];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int pp = m0 + pw * 16 + (lane >> 4) * 4 + r;
            if (pp < HWo) {
                float v = acc[j][r] + b;
                if (a.act == 1) v = 1.0f / (1.0f + __expf(-v));
                out[(size_t)n * a.out_cstride + pp] = a.accumulate ? prev[j][r] + v : v;
            }
        }
    }
}

template <int KS, bool TRANSPOSED, int FN, int CK, int NG>
__global__ __launch_bounds__(256 * NG) void conv_igemm_kernel(ConvArgs a) {
    __shared__ float As[ConvTile<KS, FN, CK>::A_FLOATS];
    __shared__ float Ws[ConvTile<KS, FN, CK>::W_FLOATS];
    conv_igemm_body<KS, TRANSPOSED, FN, CK, NG>(a, blockIdx.x, blockIdx.y, blockIdx.z, As, Ws);
}
// Two independent convolutions in one launch: blocks [0, na) run convolution A (KS = KSA ...), the rest convolution B; each with
// the block coordinates of its own grid (gxa = A's gridDim.x, gxb = B's), blockIdx.z = image for both.  Each keeps the wave
// groups (NGA / NGB) of its own launch -- the surplus waves of the smaller one leave at once (a barrier does not wait for
// waves that have ended) -- so a convolution's bits do not depend on whether it was paired.  LDS is the larger footprint.
template <int KSA, bool TRA, int FNA, int CKA, int NGA, int KSB, bool TRB, int FNB, int CKB, int NGB>
__global__ __launch_bounds__(256 * (NGA > NGB ? NGA : NGB)) void conv_pair_kernel(ConvArgs a, ConvArgs b, int na, int gxa, int gxb) {
    using TA = ConvTile<KSA, FNA, CKA>;
    using TB = ConvTile<KSB, FNB, CKB>;
    constexpr int AF = TA::A_FLOATS > TB::A_FLOATS ? TA::A_FLOATS : TB::A_FLOATS;
    constexpr int WF = TA::W_FLOATS > TB::W_FLOATS ? TA::W_FLOATS : TB::W_FLOATS;
    __shared__ float As[AF];
    __shared__ float Ws[WF];
    const int bid = blockIdx.x;
    if (bid < na) {
        if (NGA < NGB && threadIdx.x >= 256 * NGA) return;
        conv_igemm_body<KSA, TRA, FNA, CKA, NGA>(a, bid % gxa, bid / gxa, blockIdx.z, As, Ws);
    } else {
        if (NGB < NGA && threadIdx.x >= 256 * NGB) return;
        conv_igemm_body<KSB, TRB, FNB, CKB, NGB>(b, (bid - na) % gxb, (bid - na) / gxb, blockIdx.z, As, Ws);
    }
}

// out = (accumulate ? out : 0) + bias + sum_slices ws   (slice order fixed)
__global__ void conv_splitk_reduce_kernel(ConvArgs a, int ksplit) {
    const int HWo = a.Ho * a.Wo;
    const size_t per = (size_t)a.N * a.Cout * HWo;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < per; i += (size_t)gridDim.x * 256) {
        const int pp = i % HWo;
        const int n = (i / HWo) % a.Cout;
        const int img = i / ((size_t)HWo * a.Cout);
        float v = a.bias ? a.bias[conv_arena(a, img) + n] : 0.f;
        float* q = a.out + (size_t)img * a.out_nstride + (size_t)n * a.out_cstride + pp;
        const float prev = a.accumulate ? *q : 0.f;
        int k = 0;
        for (; k + 3 < ksplit; k += 4) {   // four slices in flight, added in slice order
            const float t0 = a.ws[(size_t)k * per + i], t1 = a.ws[(size_t)(k + 1) * per + i], t2 = a.ws[(size_t)(k + 2) * per + i],
                        t3 = a.ws[(size_t)(k + 3) * per + i];
            v += t0; v += t1; v += t2; v += t3;
        }
        for (; k < ksplit; ++k) v += a.ws[(size_t)k * per + i];
        if (a.act == 1) v = 1.0f / (1.0f + __expf(-v));
        *q = a.accumulate ? prev + v : v;
    }
}

// launch policy of one convolution (KS x KS filter, CK channels per K tile): output-channel fragments per workgroup, 8-wave
// workgroups (NG = 2), split-K; the grid is (mt, ny, N)
struct ConvPolicy { int fn_run, ng, ksplit, mt, ny; };
static ConvPolicy conv_policy(const ConvArgs& a, int KS, int CK) {
    const int HWo = a.Ho * a.Wo;
    const int mt = cdiv(HWo, 64);
    // output-channel fragments per workgroup, tuned in-step with alternating runs: the 64 / 128-channel layers of the deep
    // scales run fastest with ONE 16-channel fragment per workgroup (FN = 4: +2.2 %, FN = 2: +0.6 %) -- these launches are
    // latency-bound and more, smaller workgroups shorten them; the 32-channel layers are indifferent (2 kept)
    const int fn = (KS < 5 && a.Cout > 16 && a.Cout <= 32) ? 2 : 1;
    const int nt = cdiv(a.Cout, 16 * fn);
    // Several images per launch (pairs side by side, or the crops of one pair): the chip is full anyway, and a workgroup that owns
    // 32 output channels gathers its input tile once instead of twice (same-box A/B at 4 / 8 pairs per GPU: 2 fragments -1.0 % /
    // -0.75 % step time, 4 fragments -0.3 % / 0; profiles/r03_conv_fn_ab.txt).  Which output channels share a workgroup does not
    // touch any sum, so a pair's bits do not depend on it -- the split-K / wave-group policy below (which does change the
    // summation order) keeps using the one-image fragment count.
    constexpr int batch_fn = 2;
    constexpr int batch_min = 4;
    int fn_run = (KS < 5 && fn == 1 && a.Cout >= 64 && a.N >= batch_min && (batch_fn == 2 || batch_fn == 4)) ? batch_fn : fn;
    // Big planes (round 5; the reference's default 855 .. 900 crops, 448^2, 512^2): thousands of pixel tiles per layer fill the chip whatever the
    // channel split, and every 16-channel fragment a workgroup does NOT own is a second gather of the same input tile by another workgroup
    static const int big_fn = getenv("SPLICE_CONV_BIG_FN") ? atoi(getenv("SPLICE_CONV_BIG_FN")) : 4;   // same-box A/B at 900 x 1200: 0 -> 10.14, 2 -> 10.12, 4 -> 10.10 ms per step
    constexpr int big_mt = 512;
    if (KS < 5 && (big_fn == 2 || big_fn == 4) && mt >= big_mt && a.Cout > 16) {
        const int want = a.Cout > 32 ? big_fn : 2;
        if (want > fn_run) fn_run = want;
    }
    const int nt_run = cdiv(a.Cout, 16 * fn_run);
    // launch policy (split-K, 8-wave workgroups) from the workgroups of ONE image when the images are independent pairs:
    // split-K changes the summation order, and a pair's result must not depend on how many pairs share the launch
    const int npol = a.p_nstride ? (a.p_group > 1 ? a.p_group : 1) : a.N;
    const int wgs = mt * nt * npol;
    int ksplit = 1;
    const int ktiles = cdiv(a.Cin, CK);
    if (a.ws && wgs < 128 && ktiles >= 4 && (size_t)a.N * a.Cout * HWo * 16 <= a.ws_floats) {
        // down to ONE channel tile per slice: in-step (cold caches, latency-bound) more, shorter workgroups win 0.5 % over
        // two tiles per slice, although the second tile's loads would overlap the first one's MFMAs
        ksplit = cdiv(256, wgs);   // (targets of 128 / 384 / 512 workgroups lose 0.3-0.6 %, splitting grids of up to 256 loses 0.8 %)
        if (ksplit > ktiles) ksplit = ktiles;
        if (ksplit > 16) ksplit = 16;
        if (ksplit < 2) ksplit = 1;
    }
    // 8-wave workgroups while the chip holds at most ~2 workgroups per CU (the serial K walk is the run time then)
    // (K tile of 72: 9 steps per wave group; the A tile is big enough for the exchange)
    const bool can8 = KS == 3 && CK == 8;
    const bool ng2 = can8 && (long)mt * nt * ksplit * npol <= 2048 && cdiv(a.Cin, CK) >= 2;
    ConvPolicy p;
    p.fn_run = KS >= 5 ? 1 : fn_run;
    p.ng = ng2 ? 2 : 1;
    p.ksplit = ksplit;
    p.mt = mt;
    p.ny = (KS >= 5 ? cdiv(a.Cout, 16) : nt_run) * ksplit;
    return p;
}
static void conv_splitk_reduce_launch(const ConvArgs& a, int ksplit, hipStream_t s) {
    const size_t per = (size_t)a.N * a.Cout * a.Ho * a.Wo;
    size_t g = (per + 255) / 256;
    if (g > 1024) g = 1024;
    SPLICE_LAUNCH(conv_splitk_reduce_kernel, dim3((unsigned)g), dim3(256), 0, s, a, ksplit);
}

// roofline leg: the layer's algorithmic work rides with the launch (prof.hip): 2 x outputs x reduction length FLOPs; input + output + weight bytes
static inline void conv_note_work(const ConvArgs& a) {
    if (g_splice_prof_open <= 0) return;
    const double outs = (double)a.N * a.Cout * a.Ho * a.Wo, red = (double)a.Cin * a.ks * a.ks;
    splice_prof_note(2.0 * outs * red, 4.0 * (outs + (double)a.N * a.Cin * a.Hi * a.Wi + (double)a.Cout * red * (a.p_nstride ? a.N / (a.p_group > 1 ? a.p_group : 1) : 1)));
}
template <int KS, bool TR, int CK>
static void conv_launch_fn(ConvArgs a, hipStream_t s, int* ksplit_out) {
    const ConvPolicy pol = conv_policy(a, KS, CK);
    conv_note_work(a);
    a.ksplit = pol.ksplit;
    const dim3 grid(pol.mt, pol.ny, a.N);
    constexpr bool CAN8 = KS == 3 && CK == 8;
    if constexpr (KS >= 5) {   // 5x5 / 7x7 (the inversion experiment's generator): one fragment per workgroup, 4 waves
        SPLICE_LAUNCH((conv_igemm_kernel<KS, TR, 1, CK, 1>), grid, dim3(256), 0, s, a);
    } else {
        if (pol.ng == 2) {
            if constexpr (CAN8) {
                if (pol.fn_run == 1) SPLICE_LAUNCH((conv_igemm_kernel<KS, TR, 1, CK, 2>), grid, dim3(512), 0, s, a);
                else if (pol.fn_run == 2) SPLICE_LAUNCH((conv_igemm_kernel<KS, TR, 2, CK, 2>), grid, dim3(512), 0, s, a);
                else SPLICE_LAUNCH((conv_igemm_kernel<KS, TR, 4, CK, 2>), grid, dim3(512), 0, s, a);
            }
        } else {
            if (pol.fn_run == 1) SPLICE_LAUNCH((conv_igemm_kernel<KS, TR, 1, CK, 1>), grid, dim3(256), 0, s, a);
            else if (pol.fn_run == 2) SPLICE_LAUNCH((conv_igemm_kernel<KS, TR, 2, CK, 1>), grid, dim3(256), 0, s, a);
            else SPLICE_LAUNCH((conv_igemm_kernel<KS, TR, 4, CK, 1>), grid, dim3(256), 0, s, a);
        }
    }
    if (ksplit_out) *ksplit_out = pol.ksplit;
    if (pol.ksplit > 1 && !a.defer_reduce) conv_splitk_reduce_launch(a, pol.ksplit, s);
}

// channels per K tile as conv_launch picks them (deeper tiles where the reduction is long)
// (K tiles of 16 channels = 144 k-values for the 3x3 layers with >= 64 / 128 input channels -- half the barrier rounds, twice the
// gathered loads in flight per round -- measured +2.0 % / +1.3 % step time at one pair per GPU, +2.4 % at eight: not kept,
// profiles/r04_gen_ab.txt)
static inline int conv_ck(const ConvArgs& a) { return a.ks == 3 ? (a.Cin >= 32 ? 8 : 4) : a.ks == 1 ? (a.Cin >= 64 ? 32 : 16) : 4; }

// Two INDEPENDENT convolutions in one launch (conv_pair_kernel).  Forward: a = the 1x1 skip convolution of a scale, b = its 3x3
// stride-2 encoder convolution (same input, models/unet/skip.py:60-66); backward: two 1x1 data-gradient convolutions (the skip
// branch's and the deeper scale's last decoder convolution).  Each keeps the launch policy, the split-K workspace and the BITS of
// its own launch, so pairing is a pure launch-count choice: it pays on the latency-bound chains of few images (-0.9 % step time at
// one pair per GPU) and not where the launches fill the chip (+0.2 % at eight: the pair runs at the larger register / LDS
// footprint), hence only below SPLICE_CONV_PAIR_MAXN images (profiles/r04_gen_ab.txt).  Combinations outside the instantiated set,
// reflection padding or 5x5 / 7x7 filters fall back to two launches.  Returns through ksplit_a / ksplit_b what conv_launch would.
template <int KSA, bool TRA, int FNA, int CKA, int KSB, bool TRB, int FNB, int CKB, int NGB>
static void conv_pair_go(const ConvArgs& a, const ConvArgs& b, const ConvPolicy& pa, const ConvPolicy& pb, hipStream_t s) {
    const int na = pa.mt * pa.ny, nb = pb.mt * pb.ny;
    SPLICE_LAUNCH((conv_pair_kernel<KSA, TRA, FNA, CKA, 1, KSB, TRB, FNB, CKB, NGB>), dim3(na + nb, 1, a.N), dim3(256 * NGB), 0, s, a, b, na, pa.mt, pb.mt);
}
int conv_pair_launch(ConvArgs a, ConvArgs b, hipStream_t s, int* ksplit_a, int* ksplit_b) {
    static const int pair_on = getenv("SPLICE_CONV_PAIR") ? atoi(getenv("SPLICE_CONV_PAIR")) : 1;
    constexpr int pair_maxn = 4;
    const int cka = conv_ck(a), ckb = conv_ck(b);
    bool done = false;
    if (pair_on && a.N == b.N && a.N < pair_maxn && !a.reflect && !b.reflect && a.ks == 1 && a.stride == 1 && (b.stride == 1 || b.stride == 2) &&
        a.transposed == b.transposed && (size_t)a.Cin * a.in_cstride <= 0x7fffffffULL && (size_t)b.Cin * b.in_cstride <= 0x7fffffffULL) {
        const ConvPolicy pa = conv_policy(a, 1, cka), pb = conv_policy(b, b.ks, ckb);
        a.ksplit = pa.ksplit; b.ksplit = pb.ksplit;
#define PAIR(TR_, FNA_, CKA_, KSB_, FNB_, CKB_, NG_)                                                                                         \
    if (!done && a.transposed == (TR_ ? 1 : 0) && pa.ng == 1 && pa.fn_run == FNA_ && cka == CKA_ && b.ks == KSB_ && pb.fn_run == FNB_ && ckb == CKB_ && pb.ng == NG_) { \
        conv_pair_go<1, TR_, FNA_, CKA_, KSB_, TR_, FNB_, CKB_, NG_>(a, b, pa, pb, s);                                                       \
        done = true;                                                                                                                          \
    }
        // forward: skip (Cout = 4: one fragment) || 3x3 encoder convolution
        PAIR(false, 1, 16, 3, 1, 4, 1) PAIR(false, 1, 16, 3, 2, 4, 1)
        PAIR(false, 1, 16, 3, 1, 8, 1) PAIR(false, 1, 16, 3, 2, 8, 1) PAIR(false, 1, 16, 3, 1, 8, 2) PAIR(false, 1, 16, 3, 2, 8, 2)
        PAIR(false, 1, 32, 3, 1, 8, 1) PAIR(false, 1, 32, 3, 2, 8, 1) PAIR(false, 1, 32, 3, 1, 8, 2) PAIR(false, 1, 32, 3, 2, 8, 2)
        // backward: skip data gradient (4 -> Cin channels) || 1x1 data gradient of the deeper scale's decoder output convolution
        PAIR(true, 1, 16, 1, 1, 16, 1) PAIR(true, 1, 16, 1, 2, 16, 1) PAIR(true, 2, 16, 1, 1, 16, 1) PAIR(true, 2, 16, 1, 2, 16, 1)
        PAIR(true, 1, 16, 1, 1, 32, 1) PAIR(true, 1, 16, 1, 2, 32, 1) PAIR(true, 2, 16, 1, 1, 32, 1) PAIR(true, 2, 16, 1, 2, 32, 1)
#undef PAIR
        if (done) {
            if (ksplit_a) *ksplit_a = pa.ksplit;
            if (ksplit_b) *ksplit_b = pb.ksplit;
            if (pa.ksplit > 1 && !a.defer_reduce) conv_splitk_reduce_launch(a, pa.ksplit, s);
            if (pb.ksplit > 1 && !b.defer_reduce) conv_splitk_reduce_launch(b, pb.ksplit, s);
            return SPLICE_OK;
        }
    }
    int rc = conv_launch(a, s, ksplit_a);
    if (rc != SPLICE_OK) return rc;
    return conv_launch(b, s, ksplit_b);
}

// ---------------------------------------------------------------------------------------
// 3x3 stride-1 convolution of BIG planes (round 5: the reference's default 855 .. 900 crops, 448^2, 512^2): a 2-D pixel tile with the input halo
// staged in LDS.  conv_igemm_body gathers 64 pixels x 72 k-values per channel tile for 18 MFMAs per wave -- every input element is fetched 9 times
// per 16 output channels, each behind its own descriptor -- and the instruction stream around the MFMAs costs twice the matrix pipe's time on
// these layers (profiles/r05_conv_big_planes.txt).  Here a workgroup owns 4 RW rows x 64 columns of output (RW = 1 is what runs: 4 rows); per channel
// chunk it stages the (4 RW + 2) x (64 + 2) input patch ONCE (padding / reflection resolved while staging, row-contiguous loads), a wave owns RW rows =
// 4 RW pixel fragments, and one weight fragment + one address add serve 4 RW MFMAs per output-channel fragment.  The k order inside a chunk, the chunk size (conv_ck) and the operand layout are those
// of conv_igemm_body: the same bits (tools/gen_bits.py under SPLICE_CONV_TILE=0 / 1).
// RW = output rows per wave (1: the 4-row tile, the default on every plane -- 118 .. 133 VGPRs, 3 - 4 waves per SIMD; 2: an 8-row tile with 1.25 x instead of
// 1.5 x the halo and 167 .. 183 VGPRs, measured slower everywhere: SPLICE_CONV_TILE_RW1_MAX)
template <bool TRANSPOSED, int FN, int CK, int RW>
__global__ __launch_bounds__(256) void conv3x3_tile_kernel(ConvArgs a, int tiles_x) {
    constexpr int CT_TH = 4 * RW, CT_PH = CT_TH + 2, CT_PLANE = CT_PH * CT_PW, NF = 4 * RW;   // NF = 16-pixel fragments per wave
    constexpr int KT = CK * 9, KSTEPS = KT / 4, LDW = KT + 2, BN = 16 * FN;
    constexpr int PE = CK * CT_PLANE;                 // patch elements per chunk
    constexpr int NP = (PE + 255) / 256;              // ... per thread
    constexpr int NW = (BN * KT + 255) / 256;         // weight elements per thread per chunk
    __shared__ float Ps[PE];
    __shared__ float Ws[BN * LDW];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.z;
    const int x0 = (blockIdx.x % tiles_x) * CT_TW, y0 = (blockIdx.x / tiles_x) * CT_TH;
    const int n0 = blockIdx.y * BN;
    const float* in = a.in + (size_t)img * a.in_nstride;
    const float* wgt = a.w + conv_arena(a, img);
    const float* bias = a.bias ? a.bias + conv_arena(a, img) : nullptr;
    // source coordinates of the patch origin: forward sy = oy - pad + ky, data gradient sy = oy + pad - ky (ky = 0 .. 2)
    const int sy0 = TRANSPOSED ? y0 + a.pad - 2 : y0 - a.pad, sx0 = TRANSPOSED ? x0 + a.pad - 2 : x0 - a.pad;
    // ---- staging descriptors: patch element e = tid + 256 j = (channel, patch row, patch column); fixed for the kernel, the chunk enters as the scalar offset
    int p_vo[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int e = tid + 256 * j;
        const int c = e / CT_PLANE, rem = e % CT_PLANE, r = rem / CT_PW, x = rem % CT_PW;
        int sy = sy0 + r, sx = sx0 + x;
        if (!TRANSPOSED && a.reflect) {   // nn.ReflectionPad2d in front of the convolution: mirror without the edge
            sy = sy < 0 ? -sy : (sy >= a.Hi ? 2 * (a.Hi - 1) - sy : sy);
            sx = sx < 0 ? -sx : (sx >= a.Wi ? 2 * (a.Wi - 1) - sx : sx);
        }
        const bool ok = e < PE && sy >= 0 && sy < a.Hi && sx >= 0 && sx < a.Wi;
        p_vo[j] = ok ? (int)(c * a.in_cstride + (size_t)sy * a.Wi + sx) * 4 : (int)0x80000000;
    }
    int w_vo[NW], w_lds[NW];
#pragma unroll
    for (int t = 0; t < NW; ++t) {
        const int e = tid + 256 * t;
        const int j = e / KT, k = e % KT;
        const int cl = k / 9, tap = k % 9;
        const bool ok = e < BN * KT && (n0 + j) < a.Cout;
        w_vo[t] = ok ? (int)((size_t)(n0 + j) * a.w_jstride + (size_t)cl * a.w_cstride + tap) * 4 : (int)0x80000000;
        w_lds[t] = e < BN * KT ? j * LDW + k : -1;
    }
    // ---- fragment addressing: lane (pixel i = lane & 15, k group g = lane >> 4); k = kk * 4 + g = (channel, ky, kx) -> offset inside the patch
    int koff[KSTEPS];
#pragma unroll
    for (int kk = 0; kk < KSTEPS; ++kk) {
        const int k = kk * 4 + (lane >> 4);
        const int c = k / 9, tap = k % 9, ky = tap / 3, kx = tap % 3;
        koff[kk] = c * CT_PLANE + (TRANSPOSED ? 2 - ky : ky) * CT_PW + (TRANSPOSED ? 2 - kx : kx);
    }
    int a_rd = (RW * wave) * CT_PW + (lane & 15);                 // pixel (row 2 wave, column lane & 15) of the tile, in patch coordinates without the tap
    int w_rd = (lane & 15) * LDW + (lane >> 4);
    const __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(in), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(wgt), 0, 0x7FFFFFFF, 0x00020000);
    const int Kc = a.Cin;
    float pv[NP], wv[NW];
    auto fetch = [&](int c0) __attribute__((always_inline)) {
        const int so_a = __builtin_amdgcn_readfirstlane(c0 * (int)a.in_cstride * 4), so_w = __builtin_amdgcn_readfirstlane(c0 * (int)a.w_cstride * 4);
        if (c0 + CK <= Kc) {
#pragma unroll
            for (int j = 0; j < NP; ++j) pv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, p_vo[j], so_a, 0));
#pragma unroll
            for (int t = 0; t < NW; ++t) wv[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, w_vo[t], so_w, 0));
        } else {   // the last, partial chunk of the reduction: channels behind Kc read as 0
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                const bool cok = c0 + (tid + 256 * j) / CT_PLANE < Kc;
                pv[j] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, cok ? p_vo[j] : (int)0x80000000, so_a, 0));
            }
#pragma unroll
            for (int t = 0; t < NW; ++t) {
                const bool cok = c0 + ((tid + 256 * t) % KT) / 9 < Kc;
                wv[t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rw, cok ? w_vo[t] : (int)0x80000000, so_w, 0));
            }
        }
    };
    const int fn_live = __builtin_amdgcn_readfirstlane(min(FN, (a.Cout - n0 + 15) / 16));   // fragments of this workgroup that hold output channels
    f32x4 acc[NF][FN];
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[f][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    fetch(0);
    for (int c0 = 0; c0 < Kc; c0 += CK) {
        asm volatile("" : "+v"(a_rd), "+v"(w_rd));   // (LDS bases re-defined per trip: base + instruction offset instead of one register per address)
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (tid + 256 * j < PE) Ps[tid + 256 * j] = pv[j];
#pragma unroll
        for (int t = 0; t < NW; ++t)
            if (w_lds[t] >= 0) Ws[w_lds[t]] = wv[t];
        __syncthreads();
        if (c0 + CK < Kc) fetch(c0 + CK);
        // fragments of k step kk + 1 are on their way while step kk feeds 8 x FN MFMAs
        float af[2][NF], bf[2][FN];
        auto frag = [&](int buf, int kk) __attribute__((always_inline)) {
            const int ao = a_rd + koff[kk];
#pragma unroll
            for (int f = 0; f < NF; ++f) af[buf][f] = Ps[ao + (f >> 2) * CT_PW + (f & 3) * 16];
#pragma unroll
            for (int j = 0; j < FN; ++j) bf[buf][j] = Ws[w_rd + j * 16 * LDW + kk * 4];
        };
        frag(0, 0);
#pragma unroll
        for (int kk = 0; kk < KSTEPS; ++kk) {
            if (kk + 1 < KSTEPS) frag((kk + 1) & 1, kk + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < FN; ++j) {
                if (j > 0 && j >= fn_live) continue;   // a 16-channel fragment wholly behind Cout (36 = 32 + 4, 68, 132 output channels): no MFMAs for it
#pragma unroll
                for (int f = 0; f < NF; ++f) acc[f][j] = mfma4(af[kk & 1][f], bf[kk & 1][j], acc[f][j]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // ---- epilogue: acc[f][j][r] = out[n = n0 + j*16 + (lane & 15)][row y0 + 2 wave + (f >> 2)][column x0 + (f & 3) * 16 + (lane >> 4) * 4 + r]
    float* out = a.out + (size_t)img * a.out_nstride;
#pragma unroll
    for (int j = 0; j < FN; ++j) {
        const int n = n0 + j * 16 + (lane & 15);
        if (n >= a.Cout) continue;
        const float b = bias ? bias[n] : 0.f;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int row = y0 + RW * wave + (f >> 2), col = x0 + (f & 3) * 16 + (lane >> 4) * 4;
            if (row >= a.Ho || col >= a.Wo) continue;
            float* q = out + (size_t)n * a.out_cstride + (size_t)row * a.Wo + col;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = acc[f][j][r] + b;   // (no activation in this kernel: the generator's only sigmoid sits behind a 1x1 convolution; conv_tile_ok)
            }
            if (a.accumulate) {
                float pr[4];
                ld_run(q, 0, a.Wo - col, pr);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = pr[r] + v[r];
            }
            st_run(q, 0, a.Wo - col, v);
        }
    }
}
static bool conv_tile_ok(const ConvArgs& a) {
    static const int on = getenv("SPLICE_CONV_TILE") ? atoi(getenv("SPLICE_CONV_TILE")) : 1;
    // planes above 40000 pixels (same-box A/B, ms per step at min 65536 / 40000 / 12000: one pair at 224^2 3.630 / 3.609 / 3.717, eight pairs 16.40 / 16.25 / 16.12,
    // 900 x 1200 9.42 / 9.23 / 9.41: the 112^2 planes are 28 tiles -- too few for one image, and the policy must not depend on the images per launch)
    static const int min_px = getenv("SPLICE_CONV_TILE_MIN") ? atoi(getenv("SPLICE_CONV_TILE_MIN")) : 40000;
    return on && a.ks == 3 && a.stride == 1 && !a.act && a.Wo >= 64 && (long long)a.Ho * a.Wo > min_px && !(a.reflect && a.transposed) &&
           (size_t)a.Cin * a.in_cstride <= 0x1fffffffULL;
}
template <bool TR, int CK>
static void conv_tile_launch(const ConvArgs& a, hipStream_t s) {
    conv_note_work(a);
    constexpr int rw1_max = 0x7fffffff;   // planes up to this many pixels take the 4-row tile: all of them (same-box A/B against the 8-row tile: 900 x 1200 9.20 -> 9.07 ms, one pair at 224^2 3.594 -> 3.574, eight pairs 16.33 -> 16.30: 118 .. 133 instead of 167 .. 183 VGPRs)
    const bool rw1 = (long long)a.Ho * a.Wo <= rw1_max;
    const int tiles_x = cdiv(a.Wo, CT_TW), tiles_y = cdiv(a.Ho, rw1 ? 4 : 8);
    if (rw1) {
        if (a.Cout <= 16) SPLICE_LAUNCH((conv3x3_tile_kernel<TR, 1, CK, 1>), dim3(tiles_x * tiles_y, 1, a.N), dim3(256), 0, s, a, tiles_x);
        else SPLICE_LAUNCH((conv3x3_tile_kernel<TR, 2, CK, 1>), dim3(tiles_x * tiles_y, cdiv(a.Cout, 32), a.N), dim3(256), 0, s, a, tiles_x);
        return;
    }
    if (a.Cout <= 16) SPLICE_LAUNCH((conv3x3_tile_kernel<TR, 1, CK, 2>), dim3(tiles_x * tiles_y, 1, a.N), dim3(256), 0, s, a, tiles_x);
    else SPLICE_LAUNCH((conv3x3_tile_kernel<TR, 2, CK, 2>), dim3(tiles_x * tiles_y, cdiv(a.Cout, 32), a.N), dim3(256), 0, s, a, tiles_x);
}

int conv_launch(const ConvArgs& a, hipStream_t s, int* ksplit_out) {
    if (a.ks != 1 && a.ks != 3 && a.ks != 5 && a.ks != 7) return SPLICE_ERR_ARG;
    if (a.reflect && a.transposed) return SPLICE_ERR_ARG;   // the data gradient of a reflection-padded conv goes through conv_reflect_dgrad_launch
    if (a.ks >= 5) {
        if (a.ks == 5) { if (a.transposed) conv_launch_fn<5, true, 4>(a, s, ksplit_out); else conv_launch_fn<5, false, 4>(a, s, ksplit_out); }
        else { if (a.transposed) conv_launch_fn<7, true, 4>(a, s, ksplit_out); else conv_launch_fn<7, false, 4>(a, s, ksplit_out); }
        return SPLICE_OK;
    }
    if (a.stride != 1 && a.stride != 2) return SPLICE_ERR_ARG;
    if ((size_t)a.Cin * a.in_cstride > 0x7fffffffULL) return SPLICE_ERR_ARG;   // 32-bit gather offsets
    // deeper channel tiles where the reduction is long (fewer barrier rounds on the small, deep layers)
    if (conv_tile_ok(a)) {   // big planes: the LDS-halo tile (no split-K there)
        if (a.Cin >= 32) { if (a.transposed) conv_tile_launch<true, 8>(a, s); else conv_tile_launch<false, 8>(a, s); }
        else { if (a.transposed) conv_tile_launch<true, 4>(a, s); else conv_tile_launch<false, 4>(a, s); }
        if (ksplit_out) *ksplit_out = 1;
        return SPLICE_OK;
    }
    if (a.ks == 3) {
        if (a.Cin >= 32) { if (a.transposed) conv_launch_fn<3, true, 8>(a, s, ksplit_out); else conv_launch_fn<3, false, 8>(a, s, ksplit_out); }
        else { if (a.transposed) conv_launch_fn<3, true, 4>(a, s, ksplit_out); else conv_launch_fn<3, false, 4>(a, s, ksplit_out); }
    } else {
        if (a.Cin >= 64) { if (a.transposed) conv_launch_fn<1, true, 32>(a, s, ksplit_out); else conv_launch_fn<1, false, 32>(a, s, ksplit_out); }
        else { if (a.transposed) conv_launch_fn<1, true, 16>(a, s, ksplit_out); else conv_launch_fn<1, false, 16>(a, s, ksplit_out); }
    }
    return SPLICE_OK;
}

// The path conv_launch takes for `a`, as five ints {tile kernel, CK, fn_run, ng, ksplit}: read off conv_tile_ok / conv_ck / conv_policy, the
// functions the dispatch itself asks (the op-level test hooks report it; nothing else calls this)
void conv_form_report(const ConvArgs& a, int* form) {
    const bool tile = a.ks == 3 && conv_tile_ok(a);
    const int CK = a.ks >= 5 ? 4 : conv_ck(a);
    const ConvPolicy pol = conv_policy(a, a.ks, CK);
    form[0] = tile ? 1 : 0;
    form[1] = CK;
    form[2] = tile ? (a.Cout <= 16 ? 1 : 2) : pol.fn_run;
    form[3] = tile ? 1 : pol.ng;
    form[4] = tile ? 1 : pol.ksplit;
}

// Data gradient of a reflection-padded convolution: y = conv(pad_reflect(x)), so dL/dx = fold(dL/dx_pad) where dL/dx_pad is the
// plain transposed convolution on the PADDED domain (Hi + 2p) x (Wi + 2p) -- conv_launch in data-gradient form with pad 0 --
// and fold adds every padded position into the interior pixel it mirrors (separable: up to 3 source rows x 3 source
// columns per pixel, fixed order).
__global__ __launch_bounds__(256) void reflect_fold_kernel(const float* __restrict__ dpad, float* __restrict__ dx, size_t dx_nstride, size_t dx_cstride,
                                                           int C, int H, int W, int p, int accumulate) {
    const int Hp = H + 2 * p, Wp = W + 2 * p;
    const int c = blockIdx.y, img = blockIdx.z;
    const float* src = dpad + ((size_t)img * C + c) * Hp * Wp;
    float* dst = dx + (size_t)img * dx_nstride + (size_t)c * dx_cstride;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < H * W; i += gridDim.x * 256) {
        const int y = i / W, x = i % W;
        int ys[3], xs[3], ny = 0, nx = 0;
        ys[ny++] = y + p;
        if (y >= 1 && y <= p) ys[ny++] = p - y;                               // top border mirrors rows 1..p
        if (y <= H - 2 && y >= H - 1 - p) ys[ny++] = p + 2 * (H - 1) - y;     // bottom border mirrors rows H-1-p..H-2
        xs[nx++] = x + p;
        if (x >= 1 && x <= p) xs[nx++] = p - x;
        if (x <= W - 2 && x >= W - 1 - p) xs[nx++] = p + 2 * (W - 1) - x;
        float acc = 0.f;
        for (int a = 0; a < ny; ++a)
            for (int b = 0; b < nx; ++b) acc += src[(size_t)ys[a] * Wp + xs[b]];
        dst[i] = accumulate ? dst[i] + acc : acc;
    }
}
// a: the layer in data-gradient form as for the zero-padded case (in = dy, out = d_in [N][Cout][Ho][Wo], pad = the layer's
// padding); pad_scratch: N * Cout * (Ho + 2 pad) * (Wo + 2 pad) floats
int conv_reflect_dgrad_launch(ConvArgs a, float* pad_scratch, hipStream_t s) {
    const int p = a.pad, Hp = a.Ho + 2 * p, Wp = a.Wo + 2 * p;
    float* out = a.out;
    const size_t out_ns = a.out_nstride, out_cs = a.out_cstride;
    const int acc = a.accumulate, H = a.Ho, W = a.Wo;
    a.out = pad_scratch; a.out_nstride = (size_t)a.Cout * Hp * Wp; a.out_cstride = (size_t)Hp * Wp;
    a.Ho = Hp; a.Wo = Wp; a.pad = 0; a.accumulate = 0; a.reflect = 0; a.transposed = 1; a.ws = nullptr;
    const int rc = conv_launch(a, s);
    if (rc != SPLICE_OK) return rc;
    int gx = cdiv(H * W, 256);
    if (gx > 64) gx = 64;
    SPLICE_LAUNCH(reflect_fold_kernel, dim3(gx, a.Cout, a.N), dim3(256), 0, s, pad_scratch, out, out_ns, out_cs, a.Cout, H, W, p, acc);
    return SPLICE_OK;
}
