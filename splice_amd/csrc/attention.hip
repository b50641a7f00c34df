// Fused multi-head self-attention (head dim 64) for the DINO ViT, forward + backward,
// gfx950.  Replaces the DINO `Attention.forward` the reference reaches through
// `self.model(input_img)` (models/extractor.py:83,91,99): softmax(q k^T / sqrt(d)) v,
// without materialising the [h,T,T] probability tensors the reference's hooks keep.
//
// This file: the tile toolkit shared by the kernels below, the e4m3 forward of BASELINE configs[4] (16x16x32 fp8 MFMAs), the 16x16x32 bf16
// backward halves that serve plain (un-scaled) q at the op-level C-ABI, the small delta / probability kernels, and the launch policy.  The
// kernels the ViT engine runs -- q pre-scaled, 32x32x16 bf16 MFMAs -- live in attn_x32.h (forward) and attn_bwd_x32.h (backward).  In every
// kernel the products are "swapped" so that a lane owns ONE query (or one key) column of the score tile: softmax statistics are per-lane
// scalars and the probabilities feed the second MFMA straight from registers (no LDS round trip, no cross-lane traffic in the hot loop).
//
// Inputs: qkv  bf16 [B*Tld][3D]  (row = b*Tld + token; q | k | v column blocks, heads
//                                 contiguous inside each block -- the layout
//                                 models/extractor.py:136-151 reshapes)
//         qkvT bf16 [3D][ldt]    the same matrix transposed (only the [CLS]-row kernels of vit_cls.hip still read it; written by the QKV GEMM
//                                 epilogue) -- supplies the token-contiguous operands.
// Tokens t >= T inside a pass are padding: masked as keys, harmless as queries.
#include "kernels.h"
#include <cstdlib>


#define NEG_BIG (-1.0e30f)
#define LOG2E 1.4426950408889634f
#define LN2 0.6931471805599453f
// softmax runs in base 2: scores are scaled by scale*log2(e) once, probabilities are v_exp_f32 (exp2) directly,
// and the saved log-sum-exp is kept in log2 units (lse2 = m2 + log2(l)); the backward uses exp2(s*c - lse2).

__device__ __forceinline__ u32x4 ld16v(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }
__device__ __forceinline__ u32x4 pack8v(const f32x4& a, const f32x4& b) {
    return u32x4{pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
}
__device__ __forceinline__ void st4bf(bf16_t* p, const f32x4& v, float s) {
    *reinterpret_cast<uint2*>(p) = uint2{pack2bf(v[0] * s, v[1] * s), pack2bf(v[2] * s, v[3] * s)};
}
__device__ __forceinline__ float group4_max(float v) {  // across the 4 lane groups (same lane&15)
    v = fmaxf(v, __shfl_xor(v, 16, 64));
    return fmaxf(v, __shfl_xor(v, 32, 64));
}
__device__ __forceinline__ float group4_sum(float v) {
    v += __shfl_xor(v, 16, 64);
    return v + __shfl_xor(v, 32, 64);
}

// ---------------------------------------------------------------------------------------
// Tile toolkit: LDS-DMA staging (global_load_lds, 16 B per lane, no VGPR round trip) + fragment layouts that
// need ONE ds_read_b128 (or two transposing 8-byte reads) per MFMA operand.
//
// A wave-instruction of the DMA fills 8 rows x 128 B of LDS linearly (dest = piece base + lane*16), so the
// swizzle is applied on the SOURCE chunk a lane fetches.  Wave w of the 4 moves the 1-KiB pieces w and w+4 of a
// [64][64] bf16 tile.
//
//   Every operand is staged ONCE, as a "token" tile [64 tokens][64 d] (rows of q / k / v / dO as they lie in memory).
//   * Token-major fragments (the operand whose rows become the ROWS of the score MFMA: keys in the forward / dQ kernels, queries
//     in the dK/dV kernel) are one ds_read_b128 each.  Block nb (16 MFMA rows) of 32-token sub-tile `sub` takes row i = 4*j + r
//     from token sub*32 + 8*j + 4*nb + r: lane group g then owns, over nb = 0,1, the EIGHT CONSECUTIVE tokens sub*32 + 8g .. 8g+7,
//     which is exactly the k-slot order of the packed probabilities it feeds to the second MFMA.
//   * The TRANSPOSED operand of that second MFMA (V^T in the forward, K^T in the dQ half, dO^T / Q^T in the dK/dV half: rows =
//     head dimension, k = token) comes out of the same kind of tile with ds_read_b64_tr_b16: within a 16-lane group lane m points
//     at the 4 consecutive d values (m & 3) of token row (m >> 2), and lane i receives the column d0 + i of that 4 x 16 block --
//     4 consecutive tokens at one d (tools/micro/tr_read.hip); two such reads are one 16 x 32 operand.  Up to round 3 these
//     operands were staged from transposed copies (qkvT / doutT) written by the producing GEMMs: twice the LDS-DMA traffic and
//     LDS footprint in the backward, and an extra output per GEMM.
//   16-byte chunk c of a row is stored at position c ^ swz(row), swz = (row bit 1) << 1 | (row bit 3) << 2: conflict-free for the
//   permuted row set above under the b128 lane groups AND for the transposing reads (SQ_LDS_BANK_CONFLICT = 0 for both,
//   tools/micro/tr_conflict.hip, profiles/r03_tr_read_conflicts.txt).
typedef __attribute__((address_space(3))) void lds_void;
typedef __attribute__((address_space(1))) const void glb_void;

template <int NW>   // waves that move one tile set: 4 (pieces w and w + 4 each) or 8 (one piece each)
struct TileDmaT {
    int wave;                 // scalar
    int lrow, tchunk;
    // wave = index of the wave inside its group of NW (a group moves one tile set; two-group workgroups hold two groups of 4)
    __device__ __forceinline__ TileDmaT() {
        const int lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & (NW - 1);
        lrow = lane >> 3;
        tchunk = (lane & 7) ^ ((((lrow >> 1) & 1) << 1) | ((wave & 1) << 2));   // token tile: row = piece*8 + lrow, piece & 1 == wave & 1
    }
    __device__ __forceinline__ void piece(const bf16_t* src, bf16_t* lds, int i) const {
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(lds + (wave + NW * i) * 512), 16, 0, 0);
    }
    // Interior tiles: a uniform (scalar) tile base + per-lane byte offsets that are fixed for the whole kernel -- one
    // VALU op per DMA instead of the clamp / multiply / 64-bit add chain.
    __device__ __forceinline__ uint32_t token_off(int ld) const { return (uint32_t)(((wave * 8 + lrow) * ld + tchunk * 8) * 2); }
    // tile = first element of the tile (base + tok0*ld); stride = ld
    __device__ __forceinline__ void fast_tile(const bf16_t* tile, uint32_t off, int stride, bf16_t* lds) const {
        const char* b0 = reinterpret_cast<const char*>(tile);
        if (NW == 8) {
            asm volatile("" : "+s"(b0));   // keep the base scalar
            piece(reinterpret_cast<const bf16_t*>(b0 + off), lds, 0);
            return;
        }
        const char* b1 = reinterpret_cast<const char*>(tile + (size_t)32 * stride);
        asm volatile("" : "+s"(b0), "+s"(b1));   // keep the bases scalar
        piece(reinterpret_cast<const bf16_t*>(b0 + off), lds, 0);
        piece(reinterpret_cast<const bf16_t*>(b1 + off), lds, 1);
    }
    // Edge tiles: token-major source, rows = tokens tok0.. (clamped to tok_max), 64 contiguous d at base + tok*ld
    __device__ __forceinline__ void token_tile(const bf16_t* base, int ld, int tok0, int tok_max, bf16_t* lds) const {
#pragma unroll
        for (int i = 0; i < 8 / NW; ++i) {
            int t = tok0 + (wave + NW * i) * 8 + lrow;
            t = t < tok_max ? t : tok_max;
            piece(base + (size_t)t * ld + tchunk * 8, lds, i);
        }
    }
};
typedef TileDmaT<4> TileDma;

struct FragAddr {   // per-lane LDS element offsets of the fragment reads (everything else is an immediate)
    int tok[2];     // token tile: block nb of sub-tile sub, d-half hf   -> tok[hf] + sub*2048 + nb*256
    int tr[4];      // token tile, transposing read: d block nd, sub-tile sub, token half t4 -> tr[nd] + sub*2048 + t4*256
    __device__ __forceinline__ FragAddr(int g, int c) {
        const int swz = (((c >> 1) & 1) << 1) | (((c >> 2) & 1) << 2);   // of row (c>>2)*8 + (c&3): row bit 1 = c bit 1, row bit 3 = c bit 2
        const int row = (c >> 2) * 8 + (c & 3);
        tok[0] = row * 64 + ((g ^ swz) << 3);
        tok[1] = row * 64 + (((4 + g) ^ swz) << 3);
        // lane (g, m = c): token row 8g + (m >> 2), d piece m & 3 (4 values) of d block nd: chunk 2 nd + (m >> 1 & 1), half m & 1
        const int trow = 8 * g + (c >> 2);
        const int tswz = (((trow >> 1) & 1) << 1) | (((trow >> 3) & 1) << 2);
#pragma unroll
        for (int nd = 0; nd < 4; ++nd) tr[nd] = trow * 64 + ((((nd << 1) | ((c >> 1) & 1)) ^ tswz) << 3) + (c & 1) * 4;
    }
};
// one 16 x 32 MFMA operand out of a token tile, transposed: rows = d (lane & 15 within block nd), k = tokens sub*32 + 8g .. 8g+7
typedef short tr_v4s __attribute__((ext_vector_type(4)));
__device__ __forceinline__ u32x4 lds_tr16(const bf16_t* tile, int off) {
    typedef __attribute__((address_space(3))) tr_v4s lds_v4s;
    const tr_v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(tile + off));          // tokens 8g .. 8g+3
    const tr_v4s hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s*)(tile + off + 256));    // tokens 8g+4 .. 8g+7 (4 rows on)
    const uint2 l = __builtin_bit_cast(uint2, lo), h = __builtin_bit_cast(uint2, hi);
    return u32x4{l.x, l.y, h.x, h.y};
}
__device__ __forceinline__ u32x4 lds16(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

// Workgroup -> (query/key block, head, pass): a 1-D grid walked through xcd_remap so that all blocks of one
// (pass, head) run on ONE XCD and its K / V (200 KB) are fetched into a single L2.
__device__ __forceinline__ void attn_block_coords(int nx, int H, int B, int& xb, int& h, int& b) {
    const int lid = xcd_remap(blockIdx.x, nx * H * B);
    xb = lid % nx;
    const int bh = lid / nx;
    h = bh % H;
    b = bh / H;
}
// x0 * a0 + x1 * a1 with a FIXED rounding sequence: round(x0 * a0), then one fused multiply-add.  The two launch forms of the
// forward (two wave groups / one group walking both key ranges) merge their partial softmax states with this; left to the
// compiler's contraction the two code contexts fused different products and the forms differed in the last bit.
__device__ __forceinline__ float merge2(float x0, float a0, float x1, float a1) {
#pragma clang fp contract(off)
    const float t = x0 * a0;          // (not inline asm: an asm statement reading MFMA results gets no hazard wait states)
    return __builtin_fmaf(x1, a1, t);
}
// all of this wave's LDS-DMA has landed, then the workgroup barrier (other waves' pieces + ring slot free)
__device__ __forceinline__ void dma_wait_barrier() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

#define ATTN_RESCALE_LIMIT 1073741824.0f   // a lane whose partial row sum reaches this takes the rescale / exact path (attn_x32.h, the e4m3 forward)

#include "attn_x32.h"
#include "attn_bwd_x32.h"

// ---------------------------------------------------------------------------------------
// e4m3 forward (BASELINE configs[4], "fp8 MFMA attention"): Q K^T and P V on v_mfma_f32_16x16x32_fp8_fp8 from the unscaled
// e4m3 copies of q, k, v the fp8 QKV projection writes beside its bf16 outputs (e4m3 is a floating format: its relative
// precision, 2^-4, holds over 2^-9 .. 448 without a scale).  Same structure as the bf16 kernel -- swapped MFMAs, one query per
// lane column, permuted score rows so that a lane's 8 probabilities are 8 consecutive tokens, LDS-DMA ring, deferred max, key
// range in two halves -- on tiles of HALF the bytes:
//   K  tile [64 keys][64 B of d]: one ds_read_b128 per 16-key block = the operands of BOTH k = 32 MFMAs of a score block
//      (a lane's 16 bytes are d = 16 g .. 16 g + 15: low half -> first MFMA, high half -> second; Q is cut the same way);
//   V^T tile [64 d][64 B of tokens]: one ds_read_b64 per (d block, 32-key sub-tile).
// Rows are 64 B, so four rows share a bank window: K chunks are stored at c ^ 3 * (row bit 4), V^T chunks at c ^ (row >> 2 & 3)
// (source-side swizzle of the DMA, both conflict-free for the lane groups of b128 / b64 reads).
// Probabilities are formed against a reference point 6 binary orders BELOW the running maximum (p = 64 at the maximum) so
// that e4m3's subnormal floor sits at 2^-15 of the largest term; a lane whose partial row sum reaches 448 (the format's
// maximum) takes the exact-maximum path.  The row sums l accumulate the unquantised fp32 probabilities.
// The backward stays on the bf16 kernels (it re-forms P from the bf16 q, k and the log-sum-exp saved here).
typedef long fp8x8_t;
struct TileDma8 {
    int wave, r16, c16;
    __device__ __forceinline__ TileDma8() {
        const int lane = threadIdx.x & 63;
        wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) & 3;
        r16 = lane >> 2;
        c16 = lane & 3;
    }
    // rows = tokens tok0 .. tok0 + 63 (clamped to tok_max), 64 contiguous bytes at base + tok * ld; wave w moves rows 16 w .. 16 w + 15
    __device__ __forceinline__ void token_tile(const uint8_t* base, int ld, int tok0, int tok_max, uint8_t* lds) const {
        int t = tok0 + wave * 16 + r16;
        t = t < tok_max ? t : tok_max;
        const uint8_t* src = base + (size_t)t * ld + ((c16 ^ ((wave & 1) * 3)) << 4);
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(lds + wave * 1024), 16, 0, 0);
    }
    // rows = d, 64 contiguous tokens from tok0 at baseT + d * ldt; a 16-token chunk starting past tok_lim - 16 is replaced by the
    // last in-bounds chunk (masked keys)
    __device__ __forceinline__ void dim_tile(const uint8_t* baseT, int ldt, int tok0, int tok_lim, uint8_t* lds) const {
        int t = tok0 + ((c16 ^ ((r16 >> 2) & 3)) << 4);
        t = t <= tok_lim - 16 ? t : tok_lim - 16;
        const uint8_t* src = baseT + (size_t)(wave * 16 + r16) * ldt + t;
        __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(lds + wave * 1024), 16, 0, 0);
    }
};
struct FragAddr8 {   // per-lane LDS BYTE offsets
    int tok;         // K tile: block nb of sub-tile sub -> tok + sub * 2048 + nb * 256      (b128)
    int dim[2];      // V^T tile: d block nd, sub-tile sub -> dim[sub] + nd * 1024          (b64)
    __device__ __forceinline__ FragAddr8(int g, int c) {
        tok = ((c >> 2) * 8 + (c & 3)) * 64 + ((g ^ (((c >> 3) & 1) * 3)) << 4);
        dim[0] = c * 64 + ((((g >> 1)) ^ ((c >> 2) & 3)) << 4) + ((g & 1) << 3);
        dim[1] = c * 64 + (((2 + (g >> 1)) ^ ((c >> 2) & 3)) << 4) + ((g & 1) << 3);
    }
};
__device__ __forceinline__ f32x4 mfma8(fp8x8_t a, fp8x8_t b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a, b, c, 0, 0, 0); }
__device__ __forceinline__ fp8x8_t pack8_e4m3(const f32x4& a, const f32x4& b) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(a[0], a[1], lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(a[2], a[3], lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(b[0], b[1], hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(b[2], b[3], hi, true);
    return (fp8x8_t)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
#define ATTN8_REF_SHIFT 6.0f      // p = 2^6 at the reference maximum
#define ATTN8_RESCALE_LIMIT 448.0f
template <int QB, int NSUB, bool MASK>
__device__ __forceinline__ void attn_fwd8_tile(const uint8_t* Ks, const uint8_t* Vs, const FragAddr8& fa, const u32x4 (&qf)[QB], float (&m)[QB],
                                               float (&l)[QB], f32x4 (&o)[QB][4], float c2, int kt, int T, int g) {
    f32x4 s[QB][NSUB * 2];
#pragma unroll
    for (int nb = 0; nb < NSUB * 2; ++nb) {
        const u32x4 kf = *reinterpret_cast<const u32x4*>(Ks + fa.tok + (nb >> 1) * 2048 + (nb & 1) * 256);
        const fp8x8_t k0 = (fp8x8_t)(((unsigned long long)kf[1] << 32) | kf[0]), k1 = (fp8x8_t)(((unsigned long long)kf[3] << 32) | kf[2]);
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const fp8x8_t q0 = (fp8x8_t)(((unsigned long long)qf[qb][1] << 32) | qf[qb][0]), q1 = (fp8x8_t)(((unsigned long long)qf[qb][3] << 32) | qf[qb][2]);
            s[qb][nb] = mfma8(k0, q0, f32x4{0.f, 0.f, 0.f, 0.f});
            s[qb][nb] = mfma8(k1, q1, s[qb][nb]);
        }
    }
    if (MASK) {
#pragma unroll
        for (int nb = 0; nb < NSUB * 2; ++nb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool valid = kt + (nb >> 1) * 32 + g * 8 + (nb & 1) * 4 + r < T;
#pragma unroll
                for (int qb = 0; qb < QB; ++qb) s[qb][nb][r] = valid ? s[qb][nb][r] : NEG_BIG;
            }
    }
    f32x4 p[QB][NSUB * 2];
    float ps[QB];
    bool over[QB];
    bool redo = false;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        ps[qb] = 0.f;
#pragma unroll
        for (int nb = 0; nb < NSUB * 2; ++nb) {
#pragma unroll
            for (int r = 0; r < 4; ++r) p[qb][nb][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[qb][nb][r], c2, -m[qb]));
            ps[qb] += (p[qb][nb][0] + p[qb][nb][1]) + (p[qb][nb][2] + p[qb][nb][3]);
        }
        over[qb] = !(ps[qb] < ATTN8_RESCALE_LIMIT);
        redo |= over[qb];
    }
    if (__any(redo)) {
        // exact step, executed by the whole wave but taking effect PER QUERY: only a query one of whose four lanes ran over moves its
        // reference point (to its maximum - 6 binary orders); for the others mn = m, alpha = 1 and the same p come out again.  With
        // the 448 limit this path runs now and then on real data, and a query's result must not depend on which other queries share
        // its wave (16 or 32 per wave, one or two key groups: the launch forms have to agree bit for bit).
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            float mx = NEG_BIG;
#pragma unroll
            for (int nb = 0; nb < NSUB * 2; ++nb)
#pragma unroll
                for (int r = 0; r < 4; ++r) mx = fmaxf(mx, s[qb][nb][r]);
            mx = group4_max(mx) * c2 - ATTN8_REF_SHIFT;
            const bool mine = group4_max(over[qb] ? 1.0f : 0.0f) > 0.f;
            const float mn = mine ? fmaxf(m[qb], mx) : m[qb];
            const float alpha = __builtin_amdgcn_exp2f(m[qb] - mn);
            m[qb] = mn;
            l[qb] *= alpha;
#pragma unroll
            for (int nd = 0; nd < 4; ++nd)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[qb][nd][r] *= alpha;
            ps[qb] = 0.f;
#pragma unroll
            for (int nb = 0; nb < NSUB * 2; ++nb) {
#pragma unroll
                for (int r = 0; r < 4; ++r) p[qb][nb][r] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[qb][nb][r], c2, -mn));
                ps[qb] += (p[qb][nb][0] + p[qb][nb][1]) + (p[qb][nb][2] + p[qb][nb][3]);   // (the summation order of the fast path: an unaffected query keeps its bits)
            }
        }
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) l[qb] += ps[qb];
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
        fp8x8_t pb[QB];
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) pb[qb] = pack8_e4m3(p[qb][sub * 2], p[qb][sub * 2 + 1]);
#pragma unroll
        for (int nd = 0; nd < 4; ++nd) {
            const fp8x8_t vf = *reinterpret_cast<const fp8x8_t*>(Vs + fa.dim[sub] + nd * 1024);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) o[qb][nd] = mfma8(vf, pb[qb], o[qb][nd]);
        }
    }
}

template <int QB, int KS>
__global__ __launch_bounds__(256 * KS) void attn_fwd8_kernel(AttnArgs a, int nx) {
    // [group][stage][K | V^T]; two groups: the merge exchange reuses it at the end; one group: the parked first state sits behind the ring
    __shared__ __attribute__((aligned(16))) uint8_t smem[KS == 1 ? 2 * 8192 + 4 * QB * 18 * 256 : (KS * 2 * 8192 > 4 * QB * 18 * 256 ? KS * 2 * 8192 : 4 * QB * 18 * 256)];
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, c = lane & 15;
    const int grp = KS > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 8) : 0;
    int xb, h, b;
    attn_block_coords(nx, a.H, a.B, xb, h, b);
    const int ld = 3 * a.D;
    const TileDma8 dma;
    const FragAddr8 fa(g, c);
    const int qbase = xb * (64 * QB) + dma.wave * (16 * QB);
    const bool active = qbase < a.Tld;
    const uint8_t* qkv_b = a.qkv8 + (size_t)b * a.Tld * ld;
    const uint8_t* kbase = qkv_b + a.D + h * 64;
    const uint8_t* vT = a.qkvT8 + (size_t)(2 * a.D + h * 64) * a.ldt8 + (size_t)b * a.Tld;
    u32x4 qf[QB];
    int qidx[QB];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        int q = qbase + qb * 16 + c;
        qidx[qb] = q;
        q = q < a.Tld ? q : a.Tld - 1;
        qf[qb] = *reinterpret_cast<const u32x4*>(qkv_b + (size_t)q * ld + h * 64 + g * 16);
    }
    auto issue = [&](int kt, uint8_t* st) {
        dma.token_tile(kbase, ld, kt, a.Tld - 1, st);
        dma.dim_tile(vT, a.ldt8, kt, a.Tld, st + 4096);
    };
    const int nt = (a.T + 63) / 64, per = (nt + 1) / 2;
    const int t0 = KS > 1 ? grp * per : 0, t1 = KS > 1 ? min(nt, t0 + per) : nt;
    uint8_t* ring = smem + grp * (2 * 8192);
    if (t0 < t1) issue(t0 * 64, ring);
    float m[QB], l[QB];
    f32x4 o[QB][4];
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        m[qb] = NEG_BIG;
        l[qb] = 0.f;
#pragma unroll
        for (int nd = 0; nd < 4; ++nd) o[qb][nd] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    const float c2 = a.scale * LOG2E;
    auto run_tile = [&](int tile, const uint8_t* cur) {
        const int kt = tile * 64;
        if (kt + 64 <= a.T) attn_fwd8_tile<QB, 2, false>(cur, cur + 4096, fa, qf, m, l, o, c2, kt, a.T, g);
        else if (kt + 32 < a.T) attn_fwd8_tile<QB, 2, true>(cur, cur + 4096, fa, qf, m, l, o, c2, kt, a.T, g);
        else attn_fwd8_tile<QB, 1, true>(cur, cur + 4096, fa, qf, m, l, o, c2, kt, a.T, g);
    };
    if (KS == 1) {
        // One group walks BOTH key ranges, one after the other, and merges the two softmax states with the arithmetic of the
        // two-group form below: bit for bit the same output (the batched launches keep their 4-wave workgroups -- many waves per
        // SIMD anyway -- without making a pass's result depend on the batch size).  The first state waits in LDS, lane for lane
        // (kept in registers it cost 40 VGPRs and a third of the batched kernel's speed).
        const int per2 = (nt + 1) / 2;
        float* park = reinterpret_cast<float*>(smem + 2 * 8192);   // [wave][QB][18][64], behind the ring
        auto walk = [&](int tb, int te) {
            for (int it = tb; it < te; ++it) {
                dma_wait_barrier();
                if (it + 1 < nt) issue((it + 1) * 64, ring + ((it + 1) & 1) * 8192);
                if (active) run_tile(it, ring + (it & 1) * 8192);
            }
        };
        walk(0, per2);
        if (nt > per2) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                float* e = park + ((dma.wave * QB + qb) * 18) * 64 + lane;
                e[0] = m[qb];
                e[64] = l[qb];
                m[qb] = NEG_BIG; l[qb] = 0.f;
#pragma unroll
                for (int nd = 0; nd < 4; ++nd) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) e[(2 + nd * 4 + r) * 64] = o[qb][nd][r];
                    o[qb][nd] = f32x4{0.f, 0.f, 0.f, 0.f};
                }
            }
            walk(per2, nt);
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                const float* e = park + ((dma.wave * QB + qb) * 18) * 64 + lane;
                const float m0 = e[0], l0 = e[64], m1 = m[qb], l1 = l[qb];
                const float mn = fmaxf(m0, m1);
                const float a0 = __builtin_amdgcn_exp2f(m0 - mn), a1 = __builtin_amdgcn_exp2f(m1 - mn);
                m[qb] = mn;
                l[qb] = merge2(l0, a0, l1, a1);
#pragma unroll
                for (int nd = 0; nd < 4; ++nd)
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[qb][nd][r] = merge2(e[(2 + nd * 4 + r) * 64], a0, o[qb][nd][r], a1);
            }
        }
    } else {
        for (int it = 0; it < per; ++it) {
            dma_wait_barrier();
            const int tile = t0 + it;
            if (tile + 1 < t1) issue((tile + 1) * 64, ring + ((it + 1) & 1) * 8192);
            if (active && tile < t1) run_tile(tile, ring + (it & 1) * 8192);
        }
        float* ex = reinterpret_cast<float*>(smem);   // [wave4][QB][18][64]
        __syncthreads();
        if (grp == 1) {
#pragma unroll
            for (int qb = 0; qb < QB; ++qb) {
                float* e = ex + ((dma.wave * QB + qb) * 18) * 64 + lane;
                e[0] = m[qb];
                e[64] = l[qb];
#pragma unroll
                for (int nd = 0; nd < 4; ++nd)
#pragma unroll
                    for (int r = 0; r < 4; ++r) e[(2 + nd * 4 + r) * 64] = o[qb][nd][r];
            }
        }
        __syncthreads();
        if (grp == 1) return;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) {
            const float* e = ex + ((dma.wave * QB + qb) * 18) * 64 + lane;
            const float m1 = e[0], l1 = e[64];
            const float mn = fmaxf(m[qb], m1);
            const float a0 = __builtin_amdgcn_exp2f(m[qb] - mn), a1 = __builtin_amdgcn_exp2f(m1 - mn);
            m[qb] = mn;
            l[qb] = merge2(l[qb], a0, l1, a1);
#pragma unroll
            for (int nd = 0; nd < 4; ++nd)
#pragma unroll
                for (int r = 0; r < 4; ++r) o[qb][nd][r] = merge2(o[qb][nd][r], a0, e[(2 + nd * 4 + r) * 64], a1);
        }
    }
    if (!active) return;
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
        const float lt = group4_sum(l[qb]);
        const int q = qidx[qb];
        if (q < a.Tld) {
            const float inv = 1.0f / lt;
            bf16_t* op = a.out + ((size_t)b * a.Tld + q) * a.D + h * 64 + g * 4;
#pragma unroll
            for (int nd = 0; nd < 4; ++nd) st4bf(op + nd * 16, o[qb][nd], inv);
            if (g == 0) a.lse[((size_t)b * a.H + h) * a.Tld + q] = m[qb] + __builtin_amdgcn_logf(lt);   // log2 units
        }
    }
}

// ---------------------------------------------------------------------------------------
// backward (same toolkit as the forward: LDS-DMA ring, one b128 read per MFMA operand, padding handled in a
// peeled last tile so the hot loops are branch-free).
//
// delta[b][h][q] = sum_d dO[q][h*64+d] * O[q][h*64+d] is an INPUT of both halves (the ViT engine forms it in the
// epilogue of the proj dgrad GEMM that produces dO; the stand-alone C entry point runs attn_delta_kernel first).
// dQ half: wave owns 16 queries (lane&15 = query); K, V (token tiles) and K^T (dim tile) shared via LDS.
template <int NSUB, bool MASK>
__device__ __forceinline__ void attn_bwd_q_tile(const bf16_t* Ks, const bf16_t* Vs, const FragAddr& fa,
                                                const u32x4 (&qf)[2], const u32x4 (&dof)[2], float lse_q, float del_q, f32x4 (&dq)[4],
                                                float c2, int kt, int T, int g) {
    f32x4 s[NSUB * 2], dp[NSUB * 2];
#pragma unroll
    for (int nb = 0; nb < NSUB * 2; ++nb) {
        const int off = (nb >> 1) * 2048 + (nb & 1) * 256;
        s[nb] = mfma16(lds16(Ks + fa.tok[0] + off), qf[0], f32x4{0.f, 0.f, 0.f, 0.f});      // S^T[key][q]
        dp[nb] = mfma16(lds16(Vs + fa.tok[0] + off), dof[0], f32x4{0.f, 0.f, 0.f, 0.f});    // dP^T[key][q]
        s[nb] = mfma16(lds16(Ks + fa.tok[1] + off), qf[1], s[nb]);
        dp[nb] = mfma16(lds16(Vs + fa.tok[1] + off), dof[1], dp[nb]);
    }
#pragma unroll
    for (int nb = 0; nb < NSUB * 2; ++nb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[nb][r], c2, -lse_q));
            if (MASK) p = kt + (nb >> 1) * 32 + g * 8 + (nb & 1) * 4 + r < T ? p : 0.f;
            dp[nb][r] = p * (dp[nb][r] - del_q);
        }
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
        const u32x4 dsb = pack8v(dp[sub * 2], dp[sub * 2 + 1]);
#pragma unroll
        for (int nd = 0; nd < 4; ++nd) dq[nd] = mfma16(lds_tr16(Ks, fa.tr[nd] + sub * 2048), dsb, dq[nd]);   // dQ^T[d][q]: K^T out of the K tile
    }
}

__device__ __forceinline__ float dot8bf(const u32x4& x, const u32x4& y) {
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        acc = __builtin_fmaf(__uint_as_float(x[j] << 16), __uint_as_float(y[j] << 16), acc);
        acc = __builtin_fmaf(__uint_as_float(x[j] & 0xFFFF0000u), __uint_as_float(y[j] & 0xFFFF0000u), acc);
    }
    return acc;
}

constexpr int Q_STAGE = 2 * 4096;   // bf16 elements per ring stage of the dQ half: K and V token tiles
// (Measured and not kept, round 3: a two-wave-group form of both halves -- the tile range split over two groups of 4 waves, partial
// sums added through LDS, as in the forward: 27.0 against 25.0 us at one pass of T = 785, 100 against 88 us at eight, equal at
// T = 3137 -- with 33 KB of LDS the one-group workgroups already sit four to a CU; and one loop over all tiles with the partial
// tile peeled behind it instead of in front: the same at one pair, +1.2 % step time at eight; a 3-stage ring (two tiles in flight,
// asm-issued DMA, counted waits) for the merged launch: +1.7 % step time at one pair, +1.3 % at two -- the one-pass launches are
// not waiting on the tile feed.)
template <int NW = 4>   // waves sharing the ring: 4 (64 queries per workgroup) or 8 (128; the two-launch form of chip-filling batches)
__device__ __forceinline__ void attn_bwd_q_body(const AttnArgs& a, int xb, int h, int b, bf16_t* smem /* [stage][K | V] */) {
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, c = lane & 15;
    const int ld = 3 * a.D;
    const TileDmaT<NW> dma;
    const FragAddr fa(g, c);
    const int qbase = xb * (16 * NW) + dma.wave * 16;
    const bool active = qbase < a.Tld;
    const int q = qbase + c;
    const int qc = q < a.Tld ? q : a.Tld - 1;
    const bf16_t* qkv_b = a.qkv + (size_t)b * a.Tld * ld;
    u32x4 qf[2], dof[2];
    {
        const bf16_t* pq = qkv_b + (size_t)qc * ld + h * 64 + g * 8;
        const bf16_t* pd = a.dout + ((size_t)b * a.Tld + qc) * a.D + h * 64 + g * 8;
        qf[0] = ld16v(pq); qf[1] = ld16v(pq + 32);
        dof[0] = ld16v(pd); dof[1] = ld16v(pd + 32);
    }
    const float lse_q = a.lse[((size_t)b * a.H + h) * a.Tld + qc];
    const float del_q = a.delta[((size_t)b * a.H + h) * a.Tld + qc];
    const bf16_t* krow = qkv_b + a.D + h * 64;
    const bf16_t* vrow = qkv_b + 2 * a.D + h * 64;
    const uint32_t koff = dma.token_off(ld);
    auto issue = [&](int kt, bf16_t* st) {
        if (kt + 64 <= a.Tld) {
            dma.fast_tile(krow + (size_t)kt * ld, koff, ld, st);
            dma.fast_tile(vrow + (size_t)kt * ld, koff, ld, st + 4096);
        } else {
            dma.token_tile(krow, ld, kt, a.Tld - 1, st);
            dma.token_tile(vrow, ld, kt, a.Tld - 1, st + 4096);
        }
    };
    issue(0, smem);
    f32x4 dq[4];
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) dq[nd] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float c2 = a.scale * LOG2E;
    const int nfull = a.T / 64;
    for (int it = 0; it < nfull; ++it) {
        dma_wait_barrier();
        const int kn = it * 64 + 64;
        if (kn < a.Tld) issue(kn, smem + ((it + 1) & 1) * Q_STAGE);
        if (active) {
            const bf16_t* cur = smem + (it & 1) * Q_STAGE;
            attn_bwd_q_tile<2, false>(cur, cur + 4096, fa, qf, dof, lse_q, del_q, dq, c2, it * 64, a.T, g);
        }
    }
    if (nfull * 64 < a.T) {
        dma_wait_barrier();
        const int kt = nfull * 64;
        if (active) {
            const bf16_t* cur = smem + (nfull & 1) * Q_STAGE;
            if (kt + 32 < a.T) attn_bwd_q_tile<2, true>(cur, cur + 4096, fa, qf, dof, lse_q, del_q, dq, c2, kt, a.T, g);
            else attn_bwd_q_tile<1, true>(cur, cur + 4096, fa, qf, dof, lse_q, del_q, dq, c2, kt, a.T, g);
        }
    }
    if (active && q < a.Tld) {
        bf16_t* p = a.dqkv + ((size_t)b * a.Tld + q) * ld + h * 64 + g * 4;
#pragma unroll
        for (int nd = 0; nd < 4; ++nd) st4bf(p + nd * 16, dq[nd], a.scale);
    }
}

// dK / dV kernel: wave owns 16 keys (lane&15 = key); the workgroup's 4 waves share 64-query tiles of Q, dO (token
// tiles) and Q^T, dO^T (dim tiles) plus lse / delta through LDS.  Padding keys accumulate garbage in their own
// lanes only (MFMA output columns are independent) and are stored as exact zeros.
#define KV_STAGE (2 * 4096 + 256)   // bf16 elements per ring stage: the Q and dO token tiles + 64 lse + 64 delta floats
template <int NSUB>
__device__ __forceinline__ void attn_bwd_kv_tile(const bf16_t* st, const FragAddr& fa, const u32x4 (&kf)[2], const u32x4 (&vf)[2],
                                                 f32x4 (&dk)[4], f32x4 (&dv)[4], float c2, int g) {
    const bf16_t *Qs = st, *Ds = st + 4096;
    const float* Ls = reinterpret_cast<const float*>(st + 8192);
    const float* Es = Ls + 64;
    f32x4 s[NSUB * 2], dp[NSUB * 2];
#pragma unroll
    for (int nb = 0; nb < NSUB * 2; ++nb) {
        const int off = (nb >> 1) * 2048 + (nb & 1) * 256;
        s[nb] = mfma16(lds16(Qs + fa.tok[0] + off), kf[0], f32x4{0.f, 0.f, 0.f, 0.f});      // S[q][key]
        dp[nb] = mfma16(lds16(Ds + fa.tok[0] + off), vf[0], f32x4{0.f, 0.f, 0.f, 0.f});     // dP[q][key]
        s[nb] = mfma16(lds16(Qs + fa.tok[1] + off), kf[1], s[nb]);
        dp[nb] = mfma16(lds16(Ds + fa.tok[1] + off), vf[1], dp[nb]);
    }
#pragma unroll
    for (int nb = 0; nb < NSUB * 2; ++nb) {
        const f32x4 ls = *reinterpret_cast<const f32x4*>(Ls + (nb >> 1) * 32 + g * 8 + (nb & 1) * 4);
        const f32x4 de = *reinterpret_cast<const f32x4*>(Es + (nb >> 1) * 32 + g * 8 + (nb & 1) * 4);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float p = __builtin_amdgcn_exp2f(__builtin_fmaf(s[nb][r], c2, -ls[r]));
            s[nb][r] = p;
            dp[nb][r] = p * (dp[nb][r] - de[r]);
        }
    }
#pragma unroll
    for (int sub = 0; sub < NSUB; ++sub) {
        const u32x4 pb = pack8v(s[sub * 2], s[sub * 2 + 1]), dsb = pack8v(dp[sub * 2], dp[sub * 2 + 1]);
#pragma unroll
        for (int nd = 0; nd < 4; ++nd) {
            dv[nd] = mfma16(lds_tr16(Ds, fa.tr[nd] + sub * 2048), pb, dv[nd]);    // dV^T[d][key]: dO^T out of the dO tile
            dk[nd] = mfma16(lds_tr16(Qs, fa.tr[nd] + sub * 2048), dsb, dk[nd]);   // dK^T[d][key]: Q^T out of the Q tile
        }
    }
}

template <int NW = 4>
__device__ __forceinline__ void attn_bwd_kv_body(const AttnArgs& a, int xb, int h, int b, bf16_t* smem /* 2 * KV_STAGE */) {
    const int lane = threadIdx.x & 63;
    const int g = lane >> 4, c = lane & 15;
    const int ld = 3 * a.D;
    const TileDmaT<NW> dma;
    const FragAddr fa(g, c);
    const int kbase = xb * (16 * NW) + dma.wave * 16;
    const bool active = kbase < a.Tld;
    const int key = kbase + c;
    const int keyc = key < a.Tld ? key : a.Tld - 1;
    const bf16_t* qkv_b = a.qkv + (size_t)b * a.Tld * ld;
    u32x4 kf[2], vf[2];
    {
        const bf16_t* pk = qkv_b + (size_t)keyc * ld + a.D + h * 64 + g * 8;
        const bf16_t* pv = qkv_b + (size_t)keyc * ld + 2 * a.D + h * 64 + g * 8;
        kf[0] = ld16v(pk); kf[1] = ld16v(pk + 32);
        vf[0] = ld16v(pv); vf[1] = ld16v(pv + 32);
    }
    const bf16_t* qrow = qkv_b + h * 64;
    const bf16_t* dorow = a.dout + (size_t)b * a.Tld * a.D + h * 64;
    const float* lse = a.lse + ((size_t)b * a.H + h) * a.Tld;
    const float* dl = a.delta + ((size_t)b * a.H + h) * a.Tld;
    const uint32_t qoff = dma.token_off(ld), dooff = dma.token_off(a.D);
    auto issue = [&](int qt, bf16_t* st) {
        if (qt + 64 <= a.Tld) {
            dma.fast_tile(qrow + (size_t)qt * ld, qoff, ld, st);
            dma.fast_tile(dorow + (size_t)qt * a.D, dooff, a.D, st + 4096);
        } else {
            dma.token_tile(qrow, ld, qt, a.Tld - 1, st);
            dma.token_tile(dorow, a.D, qt, a.Tld - 1, st + 4096);
        }
        if (dma.wave < 2) {   // wave 0: 64 lse values, wave 1: 64 delta values (4 bytes per lane)
            const int qq = qt + lane < a.Tld ? qt + lane : a.Tld - 1;
            const float* src = (dma.wave == 0 ? lse : dl) + qq;
            __builtin_amdgcn_global_load_lds((glb_void*)src, (lds_void*)(st + 8192 + dma.wave * 128), 4, 0, 0);
        }
    };
    issue(0, smem);
    f32x4 dk[4], dv[4];
#pragma unroll
    for (int nd = 0; nd < 4; ++nd) { dk[nd] = f32x4{0.f, 0.f, 0.f, 0.f}; dv[nd] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    const float c2 = a.scale * LOG2E;
    const int nfull = a.Tld / 64;   // padding QUERIES carry dO = 0, delta = 0: no masking needed inside Tld
    for (int it = 0; it < nfull; ++it) {
        dma_wait_barrier();
        const int qn = it * 64 + 64;
        if (qn < a.Tld) issue(qn, smem + ((it + 1) & 1) * KV_STAGE);
        if (active) attn_bwd_kv_tile<2>(smem + (it & 1) * KV_STAGE, fa, kf, vf, dk, dv, c2, g);
    }
    if (nfull * 64 < a.Tld) {   // Tld % 64 == 32: one more half tile (rows beyond Tld are clamped duplicates: skipped)
        dma_wait_barrier();
        if (active) attn_bwd_kv_tile<1>(smem + (nfull & 1) * KV_STAGE, fa, kf, vf, dk, dv, c2, g);
    }
    if (active && key < a.Tld) {
        const float sk = key < a.T ? a.scale : 0.f, sv = key < a.T ? 1.0f : 0.f;
        bf16_t* pk = a.dqkv + ((size_t)b * a.Tld + key) * ld + a.D + h * 64 + g * 4;
        bf16_t* pv = a.dqkv + ((size_t)b * a.Tld + key) * ld + 2 * a.D + h * 64 + g * 4;
#pragma unroll
        for (int nd = 0; nd < 4; ++nd) {
            st4bf(pk + nd * 16, dk[nd], sk);
            st4bf(pv + nd * 16, dv[nd], sv);
        }
    }
}

// One launch for the whole attention backward: the dQ and the dK/dV halves are independent given delta, so their
// workgroups are interleaved in one grid (even logical id = dQ block, odd = dK/dV block of the same (pass, head, block)
// triple, neighbours on one XCD) instead of two dependent launches of ~15 us each.
__global__ __launch_bounds__(256) void attn_bwd_kernel(AttnArgs a, int nx) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * KV_STAGE];
    const int n = nx * a.H * a.B;
    const int lid = xcd_remap(blockIdx.x, 2 * n);
    const int pair = lid >> 1;
    const int xb = pair % nx, bh = pair / nx;
    const int h = bh % a.H, b = bh / a.H;
    if (lid & 1) attn_bwd_kv_body(a, xb, h, b, smem);
    else attn_bwd_q_body(a, xb, h, b, smem);
}

template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_q_kernel(AttnArgs a, int nx) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * Q_STAGE];
    int xb, h, b;
    attn_block_coords(nx, a.H, a.B, xb, h, b);
    attn_bwd_q_body<NW>(a, xb, h, b, smem);
}
template <int NW>
__global__ __launch_bounds__(64 * NW) void attn_bwd_kv_kernel(AttnArgs a, int nx) {
    __shared__ __attribute__((aligned(16))) bf16_t smem[2 * KV_STAGE];
    int xb, h, b;
    attn_block_coords(nx, a.H, a.B, xb, h, b);
    attn_bwd_kv_body<NW>(a, xb, h, b, smem);
}

__global__ void attn_delta_kernel(AttnArgs a) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;  // over B*Tld*H
    if (idx >= a.B * a.Tld * a.H) return;
    const int h = idx % a.H, row = idx / a.H;
    const int b = row / a.Tld, q = row % a.Tld;
    const bf16_t* po = a.out + (size_t)row * a.D + h * 64;
    const bf16_t* pd = a.dout + (size_t)row * a.D + h * 64;
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) acc += dot8bf(ld16v(po + i * 8), ld16v(pd + i * 8));
    a.delta[((size_t)b * a.H + h) * a.Tld + q] = acc;
}

// attention probabilities of one layer, fp32 [B][H][T][T] (models/extractor.py:44-45,97-103);
// only materialised when the API asks for them.
__global__ void attn_probs_kernel(AttnArgs a, float* probs) {
    const int q = blockIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int ld = 3 * a.D;
    const bf16_t* qkv_b = a.qkv + (size_t)b * a.Tld * ld;
    const bf16_t* pq = qkv_b + (size_t)q * ld + h * 64;
    const float lse = a.lse[((size_t)b * a.H + h) * a.Tld + q];
    float qv[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) qv[d] = bf2f(pq[d]);
    float* out = probs + (((size_t)b * a.H + h) * a.T + q) * a.T;
    for (int key = threadIdx.x; key < a.T; key += blockDim.x) {
        const bf16_t* pk = qkv_b + (size_t)key * ld + a.D + h * 64;
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 64; ++d) s += qv[d] * bf2f(pk[d]);
        out[key] = __builtin_amdgcn_exp2f(s * a.scale * LOG2E - lse);
    }
}

// ---------------------------------------------------------------------------------------
// Launch policy.  No environment reads: the only switches are the two C-ABI hooks below (splice_attention_variant /
// splice_attention_bwd_variant), which the op-level tests use to force EVERY launch form the policy can pick and compare bits.
static int g_attn_variant = 0;       // forward: 0 automatic; 41 / 42 / 48 = the 32x32x16 kernel with 4 / 2 / 8 waves; e4m3 forward: queries per wave / 16 + 10 * (two wave groups)
void attn_set_variant(int v) { g_attn_variant = v; }
static int g_attn_qfold = 0;         // the stand-alone entry points take pre-scaled q (AttnArgs::qfold) when set
void attn_set_qfold(int on) { g_attn_qfold = on; }
int attn_qfold_hook() { return g_attn_qfold; }

// hipFuncSetAttribute once per (kernel, device): a flag per device ordinal, so a second device of the same process sets its own
struct AttrOnce {
    bool done[64] = {};
    void set(const void* fn, int bytes) {
        int dev = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= 64) { (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); return; }
        if (!done[dev]) { (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes); done[dev] = true; }
    }
};

template <int NW, bool FOLD>
static void attn_fwd_x32_go(const AttnArgs* a, hipStream_t s) {
    static AttrOnce attr;
    attr.set((const void*)attn_fwd_x32_kernel<NW, FOLD>, X32<NW>::LDS_BYTES);
    const int nx = cdiv(a->Tld, 32 * NW);
    SPLICE_LAUNCH((attn_fwd_x32_kernel<NW, FOLD>), dim3(nx * a->H * a->B), dim3(64 * NW), X32<NW>::LDS_BYTES, s, *a, nx);
}

// Every launcher below refuses what its kernels do not bound on their own -- no pass, no token, more tokens than the row pitch holds, a NULL
// operand -- before anything is launched (the kernels clamp rows to Tld - 1 and mask keys against T; T > Tld would walk past the buffers).
static bool attn_shape_bad(const AttnArgs* a) {
    return a->B < 1 || a->T < 1 || a->T > a->Tld || a->Tld % 32 || a->D % 64 || a->D / 64 != a->H;
}

int attn_fwd_launch(const AttnArgs* a, hipStream_t s) {
    if (attn_shape_bad(a) || !a->out || !a->lse || (!a->qkv && !a->qkv8)) return SPLICE_ERR_ARG;
    if (!a->qkv8) {
        // bf16: the 32x32x16 kernel (attn_x32.h), four waves (128 queries) per workgroup.  Every form of it gives a query the same bits
        // (the arithmetic does not depend on the wave count: tests/test_ops_gpu.py forces 2 / 4 / 8), so a pass's output does not
        // depend on how many passes share the launch.  The 16x16x32 forms of rounds 1-4 and the ping-pong form of round 5
        // (profiles/r05_attn_pp1.txt: 0.93 x) are gone from the library; their records stay in profiles/ and DESIGN section 8.
        const int nwv = g_attn_variant / 10 == 4 ? g_attn_variant % 10 : 4;
        if (a->qfold) { if (nwv == 2) attn_fwd_x32_go<2, true>(a, s); else if (nwv == 8) attn_fwd_x32_go<8, true>(a, s); else attn_fwd_x32_go<4, true>(a, s); }
        else { if (nwv == 2) attn_fwd_x32_go<2, false>(a, s); else if (nwv == 8) attn_fwd_x32_go<8, false>(a, s); else attn_fwd_x32_go<4, false>(a, s); }
        return SPLICE_OK;
    }
    // e4m3 forward (configs[4]): 16 or 32 queries per wave, the key range walked by one wave group or by two side by side (same bits from all
    // four forms, tests/test_fp8_gpu.py).  Policy measured in the step (profiles/r03_attn_fwd_forms_in_step.txt): two groups until the launch
    // fills the chip (more than 512 workgroups) on short key walks; 32 queries per wave only for very long batches.
    if (!a->qkvT8 || a->ldt8 % 16 || a->D % 16) return SPLICE_ERR_ARG;
    const long tasks = (long)a->B * a->H * cdiv(a->Tld, 16);
    const int qb = g_attn_variant ? g_attn_variant % 10 : (tasks > 60000 ? 2 : 1);
    const long wgs = (long)cdiv(a->Tld, 64 * qb) * a->H * a->B;
    const int ks = g_attn_variant ? (g_attn_variant / 10 == 1 ? 2 : 1) : ((wgs > 512 && a->T <= 2048) ? 1 : 2);
    const int nx = cdiv(a->Tld, 64 * qb);
    const dim3 grid(nx * a->H * a->B);
    if (ks == 2) {
        if (qb == 2) SPLICE_LAUNCH((attn_fwd8_kernel<2, 2>), grid, dim3(512), 0, s, *a, nx);
        else SPLICE_LAUNCH((attn_fwd8_kernel<1, 2>), grid, dim3(512), 0, s, *a, nx);
    } else {
        if (qb == 2) SPLICE_LAUNCH((attn_fwd8_kernel<2, 1>), grid, dim3(256), 0, s, *a, nx);
        else SPLICE_LAUNCH((attn_fwd8_kernel<1, 1>), grid, dim3(256), 0, s, *a, nx);
    }
    return SPLICE_OK;
}

// backward hook: 0 automatic; 1 = the 16x16x32 halves (what plain, un-scaled q gets in any case); 2 / 3 = the 32x32x16 halves in one / two
// launches (pre-scaled q only); 4 = the 32x32x16 halves, one launch of two-wave workgroups
static int g_attn_bwd_variant = 0;
void attn_set_bwd_variant(int v) { g_attn_bwd_variant = v; }
static const int kAttnBwdMergeMaxX32 = 1400;   // workgroups of the merged 32x32x16 launch up to which ONE launch is used (round 6: 1024 -> 1400, profiles/r06_attn_bwd_merge.txt:
                                               // 8 passes of T = 785 = 1344 workgroups 84.2 us merged against 90.8 in two launches, 2 passes of T = 3137 = 1200: 234.6 against 254.4; beyond ~2000 a wash)
static const int kAttnBwdMergeMax16 = 768;     // the same bound for the 16x16x32 halves

int attn_bwd_launch(const AttnArgs* a, hipStream_t s) {
    if (attn_shape_bad(a) || !a->qkv || !a->lse || !a->dout || !a->delta || !a->dqkv || (!a->delta_ready && !a->out)) return SPLICE_ERR_ARG;
    const int nx = cdiv(a->Tld, 64);
    if (!a->delta_ready) SPLICE_LAUNCH(attn_delta_kernel, dim3(cdiv(a->B * a->Tld * a->H, 256)), dim3(256), 0, s, *a);
    if (a->qfold && g_attn_bwd_variant != 1) {   // the 32x32x16 halves (attn_bwd_x32.h): what the engine runs
        static AttrOnce at_m, at_q, at_kv, at_m2;
        at_m.set((const void*)attn_bwd_x32_kernel<4>, BX_KV_LDS);
        at_q.set((const void*)attn_bwd_q_x32_kernel<4>, BX_Q_LDS);
        at_kv.set((const void*)attn_bwd_kv_x32_kernel<4>, BX_KV_LDS);
        if (g_attn_bwd_variant == 4) {   // two waves (64 queries / keys) per workgroup: twice the workgroups, same bits (tested; not selected by the policy)
            at_m2.set((const void*)attn_bwd_x32_kernel<2>, BX_KV_LDS);
            const int nx2 = cdiv(a->Tld, 64), n2 = nx2 * a->H * a->B;
            SPLICE_LAUNCH((attn_bwd_x32_kernel<2>), dim3(2 * n2), dim3(128), BX_KV_LDS, s, *a, nx2);
            return SPLICE_OK;
        }
        const int nx4 = cdiv(a->Tld, 128), n4 = nx4 * a->H * a->B;
        // both forms run the same bodies (same bits, tested at op level and through the multi-pair step): one launch while the chip is not
        // full anyway (a dependent launch costs more than the mix of the two halves' durations), two once every CU holds several workgroups
        // (T = 3137, 4 passes = 2400 workgroups: 426 against 445 us; 2 passes of T = 785: 37.9 against 32.7 us; profiles/r05_attn_bwd_x32.txt)
        if (g_attn_bwd_variant == 3 || (g_attn_bwd_variant != 2 && 2 * n4 > kAttnBwdMergeMaxX32)) {
            SPLICE_LAUNCH((attn_bwd_q_x32_kernel<4>), dim3(n4), dim3(256), BX_Q_LDS, s, *a, nx4);
            SPLICE_LAUNCH((attn_bwd_kv_x32_kernel<4>), dim3(n4), dim3(256), BX_KV_LDS, s, *a, nx4);
        } else SPLICE_LAUNCH((attn_bwd_x32_kernel<4>), dim3(2 * n4), dim3(256), BX_KV_LDS, s, *a, nx4);
        return SPLICE_OK;
    }
    // plain q (the op-level C-ABI without splice_attention_qfold): the 16x16x32 halves; one launch while the chip is not full anyway,
    // two once every CU has several workgroups
    const int n = nx * a->H * a->B;
    if (2 * n <= kAttnBwdMergeMax16) {
        SPLICE_LAUNCH(attn_bwd_kernel, dim3(2 * n), dim3(256), 0, s, *a, nx);
    } else {
        SPLICE_LAUNCH(attn_bwd_q_kernel<4>, dim3(n), dim3(256), 0, s, *a, nx);
        SPLICE_LAUNCH(attn_bwd_kv_kernel<4>, dim3(n), dim3(256), 0, s, *a, nx);
    }
    return SPLICE_OK;
}

int attn_probs_launch(const AttnArgs* a, float* probs, hipStream_t s) {
    if (attn_shape_bad(a) || !a->qkv || !a->lse || !probs) return SPLICE_ERR_ARG;
    dim3 grid(a->T, a->H, a->B);
    SPLICE_LAUNCH(attn_probs_kernel, grid, dim3(128), 0, s, *a, probs);
    return SPLICE_OK;
}
