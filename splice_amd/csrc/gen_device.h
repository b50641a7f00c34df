// Device helpers and segment geometry shared by the generator kernel families (gen_conv.hip, gen_wgrad.hip, gen_bn.hip,
// gen_pointwise.hip).  Private to those units: the host-side interface is gen_kernels.h.
#pragma once
#include "gen_kernels.h"

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    // A: lane l holds A[i = l&15][k = l>>4];  B: lane l holds B[k = l>>4][n = l&15]
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// 16-byte accesses at 4-byte alignment (gfx950's global accesses need dword alignment only): runs of 4 consecutive pixels of odd-sized planes
typedef float f4u __attribute__((ext_vector_type(4), aligned(4)));
// run k of this thread inside the segment [lo, hi): pixels i .. i + 3, i = lo + 4 (threadIdx.x + 256 k); pixels behind `hi` read as 0
__device__ __forceinline__ void ld_run(const float* __restrict__ p, int i, int hi, float (&v)[4]) {
    if (i + 3 < hi) {
        const f4u t = *(const f4u*)(p + i);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = i + j < hi ? p[i + j] : 0.f;
    }
}
__device__ __forceinline__ void st_run(float* __restrict__ p, int i, int hi, const float (&v)[4]) {
    if (i + 3 < hi) {
        f4u t; t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *(f4u*)(p + i) = t;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i + j < hi) p[i + j] = v[j];
    }
}

// width of the 3x3 tile kernels' output tile and of its staged input patch (conv3x3_tile_kernel, conv_wgrad_tile_kernel)
constexpr int CT_TW = 64, CT_PW = CT_TW + 2;

// block-wide fixed-order sum of two values (256 threads)
__device__ __forceinline__ void block_sum2(float& a, float& b, float* red) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[4 + w] = b; }
    __syncthreads();
    a = red[0] + red[1] + red[2] + red[3];
    b = red[4] + red[5] + red[6] + red[7];
}

// Plane reductions run in two deterministic stages so that planes with few channels still fill the
// chip: stage 1 = PB workgroups per (image, channel) plane write partials; stage 2 = the consuming
// element-wise kernel recombines the <= 64 partials in a fixed order in its prologue.
constexpr int MAX_PB = 64;
// Planes of more than 64 x 1024 pixels (every 448^2 / 512^2 / 900^2 layer; round 5): up to MAX_PB_V segments of <= BN_V_CH x 1024 pixels whose
// length is a multiple of 4, so that a thread owns runs of 4 consecutive pixels and moves them as ONE 16-byte access (4-byte aligned:
// gfx950's global accesses need dword alignment only, so odd plane sizes -- the random 855 .. 900 crops -- need no peeling).  A segment
// count above MAX_PB is what selects that layout everywhere (seg_len, the combines); the 224^2 layers keep theirs, bit for bit.
constexpr int MAX_PB_V = 256;
constexpr int BN_V_CH = 5;   // 16-byte runs a thread holds: 5 x 4 x 256 = 5120 pixels per segment at most (1.31 M pixel planes)
__host__ __device__ inline int seg_len(int HW, int PB) {
    const int s = (HW + PB - 1) / PB;
    return PB > MAX_PB ? (s + 3) & ~3 : s;
}
// 512-pixel segments (tuned in-step with alternating runs: 1024 +0.45 %, 256 / 384 +0.1 %, 2048 +1.3 %)
static inline int plane_blocks(int HW) { int b = cdiv(HW, 512); return b < 1 ? 1 : (b > MAX_PB ? MAX_PB : b); }

// x2 bilinear (align_corners=False) source coordinates of output o, and one upsampled value from a plane p[h][w] (global
// or LDS): the expression order of upsample2x_fwd_kernel
__device__ __forceinline__ void up_coord(int o, int n, int& i0, int& i1, float& lam) {
    float src = ((float)o + 0.5f) * 0.5f - 0.5f;
    src = src < 0.f ? 0.f : src;
    i0 = (int)src;
    i1 = i0 + 1 < n ? i0 + 1 : n - 1;
    lam = src - (float)i0;
}
template <class P>
__device__ __forceinline__ float up_value(P p, int h, int w, int oy, int ox) {
    int y0, y1, x0, x1;
    float ly, lx;
    up_coord(oy, h, y0, y1, ly);
    up_coord(ox, w, x0, x1, lx);
    const float top = p[y0 * w + x0] * (1.f - lx) + p[y0 * w + x1] * lx;
    const float bot = p[y1 * w + x0] * (1.f - lx) + p[y1 * w + x1] * lx;
    return top * (1.f - ly) + bot * ly;
}
__device__ __forceinline__ void up_adjoint_weights(int m, int n, int No, float (&wt)[4]) {
    wt[0] = m > 0 ? 0.25f : 0.f;                  // o = 2m-1 (odd output of input m-1, upper neighbour = m)
    wt[1] = m > 0 ? 0.75f : 1.0f;                 // o = 2m   (source m - 1/4, clamped to 0 at the border)
    wt[2] = m < n - 1 ? 0.75f : 1.0f;             // o = 2m+1 (source m + 1/4, upper neighbour clamped to n-1)
    wt[3] = m < n - 1 ? 0.25f : 0.f;              // o = 2m+2 (even output of input m+1, lower neighbour = m)
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (2 * m - 1 + t >= No) wt[t] = 0.f;
}
// adjoint of the above for input pixel (my, mx), read from the output-sized gradient plane p[Ho][Wo] (upsample2x_bwd_kernel)
template <class P>
__device__ __forceinline__ float up_adjoint_value(P p, int h, int w, int Ho, int Wo, int my, int mx) {
    float wy[4], wx[4];
    up_adjoint_weights(my, h, Ho, wy);
    up_adjoint_weights(mx, w, Wo, wx);
    float t[4][4];
#pragma unroll
    for (int ty = 0; ty < 4; ++ty) {
        const int oy = min(max(2 * my - 1 + ty, 0), Ho - 1);
#pragma unroll
        for (int tx = 0; tx < 4; ++tx) t[ty][tx] = p[oy * Wo + min(max(2 * mx - 1 + tx, 0), Wo - 1)];
    }
    float acc = 0.f;
#pragma unroll
    for (int ty = 0; ty < 4; ++ty) {
        float row = 0.f;
#pragma unroll
        for (int tx = 0; tx < 4; ++tx) row += wx[tx] != 0.f ? wx[tx] * t[ty][tx] : 0.f;
        acc += wy[ty] != 0.f ? wy[ty] * row : 0.f;
    }
    return acc;
}
