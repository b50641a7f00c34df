// Train-mode BatchNorm (+ LeakyReLU) of the generator, forward and backward, in four kernel forms by plane size (bn_form), and the
// running-statistics update (see gen_conv.hip for the family overview).
#include "gen_device.h"
#include "plateau.h"
#include <atomic>
#include <cstdlib>

// ---------------------------------------------------------------------------------------
// fixed-order sum of component `comp` of the PB per-segment pairs of a plane by one wave (PB <= 64: lane b holds segment b, as before)
__device__ __forceinline__ float part_sum(const float* __restrict__ pp, int PB, int comp, int lane) {
    if (PB <= MAX_PB) return wave_sum(lane < PB ? pp[2 * lane + comp] : 0.f);
    float a = 0.f;
    for (int b = lane; b < PB; b += 64) a += pp[2 * b + comp];
    return wave_sum(a);
}

// stage 1 of the BN statistics: per-segment (count, mean, M2), two-pass inside the segment
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(const float* y, size_t nstride, int C, int HW, int PB,
                                                               float* __restrict__ part /* [N][C][PB][2] */, BnUpsample up) {
    __shared__ float red[8];
    const int pb = blockIdx.x, c = blockIdx.y, img = blockIdx.z;
    const int seg = seg_len(HW, PB), lo = pb * seg, hi = min(lo + seg, HW);
    const float* p = y + (size_t)img * nstride + (size_t)c * HW;
    float s = 0.f, dummy = 0.f;
    // segments of up to 1024 elements (every plane up to 256 x 256) stay in registers between the two passes: the second pass
    // used to re-read them (a dependent L2 round trip per workgroup); same values, same order of additions, same bits
    const bool in_regs = seg <= 1024;
    float keep[4] = {0.f, 0.f, 0.f, 0.f};
    if (up.src && c >= up.c0) {   // upsampled channel: the values are produced here (and stored: the apply kernel and the backward read them)
        const float* sp = up.src + (size_t)img * up.src_ns + (size_t)(c - up.c0) * up.h * up.w;
        float* yo = const_cast<float*>(p);
        if (in_regs) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = lo + threadIdx.x + k * 256;
                if (i < hi) {
                    const float v = up_value(sp, up.h, up.w, i / up.Wo, i % up.Wo);
                    yo[i] = v;
                    keep[k] = v;
                    s += v;
                }
            }
        } else {
            for (int i = lo + threadIdx.x; i < hi; i += 256) {
                const float v = up_value(sp, up.h, up.w, i / up.Wo, i % up.Wo);
                yo[i] = v;
                s += v;
            }
        }
    } else if (in_regs) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = lo + threadIdx.x + k * 256;
            keep[k] = i < hi ? p[i] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lo + threadIdx.x + k * 256 < hi) s += keep[k];
    } else {
        for (int i = lo + threadIdx.x; i < hi; i += 256) s += p[i];
    }
    block_sum2(s, dummy, red);
    const int cnt = hi - lo;
    const float m = cnt > 0 ? s / (float)cnt : 0.f;
    float sq = 0.f;
    dummy = 0.f;
    if (in_regs) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (lo + threadIdx.x + k * 256 < hi) { const float d = keep[k] - m; sq = __builtin_fmaf(d, d, sq); }
    } else {
        for (int i = lo + threadIdx.x; i < hi; i += 256) { const float d = p[i] - m; sq = __builtin_fmaf(d, d, sq); }
    }
    block_sum2(sq, dummy, red);
    if (threadIdx.x == 0) {
        float* o = part + (((size_t)img * C + c) * PB + pb) * 2;
        o[0] = m;
        o[1] = sq;
    }
}

// the same stage for the big planes (PB > MAX_PB): the segment sits in registers as BN_V_CH runs of 4 pixels per thread, loaded (or, for an
// upsampled channel, produced and stored) with 16-byte accesses that are all in flight before the first sum
__global__ __launch_bounds__(256) void bn_stats_partial_v_kernel(const float* y, size_t nstride, int C, int HW, int PB,
                                                                 float* __restrict__ part /* [N][C][PB][2] */, BnUpsample up) {
    __shared__ float red[8];
    const int pb = blockIdx.x, c = blockIdx.y, img = blockIdx.z;
    const int seg = seg_len(HW, PB), lo = pb * seg, hi = min(lo + seg, HW);
    const float* p = y + (size_t)img * nstride + (size_t)c * HW;
    float keep[BN_V_CH][4];
    if (up.src && c >= up.c0) {
        const float* sp = up.src + (size_t)img * up.src_ns + (size_t)(c - up.c0) * up.h * up.w;
        float* yo = const_cast<float*>(p);
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k) {
            const int i = lo + 4 * (threadIdx.x + 256 * k);
            int oy = i / up.Wo, ox = i - oy * up.Wo;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                keep[k][j] = i + j < hi ? up_value(sp, up.h, up.w, oy, ox) : 0.f;
                if (++ox == up.Wo) { ox = 0; ++oy; }
            }
            if (i < hi) st_run(yo, i, hi, keep[k]);
        }
    } else {
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k) ld_run(p, lo + 4 * (threadIdx.x + 256 * k), hi, keep[k]);
    }
    float s = 0.f, dummy = 0.f;
#pragma unroll
    for (int k = 0; k < BN_V_CH; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) s += keep[k][j];   // (pixels behind `hi` are zeros)
    block_sum2(s, dummy, red);
    const int cnt = hi - lo;
    const float m = cnt > 0 ? s / (float)cnt : 0.f;
    float sq = 0.f;
    dummy = 0.f;
#pragma unroll
    for (int k = 0; k < BN_V_CH; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lo + 4 * ((int)threadIdx.x + 256 * k) + j < hi) { const float d = keep[k][j] - m; sq = __builtin_fmaf(d, d, sq); }
    block_sum2(sq, dummy, red);
    if (threadIdx.x == 0) {
        float* o = part + (((size_t)img * C + c) * PB + pb) * 2;
        o[0] = m;
        o[1] = sq;
    }
}

// Chan et al. pairwise combination of the <= 64 segment statistics by ONE wave: lane b holds segment b, a fixed
// binary tree (lane l absorbs lane l + off, off = 32 .. 1) leaves the plane's (mean, M2) in lane 0.  Deterministic, and
// ~100 cycles instead of a 49-step dependent chain in front of every workgroup of the apply kernel.
__device__ __forceinline__ void bn_combine_wave_raw(const float* part, int PB, int HW, float& mean, float& M2out);
__device__ __forceinline__ void bn_combine_wave(const float* part, int PB, int HW, float eps, float& mean, float& rstd) {
    float M2;
    bn_combine_wave_raw(part, PB, HW, mean, M2);
    rstd = rsqrtf(M2 / (float)HW + eps);
}
// (mean, M2) of one plane from its <= 64 segment statistics; every lane returns lane 0's result
__device__ __forceinline__ void bn_combine_wave_raw(const float* part, int PB, int HW, float& mean, float& M2out) {
    const int lane = threadIdx.x & 63;
    const int seg = seg_len(HW, PB), lo = lane * seg;
    int cnt = lane < PB ? min(lo + seg, HW) - lo : 0;
    cnt = cnt > 0 ? cnt : 0;
    float n = (float)cnt, m = cnt > 0 ? part[2 * lane] : 0.f, M2 = cnt > 0 ? part[2 * lane + 1] : 0.f;
    if (PB > MAX_PB) {   // big planes: lane l first merges its G consecutive segments l G .. l G + G - 1 in order, then the same tree
        const int G = (PB + 63) >> 6;
        n = 0.f; m = 0.f; M2 = 0.f;
        for (int g = 0; g < G; ++g) {
            const int b = lane * G + g, blo = b * seg;
            const int bc = b < PB ? min(blo + seg, HW) - blo : 0;
            if (bc > 0) {
                const float nb = (float)bc, mb = part[2 * b], Mb = part[2 * b + 1];
                const float nt = n + nb, d = mb - m, w = nb / nt;
                m += d * w;
                M2 += Mb + d * d * n * w;
                n = nt;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float nb = __shfl_down(n, off, 64), mb = __shfl_down(m, off, 64), Mb = __shfl_down(M2, off, 64);
        const float nt = n + nb;
        if (nb > 0.f) {
            const float d = mb - m, w = nb / nt;
            m += d * w;
            M2 += Mb + d * d * n * w;
            n = nt;
        }
    }
    mean = __shfl(m, 0, 64);
    M2out = __shfl(M2, 0, 64);
}
// The BatchNorm kernels' `batch`: 0 = per-image statistics; > 0 = statistics over groups of `batch` consecutive images (one netG call on
// the crops of one pair: batch = N for a single pair, n_crops per pair for several pairs side by side).  Image img reads its parameters at
// + bn_arena(...): its own arena (independent images), its group's arena (grouped images) or the one arena (p_nstride == 0).
__device__ __forceinline__ size_t bn_arena(int img, size_t p_nstride, int batch) { return (size_t)(batch ? img / batch : img) * p_nstride; }
// batch statistics (nn.BatchNorm2d over a batch of N images, models/unet/common.py:95-96 when netG is fed n_crops > 1
// crops at once): Chan merge of the N planes' (mean, M2) in image order
__device__ __forceinline__ void bn_combine_batch(const float* part_c0 /* image 0, channel c */, size_t img_stride, int N, int PB, int HW, float eps,
                                                 float& mean, float& rstd) {
    float n = 0.f, m = 0.f, M2 = 0.f;
    for (int i = 0; i < N; ++i) {
        float mb, Mb;
        bn_combine_wave_raw(part_c0 + (size_t)i * img_stride, PB, HW, mb, Mb);
        const float nb = (float)HW, nt = n + nb, d = mb - m, w = nb / nt;
        m += d * w;
        M2 += Mb + d * d * n * w;
        n = nt;
    }
    mean = m;
    rstd = rsqrtf(M2 / n + eps);
}

// the affine map of the big-plane forward with its two roundings pinned (one fma each), so that the backward can re-form the pre-activation
// value from y, mean, rstd, gamma, beta to the bit and read the activation's sign off it instead of loading the activated tensor
__device__ __forceinline__ float bn_shift(float beta, float mean, float sc) { return __builtin_fmaf(-mean, sc, beta); }
__device__ __forceinline__ float bn_affine(float y, float sc, float sh) { return __builtin_fmaf(y, sc, sh); }
// stage 2 + apply: a = act(gamma * (y - mean) * rstd + beta), written to a channel slice of `out`
__global__ __launch_bounds__(256) void bn_act_kernel(const float* __restrict__ y, size_t y_nstride, float* __restrict__ out,
                                                     size_t out_nstride, int C, int HW, int PB, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ part, float eps,
                                                     float* __restrict__ mean_o, float* __restrict__ rstd_o, float slope, size_t p_nstride, int batch) {
    __shared__ float st[2];
    const int c = blockIdx.y, img = blockIdx.z;
    gamma += bn_arena(img, p_nstride, batch); beta += bn_arena(img, p_nstride, batch);
    if (threadIdx.x < 64) {
        float m, r;
        if (batch) bn_combine_batch(part + ((size_t)(img / batch * batch) * C + c) * PB * 2, (size_t)C * PB * 2, batch, PB, HW, eps, m, r);
        else bn_combine_wave(part + ((size_t)img * C + c) * PB * 2, PB, HW, eps, m, r);
        if (threadIdx.x == 0) {
            st[0] = m; st[1] = r;
            if (blockIdx.x == 0) { mean_o[img * C + c] = m; rstd_o[img * C + c] = r; }
        }
    }
    __syncthreads();
    const float sc = gamma[c] * st[1];
    const float sh = beta[c] - st[0] * sc;
    const float* p = y + (size_t)img * y_nstride + (size_t)c * HW;
    float* q = out + (size_t)img * out_nstride + (size_t)c * HW;
    if (PB > MAX_PB) {   // big planes: the workgroup's own segment as 16-byte runs, all loads in flight before the first store
        const int seg = seg_len(HW, PB), lo = blockIdx.x * seg, hi = min(lo + seg, HW);
        float v[BN_V_CH][4];
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k) ld_run(p, lo + 4 * (threadIdx.x + 256 * k), hi, v[k]);
        const float shv = bn_shift(beta[c], st[0], sc);
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k) {
            const int i = lo + 4 * (threadIdx.x + 256 * k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = bn_affine(v[k][j], sc, shv);   // (the backward of these planes re-forms t from y to get the activation's sign)
                v[k][j] = t > 0.f ? t : t * slope;
            }
            if (i < hi) st_run(q, i, hi, v[k]);
        }
        return;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        const float v = p[i] * sc + sh;
        q[i] = v > 0.f ? v : v * slope;
    }
}

// BN backward stage 1: per-segment s1 = sum dz, s2 = sum dz * xhat, dz = da * act'(a)
__global__ __launch_bounds__(256) void bn_bwd_partial_kernel(const float* __restrict__ da, size_t da_nstride, const float* __restrict__ aout,
                                                             size_t a_nstride, const float* __restrict__ y, size_t y_nstride, int C, int HW,
                                                             int PB, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                             float slope, float* __restrict__ part /* [N][C][PB][2] */,
                                                             const float* __restrict__ gamma, const float* __restrict__ beta, size_t p_nstride) {
    __shared__ float red[8];
    const int pb = blockIdx.x, c = blockIdx.y, img = blockIdx.z;
    const int seg = seg_len(HW, PB), lo = pb * seg, hi = min(lo + seg, HW);
    const float m = mean[img * C + c], r = rstd[img * C + c];
    const float* pd = da + (size_t)img * da_nstride + (size_t)c * HW;
    const float* pa = aout + (size_t)img * a_nstride + (size_t)c * HW;
    const float* py = y + (size_t)img * y_nstride + (size_t)c * HW;
    float s1 = 0.f, s2 = 0.f;
    if (PB > MAX_PB) {
        const bool act = slope != 1.0f, from_y = act && beta != nullptr;   // the activation's sign from y (bn_affine): one tensor less to read
        float d[BN_V_CH][4], a[BN_V_CH][4], yy[BN_V_CH][4];
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k) {
            const int i = lo + 4 * (threadIdx.x + 256 * k);
            ld_run(pd, i, hi, d[k]);
            ld_run(py, i, hi, yy[k]);
            if (act && !from_y) ld_run(pa, i, hi, a[k]);
        }
        float sc = 0.f, sh = 0.f;
        if (from_y) { sc = gamma[(size_t)img * p_nstride + c] * r; sh = bn_shift(beta[(size_t)img * p_nstride + c], m, sc); }
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) {   // (pixels behind `hi`: dz = 0 adds nothing to either sum)
                float dz = d[k][j];
                const float av = from_y ? bn_affine(yy[k][j], sc, sh) : a[k][j];
                if (act && !(av > 0.f)) dz *= slope;
                s1 += dz;
                s2 += dz * (yy[k][j] - m) * r;
            }
    } else
    for (int i = lo + threadIdx.x; i < hi; i += 256) {
        float dz = pd[i];
        if (slope != 1.0f && !(pa[i] > 0.f)) dz *= slope;
        s1 += dz;
        s2 += dz * (py[i] - m) * r;
    }
    block_sum2(s1, s2, red);
    if (threadIdx.x == 0) {
        float* o = part + (((size_t)img * C + c) * PB + pb) * 2;
        o[0] = s1;
        o[1] = s2;
    }
}

// stage 2 + apply: dy = gamma * rstd * (dz - s1/HW - xhat * s2/HW); also dgamma/dbeta (sum over images)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ da, size_t da_nstride, const float* __restrict__ aout,
                                                           size_t a_nstride, const float* __restrict__ y, size_t y_nstride,
                                                           float* __restrict__ dy, size_t dy_nstride, int C, int HW, int N, int PB,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float slope, const float* __restrict__ part,
                                                           float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate, size_t p_nstride, int batch,
                                                           const float* __restrict__ beta) {
    __shared__ float st[2];
    const int c = blockIdx.y, img = blockIdx.z;
    gamma += bn_arena(img, p_nstride, batch);
    if (threadIdx.x < 64) {   // one wave: lane k holds segment k (PB <= 64), fixed-order tree sums
        const int lane = threadIdx.x;
        const float* pp = part + ((size_t)img * C + c) * PB * 2;
        const float a = part_sum(pp, PB, 0, lane), b = part_sum(pp, PB, 1, lane);
        if (lane == 0) { st[0] = a; st[1] = b; }
        if (p_nstride) {   // independent images: every image owns its parameter gradients (the sums of the N = 1 path: 0 + x); grouped: below
            if (!batch && blockIdx.x == 0 && lane == 0) {
                float* dg = dgamma + (size_t)img * p_nstride + c;
                float* db = dbeta + (size_t)img * p_nstride + c;
                const float g = 0.f + b, be = 0.f + a;
                *dg = accumulate ? *dg + g : g;
                *db = accumulate ? *db + be : be;
            }
        } else if (img == 0 && blockIdx.x == 0) {   // parameter gradients: sum over the images in order
            float g = 0.f, be = 0.f;
            for (int n = 0; n < N; ++n) {
                const float* pn = part + ((size_t)n * C + c) * PB * 2;
                be += part_sum(pn, PB, 0, lane);
                g += part_sum(pn, PB, 1, lane);
            }
            if (lane == 0) {
                dgamma[c] = accumulate ? dgamma[c] + g : g;
                dbeta[c] = accumulate ? dbeta[c] + be : be;
            }
        }
    }
    if (batch && threadIdx.x < 64) {   // batch statistics: the two sums run over every image of the batch / group (image order)
        const int lane = threadIdx.x, n0 = img / batch * batch;
        float a = 0.f, b = 0.f;
        for (int n = 0; n < batch; ++n) {
            const float* pn = part + ((size_t)(n0 + n) * C + c) * PB * 2;
            a += part_sum(pn, PB, 0, lane);
            b += part_sum(pn, PB, 1, lane);
        }
        if (lane == 0) {
            st[0] = a; st[1] = b;
            if (p_nstride && img == n0 && blockIdx.x == 0) {   // grouped: the group's parameter gradients are these sums (those of the one-group path)
                float* dg = dgamma + bn_arena(img, p_nstride, batch) + c;
                float* db = dbeta + bn_arena(img, p_nstride, batch) + c;
                *dg = accumulate ? *dg + b : b;
                *db = accumulate ? *db + a : a;
            }
        }
    }
    __syncthreads();
    const float m = mean[img * C + c], r = rstd[img * C + c];
    const float cnt = batch ? (float)HW * (float)batch : (float)HW;
    const float k1 = st[0] / cnt, k2 = st[1] / cnt;
    const float gr = gamma[c] * r;
    const float* pd = da + (size_t)img * da_nstride + (size_t)c * HW;
    const float* pa = aout + (size_t)img * a_nstride + (size_t)c * HW;
    const float* py = y + (size_t)img * y_nstride + (size_t)c * HW;
    float* po = dy + (size_t)img * dy_nstride + (size_t)c * HW;
    if (PB > MAX_PB) {
        const int seg = seg_len(HW, PB), lo = blockIdx.x * seg, hi = min(lo + seg, HW);
        const bool act = slope != 1.0f, from_y = act && beta != nullptr;
        float d[BN_V_CH][4], a[BN_V_CH][4], yy[BN_V_CH][4];
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k) {
            const int i = lo + 4 * (threadIdx.x + 256 * k);
            ld_run(pd, i, hi, d[k]);
            ld_run(py, i, hi, yy[k]);
            if (act && !from_y) ld_run(pa, i, hi, a[k]);
        }
        const float sc = gr, sh = from_y ? bn_shift(beta[bn_arena(img, p_nstride, batch) + c], m, sc) : 0.f;
#pragma unroll
        for (int k = 0; k < BN_V_CH; ++k) {
            const int i = lo + 4 * (threadIdx.x + 256 * k);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float dz = d[k][j];
                const float av = from_y ? bn_affine(yy[k][j], sc, sh) : a[k][j];
                if (act && !(av > 0.f)) dz *= slope;
                d[k][j] = gr * (dz - k1 - (yy[k][j] - m) * r * k2);
            }
            if (i < hi) st_run(po, i, hi, d[k]);
        }
        return;
    }
    for (int i = blockIdx.x * 256 + threadIdx.x; i < HW; i += gridDim.x * 256) {
        float dz = pd[i];
        if (slope != 1.0f && !(pa[i] > 0.f)) dz *= slope;
        po[i] = gr * (dz - k1 - (py[i] - m) * r * k2);
    }
}

// Small planes (<= BN_SMALL_HW pixels: every layer from the 56x56 scale down at 224^2): ONE workgroup owns a whole
// (image, channel) plane, so statistics + apply are a single launch (the plane is re-read from L1/L2).  These layers are
// pure launch latency -- a kernel boundary costs more than the work.
// pins a value in a register as the rounded fp32 number it is: the compiler cannot fuse the multiply that produced it into an
// add that consumes it (-ffp-contract=fast works across statements), which keeps a fused kernel bit-identical to the two kernels
// it replaces, where the value went through memory
__device__ __forceinline__ void rounded(float& x) { asm volatile("" : "+v"(x)); }
// The BatchNorm backward's per-element arithmetic, written once with every rounding pinned (products that feed a sum are rounded
// or fused EXPLICITLY), so that the stand-alone kernels and the chained forms (BnPre) cannot be contracted differently:
//   dz = da * (a > 0 ? 1 : slope);  xhat = (y - mean) rstd;  s1 += dz;  s2 = fma(dz, xhat, s2);
//   dy = gamma rstd ((dz - s1/n) - xhat (s2/n))
__device__ __forceinline__ float bn_dz(float d, float a, float slope, bool act) {
    if (act && !(a > 0.f)) { d *= slope; rounded(d); }
    return d;
}
__device__ __forceinline__ float bn_xhat(float y, float m, float r) {
    float x = (y - m) * r;
    rounded(x);
    return x;
}
__device__ __forceinline__ float bn_dy(float gr, float dz, float k1, float xh, float k2) {
    float t = xh * k2;
    rounded(t);
    float g = gr * ((dz - k1) - t);
    rounded(g);
    return g;
}
// the plane size as a value the compiler has not seen: the 16 per-element bounds masks (an SGPR pair each) are formed again in the phase
// that follows instead of being kept alive -- spilled -- from the first loads to the last stores
__device__ __forceinline__ int bn_fresh(int hw) { asm volatile("" : "+s"(hw)); return hw; }
constexpr int BN_SMALL_HW = 4096;
constexpr int BN_MAX_BATCH = 8;               // images per batch-statistics call (n_crops)
constexpr int BN_SMALL_PER = BN_SMALL_HW / 256;   // most plane elements a thread keeps in registers (kernels are instantiated for 1, 4 and 16:
                                                  // a 7x7 plane running the 16-element code fetched ten times the instructions it executed)
constexpr int BN_UP_SRC = 34 * 34;            // low-resolution plane of a fused upsampling staged in LDS (else read from global)
// What a small-plane launch can need beyond the plain plane.  The kernels take a mask F of these, fixed per launch, and an instance compiles
// only the paths of its mask: the fully general <16> backward was 13.6 k instructions, 261 VGPRs and 293 spilled SGPRs, most of it code a
// launch never ran, fetched cold at every launch (profiles/gen_bwd_slim_isa.txt).  The arithmetic of a path does not depend on the mask: every
// instance that covers a launch's needs gives the same bits (tests/test_bn_small_instances_gpu.py).
enum : unsigned {
    BN_F_BATCH = 1,    // batch statistics (batch > 0)
    BN_F_TAIL = 2,     // backward: one parameter set shared by N > 1 images -- image 0 walks the other images' sums
    BN_F_SLABS = 4,    // split-K slabs summed while the plane is loaded (forward: the conv's or the BnPre's; backward: BnSlabs)
    BN_F_PRE = 8,      // a BnPre rides in the launch
    BN_F_UP = 16,      // a BnUpsample rides in the launch
    BN_F_ALL = 31
};
// slabs != null: the plane is first formed as bias + sum of the feeding convolution's split-K slabs (slice order) and stored to y
template <int PER, unsigned F>   // PER: plane elements a thread keeps in registers: 1, 4 or 16 (planes of <= 256, <= 1024, <= 4096 pixels)
__global__ __launch_bounds__(256) void bn_small_fwd_kernel(const float* y, size_t y_nstride, float* __restrict__ out,
                                                           size_t out_nstride, int C, int HW, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float eps, float* __restrict__ mean_o,
                                                           float* __restrict__ rstd_o, float slope, const float* __restrict__ slabs,
                                                           int ksplit, const float* __restrict__ bias, float* __restrict__ y_out, BnUpsample up,
                                                           size_t p_nstride, int batch, BnPre pre) {
    __shared__ float red[8];
    __shared__ float up_src_s[(F & BN_F_UP) ? BN_UP_SRC : 1];
    const int c = blockIdx.x, img = blockIdx.y;
    if (!(F & BN_F_BATCH)) batch = 0;
    gamma += bn_arena(img, p_nstride, batch); beta += bn_arena(img, p_nstride, batch);
    if (bias) bias += bn_arena(img, p_nstride, batch);
    const float* p = y + (size_t)img * y_nstride + (size_t)c * HW;
    float* q = out + (size_t)img * out_nstride + (size_t)c * HW;
    // loads are issued branch-free (wave-uniform guards only; a thread past the end of the plane re-reads element 0 and
    // is masked afterwards): lane-guarded loads compile to load + s_waitcnt per element, i.e. one memory round trip each
    float v[PER];
    float s = 0.f, dummy = 0.f;
    if ((F & BN_F_PRE) && pre.y && c < pre.C) {
        // ---- the skip branch's own BatchNorm + LeakyReLU on this plane (BnPre), in front of the concat's: the plane is formed
        // (from the skip convolution's output, or from its split-K slabs + bias), normalised with ITS statistics, activated and
        // stored into the concat buffer (the backward reads it there); v then holds the concat BatchNorm's input
        const float* py1 = pre.y + (size_t)img * pre.y_ns + (size_t)c * HW;
        if ((F & BN_F_SLABS) && pre.slabs) {
            const size_t per = (size_t)gridDim.y * pre.C * HW;
            const float* sp = pre.slabs + ((size_t)img * pre.C + c) * HW;
            float* yo = const_cast<float*>(py1);
            const float b = pre.bias ? pre.bias[(size_t)img * p_nstride + c] : 0.f;
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = b;
            for (int ks = 0; ks < pre.ksplit; ks += 4) {   // slice order, four slices of loads in flight (as the slabs path below)
                float t[4][PER];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (ks + u >= pre.ksplit) continue;
                    const float* sk = sp + (size_t)(ks + u) * per;
#pragma unroll
                    for (int k = 0; k < PER; ++k) {
                        if (k * 256 >= HW) continue;
                        const int i = threadIdx.x + k * 256;
                        t[u][k] = sk[i < HW ? i : 0];
                    }
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if (ks + u >= pre.ksplit) continue;
#pragma unroll
                    for (int k = 0; k < PER; ++k)
                        if (k * 256 < HW) v[k] += t[u][k];
                }
            }
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + k * 256;
                if (i < HW) yo[i] = v[k]; else v[k] = 0.f;
            }
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + k * 256;
                v[k] = k * 256 < HW ? py1[i < HW ? i : 0] : 0.f;
            }
#pragma unroll
            for (int k = 0; k < PER; ++k)
                if (threadIdx.x + k * 256 >= HW) v[k] = 0.f;
        }
        float s1 = 0.f, d1 = 0.f;
#pragma unroll
        for (int k = 0; k < PER; ++k) s1 += v[k];
        block_sum2(s1, d1, red);
        const float m1 = s1 / (float)HW;
        float q1 = 0.f;
        d1 = 0.f;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const float d = threadIdx.x + k * 256 < HW ? v[k] - m1 : 0.f;
            q1 += d * d;
        }
        block_sum2(q1, d1, red);
        const float r1 = rsqrtf(q1 / (float)HW + eps);
        if (threadIdx.x == 0) { pre.mean[img * pre.C + c] = m1; pre.rstd[img * pre.C + c] = r1; }
        const float sc1 = pre.gamma[(size_t)img * p_nstride + c] * r1;
        const float sh1 = pre.beta[(size_t)img * p_nstride + c] - m1 * sc1;
        float* yo2 = const_cast<float*>(p);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = threadIdx.x + k * 256;
            const float t = v[k] * sc1 + sh1;
            v[k] = i < HW ? (t > 0.f ? t : t * pre.slope) : 0.f;
            rounded(v[k]);   // the value the stand-alone kernels hand over through memory: nothing may be contracted across it
            if (i < HW) yo2[i] = v[k];
            s += v[k];
        }
    } else if ((F & BN_F_SLABS) && slabs) {
        const size_t per = (size_t)gridDim.y * C * HW;
        const float* sp = slabs + ((size_t)img * C + c) * HW;
        float* yo = y_out + (size_t)img * y_nstride + (size_t)c * HW;
        const float b = bias ? bias[c] : 0.f;
#pragma unroll
        for (int k = 0; k < PER; ++k) v[k] = b;
        for (int ks = 0; ks < ksplit; ks += 4) {   // slice order (as conv_splitk_reduce_kernel); four slices of loads in flight
            float t[4][PER];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ks + u >= ksplit) continue;
                const float* sk = sp + (size_t)(ks + u) * per;
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    if (k * 256 >= HW) continue;
                    const int i = threadIdx.x + k * 256;
                    t[u][k] = sk[i < HW ? i : 0];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (ks + u >= ksplit) continue;
#pragma unroll
                for (int k = 0; k < PER; ++k)
                    if (k * 256 < HW) v[k] += t[u][k];
            }
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < HW) yo[i] = v[k]; else v[k] = 0.f;
            s += v[k];
        }
    } else if ((F & BN_F_UP) && up.src && c >= up.c0) {
        // upsampled channel of the concat: the values are produced here from the low-resolution plane (staged through LDS
        // when it fits) and stored into y for the backward -- the upsampling is not a launch of its own
        const float* sp = up.src + (size_t)img * up.src_ns + (size_t)(c - up.c0) * up.h * up.w;
        float* yo = const_cast<float*>(p);
        const bool in_lds = up.h * up.w <= BN_UP_SRC;
        if (in_lds) {
            for (int e = threadIdx.x; e < up.h * up.w; e += 256) up_src_s[e] = sp[e];
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = threadIdx.x + k * 256;
            v[k] = 0.f;
            if (k * 256 < HW) {
                const int ii = i < HW ? i : HW - 1;
                const int oy = ii / up.Wo, ox = ii - oy * up.Wo;
                v[k] = in_lds ? up_value((const float*)up_src_s, up.h, up.w, oy, ox) : up_value(sp, up.h, up.w, oy, ox);
                if (i < HW) yo[i] = v[k];
            }
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (threadIdx.x + k * 256 >= HW) v[k] = 0.f;
            s += v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = threadIdx.x + k * 256;
            v[k] = k * 256 < HW ? p[i < HW ? i : 0] : 0.f;
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (threadIdx.x + k * 256 >= HW) v[k] = 0.f;
            s += v[k];
        }
    }
    block_sum2(s, dummy, red);
    float m = s / (float)HW;
    float sq = 0.f;
    dummy = 0.f;
    float cnt = (float)HW;
    if (batch) {
        // batch statistics: every workgroup of channel c walks all N planes of its batch / group in image order (same bits in each);
        // the other planes are re-read (small, L2-resident); slabs / fused upsampling are not combined with this mode
        const int N = batch;
        const float* yg = y + (size_t)(img / batch * batch) * y_nstride;
        float tot = 0.f;
        for (int n = 0; n < N; ++n) {
            const float* pn = yg + (size_t)n * y_nstride + (size_t)c * HW;
            float sn = 0.f, d2 = 0.f;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + k * 256;
                if (k * 256 < HW) sn += i < HW ? pn[i] : 0.f;
            }
            block_sum2(sn, d2, red);
            tot += sn;
        }
        cnt = (float)HW * (float)N;
        m = tot / cnt;
        for (int n = 0; n < N; ++n) {
            const float* pn = yg + (size_t)n * y_nstride + (size_t)c * HW;
            float qn = 0.f, d2 = 0.f;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + k * 256;
                if (k * 256 < HW) { const float d = i < HW ? pn[i] - m : 0.f; qn += d * d; }
            }
            block_sum2(qn, d2, red);
            sq += qn;
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const float d = threadIdx.x + k * 256 < HW ? v[k] - m : 0.f;
            sq += d * d;
        }
        block_sum2(sq, dummy, red);
    }
    const float r = rsqrtf(sq / cnt + eps);
    if (threadIdx.x == 0) { mean_o[img * C + c] = m; rstd_o[img * C + c] = r; }
    const float sc = gamma[c] * r;
    const float sh = beta[c] - m * sc;
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = threadIdx.x + k * 256;
        if (i < HW) {
            const float t = v[k] * sc + sh;
            q[i] = t > 0.f ? t : t * slope;
        }
    }
}
// one workgroup per (channel, image); each plane is read once and kept in registers between the reduction and the apply
// pass.  dgamma / dbeta need the sums of EVERY image: the workgroup of image 0 recomputes the other images' two sums
// (reads only) and adds them in image order -- deterministic, no second launch, no cross-workgroup wait.
// sl.slabs != null: the output gradient of this plane was left as split-K slabs by the data-gradient convolution that produces it
// (BnSlabs): d = (accumulate ? the value at pd : 0) + (0 + slab 0 + slab 1 + ...), the arithmetic of conv_splitk_reduce_kernel
template <int PER>
__device__ __forceinline__ void bn_small_bwd_sums(const float* pd, const float* pa, const float* py, int HW, float m, float r, float slope,
                                                  float (&dz)[PER], float (&xh)[PER], float& s1, float& s2, float* red,
                                                  const float* sp = nullptr, size_t per = 0, int ksplit = 0, int sl_acc = 0) {
    s1 = 0.f; s2 = 0.f;
    // branch-free loads first (see bn_small_fwd_kernel), arithmetic after
    const bool act = slope != 1.0f;
    // ... and free of wave-uniform value selects too: `act ? pa[j] : 1.f` put every load of the activated plane into a block of its own with
    // the sign test behind it -- load, s_waitcnt vmcnt(0), compare, once per element: 16 dependent memory round trips in the 56x56
    // kernel.  Without an activation nobody reads the activated plane: the loads then go to the y plane, whose lines the vy loads fetch anyway.
    const float* pa_ld = act ? pa : py;
    float vd[PER], va[PER], vy[PER];
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        if (k * 256 >= HW) continue;
        const int i = threadIdx.x + k * 256;
        const int j = i < HW ? i : 0;
        vy[k] = py[j];
        va[k] = pa_ld[j];
    }
    if (!sp || sl_acc) {   // (plain slabs: the gradient is the slabs' sum alone)
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            if (k * 256 >= HW) continue;
            const int i = threadIdx.x + k * 256;
            vd[k] = pd[i < HW ? i : 0];
        }
    } else {
#pragma unroll
        for (int k = 0; k < PER; ++k) vd[k] = 0.f;
    }
    if (sp) {
        float v[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) v[k] = 0.f;
        // slice order, four slices of loads in flight; the full groups run without a guard per slice (64 guarded loads kept half the
        // register file busy), the last group of 1 to 3 slices with them
        auto group = [&](int ks, int nu) {
            float t[4][PER];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (u >= nu) continue;
                const float* sk = sp + (size_t)(ks + u) * per;
#pragma unroll
                for (int k = 0; k < PER; ++k) {
                    if (k * 256 >= HW) continue;
                    const int i = threadIdx.x + k * 256;
                    t[u][k] = sk[i < HW ? i : 0];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (u >= nu) continue;
#pragma unroll
                for (int k = 0; k < PER; ++k)
                    if (k * 256 < HW) v[k] += t[u][k];
            }
        };
        int ks = 0;
        for (; ks + 3 < ksplit; ks += 4) group(ks, 4);
        if (ks < ksplit) group(ks, ksplit - ks);
#pragma unroll
        for (int k = 0; k < PER; ++k)
            if (k * 256 < HW) vd[k] = sl_acc ? vd[k] + v[k] : v[k];
    }
    if (PER > 4) HW = bn_fresh(HW);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
        const int i = threadIdx.x + k * 256;
        float d = 0.f, x = 0.f;
        if (k * 256 < HW) {
            rounded(va[k]);   // keeps the sign test here, behind every load (it was folded into the load's block: a wait per element)
            d = bn_dz(vd[k], va[k], slope, act);
            x = bn_xhat(vy[k], m, r);
            if (i >= HW) { d = 0.f; x = 0.f; }
        }
        dz[k] = d; xh[k] = x;
        s1 += d;
        s2 = __builtin_fmaf(d, x, s2);
    }
    block_sum2(s1, s2, red);
}
template <int PER, unsigned F>
__global__ __launch_bounds__(256) void bn_small_bwd_kernel(const float* __restrict__ da, size_t da_nstride, const float* __restrict__ aout,
                                                           size_t a_nstride, const float* __restrict__ y, size_t y_nstride,
                                                           float* __restrict__ dy, size_t dy_nstride, int C, int HW, int N,
                                                           const float* __restrict__ gamma, const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, float slope, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int accumulate, BnUpsample up, size_t p_nstride, int batch, BnPre pre,
                                                           BnSlabs sl) {
    __shared__ float red[8];
    __shared__ float up_grad_s[(F & BN_F_UP) ? BN_SMALL_HW : 1];   // fused upsampling adjoint: this plane's input gradient
    const int c = blockIdx.x, img = blockIdx.y;
    if (!(F & BN_F_BATCH)) batch = 0;
    gamma += bn_arena(img, p_nstride, batch);
    const int n0 = batch ? img / batch * batch : 0;   // first image of the batch / group
    float dz[PER], xh[PER];
    float s1, s2;
    const bool chained = (F & BN_F_PRE) && pre.y && c < pre.C;   // workgroup-uniform: a skip-branch BatchNorm sits in front of this channel (BnPre)
    // the chained adjoint's operands are fetched with the plane's own loads, not in a round trip of their own behind the first block sum
    constexpr int CPER = (F & BN_F_PRE) ? PER : 1;
    float cva[CPER], cvy[CPER];
    float m1 = 0.f, r1 = 0.f, g1 = 0.f;
    if constexpr ((F & BN_F_PRE) != 0) {
        if (chained) {
            m1 = pre.mean[img * pre.C + c]; r1 = pre.rstd[img * pre.C + c]; g1 = pre.gamma[(size_t)img * p_nstride + c];
            const float* pa1 = y + (size_t)img * y_nstride + (size_t)c * HW;                   // a = act(bn1(y1)): sign selects the LeakyReLU branch
            const float* py1 = pre.y + (size_t)img * pre.y_ns + (size_t)c * HW;
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                if (k * 256 >= HW) continue;
                const int i = threadIdx.x + k * 256, j = i < HW ? i : 0;
                cva[k] = pa1[j];
                cvy[k] = py1[j];
            }
            asm volatile("" : : : "memory");   // the loads stay here (they were sunk behind the first block sum again)
        }
    }
    {
        const float m = mean[img * C + c], r = rstd[img * C + c];
        float b1 = 0.f, b2 = 0.f;   // batch statistics: sums over every image of the batch, in image order; the own plane last (dz / xh stay)
        if ((F & BN_F_BATCH) && batch) {
            float t1s[BN_MAX_BATCH], t2s[BN_MAX_BATCH];
#pragma unroll
            for (int n = 0; n < BN_MAX_BATCH; ++n) {
                t1s[n] = 0.f; t2s[n] = 0.f;
                const int gn = n0 + n;
                if (n < batch && gn != img)
                    bn_small_bwd_sums<PER>(da + (size_t)gn * da_nstride + (size_t)c * HW, aout + (size_t)gn * a_nstride + (size_t)c * HW,
                                      y + (size_t)gn * y_nstride + (size_t)c * HW, HW, mean[gn * C + c], rstd[gn * C + c], slope, dz, xh, t1s[n], t2s[n], red);
            }
            bn_small_bwd_sums<PER>(da + (size_t)img * da_nstride + (size_t)c * HW, aout + (size_t)img * a_nstride + (size_t)c * HW,
                              y + (size_t)img * y_nstride + (size_t)c * HW, HW, m, r, slope, dz, xh, s1, s2, red);
#pragma unroll
            for (int n = 0; n < BN_MAX_BATCH; ++n)
                if (n < batch) { b1 += n0 + n == img ? s1 : t1s[n]; b2 += n0 + n == img ? s2 : t2s[n]; }
        } else {
            bn_small_bwd_sums<PER>(da + (size_t)img * da_nstride + (size_t)c * HW, aout + (size_t)img * a_nstride + (size_t)c * HW,
                              y + (size_t)img * y_nstride + (size_t)c * HW, HW, m, r, slope, dz, xh, s1, s2, red,
                              (F & BN_F_SLABS) && sl.slabs ? sl.slabs + ((size_t)img * C + c) * HW : nullptr, (size_t)gridDim.y * C * HW, sl.ksplit, sl.accumulate);
        }
        const float cnt = batch ? (float)HW * (float)batch : (float)HW;
        const float k1 = (batch ? b1 : s1) / cnt, k2 = (batch ? b2 : s2) / cnt;
        if (batch) { s1 = b1; s2 = b2; }   // the parameter gradients are exactly these sums
        const float gr = gamma[c] * r;
        float* po = dy + (size_t)img * dy_nstride + (size_t)c * HW;
        const bool through_adjoint = (F & BN_F_UP) && up.d_src && c >= up.c0;   // workgroup-uniform
        if (PER > 4) HW = bn_fresh(HW);
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = threadIdx.x + k * 256;
            if (i < HW) {
                const float gv = bn_dy(gr, dz[k], k1, xh[k], k2);
                if (through_adjoint) up_grad_s[i] = gv; else if (chained) dz[k] = gv; else po[i] = gv;
            } else if (chained) dz[k] = 0.f;
        }
        if constexpr ((F & BN_F_PRE) != 0) if (chained) {
            // ---- the adjoint of the skip branch's BatchNorm + LeakyReLU behind the concat's, on the same plane: dz holds the
            // gradient w.r.t. the activated skip plane a (= this BatchNorm's input y, in the concat buffer)
            float t1 = 0.f, t2 = 0.f;
            if (PER > 4) HW = bn_fresh(HW);
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + k * 256;
                float d = 0.f, x = 0.f;
                if (k * 256 < HW && i < HW) {
                    rounded(cva[k]);   // as in bn_small_bwd_sums: the sign test stays behind the loads
                    d = bn_dz(dz[k], cva[k], pre.slope, true);
                    x = bn_xhat(cvy[k], m1, r1);
                }
                dz[k] = d; xh[k] = x;
                t1 += d;
                t2 = __builtin_fmaf(d, x, t2);
            }
            block_sum2(t1, t2, red);
            const float j1 = t1 / (float)HW, j2 = t2 / (float)HW;
            const float gr1 = g1 * r1;
            float* pd1 = pre.dy + (size_t)img * pre.y_ns + (size_t)c * HW;
            if (PER > 4) HW = bn_fresh(HW);
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                const int i = threadIdx.x + k * 256;
                if (i < HW) pd1[i] = bn_dy(gr1, dz[k], j1, xh[k], j2);
            }
            if (threadIdx.x == 0) {
                float* dg = pre.dgamma + (size_t)img * p_nstride + c;
                float* db = pre.dbeta + (size_t)img * p_nstride + c;
                *dg = accumulate ? *dg + t2 : t2;
                *db = accumulate ? *db + t1 : t1;
            }
        }
        if (through_adjoint) {
            // this channel is an upsampled one: nobody but the upsampling's adjoint reads its input gradient, so it goes
            // from LDS straight into the gradient of the low-resolution plane (the arithmetic of upsample2x_bwd_kernel)
            __syncthreads();
            float* qd = up.d_src + (size_t)img * up.d_src_ns + (size_t)(c - up.c0) * up.h * up.w;
            for (int e = threadIdx.x; e < up.h * up.w; e += 256)
                qd[e] = up_adjoint_value((const float*)up_grad_s, up.h, up.w, up.Ho, up.Wo, e / up.w, e % up.w);
        }
    }
    if (p_nstride) {   // independent images: every image owns its parameter gradients; grouped: the group's first image writes its sums
        if (threadIdx.x == 0 && (!batch || img == n0)) {
            float* dg = dgamma + bn_arena(img, p_nstride, batch) + c;
            float* db = dbeta + bn_arena(img, p_nstride, batch) + c;
            *dg = accumulate ? *dg + s2 : s2;
            *db = accumulate ? *db + s1 : s1;
        }
        return;
    }
    if (img != 0) return;
    float g = s2, be = s1;
    for (int n = 1; n < ((F & BN_F_TAIL) && !batch ? N : 0); ++n) {
        float t1, t2;
        bn_small_bwd_sums<PER>(da + (size_t)n * da_nstride + (size_t)c * HW, aout + (size_t)n * a_nstride + (size_t)c * HW,
                          y + (size_t)n * y_nstride + (size_t)c * HW, HW, mean[n * C + c], rstd[n * C + c], slope, dz, xh, t1, t2, red);
        be += t1;
        g += t2;
    }
    if (threadIdx.x == 0) {
        dgamma[c] = accumulate ? dgamma[c] + g : g;
        dbeta[c] = accumulate ? dbeta[c] + be : be;
    }
}

// ---- middle planes (BN_SMALL_HW < pixels <= BN_MID_HW: the 112 x 112 planes of a 224 x 224 image) --------------------------------
// The two-stage form costs two launches of ~5 us each per BatchNorm in every direction.  One workgroup of 1024 threads owns a
// whole (image, channel) plane, as for the small planes, with the plane staged in LDS instead of registers (a register tile of 49
// elements per thread would be 18 k instructions of straight-line code): statistics + apply in ONE launch (round 4: 6 BatchNorms
// per image and direction at 224 x 224).  Same arithmetic as the small-plane kernels up to the order of the block-wide sums.
constexpr int BN_MID_HW = 16384;        // floats of LDS plane (64 KB)
constexpr int BN_MID_THREADS = 1024;
__device__ __forceinline__ void block_sum2_1024(float& a, float& b, float* red /* 32 floats */) {
    a = wave_sum(a);
    b = wave_sum(b);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red[w] = a; red[16 + w] = b; }
    __syncthreads();
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) { sa += red[k]; sb += red[16 + k]; }   // fixed order
    a = sa; b = sb;
}
constexpr int BN_MID_SRC = 4096;        // low-resolution source plane of a fused upsampling, staged behind the plane (else read from global)
// plane elements in groups of 4 (16-byte accesses, every thread's loads of a pass in flight together); tail elements one by one
template <class F4, class F1>
__device__ __forceinline__ void bn_mid_for(int HW, bool vec, F4&& f4, F1&& f1) {
    const int n4 = vec ? HW >> 2 : 0;
    for (int i = threadIdx.x; i < n4; i += BN_MID_THREADS) f4(i);
    for (int i = n4 * 4 + threadIdx.x; i < HW; i += BN_MID_THREADS) f1(i);
}
__global__ __launch_bounds__(BN_MID_THREADS) void bn_mid_fwd_kernel(const float* y, size_t y_nstride, float* __restrict__ out, size_t out_nstride, int C, int HW,
                                                                    const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                                    float* __restrict__ mean_o, float* __restrict__ rstd_o, float slope, BnUpsample up,
                                                                    size_t p_nstride, BnPre pre) {
    extern __shared__ __attribute__((aligned(16))) float bn_mid_plane[];   // HW floats (+ the upsampling source)
    __shared__ float red[32];
    const int c = blockIdx.x, img = blockIdx.y;
    gamma += (size_t)img * p_nstride; beta += (size_t)img * p_nstride;
    const float* p = y + (size_t)img * y_nstride + (size_t)c * HW;
    float* q = out + (size_t)img * out_nstride + (size_t)c * HW;
    const bool vec = !(HW & 3) && !((reinterpret_cast<size_t>(p) | reinterpret_cast<size_t>(q)) & 15);
    float s = 0.f, dummy = 0.f;
    if (pre.y && c < pre.C) {
        // the skip branch's own BatchNorm + LeakyReLU in front of the concat's, on the same plane (BnPre; see bn_small_fwd_kernel).
        // Same access pattern and summation order as a launch of this kernel on the skip unit alone: the same bits either way.
        const float* py1 = pre.y + (size_t)img * pre.y_ns + (size_t)c * HW;
        const bool vec1 = vec && !(reinterpret_cast<size_t>(py1) & 15);
        float s1 = 0.f, d1 = 0.f;
        bn_mid_for(HW, vec1,
                   [&](int i) { const float4 v = reinterpret_cast<const float4*>(py1)[i]; reinterpret_cast<float4*>(bn_mid_plane)[i] = v; s1 += (v.x + v.y) + (v.z + v.w); },
                   [&](int i) { const float v = py1[i]; bn_mid_plane[i] = v; s1 += v; });
        block_sum2_1024(s1, d1, red);
        const float m1 = s1 / (float)HW;
        float q1 = 0.f;
        d1 = 0.f;
        bn_mid_for(HW, vec1,
                   [&](int i) { const float4 v = reinterpret_cast<const float4*>(bn_mid_plane)[i]; const float a = v.x - m1, b = v.y - m1, cc = v.z - m1, d = v.w - m1; q1 += (a * a + b * b) + (cc * cc + d * d); },
                   [&](int i) { const float d = bn_mid_plane[i] - m1; q1 += d * d; });
        block_sum2_1024(q1, d1, red);
        const float r1 = rsqrtf(q1 / (float)HW + eps);
        if (threadIdx.x == 0) { pre.mean[img * pre.C + c] = m1; pre.rstd[img * pre.C + c] = r1; }
        const float sc1 = pre.gamma[(size_t)img * p_nstride + c] * r1;
        const float sh1 = pre.beta[(size_t)img * p_nstride + c] - m1 * sc1;
        float* yo2 = const_cast<float*>(p);
        auto act1 = [&](float x) { const float t = x * sc1 + sh1; float a = t > 0.f ? t : t * pre.slope; rounded(a); return a; };
        bn_mid_for(HW, vec1,
                   [&](int i) {
                       const float4 v = reinterpret_cast<const float4*>(bn_mid_plane)[i];
                       const float4 a = float4{act1(v.x), act1(v.y), act1(v.z), act1(v.w)};
                       reinterpret_cast<float4*>(bn_mid_plane)[i] = a;
                       reinterpret_cast<float4*>(yo2)[i] = a;
                       s += (a.x + a.y) + (a.z + a.w);
                   },
                   [&](int i) { const float a = act1(bn_mid_plane[i]); bn_mid_plane[i] = a; yo2[i] = a; s += a; });
    } else if (up.src && c >= up.c0) {   // upsampled channel of the concat: produced here, stored into y for the backward
        const float* sp = up.src + (size_t)img * up.src_ns + (size_t)(c - up.c0) * up.h * up.w;
        float* yo = const_cast<float*>(p);
        const int hw = up.h * up.w;
        const bool in_lds = hw <= BN_MID_SRC;
        float* srcs = bn_mid_plane + ((HW + 3) & ~3);
        if (in_lds) {
            for (int e = threadIdx.x; e < hw; e += BN_MID_THREADS) srcs[e] = sp[e];
            __syncthreads();
        }
        for (int i = threadIdx.x; i < HW; i += BN_MID_THREADS) {
            const int oy = i / up.Wo, ox = i - oy * up.Wo;
            const float v = in_lds ? up_value((const float*)srcs, up.h, up.w, oy, ox) : up_value(sp, up.h, up.w, oy, ox);
            yo[i] = v;
            bn_mid_plane[i] = v;
            s += v;
        }
    } else {
        bn_mid_for(HW, vec,
                   [&](int i) { const float4 v = reinterpret_cast<const float4*>(p)[i]; reinterpret_cast<float4*>(bn_mid_plane)[i] = v; s += (v.x + v.y) + (v.z + v.w); },
                   [&](int i) { const float v = p[i]; bn_mid_plane[i] = v; s += v; });
    }
    block_sum2_1024(s, dummy, red);
    const float m = s / (float)HW;
    float sq = 0.f;
    dummy = 0.f;
    bn_mid_for(HW, vec,
               [&](int i) { const float4 v = reinterpret_cast<const float4*>(bn_mid_plane)[i]; const float a = v.x - m, b = v.y - m, cc = v.z - m, d = v.w - m; sq += (a * a + b * b) + (cc * cc + d * d); },
               [&](int i) { const float d = bn_mid_plane[i] - m; sq += d * d; });
    block_sum2_1024(sq, dummy, red);
    const float r = rsqrtf(sq / (float)HW + eps);
    if (threadIdx.x == 0) { mean_o[img * C + c] = m; rstd_o[img * C + c] = r; }
    const float sc = gamma[c] * r;
    const float sh = beta[c] - m * sc;
    auto act = [&](float x) { const float t = x * sc + sh; return t > 0.f ? t : t * slope; };
    bn_mid_for(HW, vec,
               [&](int i) { const float4 v = reinterpret_cast<const float4*>(bn_mid_plane)[i]; reinterpret_cast<float4*>(q)[i] = float4{act(v.x), act(v.y), act(v.z), act(v.w)}; },
               [&](int i) { q[i] = act(bn_mid_plane[i]); });
}
// backward: dz = da * act'(a) staged in LDS while s1 = sum dz and s2 = sum dz xhat are taken; second pass forms
// dy = gamma rstd (dz - s1/HW - xhat s2/HW) (xhat from a second read of y), or -- for an upsampled channel -- sends it through
// the x2 bilinear adjoint out of LDS.  Per-image parameter gradients (independent generators) or a single image.
__global__ __launch_bounds__(BN_MID_THREADS) void bn_mid_bwd_kernel(const float* __restrict__ da, size_t da_nstride, const float* __restrict__ aout, size_t a_nstride,
                                                                    const float* __restrict__ y, size_t y_nstride, float* __restrict__ dy, size_t dy_nstride, int C, int HW,
                                                                    const float* __restrict__ gamma, const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    float slope, float* __restrict__ dgamma, float* __restrict__ dbeta, int accumulate, BnUpsample up,
                                                                    size_t p_nstride, BnPre pre) {
    extern __shared__ __attribute__((aligned(16))) float bn_mid_plane[];
    __shared__ float red[32];
    const int c = blockIdx.x, img = blockIdx.y;
    gamma += (size_t)img * p_nstride;
    const float m = mean[img * C + c], r = rstd[img * C + c];
    const float* pd = da + (size_t)img * da_nstride + (size_t)c * HW;
    const float* pa = aout + (size_t)img * a_nstride + (size_t)c * HW;
    const float* py = y + (size_t)img * y_nstride + (size_t)c * HW;
    float* po = dy + (size_t)img * dy_nstride + (size_t)c * HW;
    const bool act = slope != 1.0f;
    const bool vec = !(HW & 3) && !((reinterpret_cast<size_t>(pd) | reinterpret_cast<size_t>(pa) | reinterpret_cast<size_t>(py) | reinterpret_cast<size_t>(po)) & 15);
    float s1 = 0.f, s2 = 0.f;
    auto one = [&](float d, float a, float yv) {
        d = bn_dz(d, a, slope, act);
        s1 += d;
        s2 = __builtin_fmaf(d, bn_xhat(yv, m, r), s2);
        return d;
    };
    bn_mid_for(HW, vec,
               [&](int i) {
                   const float4 d = reinterpret_cast<const float4*>(pd)[i], yv = reinterpret_cast<const float4*>(py)[i];
                   const float4 a = act ? reinterpret_cast<const float4*>(pa)[i] : float4{1.f, 1.f, 1.f, 1.f};
                   reinterpret_cast<float4*>(bn_mid_plane)[i] = float4{one(d.x, a.x, yv.x), one(d.y, a.y, yv.y), one(d.z, a.z, yv.z), one(d.w, a.w, yv.w)};
               },
               [&](int i) { bn_mid_plane[i] = one(pd[i], act ? pa[i] : 1.f, py[i]); });
    block_sum2_1024(s1, s2, red);
    const float k1 = s1 / (float)HW, k2 = s2 / (float)HW;
    const float gr = gamma[c] * r;
    const bool through_adjoint = up.d_src && c >= up.c0;   // workgroup-uniform
    auto grad = [&](float dz, float yv) { return bn_dy(gr, dz, k1, bn_xhat(yv, m, r), k2); };
    if (pre.y && c < pre.C) {
        // the adjoint of the skip branch's BatchNorm + LeakyReLU behind the concat's (BnPre): the gradient w.r.t. the activated skip
        // plane a (= this BatchNorm's input y) stays in LDS.  Access pattern and summation order of a launch on the skip unit alone.
        const float m1 = pre.mean[img * pre.C + c], r1 = pre.rstd[img * pre.C + c];
        const float* py1 = pre.y + (size_t)img * pre.y_ns + (size_t)c * HW;
        float* pd1 = pre.dy + (size_t)img * pre.y_ns + (size_t)c * HW;
        const bool vec1 = vec && !((reinterpret_cast<size_t>(py1) | reinterpret_cast<size_t>(pd1)) & 15);
        float t1 = 0.f, t2 = 0.f;
        auto one1 = [&](float dzc, float a, float y1) {
            const float d = bn_dz(grad(dzc, a), a, pre.slope, true);
            t1 += d;
            t2 = __builtin_fmaf(d, bn_xhat(y1, m1, r1), t2);
            return d;
        };
        bn_mid_for(HW, vec1,
                   [&](int i) {
                       const float4 dzc = reinterpret_cast<const float4*>(bn_mid_plane)[i], a = reinterpret_cast<const float4*>(py)[i], y1 = reinterpret_cast<const float4*>(py1)[i];
                       reinterpret_cast<float4*>(bn_mid_plane)[i] = float4{one1(dzc.x, a.x, y1.x), one1(dzc.y, a.y, y1.y), one1(dzc.z, a.z, y1.z), one1(dzc.w, a.w, y1.w)};
                   },
                   [&](int i) { bn_mid_plane[i] = one1(bn_mid_plane[i], py[i], py1[i]); });
        block_sum2_1024(t1, t2, red);
        const float j1 = t1 / (float)HW, j2 = t2 / (float)HW;
        const float gr1 = pre.gamma[(size_t)img * p_nstride + c] * r1;
        auto grad1 = [&](float dz, float y1) { return bn_dy(gr1, dz, j1, bn_xhat(y1, m1, r1), j2); };
        bn_mid_for(HW, vec1,
                   [&](int i) {
                       const float4 dz = reinterpret_cast<const float4*>(bn_mid_plane)[i], y1 = reinterpret_cast<const float4*>(py1)[i];
                       reinterpret_cast<float4*>(pd1)[i] = float4{grad1(dz.x, y1.x), grad1(dz.y, y1.y), grad1(dz.z, y1.z), grad1(dz.w, y1.w)};
                   },
                   [&](int i) { pd1[i] = grad1(bn_mid_plane[i], py1[i]); });
        if (threadIdx.x == 0) {
            float* dg = pre.dgamma + (size_t)img * p_nstride + c;
            float* db = pre.dbeta + (size_t)img * p_nstride + c;
            *dg = accumulate ? *dg + t2 : t2;
            *db = accumulate ? *db + t1 : t1;
        }
    } else if (through_adjoint) {
        for (int i = threadIdx.x; i < HW; i += BN_MID_THREADS) bn_mid_plane[i] = grad(bn_mid_plane[i], py[i]);
        __syncthreads();
        float* qd = up.d_src + (size_t)img * up.d_src_ns + (size_t)(c - up.c0) * up.h * up.w;
        for (int e = threadIdx.x; e < up.h * up.w; e += BN_MID_THREADS)
            qd[e] = up_adjoint_value((const float*)bn_mid_plane, up.h, up.w, up.Ho, up.Wo, e / up.w, e % up.w);
    } else {
        bn_mid_for(HW, vec,
                   [&](int i) {
                       const float4 dz = reinterpret_cast<const float4*>(bn_mid_plane)[i], yv = reinterpret_cast<const float4*>(py)[i];
                       reinterpret_cast<float4*>(po)[i] = float4{grad(dz.x, yv.x), grad(dz.y, yv.y), grad(dz.z, yv.z), grad(dz.w, yv.w)};
                   },
                   [&](int i) { po[i] = grad(bn_mid_plane[i], py[i]); });
    }
    if (threadIdx.x == 0) {
        float* dg = dgamma + (size_t)img * p_nstride + c;
        float* db = dbeta + (size_t)img * p_nstride + c;
        *dg = accumulate ? *dg + s2 : s2;
        *db = accumulate ? *db + s1 : s1;
    }
}
static void bn_mid_allow_lds() {   // > 48 KB of dynamic LDS has to be allowed once per kernel and device
    int dev = 0;
    (void)hipGetDevice(&dev);
    static std::atomic<unsigned long long> done{0};
    const unsigned long long bit = 1ull << (dev & 63);
    if (!(done.load(std::memory_order_relaxed) & bit)) {
        (void)hipFuncSetAttribute((const void*)bn_mid_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (BN_MID_HW + BN_MID_SRC) * 4);
        (void)hipFuncSetAttribute((const void*)bn_mid_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, BN_MID_HW * 4);
        done.fetch_or(bit, std::memory_order_relaxed);
    }
}
// the instantiation whose register tile just covers the plane (same arithmetic in the same order: the surplus elements of a
// bigger tile only ever added zeros)
// ... and whose feature mask covers what the launch needs.  The instances that exist: what the engine issues (the plain plane; slabs; the
// concat unit, which carries a BnPre and / or a BnUpsample, with or without slabs; batch statistics; the shared-parameter tail) and the fully
// general one, which takes every other combination.  First entry of the list that covers the need.
static const unsigned BN_SMALL_INSTANCES[] = {0, BN_F_SLABS, BN_F_UP, BN_F_PRE | BN_F_UP, BN_F_PRE | BN_F_UP | BN_F_SLABS, BN_F_BATCH, BN_F_TAIL, BN_F_ALL};
static std::atomic<int> g_bn_small_forced{-1};   // test hook (splice_gen_bn_small_instance): >= 0 = the instance every small-plane launch takes
int bn_small_force_instance(int mask) {
    if (mask < 0) { g_bn_small_forced.store(-1); return SPLICE_OK; }
    for (unsigned m : BN_SMALL_INSTANCES)
        if ((unsigned)mask == m) { g_bn_small_forced.store(mask); return SPLICE_OK; }
    return SPLICE_ERR_ARG;
}
// the instance of a launch that needs `need`; -1: a forced instance that lacks a feature the arguments need
static int bn_small_instance(unsigned need) {
    const int forced = g_bn_small_forced.load(std::memory_order_relaxed);
    if (forced >= 0) return (need & ~(unsigned)forced) ? -1 : forced;
    for (unsigned m : BN_SMALL_INSTANCES)
        if (!(need & ~m)) return (int)m;
    return (int)BN_F_ALL;
}
#define BN_SMALL_PER_DISPATCH(HW_, KERNEL, F_, GRID, STREAM, ...)                                                 \
    do {                                                                                                          \
        if ((HW_) <= 256) SPLICE_LAUNCH((KERNEL<1, F_>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);            \
        else if ((HW_) <= 1024) SPLICE_LAUNCH((KERNEL<4, F_>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);      \
        else SPLICE_LAUNCH((KERNEL<16, F_>), GRID, dim3(256), 0, STREAM, __VA_ARGS__);                        \
    } while (0)
#define BN_SMALL_DISPATCH(INST_, HW_, KERNEL, GRID, STREAM, ...)                                                                      \
    switch (INST_) {                                                                                                                  \
    case 0: BN_SMALL_PER_DISPATCH(HW_, KERNEL, 0u, GRID, STREAM, __VA_ARGS__); break;                                                \
    case BN_F_SLABS: BN_SMALL_PER_DISPATCH(HW_, KERNEL, BN_F_SLABS, GRID, STREAM, __VA_ARGS__); break;                               \
    case BN_F_UP: BN_SMALL_PER_DISPATCH(HW_, KERNEL, BN_F_UP, GRID, STREAM, __VA_ARGS__); break;                                     \
    case BN_F_PRE | BN_F_UP: BN_SMALL_PER_DISPATCH(HW_, KERNEL, BN_F_PRE | BN_F_UP, GRID, STREAM, __VA_ARGS__); break;               \
    case BN_F_PRE | BN_F_UP | BN_F_SLABS: BN_SMALL_PER_DISPATCH(HW_, KERNEL, BN_F_PRE | BN_F_UP | BN_F_SLABS, GRID, STREAM, __VA_ARGS__); break; \
    case BN_F_BATCH: BN_SMALL_PER_DISPATCH(HW_, KERNEL, BN_F_BATCH, GRID, STREAM, __VA_ARGS__); break;                               \
    case BN_F_TAIL: BN_SMALL_PER_DISPATCH(HW_, KERNEL, BN_F_TAIL, GRID, STREAM, __VA_ARGS__); break;                                 \
    default: BN_SMALL_PER_DISPATCH(HW_, KERNEL, BN_F_ALL, GRID, STREAM, __VA_ARGS__); break;                                         \
    }
int bn_part_floats(int N, int C) { return N * C * MAX_PB_V * 2; }
// segments of a two-stage plane.  Big planes (round 5): segments of <= 4096 pixels moved in 16-byte runs, a count above MAX_PB; everything
// else keeps the 64-segment scalar layout
static inline int bn_plane_blocks(int HW) {
    if (!(HW > MAX_PB * 1024 && (long long)HW <= (long long)MAX_PB_V * BN_V_CH * 1024)) return plane_blocks(HW);
    const int b = cdiv(HW, 4096);
    return b <= MAX_PB ? MAX_PB + 1 : (b > MAX_PB_V ? MAX_PB_V : b);
}
// The one decision of which form a plane runs in and what the form absorbs (table: gen_kernels.h).  The launchers below dispatch on it and
// the engine plans with it, so a prediction cannot disagree with the dispatch.
BnForm bn_form(int HW, int N, size_t p_nstride, int batch) {
    static const int chain = getenv("SPLICE_BN_CHAIN") ? atoi(getenv("SPLICE_BN_CHAIN")) : 1;
    static const int bwd_slabs = getenv("SPLICE_BN_BWD_SLABS") ? atoi(getenv("SPLICE_BN_BWD_SLABS")) : 1;
    static const int sign_from_y = getenv("SPLICE_BN_SIGN_FROM_Y") ? atoi(getenv("SPLICE_BN_SIGN_FROM_Y")) : 1;
    // one image per parameter set (a single image, or independent generators) and per-image statistics: every image's workgroup reads
    // only its own plane -- what the mid kernels cover, and what lets a one-launch kernel take on a neighbour's work
    const bool own_plane = !batch && (N == 1 || p_nstride);
    BnForm f;
    f.kind = HW <= BN_SMALL_HW ? BnForm::SMALL
           : HW <= BN_MID_HW && own_plane ? BnForm::MID
           : bn_plane_blocks(HW) > MAX_PB ? BnForm::TWO_STAGE_VEC : BnForm::TWO_STAGE;
    const bool one_launch = f.kind == BnForm::SMALL || f.kind == BnForm::MID;
    // (chained or not, the skip branch's BatchNorm yields the same bits -- shared arithmetic helpers with pinned roundings,
    // tests/test_generator_gpu.py::test_launch_count_forms_are_bit_neutral -- so this is a pure launch-count choice.  With the chained
    // skip convolution's split-K slabs summed inside the concat kernel it wins at every batch size: -1.3 % step time at one pair per
    // GPU, -1.0 % at four, -0.6 % at eight; profiles/r04_gen_ab.txt.)
    f.hosts_pre = chain && own_plane && one_launch;
    // small planes: a split-K convolution leaves its slabs for the BatchNorm kernel, which adds them while it loads the plane
    f.fwd_takes_slabs = f.kind == BnForm::SMALL && !batch;
    f.bwd_takes_slabs = bwd_slabs && f.kind == BnForm::SMALL && own_plane;
    // batch statistics: the upsampled channels are materialised first (no fusion with the statistics pass) and their gradient takes
    // the adjoint's own launch; the two-stage backward never runs the adjoint
    f.fwd_fuses_upsample = !batch;
    f.bwd_fuses_upsample = !batch && one_launch;
    // big planes: the activation's sign is re-formed from y (needs beta; batch statistics keep reading the activated tensor: their mean / rstd arrays
    // are per image while the forward normalised with the batch's)
    f.sign_from_y = sign_from_y && !batch && f.kind == BnForm::TWO_STAGE_VEC;
    return f;
}
// the argument checks under the engine: a batch the kernels do not cover, a BnPre / slabs on a form that cannot take them
static bool bn_args_ok(const BnArgs& a, const BnForm& f) {
    if (a.batch && (a.batch > BN_MAX_BATCH || a.N % a.batch || (a.N != a.batch && !a.p_nstride))) return false;
    if (a.pre && !f.hosts_pre) return false;
    if (a.slabs && (!f.fwd_takes_slabs || a.ksplit < 2 || a.up || a.pre)) return false;
    if (a.da_slabs && a.da_slabs->slabs && !f.bwd_takes_slabs) return false;
    return true;
}
int bn_fwd_launch(const BnArgs& a, hipStream_t s) {
    const BnForm f = bn_form(a.HW, a.N, a.p_nstride, a.batch);
    if (!bn_args_ok(a, f)) return SPLICE_ERR_ARG;
    const int N = a.N, C = a.C, HW = a.HW;
    const bool fused_up = a.up && f.fwd_fuses_upsample;
    if (a.up && !fused_up) {   // the upsampled channels are materialised in y by a launch of their own, in front
        const int rc = upsample2x_fwd_launch(a.up->src, a.up->src_ns, const_cast<float*>(a.y) + (size_t)a.up->c0 * HW, a.y_nstride, N, C - a.up->c0, a.up->h,
                                             a.up->w, a.up->Ho, a.up->Wo, s);
        if (rc != SPLICE_OK) return rc;
    }
    const BnUpsample u = fused_up ? *a.up : BnUpsample{};
    const BnPre pr = a.pre ? *a.pre : BnPre{};
    switch (f.kind) {
    case BnForm::SMALL: {
        const int ksplit = a.slabs ? a.ksplit : 0;
        const float* bias = a.slabs ? a.bias : nullptr;
        float* y_store = a.slabs ? const_cast<float*>(a.y) : nullptr;
        const int inst = bn_small_instance((a.batch ? BN_F_BATCH : 0) | (a.slabs || pr.slabs ? BN_F_SLABS : 0) | (pr.y ? BN_F_PRE : 0) | (u.src ? BN_F_UP : 0));
        if (inst < 0) return SPLICE_ERR_ARG;
        BN_SMALL_DISPATCH(inst, HW, bn_small_fwd_kernel, dim3(C, N), s, a.y, a.y_nstride, a.out, a.out_nstride, C, HW, a.gamma, a.beta, a.eps, a.mean, a.rstd, a.slope,
                          a.slabs, ksplit, bias, y_store, u, a.p_nstride, a.batch, pr);
        break;
    }
    case BnForm::MID:
        bn_mid_allow_lds();
        SPLICE_LAUNCH(bn_mid_fwd_kernel, dim3(C, N), dim3(BN_MID_THREADS), (size_t)(((HW + 3) & ~3) + (u.src ? BN_MID_SRC : 0)) * 4, s, a.y, a.y_nstride, a.out, a.out_nstride, C, HW, a.gamma, a.beta, a.eps, a.mean, a.rstd, a.slope, u, a.p_nstride, pr);
        break;
    case BnForm::TWO_STAGE:
    case BnForm::TWO_STAGE_VEC: {
        const int PB = bn_plane_blocks(HW);
        if (f.kind == BnForm::TWO_STAGE_VEC) SPLICE_LAUNCH(bn_stats_partial_v_kernel, dim3(PB, C, N), dim3(256), 0, s, a.y, a.y_nstride, C, HW, PB, a.part, u);
        else SPLICE_LAUNCH(bn_stats_partial_kernel, dim3(PB, C, N), dim3(256), 0, s, a.y, a.y_nstride, C, HW, PB, a.part, u);
        SPLICE_LAUNCH(bn_act_kernel, dim3(PB, C, N), dim3(256), 0, s, a.y, a.y_nstride, a.out, a.out_nstride, C, HW, PB, a.gamma, a.beta, a.part, a.eps, a.mean, a.rstd, a.slope, a.p_nstride, a.batch);
        break;
    }
    }
    return SPLICE_OK;
}
int bn_bwd_launch(const BnArgs& a, hipStream_t s) {
    const BnForm f = bn_form(a.HW, a.N, a.p_nstride, a.batch);
    if (!bn_args_ok(a, f)) return SPLICE_ERR_ARG;
    const int N = a.N, C = a.C, HW = a.HW;
    const bool fused_up = a.up && f.bwd_fuses_upsample;
    const BnUpsample u = fused_up ? *a.up : BnUpsample{};
    const BnPre pr = a.pre ? *a.pre : BnPre{};
    switch (f.kind) {
    case BnForm::SMALL: {
        const BnSlabs sl = a.da_slabs ? *a.da_slabs : BnSlabs{};
        const int inst = bn_small_instance((a.batch ? BN_F_BATCH : 0) | (!a.batch && !a.p_nstride && N > 1 ? BN_F_TAIL : 0) | (sl.slabs ? BN_F_SLABS : 0) |
                                           (pr.y ? BN_F_PRE : 0) | (u.d_src ? BN_F_UP : 0));
        if (inst < 0) return SPLICE_ERR_ARG;
        BN_SMALL_DISPATCH(inst, HW, bn_small_bwd_kernel, dim3(C, N), s, a.da, a.da_nstride, a.out, a.out_nstride, a.y, a.y_nstride, a.dy, a.dy_nstride, C, HW, N,
                          a.gamma, a.mean, a.rstd, a.slope, a.dgamma, a.dbeta, a.accumulate, u, a.p_nstride, a.batch, pr, sl);
        break;
    }
    case BnForm::MID:
        bn_mid_allow_lds();
        SPLICE_LAUNCH(bn_mid_bwd_kernel, dim3(C, N), dim3(BN_MID_THREADS), (size_t)HW * 4, s, a.da, a.da_nstride, a.out, a.out_nstride, a.y, a.y_nstride, a.dy, a.dy_nstride, C, HW, a.gamma, a.mean,
                      a.rstd, a.slope, a.dgamma, a.dbeta, a.accumulate, u, a.p_nstride, pr);
        break;
    case BnForm::TWO_STAGE:
    case BnForm::TWO_STAGE_VEC: {
        const int PB = bn_plane_blocks(HW);
        const float* be = f.sign_from_y ? a.beta : nullptr;
        SPLICE_LAUNCH(bn_bwd_partial_kernel, dim3(PB, C, N), dim3(256), 0, s, a.da, a.da_nstride, a.out, a.out_nstride, a.y, a.y_nstride, C, HW, PB, a.mean, a.rstd, a.slope, a.part, a.gamma, be, a.p_nstride);
        SPLICE_LAUNCH(bn_bwd_apply_kernel, dim3(PB, C, N), dim3(256), 0, s, a.da, a.da_nstride, a.out, a.out_nstride, a.y, a.y_nstride, a.dy,
                           a.dy_nstride, C, HW, N, PB, a.gamma, a.mean, a.rstd, a.slope, a.part, a.dgamma, a.dbeta, a.accumulate, a.p_nstride, a.batch, be);
        break;
    }
    }
    // the upsampled channels' gradient sits in dy: through the adjoint in a launch of its own where the form did not run it
    if (a.up && !fused_up)
        return upsample2x_bwd_launch(a.dy + (size_t)a.up->c0 * HW, a.dy_nstride, a.up->d_src, a.up->d_src_ns, N, C - a.up->c0, a.up->h, a.up->w, a.up->Ho, a.up->Wo, s);
    return SPLICE_OK;
}

// ---------------------------------------------------------------------------------------
// nn.BatchNorm2d bookkeeping (models/unet/common.py:95-96: every netG call in train mode moves running_mean / running_var
// with momentum 0.1; nothing ever reads them, but they are part of netG.state_dict()).  One launch covers every
// BatchNorm of up to RUNSTAT_MAX_PLANS generator calls IN CALL ORDER: thread (bn, channel) walks the plans in order (the
// updates of one buffer do not commute exactly), and the images of a plan in order unless they are independent
// generators (blockIdx.y = image = its own buffer arena).  var_unbiased is rebuilt from the saved rstd.
// MASKED (the plateau stop rule, plateau.h): the buffer arena of a slot that is frozen at this step (index *mask_step - 1) is not
// touched.  The slot is the arena: blockIdx.y for independent images and for grouped plans (t.N counts a grouped plan's groups, so
// this is image / group size), 0 for a plan that is one generator.
template <bool MASKED>
__global__ __launch_bounds__(256) void bn_running_update_kernel(RunStatTable t, float* __restrict__ running, size_t r_nstride, float momentum, float eps,
                                                                const splice_stop_state* __restrict__ mask, const int* __restrict__ mask_step) {
    const int bn = blockIdx.x, c = threadIdx.x;
    if (c >= t.C[bn]) return;
    const int step_idx = MASKED ? *mask_step - 1 : 0;
    for (int p = 0; p < t.n_plans; ++p) {
        const bool indep = t.indep[p] != 0;
        if (indep && (int)blockIdx.y >= t.N[p]) continue;
        if (!indep && blockIdx.y != 0) continue;
        if (MASKED && stop_frozen(mask + (indep ? blockIdx.y : 0), step_idx)) continue;
        const int n_lo = indep ? blockIdx.y : 0, n_hi = indep ? blockIdx.y + 1 : t.N[p];
        const int step = t.img_step[p] > 1 ? t.img_step[p] : 1;   // grouped plans: update n reads the statistics of its group's first image
        float* arena = running + (indep ? (size_t)blockIdx.y * r_nstride : 0) + t.r_off[bn];
        const float hw = (float)t.HW[p][bn];
        const float unbias = hw > 1.f ? hw / (hw - 1.f) : 1.f;
        for (int n = n_lo; n < n_hi; ++n) {
            const float m = t.mean[p][bn][n * step * t.C[bn] + c], r = t.rstd[p][bn][n * step * t.C[bn] + c];
            const float var = fmaxf(1.0f / (r * r) - eps, 0.f) * unbias;
            arena[c] = (1.f - momentum) * arena[c] + momentum * m;
            arena[t.C[bn] + c] = (1.f - momentum) * arena[t.C[bn] + c] + momentum * var;
        }
    }
}
int bn_running_update_launch(const RunStatTable& t, float* running, size_t r_nstride, float momentum, float eps, int max_images, hipStream_t s,
                             const splice_stop_state* mask, const int* mask_step) {
    if (t.n_plans < 1 || t.n_plans > RUNSTAT_MAX_PLANS || t.n_bn < 1 || t.n_bn > RUNSTAT_MAX_BN || (mask && !mask_step)) return SPLICE_ERR_ARG;
    // one thread per channel: the concat BatchNorm of an architecture within arch_check has up to 128 + 128 = 256 channels
    if (mask) SPLICE_LAUNCH(bn_running_update_kernel<true>, dim3(t.n_bn, max_images), dim3(256), 0, s, t, running, r_nstride, momentum, eps, mask, mask_step);
    else SPLICE_LAUNCH(bn_running_update_kernel<false>, dim3(t.n_bn, max_images), dim3(256), 0, s, t, running, r_nstride, momentum, eps, mask, mask_step);
    return SPLICE_OK;
}
