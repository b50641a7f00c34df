// Pointwise kernels of the generator (see gen_conv.hip for the family overview): the x2 bilinear upsampling and its adjoint as launches
// of their own (where a BatchNorm form does not absorb them), and the sigmoid head's backward with the head bias gradient.
#include "gen_device.h"

// ---------------------------------------------------------------------------------------
// bilinear x2 (align_corners=False) of in[C][h][w] -> the top-left Ho x Wo window of the 2h x 2w
// result (Concat's centre-crop offset is always 0 here: models/unet/common.py:24-37).
__global__ __launch_bounds__(256) void upsample2x_fwd_kernel(const float* __restrict__ in, size_t in_nstride, float* __restrict__ out,
                                                             size_t out_nstride, int C, int h, int w, int Ho, int Wo) {
    const int c = blockIdx.y, img = blockIdx.z;
    const float* p = in + (size_t)img * in_nstride + (size_t)c * h * w;
    float* q = out + (size_t)img * out_nstride + (size_t)c * Ho * Wo;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < Ho * Wo; i += gridDim.x * 256) {
        q[i] = up_value(p, h, w, i / Wo, i % Wo);
    }
}
__global__ __launch_bounds__(256) void upsample2x_bwd_kernel(const float* __restrict__ dout, size_t dout_nstride, float* __restrict__ din,
                                                             size_t din_nstride, int C, int h, int w, int Ho, int Wo) {
    const int c = blockIdx.y, img = blockIdx.z;
    const float* p = dout + (size_t)img * dout_nstride + (size_t)c * Ho * Wo;
    float* q = din + (size_t)img * din_nstride + (size_t)c * h * w;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < h * w; i += gridDim.x * 256) {
        // adjoint weights of the x2 bilinear (align_corners=False) in closed form: output o = 2m-1+t, t = 0..3, reads input m
        // with weight {1/4, 3/4, 3/4, 1/4}; at the borders the clamped source index folds the missing neighbour's share
        // in (o = 0 and o = 2n-1 read their input pixel with weight 1), and outputs outside the Ho x Wo window do not exist.
        // All 16 taps are loaded unconditionally from clamped coordinates (a zero weight marks the taps that do not exist).
        q[i] = up_adjoint_value(p, h, w, Ho, Wo, i / w, i % w);
    }
}
int upsample2x_fwd_launch(const float* in, size_t in_nstride, float* out, size_t out_nstride, int N, int C, int h, int w, int Ho, int Wo, hipStream_t s) {
    SPLICE_LAUNCH(upsample2x_fwd_kernel, dim3(plane_blocks(Ho * Wo), C, N), dim3(256), 0, s, in, in_nstride, out, out_nstride, C, h, w, Ho, Wo);
    return SPLICE_OK;
}
int upsample2x_bwd_launch(const float* dout, size_t dout_nstride, float* din, size_t din_nstride, int N, int C, int h, int w, int Ho, int Wo, hipStream_t s) {
    SPLICE_LAUNCH(upsample2x_bwd_kernel, dim3(cdiv(h * w, 256), C, N), dim3(256), 0, s, dout, dout_nstride, din, din_nstride, C, h, w, Ho, Wo);
    return SPLICE_OK;
}

// ---------------------------------------------------------------------------------------
// dpre = dout * s * (1 - s) and the per-segment sums of dpre for the head bias gradient: block (pb, c) handles segment pb of
// channel c over every image (gridDim.z > 1: independent images -- blockIdx.z = image, partials per image).  The partials are laid
// out [image][segment][channel] = the [chunk][element] layout of the weight-gradient partials, so the backward's ONE
// wgrad_reduce_all launch sums them with everything else (round 4: the bias had a reduce launch of its own).
__global__ __launch_bounds__(256) void sigmoid_bwd_bias_kernel(const float* __restrict__ dout, const float* __restrict__ sout,
                                                               float* __restrict__ dpre, int N, int C, int HW, int PB,
                                                               float* __restrict__ part, int per) {
    __shared__ float red[8];
    const int pb = blockIdx.x, c = blockIdx.y;
    const int seg = seg_len(HW, PB), lo = pb * seg, hi = min(lo + seg, HW);
    float acc = 0.f, dummy = 0.f;
    const int n_lo = gridDim.z > 1 ? blockIdx.z * per : 0, n_hi = gridDim.z > 1 ? n_lo + per : N;
    part += (size_t)(gridDim.z > 1 ? blockIdx.z : 0) * C * PB;
    for (int n = n_lo; n < n_hi; ++n) {
        const size_t base = ((size_t)n * C + c) * HW;
        for (int i = lo + threadIdx.x; i < hi; i += 256) {
            const float sv = sout[base + i];
            const float d = dout[base + i] * sv * (1.f - sv);
            dpre[base + i] = d;
            acc += d;
        }
    }
    block_sum2(acc, dummy, red);
    if (threadIdx.x == 0) part[pb * C + c] = acc;
}
// returns the number of partial "chunks" per parameter (for the reduce entry): PB, or N / group * PB for independent images / groups
// of `group` images (blockIdx.z = group: its images in image order, as the one-group path walks them)
int sigmoid_bwd_bias_launch(const float* dout, const float* sout, float* dpre, int N, int C, int HW, float* part, hipStream_t s, size_t p_nstride, int* chunks,
                            int group) {
    const int PB = plane_blocks(HW);
    const int per = group > 1 ? group : 1;
    const int nz = p_nstride ? N / per : 1;
    SPLICE_LAUNCH(sigmoid_bwd_bias_kernel, dim3(PB, C, nz), dim3(256), 0, s, dout, sout, dpre, N, C, HW, PB, part, per);
    if (chunks) *chunks = PB * nz;
    return SPLICE_OK;
}
int sigmoid_bias_part_floats(int N, int C) { return N * C * MAX_PB; }
