// The two image-space loss terms of the fused step, on the generator's outputs at the crops' own resolution:
//   total variation of x' = G(A_crop):   TV(x) = mean |x[:,1:,:] - x[:,:-1,:]| + mean |x[:,:,1:] - x[:,:,:-1]|   per image [3][h][w], each mean over
//                                        its own count nv = 3 (h - 1) w / nh = 3 h (w - 1); a direction without differences contributes 0
//   pixel identity of y' = G(B_crop):    mean((y' - B_crop)^2) over 3 h w
// One VALUE launch at the loss stage writes fixed-order partial sums into the step's partials buffer (terms 6 and 7), which the total-loss
// kernel adds like every other term's; one GRADIENT-ADD launch per backward chain adds lambda * d(term)/d(image) into the chain's image
// gradient in place, recomputing the stencil from the saved generator output.  No float atomics, no scratch image.  All global accesses
// are single dwords, lane i at element i of a plane: crop widths are odd in general (213, 855), a row then starts at any dword, and both
// kernels move a few hundred KiB once -- there is no 16-byte path and therefore no ragged tail.
#include "kernels.h"

// the value kernel: one workgroup of 256 threads per IMAGE_TERMS_CHUNK consecutive floats of an image, counted from the image's start --
// thread t takes elements t, t + 256, ... of its chunk in that order, the 256 sums meet in the wave tree (wave_sum) and the four waves'
// results are added in wave order.  The grid of an image depends on h and w only, so its partials have the same bits whichever batch
// it rides in and wherever it stands in it.
struct ImageValueTerm {
    const float* x;       // [n_img][3][h][w]   the generated images
    const float* ref;     // pixel identity: the images they are compared with (same layout); TV: unused
    float* part;          // image i's partials at part + i * part_istride, one float per chunk
    int n_img, h, w, tv;  // tv != 0: total variation; else pixel identity
};
struct ImageValueArgs { ImageValueTerm t[2]; size_t part_istride; };

__global__ __launch_bounds__(256) void image_terms_value_kernel(ImageValueArgs a) {
    const ImageValueTerm& t = a.t[blockIdx.z];
    const unsigned n = 3u * (unsigned)t.h * (unsigned)t.w, c0 = blockIdx.x * (unsigned)IMAGE_TERMS_CHUNK;
    if ((int)blockIdx.y >= t.n_img || c0 >= n) return;   // (the grid covers the larger of the two terms)
    const float* x = t.x + (size_t)blockIdx.y * n;
    const unsigned h = (unsigned)t.h, w = (unsigned)t.w;
    float s0 = 0.f, s1 = 0.f;   // TV: vertical / horizontal addends; pixel identity: squared differences / unused
    if (t.tv) {
#pragma unroll 4
        for (unsigned j = 0; j < IMAGE_TERMS_CHUNK / 256; ++j) {
            const unsigned i = c0 + j * 256 + threadIdx.x;
            if (i < n) {
                const unsigned r = i / w, col = i - r * w, row = r % h;
                const float v = x[i];
                // (a row's last pixel has no right neighbour, a plane's last row none below: i + 1 / i + w would be the next row / plane)
                if (row + 1 < h) s0 += fabsf(x[i + w] - v);
                if (col + 1 < w) s1 += fabsf(x[i + 1] - v);
            }
        }
    } else {
        const float* b = t.ref + (size_t)blockIdx.y * n;
#pragma unroll 4
        for (unsigned j = 0; j < IMAGE_TERMS_CHUNK / 256; ++j) {
            const unsigned i = c0 + j * 256 + threadIdx.x;
            if (i < n) {
                const float d = x[i] - b[i];
                s0 = __builtin_fmaf(d, d, s0);
            }
        }
    }
    __shared__ float red[2][4];
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s0; red[1][threadIdx.x >> 6] = s1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float a0 = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3], a1 = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        float out;
        if (t.tv) {
            const unsigned nv = 3u * (h - 1) * w, nh = 3u * h * (w - 1);
            out = (nv ? a0 / (float)nv : 0.f) + (nh ? a1 / (float)nh : 0.f);
        } else {
            out = a0 / (float)n;
        }
        t.part[(size_t)blockIdx.y * a.part_istride + blockIdx.x] = out;
    }
}

static bool image_shape_ok(int n_img, int h, int w) {
    // 3 h w below 2^31 - 2^16 (unsigned element indices with room for the last chunk), planes within grid.y
    return n_img >= 1 && h >= 1 && w >= 1 && (unsigned long long)3 * h * w < 0x7fff0000ull && (long long)3 * n_img <= 65535;
}
static unsigned image_chunks(int h, int w) { return (unsigned)(((size_t)3 * h * w + IMAGE_TERMS_CHUNK - 1) / IMAGE_TERMS_CHUNK); }

int image_terms_value_launch(const float* x, int n_x, int xh, int xw, float* part_tv, const float* y, const float* b, int n_y, int yh, int yw,
                             float* part_pix, size_t part_istride, size_t part_cap, hipStream_t s) {
    if (!x && !y) return SPLICE_OK;   // both terms off: nothing is launched, nothing is read
    ImageValueArgs a = {};
    a.part_istride = part_istride;
    unsigned nt = 0, chunks = 0;
    int imgs = 0;
    if (x) {
        if (!part_tv || !image_shape_ok(n_x, xh, xw) || image_chunks(xh, xw) > part_cap) {
            splice_set_error("image_terms_value_launch: %d image(s) [3][%d][%d] need %u partial slots, the buffer has %zu", n_x, xh, xw, image_chunks(xh, xw), part_cap);
            return SPLICE_ERR_ARG;
        }
        a.t[nt++] = ImageValueTerm{x, nullptr, part_tv, n_x, xh, xw, 1};
        chunks = image_chunks(xh, xw); imgs = n_x;
    }
    if (y) {
        if (!b || !part_pix || !image_shape_ok(n_y, yh, yw) || image_chunks(yh, yw) > part_cap) {
            splice_set_error("image_terms_value_launch: %d image(s) [3][%d][%d] need %u partial slots, the buffer has %zu", n_y, yh, yw, image_chunks(yh, yw), part_cap);
            return SPLICE_ERR_ARG;
        }
        a.t[nt++] = ImageValueTerm{y, b, part_pix, n_y, yh, yw, 0};
        if (image_chunks(yh, yw) > chunks) chunks = image_chunks(yh, yw);
        if (n_y > imgs) imgs = n_y;
    }
    SPLICE_LAUNCH(image_terms_value_kernel, dim3(chunks, (unsigned)imgs, nt), dim3(256), 0, s, a);
    return SPLICE_OK;
}

// The gradient-add kernels: blockIdx.y = plane (image * 3 + channel), one thread per pixel of the plane.  The coefficients are doubles and
// the term's gradient is formed in double from exact integer signs (TV) or the exact difference of the two fp32 pixels (pixel identity),
// then rounded to fp32 once and added: two roundings per element in all.  sign(0) = 0, as torch.abs gives under autograd; the sign is that of
// the fp32 subtraction the value kernel takes the absolute value of.
__device__ __forceinline__ int sign_of(float t) { return (t > 0.f) - (t < 0.f); }

__global__ __launch_bounds__(256) void image_tv_grad_add_kernel(const float* __restrict__ x, float* __restrict__ d, int h, int w, double cv, double ch) {
    const unsigned hw = (unsigned)h * (unsigned)w, q = blockIdx.x * 256u + threadIdx.x;
    if (q >= hw) return;
    const size_t base = (size_t)blockIdx.y * hw;
    const float* xp = x + base;
    const unsigned row = q / (unsigned)w, col = q - row * (unsigned)w;
    const float v = xp[q];
    // pixel (row, col) is the minuend of the difference with its upper / left neighbour and the subtrahend of the one with its lower /
    // right neighbour; border pixels have one neighbour per direction
    int sv = 0, sh = 0;
    if (row > 0) sv += sign_of(v - xp[q - w]);
    if (row + 1 < (unsigned)h) sv -= sign_of(xp[q + w] - v);
    if (col > 0) sh += sign_of(v - xp[q - 1]);
    if (col + 1 < (unsigned)w) sh -= sign_of(xp[q + 1] - v);
    d[base + q] += (float)(cv * (double)sv + ch * (double)sh);
}
__global__ __launch_bounds__(256) void image_pix_grad_add_kernel(const float* __restrict__ y, const float* __restrict__ b, float* __restrict__ d, unsigned hw,
                                                                 double c) {
    const unsigned q = blockIdx.x * 256u + threadIdx.x;
    if (q >= hw) return;
    const size_t i = (size_t)blockIdx.y * hw + q;
    d[i] += (float)(c * ((double)y[i] - (double)b[i]));
}

// d[n_img][3][h][w] += lambda * dTV/dx of every image: the normalisers come from this launch's h and w
int image_tv_grad_add_launch(const float* x, float* d, int n_img, int h, int w, float lambda, hipStream_t s) {
    if (!x || !d || !image_shape_ok(n_img, h, w) || !(lambda >= 0.f)) { splice_set_error("image_tv_grad_add_launch: invalid argument"); return SPLICE_ERR_ARG; }
    const double nv = 3.0 * (h - 1) * w, nh = 3.0 * h * (w - 1);
    const unsigned hw = (unsigned)h * (unsigned)w;
    SPLICE_LAUNCH(image_tv_grad_add_kernel, dim3((hw + 255) / 256, 3u * n_img), dim3(256), 0, s, x, d, h, w, nv > 0 ? (double)lambda / nv : 0.0,
                  nh > 0 ? (double)lambda / nh : 0.0);
    return SPLICE_OK;
}
// d[n_img][3][h][w] += lambda * 2 (y - b) / (3 h w)
int image_pix_grad_add_launch(const float* y, const float* b, float* d, int n_img, int h, int w, float lambda, hipStream_t s) {
    if (!y || !b || !d || !image_shape_ok(n_img, h, w) || !(lambda >= 0.f)) { splice_set_error("image_pix_grad_add_launch: invalid argument"); return SPLICE_ERR_ARG; }
    const unsigned hw = (unsigned)h * (unsigned)w;
    SPLICE_LAUNCH(image_pix_grad_add_kernel, dim3((hw + 255) / 256, 3u * n_img), dim3(256), 0, s, y, b, d, hw, 2.0 * (double)lambda / (3.0 * h * w));
    return SPLICE_OK;
}
