// How exact is v_mfma_f32_16x16x32_fp8_fp8?  One wave, one 16x16 output, K = 64 as two chained instructions (what the e4m3 attention forward
// issues per score block).  Designed operands show where product bits are dropped inside an instruction; random N(0, 1) e4m3 operands give the
// size of the error against an exact dot.  Result (profiles/mfma8_accuracy.txt): products are aligned to the largest exponent sum of the
// instruction's operand pairs and lose every bit below 2^-13 of it; oracle/attention.py::fp8_score_bound builds on that rule.
//   hipcc --offload-arch=gfx950 -O2 -o mfma8_accuracy tools/micro/mfma8_accuracy.hip && ./mfma8_accuracy
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cmath>
#include <vector>
#include <random>
typedef float f32x4 __attribute__((ext_vector_type(4)));
__global__ void probe(const uint8_t* A, const uint8_t* B, float* Dm, float c0) {   // A [16][64], B [16][64] (row n = column n of B^T), D [16][16]
    const int lane = threadIdx.x, r = lane & 15, g = lane >> 4;
    long a0 = *reinterpret_cast<const long*>(A + r * 64 + g * 8), a1 = *reinterpret_cast<const long*>(A + r * 64 + 32 + g * 8);
    long b0 = *reinterpret_cast<const long*>(B + r * 64 + g * 8), b1 = *reinterpret_cast<const long*>(B + r * 64 + 32 + g * 8);
    f32x4 acc = {c0, c0, c0, c0};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(a1, b1, acc, 0, 0, 0);
    for (int i = 0; i < 4; ++i) Dm[(g * 4 + i) * 16 + r] = acc[i];   // D[row = 4 g + i (A row)][col = r (B row)]
}
static float e4m3_dec(uint8_t v) {
    int s = v >> 7, e = (v >> 3) & 15, m = v & 7;
    float x = e == 0 ? ldexpf((float)m, -9) : ldexpf(1.0f + m / 8.0f, e - 7);
    return s ? -x : x;
}
static uint8_t e4m3_enc(float x) {   // nearest, by search (probe only)
    uint8_t best = 0; float bd = 1e30f;
    for (int v = 0; v < 256; ++v) { if ((v & 0x7F) == 0x7F) continue; float d = fabsf(e4m3_dec((uint8_t)v) - x); if (d < bd) { bd = d; best = (uint8_t)v; } }
    return best;
}
static void run(const std::vector<uint8_t>& A, const std::vector<uint8_t>& B, float c0, std::vector<float>& D) {
    uint8_t *dA, *dB; float* dD;
    hipMalloc(&dA, 1024); hipMalloc(&dB, 1024); hipMalloc(&dD, 1024);
    hipMemcpy(dA, A.data(), 1024, hipMemcpyHostToDevice); hipMemcpy(dB, B.data(), 1024, hipMemcpyHostToDevice);
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, dA, dB, dD, c0);
    D.resize(256);
    hipMemcpy(D.data(), dD, 1024, hipMemcpyDeviceToHost);
    hipFree(dA); hipFree(dB); hipFree(dD);
}
int main() {
    std::vector<uint8_t> A(1024), B(1024); std::vector<float> D;
    // test 1: cancellation inside ONE instruction: +big, -big, small; small = 1.875 * 1.875 * 2^-s (8 significant bits), big = (mb * 16)^2, mb = 1 or 1.875
    for (int mb = 0; mb < 2; ++mb) {
        float bigv = mb ? 30.f : 16.f;
        std::fill(A.begin(), A.end(), 0); std::fill(B.begin(), B.end(), 0);
        for (int i = 0; i < 16; ++i) {
            int e = i < 8 ? i : 8;
            A[i * 64] = e4m3_enc(bigv); A[i * 64 + 1] = e4m3_enc(bigv); A[i * 64 + 2] = e4m3_enc(ldexpf(1.875f, -e));
            B[i * 64] = e4m3_enc(bigv); B[i * 64 + 1] = e4m3_enc(-bigv); B[i * 64 + 2] = e4m3_enc(ldexpf(1.875f, -e));
        }
        run(A, B, 0.f, D);
        printf("cancel test, big product %g: small = 225 * 2^-(s+6) -> got in units of 2^-(s+6)\n", bigv * bigv);
        for (int s = 0; s <= 16; ++s) { int i = s < 8 ? s : 8, n = s - i; printf("  s=%d (top bit 2^%d, lowest bit 2^%d): %g\n", s, 1 - s, -6 - s, D[i * 16 + n] * ldexp(1.0, s + 6)); }
    }
    // test 2: random N(0, 1) e4m3 operands, K = 64: error against the exact dot in units of u * sum|ab| and of u * 64 * max|ab|
    std::mt19937 rng(5); std::normal_distribution<float> nd(0.f, 1.f);
    double worst_sum = 0, worst_max = 0, sq = 0; int cnt = 0;
    for (int rep = 0; rep < 200; ++rep) {
        for (auto& x : A) x = e4m3_enc(nd(rng));
        for (auto& x : B) x = e4m3_enc(nd(rng));
        run(A, B, 0.f, D);
        for (int i = 0; i < 16; ++i) for (int n = 0; n < 16; ++n) {
            double ex = 0, sa = 0, mx = 0;
            for (int k = 0; k < 64; ++k) { double p = (double)e4m3_dec(A[i * 64 + k]) * e4m3_dec(B[n * 64 + k]); ex += p; sa += fabs(p); mx = fmax(mx, fabs(p)); }
            double err = fabs((double)D[i * 16 + n] - ex), u = ldexp(1.0, -24);
            worst_sum = fmax(worst_sum, err / (u * sa)); worst_max = fmax(worst_max, err / (u * 64 * mx)); sq += err * err / (sa * sa); ++cnt;
            if (rep == 0 && i == 0 && n < 2) printf("  sample: got %.9g exact %.12g sum|ab| %.6g\n", D[i * 16 + n], ex, sa);
        }
    }
    printf("random K=64: worst err / (u sum|ab|) = %.1f, worst err / (u 64 max|ab|) = %.1f, rms err / sum|ab| = %.3g (u = 2^-24)\n", worst_sum, worst_max, sqrt(sq / cnt));
    return 0;
}
