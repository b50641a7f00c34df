// extern "C" op-level entry points of include/splice_hip.h (thin argument checks + launch).
#include <stdarg.h>
#include <stdio.h>

#include "kernels.h"

static thread_local char g_err[512] = "";

void splice_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int finish(int rc, const char* what) {
    if (rc != SPLICE_OK) {
        splice_set_error("%s: invalid argument", what);
        return rc;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        splice_set_error("%s: HIP error %d (%s)", what, (int)e, hipGetErrorString(e));
        return SPLICE_ERR_HIP;
    }
    return SPLICE_OK;
}

#define ST(s) ((hipStream_t)(s))

extern "C" {

int splice_version(void) { return 100; }
int splice_dev_switches(void) {
#ifdef SPLICE_DEV_SWITCHES
    return 1;
#else
    return 0;
#endif
}
const char* splice_last_error(void) { return g_err; }

int splice_gemm_nt_bf16(unsigned flags, const splice_bf16* A, int lda, const splice_bf16* B, int ldb, int M, int N, int K,
                        const splice_gemm_epilogue* epi, splice_stream_t stream) {
    if (!A || !B || !epi) return finish(SPLICE_ERR_ARG, "splice_gemm_nt_bf16");
    return finish(gemm_nt_launch(flags, A, lda, B, ldb, M, N, K, *epi, ST(stream)), "splice_gemm_nt_bf16");
}

int splice_gemm_nt_fp8(unsigned flags, const uint8_t* A, int lda, const uint8_t* B, int ldb, int M, int N, int K,
                       const splice_gemm_epilogue* epi, splice_stream_t stream) {
    if (!A || !B || !epi) return finish(SPLICE_ERR_ARG, "splice_gemm_nt_fp8");
    return finish(gemm_nt_fp8_launch(flags, A, lda, B, ldb, M, N, K, *epi, ST(stream)), "splice_gemm_nt_fp8");
}
int splice_quantize_rows_fp8(const float* x, int ldx, uint8_t* q, int ldq, float* scale, int rows, int cols, splice_stream_t stream) {
    if (!x || !q || !scale) return finish(SPLICE_ERR_ARG, "splice_quantize_rows_fp8");
    return finish(quantize_rows_fp8_launch(x, ldx, q, ldq, scale, rows, cols, ST(stream)), "splice_quantize_rows_fp8");
}

int splice_gemm_splitk_slabs(int M, int ksplit) { return gemm_splitk_slabs(M, ksplit); }

/* benchmarking hook: force the GEMM tile (0 auto, 1 128x128, 2 128x64, 3 64x64) */
int splice_gemm_force_tile(int tile) { gemm_force_tile(tile); return SPLICE_OK; }
int splice_attention_variant(int variant) { attn_set_variant(variant); return SPLICE_OK; }
int splice_attention_qfold(int on) { attn_set_qfold(on); return SPLICE_OK; }
int splice_attention_bwd_variant(int variant) { attn_set_bwd_variant(variant); return SPLICE_OK; }

int splice_layernorm_fwd(const float* x, const float* gamma, const float* beta, splice_bf16* y, float* mean, float* rstd,
                         int rows, int D, float eps, splice_stream_t stream) {
    return finish(layernorm_fwd_launch(x, gamma, beta, y, mean, rstd, rows, D, eps, ST(stream)), "splice_layernorm_fwd");
}
int splice_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                         const float* g_in, float* g_out, splice_bf16* g_out_bf, int rows, int D, splice_stream_t stream) {
    return finish(layernorm_bwd_launch(dy, x, gamma, mean, rstd, g_in, g_out, g_out_bf, rows, D, ST(stream)), "splice_layernorm_bwd");
}

int splice_attention_fwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld, int D, int H,
                         float scale, splice_bf16* out, float* lse, splice_stream_t stream) {
    AttnArgs a = {};
    a.qkv = qkv; a.qkvT = qkvT; a.ldt = ldt; a.B = B; a.T = T; a.Tld = Tld; a.D = D; a.H = H; a.scale = scale;
    a.out = out; a.lse = lse; a.qfold = attn_qfold_hook();
    return finish(attn_fwd_launch(&a, ST(stream)), "splice_attention_fwd");
}
int splice_attention_fwd_fp8(const uint8_t* qkv8, const uint8_t* qkvT8, int ldt8, int B, int T, int Tld, int D, int H, float scale,
                             splice_bf16* out, float* lse, splice_stream_t stream) {
    if (!qkv8 || !qkvT8 || !out || !lse) return finish(SPLICE_ERR_ARG, "splice_attention_fwd_fp8");
    AttnArgs a = {};
    a.qkv8 = qkv8; a.qkvT8 = qkvT8; a.ldt8 = ldt8; a.ldt = 4; a.B = B; a.T = T; a.Tld = Tld; a.D = D; a.H = H; a.scale = scale;
    a.out = out; a.lse = lse;
    return finish(attn_fwd_launch(&a, ST(stream)), "splice_attention_fwd_fp8");
}
int splice_attention_bwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld, int D, int H,
                         float scale, const splice_bf16* out, const float* lse, const splice_bf16* dout,
                         const splice_bf16* doutT, float* delta, splice_bf16* dqkv, splice_stream_t stream) {
    AttnArgs a = {};
    a.qkv = qkv; a.qkvT = qkvT; a.ldt = ldt; a.B = B; a.T = T; a.Tld = Tld; a.D = D; a.H = H; a.scale = scale;
    a.out = const_cast<splice_bf16*>(out); a.lse = const_cast<float*>(lse);
    a.dout = dout; a.doutT = doutT; a.delta = delta; a.dqkv = dqkv; a.qfold = attn_qfold_hook();
    return finish(attn_bwd_launch(&a, ST(stream)), "splice_attention_bwd");
}
int splice_attention_probs(const splice_bf16* qkv, int B, int T, int Tld, int D, int H, float scale, const float* lse,
                           float* probs, splice_stream_t stream) {
    AttnArgs a = {};
    a.qkv = qkv; a.B = B; a.T = T; a.Tld = Tld; a.D = D; a.H = H; a.scale = scale; a.lse = const_cast<float*>(lse);
    return finish(attn_probs_launch(&a, probs, ST(stream)), "splice_attention_probs");
}

int splice_augment_structure(const float* img, float* out, float* scratch, int H, int W, int flip, int n_ops, const int* order,
                             const float* factors, float blur_sigma, splice_stream_t stream) {
    return finish(augment_structure_launch(img, out, scratch, H, W, flip, n_ops, order, factors, blur_sigma, ST(stream)), "splice_augment_structure");
}

size_t splice_keys_selfsim_ws_bytes(int T, int D) { return selfsim_ws_bytes(T, D); }
int splice_keys_selfsim_fwd(const float* K, int ldk, int T, int D, float eps, float* S, void* ws, splice_stream_t stream) {
    SelfSimWs w;
    selfsim_ws_carve(ws, T, D, &w);
    return finish(selfsim_fwd_launch(K, ldk, T, D, eps, S, w, ST(stream)), "splice_keys_selfsim_fwd");
}
int splice_keys_selfsim_bwd(const float* dS, const float* S, int T, int D, float eps, float* dK, int lddk, int accumulate,
                            void* ws, splice_stream_t stream) {
    SelfSimWs w;
    selfsim_ws_carve(ws, T, D, &w);
    return finish(selfsim_bwd_launch(dS, S, T, D, eps, dK, lddk, accumulate, w, ST(stream)), "splice_keys_selfsim_bwd");
}
int splice_mse(const float* a, int lda, const float* b, int ldb, int rows, int cols, float weight, float* loss_accum,
               float* grad, int ldg, splice_stream_t stream) {
    return finish(mse_launch(a, lda, b, ldb, rows, cols, weight, loss_accum, grad, ldg, ST(stream)), "splice_mse");
}

/* test hooks: the loss-stage launchers of the fused step on caller-owned buffers */
size_t splice_selfsim_loss_pairs_ws_bytes(int T, int D, int pairs) { return selfsim_batch_ws_bytes(T, D, pairs); }
int splice_selfsim_loss_pairs(const splice_bf16* k_tgt, const splice_bf16* k_x, int ldk, size_t k_pstride, const splice_bf16* kT_x, int ldt,
                              size_t kT_pstride, int T, int D, int pairs, float lambda, const float* e_scale_tab, int fp8, float eps,
                              float* loss_part, size_t part_pstride, float* dk, int lddk, size_t dk_pstride, void* ws, splice_stream_t stream) {
    const char* who = "splice_selfsim_loss_pairs";
    if (!k_tgt || !k_x || !kT_x || !loss_part || !dk || !ws || T < 1 || pairs < 1 || D < 64 || D % 64 || ldk < D || ldk % 8 || ldt % 8 ||
        k_pstride % 8 || kT_pstride % 8 || lddk < D)
        return finish(SPLICE_ERR_ARG, who);
    // the two launchers' own refusals, asked before the first of them launches (the second's would come behind the target's kernels)
    const int nt = (T + 63) / 64;
    if ((fp8 && D % 128) || (size_t)(nt * (nt + 1) / 2) > part_pstride) return finish(SPLICE_ERR_ARG, who);
    SelfSimBatch b = {};
    selfsim_batch_carve(ws, T, D, pairs, &b);
    b.ldk = ldk; b.ldt = ldt; b.k_pstride = k_pstride; b.kT_pstride = kT_pstride;
    b.k_tgt = k_tgt; b.k_x = k_x; b.kT_x = kT_x;
    b.loss_part = loss_part; b.part_pstride = part_pstride;
    b.dk = dk; b.dk_pstride = dk_pstride; b.lddk = lddk;
    b.eps = eps;
    b.fp8 = fp8 != 0;
    b.loss_scale = 1.0f / ((float)T * (float)T);   // the fp32 expressions of the step's ssim_batch
    b.e_scale = 4.0f * lambda * b.loss_scale;
    b.e_scale_tab = e_scale_tab;
    const int rc = selfsim_target_launch(b, ST(stream));
    if (rc != SPLICE_OK) return finish(rc, who);
    return finish(selfsim_loss_launch(b, ST(stream)), who);
}
int splice_mse_pairs(const float* a, int lda, size_t a_ps, const float* b, int ldb, size_t b_ps, int rows, int cols, float loss_weight,
                     float grad_weight, float* part, size_t part_ps, float* grad, int ldg, size_t g_ps, int pairs, const float* grad_tab,
                     splice_stream_t stream) {
    if (!a || !b || rows < 1 || cols < 1) return finish(SPLICE_ERR_ARG, "splice_mse_pairs");
    return finish(mse_batched_launch(a, lda, a_ps, b, ldb, b_ps, rows, cols, loss_weight, grad_weight, part, part_ps, grad, ldg, g_ps, pairs,
                                     ST(stream), grad_tab),
                  "splice_mse_pairs");
}

/* test hooks: the [CLS]-tail launchers of the top ViT block (vit_cls.hip) on caller-owned buffers.  They only validate and forward. */
static bool attn_cls_args_ok(const void* qkv, const void* qkvT, int ldt, int B, int T, int Tld, int D, int H, size_t lds) {
    if (!qkv || !qkvT || B < 1 || T < 1 || T > Tld || Tld % 32 || ldt % 8 || (long long)ldt < (long long)B * Tld || D < 64 || D % 64 || H != D / 64)
        return false;
    int dev = 0, lim = 0;   // the launchers set no function attribute: the default dynamic LDS ceiling holds, and the device's own where it is lower
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess) return false;
    return lds <= (size_t)(lim < 65536 ? lim : 65536);
}
int splice_attn_cls_fwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld, int D, int H, float scale, splice_bf16* out,
                        float* probs, splice_stream_t stream) {
    const char* who = "splice_attn_cls_fwd";
    if (!out || !probs || !attn_cls_args_ok(qkv, qkvT, ldt, B, T, Tld, D, H, ((size_t)Tld + Tld / 2 + 256 + 8) * sizeof(float)))
        return finish(SPLICE_ERR_ARG, who);
    return finish(attn_cls_fwd_launch(qkv, qkvT, ldt, B, T, Tld, D, H, scale, out, probs, ST(stream)), who);
}
int splice_attn_cls_bwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld, int D, int H, float scale, const float* probs,
                        const float* dout_slabs, int n_slabs, size_t slab_stride, splice_bf16* dqkv, splice_stream_t stream) {
    const char* who = "splice_attn_cls_bwd";
    if (!probs || !dout_slabs || !dqkv || n_slabs < 1 || n_slabs > 16 ||
        !attn_cls_args_ok(qkv, qkvT, ldt, B, T, Tld, D, H, ((size_t)Tld + Tld / 2 + 64 + 64 + 32 + 256 + 8) * sizeof(float)))
        return finish(SPLICE_ERR_ARG, who);
    return finish(attn_cls_bwd_launch(qkv, qkvT, ldt, B, T, Tld, D, H, scale, probs, dout_slabs, n_slabs, slab_stride, dqkv, ST(stream)), who);
}
int splice_ln_rows_fwd(float* x, size_t xs, const float* gamma, const float* beta, splice_bf16* y, size_t ys, float* mean, float* rstd, size_t ss,
                       int rows, int D, float eps, const float* slabs, int n_slabs, size_t slab_stride, const float* bias, const float* resid, size_t rs,
                       splice_stream_t stream) {
    const char* who = "splice_ln_rows_fwd";
    if (!x || !gamma || !beta || !y || !mean || !rstd || (slabs && (n_slabs < 1 || !bias || !resid))) return finish(SPLICE_ERR_ARG, who);
    return finish(ln_rows_fwd_launch(x, xs, gamma, beta, y, ys, mean, rstd, ss, rows, D, eps, slabs, n_slabs, slab_stride, bias, resid, rs, ST(stream)), who);
}
int splice_ln_rows_bwd(float* dy, size_t dys, const float* x, size_t xs, const float* gamma, const float* mean, const float* rstd, size_t ss, float* g,
                       splice_bf16* g_bf, int rows, int D, int n_slabs, size_t slab_stride, splice_stream_t stream) {
    const char* who = "splice_ln_rows_bwd";
    if (!dy || !x || !gamma || !mean || !rstd || !g || !g_bf) return finish(SPLICE_ERR_ARG, who);
    return finish(ln_rows_bwd_launch(dy, dys, x, xs, gamma, mean, rstd, ss, g, g_bf, rows, D, n_slabs, slab_stride, ST(stream)), who);
}
int splice_rows_finish(int mode, const float* slabs, int n_slabs, size_t slab_stride, int rows, int N, const float* bias, const float* resid, size_t rs,
                       float* out_f32, size_t os, splice_bf16* out_bf, splice_bf16* pre_bf, const splice_bf16* aux, size_t ps, int pre_lo,
                       splice_stream_t stream) {
    const char* who = "splice_rows_finish";
    if (mode < 0 || mode > 2 || !slabs || n_slabs < 1 || rows < 1 || N < 1 || (long long)rows * N > 0x7fffffffLL) return finish(SPLICE_ERR_ARG, who);
    if ((mode == 0 && (!out_f32 || !resid)) || (mode != 0 && !out_bf) || (mode == 2 && !aux)) return finish(SPLICE_ERR_ARG, who);
    return finish(rows_finish_launch(mode, slabs, n_slabs, slab_stride, rows, N, bias, resid, rs, out_f32, os, out_bf, pre_bf, aux, ps, pre_lo, ST(stream)), who);
}

int splice_patchify(const float* img, splice_bf16* patches, int B, int H, int W, int p, int Tld, int normalize,
                    splice_stream_t stream) {
    return finish(patchify_launch(img, patches, B, H, W, p, Tld, normalize, ST(stream)), "splice_patchify");
}
int splice_unpatchify(const float* dpatches, float* dimg, int B, int H, int W, int p, int Tld, int normalize,
                      splice_stream_t stream) {
    return finish(unpatchify_launch(dpatches, dimg, B, H, W, p, Tld, normalize, ST(stream)), "splice_unpatchify");
}
int splice_cast_f32_bf16(const float* x, splice_bf16* y, size_t n, splice_stream_t stream) {
    return finish(cast_f32_bf16_launch(x, y, n, ST(stream)), "splice_cast_f32_bf16");
}
int splice_cast_bf16_f32(const splice_bf16* x, float* y, size_t n, splice_stream_t stream) {
    return finish(cast_bf16_f32_launch(x, y, n, ST(stream)), "splice_cast_bf16_f32");
}
int splice_resize_bilinear_fwd(const float* in, float* out, int planes, int h, int w, int oh, int ow, splice_stream_t stream) {
    return finish(resize_bilinear_fwd_launch(in, out, planes, h, w, oh, ow, ST(stream)), "splice_resize_bilinear_fwd");
}
int splice_resize_bilinear_bwd(const float* dout, float* din, int planes, int h, int w, int oh, int ow, splice_stream_t stream) {
    return finish(resize_bilinear_bwd_launch(dout, din, planes, h, w, oh, ow, ST(stream)), "splice_resize_bilinear_bwd");
}
int splice_transpose_f32_bf16(const float* x, splice_bf16* y, int rows, int cols, int ldy, splice_stream_t stream) {
    return finish(transpose_f32_to_bf16_launch(x, y, rows, cols, ldy, ST(stream)), "splice_transpose_f32_bf16");
}
}
