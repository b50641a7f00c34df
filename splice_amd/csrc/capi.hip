// extern "C" op-level entry points of include/splice_hip.h (thin argument checks + launch).
#include <stdarg.h>
#include <stdio.h>

#include "gen_kernels.h"
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
/* the same two launchers with the layer table of the step (splice_step_set_ssim_layers): n_layers problems in the same three launches */
int splice_selfsim_loss_layers(int n_layers, const splice_bf16* const* k_tgt, const splice_bf16* const* k_x, const splice_bf16* const* kT_x,
                               const float* weights, int ldk, size_t k_pstride, int ldt, size_t kT_pstride, int T, int D, int pairs, float lambda,
                               const float* e_scale_tab, float eps, float* loss_part, size_t part_pstride, float* const* dk, int lddk,
                               size_t dk_pstride, void* const* ws, splice_stream_t stream) {
    const char* who = "splice_selfsim_loss_layers";
    if (n_layers < 1 || n_layers > SELFSIM_MAX_LAYERS || !k_tgt || !k_x || !kT_x || !weights || !loss_part || !dk || !ws || T < 1 || pairs < 1 || D < 64 ||
        D % 64 || ldk < D || ldk % 8 || ldt % 8 || k_pstride % 8 || kT_pstride % 8 || lddk < D)
        return finish(SPLICE_ERR_ARG, who);
    const int nt = (T + 63) / 64;
    if ((size_t)n_layers * (nt * (nt + 1) / 2) > part_pstride) return finish(SPLICE_ERR_ARG, who);
    SelfSimBatch b = {};
    SelfSimLayers tab = {};
    tab.n = n_layers;
    for (int i = 0; i < n_layers; ++i) {
        if (!k_tgt[i] || !k_x[i] || !kT_x[i] || !dk[i] || !ws[i] || !(weights[i] > 0.f) || !(weights[i] <= 3.402823466e+38f)) return finish(SPLICE_ERR_ARG, who);
        SelfSimBatch w = {};
        selfsim_batch_carve(ws[i], T, D, pairs, &w);
        if (i == 0) b = w;
        SelfSimLayer& e = tab.e[i];
        e.k_tgt = k_tgt[i]; e.k_x = k_x[i]; e.kT_x = kT_x[i];
        e.S_tgt = w.S_tgt; e.wmat = w.wmat; e.norm_x = w.norm_x; e.rpart = w.rpart;
        e.dk = dk[i]; e.weight = weights[i];
    }
    b.ldk = ldk; b.ldt = ldt; b.k_pstride = k_pstride; b.kT_pstride = kT_pstride;
    b.k_tgt = k_tgt[0]; b.k_x = k_x[0]; b.kT_x = kT_x[0];
    b.loss_part = loss_part; b.part_pstride = part_pstride;
    b.dk = dk[0]; b.dk_pstride = dk_pstride; b.lddk = lddk;
    b.eps = eps;
    b.loss_scale = 1.0f / ((float)T * (float)T);   // the fp32 expressions of the step's ssim_batch
    b.e_scale = 4.0f * lambda * b.loss_scale;
    b.e_scale_tab = e_scale_tab;
    const int rc = selfsim_target_launch(b, ST(stream), &tab);
    if (rc != SPLICE_OK) return finish(rc, who);
    return finish(selfsim_loss_launch(b, ST(stream), &tab), who);
}
/* the layered [CLS] launch of the step (splice_step_set_cls_layers) on caller buffers */
int splice_cls_loss_layers(int n_layers, const float* const* x, const float* const* tgt, const float* weights, size_t x_pstride, size_t t_pstride,
                           int D, int slots, float lambda, const float* grad_tab, float* part, size_t part_pstride, float* const* seeds,
                           size_t seed_pstride, float* values, splice_stream_t stream) {
    const char* who = "splice_cls_loss_layers";
    if (n_layers < 1 || n_layers > CLS_MAX_LAYERS || !x || !tgt || !weights || !seeds || !part || !values || D < 1 || slots < 1 || seed_pstride < (size_t)D)
        return finish(SPLICE_ERR_ARG, who);
    ClsLayers tab = {};
    tab.n = n_layers; tab.D = D; tab.x_ps = x_pstride; tab.t_ps = t_pstride; tab.seed_step = 1;
    for (int i = 0; i < n_layers; ++i) {
        ClsLayer& e = tab.e[i];
        e.x = x[i]; e.tgt = tgt[i]; e.seed = seeds[i]; e.seed_ps = seed_pstride; e.weight = weights[i];
    }
    return finish(cls_layers_launch(tab, slots, lambda / (float)(size_t)D, grad_tab, part, part_pstride, values, (size_t)n_layers, ST(stream)), who);
}
/* the two layered identity launches of the step (splice_step_set_id_layers) on caller buffers */
int splice_id_loss_layers(int n_layers, const float* const* x, const int* ldx, const float* const* tgt, const int* ldt, const float* weights,
                          size_t x_rstride, size_t t_rstride, int T, int D, int slots, float lambda, const float* grad_tab, float* const* grad, int ldg,
                          size_t g_rstride, float* scratch, size_t scratch_floats, float* values, float* part, size_t part_pstride, int max_wg,
                          splice_stream_t stream) {
    const char* who = "splice_id_loss_layers";
    if (n_layers < 1 || n_layers > ID_MAX_LAYERS || !x || !ldx || !tgt || !ldt || !weights || !grad || !scratch || !values || !part || T < 1 || D < 4 ||
        slots < 1 || max_wg < 0)
        return finish(SPLICE_ERR_ARG, who);
    const int G = id_layers_wg(T, D, max_wg);
    if (G < 1 || scratch_floats < (size_t)slots * n_layers * G) return finish(SPLICE_ERR_ARG, who);
    IdLayers tab = {};
    tab.n = n_layers; tab.T = T; tab.D = D; tab.x_rs = x_rstride; tab.t_rs = t_rstride; tab.g_rs = g_rstride;
    for (int i = 0; i < n_layers; ++i) {
        IdLayer& e = tab.e[i];
        e.x = x[i]; e.tgt = tgt[i]; e.grad = grad[i]; e.ldx = ldx[i]; e.ldt = ldt[i]; e.ldg = ldg; e.weight = weights[i];
    }
    const int rc = id_layers_launch(tab, slots, lambda / (float)((size_t)T * D), grad_tab, scratch, max_wg, ST(stream));
    if (rc != SPLICE_OK) return finish(rc, who);
    return finish(id_layers_finish_launch(tab, slots, grad_tab, scratch, max_wg, values, (size_t)n_layers, part, part_pstride, ST(stream)), who);
}
/* the three launches of the key second-moment term (splice_step_set_key_gram) on caller buffers, one crop per pair */
int splice_key_gram_pairs(const splice_bf16* k_x, int ldk, size_t k_ps, const splice_bf16* kT_x, int ldt_x, size_t tx_ps, const splice_bf16* kT_b,
                          int ldt_b, size_t tb_ps, int T, int D, int pairs, float scale, splice_bf16* delta, float* part, size_t part_ps, float* value,
                          float* dk, int lddk, size_t dk_ps, splice_stream_t stream) {
    const char* who = "splice_key_gram_pairs";
    KeyGram a = {};
    a.kT_x = kT_x; a.kT_b = kT_b; a.k_x = k_x; a.ldt_x = ldt_x; a.ldt_b = ldt_b; a.ldk = ldk; a.tx_ps = tx_ps; a.tb_ps = tb_ps; a.k_ps = k_ps;
    a.T = T; a.D = D; a.delta = delta; a.part = part; a.part_ps = part_ps; a.value = value; a.dk = dk; a.lddk = lddk; a.dk_ps = dk_ps; a.scale = scale;
    if (!(scale == scale) || scale - scale != 0.f) return finish(SPLICE_ERR_ARG, who);   // (finite)
    if (int rc = key_gram_check(a, pairs, 1)) return finish(rc, who);   // (nothing launched on a refusal)
    const int rc = key_gram_loss_launch(a, pairs, 1, ST(stream));
    if (rc != SPLICE_OK) return finish(rc, who);
    return finish(key_gram_dk_launch(a, pairs, 1, ST(stream)), who);
}
/* the launches of the key second-moment term over several blocks (splice_step_set_key_gram_layers) on caller buffers, one crop per pair */
int splice_key_gram_layers_pairs(int n_layers, const splice_bf16* const* k_x, const splice_bf16* const* kT_x, const splice_bf16* const* kT_b,
                                 splice_bf16* const* delta, float* const* part, float* const* dk, const float* weights, const float* scales, int ldk,
                                 size_t k_ps, int ldt_x, size_t tx_ps, int ldt_b, size_t tb_ps, int T, int D, int pairs, int centered, size_t part_ps,
                                 float* values, float* value, float* mu, int lddk, size_t dk_ps, splice_stream_t stream) {
    const char* who = "splice_key_gram_layers_pairs";
    if (n_layers < 1 || n_layers > KEY_GRAM_MAX_LAYERS || !k_x || !kT_x || !kT_b || !delta || !part || !dk || !weights || !scales) return finish(SPLICE_ERR_ARG, who);
    KeyGramLayers t = {};
    t.n = n_layers; t.centered = centered ? 1 : 0;
    t.ldt_x = ldt_x; t.ldt_b = ldt_b; t.ldk = ldk; t.tx_ps = tx_ps; t.tb_ps = tb_ps; t.k_ps = k_ps; t.T = T; t.D = D; t.part_ps = part_ps;
    t.lddk = lddk; t.dk_ps = dk_ps; t.values = values; t.value = value; t.mu = mu;
    for (int i = 0; i < n_layers; ++i) {
        KeyGramLayer& e = t.e[i];
        e.kT_x = kT_x[i]; e.kT_b = kT_b[i]; e.k_x = k_x[i]; e.dk = dk[i]; e.delta = delta[i]; e.part = part[i]; e.weight = weights[i]; e.scale = scales[i];
    }
    if (int rc = key_gram_layers_check(t, pairs, 1)) return finish(rc, who);   // (nothing launched on a refusal)
    const int rc = key_gram_layers_loss_launch(t, pairs, 1, ST(stream));
    if (rc != SPLICE_OK) return finish(rc, who);
    return finish(key_gram_layers_dk_launch(t, pairs, 1, ST(stream)), who);
}
/* the four launches of the nearest-neighbour key term (splice_step_set_key_nn) on caller buffers, one crop per pair */
size_t splice_key_nn_ws_bytes(int T, int D, int pairs) { return key_nn_ws_bytes(T, D, pairs); }
int splice_key_nn_pairs(const splice_bf16* k_x, const splice_bf16* k_b, int ldk, size_t kx_ps, size_t kb_ps, int T, int D, int pairs, float scale,
                        float eps, int* match, float* cos, float* part, size_t part_ps, float* value, float* dk, int lddk, size_t dk_ps, void* ws,
                        splice_stream_t stream) {
    const char* who = "splice_key_nn_pairs";
    KeyNn a = {};
    a.k_x = k_x; a.k_b = k_b; a.ldk = ldk; a.kx_ps = kx_ps; a.kb_ps = kb_ps; a.T = T; a.D = D; a.scale = scale; a.eps = eps;
    a.inv_t = T > 0 ? 1.0f / (float)T : 0.f;
    a.match = match; a.cos = cos; a.part = part; a.part_ps = part_ps; a.value = value; a.dk = dk; a.lddk = lddk; a.dk_ps = dk_ps; a.ws = ws;
    if (int rc = key_nn_check(a, pairs, 1)) return finish(rc, who);   // (nothing launched on a refusal)
    return finish(key_nn_launch(a, pairs, 1, ST(stream)), who);
}
int splice_mse_pairs(const float* a, int lda, size_t a_ps, const float* b, int ldb, size_t b_ps, int rows, int cols, float loss_weight,
                     float grad_weight, float* part, size_t part_ps, float* grad, int ldg, size_t g_ps, int pairs, const float* grad_tab,
                     splice_stream_t stream) {
    if (!a || !b || rows < 1 || cols < 1) return finish(SPLICE_ERR_ARG, "splice_mse_pairs");
    return finish(mse_batched_launch(a, lda, a_ps, b, ldb, b_ps, rows, cols, loss_weight, grad_weight, part, part_ps, grad, ldg, g_ps, pairs,
                                     ST(stream), grad_tab),
                  "splice_mse_pairs");
}

/* test hooks: the image-space terms' launchers (image_terms.hip) on caller-owned buffers, in the step's partials layout */
static_assert(SPLICE_IMAGE_TERMS_CHUNK == IMAGE_TERMS_CHUNK, "the header states the value kernel's chunk");
int splice_image_terms_value(const float* x, int n_x, int xh, int xw, const float* y, const float* b, int n_y, int yh, int yw, float* lbase,
                             size_t lstride, int lp, splice_stream_t stream) {
    const char* who = "splice_image_terms_value";
    if (!lbase || lp < 1 || lstride < 8 + (size_t)8 * lp || (!x && !y) || (y && !b)) return finish(SPLICE_ERR_ARG, who);
    const int rc = image_terms_value_launch(x, n_x, xh, xw, lbase + 8 + (size_t)6 * lp, y, b, n_y, yh, yw, lbase + 8 + (size_t)7 * lp, lstride, (size_t)lp,
                                            ST(stream));
    if (rc != SPLICE_OK) return rc;   // (the launcher's own message stays)
    return finish(rc, who);
}
int splice_image_terms_grad_add(const float* x, const float* b, float* d, int n_img, int h, int w, float lambda, splice_stream_t stream) {
    if (!(lambda <= 3.402823466e+38f)) return finish(SPLICE_ERR_ARG, "splice_image_terms_grad_add");
    const int rc = b ? image_pix_grad_add_launch(x, b, d, n_img, h, w, lambda, ST(stream)) : image_tv_grad_add_launch(x, d, n_img, h, w, lambda, ST(stream));
    if (rc != SPLICE_OK) return rc;
    return finish(rc, "splice_image_terms_grad_add");
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

/* test hooks: generator launchers on caller-owned buffers.  They only validate and forward: no launcher, policy or kernel is theirs. */
static bool gen_conv_args_ok(const splice_gen_conv_args* g, bool reflect_dgrad) {
    if (!g || !g->in || !g->w || !g->out) return false;
    if (g->N < 1 || g->Cin < 1 || g->Hi < 1 || g->Wi < 1 || g->Cout < 1 || g->Ho < 1 || g->Wo < 1 || g->pad < 0) return false;
    if (g->ks != 1 && g->ks != 3 && g->ks != 5 && g->ks != 7) return false;
    if (g->stride != 1 && g->stride != 2) return false;
    if ((g->act != 0 && g->act != 1) || (g->reflect && g->transposed && !reflect_dgrad)) return false;
    const long long HWi = (long long)g->Hi * g->Wi, HWo = (long long)g->Ho * g->Wo;
    if (HWi > 0x1fffffffLL || HWo > 0x1fffffffLL) return false;
    if (g->in_cstride < (size_t)HWi || g->out_cstride < (size_t)HWo) return false;
    if (g->N > 1 && (g->in_nstride < (size_t)g->Cin * g->in_cstride || g->out_nstride < (size_t)g->Cout * g->out_cstride)) return false;
    // the 32-bit offsets of the gathers (bytes, bit 31 reserved as the out-of-range mark): reduction channels x channel stride, the weight block
    if ((size_t)g->Cin * g->in_cstride > 0x1fffffffULL) return false;
    if ((size_t)g->Cout * g->w_jstride + (size_t)g->Cin * g->w_cstride + (size_t)g->ks * g->ks > 0x1fffffffULL) return false;
    if ((size_t)g->Cout * g->out_cstride > 0x7fffffffULL) return false;
    if (g->w_jstride < 1 || g->w_cstride < 1) return false;
    if (g->p_group < 0 || (g->p_group > 1 && (!g->p_nstride || g->N % g->p_group))) return false;
    if (g->reflect && !reflect_dgrad && (g->pad >= g->Hi || g->pad >= g->Wi)) return false;   // a mirror needs pad < size
    if (reflect_dgrad && (g->pad >= g->Ho || g->pad >= g->Wo || g->act)) return false;
    if (g->ws && g->ws_floats < 1) return false;
    if (g->defer_reduce && !g->ws) return false;
    return true;
}
static ConvArgs gen_conv_fill(const splice_gen_conv_args* g) {
    ConvArgs a = {};
    a.in = g->in; a.w = g->w; a.bias = g->bias; a.out = g->out;
    a.in_nstride = g->in_nstride; a.in_cstride = g->in_cstride; a.out_nstride = g->out_nstride; a.out_cstride = g->out_cstride;
    a.w_jstride = g->w_jstride; a.w_cstride = g->w_cstride; a.p_nstride = g->p_nstride;
    a.N = g->N; a.Cin = g->Cin; a.Hi = g->Hi; a.Wi = g->Wi; a.Cout = g->Cout; a.Ho = g->Ho; a.Wo = g->Wo;
    a.ks = g->ks; a.stride = g->stride; a.pad = g->pad;
    a.reflect = g->reflect; a.act = g->act; a.transposed = g->transposed; a.accumulate = g->accumulate;
    a.ws = g->ws; a.ws_floats = g->ws_floats; a.p_group = g->p_group; a.defer_reduce = g->defer_reduce;
    return a;
}
int splice_gen_conv(const splice_gen_conv_args* args, int* form_out, splice_stream_t stream) {
    const char* who = "splice_gen_conv";
    if (!gen_conv_args_ok(args, false)) return finish(SPLICE_ERR_ARG, who);
    const ConvArgs a = gen_conv_fill(args);
    if (form_out) conv_form_report(a, form_out);
    return finish(conv_launch(a, ST(stream)), who);
}
int splice_gen_conv_pair(const splice_gen_conv_args* a_args, const splice_gen_conv_args* b_args, int* forms_out, splice_stream_t stream) {
    const char* who = "splice_gen_conv_pair";
    if (!gen_conv_args_ok(a_args, false) || !gen_conv_args_ok(b_args, false)) return finish(SPLICE_ERR_ARG, who);
    const ConvArgs a = gen_conv_fill(a_args), b = gen_conv_fill(b_args);
    if (forms_out) { conv_form_report(a, forms_out); conv_form_report(b, forms_out + SPLICE_GEN_CONV_FORM_INTS); }
    return finish(conv_pair_launch(a, b, ST(stream)), who);
}
int splice_gen_conv_reflect_dgrad(const splice_gen_conv_args* args, float* pad_scratch, size_t scratch_floats, splice_stream_t stream) {
    const char* who = "splice_gen_conv_reflect_dgrad";
    if (!gen_conv_args_ok(args, true) || !pad_scratch) return finish(SPLICE_ERR_ARG, who);
    const size_t Hp = (size_t)args->Ho + 2 * args->pad, Wp = (size_t)args->Wo + 2 * args->pad;
    if (scratch_floats < (size_t)args->N * args->Cout * Hp * Wp || (size_t)args->Cout * Hp * Wp > 0x7fffffffULL) return finish(SPLICE_ERR_ARG, who);
    return finish(conv_reflect_dgrad_launch(gen_conv_fill(args), pad_scratch, ST(stream)), who);
}

static bool gen_wgrad_args_ok(const splice_gen_wgrad_args* g) {
    if (!g || !g->x || !g->dy) return false;
    if (g->N < 1 || g->Cin < 1 || g->Hi < 1 || g->Wi < 1 || g->Cout < 1 || g->Ho < 1 || g->Wo < 1 || g->pad < 0 || g->pad > 255) return false;
    if (g->ks != 1 && g->ks != 3 && g->ks != 5 && g->ks != 7) return false;
    if ((g->stride != 1 && g->stride != 2) || g->Cout > 128) return false;
    if (g->Hi > 65535 || g->Wi > 65535 || g->Ho > 65535 || g->Wo > 65535 || g->Cin > 65535) return false;
    const long long HWi = (long long)g->Hi * g->Wi, HWo = (long long)g->Ho * g->Wo;
    if (HWo > (1LL << 22)) return false;   // pix_per_chunk is a 16-bit field of the descriptor (128 chunks per image): planes far below 128 x 65535 pixels
    if (g->x_cstride < (size_t)HWi || g->dy_cstride < (size_t)HWo) return false;
    if (g->N > 1 && (g->x_nstride < (size_t)g->Cin * g->x_cstride || g->dy_nstride < (size_t)g->Cout * g->dy_cstride)) return false;
    if ((size_t)g->Cin * g->x_cstride > 0x1fffffffULL || (size_t)g->Cout * g->dy_cstride > 0x1fffffffULL) return false;   // 32-bit byte offsets
    if (g->x_nstride > 0xffffffffULL || g->dy_nstride > 0xffffffffULL) return false;
    if (g->reflect && (g->pad >= g->Hi || g->pad >= g->Wi)) return false;
    return true;
}
size_t splice_gen_conv_wgrad_ws_floats(int N, int Cin, int Cout, int ks, int Ho, int Wo) {
    if (N < 1 || Cin < 1 || Cout < 1 || ks < 1 || Ho < 1 || Wo < 1) return 0;
    int ppc = 0, cpi = 0;
    return (size_t)wgrad_chunks(N, Ho, Wo, &ppc, &cpi) * Cout * Cin * ks * ks;
}
int splice_gen_conv_wgrad(const splice_gen_wgrad_args* args, float* dw, int accumulate, int n_img, size_t p_nstride, int* form_out, splice_stream_t stream) {
    const char* who = "splice_gen_conv_wgrad";
    if (!gen_wgrad_args_ok(args) || !dw || !args->ws) return finish(SPLICE_ERR_ARG, who);
    const size_t n = (size_t)args->Cout * args->Cin * args->ks * args->ks;
    if (n > 0x7fffffffULL || args->ws_floats < splice_gen_conv_wgrad_ws_floats(args->N, args->Cin, args->Cout, args->ks, args->Ho, args->Wo))
        return finish(SPLICE_ERR_ARG, who);
    // independent images (p_nstride > 0): image i's chunks are summed into dw + i * p_nstride; else one sum over every image
    if (p_nstride ? (n_img != args->N || p_nstride < n) : n_img != 1) return finish(SPLICE_ERR_ARG, who);
    WgradArgs a = {};
    a.x = args->x; a.dy = args->dy; a.ws = args->ws;
    a.x_nstride = args->x_nstride; a.x_cstride = args->x_cstride; a.dy_nstride = args->dy_nstride; a.dy_cstride = args->dy_cstride;
    a.N = args->N; a.Cin = args->Cin; a.Hi = args->Hi; a.Wi = args->Wi; a.Cout = args->Cout; a.Ho = args->Ho; a.Wo = args->Wo;
    a.ks = args->ks; a.stride = args->stride; a.pad = args->pad; a.reflect = args->reflect;
    WgradBatchPair pair = {};
    int chunks = 0;
    int rc = conv_wgrad_add(&pair, a, &chunks);
    if (rc != SPLICE_OK) return finish(rc, who);
    WgradReduceAll r = {};
    r.count = 1; r.n[0] = (int)n; r.chunks[0] = chunks; r.ws_off[0] = 0; r.dw_off[0] = 0;
    if (form_out) {   // class and variant as the queue holds them; the reduce's 16-byte form by the launcher's own rule (SPLICE_WGRAD_REDUCE_VEC unset)
        const WgradBatch& b = pair.tile.count ? pair.tile : pair.big.count ? pair.big : pair.small;
        form_out[0] = pair.tile.count ? 2 : pair.big.count ? 1 : 0;
        form_out[1] = b.d[0].variant;
        form_out[2] = b.d[0].pix_per_chunk;
        form_out[3] = chunks;
        form_out[4] = !((reinterpret_cast<size_t>(args->ws) | reinterpret_cast<size_t>(dw)) & 15) && p_nstride % 4 == 0 && n % 4 == 0;
        form_out[5] = b.total_wgs;
    }
    rc = conv_wgrad_batched_launch(pair, ST(stream));
    if (rc != SPLICE_OK) return finish(rc, who);
    return finish(wgrad_reduce_all_launch(r, args->ws, dw, accumulate, ST(stream), n_img, p_nstride), who);
}

int splice_gen_wgrad_reduce(const float* partials, int n, int chunks, float* dw, int accumulate, int n_img, size_t p_nstride, splice_stream_t stream) {
    const char* who = "splice_gen_wgrad_reduce";
    if (!partials || !dw || n < 1 || chunks < 0 || n_img < 1 || n_img > 65535 || (long long)n * (chunks > 0 ? chunks : 1) > 0x7fffffffLL) return finish(SPLICE_ERR_ARG, who);
    if (p_nstride ? (chunks % n_img || p_nstride < (size_t)n) : n_img != 1) return finish(SPLICE_ERR_ARG, who);
    WgradReduceAll r = {};
    r.count = 1; r.n[0] = n; r.chunks[0] = chunks; r.ws_off[0] = 0; r.dw_off[0] = 0;
    return finish(wgrad_reduce_all_launch(r, partials, dw, accumulate, ST(stream), n_img, p_nstride), who);
}

int splice_gen_bn_small_instance(int mask) { return finish(bn_small_force_instance(mask), "splice_gen_bn_small_instance"); }
int splice_gen_bn_form(int HW, int N, size_t p_nstride, int batch, int* out) {
    if (HW < 1 || N < 1 || batch < 0 || !out) return finish(SPLICE_ERR_ARG, "splice_gen_bn_form");
    const BnForm f = bn_form(HW, N, p_nstride, batch);
    out[0] = (int)f.kind; out[1] = f.hosts_pre; out[2] = f.fwd_takes_slabs; out[3] = f.bwd_takes_slabs;
    out[4] = f.fwd_fuses_upsample; out[5] = f.bwd_fuses_upsample; out[6] = f.sign_from_y;
    return SPLICE_OK;
}
size_t splice_gen_bn_part_floats(int N, int C) { return N < 1 || C < 1 ? 0 : (size_t)bn_part_floats(N, C); }
// what both directions need; fills the launcher's structs (up / pre / slabs point into the caller's frame)
static bool gen_bn_fill(const splice_gen_bn_args* g, bool bwd, BnArgs* a, BnUpsample* up, BnPre* pre, BnSlabs* sl) {
    if (!g || !g->y || !g->out || !g->gamma || !g->mean || !g->rstd) return false;
    if (g->N < 1 || g->C < 1 || g->HW < 1 || g->N > 65535 || g->C > 65535 || g->batch < 0 || g->batch > 8) return false;
    if (g->batch && (g->N % g->batch || (g->N != g->batch && !g->p_nstride))) return false;
    if (g->N > 1 && (g->y_nstride < (size_t)g->C * g->HW || g->out_nstride < (size_t)g->C * g->HW)) return false;
    const BnForm f = bn_form(g->HW, g->N, g->p_nstride, g->batch);
    const bool two_stage = f.kind == BnForm::TWO_STAGE || f.kind == BnForm::TWO_STAGE_VEC;
    if (two_stage && (!g->part || g->part_floats < (size_t)bn_part_floats(g->N, g->C))) return false;
    if (!bwd && !g->beta) return false;
    if (bwd && ((f.sign_from_y && !g->beta) || !g->da || !g->dy || !g->dgamma || !g->dbeta)) return false;
    if (bwd && g->N > 1 && (g->da_nstride < (size_t)g->C * g->HW || g->dy_nstride < (size_t)g->C * g->HW)) return false;
    a->y = g->y; a->y_nstride = g->y_nstride; a->out = g->out; a->out_nstride = g->out_nstride;
    a->N = g->N; a->C = g->C; a->HW = g->HW; a->gamma = g->gamma; a->beta = g->beta; a->eps = g->eps; a->slope = g->slope;
    a->p_nstride = g->p_nstride; a->batch = g->batch; a->part = g->part; a->mean = g->mean; a->rstd = g->rstd;
    if (g->up_src || g->up_d_src) {
        if (bwd ? !g->up_d_src : !g->up_src) return false;
        if (g->up_c0 < 0 || g->up_c0 >= g->C || g->up_h < 1 || g->up_w < 1 || g->up_Ho < 1 || g->up_Wo < 1) return false;
        if (g->up_Ho > 2 * g->up_h || g->up_Wo > 2 * g->up_w || (long long)g->up_Ho * g->up_Wo != g->HW) return false;
        const size_t src = (size_t)(g->C - g->up_c0) * g->up_h * g->up_w;
        if (g->N > 1 && (bwd ? g->up_d_src_ns : g->up_src_ns) < src) return false;
        up->src = g->up_src; up->src_ns = g->up_src_ns; up->d_src = g->up_d_src; up->d_src_ns = g->up_d_src_ns;
        up->c0 = g->up_c0; up->h = g->up_h; up->w = g->up_w; up->Ho = g->up_Ho; up->Wo = g->up_Wo;
        a->up = up;
    }
    if (g->pre_y) {
        if (!g->pre_gamma || !g->pre_beta || !g->pre_mean || !g->pre_rstd || g->pre_C < 1 || g->pre_C > (a->up ? g->up_c0 : g->C)) return false;
        if (g->N > 1 && g->pre_y_ns < (size_t)g->pre_C * g->HW) return false;
        if (g->pre_slabs && (bwd || !f.fwd_takes_slabs || g->pre_ksplit < 1 || g->pre_ksplit > 16)) return false;   // only the small-plane kernel forms the skip plane from slabs
        if (bwd && (!g->pre_dy || !g->pre_dgamma || !g->pre_dbeta)) return false;
        pre->y = g->pre_y; pre->y_ns = g->pre_y_ns; pre->slabs = g->pre_slabs; pre->ksplit = g->pre_ksplit; pre->bias = g->pre_bias;
        pre->gamma = g->pre_gamma; pre->beta = g->pre_beta; pre->mean = g->pre_mean; pre->rstd = g->pre_rstd; pre->slope = g->pre_slope; pre->C = g->pre_C;
        pre->dy = g->pre_dy; pre->dgamma = g->pre_dgamma; pre->dbeta = g->pre_dbeta;
        a->pre = pre;
    }
    if (!bwd && g->slabs) {
        if (g->ksplit < 2 || g->ksplit > 16) return false;
        a->slabs = g->slabs; a->ksplit = g->ksplit; a->bias = g->bias;
    }
    if (bwd) {
        a->da = g->da; a->da_nstride = g->da_nstride; a->dy = g->dy; a->dy_nstride = g->dy_nstride;
        a->dgamma = g->dgamma; a->dbeta = g->dbeta; a->accumulate = g->accumulate;
        if (g->da_slabs) {
            if (g->da_ksplit < 1 || g->da_ksplit > 16) return false;
            sl->slabs = g->da_slabs; sl->ksplit = g->da_ksplit; sl->accumulate = g->da_accumulate;
            a->da_slabs = sl;
        }
    }
    return true;
}
int splice_gen_bn_fwd(const splice_gen_bn_args* args, splice_stream_t stream) {
    BnArgs a; BnUpsample up; BnPre pre; BnSlabs sl;
    if (!gen_bn_fill(args, false, &a, &up, &pre, &sl)) return finish(SPLICE_ERR_ARG, "splice_gen_bn_fwd");
    return finish(bn_fwd_launch(a, ST(stream)), "splice_gen_bn_fwd");
}
int splice_gen_bn_bwd(const splice_gen_bn_args* args, splice_stream_t stream) {
    BnArgs a; BnUpsample up; BnPre pre; BnSlabs sl;
    if (!gen_bn_fill(args, true, &a, &up, &pre, &sl)) return finish(SPLICE_ERR_ARG, "splice_gen_bn_bwd");
    return finish(bn_bwd_launch(a, ST(stream)), "splice_gen_bn_bwd");
}

static bool gen_up_args_ok(const void* a, const void* b, size_t in_ns, size_t out_ns, int N, int C, int h, int w, int Ho, int Wo) {
    if (!a || !b || N < 1 || C < 1 || h < 1 || w < 1 || Ho < 1 || Wo < 1 || N > 65535 || C > 65535) return false;
    if (Ho > 2 * h || Wo > 2 * w || (long long)h * w > 0x7fffffffLL / 4 || (long long)Ho * Wo > 0x7fffffffLL) return false;
    return N == 1 || (in_ns >= (size_t)C * h * w && out_ns >= (size_t)C * Ho * Wo);
}
int splice_gen_upsample2x_fwd(const float* in, size_t in_nstride, float* out, size_t out_nstride, int N, int C, int h, int w, int Ho, int Wo,
                              splice_stream_t stream) {
    if (!gen_up_args_ok(in, out, in_nstride, out_nstride, N, C, h, w, Ho, Wo)) return finish(SPLICE_ERR_ARG, "splice_gen_upsample2x_fwd");
    return finish(upsample2x_fwd_launch(in, in_nstride, out, out_nstride, N, C, h, w, Ho, Wo, ST(stream)), "splice_gen_upsample2x_fwd");
}
int splice_gen_upsample2x_bwd(const float* dout, size_t dout_nstride, float* din, size_t din_nstride, int N, int C, int h, int w, int Ho, int Wo,
                              splice_stream_t stream) {
    if (!gen_up_args_ok(din, dout, din_nstride, dout_nstride, N, C, h, w, Ho, Wo)) return finish(SPLICE_ERR_ARG, "splice_gen_upsample2x_bwd");
    return finish(upsample2x_bwd_launch(dout, dout_nstride, din, din_nstride, N, C, h, w, Ho, Wo, ST(stream)), "splice_gen_upsample2x_bwd");
}
size_t splice_gen_sigmoid_bias_part_floats(int N, int C) { return N < 1 || C < 1 ? 0 : (size_t)sigmoid_bias_part_floats(N, C); }
int splice_gen_sigmoid_bwd_bias(const float* dout, const float* sout, float* dpre, int N, int C, int HW, float* part, size_t part_floats, size_t p_nstride,
                                int group, int* chunks_out, splice_stream_t stream) {
    const char* who = "splice_gen_sigmoid_bwd_bias";
    if (!dout || !sout || !dpre || !part || N < 1 || C < 1 || HW < 1 || N > 65535 || C > 65535 || group < 1) return finish(SPLICE_ERR_ARG, who);
    if (part_floats < splice_gen_sigmoid_bias_part_floats(N, C) || (group > 1 && !p_nstride) || N % group) return finish(SPLICE_ERR_ARG, who);
    return finish(sigmoid_bwd_bias_launch(dout, sout, dpre, N, C, HW, part, ST(stream), p_nstride, chunks_out, group), who);
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
