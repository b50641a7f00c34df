// Internal launcher declarations (one per hand-written gfx950 kernel family).
// The public C ABI is include/splice_hip.h, implemented in capi.hip / engine.hip.
#pragma once
#include "common.h"
#include "gemm.h"

// ---- attention.hip -------------------------------------------------------------------
struct AttnArgs {
    const bf16_t* qkv;     // [B*Tld][3D]
    const bf16_t* qkvT;    // [3D][ldt]
    int ldt;
    int B, T, Tld, D, H;
    float scale;
    bf16_t* out;           // [B*Tld][D]
    float* lse;            // [B][H][Tld]
    // backward only
    const bf16_t* dout;    // [B*Tld][D]
    const bf16_t* doutT;   // [D][ldt]
    float* delta;          // [B][H][Tld]  rowsum(dO * O)
    int delta_ready;       // != 0: the caller already filled delta (the ViT engine: proj-dgrad GEMM epilogue)
    bf16_t* dqkv;          // [B*Tld][3D]
    // e4m3 forward (BASELINE configs[4]; null = bf16 forward): the same qkv as unscaled e4m3 bytes, row-major and transposed
    const uint8_t* qkv8;   // [B*Tld][3D]
    const uint8_t* qkvT8;  // [3D][ldt8]
    int ldt8;
    int qfold;             // != 0: the q columns of qkv hold q * scale * log2(e) (the ViT engine's packing of the QKV projection); scores are exponents as they leave the MFMA
};
int attn_fwd_launch(const AttnArgs* a, hipStream_t s);
int attn_bwd_launch(const AttnArgs* a, hipStream_t s);
int attn_probs_launch(const AttnArgs* a, float* probs, hipStream_t s);
void attn_set_variant(int v);   // benchmarking hook
void attn_set_bwd_variant(int v);
int attn_qfold_hook();
void attn_set_qfold(int on);    // benchmarking hook: the stand-alone entry points take pre-scaled q

// ---- vit_cls.hip: the tail of the top block on the [CLS] rows only ---------------------------
int attn_cls_fwd_launch(const bf16_t* qkv, const bf16_t* qkvT, int ldt, int B, int T, int Tld, int D, int H, float scale, bf16_t* out, float* probs,
                        hipStream_t s);
int attn_cls_bwd_launch(const bf16_t* qkv, const bf16_t* qkvT, int ldt, int B, int T, int Tld, int D, int H, float scale, const float* probs,
                        const float* dout_slabs, int n_slabs, size_t slab_stride, bf16_t* dqkv, hipStream_t s);
int ln_rows_fwd_launch(float* x, size_t xs, const float* gamma, const float* beta, bf16_t* y, size_t ys, float* mean, float* rstd, size_t ss, int rows,
                       int D, float eps, const float* slabs, int n_slabs, size_t slab_stride, const float* bias, const float* resid, size_t rs, hipStream_t s);
int ln_rows_bwd_launch(float* dy, size_t dys, const float* x, size_t xs, const float* gamma, const float* mean, const float* rstd, size_t ss, float* g,
                       bf16_t* g_bf, int rows, int D, int n_slabs, size_t slab_stride, hipStream_t s);
int rows_finish_launch(int mode, const float* slabs, int n_slabs, size_t slab_stride, int rows, int N, const float* bias, const float* resid, size_t rs,
                       float* out_f32, size_t os, bf16_t* out_bf, bf16_t* pre_bf, const bf16_t* aux, size_t ps, int pre_lo, hipStream_t s);

// ---- gemm.hip --------------------------------------------------------------------------
// Runtime dispatch over the instantiated (tile, epilogue-flag) combinations.
int gemm_nt_launch(unsigned flags, const bf16_t* A, int lda, const bf16_t* B, int ldb, int M, int N, int K,
                   const GemmEpi& e, hipStream_t s);

void gemm_force_tile(int t);   // benchmarking hook: 0 auto, 1 128x128, 2 128x64, 3 64x64
// e4m3 operands (bytes; lda / ldb / K in elements = bytes): flags must include EPI_SCALE_RC
int gemm_nt_fp8_launch(unsigned flags, const uint8_t* A, int lda, const uint8_t* B, int ldb, int M, int N, int K, const GemmEpi& e, hipStream_t s);

// ---- vit_ops.hip -----------------------------------------------------------------------
// LayerNorm over the last dim (D % 256 == 0 handled generally), one wave per row.
int layernorm_fwd_launch(const float* x, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                         int rows, int D, float eps, hipStream_t s);
// fp8 (e4m3) operand path: LayerNorm output quantised per token (y bytes [rows][D], yscale[rows]: y_true ~= y * yscale[row])
int layernorm_fwd_fp8_launch(const float* x, const float* gamma, const float* beta, uint8_t* y, float* yscale, float* mean, float* rstd,
                             int rows, int D, float eps, hipStream_t s);
int quantize_rows_fp8_launch(const float* x, int ldx, uint8_t* q, int ldq, float* scale, int rows, int cols, hipStream_t s);
int quantize_rows_bf16_fp8_launch(const bf16_t* x, int ldx, uint8_t* q, int ldq, float* scale, int rows, int cols, hipStream_t s);
int quantize_keys_fp8_launch(const bf16_t* k, int ldk, size_t k_pstride, uint8_t* q, int ldq, size_t q_pstride, float* qnorm, int T, int Tp, int D,
                             int pairs, hipStream_t s);
// g_out = g_in + LN_backward(dy); also emits bf16(g_out).  dy is fp32 [rows][D].
int layernorm_bwd_launch(const float* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                         const float* g_in, float* g_out, bf16_t* g_out_bf, int rows, int D, hipStream_t s);
// same with dy given as n_slabs split-K slabs (dy + s * slab_stride), summed in order
int layernorm_bwd_slabs_launch(const float* dy, int n_slabs, size_t slab_stride, const float* x, const float* gamma, const float* mean,
                               const float* rstd, const float* g_in, float* g_out, bf16_t* g_out_bf, int rows, int D, hipStream_t s);
// image [B][3][H][W] fp32 -> patch matrix bf16 [B*Tld][3*p*p] (row b*Tld+1+patch; row 0 and
// rows >= T are zero), k index = c*p*p + py*p + px (Conv2d weight order).  Optional
// ImageNet normalisation (x-mean)/std fused in.
int patchify_launch(const float* img, bf16_t* patches, int B, int H, int W, int p, int Tld, int normalize, hipStream_t s);
// d(patch matrix) fp32 [B*Tld][3*p*p] -> d(image) [B][3][H][W] (divides by std when normalize).
int unpatchify_launch(const float* dpatches, float* dimg, int B, int H, int W, int p, int Tld, int normalize, hipStream_t s);
int cast_f32_bf16_launch(const float* x, bf16_t* y, size_t n, hipStream_t s);
int cast_bf16_f32_launch(const bf16_t* x, float* y, size_t n, hipStream_t s);
int transpose_f32_to_bf16_launch(const float* x, bf16_t* y, int rows, int cols, int ldy, hipStream_t s);  // y[c][r]
int fill_f32_launch(float* x, float v, size_t n, hipStream_t s);
// kernel-based copy / zero (graph-capture safe replacements of hipMemcpyAsync / hipMemsetAsync, bytes % 4 == 0)
int dev_copy_launch(void* dst, const void* src, size_t bytes, hipStream_t s);
int dev_zero_launch(void* dst, size_t bytes, hipStream_t s);
// torchvision-0.10 tensor Resize = F.interpolate(bilinear, align_corners=False, no antialias) on [N][C][h][w]
// (util/losses.py:20,77-78); backward is the exact adjoint in gather form (deterministic).
int resize_bilinear_fwd_launch(const float* in, float* out, int planes, int h, int w, int oh, int ow, hipStream_t s);
int resize_bilinear_bwd_launch(const float* dout, float* din, int planes, int h, int w, int oh, int ow, hipStream_t s);
int add_f32_launch(float* y, const float* x, size_t n, hipStream_t s);  // y += x

// ---- augment.hip ----------------------------------------------------------------------
int augment_structure_launch(const float* img, float* out, float* scratch, int H, int W, int flip, int n_ops, const int* order,
                             const float* factors, float blur_sigma, hipStream_t s);

// ---- selfsim.hip -----------------------------------------------------------------------
// Cosine self-similarity of the rows of K (fp32 [T][ldk], D columns), models/extractor.py:4-9.
struct SelfSimWs {          // carved from caller-provided scratch (selfsim_ws_bytes)
    bf16_t* kbf;            // [Tp][D]   bf16 keys (rows >= T zero), Tp = roundup(T, 64)
    bf16_t* kbfT;           // [D][Tp]
    float* norm;            // [Tp]      L2 norms of the bf16-rounded rows
    bf16_t* wmat;           // [Tp][Tp]  backward weights  (dS + dS^T) / max(n_i n_j, eps)
    float* rowdot;          // [Tp]      sum_j (dS+dS^T)_ij S_ij / n_i^2
    int Tp;
};
size_t selfsim_ws_bytes(int T, int D);
void selfsim_ws_carve(void* base, int T, int D, SelfSimWs* ws);
// S = cos-sim(K) -> fp32 [T][T]; fills ws.kbf / kbfT / norm (needed by the backward).
int selfsim_fwd_launch(const float* K, int ldk, int T, int D, float eps, float* S, const SelfSimWs& ws, hipStream_t s);
// dK fp32 [T][lddk] (+= if accumulate) from dS fp32 [T][T] (any, not nec. symmetric); needs the
// ws state left by selfsim_fwd_launch on the same K, and S.
int selfsim_bwd_launch(const float* dS, const float* S, int T, int D, float eps, float* dK, int lddk, int accumulate,
                       const SelfSimWs& ws, hipStream_t s);
// ---- fused + batched structure loss of the optimisation step (blockIdx.y = pair); see selfsim.hip
struct SelfSimBatch {
    int T, Tp, D, pairs;
    int ldk, ldt;                   // leading dimensions of the key matrices below
    size_t k_pstride, kT_pstride;   // element strides between the pairs' problems
    const bf16_t* k_tgt;            // target keys (A' passes)     bf16 [T][ldk], pair p at + p * k_pstride
    const bf16_t* k_x;              // generated keys (x' passes)
    const bf16_t* kT_x;             // transposed generated keys   bf16 [D][ldt], pair p at + p * kT_pstride
    float* S_tgt;                   // [pairs][T][T] fp32 (upper-triangular 64x64 tiles valid)
    bf16_t* wmat;                   // [pairs][Tp][Tp]
    float *norm_tgt, *norm_x;       // [pairs][Tp]
    float* rpart;                   // [pairs][Tp/64][Tp] per-tile partial row dots
    float* loss_part;               // pair p's per-tile loss partials at + p * part_pstride (>= nt(nt+1)/2 floats, summed by the caller)
    size_t part_pstride;
    float* dk;                      // d keys fp32: pair p at + p * dk_pstride, [T][lddk]
    size_t dk_pstride; int lddk;
    float eps, e_scale, loss_scale; // e_scale = 4 lambda / T^2 ; loss_scale = 1 / T^2
    const float* e_scale_tab;       // optional [pairs] per-pair e_scale (replaces e_scale); a pair whose entry is 0 writes nothing
    int fp8;                        // != 0: the two Gram matrices run on the fp8 MFMA from per-row quantised keys (D % 128 == 0)
    uint8_t *k8_tgt, *k8_x;         // [pairs][Tp][D] e4m3 rows (workspace)
    float *qnorm_tgt, *qnorm_x;     // [pairs][Tp] norms of the quantised rows
};
// The structure term over the keys of several ViT blocks: a by-value table, one entry per layer, of what differs
// between the layers' problems -- the layer is one more grid dimension of the same three launches.  Entry i's tile partials go to slots
// [i tiles, (i + 1) tiles) of b.loss_part's row (tiles = nt (nt + 1) / 2); its weight multiplies loss_scale and e_scale.  bf16 only.
#define SELFSIM_MAX_LAYERS 12
struct SelfSimLayer {
    const bf16_t *k_tgt, *k_x, *kT_x;   // as in SelfSimBatch, of this layer's qkv buffers
    float* S_tgt; bf16_t* wmat;         // the layer's own workspace (a selfsim_batch_carve of its own)
    float *norm_x, *rpart;
    float* dk;
    float weight;
};
struct SelfSimLayers { int n; SelfSimLayer e[SELFSIM_MAX_LAYERS]; };
size_t selfsim_batch_ws_bytes(int T, int D, int pairs);
void selfsim_batch_carve(void* base, int T, int D, int pairs, SelfSimBatch* b);   // fills T, Tp, D, pairs and the workspace pointers
// layers (optional): every entry of the table in the same launches (grid z); b's own operand pointers are then not read
int selfsim_target_launch(const SelfSimBatch& b, hipStream_t s, const SelfSimLayers* layers = nullptr);   // S* with the row norms taken inside the Gram kernel (1 launch; 2 on the fp8 path)
int selfsim_loss_launch(const SelfSimBatch& b, hipStream_t s, const SelfSimLayers* layers = nullptr);     // fused S / loss / W (norms in-kernel) + dK (2 launches; 3 on the fp8 path)
// grad_tab (optional, [pairs]): per-pair gradient weight, the value grad_weight / (rows * cols) takes otherwise; a pair whose entry
// is 0 writes no partials and no gradient
int mse_batched_launch(const float* a, int lda, size_t a_ps, const float* b, int ldb, size_t b_ps, int rows, int cols, float loss_weight,
                       float grad_weight, float* part, size_t part_ps, float* grad, int ldg, size_t g_ps, int pairs, hipStream_t s,
                       const float* grad_tab = nullptr);
// ---- cls_layers.hip: the [CLS] appearance term over several ViT blocks ----
// A by-value table, one entry per layer in ascending block order, of what differs between the layers' problems, and the strides they
// share.  Slot s (a pair, or a pair-crop) compares row x + s * x_ps with row tgt + s * t_ps (D floats each), writes entry i's addend
// S_i * (weight_i / D) to values[s * values_ps + i], the seed row 2 * (g * weight_i) * d to seed + s * seed_step * seed_ps, and the
// ascending fp32 sum of the addends to part[s * part_ps] -- slot 0 of the slot's term row, whose other slots the step's zeroing left at 0.
#define CLS_MAX_LAYERS 12
struct ClsLayer {
    const float* x;     // [CLS] row of the first slot's generated pass, block output of this layer
    const float* tgt;   // the same of its target pass
    float* seed;        // the first slot's seed row: a [passes][D] seed buffer (seed_ps = D), or row 0 of a [rows][D] gradient buffer (seed_ps = Tld * D)
    size_t seed_ps;     // floats between the seed rows of consecutive passes
    float weight;
};
struct ClsLayers {
    int n, D;
    size_t x_ps, t_ps;   // floats between the rows of consecutive slots on the two sides
    int seed_step;       // passes between consecutive slots on the generated side (1, or the crops per pair of a per-crop-index launch)
    ClsLayer e[CLS_MAX_LAYERS];
};
// g: the gradient weight of the plain path, lambda / (float)D; grad_tab (optional, [slots]): the slot's own, a slot whose entry is 0
// takes no part (nothing of it is written).  One launch, one 256-thread workgroup per slot.
int cls_layers_launch(const ClsLayers& tab, int slots, float g, const float* grad_tab, float* part, size_t part_ps, float* values,
                      size_t values_ps, hipStream_t s);
// ---- id_layers.hip: the key-identity term over several ViT blocks ----
// A by-value table, one entry per layer in ascending block order.  Slot s (a B crop) compares the T x D fp32 keys at x + s * x_rs * ldx
// (rows ldx apart) with those at tgt + s * t_rs * ldt (rows ldt apart) and writes 2 * (g * weight) * (x - tgt) to grad + s * g_rs * ldg
// (rows ldg apart): the slot strides are counted in ROWS, since the top block's keys sit inside [rows][3D] and a lower block's in [rows][D].
// Every pointer and leading dimension is a multiple of 16 bytes, D of 4: the kernel moves float4s.
#define ID_MAX_LAYERS 12
#define ID_MAX_WG 64   // workgroups per (slot, layer) of the main launch unless the caller caps them lower
struct IdLayer {
    const float* x;     // keys of the first slot's generated pass: the key columns of qkv_last_f32 (ldx = 3D), or a block's [rows][D] fp32 key buffer
    const float* tgt;   // the same of its target pass
    float* grad;        // the first slot's rows of the block's key-gradient buffer
    int ldx, ldt, ldg;
    float weight;
};
struct IdLayers {
    int n, T, D;
    size_t x_rs, t_rs, g_rs;   // rows between consecutive slots on the generated, the target and the gradient side
    IdLayer e[ID_MAX_LAYERS];
};
// Workgroups per (slot, layer): one per 256 float4s of a slot's T * D keys, at most max_wg (0: ID_MAX_WG) -- a function of one slot's
// size alone, never of the batch.
int id_layers_wg(int T, int D, int max_wg);
// The main launch, grid (G, slots, n): workgroup b of (slot, layer) writes its fixed-tree sum of d^2 to scratch[(slot * n + layer) * G + b].
// g: the gradient weight of the plain path, lambda / (float)(T * D); grad_tab (optional, [slots]): the slot's own, a slot whose entry is
// 0 takes no part (nothing of it is read or written, in either launch).  Refuses a table that is not 16-byte aligned throughout.
int id_layers_launch(const IdLayers& tab, int slots, float g, const float* grad_tab, float* scratch, int max_wg, hipStream_t s);
// The finish launch, one wave per slot: values[s * values_ps + i] = (layer i's G partials added in index order) * (weight_i / (float)(T * D)),
// part[s * part_ps] = the fp32 sum of the slot's values, ascending from 0.
int id_layers_finish_launch(const IdLayers& tab, int slots, const float* grad_tab, const float* scratch, int max_wg, float* values,
                            size_t values_ps, float* part, size_t part_ps, hipStream_t s);
// ---- key_gram.hip: the key second-moment appearance term ----
// Slot s = pair * crops + crop compares the T x D keys of one block of a generated pass with those of its target pass through their
// D x D second moments.  The Gram operands are the transposed bf16 key copies, feature rows of tokens: slot s's feature f at
// kT_x + s * tx_ps + f * ldt_x (the target: kT_b, tb_ps, ldt_b); the backward reads the row-major bf16 keys k_x + s * k_ps (rows ldk apart)
// and adds into dk + s * dk_ps (rows lddk apart).  Every bf16 pointer, leading dimension and slot stride is a multiple of 16 bytes,
// D of 64, and a transposed row holds round_up(T, 8) columns; what the columns >= T hold reaches no output bit.
struct KeyGram {
    const bf16_t* kT_x;
    const bf16_t* kT_b;
    const bf16_t* k_x;
    int ldt_x, ldt_b, ldk;
    size_t tx_ps, tb_ps, k_ps;
    int T, D;
    bf16_t* delta;     // [slots][D][D]: G(K_x') - G(K_B') in bf16, both triangles
    float* part;       // slot s's tile partials at part + s * part_ps, key_gram_tiles(D) of them, each written exactly once
    size_t part_ps;
    float* value;      // [pairs]: the raw term, the pair's crops added in crop order
    float* dk;
    int lddk;
    size_t dk_ps;
    float scale;       // c = 4 lambda / (T D^2)
};
int key_gram_tiles(int D);   // upper-triangular 64 x 64 tiles of D x D; 0: D is no multiple of 64
int key_gram_check(const KeyGram& a, int pairs, int crops);
// the loss launch and its one-wave finish: delta, part and value of every slot; dk is not touched
int key_gram_loss_launch(const KeyGram& a, int pairs, int crops, hipStream_t s);
// dk[rows < T] += scale * k_x * delta for every slot
int key_gram_dk_launch(const KeyGram& a, int pairs, int crops, hipStream_t s);
// The term over several blocks, optionally centred: the layer is a grid dimension of instances of their own, the
// table goes by value.  Entry i holds block i's operands (the KeyGram fields of the same names; delta [slots][D][D], part [slots][part_ps]),
// its weight w_i (finite, > 0) and its scale c_i = fl(fl(4 lambda / (T D^2)) * w_i); strides, T and D are shared.  No two entries share
// a dk, delta or part pointer (refused).  centered: M(K) = K^T K / T - mu mu^T with mu the fp32 mean of the tokens < T; mu then holds
// [n][slots][2][D] floats (x' row, target row), written by a launch of its own in front of the loss launch.
constexpr int KEY_GRAM_MAX_LAYERS = 12;
struct KeyGramLayer {
    const bf16_t* kT_x;
    const bf16_t* kT_b;
    const bf16_t* k_x;
    float* dk;
    bf16_t* delta;
    float* part;
    float weight, scale;
};
struct KeyGramLayers {
    int n, centered;
    int ldt_x, ldt_b, ldk;
    size_t tx_ps, tb_ps, k_ps;
    int T, D;
    size_t part_ps;
    int lddk;
    size_t dk_ps;
    float* values;     // [pairs][n]: w_i * (block i's raw term, the pair's crops added in crop order)
    float* value;      // [pairs]: the fp32 sum of the pair's values, ascending from 0
    float* mu;         // centred only
    KeyGramLayer e[KEY_GRAM_MAX_LAYERS];
};
int key_gram_layers_check(const KeyGramLayers& t, int pairs, int crops);
// (the mean launch where centred,) the loss launch and its one-wave finish: delta and part of every entry, values and value; dk is not touched
int key_gram_layers_loss_launch(const KeyGramLayers& t, int pairs, int crops, hipStream_t s);
// dk_i[rows < T] += c_i * (k_x delta_i - 1 (delta_i mu_x)^T) for every entry and slot (the second part where centred)
int key_gram_layers_dk_launch(const KeyGramLayers& t, int pairs, int crops, hipStream_t s);
// ---- key_nn.hip: the nearest-neighbour key appearance term ----
// Slot s = pair * crops + crop pulls every key row of a generated pass towards the most similar key row, in cosine, of its target pass.
// Both operands are row-major bf16 keys, rows ldk apart: slot s's generated keys at k_x + s * kx_ps, its target keys at k_b + s * kb_ps.
// Every bf16 pointer, ldk and the slot strides are multiples of 16 bytes, D of 64.  Rows >= T of either array reach no output bit.
struct KeyNn {
    const bf16_t* k_x;
    const bf16_t* k_b;
    int ldk;
    size_t kx_ps, kb_ps;
    int T, D;
    float scale;       // lambda / T, rounded once on the host
    float eps;
    float inv_t;       // 1 / T, rounded once on the host
    int* match;        // [slots][T]: j*(i)
    float* cos;        // [slots][T]: c_i,j*(i)
    float* part;       // slot s's row-kernel partials at part + s * part_ps, key_nn_parts(T) of them, each written exactly once
    size_t part_ps;
    float* value;      // [pairs]: the raw term, the pair's crops added in crop order
    float* dk;         // slot s's key gradient at dk + s * dk_ps, rows lddk apart: ADDED into, rows < T
    int lddk;
    size_t dk_ps;
    void* ws;          // key_nn_ws_bytes(T, D, slots) bytes of scratch: the norms and the column-tile partials
};
int key_nn_parts(int T);                             // ceil(T / 4): workgroups of the row launch
size_t key_nn_ws_bytes(int T, int D, int slots);     // 0: T, D or slots < 1
int key_nn_check(const KeyNn& a, int pairs, int crops);
// the four launches: norms, match, row (match, cos, dk, part), finish (value)
int key_nn_launch(const KeyNn& a, int pairs, int crops, hipStream_t s);
// 2-D strided MSE: loss_accum[0] += weight * mean((a-b)^2); grad (optional) = weight * 2 (a-b) / (rows*cols)
int mse_launch(const float* a, int lda, const float* b, int ldb, int rows, int cols, float weight, float* loss_accum,
               float* grad, int ldg, hipStream_t s);
// same with separate scales: loss_accum[0] += loss_weight * mean(d^2); grad = grad_weight * 2 d / n
// partial sums only (no atomics): part = SPLICE_MSE_PARTIALS zeroed floats, summed in index order by the caller
#define SPLICE_MSE_PARTIALS 1024
int mse_partials_launch(const float* a, int lda, const float* b, int ldb, int rows, int cols, float loss_weight, float grad_weight,
                        float* part, float* grad, int ldg, hipStream_t s);
int mse2_launch(const float* a, int lda, const float* b, int ldb, int rows, int cols, float loss_weight, float grad_weight,
                float* loss_accum, float* grad, int ldg, hipStream_t s);

// ---- image_terms.hip: the image-space loss terms of the step (total variation of x', pixel identity of y') ----
#define IMAGE_TERMS_CHUNK 4096   // floats of an image per workgroup (and per partial slot) of the value kernel
// Partial sums of TV(x_i) (x: [n_x][3][xh][xw]; NULL: term off) into part_tv + i * part_istride and of mean((y_i - b_i)^2) (y, b:
// [n_y][3][yh][yw]; y NULL: term off) into part_pix + i * part_istride: chunk c of an image writes slot c, ceil(3 h w / IMAGE_TERMS_CHUNK) <=
// part_cap slots per image, each already divided by its mean's count; the other slots are not written.  One launch; none with both off.
int image_terms_value_launch(const float* x, int n_x, int xh, int xw, float* part_tv, const float* y, const float* b, int n_y, int yh, int yw,
                             float* part_pix, size_t part_istride, size_t part_cap, hipStream_t s);
// d += lambda * dTV/dx  and  d += lambda * 2 (y - b) / (3 h w)  on [n_img][3][h][w], in place
int image_tv_grad_add_launch(const float* x, float* d, int n_img, int h, int w, float lambda, hipStream_t s);
int image_pix_grad_add_launch(const float* y, const float* b, float* d, int n_img, int h, int w, float lambda, hipStream_t s);
