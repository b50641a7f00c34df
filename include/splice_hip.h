/* splice_hip.h -- C ABI of libsplice_hip.so: the MI355X (gfx950) implementation of the
 * Splice per-pair optimisation hot path.
 *
 * The reference (omerbt/Splice) has NO native/FFI boundary: its hot path is the Python API
 * of models/extractor.py, models/model.py, models/unet/skip.py, models/unet/common.py, util/losses.py, util/util.py
 * and the loop of train.py:51-80, executed as stock ATen ops.  This header is the boundary
 * a maintainer binds instead (ctypes stub: splice_amd/_lib.py).  Each
 * entry point cites the reference code it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  All pointers are DEVICE
 *     pointers owned by the caller unless stated otherwise; the library never frees them.
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and returns 0 (SPLICE_OK) or a negative error code; the message
 *     is available from splice_last_error() (thread-local).  No exception crosses the ABI.
 *   - bf16 tensors are raw uint16 (splice_bf16).  "Tld" is the per-pass row stride of a
 *     token matrix (multiple of 32, >= T); rows T..Tld-1 of a pass are padding.
 *   - one handle <-> one device <-> one stream at a time; handles are not thread-safe;
 *     handles on different GPUs are independent (one process per GPU, no collectives).
 */
#ifndef SPLICE_HIP_H
#define SPLICE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t splice_bf16;
typedef void* splice_stream_t;

#define SPLICE_OK 0
#define SPLICE_ERR_ARG -1
#define SPLICE_ERR_HIP -2
#define SPLICE_ERR_STATE -3
#define SPLICE_ERR_NOMEM -4

int splice_version(void);
/* 1 when the library was built with the timing-only experiment switches (make DEV=1: SPLICE_STEP_ABLATE skips work, results
 * are garbage); 0 for the product build.  bench.py refuses to run on a 1. */
int splice_dev_switches(void);
const char* splice_last_error(void);

/* ------------------------------------------------------------------ op level: ViT GEMMs
 * C[M][N] = sum_k A[m][k] * B[n][k]  (bf16 in, fp32 accumulate) + fused epilogue.
 * Replaces the nn.Linear / Conv2d(patch-embed) call sites inside the DINO ViT that the
 * reference reaches through self.model(input_img) (models/extractor.py:83,91,99) and their
 * autograd dgrads (train.py:78).  K % 64 == 0, lda/ldb % 8 == 0. */
typedef struct splice_gemm_epilogue {
    const float* bias;        /* [N] */
    const float* resid;       /* fp32 [*][ldr]; row = resid_mod ? row % resid_mod : row */
    int ldr, resid_mod;
    float* out_f32;           /* [M][ldo] */
    int ldo;
    splice_bf16* out_bf;      /* [M][ldbf] */
    int ldbf;
    splice_bf16* out_bf_t;    /* transposed [N][ldt] (ldt % 4 == 0) */
    int ldt;
    splice_bf16* out_pre;     /* [M][ldp] value before GELU (may be NULL); written for rows >= pre_row_lo */
    int ldp, pre_row_lo;
    const splice_bf16* aux;   /* [M][ldaux] pre-GELU activations for SPLICE_EPI_GELU_GRAD */
    int ldaux;
    float* out_f32_cols;      /* fp32 copy of columns [col_lo, col_hi): [M][ld_cols] */
    int ld_cols, col_lo, col_hi;
    float alpha;
    int ksplit;               /* > 1 with flags == SPLICE_EPI_OUT_F32 only: K is cut into ksplit slices, slice s writes */
    long long slab_stride;    /* out_f32 + s * slab_stride; the consumer adds the slabs in order (deterministic split-K).
                               * With splice_gemm_splitk_slabs(M, ksplit) == 1 (many rows) the slices are summed IN the kernel,
                               * in the same order -- the same bits -- and only slab 0 is written.
                               * K % (ksplit * 64) != 0: the call runs UNSPLIT -- slab 0 holds the whole product and the other slabs
                               * are not written -- while splice_gemm_splitk_slabs(M, ksplit) still answers ksplit: a caller that
                               * sums the slabs must keep K a multiple of ksplit * 64 (the ViT engine's ks rules do) */
    /* SPLICE_EPI_ROWDOT (with OUT_BF): rowdot[(row / rd_rows) * (N/64) * rd_rows + (col/64) * rd_rows + row % rd_rows]
     * = sum over the 64 columns [col, col+64) of bf16(C[row][c]) * rd_other[row][c] -- the attention backward's
     * delta = rowsum(dO * O) per (pass, head, query), formed where dO is produced (proj dgrad).  N % 64 == 0. */
    const splice_bf16* rd_other;   /* [M][ld_rd] */
    int ld_rd, rd_rows;
    float* rowdot;
    /* SPLICE_EPI_SCALE_RC (fp8 operands): C[m][n] *= row_scale[m] * col_scale[n] before the bias -- the per-token scale of the
     * quantised activations times the per-output-channel scale of the quantised weights */
    const float* row_scale;        /* [M]; NULL = 1 (unscaled e4m3 activations) */
    const float* col_scale;        /* [N] */
    /* SPLICE_EPI_OUT_F8: the result as e4m3 bytes [M][ld8] (saturated at +-448, no scale: the format's relative precision holds
     * over 2^-9 .. 448) -- the GELU output of fc1 as the operand of the fp8 fc2.  N % 16 == 0, ld8 % 16 == 0. */
    uint8_t* out_f8;
    int ld8;
    /* SPLICE_EPI_OUT_F8T: the same e4m3 bytes transposed, [N][ldt8] (ldt8 % 16 == 0) -- the token-contiguous operands of the
     * fp8 attention (V^T tiles), written next to the row-major copy by the QKV projection */
    uint8_t* out_f8_t;
    int ldt8;
} splice_gemm_epilogue;

enum {
    SPLICE_EPI_BIAS = 1, SPLICE_EPI_RESID = 2, SPLICE_EPI_OUT_F32 = 4, SPLICE_EPI_OUT_BF = 8,
    SPLICE_EPI_OUT_T = 16, SPLICE_EPI_GELU = 32, SPLICE_EPI_GELU_GRAD = 64,
    SPLICE_EPI_COLS_F32 = 128, SPLICE_EPI_ALPHA = 256, SPLICE_EPI_ROWDOT = 512, SPLICE_EPI_SCALE_RC = 1024, SPLICE_EPI_OUT_F8 = 2048,
    SPLICE_EPI_OUT_F8T = 4096
};

int splice_gemm_nt_bf16(unsigned flags, const splice_bf16* A, int lda, const splice_bf16* B, int ldb,
                        int M, int N, int K, const splice_gemm_epilogue* epi, splice_stream_t stream);

/* The same product with e4m3 (OCP fp8) operands on the gfx950 block-scaled K = 128 MFMA (v_mfma_scale_f32_16x16x128_f8f6f4
 * with unit block scales: twice the bf16 issue rate, half the operand bytes): A [M][K] and B [N][K] are bytes, lda / ldb in
 * bytes (multiples of 16), K % 128 == 0.  BASELINE configs[4] ("fp8 MFMA attention + self-sim path"): the QKV, fc1 and fc2
 * projections of a ViT context in fp8 mode (splice_vit_ctx_set_fp8).  flags must contain SPLICE_EPI_SCALE_RC. */
int splice_gemm_nt_fp8(unsigned flags, const uint8_t* A, int lda, const uint8_t* B, int ldb, int M, int N, int K,
                       const splice_gemm_epilogue* epi, splice_stream_t stream);
/* Row-wise e4m3 quantisation: q[r][:] = fp8(x[r][:] * 448 / amax_r), scale[r] = amax_r / 448 (x ~= q * scale[r]).
 * x fp32 [rows][ldx] (cols % 8 == 0), q bytes [rows][ldq].  Packs the frozen weights per output channel. */
int splice_quantize_rows_fp8(const float* x, int ldx, uint8_t* q, int ldq, float* scale, int rows, int cols, splice_stream_t stream);
/* number of slabs a split-K call with M rows leaves for its consumer: ksplit (few rows) or 1 (the sum formed in the kernel) */
int splice_gemm_splitk_slabs(int M, int ksplit);
/* benchmarking / test hook (tools/gemm_bench.py, tests/test_ops_gpu.py): force the tile shape, 0 = automatic; tile + 10 * ring with tile 1..3 =
 * the one-barrier tiles 128x128, 128x64, 64x64 and ring 0 / 1 / 2 = 2 / 4 / 3 LDS stages; 5 = the 8-phase 256x256 tile (gemm8p.h) wherever its operand and
 * epilogue constraints hold (N % 256 == 0, K % 128 == 0, bias [+GELU] -> bf16 or bias + residual -> fp32) */
int splice_gemm_force_tile(int tile);
/* test / benchmarking hook: attention forward launch form, 0 = automatic.  bf16: 41 / 42 / 48 = the 32x32x16 kernel with 4 / 2 / 8 waves per workgroup
 * (same bits from all three, tests/test_ops_gpu.py); e4m3 forward: queries per wave / 16 + 10 * (two wave groups) */
int splice_attention_variant(int variant);
/* test / benchmarking hook: != 0 -> the stand-alone attention entry points take q columns pre-multiplied by scale * log2(e) and scale = ln 2
 * (what the ViT engine runs: attn_fwd_x32_kernel<., FOLD>, attn_bwd_x32_kernel); 0 -> plain q and scale = d^-1/2 */
int splice_attention_qfold(int on);
/* test / benchmarking hook: attention backward form, 0 automatic; 1 = the 16x16x32 halves (what plain q gets in any case); pre-scaled q only:
 * 2 / 3 = the 32x32x16 halves in one / two launches, 4 = one launch of two-wave workgroups (same bits from 2, 3 and 4) */
int splice_attention_bwd_variant(int variant);

/* LayerNorm(D, eps) of the DINO blocks (eps 1e-6), fp32 in -> bf16 out, and its dgrad
 * accumulated into the fp32 residual-gradient stream: g_out = g_in + dLN(dy). */
int splice_layernorm_fwd(const float* x, const float* gamma, const float* beta, splice_bf16* y,
                         float* mean, float* rstd, int rows, int D, float eps, splice_stream_t stream);
int splice_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                         const float* rstd, const float* g_in, float* g_out, splice_bf16* g_out_bf,
                         int rows, int D, splice_stream_t stream);

/* Multi-head self-attention (head dim 64), DINO Attention.forward: softmax(q k^T d^-1/2) v.
 * qkv [B*Tld][3D] bf16 (layout of models/extractor.py:136-151).  qkvT / ldt (the transpose [3D][ldt]) are not read any more --
 * V^T comes out of the V tile inside LDS (ds_read_b64_tr_b16) -- and may be NULL / 0; the parameters stay for ABI stability.
 * out [B*Tld][D] bf16; lse [B][H][Tld] fp32 (saved for the backward).
 * SPLICE_ERR_ARG, and nothing is launched, for B < 1, T < 1, T > Tld, Tld % 32 != 0, D % 64 != 0, H != D / 64 or a NULL qkv, out or lse. */
int splice_attention_fwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld,
                         int D, int H, float scale, splice_bf16* out, float* lse, splice_stream_t stream);
/* The forward with e4m3 operands (BASELINE configs[4]): Q K^T and P V on the fp8 MFMA from UNSCALED e4m3 copies of qkv --
 * qkv8 bytes [B*Tld][3D] row-major and qkvT8 bytes [3D][ldt8] transposed (ldt8 % 16 == 0), as the fp8 QKV projection writes them
 * (SPLICE_EPI_OUT_F8 | SPLICE_EPI_OUT_F8T).  Output / lse as splice_attention_fwd; the backward runs on the bf16 tensors.
 * Refuses what splice_attention_fwd refuses (qkv8 and qkvT8 in the place of qkv), and ldt8 % 16 != 0. */
int splice_attention_fwd_fp8(const uint8_t* qkv8, const uint8_t* qkvT8, int ldt8, int B, int T, int Tld, int D, int H, float scale,
                             splice_bf16* out, float* lse, splice_stream_t stream);
/* dqkv [B*Tld][3D] bf16 from dout [B*Tld][D]; delta is [B][H][Tld] fp32 scratch (rowsum(dO * O), formed by the call).
 * qkvT / ldt / doutT are not read any more (the kernels take the transposed operands out of the token tiles with
 * ds_read_b64_tr_b16) and may be NULL / 0: the parameters stay for ABI stability.
 * SPLICE_ERR_ARG, and nothing is launched (delta is not formed either), for B < 1, T < 1, T > Tld, Tld % 32 != 0, D % 64 != 0, H != D / 64 or a
 * NULL qkv, out, lse, dout, delta or dqkv. */
int splice_attention_bwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld,
                         int D, int H, float scale, const splice_bf16* out, const float* lse,
                         const splice_bf16* dout, const splice_bf16* doutT, float* delta,
                         splice_bf16* dqkv, splice_stream_t stream);
/* attention probabilities [B][H][T][T] fp32 (the tensors models/extractor.py:44-45 hooks).
 * SPLICE_ERR_ARG, and nothing is launched, for B < 1, T < 1, T > Tld, Tld % 32 != 0, D % 64 != 0, H != D / 64 or a NULL qkv, lse or probs. */
int splice_attention_probs(const splice_bf16* qkv, int B, int T, int Tld, int D, int H, float scale,
                           const float* lse, float* probs, splice_stream_t stream);

/* dino_structure_transforms (data/transforms.py:30-37) on a device image fp32 [3][H][W] in [0,1]: horizontal flip,
 * ColorJitter (order[k] in {0 brightness, 1 contrast, 2 saturation, 3 hue}: the op order of this draw, n_ops = 0 for
 * none; factors[4] indexed by op) and GaussianBlur(3) (blur_sigma <= 0 for none); torchvision-0.10 tensor arithmetic.
 * out != img; scratch >= 3*H*W + 256 floats.  Replaces the per-step PIL pipeline of data/Dataset.py:62-70. */
int splice_augment_structure(const float* img, float* out, float* scratch, int H, int W, int flip, int n_ops, const int* order,
                             const float* factors, float blur_sigma, splice_stream_t stream);

/* attn_cosine_sim (models/extractor.py:4-9) on K fp32 [T][ldk] (D columns): S fp32 [T][T].
 * `ws` is caller scratch of splice_keys_selfsim_ws_bytes(T, D) bytes; the backward needs the
 * state the forward left in it. */
size_t splice_keys_selfsim_ws_bytes(int T, int D);
int splice_keys_selfsim_fwd(const float* K, int ldk, int T, int D, float eps, float* S, void* ws,
                            splice_stream_t stream);
int splice_keys_selfsim_bwd(const float* dS, const float* S, int T, int D, float eps, float* dK, int lddk,
                            int accumulate, void* ws, splice_stream_t stream);

/* F.mse_loss(a, b) (util/losses.py:82,93,104) on 2-D strided fp32 views:
 * loss_accum[0] += weight * mean((a-b)^2); grad (optional) = weight * 2 (a-b) / (rows*cols).
 * Workgroup partials are added in a fixed order (no float atomics) through a scratch line owned by the (device, stream)
 * pair of the call: calls on different streams or devices are independent. */
int splice_mse(const float* a, int lda, const float* b, int ldb, int rows, int cols, float weight,
               float* loss_accum, float* grad, int ldg, splice_stream_t stream);

/* patch-embed operand builders (Conv2d(3,D,p,p) as a GEMM; optional fused ImageNet Normalize,
 * util/losses.py:19) and helpers */
int splice_patchify(const float* img, splice_bf16* patches, int B, int H, int W, int p, int Tld,
                    int normalize, splice_stream_t stream);
int splice_unpatchify(const float* dpatches, float* dimg, int B, int H, int W, int p, int Tld,
                      int normalize, splice_stream_t stream);
int splice_cast_f32_bf16(const float* x, splice_bf16* y, size_t n, splice_stream_t stream);
int splice_cast_bf16_f32(const splice_bf16* x, float* y, size_t n, splice_stream_t stream);
int splice_transpose_f32_bf16(const float* x, splice_bf16* y, int rows, int cols, int ldy, splice_stream_t stream);
/* transforms.Resize on tensors (util/losses.py:20; torchvision 0.10: bilinear, align_corners=False,
 * no antialias) on `planes` images [h][w] -> [oh][ow], and its exact adjoint (deterministic gather). */
int splice_resize_bilinear_fwd(const float* in, float* out, int planes, int h, int w, int oh, int ow, splice_stream_t stream);
int splice_resize_bilinear_bwd(const float* dout, float* din, int planes, int h, int w, int oh, int ow, splice_stream_t stream);

/* ------------------------------------------------------------------ ViT engine (handle level)
 * Replaces VitExtractor.__init__ + the hooked self.model(img) forwards of
 * models/extractor.py:19-103 and the autograd backward through them (train.py:78).
 * Weights are the DINO state-dict entries (public checkpoint key names), frozen and
 * re-packed to bf16 ([out][in] and [in][out]) inside the handle. */
int splice_vit_create(int patch, int dim, int depth, int heads, void** out_handle);
void splice_vit_destroy(void* vit);
int splice_vit_set_param(void* vit, const char* name, const float* data, long long numel, splice_stream_t stream);
/* The factor the stored q columns of every layer's qkv carry (d^-1/2 * log2(e)).  splice_vit_read_tensor
 * kinds 1 and 3 divide it out of the copy; kind 7 (= kind 1 as stored) and the zero-copy splice_vit_get_tensor pointers do not -- attention entry
 * points fed with stored q take scale = ln 2 instead of d^-1/2. */
float splice_vit_qscale(void* vit);
int splice_vit_params_complete(void* vit);
/* BASELINE configs[4] fp8 path: prepares e4m3 copies of the QKV / fc1 / fc2 weights (per-output-channel scales).  A context
 * opts in with splice_vit_ctx_set_fp8: its three big forward projections then run on the fp8 MFMA (e4m3 LayerNorm outputs with
 * per-token scales, e4m3 GELU output), de-quantised in the GEMM epilogues.  dim % 128 == 0.  The backward (dgrad through bf16
 * weights) is unchanged. */
int splice_vit_enable_fp8(void* vit, splice_stream_t stream);
/* A context = one (batch, image shape): owns the activations of the last forward.
 * pos_TD: position table for this token grid, fp32 [T][dim] (interpolate_pos_encoding done
 * once per shape by the host). need_grad != 0 also allocates the backward workspace. */
int splice_vit_ctx_create(void* vit, int B, int H, int W, const float* pos_TD, int need_grad,
                          splice_stream_t stream, void** out_ctx);
void splice_vit_ctx_destroy(void* ctx);
int splice_vit_ctx_info(void* ctx, int* T, int* Tld, int* rows);
/* on != 0: behind the QKV projection of the TOP block only the [CLS] row of every pass is computed -- all the Splice losses
 * read of that block besides its keys (util/losses.py:90: [CLS] of block 11).  Then kind-0 rows other than [CLS] are
 * undefined for layer depth-1, and d_block[depth-1] must be zero outside the [CLS] rows.  splice_step_create switches its
 * contexts to this mode; the extractor API (models/extractor.py:81-103 hands out every token) never does. */
int splice_vit_ctx_set_top_cls_only(void* ctx, int on);
/* The blocks (n distinct indices in [0, depth)) whose QKV projection also writes the transposed bf16 copy of its output, [3D][rows], as
 * the top block's always does -- what the structure loss over the keys of those blocks multiplies in its dK product
 * (splice_step_set_ssim_layers calls this on its contexts).  Before the context's first forward only.  splice_vit_get_tensor kind 8
 * returns the copies; a context without this call runs the launches it always ran. */
int splice_vit_ctx_set_transposed_layers(void* ctx, int n, const int* layers);
/* The blocks (n distinct indices in [0, depth)) below the top whose QKV projection also writes the KEY columns of its output in fp32,
 * [rows][D] -- the values its bf16 qkv rounds -- what the key-identity loss over those blocks compares (splice_step_set_id_layers calls
 * this on its global context).  The top block may be named and changes nothing: its fp32 keys stay columns [D, 2D) of kind 3.  Before
 * the context's first forward only; refused on an fp8 context (which in turn refuses fp8 behind it).  splice_vit_get_tensor kind 9
 * returns the buffers; every tensor the context wrote before keeps its bits, and a context without this call runs the launches it
 * always ran. */
int splice_vit_ctx_set_key_f32_layers(void* ctx, int n, const int* layers);
/* [CLS]-row gradient seeds of block outputs: seeds = [depth] device pointers, each [B][D] fp32 (row p: the gradient w.r.t. row 0 of block
 * l's output of pass p) or NULL, armed for the passes [pass_begin, pass_end).  A later splice_vit_backward whose range meets the armed
 * one adds seeds[l]'s rows into row 0 of those passes of its gradient stream in front of block l's backward (g += seed, g_bf = bf16(g);
 * where the stream is not live yet it starts there, zero outside those rows): what a d_block[l] that is zero outside row 0 gives,
 * element for element, without the [rows][D] buffer.  A backward the armed range does not meet launches what it always did.  The
 * pointer table is copied; seeds NULL or an empty range disarms.  Needs a context created with need_grad. */
int splice_vit_ctx_set_cls_seeds(void* ctx, const float* const* seeds, int pass_begin, int pass_end);
/* precision of THIS context's forward: 0 bf16 (default); 1 = QKV / fc1 / fc2 projections on the fp8 MFMA; 3 = those + the attention
 * forward (Q K^T, P V) on the fp8 MFMA.  Needs splice_vit_enable_fp8 on the engine.  The backward is bf16 in every mode. */
int splice_vit_ctx_set_fp8(void* ctx, int mode);
/* img fp32 [B][3][H][W]; normalize != 0 fuses transforms.Normalize (util/losses.py:19). */
int splice_vit_forward(void* ctx, const float* img, int normalize, splice_stream_t stream);
/* same; passes [0, grad_pass_begin) are no-grad targets (util/losses.py:79,91,101 `with torch.no_grad()`):
 * tensors only a backward would read are not stored for them */
int splice_vit_forward_ex(void* ctx, const float* img, int normalize, int grad_pass_begin, splice_stream_t stream);
/* same, restricted to passes (images) [pass_begin, pass_end) of the ctx batch; img is still the full [B] batch.
 * The forward is row-parallel over the token matrix: disjoint pass ranges of one ctx may run concurrently on
 * different streams (splice_step_run computes the no-grad target passes beside the generator forward). */
int splice_vit_forward_passes(void* ctx, const float* img, int normalize, int grad_pass_begin, int pass_begin, int pass_end,
                              splice_stream_t stream);
/* kind 0: block output l fp32 [rows][D] (models/extractor.py:56-60) | 1: raw qkv l bf16
 * [rows][3D] (:68-72) | 2: attention output l bf16 [rows][D] | 3: last-layer qkv fp32
 * [rows][3D] | 4: lse l fp32 [B][H][Tld] | 5: embedded tokens fp32 [rows][D] | 6: raw qkv l transposed, bf16 [3D][rows] (l = depth - 1
 * only) | 7: as 1 | 8: as 6, of the top block or a block named by splice_vit_ctx_set_transposed_layers (any other is refused) | 9: the
 * key columns of raw qkv l in fp32, [rows][D], of a block below the top named by splice_vit_ctx_set_key_f32_layers (any other is refused;
 * the top block's fp32 keys are columns [D, 2D) of kind 3).
 * ZERO-COPY: the pointers are the engine's own buffers, so the q columns of kinds 1 / 3 / 6 / 7 carry the factor splice_vit_qscale()
 * (a C caller that wants the reference's q divides it out, or calls splice_vit_read_tensor, whose copies of kinds 1 and 3
 * are un-scaled -- in bf16 for kind 1: one more rounding; Python's VitExtractor reads kind 7 and divides in fp32). */
int splice_vit_get_tensor(void* ctx, int kind, int layer, void** out_ptr);
int splice_vit_read_tensor(void* ctx, int kind, int layer, void* dst, size_t bytes, splice_stream_t stream);
/* dgrad-only backward over passes [pass_begin, pass_end): gradients may be injected at
 * any block output (d_block[l], fp32 [rows][D]), any raw qkv (d_qkv[l], fp32 [rows][3D])
 * or its key columns only (d_keys[l], fp32 [rows][D]); arrays of `depth` pointers, NULL
 * entries / NULL arrays allowed.  d_img fp32 [B][3][H][W] (selected passes written). */
int splice_vit_backward(void* ctx, int pass_begin, int pass_end, const float* const* d_block,
                        const float* const* d_qkv, const float* const* d_keys, float* d_img,
                        int normalize, splice_stream_t stream);

/* ------------------------------------------------------------------ generator engine
 * The reference's define_G() -> skip() U-Net (models/networks.py:56-58, models/unet/skip.py:4-102,
 * models/unet/common.py:11-124), forward + full backward, fp32.  Parameters / gradients are
 * ONE flat fp32 arena in netG.parameters() order; splice_gen_tensor_info gives the per-tensor
 * (state_dict name, offset, numel) table.  A plan = (N side-by-side generator calls, H, W). */
int splice_gen_create(void** out_handle);
/* Any skip() the kernels cover (models/unet/skip.py:4-11): e.g. the feature-inversion net of inversion.py:21-25 -- 6 scales,
 * 32 noise input channels, filter_size_down = filter_size_up = {7,7,5,5,3,3}, pad = 'reflection'.  Same engine, same plans,
 * same flat parameter arena (state_dict names follow the reference's numbering, incl. the ".1" Conv2d index behind a
 * ReflectionPad2d).  Fixed: stride-2 'stride' down-sampling, bilinear up-sampling, LeakyReLU(0.2), 1x1 skip and post-up
 * filters, sigmoid head, every scale with skip channels.  NULL = the default architecture of define_G. */
#define SPLICE_GEN_MAX_SCALES 6
typedef struct splice_gen_arch {
    int n_scales, in_channels, out_channels;
    int down[SPLICE_GEN_MAX_SCALES], up[SPLICE_GEN_MAX_SCALES], skip[SPLICE_GEN_MAX_SCALES];   /* channels (<= 128) */
    int filter_down[SPLICE_GEN_MAX_SCALES], filter_up[SPLICE_GEN_MAX_SCALES];                  /* 1 / 3 / 5 / 7 */
    int filter_skip;                                                                          /* 1 */
    int reflect;                                                                              /* pad = 'reflection' (else 'zero') */
} splice_gen_arch;
int splice_gen_create_arch(const splice_gen_arch* arch, void** out_handle);
void splice_gen_destroy(void* gen);
long long splice_gen_param_count(void* gen);
int splice_gen_num_tensors(void* gen);
int splice_gen_tensor_info(void* gen, int i, const char** name, long long* offset, long long* numel);
int splice_gen_plan_create(void* gen, int N, int H, int W, int need_grad, void** out_plan);
void splice_gen_plan_destroy(void* plan);
/* y = netG(x) per image (models/model.py:15-23): x,y fp32 [N][3][H][W] */
int splice_gen_forward(void* plan, const float* params, const float* x, float* y, splice_stream_t stream);
/* same, without the plan's private copies of x and y (two launches): the caller keeps both buffers unchanged until the
 * matching splice_gen_backward has run (splice_step_run owns its staged inputs and outputs) */
int splice_gen_forward_borrowed(void* plan, const float* params, const float* x, float* y, splice_stream_t stream);
/* parameter gradients of the last forward from dy = dL/dy (autograd backward through netG,
 * train.py:78); grads overwritten, or accumulated when accumulate != 0 */
int splice_gen_backward(void* plan, const float* params, const float* dy, float* grads, int accumulate,
                        splice_stream_t stream);
/* BatchNorm buffers of netG.state_dict() ("<bn>.running_mean", "<bn>.running_var"; fp32 arena in state_dict order) and their
 * train-mode update from the batch statistics of the LAST forward of each listed plan, applied in the order given (the
 * order of the netG calls).  Plans of independent images (arena stride set) update arena n for image n. */
long long splice_gen_buffer_count(void* gen);
int splice_gen_num_buffers(void* gen);
int splice_gen_buffer_info(void* gen, int i, const char** name, long long* offset, long long* numel);
int splice_gen_running_stats_update(void* const* plans, int n_plans, float* running, long long running_stride, float momentum,
                                    splice_stream_t stream);
/* torch.optim.Adam(lr, betas) step (util/util.py:28-32, train.py:79) fused over the arena;
 * step counts from 1; zero_grad != 0 also clears grads (optimizer.zero_grad, train.py:56) */
int splice_adam_step(float* params, float* grads, float* m, float* v, long long n, float lr, float beta1,
                     float beta2, float eps, int step, int zero_grad, splice_stream_t stream);
/* One step of the optimiser the config names (util/util.py:28-39: optimizer adam / rmsprop / sgd, every other argument at
 * torch.optim's default) fused over the arena.  kind 0 Adam: hp0 = beta1, hp1 = beta2, step counts from 1 (as splice_adam_step).
 * kind 1 RMSprop: hp0 = alpha (0.99), v holds square_avg, m is not touched (may be NULL); no momentum, not centred.  kind 2 SGD:
 * p -= lr * g; m and v are not touched (may be NULL).  zero_grad != 0 also clears grads.  An element's result does not depend on
 * where it sits in the arena. */
int splice_optim_step(int kind, float* params, float* grads, float* m, float* v, long long n, float lr, float hp0, float hp1,
                      float eps, int step, int zero_grad, splice_stream_t stream);
/* as splice_optim_step, plus g2 (may be NULL): a second gradient arena of n floats folded in first (grads += g2, written back), and
 * lr_dev (may be NULL): a device float the kernel reads as the learning rate when it runs (lr is then ignored) */
int splice_optim_step_ex(int kind, float* params, float* grads, const float* g2, float* m, float* v, long long n, float lr,
                         const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad, splice_stream_t stream);
/* n_pairs arenas in one launch, each with its own learning rate: pair p's n floats start at p * stride (stride >= n, a multiple of 4)
 * and use lr_dev[p] (device, n_pairs floats).  All n_pairs * stride floats are updated (the padding holds zero gradients); g2, m
 * and v span the same range.  Bit for bit the result of n_pairs splice_optim_step_ex calls, one per arena with its lr. */
int splice_optim_step_pairs(int kind, float* params, float* grads, const float* g2, float* m, float* v, int n_pairs, long long stride,
                            long long n, const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad,
                            splice_stream_t stream);
/* Weight average (an extension; the reference keeps none): as splice_optim_step_ex, plus `ema`, an arena of n floats written in the same
 * walk behind the parameter of the element.  With p' the parameter just written and step the update's count (>= 1, for every kind):
 * step <= ema_start: ema = p'; later ema = ema_decay * ema + (1 - ema_decay) * p' (fp32, one rounding per operation).  0 < ema_decay < 1,
 * ema_start >= 0.  params, m and v are, bit for bit, those of the same call to splice_optim_step_ex. */
int splice_optim_step_ema(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, long long n, float lr,
                          const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad, float ema_decay, int ema_start,
                          splice_stream_t stream);

/* The extended rules of the fused update (extensions; the reference sets none of these): torch.optim's weight_decay, momentum / dampening /
 * nesterov (SGD), momentum / centered (RMSprop), amsgrad (Adam) and AdamW's decoupled decay (kind 0 with `decoupled`).  A call that
 * passes this record runs the extended kernels, also when every option is neutral; they then compute the bits of the plain rules
 * (a zero weight_decay or momentum is a branch, not a multiplication by zero).  An option the kind has no argument for must be neutral. */
typedef struct splice_optim_ext {
    float weight_decay;   /* >= 0, finite.  decoupled == 0: L2, added to the gradient the rule sees; decoupled != 0: AdamW */
    float momentum;       /* >= 0, finite; SGD and RMSprop: the buffer lives in the m arena */
    float dampening;      /* SGD */
    int nesterov;         /* SGD; needs momentum > 0 and dampening == 0 */
    int decoupled;        /* Adam: p = p (1 - lr weight_decay) in front of the update, the moments see the gradient alone (torch.optim.AdamW) */
    int amsgrad;          /* Adam: the w arena holds max_exp_avg_sq */
    int centered;         /* RMSprop: the w arena holds grad_avg */
} splice_optim_ext;
/* The arithmetic, fp32 with one rounding per operation and no contraction, like the plain rules.  g: the gradient the rule sees today,
 * fl(grads + g2), times the clip coefficient under clipping; where grads is written back (g2 or zero_grad) it holds exactly what the
 * plain rules leave there -- the decay term is never written into the gradient arena, and the norm launches see no decay.  t: the
 * update's step count (>= 1): the device count where the call has one, else `step`; EVERY extended rule needs it.  lr: the slot's
 * effective learning rate.  wd = weight_decay, mu = momentum.
 *   SGD      d = wd ? g + wd p : g.  mu > 0: b = (t == 1) ? d : mu b + (1 - dampening) d, kept in m; d = nesterov ? d + mu b : b.
 *            p -= lr d.  "First step" means t == 1: a slot whose first update was skipped by the non-finite-norm guard starts from
 *            b = 0 at t == 2, where torch ("the buffer is None") would copy d.
 *   RMSprop  d as SGD; v = alpha v + (1 - alpha) d d.  centered: a = alpha a + (1 - alpha) d, kept in w; avg = sqrt(v - a a) + eps, not
 *            clamped, as torch does not clamp it: a gradient that is constant over thousands of steps can round v - a a below 0 and
 *            the weights then turn NaN.  Else avg = sqrt(v) + eps.  mu > 0: b = mu b + d / avg, kept in m; p -= lr b.  Else p -= lr (d / avg).
 *   Adam     decoupled and wd > 0: first p = p (1 - lr wd), then d = g; else d = wd ? g + wd p : g.  m and v as splice_optim_step with d
 *            for g.  amsgrad: w = max(w, v) and denom = sqrt(w) / bc2_sqrt + eps; else denom = sqrt(v) / bc2_sqrt + eps.
 *            p -= (lr / bc1) (m / denom).
 * A slot that is frozen by the stop rule or skipped by the clip guard writes none of p, m, v, w, and its decoupled decay is not applied.
 * The padding floats between two arenas (p = 0, g = 0) stay 0 under every rule.  w is laid out like m and v, is needed exactly with
 * amsgrad / centered, and takes part in the 16-byte alignment test of the walk like every arena.
 * splice_optim_step_ext: one arena, as splice_optim_step_ex (step >= 1 for every kind). */
int splice_optim_step_ext(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* w, long long n, float lr,
                          const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad, const splice_optim_ext* options,
                          splice_stream_t stream);

/* live timing of one kernel family (bench.py roofline leg, prof.hip): while a family is armed its kernels are launched with
 * a start / stop event pair each (hipExtLaunchKernelGGL: the kernel's own begin / end time stamps, as rocprofv3 reports them).
 * which 1 = fc1 GEMM fwd, 2 = qkv GEMM fwd (layers 0..depth-2), 3 = attention fwd, 4 = fc2 GEMM fwd, 5 = split-K dgrad GEMMs
 * (fc1^T, qkv^T), 6 = attention bwd, 7 = generator (all kernels of splice_gen_forward* / splice_gen_backward), 8 = key
 * self-similarity loss kernels, 9 = proj GEMM fwd.  end: summed kernel time, host calls of the family, kernels launched. */
int splice_prof_begin(int which);
int splice_prof_end(float* total_ms, int* launches);
int splice_prof_end_ex(float* total_ms, int* calls, int* kernels);
/* as splice_prof_end_ex, plus one text line per distinct kernel of the family in `detail` (may be NULL):
 * "kernel\tlaunches\ttotal ms\talgorithmic FLOPs\talgorithmic bytes\n", longest first (the work columns are what the launchers noted: the convolutions) */
int splice_prof_end_detail(float* total_ms, int* calls, int* kernels, char* detail, int detail_len);
int splice_prof_active(void);
int splice_vit_ctx_dims(void* ctx, int* B, int* H, int* W, int* D, int* depth, int* heads, int* patch);
int splice_gen_plan_dims(void* plan, int* N, int* H, int* W, long long* nparams);
/* stride > 0: the N images of the plan are INDEPENDENT generators (P image pairs optimised side by side: the reference
 * runs train.py once per pair): image n reads params + n*stride, its gradient goes to grads + n*stride, BatchNorm and
 * launch policies are per image -- a pair's result is bit-identical to its N = 1 run.  0 (default): one generator. */
int splice_gen_plan_set_arena_stride(void* plan, long long stride);
/* on != 0: the plan is ONE netG call on a batch of N <= 8 images (n_crops > 1: models/model.py:15, data/transforms.py:19-27):
 * BatchNorm statistics over the whole batch as nn.BatchNorm2d takes them; gradients summed over the images.  Default 0:
 * N separate batch-1 calls. */
int splice_gen_plan_set_batch_stats(void* plan, int on);
/* groups of images per netG call: images [k*g, (k+1)*g) are ONE call on a batch of g images (the n_crops crops of pair k) --
 * BatchNorm statistics over those g images, parameters / gradients at + k*stride (splice_gen_plan_set_arena_stride first when
 * there is more than one group).  Group k is bit-identical to a batch-statistics plan of g images on its images.  g = 1: N
 * independent images; g = N: splice_gen_plan_set_batch_stats.  Needs N % g == 0 and 1 <= g <= 8. */
int splice_gen_plan_set_groups(void* plan, int images_per_group);
/* re-target a plan to a smaller input without reallocating (per-step random crop sizes,
 * data/transforms.py:21-22) */
int splice_gen_plan_resize(void* plan, int H, int W);

/* ------------------------------------------------------------------ fused optimisation step
 * train.py:51-80 for P image pairs side by side (P = 1: the reference's one pair per process): Model.forward
 * (models/model.py:12-25), LossG.forward incl. its lambda schedule (util/losses.py:34-72), loss.backward(),
 * optimizer.step().  Built on a B = 4P ViT context [A'_0.. | B'_0.. | x'_0.. | y'_0..] (X' = T(X crop), x = G(A crop),
 * y = G(B crop)), two generator plans of P independent images (A crops, B crops) and, for the every-75th-step
 * entire-image branch, a B = 2P context and a third plan.  Pairs share only the frozen ViT; a pair's results do not
 * depend on P (bit-identical to its P = 1 run). */
typedef struct splice_step_config {
    int crop_h, crop_w;          /* (maximum) size of the global crops fed to G */
    int vit_h, vit_w;            /* after global_transform's Resize (== crop when it is the identity) */
    int ent_h, ent_w;            /* entire structure image (0 = branch disabled) */
    int ent_vit_h, ent_vit_w;    /* its size after Resize */
    float lambda_global_cls, lambda_global_ssim, lambda_global_identity, lambda_entire_cls, lambda_entire_ssim;
    int entire_every, cls_warmup;
    float lr, beta1, beta2, eps;
    int pairs;                   /* P (0 or 1: one pair) */
    long long arena_stride;      /* P > 1: floats between the pairs' parameter / gradient / Adam-moment arenas (>= param count);
                                  * the generator plans must have been given the same stride (splice_gen_plan_set_arena_stride) */
    int fp8_selfsim;             /* != 0: the key self-similarity Gram matrices on the fp8 MFMA (per-row e4m3 keys; dim % 128 == 0) */
    int top_cls_only;            /* != 0: the step switches its ViT contexts to splice_vit_ctx_set_top_cls_only (the Python engine's default;
                                  * results differ from the full top block by rounding only) */
    int n_crops;                 /* > 1: global_{A,B}_crops_n_crops of conf/default/config.yaml -- the step works on n_crops crops of
                                  * each pair: A_crop / B_crop are [pairs * n_crops][3][h][w] (pair-major), the generator plans hold
                                  * pairs * n_crops images in batch-statistics mode, one netG call per pair (one pair:
                                  * splice_gen_plan_set_batch_stats; several: splice_gen_plan_set_groups(n_crops) after the arena stride;
                                  * netG sees the stacked crops, data/transforms.py:27), each loss term is summed over a pair's crops
                                  * (util/losses.py:75-105), one arena per pair.  With pairs > 1: at most SPLICE_STEP_MAX_GROUP_IMAGES
                                  * images per side; the entire-image plan holds `pairs` independent images */
    int n_crops_b;               /* 0: global_B_crops_n_crops == n_crops.  > 0: the B-crop plan holds n_crops_b images and n_crops counts
                                  * the A crops only -- the reference zips the crop lists (util/losses.py:76,87,98): structure term over the
                                  * A crops, identity term over the B crops, appearance term over min(n_crops, n_crops_b) pairs */
} splice_step_config;
/* most pairs of one step handle that can carry a config of their own (splice_step_set_pair_weights / splice_step_set_pair_lr) */
#define SPLICE_STEP_MAX_PAIR_CFGS 32
/* most images per side (pairs * max(n_crops, n_crops_b)) of a step handle with pairs > 1 and n_crops > 1 */
#define SPLICE_STEP_MAX_GROUP_IMAGES 32
/* gen_plan_a / gen_plan_b: N = P plans at the crop size for the A and the B crops; gen_plan_entire: N = P at the entire size
 * (NULL with ent_h == 0).  Contexts: need_grad, B = 4P / 2P. */
int splice_step_create(const splice_step_config* cfg, void* vit_ctx_global, void* vit_ctx_entire, void* gen_plan_a, void* gen_plan_b,
                       void* gen_plan_entire, void** out_handle);
void splice_step_destroy(void* step);
/* params / grads / m / v: [P][arena_stride] (one flat arena for P = 1); A_crop, B_crop: [P][3][h][w] at the current crop
 * sizes; A_entire: [P][3][ent_h][ent_w] or NULL (needed when step_idx % entire_every == 0).
 * losses_out: device fp32 [P][8], per pair {loss, loss_global_ssim, loss_entire_ssim, loss_entire_cls, loss_global_cls,
 * loss_global_id_B, 0, 0} -- the keys of the dict LossG.forward returns (words 6-7: the two image-space terms on a handle with
 * splice_step_set_image_terms).  Written by the step's own loss kernel; the
 * captured hipGraph is bound to the arena pointers AND to losses_out, so keep passing the same buffers (a different
 * pointer re-captures; two consecutive steps with identical pointers and crop sizes are needed before a graph is used). */
int splice_step_run(void* step, float* params, float* grads, float* m, float* v, const float* A_crop, const float* B_crop,
                    const float* A_entire, int step_idx, float* losses_out, splice_stream_t stream);
/* generator outputs of the last step: which 0 x_global [P][3][a_h][a_w], 1 x_entire, 2 y_global */
int splice_step_output(void* step, int which, float** out_ptr);
/* graph bookkeeping of this handle: out[0] = captures that updated a retired executable in place (hipGraphExecUpdate; executables are pooled per
 * step configuration and never destroyed while the process runs), out[1] = updates the runtime refused, out[2] = executables instantiated */
int splice_step_graph_stats(void* step, long long* out);
/* 1 (default): capture the step's launch sequence once per regime into a hipGraph and replay it;
 * 0: launch every kernel eagerly (also used automatically while splice_prof_begin is armed) */
int splice_step_use_graph(void* step, int on);
/* 1 = the independent chains of a step (target passes beside the generator, the two ViT backward chains) run on two
 * streams (default), 0 = one stream; results are bit-identical either way */
int splice_step_use_overlap(void* step, int on);
/* per-step crop sizes (<= creation size) of the A and the B crops (the reference draws them independently,
 * data/Dataset.py:66-67); shared by all pairs of the batch */
int splice_step_set_crops(void* step, int a_h, int a_w, int b_h, int b_w);
/* skip_adam != 0: stop after backward -- `grads` = gradient of this step's loss (+= previous content when accumulate != 0),
 * parameters untouched; several losses (the same crops at several ViT input scales) are summed that way before ONE
 * splice_adam_step */
int splice_step_set_mode(void* step, int skip_adam, int accumulate);
/* The optimiser of the step's update: kind / hp0 / hp1 / eps as splice_optim_step (0 Adam, 1 RMSprop with v = square_avg,
 * 2 SGD).  Default: Adam with the config's beta1 / beta2 / eps.  A change drops the handle's captured graphs. */
int splice_step_set_optimizer(void* step, int kind, float hp0, float hp1, float eps);
/* Learning rate of the next splice_step_run and every later one until the next call (a schedule: the host calls it once per
 * step).  The value is staged by the step's input-staging launch (phase 1) and the update reads it from device memory, so a
 * replayed graph uses the lr of its own step.  Before the first call the handle uses the config's lr, as a kernel argument. */
int splice_step_set_lr(void* step, float lr);
/* Per-pair loss weights (pairs mode, P > 1; at most SPLICE_STEP_MAX_PAIR_CFGS pairs): lambdas = host [P][5], per pair
 * {lambda_global_cls, lambda_global_ssim, lambda_global_identity, lambda_entire_cls, lambda_entire_ssim}; they replace the config's
 * five lambdas.  The device scale tables are built once, here.  A term is launched when any pair's weight is > 0 (and its gate is
 * on: cls_warmup, the entire step); a pair whose weight is 0 writes no loss partials and no gradient for it and reports 0, as a
 * single-pair step that skips the launch.  Drops the handle's graphs. */
int splice_step_set_pair_weights(void* step, const float* lambdas);
/* Per-pair learning rates (pairs mode, P > 1): lr = host [P], the per-pair form of splice_step_set_lr (staged by the input-staging
 * launch, read by the optimiser from device memory: pair p's arena uses lr[p]).  The first call drops the handle's graphs. */
int splice_step_set_pair_lr(void* step, const float* lr);
/* Run part of a step: phases = mask of 1 generator forward (+ input staging), 2 ViT forward / losses / ViT backward down to
 * the gradient of the generated images, 4 generator backward (+ Adam unless splice_step_set_mode disables it); default 7.
 * leader != NULL (phases must be 2; another step handle with the same image shapes): this handle reads the leader's staged
 * inputs and generator outputs and ADDS its image gradients to the leader's.  The several-scales step (the reference has
 * one scale, util/losses.py:22-27; BASELINE configs[4] asks for three) is leader 1|2, followers 2, leader 4: one generator
 * pass per step whatever the number of scales. */
int splice_step_set_phases(void* step, int phases, void* leader);
/* BatchNorm running statistics of netG (models/unet/common.py:95-96, momentum 0.1): when `running` is set every step
 * applies the updates of its generator calls in the reference's order (A_global, A on entire steps, B_global) to the
 * caller's buffer arena(s): layout splice_gen_buffer_info, pair p at running + p * stride.  NULL = not tracked. */
int splice_step_set_running_stats(void* step, float* running, long long stride);

/* ------------------------------------------------------------------ plateau stop rule (an extension: the reference runs a fixed n_epochs,
 * train.py:51).  Per slot (pair) and in device memory: window means of the loss over `window` COUNTED steps (step_idx >= cls_warmup and
 * not an entire-image step -- the steps whose loss is composed alike).  A window is better when mean < best * (1 - rel); the slot stops
 * at the close of the `patience`-th consecutive window that is not better, if that step's index is >= min_steps.  A slot that stopped at
 * step k is FROZEN from step k + 1 on: its parameters, optimiser moments and BatchNorm running statistics are no longer written (its
 * work still rides in the launches, its reported losses are meaningless), and they equal, bit for bit, those of the same pair after
 * exactly k + 1 steps without the rule.  fp32, one rounding per operation. */
typedef struct splice_stop_state {
    float sum;        /* of the open window's losses */
    int count;        /* counted steps in the open window */
    int windows;      /* windows closed */
    float best;       /* best window mean so far (valid when windows > 0) */
    int bad;          /* consecutive closed windows that were not better */
    int stop_step;    /* step index the slot stopped at; -1 while it runs */
} splice_stop_state;
/* Switch the rule on for every pair of the handle (window > 0; 0 < rel < 1; patience >= 1; min_steps >= 0) or leave it off (window 0).
 * Before the first splice_step_run only; refused on a handle in gradient-only (splice_step_set_mode) or phase mode
 * (splice_step_set_phases), which the rule in turn bars.  The state starts as zeros with stop_step -1. */
int splice_step_set_stop_rule(void* step, int window, float rel, int patience, int min_steps);
/* copies the handle's [pairs] state records to host memory `out` (synchronises `stream`); all zero / -1 while the rule is off */
int splice_step_stop_state(void* step, splice_stop_state* out, splice_stream_t stream);
/* Start a handle at step next_step_idx of a run that other handles carried so far (a resumed run, a compacted engine): sets what a
 * handle keeps between steps -- whether the global structure and identity terms are on (next_step_idx > cls_warmup; only the run of
 * step cls_warmup itself switches them on) and the [pairs] stop records, copied from HOST memory `stop` (synchronises `stream`).
 * `stop` is given exactly when the handle has the stop rule.  Everything else that makes a pair continue (arenas, BatchNorm buffers,
 * the other rules' records) is the caller's memory.  After the rule setters, before the first splice_step_run. */
int splice_step_restore(void* step, int next_step_idx, const splice_stop_state* stop, splice_stream_t stream);
/* Gather form of the input staging: A_crop / B_crop / A_entire of splice_step_run then hold pairs_in pairs (pair-major, as the handle's
 * own layout), and pair p of the handle takes pair rows[p] of them -- its n_crops A crops, its B crops, its entire image -- in the one
 * staging launch, the table riding in its by-value arguments.  rows: host, strictly increasing, each < pairs_in; the handle's pairs
 * <= pairs_in <= SPLICE_STEP_MAX_PAIR_CFGS.  The staged buffers hold the bytes a flat copy of the gathered batches would: captured
 * graphs and everything downstream are unchanged.  rows NULL: off (the default). */
int splice_step_set_input_rows(void* step, int pairs_in, const int* rows);
/* The rule alone, as the step's loss kernel runs it: one step of `pairs` slots.  state: device [pairs] records (the caller starts them
 * as zeros with stop_step -1); losses8: device [pairs][8], element 0 of a row is the slot's loss; counted == 0: nothing happens. */
int splice_plateau_update(splice_stop_state* state, const float* losses8, int pairs, int window, float rel, int patience, int min_steps,
                          int step_idx, int counted, splice_stream_t stream);

/* ------------------------------------------------------------------ weight average (an extension: the reference writes the weights of its
 * last step).  ema: [P][arena_stride] like `params`, the caller's (it starts as a copy of the parameters); the step's optimiser launch
 * writes it by the rule of splice_optim_step_ema with the step's own count (step_idx + 1) -- no launch more, and params / m / v / losses
 * are what they are without it.  A slot frozen by the stop rule keeps the average of its stop step.  Before the first splice_step_run
 * only; refused on a handle in gradient-only (splice_step_set_mode) or phase mode (splice_step_set_phases), which the average in turn
 * bars.  0 < decay < 1, start >= 0. */
int splice_step_set_ema(void* step, float* ema, float decay, int start);
/* as splice_optim_step_pairs with the weight average `ema` ([n_pairs][stride] like params), in the form the fused step launches: the
 * step count is read from device memory (step_dev, one int >= 1; Adam's bias corrections are then computed on the device), and with
 * `stop` (may be NULL; device, [n_pairs] records) a pair that is frozen at step index *step_dev - 1 is skipped entirely: params, grads,
 * m, v and ema of that pair are not written. */
int splice_optim_step_pairs_ema(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, int n_pairs,
                                long long stride, long long n, const float* lr_dev, float hp0, float hp1, float eps, const int* step_dev,
                                const splice_stop_state* stop, int zero_grad, float ema_decay, int ema_start, splice_stream_t stream);

/* ------------------------------------------------------------------ gradient clipping by the global norm (an extension: the reference does
 * not clip).  torch.nn.utils.clip_grad_norm_(params, max_norm) per pair, plus a guard: a pair whose norm is not finite is not updated at
 * that step.  Per pair, over the n gradient floats of its arena (s = fl(g + g2) where a second gradient arena is folded in), fp32 with one
 * rounding per operation unless noted:
 *   stage 1, one partial per chunk of SPLICE_CLIP_CHUNK floats counted from the start of the pair's arena: element e of a chunk belongs to
 *     thread t = (e / 4) % 256, round j = e / 1024, component c = e % 4; thread t adds fl(s * s) to acc = 0 in the order j = 0..3, c = 0..3
 *     (elements at or beyond n add nothing); the 256 values are combined by the halving tree a[t] += a[t + off], off = 128, 64, ..., 1.
 *   stage 2, per pair: thread t of 256 adds partials[t], partials[t + 256], ... in fp64, the same tree in fp64 combines the threads;
 *     sumsq = (float)total, norm = sqrtf(sumsq); norm finite: coef = fminf(1, max_norm / (norm + 1e-6f)), skip = 0, clipped += coef < 1;
 *     otherwise coef = 0, skip = 1, skipped += 1.
 * The update then uses fl(s * coef) as its gradient -- multiplied even when coef is 1, as torch does, which changes no bit -- and with
 * skip set writes nothing of the pair but the zeros of zero_grad.  The bits of a pair do not depend on the other pairs of the call. */
#define SPLICE_CLIP_CHUNK 4096
typedef struct splice_clip_state {
    float sumsq;      /* of the pair's gradient at the last step */
    float norm;       /* sqrtf(sumsq) */
    float coef;       /* the factor the update multiplied the gradient by (0 with skip) */
    int skip;         /* the last step's norm was not finite: the pair was not updated */
    int clipped;      /* steps so far with coef < 1 */
    int skipped;      /* steps so far with skip */
} splice_clip_state;
/* The two norm stages for n_pairs arenas of n floats, pair p at grads + p * stride (g2 alike; may be NULL).  partials: device,
 * n_pairs * ceil(n / SPLICE_CLIP_CHUNK) floats, the caller's scratch; state: device, [n_pairs] records (the caller starts the two counts
 * at zero).  n_pairs == 1: the stride is not used and n is arbitrary; otherwise stride % 4 == 0 and stride >= n.  An arena that is not
 * 16-byte aligned is read element by element, with the same result.  stop (may be NULL; device, [n_pairs] records) with step_dev (device,
 * one int, step index + 1): a pair frozen at that step is left out, its record stays.  0 < max_norm < inf. */
int splice_grad_norm_pairs(const float* grads, const float* g2, int n_pairs, long long stride, long long n, float max_norm, float* partials,
                           splice_clip_state* state, const splice_stop_state* stop, const int* step_dev, splice_stream_t stream);
/* as splice_optim_step_pairs_ema with the records splice_grad_norm_pairs has just written for the same gradient (clip: device, [n_pairs]):
 * pair p's gradient is fl(fl(g + g2) * clip[p].coef), and a pair with clip[p].skip set is not written (its grads are zeroed when zero_grad
 * is set).  Where grads is written back (g2 or zero_grad) it holds the clipped sum.  ema may be NULL (no average) and stop may be NULL;
 * n_pairs == 1: the stride is not used and n is arbitrary, lr_dev[0] is the learning rate. */
int splice_optim_step_pairs_clip(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, int n_pairs,
                                 long long stride, long long n, const float* lr_dev, float hp0, float hp1, float eps, const int* step_dev,
                                 const splice_stop_state* stop, int zero_grad, float ema_decay, int ema_start, const splice_clip_state* clip,
                                 splice_stream_t stream);
/* the host-step form for one arena of n floats (as splice_optim_step_ema, ema optional): lr / lr_dev and step as in splice_optim_step_ex,
 * clip: the one record splice_grad_norm_pairs wrote for this gradient with n_pairs == 1 */
int splice_optim_step_clip(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, long long n, float lr,
                           const float* lr_dev, float hp0, float hp1, float eps, int step, int zero_grad, float ema_decay, int ema_start,
                           const splice_clip_state* clip, splice_stream_t stream);
/* Clip every pair's gradient inside the step: the two norm launches go out on the main stream directly before the optimiser launch, which
 * then reads the records.  state: device, [pairs] records, the caller's (zeros).  The handle owns the partials.  With max_norm so large
 * that no step is clipped, params / m / v / ema / losses are, bit for bit, what they are without the rule.  A slot frozen by the stop rule
 * keeps the record of its stop step.  Before the first splice_step_run only; refused on a handle in gradient-only (splice_step_set_mode)
 * or phase mode (splice_step_set_phases), which the rule in turn bars.  0 < max_norm < inf. */
int splice_step_set_grad_clip(void* step, float max_norm, splice_clip_state* state);

/* ------------------------------------------------------------------ gradient clipping against the pair's own running norm (DESIGN.md section
 * 9h; an extension of the clipping above).  The threshold is k times a running mean of the pair's gradient norm, kept per pair and per
 * REGIME of the step -- regime 1: an entire-image step, 0: any other step from cls_warmup on, -1: a step before cls_warmup, which is
 * observed by neither reference and clipped by the absolute cap alone -- in a second record beside splice_clip_state.  Stages 1 and 2
 * of the norm are those above; then thread 0 of the pair's workgroup does (fp32, one rounding per operation, r = regime):
 *   thr_auto = (r >= 0 && count[r] >= warmup && ref[r] > 0) ? k * ref[r] : +inf
 *   thr      = max_norm > 0 ? fminf(max_norm, thr_auto) : thr_auto
 *   norm finite:  coef = fminf(1, thr / (norm + 1e-6f)), skip = 0, clipped += coef < 1; and if r >= 0:
 *                   x = fminf(norm, thr_auto)          (a spike raises the reference by at most the factor k)
 *                   ref[r] = count[r] == 0 ? x : beta * ref[r] + (1 - beta) * x;  count[r] += 1
 *   otherwise:    coef = 0, skip = 1, skipped += 1     (ref and count do not move)
 *   thr and regime of the record = thr, r
 * The splice_clip_state record keeps its meaning, and the update reads coef / skip from it as above. */
typedef struct splice_clip_auto_state {
    float ref[2];     /* running gradient norm of regime 0 (ordinary steps) and 1 (entire-image steps) */
    int count[2];     /* steps of either regime observed so far (steps with a non-finite norm are not) */
    float thr;        /* the last step's threshold; +inf: none */
    int regime;       /* the last step's regime: -1, 0 or 1 */
} splice_clip_auto_state;
/* as splice_grad_norm_pairs with the rule above: auto_state: device, [n_pairs] records (zeros at the start of a run).  max_norm: the
 * absolute cap, finite and >= 0 (0: none); k finite and >= 1; 0 <= beta < 1; warmup >= 1; regime -1, 0 or 1.  A pair frozen at the
 * step (stop / step_dev) keeps both records. */
int splice_grad_norm_pairs_auto(const float* grads, const float* g2, int n_pairs, long long stride, long long n, float max_norm, float k,
                                float beta, int warmup, int regime, float* partials, splice_clip_state* state,
                                splice_clip_auto_state* auto_state, const splice_stop_state* stop, const int* step_dev,
                                splice_stream_t stream);
/* Clip every pair's gradient inside the step by the rule above, the alternative to splice_step_set_grad_clip (a handle takes one of the
 * two): the same two norm launches, the second one in its instance with the rule; the regime is fixed per launch sequence (graph
 * variant) of the step, as "counted" is for the stop rule.  state, auto_state: device, [pairs] records each, the caller's (zeros).  No
 * launch, event or graph node more than splice_step_set_grad_clip has.  A slot frozen by the stop rule keeps both records of its stop
 * step.  Before the first splice_step_run only; refused on a handle in gradient-only (splice_step_set_mode) or phase mode
 * (splice_step_set_phases), which the rule in turn bars.  Arguments as splice_grad_norm_pairs_auto. */
int splice_step_set_grad_clip_auto(void* step, float max_norm, float k, float beta, int warmup, splice_clip_state* state,
                                   splice_clip_auto_state* auto_state);

/* ------------------------------------------------------------------ keep the best window's weights (an extension of the stop rule).  A slot
 * stops `patience` windows behind the window the rule judged best, so the weights it is frozen with are not those the rule liked.  While
 * a slot is LIVE at a counted step -- its stop_step < 0 on entry to the rule -- the rule also writes, at the close of a window:
 *   best_step = that step's index and best_window = the window's index (`windows` before its increment), where it sets best = mean
 *     (the first window, or mean < best * (1 - rel));
 *   means[windows before the increment] = mean, for the first SPLICE_STOP_HISTORY windows.
 * After its stop the slot's splice_stop_state goes on evolving as it always did; the record and the history no longer move.  The update
 * of the step whose index equals best_step then copies the parameter it has just written (and the average, where one is kept) into the
 * caller's best arena: no float is computed again, the snapshot holds the bits of params / ema after that step.  best_mean is
 * means[best_window], and stop_state.best while the slot is live. */
#define SPLICE_STOP_HISTORY 64
typedef struct splice_best_state {
    int best_step;    /* index of the step that closed the best window so far; -1 until a window has closed */
    int best_window;  /* index of that window; -1 alike */
} splice_best_state;
/* splice_plateau_update with the record and the history: best: device [pairs] records (the caller starts them as -1 / -1), means: device
 * [pairs][SPLICE_STOP_HISTORY] floats (zeros).  The state is, bit for bit, that of splice_plateau_update. */
int splice_plateau_update_best(splice_stop_state* state, splice_best_state* best, float* means, const float* losses8, int pairs, int window,
                               float rel, int patience, int min_steps, int step_idx, int counted, splice_stream_t stream);
/* as splice_optim_step_pairs_clip -- stop is required here, clip and ema may be NULL -- with the snapshot: a pair that is not frozen and
 * whose best[p].best_step equals the step index *step_dev - 1 has the params just written copied to best_params, and its ema to best_ema
 * (both laid out like params; best_ema is given exactly when ema is).  A pair whose clip record has skip set still takes the snapshot, of
 * its unchanged params / ema.  Nothing else of best_params / best_ema is written; params, grads, m, v and ema are those of
 * splice_optim_step_pairs_clip. */
int splice_optim_step_pairs_best(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* ema, int n_pairs,
                                 long long stride, long long n, const float* lr_dev, float hp0, float hp1, float eps, const int* step_dev,
                                 const splice_stop_state* stop, int zero_grad, float ema_decay, int ema_start, const splice_clip_state* clip,
                                 const splice_best_state* best, float* best_params, float* best_ema, splice_stream_t stream);
/* The extended rules (splice_optim_ext above) for n_pairs arenas with per-pair learning rates, every optional part of the update beside
 * them: w ([n_pairs][stride] like m and v; NULL where the rule keeps none), step_dev (NULL: the host's `step` counts the update), stop
 * (needs step_dev), ema, clip, best with best_params and best_ema (needs stop), as splice_optim_step_pairs_best takes them.  One pair:
 * a single arena of n floats.  Bit for bit n_pairs single-arena calls with each pair's lr. */
int splice_optim_step_pairs_ext(int kind, float* params, float* grads, const float* g2, float* m, float* v, float* w, float* ema, int n_pairs,
                                long long stride, long long n, const float* lr_dev, float hp0, float hp1, float eps, int step,
                                const int* step_dev, const splice_stop_state* stop, int zero_grad, float ema_decay, int ema_start,
                                const splice_clip_state* clip, const splice_best_state* best, float* best_params, float* best_ema,
                                const splice_optim_ext* options, splice_stream_t stream);
/* The extended rules inside the step: the update of every later splice_step_run runs the extended rule of the handle's kind
 * (splice_step_set_optimizer, called first) under `options`, with w ([P][arena_stride] like m, the caller's, zeros at the start of a
 * run; NULL unless amsgrad / centered) -- no launch more.  The m arena of splice_step_run then also holds the momentum buffer.  Before
 * the first splice_step_run only; drops the handle's graphs, as splice_step_set_optimizer does. */
int splice_step_set_optimizer_ext(void* step, const splice_optim_ext* options, float* w);
/* Keep every pair's best-window weights inside the step: the loss kernel's rule writes `state` and `means` (device, the caller's: [pairs]
 * records at -1 / -1 and [pairs][SPLICE_STOP_HISTORY] zeros), the optimiser launch of the same step reads the record and writes
 * best_params (and best_ema; both [P][arena_stride] like params, the caller's, they start as copies of params / ema).  No launch more,
 * and params / m / v / ema / losses are what they are without it.  Before the first splice_step_run only, on a handle that has a stop
 * rule (splice_step_set_stop_rule with window > 0), with best_ema given exactly when the handle keeps an average (splice_step_set_ema
 * comes first); refused on a handle in gradient-only (splice_step_set_mode) or phase mode (splice_step_set_phases), which it in turn
 * bars. */
int splice_step_set_keep_best(void* step, float* best_params, float* best_ema, splice_best_state* state, float* means);

/* ------------------------------------------------------------------ the per-step loss trace: a loss curve of every pair
 * without a device-to-host copy per step.  trace: device, the caller's, [capacity][pairs][8] floats (the caller fills it, e.g. with NaN,
 * to tell written rows from others).  The step with index s < capacity writes row s of pair p, at trace + (s * pairs + p) * 8:
 *   words 0-5   the six values the step's loss kernel writes into losses_out[p][0..5] (splice_step_run), with the same bits, stored
 *               by that kernel;
 *   words 6-7   the pair's gradient norm and clip coefficient of the step (splice_clip_state norm / coef), stored by the norm launch
 *               of a handle with gradient clipping (splice_step_set_grad_clip or splice_step_set_grad_clip_auto); without it they
 *               are not written.
 * A step with s >= capacity writes nothing and is no error.  A pair frozen by the stop rule is not written behind its stop step: row
 * stop_step is its last.  The row index is read from the step count on the device, so a replayed graph writes its own step's row.  No
 * launch, event or graph node more, and params / m / v / ema / best arenas / rule records / losses are what they are without it.
 * Before the first splice_step_run only; refused on a handle in gradient-only (splice_step_set_mode) or phase mode
 * (splice_step_set_phases), which it in turn bars. */
int splice_step_set_loss_trace(void* step, float* trace, int capacity);

/* ------------------------------------------------------------------ the plateau lr rule (an extension of the stop rule):
 * cut a slot's learning rate where the stop rule's windows stop getting better.  It uses that rule's windows, its `rel` and its verdict
 * on every window (the first window counts as better), and leaves its state as it is without the lr rule: a cut does not reset the stop
 * rule's `bad`, and min_steps does not gate cuts.  Per slot a record and a row cut_steps[SPLICE_STOP_HISTORY] of step indices.  Every
 * step, counted or not, thread 0 of the slot's loss-kernel workgroup does, in this order (fp32, one rounding per operation):
 *   lr_eff[slot] = lr_in[slot] * scale       with the scale as it stands before this step's rule: a cut made at step t first acts on
 *                                            the update of step t + 1, as a host loop that calls its scheduler behind optimizer.step();
 *   on a counted step that closes a window, and only if the slot is live on entry (stop_step < 0):
 *     better:  bad = 0
 *     else:    bad += 1; then if bad >= patience && scale > min_scale && cuts < SPLICE_STOP_HISTORY:
 *              scale = max(fl(scale * factor), min_scale); cut_steps[cuts] = step index; cuts += 1; last_cut_step = step index; bad = 0.
 * The record of a slot that stopped is never written again.  This is torch.optim.lr_scheduler.ReduceLROnPlateau(mode='min', factor,
 * patience = patience - 1, threshold = rel, threshold_mode='rel', cooldown=0) fed the window means, but for the cap of
 * SPLICE_STOP_HISTORY cuts and the floor, which is a scale (min_scale) and no learning rate. */
typedef struct splice_lr_state {
    float scale;        /* what the next update's learning rate is multiplied by; starts as 1 */
    int bad;            /* consecutive closed windows that were not better since the last cut; starts as 0 */
    int cuts;           /* cuts so far (at most SPLICE_STOP_HISTORY); starts as 0 */
    int last_cut_step;  /* step index of the last cut; -1 until the first */
} splice_lr_state;
/* Switch the rule on for every pair of the handle: 0 < factor < 1, patience >= 1 (windows), 0 <= min_scale < 1.  state: device, [pairs]
 * records, the caller's ({1, 0, 0, -1} each); cut_steps: device, [pairs][SPLICE_STOP_HISTORY] ints, the caller's (-1).  The step's loss
 * kernel writes both and lr_eff, a [pairs] table the handle owns; the optimiser launch of the same step -- always behind the loss
 * kernel -- reads its learning rate(s) there through the device-lr paths it has (one arena: lr_dev; several: lr_dev[element /
 * arena_stride], so the stride must be a multiple of 4).  lr_in is what the step stages anyway: the table of splice_step_set_pair_lr,
 * else the one value of splice_step_set_lr, else -- neither called -- the config's lr, which the handle then stages itself.  No launch,
 * event or graph node more; while no cut has happened params / m / v / ema / best arenas / rule records / losses / trace are, bit for
 * bit, what they are without the rule.  Before the first splice_step_run only, on a handle that has a stop rule
 * (splice_step_set_stop_rule with window > 0); refused on a handle in gradient-only (splice_step_set_mode) or phase mode
 * (splice_step_set_phases), which the stop rule in turn bars. */
int splice_step_set_lr_plateau(void* step, float factor, int patience, float min_scale, splice_lr_state* state, int* cut_steps);
/* The stop rule with the lr rule, as the step's loss kernel runs them (the same device function): one step of `pairs` slots.  state,
 * losses8, window .. min_steps, step_idx, counted: as splice_plateau_update, and the state records are, bit for bit, what that call
 * leaves.  lr_state / cut_steps: device, as splice_step_set_lr_plateau takes them.  lr_in: device, one float (per_pair == 0) or [pairs]
 * floats; lr_eff: device, [pairs], written at every call, counted or not. */
int splice_plateau_update_lr(splice_stop_state* state, splice_lr_state* lr_state, int* cut_steps, const float* losses8, const float* lr_in,
                             int per_pair, float* lr_eff, int pairs, int window, float rel, int patience, int min_steps, float factor,
                             int lr_patience, float min_scale, int step_idx, int counted, splice_stream_t stream);

/* ------------------------------------------------------------------ test hooks: the loss stage as the fused step launches it.  The three
 * entry points below call the step's own launchers (structure term, batched MSE, total) on the caller's buffers with the step's operand
 * layout; they add no kernel and no code path (tests/test_loss_stage_gpu.py against oracle/loss_stage.py).
 *
 * Structure term of `pairs` problems (util/losses.py:74-83): pair p's partials and key gradient of
 *     lambda * mean((cos-sim(k_x[p]) - cos-sim(k_tgt[p]))^2)         (attn_cosine_sim, models/extractor.py:4-9; both [T][D] keys)
 *   k_tgt, k_x   bf16 [T][ldk] (D columns used), pair p at + p * k_pstride elements.  Rows >= T are never read.
 *   kT_x         the transpose of k_x: bf16 [D][ldt], pair p at + p * kT_pstride elements (column t of pair p = token t).  The kernels read
 *                it Tp = roundup(T, 64) columns wide per pair -- in the step's layout the columns past a pair's own are its padding, the
 *                next pair's tokens or, for the last pair, the start of the next row -- and multiply what lies at columns >= T by exact
 *                zeros: that memory must be READABLE and FINITE (an Inf or NaN there reaches every element of the pair's gradient).
 *   lambda, e_scale_tab   loss_scale = 1 / ((float)T * (float)T) and e_scale = 4.0f * lambda * loss_scale, fp32, as the step forms them.
 *                e_scale_tab (may be NULL; device, [pairs]) replaces e_scale per pair; a pair whose entry is 0 writes nothing at all.
 *   fp8          != 0: both Gram matrices on the fp8 MFMA from per-row quantised keys; needs D % 128 == 0.  W and r use the true norms.
 *   loss_part    pair p's per-tile partials at + p * part_pstride: slot t of the nt (nt + 1) / 2 upper-triangular 64 x 64 tiles, nt = Tp / 64
 *                (row-major over tm <= tn), holds that tile's share of mean((S - S*)^2) -- an off-diagonal tile counted twice -- WITHOUT
 *                lambda; the caller adds the slots.  Slots beyond the tile count are not written.
 *   dk           fp32, pair p at + p * dk_pstride, [T][lddk]: rows < T and columns < D are overwritten (not accumulated) with
 *                dK = W K - diag(r) K,  W_ij = e_ij / max(n_i n_j, eps),  r_i = sum_j [n_i n_j > eps] e_ij S_ij / max(n_i^2, 1e-30),
 *                e = e_scale (S - S*), W rounded to bf16.  An all-zero key row i has S_ij = 0, is gated out of r by eps (r_i = 0) and gets what
 *                autograd gives it, dK_i = sum_j e_ij K_j / eps; its own terms in the other rows' gradients vanish with K_i.
 *   ws           splice_selfsim_loss_pairs_ws_bytes(T, D, pairs) bytes, 256-byte aligned.
 * Refused with SPLICE_ERR_ARG before anything is launched: a NULL operand, T / pairs < 1, D % 64, fp8 with D % 128, ldk % 8, ldt % 8,
 * k_pstride % 8 or kT_pstride % 8 (16-byte loads), part_pstride < nt (nt + 1) / 2, lddk < D. */
size_t splice_selfsim_loss_pairs_ws_bytes(int T, int D, int pairs);
int splice_selfsim_loss_pairs(const splice_bf16* k_tgt, const splice_bf16* k_x, int ldk, size_t k_pstride, const splice_bf16* kT_x, int ldt,
                              size_t kT_pstride, int T, int D, int pairs, float lambda, const float* e_scale_tab, int fp8, float eps,
                              float* loss_part, size_t part_pstride, float* dk, int lddk, size_t dk_pstride, void* ws, splice_stream_t stream);
/* The batched strided MSE of the step ([CLS] and key-identity terms): for pair p, on a + p * a_ps ([rows][lda], cols used) and b + p * b_ps,
 *   part[p * part_ps + w] = loss_weight / (rows * cols) * (sum of (a - b)^2 over workgroup w's elements), w < min(ceil(rows * cols / 256), 1024)
 *   (workgroup w owns the flat elements i with (i / 256) % workgroups == w); other slots are not written;
 *   grad (may be NULL; pair p at + p * g_ps, [rows][ldg]) = 2 * gmean * (a - b) with gmean = grad_weight / (rows * cols) or, with grad_tab
 *   (may be NULL; device, [pairs]), gmean = grad_tab[p]; a pair whose entry is 0 writes neither partials nor gradient. */
int splice_mse_pairs(const float* a, int lda, size_t a_ps, const float* b, int ldb, size_t b_ps, int rows, int cols, float loss_weight,
                     float grad_weight, float* part, size_t part_ps, float* grad, int ldg, size_t g_ps, int pairs, const float* grad_tab,
                     splice_stream_t stream);
/* The step's total-loss launch (without the stop rule) on a caller's partials buffer.  lbase holds slots of lstride floats each; a slot
 * is [8 values][term 0..5: lp partials each], i.e. term k's partials of a slot start at 8 + k * lp (k: 1 global structure, 2 entire
 * structure, 3 entire [CLS], 4 global [CLS], 5 global identity; lstride >= 8 + 6 * lp).  Pair p's slots of a term are the n consecutive
 * slots from p * n, with n = n_a (term 1), n_b (term 5), n_c (term 4), n_e (terms 2 and 3); raw_k = the slots' fixed-order sums added in
 * slot order.  Written: slot p's values [0..5] = {total, raw_1..raw_5} and, when out8 is given, out8[p][0..7] = {total, raw_1..raw_5, 0, 0};
 * total = w_ssim raw_1 + w_essim raw_2 + w_ecls raw_3 + w_cls raw_4 + w_id raw_5, added left to right -- as one product and four fused
 * multiply-adds, fma(w_id, raw_5, fma(w_cls, raw_4, fma(w_ecls, raw_3, fma(w_ssim, raw_1, w_essim raw_2)))), in every instance.  wtab (may be NULL; device,
 * [pairs][5] = {cls, ssim, id, ecls, essim}) replaces the five weights per pair: ssim and id are taken as 0 unless ssim_on, ecls and
 * essim as 0 unless entire. */
int splice_total_loss_pairs(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls, float w_id,
                            float* out8, int pairs, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on, int entire,
                            splice_stream_t stream);
/* ------------------------------------------------------------------ the image-space loss terms: two regularisers on the
 * generator's outputs at the crops' own resolution, beside the five terms seen through the ViT.  Per pair, fp32 images [3][h][w]:
 *   loss_global_tv        sum over the pair's A crops of TV(x'_i), x' = G(A_crop):
 *                           TV(x) = mean |x[:,1:,:] - x[:,:-1,:]| + mean |x[:,:,1:] - x[:,:,:-1]|,
 *                         each mean over its own count 3 (h - 1) w / 3 h (w - 1); a direction without differences contributes 0.  The
 *                         derivative takes sign(0) = 0, the sign being that of the fp32 difference of the two fp32 pixels.
 *   loss_global_pix_id_B  sum over the pair's B crops of mean((y'_i - B_crop_i)^2) over 3 h w, y' = G(B_crop), B_crop the staged input;
 *                         gradient 2 (y' - B_crop) / (3 h w).
 * Both act on every step from step 0 (cls_warmup does not gate them, entire-image steps change nothing; the entire-image output G(A) gets
 * neither).  The raw values are words 6 and 7 of the pair's losses_out row; the total becomes
 *   fma(lambda_pix, raw_7, fma(lambda_tv, raw_6, total of the five terms)),
 * so the stop rule, the plateau lr rule, keep-best and word 0 of a trace row see it.  Trace words 6-7 stay the clip norm and coefficient:
 * the two raw values are not traced.  The weights are shared by all pairs of the handle (splice_step_set_pair_weights has no column for
 * them).  Launches added with a weight > 0: one value launch at the loss stage (both terms), one gradient-add launch on that term's
 * backward chain between the un-resize of the ViT's image gradient and the generator backward; the loss kernel runs its IMG instance
 * (448 threads).  With both 0 the handle launches what it launches without the call.  Accepted before the first splice_step_run only;
 * refused: a negative or non-finite weight, a handle in gradient-only (splice_step_set_mode) or phase mode or with a leader
 * (splice_step_set_phases) -- a follower adds its image gradients into its leader's, which would count the terms once per follower --
 * and such a handle in turn refuses those two calls. */
int splice_step_set_image_terms(void* step, float lambda_tv, float lambda_pix);
/* test hook: the step's value launch on caller buffers.  x ([n_x][3][xh][xw]; NULL: TV off) and y, b ([n_y][3][yh][yw]; y NULL: pixel
 * identity off) are the images; lbase is a partials buffer in the layout of splice_total_loss_pairs with lstride >= 8 + 8 * lp, zeroed
 * by the caller.  Image i's chunk c (SPLICE_IMAGE_TERMS_CHUNK consecutive floats of the image, counted from its start) writes
 * lbase[i * lstride + 8 + k * lp + c], k = 6 (TV: chunk's vertical addends / (3 (h - 1) w) + its horizontal addends / (3 h (w - 1)),
 * a pixel's addends being those with its lower and its right neighbour) or 7 (sum of squared differences / (3 h w)); the other slots are
 * not written.  Refused before anything is launched: a missing operand, a size < 1, more than lp chunks per image. */
#define SPLICE_IMAGE_TERMS_CHUNK 4096
int splice_image_terms_value(const float* x, int n_x, int xh, int xw, const float* y, const float* b, int n_y, int yh, int yw, float* lbase,
                             size_t lstride, int lp, splice_stream_t stream);
/* test hook: the step's gradient-add launch: d[n_img][3][h][w] += lambda * dTV/dx(x) (b NULL) or += lambda * 2 (x - b) / (3 h w) (b
 * given), in place; the term's gradient is formed in double and rounded to fp32 once before the add.  lambda finite, >= 0. */
int splice_image_terms_grad_add(const float* x, const float* b, float* d, int n_img, int h, int w, float lambda, splice_stream_t stream);
/* test hook: splice_total_loss_pairs as a handle with image-space terms launches it (the IMG instance): terms 6 (n_a slots per pair) and
 * 7 (n_b slots) of the partials are summed as the others, slot p's values [6..7] and out8[p][6..7] receive raw_6 and raw_7, and
 * total = fma(w_pix, raw_7, fma(w_tv, raw_6, the total of splice_total_loss_pairs)).  lstride >= 8 + 8 * lp. */
int splice_total_loss_pairs_img(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls, float w_id,
                                float* out8, int pairs, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on, int entire,
                                float w_tv, float w_pix, splice_stream_t stream);
/* ------------------------------------------------------------------ the structure loss over the keys of several ViT blocks (DESIGN.md section
 * 9k).  With n ascending distinct block indices `layers` in [0, depth) and n finite weights > 0, every structure term of the step -- the
 * global one on every A crop, the entire-image one -- becomes
 *     raw = sum over i ascending of weights[i] * mean((cos-sim(keys of block layers[i] of the generated image) - the target's)^2),
 * reported as word 1 / 2 of the losses row and multiplied by the term's lambda in the total as before.  The key-identity term and both
 * [CLS] terms stay on the top block.  The layers ride in the three self-similarity launches a term has (grid z = layer); block i's
 * tile partials are slots [i tiles, (i + 1) tiles) of the term's partial row, tiles = nt (nt + 1) / 2, nt = ceil(T / 64).  Before the first
 * splice_step_run only; refused on a handle in gradient-only or phase mode or with a leader (which in turn refuses those calls), with
 * fp8_selfsim, and a second time.  A handle without the call launches what it always did. */
int splice_step_set_ssim_layers(void* step, int n, const int* layers, const float* weights);
/* The per-layer addends of word `term` (1: loss_global_ssim, 2: loss_entire_ssim) of the last step: out (device, [n][pairs]),
 * out[i * pairs + p] = pair p's sum of block i's slot range, the slots added in order (a pair's crops in crop order) -- weights[i] times the
 * block's mean squared difference.  With one crop per pair the reported word is their float32 sum over i ascending, exactly. */
int splice_step_ssim_layer_values(void* step, int term, float* out, splice_stream_t stream);
/* test hook: splice_selfsim_loss_pairs with the step's layer table: n_layers problems per pair in the same three launches.  k_tgt, k_x,
 * kT_x, dk, ws: host arrays of n_layers device pointers, each as the single-layer call takes it (ws[i]:
 * splice_selfsim_loss_pairs_ws_bytes(T, D, pairs) bytes of its own); the leading dimensions and pair strides are shared.  weights[i]
 * (host; finite, > 0) multiplies loss_scale and e_scale (or the pair's e_scale_tab entry) of layer i, one fp32 product each.  Layer i
 * writes slots [i tiles, (i + 1) tiles) of pair p's row of loss_part (part_pstride >= n_layers * tiles) and dk[i]; both have the bits of
 * the layer's own n_layers = 1 call, and with weight 1 those of splice_selfsim_loss_pairs.  bf16 only.  Refusals as there, before
 * anything is launched. */
int splice_selfsim_loss_layers(int n_layers, const splice_bf16* const* k_tgt, const splice_bf16* const* k_x, const splice_bf16* const* kT_x,
                               const float* weights, int ldk, size_t k_pstride, int ldt, size_t kT_pstride, int T, int D, int pairs, float lambda,
                               const float* e_scale_tab, float eps, float* loss_part, size_t part_pstride, float* const* dk, int lddk,
                               size_t dk_pstride, void* const* ws, splice_stream_t stream);
/* ------------------------------------------------------------------ the [CLS] appearance loss over several ViT blocks.
 * With n ascending distinct block indices `layers` in [0, depth) and n finite weights > 0, both appearance terms of the step -- the global
 * one on every (x', B') crop pair, the entire-image one -- become
 *     raw = sum over i ascending of weights[i] * mean((row 0 of block layers[i]'s output of the generated image - the target's)^2),
 * reported as word 4 / 3 of the losses row and multiplied by the term's lambda in the total as before.  One launch per term covers every
 * named block; a block below the top hands its gradient to the ViT backward as one seed row per pass (splice_vit_ctx_set_cls_seeds), the
 * top block through the [CLS]-only tail as always.  The top block need not be named.  Before the first splice_step_run only; refused on
 * a handle in gradient-only or phase mode or with a leader (which in turn refuses those calls), with fp8_selfsim, and a second time.  A
 * handle without the call launches what it always did. */
int splice_step_set_cls_layers(void* step, int n, const int* layers, const float* weights);
/* The per-layer addends of the appearance term (entire 0: loss_global_cls; else: loss_entire_cls) of the last step that computed it,
 * copied to the host behind a device-wide wait: out[s * n + i] = slot s's weights[i] times block i's mean squared [CLS] difference; the
 * slots are the pairs (entire, or one crop per pair), else the pairs * min(nA, nB) pair-crops, pair-major.  cap: the floats out holds
 * (>= slots * n).  A slot's partial -- with one crop per pair the reported word -- is the float32 sum of its row, ascending, exactly; a
 * slot that never took part reads 0. */
int splice_step_cls_layer_values(void* step, int entire, float* out, int cap);
/* test hook: the layered launch of the step on caller buffers.  x, tgt, seeds: host arrays of n_layers (1..12) device pointers -- the
 * first slot's row of D floats on the generated side, on the target side, and of the layer's seed buffer; slot s is x_pstride / t_pstride
 * / seed_pstride (>= D) floats further on.  weights: host, finite, > 0.  For slot s and layer i, with g = lambda / (float)D or
 * grad_tab[s] (may be NULL; device, [slots]; a slot whose entry is 0 writes nothing):
 *   values[s * n_layers + i] = (sum of d^2 over the D columns, a fixed tree) * (weights[i] / (float)D),   d = x - tgt
 *   seeds[i][s * seed_pstride + c] = 2 * (g * weights[i]) * d[c]
 *   part[s * part_pstride]  = the float32 sum of the slot's values, ascending from 0 (no other slot of part is written).
 * Layer i has the bits of its own n_layers = 1 call.  Refusals launch nothing. */
int splice_cls_loss_layers(int n_layers, const float* const* x, const float* const* tgt, const float* weights, size_t x_pstride, size_t t_pstride,
                           int D, int slots, float lambda, const float* grad_tab, float* part, size_t part_pstride, float* const* seeds,
                           size_t seed_pstride, float* values, splice_stream_t stream);
/* ------------------------------------------------------------------ the key-identity loss over several ViT blocks.
 * With n ascending distinct block indices `layers` in [0, depth) and n finite weights > 0, the identity term of the step -- on every
 * (y', B') crop pair, from cls_warmup on -- becomes
 *     raw = sum over i ascending of weights[i] * mean((keys of block layers[i] of the generated crop - the target's)^2),
 * keys = the key columns of the block's raw qkv in fp32, T * D values; reported as word 5 of the losses row and multiplied by
 * lambda_global_identity (or the slot's own) in the total as before.  Two launches cover every named block; the key gradients reach the ViT
 * backward of the y' chain where it always took them (d_keys[l]), the x' and entire-image chains launch what they launched.  The top block
 * need not be named.  Before the first splice_step_run only, and behind splice_step_set_ssim_layers where both are called; refused on a
 * handle in gradient-only or phase mode or with a leader (which in turn refuses those calls), with fp8_selfsim, and a second time.  A
 * handle without the call launches what it always did. */
int splice_step_set_id_layers(void* step, int n, const int* layers, const float* weights);
/* The per-layer addends of the identity term of the last step that computed it, copied to the host behind a device-wide wait:
 * out[s * n + i] = slot s's weights[i] times block i's mean squared key difference; the slots are the B crops, pairs * nB in pair-major
 * order.  cap: the floats out holds (>= slots * n).  A slot's partial -- with one crop per pair the reported word -- is the float32 sum
 * of its row, ascending, exactly; a slot that never took part reads 0. */
int splice_step_id_layer_values(void* step, float* out, int cap);
/* test hook: the two layered launches of the step on caller buffers.  x, tgt, grad: host arrays of n_layers (1..12) device pointers -- the
 * first slot's T x D keys on the generated side (rows ldx[i] floats apart), on the target side (ldt[i]), and its rows of the layer's
 * gradient buffer (ldg); slot s is x_rstride / t_rstride / g_rstride ROWS further on.  weights: host, finite, > 0.  D % 4 == 0 and every
 * pointer and leading dimension a multiple of 16 bytes, else refused.  G = min(max_wg ? max_wg : 64, ceil(T * D / 1024)) workgroups walk a
 * (slot, layer) grid-stride; scratch (scratch_floats >= slots * n_layers * G) takes their partials.  For slot s and layer i, with
 * g = lambda / (float)(T * D) or grad_tab[s] (may be NULL; device, [slots]; a slot whose entry is 0 reads and writes nothing):
 *   grad[i][(s * g_rstride + r) * ldg + c] = 2 * (g * weights[i]) * d[r][c],   d = x - tgt
 *   scratch[(s * n_layers + i) * G + b]    = workgroup b's sum of d^2, a fixed tree
 *   values[s * n_layers + i] = (the G partials added in index order) * (weights[i] / (float)(T * D))
 *   part[s * part_pstride]   = the float32 sum of the slot's values, ascending from 0 (no other slot of part is written).
 * Layer i has the bits of its own n_layers = 1 call.  Refusals launch nothing. */
int splice_id_loss_layers(int n_layers, const float* const* x, const int* ldx, const float* const* tgt, const int* ldt, const float* weights,
                          size_t x_rstride, size_t t_rstride, int T, int D, int slots, float lambda, const float* grad_tab, float* const* grad, int ldg,
                          size_t g_rstride, float* scratch, size_t scratch_floats, float* values, float* part, size_t part_pstride, int max_wg,
                          splice_stream_t stream);
/* ------------------------------------------------------------------ the key second-moment appearance term.
 * With lambda > 0 (finite) and one block index `layer` in [0, depth), every step from cls_warmup on -- ordinary and entire-image steps
 * alike -- adds to the total, word 0 of the losses row,
 *     lambda * raw,   raw = sum over the crop pairs i < min(nA, nB) of mean over the D * D entries of (G(K_x'_i) - G(K_B'_i))^2,
 *     G(K) = K^T K / T,   K = the T x D keys of block `layer` (every token, the heads concatenated),
 * of x' = G(A_crop) against the target pass B', the passes the [CLS] appearance term compares; its key gradient
 * (4 lambda / (T D^2)) K_x' (G(K_x') - G(K_B')) is ADDED into the block's key-gradient buffer of the x' chain behind the structure term's
 * store.  raw lives in a buffer of its own (splice_step_key_gram_values); the [P][8] losses row, the trace row and the stop rule keep
 * their layout.  Three launches (key_gram.hip).  Before the first splice_step_run only and behind splice_step_set_ssim_layers /
 * splice_step_set_id_layers where they are called; refused on a handle in gradient-only or phase mode or with a leader (which in turn
 * refuses those calls), with fp8_selfsim, with several pairs whose crop counts nA != nB differ, and a second time.  A handle without the
 * call launches what it always did. */
int splice_step_set_key_gram(void* step, float lambda, int layer);
/* The raw term of the last step that computed it, copied to the host behind a device-wide wait: out[p] = pair p's value, `pairs`
 * floats.  A pair reads 0 before the first such step. */
int splice_step_key_gram_values(void* step, float* out);
/* test hook: the three launches of the term on caller buffers, one crop per pair.  Pair p reads the row-major bf16 keys k_x + p * k_ps
 * ([T][ldk]), and the token-contiguous copies kT_x + p * tx_ps and kT_b + p * tb_ps ([D][ldt_x] / [D][ldt_b], feature rows of tokens) of the
 * generated and the target pass.  D % 64 == 0; every bf16 pointer, leading dimension and pair stride a multiple of 16 bytes; ldt_x, ldt_b >=
 * round_up(T, 8), ldk, lddk >= D; part_ps >= the D / 64 * (D / 64 + 1) / 2 upper-triangular tiles; else refused with nothing launched.  The
 * contraction of the Gram matrices runs over the tokens < T: what the columns >= T of the transposed copies hold reaches no output bit.
 *   delta[p][D][D] (bf16)  = G(K_x') - G(K_B'), both triangles -- one fp32 accumulator per entry, [K_x ; K_B]^T [K_x ; -K_B], times 1 / T
 *   part[p * part_ps + t]  = tile t's fixed-tree sum of the fp32 entries squared, twice off the diagonal, times 1 / D^2
 *   value[p]               = the partials lane-strided ascending, then the wave tree: the raw term
 *   dk[p * dk_ps + r * lddk + c] += scale * (K_x' delta)[r][c]   for r < T; rows >= T keep their bits.
 * Pair p has the bits of its own one-pair call. */
int splice_key_gram_pairs(const splice_bf16* k_x, int ldk, size_t k_ps, const splice_bf16* kT_x, int ldt_x, size_t tx_ps, const splice_bf16* kT_b,
                          int ldt_b, size_t tb_ps, int T, int D, int pairs, float scale, splice_bf16* delta, float* part, size_t part_ps, float* value,
                          float* dk, int lddk, size_t dk_ps, splice_stream_t stream);
/* ------------------------------------------------------------------ the key second-moment term over several blocks, and its centred
 * form.  n ascending distinct block indices, n finite weights > 0, centered 0 / 1:
 *     raw = sum over the blocks l, ascending, of w_l * sum over the crop pairs of mean over the D * D entries of (M(K_l,x') - M(K_l,B'))^2,
 *     M(K) = K^T K / T   (centered 0),      M(K) = K^T K / T - mu mu^T,  mu = K^T 1 / T   (centered 1),
 * in the place and on the steps of splice_step_set_key_gram's term: lambda * raw enters word 0 last.  Block l's key gradient
 * (4 lambda w_l / (T D^2)) (K_l,x' Delta_l - 1 (Delta_l mu_l,x')^T) -- the second part where centred -- is ADDED into the block's
 * key-gradient buffer of the x' chain: the top block's, a structure-list block's, else one of its own that only the x' chain reads and that
 * is zeroed on the steps the term runs.  The launch count does not depend on n: the loss launch, the finish and the key-gradient launch,
 * and one launch for the means in front of them where centred (key_gram.hip).  The refusals of splice_step_set_key_gram hold; the two
 * setters exclude each other, in either order. */
int splice_step_set_key_gram_layers(void* step, float lambda, int n, const int* layers, const float* weights, int centered);
/* The per-layer addends of the last step that computed the term, copied to the host behind a device-wide wait: out[p * n + i] = pair p's
 * w_i * (block i's raw term, the pair's crops added in crop order), pairs * n floats.  splice_step_key_gram_values reports their float32
 * sum, ascending from 0 -- with one crop per pair the sum of row p exactly.  Zeros before the first such step. */
int splice_step_key_gram_layer_values(void* step, float* out);
/* test hook: the launches of the layered term on caller buffers, one crop per pair.  Entry i < n_layers (1..12) reads k_x[i], kT_x[i],
 * kT_b[i] and writes delta[i] ([pairs][D][D]), part[i] ([pairs][part_ps]) and dk[i], laid out and constrained as splice_key_gram_pairs'
 * operands of the same names with the shared strides given here; weights[i] finite and > 0, scales[i] finite.  No two entries share a dk, a
 * delta or a part pointer: refused (two entries adding into one dk would be two unordered read-modify-writes of one launch).  centered: mu
 * ([n_layers][pairs][2][D] floats) receives the fp32 means over the tokens < T of the generated and the target pass -- a feature's tokens
 * lane-strided ascending, the wave tree, times the rounded 1 / T -- and
 *   delta_i = bf16(fl(acc / T - m)),  m = fl(mu_x[r] mu_x[c] - fl(mu_b[r] mu_b[c]))   (two fused multiply-adds; centered 0: fl(acc * fl(1 / T)))
 *   part as splice_key_gram_pairs;  values[p * n_layers + i] = fl(weights[i] * (the finish sum of entry i's partials));  value[p] = their
 *   fp32 sum, ascending from 0
 *   dk_i[r][c] += scales[i] * fl((K_x' delta_i)[r][c] - rr[c]),  rr[c] = sum over j of delta_i[c][j] mu_x[j] in four quarters of fused
 *   multiply-adds added as (q0 + q1) + (q2 + q3)   (centered 0: scales[i] * (K_x' delta_i)[r][c]),  rows r < T.
 * With centered 0, entry i's delta, part and dk have the bits of splice_key_gram_pairs on its operands with scale = scales[i], and
 * values[.][i] is fl(weights[i] * its value).  Tokens >= T reach no output bit.  Refused with nothing launched: n_layers outside 1..12, a
 * null table or entry pointer, and what splice_key_gram_pairs refuses. */
int splice_key_gram_layers_pairs(int n_layers, const splice_bf16* const* k_x, const splice_bf16* const* kT_x, const splice_bf16* const* kT_b,
                                 splice_bf16* const* delta, float* const* part, float* const* dk, const float* weights, const float* scales, int ldk,
                                 size_t k_ps, int ldt_x, size_t tx_ps, int ldt_b, size_t tb_ps, int T, int D, int pairs, int centered, size_t part_ps,
                                 float* values, float* value, float* mu, int lddk, size_t dk_ps, splice_stream_t stream);
/* ------------------------------------------------------------------ the nearest-neighbour key appearance term.
 * With lambda > 0 (finite) and one block index `layer` in [0, depth), every step from cls_warmup on -- ordinary and entire-image steps
 * alike, the steps of the key second-moment term -- adds to the total, word 0 of the losses row, lambda * raw,
 *     raw = sum over the crop pairs i < min(nA, nB) of (1 / T) sum over the tokens t of (1 - c_t,j*(t)),
 *     c_tj = (k_t . b_j) / max(|k_t| |b_j|, eps),  eps = 1e-8,   j*(t) = the LOWEST j among those with the largest c_tj,
 * k_t / b_j the bf16 key rows of block `layer` (every token, the heads concatenated) of x' = G(A_crop) and of the target pass B'.  It
 * enters word 0 last, behind the key second-moment term where both are on.  The target carries no gradient; the key gradient, that of
 * autograd through clamp and max, is ADDED into the block's key-gradient buffer of the x' chain behind the structure term's store and the
 * key second-moment term's add: the top block's, a structure-list or key-second-moment block's, else one of its own that only the x' chain
 * reads and that is zeroed on the steps the term runs.  Four launches (key_nn.hip) whatever the number of pairs and crops.  Before the
 * first splice_step_run only and behind splice_step_set_ssim_layers / _id_layers / _key_gram / _key_gram_layers where they are called;
 * refused on a handle in gradient-only or phase mode or with a leader (which in turn refuses those calls), with fp8_selfsim, with several
 * pairs whose crop counts nA != nB differ, and a second time.  A handle without the call launches what it always did. */
int splice_step_set_key_nn(void* step, float lambda, int layer);
/* The raw term of the last step that computed it, copied to the host behind a device-wide wait: out[p] = pair p's value, `pairs`
 * floats.  A pair reads 0 before the first such step. */
int splice_step_key_nn_values(void* step, float* out);
/* The assignment of that step, copied to the host behind a device-wide wait: match ([pairs][crops][T] int32) and cos (the same shape,
 * floats), crops = min(nA, nB).  Zeros before the first such step.  Either pointer may be NULL. */
int splice_step_key_nn_match(void* step, int* match, float* cos);
/* test hook: the four launches of the term on caller buffers, one crop per pair.  Pair p reads the row-major bf16 keys k_x + p * kx_ps
 * (generated) and k_b + p * kb_ps (target), [T][ldk] each.  D % 64 == 0; T, pairs >= 1; both key pointers, ldk and the pair strides
 * multiples of 16 bytes; ldk, lddk >= D; part_ps >= ceil(T / 4); scale finite, eps finite and > 0; no null pointer; else refused with
 * SPLICE_ERR_ARG and nothing launched.  ws: splice_key_nn_ws_bytes(T, D, pairs) bytes of device scratch.  Rows >= T of either key array are
 * never read.  All arithmetic is fp32; fl() is one rounding to nearest; x_d are the bf16 values widened exactly.
 *   norms    n_t = sqrt(s),  s = the row's squares x_d^2 added by fused multiply-adds on 64 lanes (lane l: d = l, l + 64, ..., ascending,
 *            from 0), then the wave tree (offsets 32, 16, ..., 1);  m_j likewise of the target rows.
 *   cosines  a_tj = the fp32 MFMA accumulation of the D exact products k_td b_jd (16x16x32 bf16, K slices ascending);
 *            c_tj = fl(a_tj / max(fl(n_t m_j), eps))   for j < T.
 *   match    per 64-column tile the (maximum, lowest column of the maximum) of row t; the tiles ascending with a strict >:
 *            match[p][t] = j*(t),  cos[p][t] = c_t,j*   (all-zero row t: every c is 0, match 0).
 *   dk       with j = j*(t), q = fl(n_t m_j), f = max(q, eps), wb = fl(-scale / f), wk = q > eps ? fl(fl(scale * c_tj) / fl(n_t n_t)) : 0:
 *            dk[p * dk_ps + t * lddk + d] = fma(wb, b_jd, fma(wk, k_td, dk[...]))   for t < T, d < D; rows >= T keep their bits.
 *   part     part[p * part_ps + g] = (r_0 + r_1) + (r_2 + r_3),  r_w = fl(1 - c_t,j*) of row t = 4 g + w, 0 for t >= T;  g < ceil(T / 4).
 *   value    value[p] = fl(S * fl(1 / T)),  S = the partials added on 64 lanes (lane l: g = l, l + 64, ..., ascending, from 0), then the
 *            wave tree (the step: the pair's crops' S added in crop order from 0 first).
 * scale is lambda / T as the caller rounded it.  Pair p has the bits of its own one-pair call. */
size_t splice_key_nn_ws_bytes(int T, int D, int pairs);
int splice_key_nn_pairs(const splice_bf16* k_x, const splice_bf16* k_b, int ldk, size_t kx_ps, size_t kb_ps, int T, int D, int pairs, float scale,
                        float eps, int* match, float* cos, float* part, size_t part_ps, float* value, float* dk, int lddk, size_t dk_ps, void* ws,
                        splice_stream_t stream);
/* splice_total_loss_pairs as a handle with a loss trace launches it (splice_step_set_loss_trace): dev_t (device) holds step index + 1,
 * and words 0-5 of row step index of trace ([capacity][pairs][8], device) receive pair p's out8 values, a row at or beyond capacity
 * left out.  stop (may be NULL; device, [pairs] records) runs the instance of a handle with the stop rule, whose rule is window (>= 1),
 * rel, patience and min_steps as splice_plateau_update takes them: a pair whose stop_step lies before the step index is not traced,
 * and with ssim_on && !entire the records take the step as splice_plateau_update would. */
int splice_total_loss_pairs_trace(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls, float w_id,
                                  float* out8, int pairs, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on, int entire,
                                  splice_stop_state* stop, int window, float rel, int patience, int min_steps, const int* dev_t,
                                  float* trace, int capacity, splice_stream_t stream);

/* ------------------------------------------------------------------ test hooks: the [CLS] tail of the top ViT block as the engine launches it
 * in top_cls_only mode (vit_cls.hip).  The five entry points below check their arguments and call the engine's own launchers on the caller's
 * buffers; they add no kernel and no code path (tests/test_cls_tail_gpu.py against oracle/cls_tail.py).
 *
 * Single-query attention of the [CLS] token (row 0) of each of B passes, heads of 64 columns (H = D / 64):
 *   qkv     bf16 [B * Tld][3D], pass b at rows b * Tld ..; columns [0, D) q, [D, 2D) k, [2D, 3D) v, head h at + 64 h.  Read: q of row 0 and k
 *           of rows < T (forward), q of row 0 and v of rows < T (backward).  Rows T..Tld-1 are never read.
 *   qkvT    its transpose, bf16 [3D][ldt], pass b at column b * Tld.  The forward reads the v rows, the backward the k rows, Tld columns wide
 *           per pass; what lies at columns T..Tld-1 is multiplied by exact zeros: it must be READABLE and FINITE (an Inf or NaN there reaches
 *           every element of out / dq of that head).
 *   scale   multiplies q . k (0.125 for plain q; ln 2 for the engine's stored q, which carries d^-1/2 log2 e).
 *   out     bf16 [B][D], one compact row per pass: sum_j p_j v_j with p rounded to bf16, fp32 accumulation.  All of it is written.
 *   probs   fp32 [B][H][Tld]: softmax over the T keys, fp32; columns T..Tld-1 are written as +0.  The backward reads columns < T only.
 *   dout_slabs  the gradient of `out` as n_slabs (1..16) fp32 split-K slabs: slab s holds [B][D] at + s * slab_stride floats.  The kernel
 *           forms dO = bf16(((0 + s_0) + s_1) + ...), in slab order.
 *   dqkv    bf16 [B * Tld][3D].  Written, for every pass and head: the whole [Tld] x (q | k | v head slices) block -- dq on row 0 (with
 *           ds rounded to bf16) and zeros on rows 1..Tld-1; dk_j = bf16(ds_j q), ds_j = p_j (dO . v_j - delta) scale, delta = sum_j p_j dO . v_j;
 *           dv_j = bf16(p_j dO); rows T..Tld-1 all-zero bits.  Nothing outside [B * Tld][3D] is written.
 * Refused with SPLICE_ERR_ARG before anything is launched: a NULL operand, B < 1, T < 1, T > Tld, Tld % 32, ldt % 8 (16-byte loads),
 * ldt < B * Tld, D % 64, H != D / 64, n_slabs outside 1..16, dynamic LDS (6 Tld + 1056 bytes forward, 6 Tld + 1696 backward) above the
 * device's limit for a launch without a function attribute (64 KiB). */
int splice_attn_cls_fwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld, int D, int H, float scale, splice_bf16* out,
                        float* probs, splice_stream_t stream);
int splice_attn_cls_bwd(const splice_bf16* qkv, const splice_bf16* qkvT, int ldt, int B, int T, int Tld, int D, int H, float scale, const float* probs,
                        const float* dout_slabs, int n_slabs, size_t slab_stride, splice_bf16* dqkv, splice_stream_t stream);
/* LayerNorm of `rows` strided rows of D <= 768 columns (one workgroup per row): row r at x + r * xs, its output at y + r * ys (bf16), its
 * statistics at mean[r * ss] / rstd[r * ss] (two-pass variance, rstd = rsqrt(var + eps)).  Strides in elements; only the D columns of a row
 * are read or written, the gaps between rows are left alone.
 *   slabs == NULL: x is read and not written.
 *   slabs != NULL: the row is first FORMED as ((bias[c] + resid[r * rs + c]) + s_0) + s_1 ..., slab s at slabs[s * slab_stride + r * D + c]
 *           (compact rows), added in slab order, stored to x (x is not read) and then normalised.  n_slabs >= 1, any number.
 * Backward: dy row r at dy + r * dys, slab s at + s * slab_stride; with n_slabs > 1 the slabs are summed in slab order and the sum is
 * stored back into slab 0 (n_slabs <= 1: dy is not written).  x, mean, rstd as the forward left them.  g (fp32) and g_bf (bf16) are both
 * strided like x (row r at + r * xs): g += rstd (dxhat - mean(dxhat) - xhat mean(dxhat xhat)), dxhat = dy gamma -- g is READ, it must be
 * finite -- and g_bf = bf16(g).
 * Refused with SPLICE_ERR_ARG before anything is launched: a NULL operand (slabs, bias and resid may be NULL together), D outside 1..768,
 * rows < 1, slabs given with n_slabs < 1 or without bias / resid. */
int splice_ln_rows_fwd(float* x, size_t xs, const float* gamma, const float* beta, splice_bf16* y, size_t ys, float* mean, float* rstd, size_t ss,
                       int rows, int D, float eps, const float* slabs, int n_slabs, size_t slab_stride, const float* bias, const float* resid, size_t rs,
                       splice_stream_t stream);
int splice_ln_rows_bwd(float* dy, size_t dys, const float* x, size_t xs, const float* gamma, const float* mean, const float* rstd, size_t ss, float* g,
                       splice_bf16* g_bf, int rows, int D, int n_slabs, size_t slab_stride, splice_stream_t stream);
/* Finisher of a split-K GEMM with `rows` rows: v = (bias[n] + s_0) + s_1 + ..., slab s at slabs[s * slab_stride + row * N + n], in slab order
 * (modes 0 and 1; bias may be NULL = 0; mode 2 takes no bias), then
 *   mode 0: out_f32[row * os + n] = v + resid[row * rs + n]                                                  (fc2: the block output rows)
 *   mode 1: out_bf[row * N + n] = bf16(gelu(v)); pre_bf[row * ps + n] = bf16(v) for rows >= pre_lo, pre_bf may be NULL        (fc1)
 *   mode 2: out_bf[row * N + n] = bf16(v * gelu'(aux[row * ps + n])), aux bf16                                              (fc2^T)
 * Only the N columns of a row are written; rows of pre_bf below pre_lo and everything a mode does not name are left alone.
 * Refused with SPLICE_ERR_ARG before anything is launched: mode outside 0..2, rows or N < 1, slabs NULL or n_slabs < 1, out_f32 or resid
 * NULL in mode 0, out_bf NULL in modes 1 and 2, aux NULL in mode 2. */
int splice_rows_finish(int mode, const float* slabs, int n_slabs, size_t slab_stride, int rows, int N, const float* bias, const float* resid, size_t rs,
                       float* out_f32, size_t os, splice_bf16* out_bf, splice_bf16* pre_bf, const splice_bf16* aux, size_t ps, int pre_lo,
                       splice_stream_t stream);

/* ------------------------------------------------------------------ test hooks: generator launchers on caller-owned buffers
 * (gen_conv.hip, gen_wgrad.hip, gen_bn.hip, gen_pointwise.hip).  Each entry point checks its arguments and calls the launcher the generator
 * engine calls, on the caller's buffers; it adds no kernel, no policy and no code path (tests/test_gen_ops_gpu.py against oracle/gen_ops.py).
 * Which kernel instantiation runs is the launchers' own decision from the shapes; the hooks report it.  Everything a launcher would index out
 * of bounds with is refused with SPLICE_ERR_ARG before anything is launched: a NULL required pointer, a size < 1, a filter size outside
 * {1, 3, 5, 7}, a stride outside {1, 2}, a channel stride smaller than its plane, an image stride smaller than its channels (N > 1), reflection
 * with pad >= height or width, more than 128 output channels in a weight gradient, a batch above 8 or one that does not divide N, scratch
 * smaller than the launcher needs, offsets beyond the 32-bit gathers (channels x channel stride and the weight block at most 2^29 - 1 floats).
 *
 * Convolution (fp32 NCHW, exact-fp32 MFMA): channel c of image n of `in` at in + n * in_nstride + c * in_cstride, [Hi][Wi]; output column j
 * at out + n * out_nstride + j * out_cstride, [Ho][Wo]; weight element (column j, reduction channel c, tap) at w + j * w_jstride + c * w_cstride
 * + tap.  Cin counts the REDUCTION channels and Cout the output columns in either direction:
 *   forward      out[j][oy][ox] = bias[j] + sum_{c,ky,kx} in[c][oy * stride + ky - pad][ox * stride + kx - pad] w[j][c][ky][kx]  (zero padding;
 *                reflect: nn.ReflectionPad2d(pad) in front instead), act = 1: sigmoid behind it.
 *   transposed   the data gradient: out[j][iy][ix] = sum_{c,ky,kx} in[c][oy][ox] w(j, c, ky, kx) over oy * stride + ky - pad = iy (and x alike);
 *                for a forward weight [Co][Ci][ks][ks] that is Cin = Co, Cout = Ci, w_jstride = ks * ks, w_cstride = Ci * ks * ks.
 *   accumulate   out = out + result (one rounding more).  p_nstride > 0: image n reads w / bias at + (p_group > 1 ? n / p_group : n) * p_nstride.
 *   ws           optional split-K scratch of ws_floats floats (NULL: no split-K); defer_reduce leaves the raw slices in ws, slice k of image n,
 *                column j at ws + ((k * N + n) * Cout + j) * Ho * Wo, and does not touch out when form_out[4] > 1.
 * form_out (SPLICE_GEN_CONV_FORM_INTS ints, may be NULL): {1 = LDS-halo tile kernel / 0 = implicit GEMM, channels per K tile, output-channel
 * fragments per workgroup, wave groups, split-K slices}. */
typedef struct splice_gen_conv_args {
    const float* in;
    const float* w;
    const float* bias;        /* [Cout] or NULL */
    float* out;
    size_t in_nstride, in_cstride, out_nstride, out_cstride, w_jstride, w_cstride, p_nstride;
    int N, Cin, Hi, Wi, Cout, Ho, Wo, ks, stride, pad;
    int reflect, act, transposed, accumulate;
    float* ws;
    size_t ws_floats;
    int p_group, defer_reduce;
} splice_gen_conv_args;
#define SPLICE_GEN_CONV_FORM_INTS 5
int splice_gen_conv(const splice_gen_conv_args* args, int* form_out, splice_stream_t stream);
/* conv_pair_launch: a (1x1, stride 1) and b in one launch where an instantiation exists, else two launches; the results of two
 * splice_gen_conv calls bit for bit.  forms_out: 2 x SPLICE_GEN_CONV_FORM_INTS ints (a's, then b's), may be NULL. */
int splice_gen_conv_pair(const splice_gen_conv_args* a, const splice_gen_conv_args* b, int* forms_out, splice_stream_t stream);
/* Data gradient of a reflection-padded convolution.  args in data-gradient form as for the zero-padded layer (in = the output gradient, out =
 * the input gradient [N][Cout][Ho][Wo], pad = the layer's padding); pad_scratch: at least N * Cout * (Ho + 2 pad) * (Wo + 2 pad) floats. */
int splice_gen_conv_reflect_dgrad(const splice_gen_conv_args* args, float* pad_scratch, size_t scratch_floats, splice_stream_t stream);

/* Weight gradient dw[j][c][tap] (+)= sum over images and pixels of dy[j][oy][ox] x[c][oy * stride + ky - pad][ox * stride + kx - pad] (reflect: of the
 * reflection-padded x): conv_wgrad_add into an empty queue, conv_wgrad_batched_launch, wgrad_reduce_all_launch with one entry.
 * ws: splice_gen_conv_wgrad_ws_floats(...) floats of chunk partials.  p_nstride == 0: n_img = 1, one sum over the N images; p_nstride > 0:
 * n_img = N independent images, image i summed into dw + i * p_nstride.
 * form_out (SPLICE_GEN_WGRAD_FORM_INTS ints, may be NULL): {0 small / 1 big / 2 tile class, kernel variant, pixels per chunk, chunks,
 * 1 = the reduction runs four elements per thread, workgroups}. */
typedef struct splice_gen_wgrad_args {
    const float* x;
    const float* dy;
    float* ws;
    size_t ws_floats;
    size_t x_nstride, x_cstride, dy_nstride, dy_cstride;
    int N, Cin, Hi, Wi, Cout, Ho, Wo, ks, stride, pad, reflect;
} splice_gen_wgrad_args;
#define SPLICE_GEN_WGRAD_FORM_INTS 6
size_t splice_gen_conv_wgrad_ws_floats(int N, int Cin, int Cout, int ks, int Ho, int Wo);
int splice_gen_conv_wgrad(const splice_gen_wgrad_args* args, float* dw, int accumulate, int n_img, size_t p_nstride, int* form_out,
                          splice_stream_t stream);
/* Test hook: the reduction alone, for one layer on caller buffers.  partials = [chunks][n] floats; dw[i] (+)= the sum over the chunks of
 * partials[c][i] in the reduction's fixed order: four chains, each in increasing c from +0 -- chunk c of a full group of four joins chain c mod 4,
 * the chunks of the last, partial group all join chain 0 -- combined as (a0 + a1) + (a2 + a3), then the optional += into dw (accumulate).  p_nstride > 0: n_img independent images -- chunks must be a multiple of n_img, image i sums chunks
 * [i * chunks / n_img, (i + 1) * chunks / n_img) into dw + i * p_nstride (p_nstride >= n); else n_img must be 1.  chunks >= 0 (0: exact zeros). */
int splice_gen_wgrad_reduce(const float* partials, int n, int chunks, float* dw, int accumulate, int n_img, size_t p_nstride, splice_stream_t stream);

/* Train-mode BatchNorm (biased variance, rstd = 1 / sqrt(var + eps)) + LeakyReLU(slope) on [N][C][HW] planes, either direction, as
 * bn_fwd_launch / bn_bwd_launch run it.  splice_gen_bn_form reports the form of a plane as SPLICE_GEN_BN_FORM_INTS ints: {kind (0 SMALL, 1 MID,
 * 2 TWO_STAGE, 3 TWO_STAGE_VEC), hosts_pre, fwd_takes_slabs, bwd_takes_slabs, fwd_fuses_upsample, bwd_fuses_upsample, sign_from_y}.
 *   y / out      the BatchNorm's input and its activated output, image n at + n * y_nstride / out_nstride.  The forward WRITES y where it forms
 *                it (slabs, upsampled channels, the channels behind a pre BatchNorm); the backward reads both.
 *   batch        0: per-image statistics; > 0: statistics over groups of `batch` images (batch <= 8, N % batch == 0, batch < N needs p_nstride).
 *   p_nstride    > 0: image n (group n / batch) reads gamma / beta -- and writes dgamma / dbeta -- at + n * p_nstride.
 *   part         splice_gen_bn_part_floats(N, C) floats of scratch, needed by the two-stage kinds.  mean / rstd: [N][C], written by the forward.
 *   up_*         channels >= up_c0 are the x2 bilinear upsampling (align_corners = False, top-left up_Ho x up_Wo window, up_Ho * up_Wo = HW) of
 *                up_src [N][C - up_c0][up_h][up_w]; the backward sends their gradient through the adjoint into up_d_src.
 *   slabs        forward: y = bias + slab 0 + slab 1 + ... is formed and stored first; slabs [ksplit][N][C][HW], ksplit >= 2.
 *   da_slabs     backward: the gradient of out is (da_accumulate ? da : 0) + (slab 0 + slab 1 + ...), slabs [da_ksplit][N][C][HW].
 *   pre_*        a BatchNorm + LeakyReLU(pre_slope) of its own in front of the first pre_C channels: its input pre_y [N][pre_C][HW] (or formed from
 *                pre_slabs + pre_bias and stored there), its activated output stored into y; backward into pre_dy / pre_dgamma / pre_dbeta.
 * A pre or slabs on a form that cannot take them is refused (SPLICE_ERR_ARG, nothing written). */
typedef struct splice_gen_bn_args {
    float* y;
    float* out;
    size_t y_nstride, out_nstride;
    int N, C, HW, batch;
    const float* gamma;
    const float* beta;
    float eps, slope;
    size_t p_nstride;
    float* part;
    size_t part_floats;
    float* mean;
    float* rstd;
    const float* up_src;
    float* up_d_src;
    size_t up_src_ns, up_d_src_ns;
    int up_c0, up_h, up_w, up_Ho, up_Wo;
    const float* slabs;
    const float* bias;
    int ksplit;
    const float* da;
    float* dy;
    size_t da_nstride, dy_nstride;
    float* dgamma;
    float* dbeta;
    int accumulate;
    const float* da_slabs;
    int da_ksplit, da_accumulate;
    float* pre_y;
    size_t pre_y_ns;
    const float* pre_slabs;
    const float* pre_bias;
    int pre_ksplit, pre_C;
    const float* pre_gamma;
    const float* pre_beta;
    float* pre_mean;
    float* pre_rstd;
    float pre_slope;
    float* pre_dy;
    float* pre_dgamma;
    float* pre_dbeta;
} splice_gen_bn_args;
#define SPLICE_GEN_BN_FORM_INTS 7
int splice_gen_bn_form(int HW, int N, size_t p_nstride, int batch, int* out);
size_t splice_gen_bn_part_floats(int N, int C);
int splice_gen_bn_fwd(const splice_gen_bn_args* args, splice_stream_t stream);
int splice_gen_bn_bwd(const splice_gen_bn_args* args, splice_stream_t stream);
/* Test hook.  The small-plane kernels (form SMALL) exist in instances that compile only the features a launch needs; `mask` is the OR of
 * 1 batch statistics, 2 shared-parameter tail (backward, N > 1 without arenas), 4 slabs, 8 a pre BatchNorm, 16 a fused upsampling.  The launchers
 * pick the first of {0, 4, 16, 24, 28, 1, 2, 31} that covers a call.  mask >= 0 (one of those) makes every later small-plane launch of the process
 * take that instance -- 31 is the fully general one -- and splice_gen_bn_fwd / _bwd return SPLICE_ERR_ARG where the call needs a feature the instance
 * lacks; -1 restores the automatic choice.  Every instance that covers a call gives the same bits. */
int splice_gen_bn_small_instance(int mask);

/* The three launchers of gen_pointwise.hip.  Upsampling: in [N][C][h][w] -> the top-left Ho x Wo window of its x2 bilinear upsampling
 * (Ho <= 2h, Wo <= 2w), and the adjoint dout [N][C][Ho][Wo] -> din [N][C][h][w]; image strides in floats.  Sigmoid backward of the compact
 * [N][C][HW] head: dpre = dout * s * (1 - s), and per-segment sums of dpre into part ([image or group][segment][channel],
 * splice_gen_sigmoid_bias_part_floats(N, C) floats); *chunks_out = the partials per channel.  p_nstride > 0: one set of partials per group of
 * `group` images (N % group == 0), else one over all N. */
int splice_gen_upsample2x_fwd(const float* in, size_t in_nstride, float* out, size_t out_nstride, int N, int C, int h, int w, int Ho, int Wo,
                              splice_stream_t stream);
int splice_gen_upsample2x_bwd(const float* dout, size_t dout_nstride, float* din, size_t din_nstride, int N, int C, int h, int w, int Ho, int Wo,
                              splice_stream_t stream);
size_t splice_gen_sigmoid_bias_part_floats(int N, int C);
int splice_gen_sigmoid_bwd_bias(const float* dout, const float* sout, float* dpre, int N, int C, int HW, float* part, size_t part_floats,
                                size_t p_nstride, int group, int* chunks_out, splice_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* SPLICE_HIP_H */
