// Launchers of the generator kernels: the host-side interface of gen_conv.hip, gen_wgrad.hip, gen_bn.hip and gen_pointwise.hip.
#pragma once
#include "common.h"

struct ConvArgs {
    const float* in;      // [N][*][Hi][Wi]; channel c at in + img*in_nstride + c*in_cstride
    const float* w;       // element (col n, red. channel c, tap) at n*w_jstride + c*w_cstride + tap
    const float* bias;    // [Cout] or null
    float* out;           // [N][*][Ho][Wo]; channel n at out + img*out_nstride + n*out_cstride
    size_t in_nstride, in_cstride, out_nstride, out_cstride;
    size_t w_jstride, w_cstride;
    size_t p_nstride;     // > 0: independent images -- image n reads w / bias at + n * p_nstride (its own parameter arena)
    int N, Cin, Hi, Wi, Cout, Ho, Wo;   // Cin = reduction channels, Cout = output columns
    int ks, stride, pad;
    int reflect;      // forward only: reflection padding (nn.ReflectionPad2d) instead of zero padding
    int act;          // 1 = sigmoid
    int transposed;   // data-gradient form
    int accumulate;   // out += result
    float* ws;        // optional split-K scratch (ws_floats floats); null disables split-K
    size_t ws_floats;
    int ksplit;       // set by the launcher
    int p_group;      // > 1 (with p_nstride): grouped images -- image n reads the arena of group n / p_group; launch policies read one group
    int defer_reduce; // split-K: leave the raw slabs in ws (ksplit_out tells how many); the consumer adds bias + slabs in slice order
};
int conv_launch(const ConvArgs& a, hipStream_t s, int* ksplit_out = nullptr);
void conv_form_report(const ConvArgs& a, int* form);   // {tile kernel, CK, fn_run, ng, ksplit} of the path conv_launch takes (test hooks)
// two independent convolutions (a: 1x1, stride 1) in ONE launch where an instantiation exists, else two launches; same results
// as two conv_launch calls up to the summation order of `a` (it adopts b's wave groups)
int conv_pair_launch(ConvArgs a, ConvArgs b, hipStream_t s, int* ksplit_a = nullptr, int* ksplit_b = nullptr);
// data gradient of a reflection-padded convolution (transposed conv on the padded domain + mirror fold); see gen_conv.hip
int conv_reflect_dgrad_launch(ConvArgs a, float* pad_scratch, hipStream_t s);

struct WgradArgs {
    const float* x;       // layer input  [N][*][Hi][Wi]
    const float* dy;      // grad of the conv output [N][*][Ho][Wo]
    float* ws;            // scratch: chunks * Cout*Cin*ks*ks floats
    size_t x_nstride, x_cstride, dy_nstride, dy_cstride;
    int N, Cin, Hi, Wi, Cout, Ho, Wo, ks, stride, pad;
    int pix_per_chunk, chunks_per_img;   // filled by the launcher
    int reflect;                         // reflection padding of the forward convolution
};
int wgrad_chunks(int N, int Ho, int Wo, int* pix_per_chunk, int* chunks_per_img);
constexpr int WGRAD_BATCH_MAX = 32;
struct WgradDesc {           // compact per-layer descriptor of the batched weight-gradient launch (72 bytes)
    const float* x; const float* dy; float* ws;
    uint32_t x_nstride, x_cstride, dy_nstride, dy_cstride;
    uint16_t Cin, Cout, Hi, Wi, Ho, Wo;
    uint8_t ks, stride, pad, variant;
    uint16_t pix_per_chunk, chunks_per_img;
    uint32_t wg_begin, chunks;
    uint32_t reflect;
};
struct WgradBatch { int count; int total_wgs; WgradDesc d[WGRAD_BATCH_MAX]; };   // by-value kernel argument
struct WgradBatchPair { WgradBatch small, big, tile; };   // layers with <= 32 / > 32 output channels (different kernel occupancy); 3x3 layers of big planes (conv_wgrad_tile_kernel)
int conv_wgrad_add(WgradBatchPair* b, WgradArgs a, int* chunks_out);       // queue one layer; partials go to a.ws
int conv_wgrad_batched_launch(const WgradBatchPair& b, hipStream_t s);     // one launch per class for every queued layer

constexpr int WGRAD_MAX_LAYERS = 64;   // 26 conv weights + 25 exact-zero bias ranges (chunks == 0)
struct WgradReduceAll {      // by-value kernel argument: one entry per conv layer of a backward
    long long prefix[WGRAD_MAX_LAYERS + 1];   // prefix sums of n (output elements), prefix[count] = total
    long long ws_off[WGRAD_MAX_LAYERS];       // offset of the layer's partials in the workspace (floats)
    long long dw_off[WGRAD_MAX_LAYERS];       // offset of the layer's weight gradient in the arena
    int n[WGRAD_MAX_LAYERS], chunks[WGRAD_MAX_LAYERS];
    long long total;
    int count;
    unsigned char vec[WGRAD_MAX_LAYERS];      // set by wgrad_reduce_all_launch: the layer is reduced four elements per thread (16-byte accesses); prefix then counts work items
};
// p_nstride > 0: independent images -- image n's chunks are summed into grads + n * p_nstride
int wgrad_reduce_all_launch(const WgradReduceAll& d, const float* ws, float* grads, int accumulate, hipStream_t s, int n_img = 1, size_t p_nstride = 0);

// train-mode BatchNorm (+LeakyReLU when slope != 1) forward: statistics in two deterministic stages
// (per-segment partials, recombined in the apply kernel); `part` = bn_part_floats(N, C) floats of scratch.
int bn_part_floats(int N, int C);
// Optional fusion of the decoder's x2 bilinear upsampling (models/unet/skip.py: nn.Upsample in front of the concat's
// BatchNorm) into the BatchNorm kernels of the concat unit: channels >= c0 of the normalised tensor ARE the upsampling of
// `src`.  Forward: they are computed on the fly (and stored into y for the backward) instead of by a launch of their
// own; backward: their input gradient goes straight through the adjoint into d_src.  A form that does not fuse a direction
// (BnForm) gets the stand-alone upsampling launch from the BatchNorm launcher: same tensors either way.
struct BnUpsample {
    const float* src = nullptr; size_t src_ns = 0;   // [N][C - c0][h][w]
    float* d_src = nullptr; size_t d_src_ns = 0;
    int c0 = 0, h = 0, w = 0, Ho = 0, Wo = 0;
};
// A BatchNorm + LeakyReLU that sits in FRONT of the first `C` channels of a concat BatchNorm's input (the skip branch of a scale:
// models/unet/skip.py:60-62 feeding the Concat + BatchNorm of :75-81).  Both BatchNorms of such a channel are reductions over the
// SAME plane, so the workgroup that owns the plane in the concat's one-launch BatchNorm kernels runs the skip branch's first
// (forward: statistics, normalise, activate, store into the concat buffer; backward: the adjoint behind the concat's) -- the skip
// branch's BatchNorm has no launch of its own in either direction (round 4).
struct BnPre {
    const float* y = nullptr; size_t y_ns = 0;      // the skip convolution's output [N][C][HW] (forward: input; slabs != null: formed and stored here)
    const float* slabs = nullptr; int ksplit = 0;    // split-K slabs of that convolution (deferred reduction), with its bias
    const float* bias = nullptr;
    const float* gamma = nullptr; const float* beta = nullptr;   // the skip BatchNorm's parameters (image n at + n * p_nstride)
    float* mean = nullptr; float* rstd = nullptr;    // its saved statistics [N][C]
    float slope = 0.2f;
    int C = 0;
    // backward only
    float* dy = nullptr;                             // gradient w.r.t. the skip convolution's output [N][C][HW]
    float* dgamma = nullptr; float* dbeta = nullptr;
};
// The output gradient of a BatchNorm, left as split-K slabs by the data-gradient convolution that produces it (deferred reduction,
// backward direction): d_out = (accumulate ? what the first writer stored at d_out : 0) + sum_k slabs[k], formed by the BatchNorm
// backward while it loads the plane -- the arithmetic and order of conv_splitk_reduce_kernel, which then has no launch (round 4).
struct BnSlabs {
    const float* slabs = nullptr;   // [ksplit][N][C][HW]
    int ksplit = 0, accumulate = 0;
};
// Which kernel form a BatchNorm plane runs in and what that form absorbs: THE table of forms -- bn_fwd_launch / bn_bwd_launch dispatch on
// it, the engine plans with it (which convolutions may leave split-K slabs, which skip branch is chained, which workspaces to keep).
//   SMALL          HW <= 4096                                      one launch, the plane in registers
//   MID            HW <= 16384, per-image statistics, own arena     one launch, the plane in LDS
//   TWO_STAGE      everything else                                  partials + apply, <= 64 scalar segments
//   TWO_STAGE_VEC  65536 < HW <= 1.31 M                             partials + apply, <= 256 segments in 16-byte runs
// batch: images per statistics group (0: per image); p_nstride: images (groups) with parameter arenas of their own.
struct BnForm {
    enum Kind { SMALL, MID, TWO_STAGE, TWO_STAGE_VEC } kind;
    bool hosts_pre;            // a BnPre can ride in this launch (SPLICE_BN_CHAIN=0: never)
    bool fwd_takes_slabs;      // forward sums the feeding convolution's split-K slabs (BnArgs::slabs)
    bool bwd_takes_slabs;      // backward sums the feeding data gradient's split-K slabs (BnSlabs; SPLICE_BN_BWD_SLABS=0: never)
    bool fwd_fuses_upsample;   // forward produces the upsampled channels itself (else the launcher runs upsample2x_fwd_kernel in front)
    bool bwd_fuses_upsample;   // backward sends them through the adjoint itself (else the launcher runs upsample2x_bwd_kernel behind)
    bool sign_from_y;          // backward re-forms the activation's sign from y and beta (SPLICE_BN_SIGN_FROM_Y=0: never)
};
BnForm bn_form(int HW, int N, size_t p_nstride, int batch);
// One BatchNorm (+ LeakyReLU when slope != 1) launch, either direction.  batch > 0: statistics over groups of `batch` images
// (nn.BatchNorm2d on a batch), batch <= 8; batch < N needs p_nstride (one arena per group).
struct BnArgs {
    const float* y = nullptr; size_t y_nstride = 0;       // the BatchNorm's input [N][C][HW] (forward with slabs or a non-fused upsampling: formed here first)
    float* out = nullptr; size_t out_nstride = 0;         // the activated output (backward: read)
    int N = 0, C = 0, HW = 0;
    const float* gamma = nullptr; const float* beta = nullptr;   // image n at + n * p_nstride
    float eps = 0.f, slope = 1.f;
    size_t p_nstride = 0;
    int batch = 0;
    float* part = nullptr;                                // bn_part_floats(N, C) floats of scratch (two-stage forms)
    float* mean = nullptr; float* rstd = nullptr;         // saved statistics [N][C] (forward: written)
    const BnUpsample* up = nullptr;                       // channels >= up->c0 are an upsampling (forward: of up->src; backward: gradient to up->d_src)
    const BnPre* pre = nullptr;                           // needs a form that hosts_pre
    // forward only: y = bias + sum_k slabs[k] is formed, stored (the backward reads it) and normalised in one launch (needs fwd_takes_slabs, ksplit >= 2)
    const float* slabs = nullptr; int ksplit = 0; const float* bias = nullptr;
    // backward only
    const float* da = nullptr; size_t da_nstride = 0;     // gradient w.r.t. out
    float* dy = nullptr; size_t dy_nstride = 0;           // gradient w.r.t. y
    float* dgamma = nullptr; float* dbeta = nullptr;
    int accumulate = 0;                                   // dgamma / dbeta += result
    const BnSlabs* da_slabs = nullptr;                    // needs bwd_takes_slabs
};
int bn_fwd_launch(const BnArgs& a, hipStream_t s);
int bn_bwd_launch(const BnArgs& a, hipStream_t s);
// test hook: the small-plane kernels are instantiated per feature mask (gen_bn.hip, BN_F_*); mask >= 0 makes every small-plane launch take that
// instance (31 = the fully general one) and fail with SPLICE_ERR_ARG where its arguments need a feature the instance lacks; -1 = automatic again
int bn_small_force_instance(int mask);
int upsample2x_fwd_launch(const float* in, size_t in_nstride, float* out, size_t out_nstride, int N, int C, int h, int w, int Ho, int Wo, hipStream_t s);
int upsample2x_bwd_launch(const float* dout, size_t dout_nstride, float* din, size_t din_nstride, int N, int C, int h, int w, int Ho, int Wo, hipStream_t s);
// sigmoid backward of the [N][C][HW] head + per-channel sums of the result (the head's bias gradient) in two
// deterministic stages; part = C * 64 floats of scratch
int sigmoid_bwd_bias_launch(const float* dout, const float* sout, float* dpre, int N, int C, int HW, float* part, hipStream_t s, size_t p_nstride, int* chunks,
                            int group = 1);
int sigmoid_bias_part_floats(int N, int C);   // floats of `part`: [image][segment][channel], summed by wgrad_reduce_all_launch
// BatchNorm running statistics of up to 3 generator calls (in call order) in one launch; see gen_bn.hip
constexpr int RUNSTAT_MAX_PLANS = 3, RUNSTAT_MAX_BN = 36;
struct RunStatTable {
    int n_plans, n_bn;
    int C[RUNSTAT_MAX_BN], r_off[RUNSTAT_MAX_BN];      // channels; offset of running_mean in the buffer arena (running_var follows at + C)
    int N[RUNSTAT_MAX_PLANS], indep[RUNSTAT_MAX_PLANS];
    int img_step[RUNSTAT_MAX_PLANS];                   // grouped plans: images per update (the group's first image holds its statistics); 0 / 1 otherwise
    int HW[RUNSTAT_MAX_PLANS][RUNSTAT_MAX_BN];
    const float* mean[RUNSTAT_MAX_PLANS][RUNSTAT_MAX_BN];   // [N][C] batch statistics saved by the forward
    const float* rstd[RUNSTAT_MAX_PLANS][RUNSTAT_MAX_BN];
};
// mask / mask_step (optional, the plateau stop rule): the arena of a slot frozen at step *mask_step - 1 is left alone
int bn_running_update_launch(const RunStatTable& t, float* running, size_t r_nstride, float momentum, float eps, int max_images, hipStream_t s,
                             const splice_stop_state* mask = nullptr, const int* mask_step = nullptr);
// splice_gen_running_stats_update with that mask (gen_engine.hip; the step engine's bookkeeping)
int gen_running_stats_update(void* const* plans, int n_plans, float* running, long long running_stride, float momentum, const splice_stop_state* mask,
                             const int* mask_step, hipStream_t s);
