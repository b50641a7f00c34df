// One Splice optimisation step (train.py:51-80) as a single host call: zero_grad, Model.forward
// (models/model.py:12-25), LossG.forward with its lambda schedule (util/losses.py:34-72),
// backward and Adam -- with the de-duplicated ViT plan of SURVEY.md section 7: the four global
// passes [T(A_crop), T(B_crop), T(G(A_crop)), T(G(B_crop))] run as ONE batched forward (the
// reference runs six batch-1 forwards, x' and B' twice), the backward covers only the two
// generated images and only data gradients.  Nothing is cached across steps.
//
// P image pairs side by side (cfg.pairs): the reference optimises one pair per process (train.py:34-49); pairs share
// nothing but the frozen ViT, so P of them can ride the SAME launches -- the ViT context holds 4P passes
// [A'_0..A'_{P-1} | B'_0.. | x'_0.. | y'_0..], every GEMM / attention / LayerNorm launch covers P times the rows, the
// generator plans hold P independent generators (own parameter / gradient / Adam arenas, own BatchNorm statistics), the
// loss kernels take the pair as a grid dimension.  Every per-pair quantity is computed exactly as in a P = 1 step (no
// policy depends on P), so a pair's trajectory is bit-identical whichever batch it rides in.
#include <algorithm>
#include <memory>
#include <vector>

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gen_kernels.h"
#include "kernels.h"
#include "optim.h"
#include "plateau.h"
#include "step_graph.h"

// The loss terms.  L_*: slot of a term in the losses buffer, and the order of total_loss_kernel's five weights.  LAM_*: column of a term in
// the host [P][5] lambdas of splice_step_set_pair_weights (and in pw_any).  PW_*: row ([P] floats each) of the device tables built from them --
// e_scale of the two structure terms, gradient weights of the three MSE terms -- followed at row PW_LAMBDAS by a copy of the [P][5] lambdas.
enum { L_TOTAL = 0, L_GLOBAL_SSIM = 1, L_ENTIRE_SSIM = 2, L_ENTIRE_CLS = 3, L_GLOBAL_CLS = 4, L_GLOBAL_ID = 5, L_TERMS = 6 };
// the two image-space terms (splice_step_set_image_terms; image_terms.hip): slots 6 and 7 of the losses row and of the partials, outside the
// tables above -- their weights are the handle's two scalars, shared by the slots of a sweep, and no schedule gates them
enum { L_GLOBAL_TV = 6, L_GLOBAL_PIX = 7 };
enum { LAM_CLS = 0, LAM_SSIM = 1, LAM_ID = 2, LAM_ECLS = 3, LAM_ESSIM = 4 };
enum { PW_ESCALE_G = 0, PW_ESCALE_E = 1, PW_CLS = 2, PW_ID = 3, PW_ECLS = 4, PW_LAMBDAS = 5, PW_ROWS = 10 };
static const int TERM_LAM[L_TERMS] = {-1, LAM_SSIM, LAM_ESSIM, LAM_ECLS, LAM_CLS, LAM_ID};          // by L_*
static const int TERM_ROW[L_TERMS] = {-1, PW_ESCALE_G, PW_ESCALE_E, PW_ECLS, PW_CLS, PW_ID};

struct VitView {
    void* ctx = nullptr;
    int B = 0, H = 0, W = 0, D = 0, depth = 0, heads = 0, patch = 0, T = 0, Tld = 0, rows = 0;
    float* d_block = nullptr;   // [rows][D]
    float* d_keys = nullptr;    // [rows][D]
    float* imgs = nullptr;      // [B][3][H][W]
    float* d_imgs = nullptr;    // [B][3][H][W]
    std::vector<const float*> pb, pk;   // per-layer pointer tables
    float* dk_layer[SELFSIM_MAX_LAYERS] = {};   // splice_step_set_ssim_layers: the key-gradient buffer of entry i of the layer list (d_keys for the top block)
    // splice_step_set_cls_layers: entry i's [CLS]-row seed buffer [B][D] (null for the top block, which keeps row 0 of d_block), the [depth]
    // table of them the context is armed with, and the per-layer addends [slots][n] of the view's appearance term
    float* cls_seed[CLS_MAX_LAYERS] = {};
    std::vector<const float*> cls_seed_tab;
    float* cls_values = nullptr;
    // splice_step_set_id_layers (global view only): the key-gradient buffer of entry i of the identity list -- d_keys for the top block, the
    // structure list's buffer of a block both lists name, else one of its own (then also in dk_id_own: its y' passes are zeroed each step) --
    // and the y' chain's key-gradient table: pk plus the identity blocks
    float* dk_id[ID_MAX_LAYERS] = {};
    float* dk_id_own[ID_MAX_LAYERS] = {};
    std::vector<const float*> pk_y;
    // splice_step_set_key_gram_layers (global view only): the key-gradient buffer entry i of the list adds into -- pk's of its block (d_keys
    // at the top, the structure list's buffer of a block that list names), else one of its own (then also in dk_kgl_own: its x' passes are
    // zeroed each step) -- and the x' chain's key-gradient table on the steps the term runs: pk plus the blocks of its own.  The one block of
    // splice_step_set_key_gram is entry 0.
    float* dk_kgl[KEY_GRAM_MAX_LAYERS] = {};
    float* dk_kgl_own[KEY_GRAM_MAX_LAYERS] = {};
    std::vector<const float*> pk_x;
    // splice_step_set_key_nn (global view only): the key-gradient buffer the nearest-neighbour term adds into -- pk_x's of its block (pk's,
    // or the key second-moment term's own), else one of its own (then also in dk_nn_own, zeroed over its x' passes like dk_kgl_own's)
    float* dk_nn = nullptr;
    float* dk_nn_own = nullptr;
};

// The blocks a per-layer loss term reads and their weights (splice_step_set_ssim_layers, ..._cls_layers, ..._id_layers,
// ..._key_gram_layers): n ascending distinct block indices, n finite weights > 0; 0 entries: the term has no list.  One record for the four
// terms, sized by the largest of their caps; no term's kernel table may hold fewer entries than it.
constexpr int LAYER_LIST_MAX = std::max({SELFSIM_MAX_LAYERS, CLS_MAX_LAYERS, ID_MAX_LAYERS, (int)KEY_GRAM_MAX_LAYERS});
static_assert(SELFSIM_MAX_LAYERS >= LAYER_LIST_MAX, "SelfSimLayers holds fewer entries than a LayerList");
static_assert(CLS_MAX_LAYERS >= LAYER_LIST_MAX, "ClsLayers holds fewer entries than a LayerList");
static_assert(ID_MAX_LAYERS >= LAYER_LIST_MAX, "IdLayers holds fewer entries than a LayerList");
static_assert(KEY_GRAM_MAX_LAYERS >= LAYER_LIST_MAX, "KeyGramLayers holds fewer entries than a LayerList");
struct LayerList {
    int n = 0;
    int layers[LAYER_LIST_MAX] = {};
    float weights[LAYER_LIST_MAX] = {};
    void set(int count, const int* l, const float* w) {
        n = count;
        for (int i = 0; i < count; ++i) { layers[i] = l[i]; weights[i] = w[i]; }
    }
};

struct SpliceStep {
    splice_step_config cfg;
    int P = 1;                   // pairs optimised side by side -- or, in crops mode, the n_crops global crops of ONE pair (max of the two counts)
    int Pa = 1, Pb = 1;          // images of the A-crop / B-crop plans: P in pairs mode; global_A_crops_n_crops / global_B_crops_n_crops in crops mode
    int crops_mode = 0;          // n_crops > 1: the slots are crops -- pair p's na A crops / nb B crops are images p * na + i / p * nb + i (pair-major)
                                 // of plans in grouped batch-statistics mode (one netG call and one arena per pair), losses summed over a pair's crops
    int pairs = 1;               // pairs (parameter arenas, rows of the loss table, images of the entire-image branch): cfg.pairs; P = pairs * max(na, nb) slots
    int na = 1, nb = 1;          // A / B crops per pair (1 in pairs mode)
    size_t astride = 0;          // floats between the pairs' parameter / gradient / moment arenas (P > 1, pairs mode)
    VitView vg, ve;
    void *plan_a = nullptr, *plan_b = nullptr, *plan_e = nullptr;   // generator plans: P independent images each
    int cropb_h = 0, cropb_w = 0;
    long long nparams = 0;
    float* gen_in = nullptr;     // [P][3][ha][wa]   A crops            (staged copies: a captured graph only sees own buffers)
    float* in_b = nullptr;       // [P][3][hb][wb]   B crops
    float* ent_in = nullptr;     // [P][3][He][We]   entire structure images
    float* gen_out = nullptr;    // [P][3][ha][wa]   x_global
    float* gen_out_b = nullptr;  // [P][3][hb][wb]   y_global
    float *d_gen_out = nullptr, *d_gen_out_b = nullptr;
    float* ent_out = nullptr;    // [P][3][He][We]
    float* d_ent_out = nullptr;
    void* ssim_ws = nullptr;     // SelfSimBatch workspace (shared by the global and the entire-image term: they run back to back)
    float* losses = nullptr;     // per pair: [8] raw per-term losses, then [8][lp] workgroup partials of each term
    size_t lp = 0, lstride = 0;  // partial slots per term; floats per pair
    std::vector<void*> allocs;
    int max_crop_h = 0, max_crop_w = 0;
    int* dev_t = nullptr;        // Adam step count on the device
    float* dev_lr = nullptr;     // learning rate of the step on the device (staged per step once splice_step_set_lr was called)
    int lr_set = 0;              // 0: the optimiser node takes cfg.lr as a kernel argument (the handle's behaviour before any splice_step_set_lr)
    float lr = 0.f;              // value staged into dev_lr by the next run
    int opt_kind = SPLICE_OPT_ADAM;      // splice_step_set_optimizer; hp0 / hp1 / eps start as cfg.beta1 / beta2 / eps
    // per-pair configs (splice_step_set_pair_weights / splice_step_set_pair_lr; pairs mode only).  pw: device tables (rows PW_*), NULL until
    // set.  pw_any[LAM_*]: some pair has that lambda > 0 (the term's launch happens).
    float* pw = nullptr;
    float* pw_tab_alloc = nullptr;   // (the tables' memory: allocated at creation for P > 1, switched on as pw by splice_step_set_pair_weights)
    int pw_any[5] = {0, 0, 0, 0, 0};
    float* dev_lrs = nullptr;    // [SPLICE_STEP_MAX_PAIR_CFGS] per-pair learning rates, staged per step once splice_step_set_pair_lr was called
    int pair_lr = 0;
    float lrs[SPLICE_STEP_MAX_PAIR_CFGS] = {};
    float opt_hp0 = 0.f, opt_hp1 = 0.f, opt_eps = 0.f;
    // the extended rules (splice_step_set_optimizer_ext): the option record and the caller's third moment arena(s); off: the step launches
    // what it always did
    int opt_ext_on = 0;
    splice_optim_ext opt_ext = {};
    float* opt_w = nullptr;
    hipStream_t own_stream = nullptr;
    // Cross-stream events, a RING of sets: an eager step records its fork / join events twice and the next step records them again
    // ~2 ms later, while waits on the previous record may still be queued; every record site has an event of its own and a set is
    // reused only EV_RING steps later (the runtime's completion handler crashed in the release chain of such marker commands once per
    // ~30 train_model runs, see step_graph.hip)
    enum { EV_IN, EV_OUT, EV_FORK, EV_JOIN, EV_GB, EV_FORK2, EV_JOIN2, EV_KINDS };
    static constexpr int EV_RING = 4;
    hipEvent_t evs[EV_RING][EV_KINDS] = {};
    int ev_slot = 0;
    hipEvent_t ev(int kind) const { return evs[ev_slot][kind]; }
    hipStream_t side_stream = nullptr;               // target-pass ViT forward beside the generator forward
    int overlap = 1;                                 // SPLICE_STEP_OVERLAP=0 serialises (debugging)
    int ablate = 0;                                  // always 0 in the product build.  Scratch builds (-DSPLICE_DEV_SWITCHES) read the SPLICE_STEP_ABLATE bitmask, TIMING experiments only (results are garbage):
                                                     // 1 skip G fwd, 2 skip G bwd, 4 skip ViT bwd, 8 skip target ViT fwd, 16 skip generated ViT fwd, 32 skip the y' chain of the ViT bwd
    StepGraphs graphs;                               // executables by variant (regime and phases); retired whenever the launch sequence or a bound pointer changes
    void* graph_ptrs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // arenas + the caller's losses / running buffers a captured graph is bound to
    float* losses_out = nullptr;                     // this step's destination of the [P][8] loss values (written by total_loss_kernel)
    int graph_crops[4] = {0, 0, 0, 0};
    float* grads_b = nullptr;                        // gradient arena(s) of the B-crop plan (added to `grads` inside Adam)
    int shape_repeats = 0;                           // consecutive steps with the same arenas and crop sizes
    int repeat_step = -1;                            // step_idx the count above was last advanced / reset for (several partial-phase calls of ONE step count once)
    int use_graph = 1;
    int dbg_sync = 0;
    int ssim_id_on = 0;          // lambda_global_ssim / lambda_global_identity switched on (util/losses.py:35-37)
    int skip_adam = 0, accumulate = 0;   // splice_step_set_mode: leave the summed gradient in `grads` (optionally += ) and do not update
    float* running = nullptr;    // BatchNorm running statistics arena(s) of the caller (null: not tracked)
    long long running_stride = 0;
    int phases = 7;              // splice_step_set_phases: 1 generator forward, 2 ViT forward / losses / ViT backward, 4 generator backward (+ Adam)
    SpliceStep* leader = nullptr;   // the handle whose staged inputs / generator outputs this one reads and whose image gradients it adds to
    // the plateau stop rule (splice_step_set_stop_rule; plateau.h): [pairs] state records on the device, allocated at creation (zeros, stop_step -1)
    splice_stop_state* stop = nullptr;
    StopRule stop_rule = {0, 0.f, 0, 0};   // window 0: off -- the step launches what it always did
    int runs = 0;                          // splice_step_run calls so far (the rule is set before the first)
    // the weight average (splice_step_set_ema): the caller's arena(s), laid out like params; null: off -- the step launches what it always did
    float* ema = nullptr;
    float ema_decay = 0.f;
    int ema_start = 0;
    // gradient clipping (splice_step_set_grad_clip): the caller's [pairs] records and the handle's chunk partials; null: off -- the step
    // launches what it always did
    splice_clip_state* clip = nullptr;
    float* clip_partials = nullptr;
    float clip_norm = 0.f;
    // ... against the pair's own running norm (splice_step_set_grad_clip_auto): the rule with the caller's second [pairs] records; its regime
    // is filled in per launch sequence; records null: the threshold is clip_norm alone
    ClipAutoRule clip_rule = {0.f, 0.f, 0, 0, nullptr};
    // keep-best (splice_step_set_keep_best): the caller's [pairs] records, window means and best arena(s); null: off -- the step launches what
    // it always did
    splice_best_state* best = nullptr;
    float* best_means = nullptr;
    float* best_p = nullptr;
    float* best_ema = nullptr;
    // the per-step loss trace (splice_step_set_loss_trace): the caller's [trace_cap][pairs][8] rows; null: off -- the step launches what it
    // always did
    float* trace = nullptr;
    int trace_cap = 0;
    // the plateau lr rule (splice_step_set_lr_plateau): the caller's [pairs] records and cut-step rows, and the handle's [pairs] table of
    // effective learning rates -- written by the loss kernel, read by the optimiser launch of the same step; null: off -- the step launches
    // what it always did
    LrRule lr_rule = {0.f, 1, 0.f};
    splice_lr_state* lr_state = nullptr;
    int* lr_cuts = nullptr;
    float* lr_eff = nullptr;
    // the row table of the gather staging (splice_step_set_input_rows): pair p of the handle is pair in_rows[p] of the caller's pairs_in
    // pairs; pairs_in 0: off -- the step launches what it always did
    int pairs_in = 0;
    int in_rows[SPLICE_STEP_MAX_PAIR_CFGS] = {};
    // the image-space terms (splice_step_set_image_terms): lambda_global_tv on x' = G(A_crop), lambda_global_pixel_identity on y' = G(B_crop)
    // against B_crop; both 0: off -- the step launches what it always did
    float lambda_tv = 0.f, lambda_pix = 0.f;
    // the blocks whose keys the two structure terms read (splice_step_set_ssim_layers), and one SelfSimBatch workspace
    // per entry (entry 0: ssim_ws); 0 entries: off -- the top block alone, the step launches what it always did
    LayerList ssim_list;
    void* ssim_ws_layer[SELFSIM_MAX_LAYERS] = {};
    // the blocks whose [CLS] row the two appearance terms read (splice_step_set_cls_layers); 0 entries: off -- the
    // top block alone, the step launches what it always did
    LayerList cls_list;
    // the blocks whose keys the identity term reads (splice_step_set_id_layers); 0 entries: off -- the top block
    // alone, the step launches what it always did.  id_scratch: the workgroup partials of the term's main launch, [Pb][n][G]; id_values: the
    // per-layer addends, [Pb][n]
    LayerList id_list;
    float *id_scratch = nullptr, *id_values = nullptr;
    // the key second-moment appearance term (splice_step_set_key_gram): its weight (0: off -- the step launches what it
    // always did) and block; kg_delta: the bf16 Gram differences, [Pc][D][D]; kg_part: the tile partials, [Pc][tiles]; kg_value: the raw
    // term, [pairs]
    float kg_lambda = 0.f;
    int kg_layer = -1;
    bf16_t* kg_delta = nullptr;
    float *kg_part = nullptr, *kg_value = nullptr;
    // ... over several blocks (splice_step_set_key_gram_layers): the list of n entries (0: the one-block term above) and
    // the centred flag; kg_delta / kg_part then hold [n][Pc]... ; kg_values: the per-layer addends, [pairs][n]; kg_mu: the fp32 means of the
    // centred form, [n][Pc][2][D]
    LayerList kg_list;
    int kg_centered = 0;
    float *kg_values = nullptr, *kg_mu = nullptr;
    // the nearest-neighbour key appearance term (splice_step_set_key_nn): its weight (0: off -- the step launches what
    // it always did) and block; nn_match / nn_cos: the assignment, [Pc][T]; nn_part: the row launch's partials, [Pc][ceil(T / 4)]; nn_value:
    // the raw term, [pairs]; nn_ws: the scratch of key_nn.hip
    float nn_lambda = 0.f;
    int nn_layer = -1;
    int* nn_match = nullptr;
    float *nn_cos = nullptr, *nn_part = nullptr, *nn_value = nullptr, *nn_ws = nullptr;
};

// the key second-moment term runs over a list of blocks (splice_step_set_key_gram_layers: the list launches) rather than over its one block
// (splice_step_set_key_gram: the one-block launches, which round their scale differently)
static bool kg_listed(const SpliceStep* st) { return st->kg_list.n > 0; }
static size_t arena_floats(const SpliceStep* st) { return st->astride ? st->pairs * st->astride : (size_t)st->nparams; }   // of all pairs' arenas
static bool create_events(SpliceStep* st) {
    for (auto& set : st->evs)
        for (hipEvent_t& e : set)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return false;
    return true;
}

template <class T>
static int salloc(SpliceStep* st, T** p, size_t n) {
    void* q = nullptr;
    if (hipMalloc(&q, n * sizeof(T) + 256) != hipSuccess) {
        splice_set_error("splice_step: hipMalloc of %zu bytes failed", n * sizeof(T));
        return SPLICE_ERR_NOMEM;
    }
    st->allocs.push_back(q);
    *p = (T*)q;
    return SPLICE_OK;
}

static int view_init(SpliceStep* st, VitView& v, void* ctx, int want_B) {
    v.ctx = ctx;
    RC(splice_vit_ctx_dims(ctx, &v.B, &v.H, &v.W, &v.D, &v.depth, &v.heads, &v.patch));
    RC(splice_vit_ctx_info(ctx, &v.T, &v.Tld, &v.rows));
    // Of the top block the losses read the keys and the [CLS] row (util/losses.py:90); cfg.top_cls_only skips the rest of it
    // (vit_cls.hip): +2.7 % / +5.2 % pair-steps/s at 4 / 8 pairs per GPU, +2.7 % at one pair once the few-row kernels of the tail
    // request their operands in one round trip, DESIGN.md section 8.
    RC(splice_vit_ctx_set_top_cls_only(ctx, st->cfg.top_cls_only));
    if (v.B != want_B) { splice_set_error("splice_step_create: ViT context has batch %d, need %d", v.B, want_B); return SPLICE_ERR_ARG; }
    RC(salloc(st, &v.d_block, (size_t)v.rows * v.D));
    RC(salloc(st, &v.d_keys, (size_t)v.rows * v.D));
    RC(salloc(st, &v.imgs, (size_t)v.B * 3 * v.H * v.W));
    RC(salloc(st, &v.d_imgs, (size_t)v.B * 3 * v.H * v.W));
    // rows no loss kernel ever writes (padding tokens, non-[CLS] rows of d_block) must read as zero gradient
    if (hipMemset(v.d_block, 0, (size_t)v.rows * v.D * sizeof(float)) != hipSuccess || hipMemset(v.d_keys, 0, (size_t)v.rows * v.D * sizeof(float)) != hipSuccess)
        return SPLICE_ERR_HIP;
    v.pb.assign(v.depth, nullptr);
    v.pk.assign(v.depth, nullptr);
    v.pb[v.depth - 1] = v.d_block;
    v.pk[v.depth - 1] = v.d_keys;
    return SPLICE_OK;
}

// blockIdx.x = pair.  raw_k = fixed-order sum of term k's workgroup partials (no float atomics anywhere: replicas are
// bit-reproducible); total = sum_k lambda_k * raw_k   (util/losses.py:53-71)
// n_a / n_b / n_c / n_e > 1 (crops mode): pair p's structure / identity / appearance / entire-image terms are the slots [p n, (p + 1) n) of the
// term's images, added in crop order (util/losses.py:75-82 `loss +=`); one pair: n_a = n_b = n_c = n_e = the slot count.
// wtab (optional, [pairs][5] in the order of splice_step_set_pair_weights): per-pair lambdas in place of the five weights, gated as the
// scalar weights are (ssim_on: global structure and identity; entire: the two entire-image terms)
// MONITOR (the plateau stop rule, plateau.h): thread 0 then runs the rule for its pair on the total it has just written, on counted steps
// -- ssim_on && !entire, both baked per graph variant -- with the step index read from dev_t (step_idx + 1: a replayed graph sees its own
// step).  kb / means (keep-best; null: off): the rule's record and window means of every pair.  The instance without MONITOR does not read
// the five trailing arguments: its code is what it was.
// TRACE (the loss trace): thread 0 also stores the six values of the out8 row, with their bits, into words 0-5 of row
// *dev_t - 1 of the pair's trace ([capacity][pairs][8]; words 6-7 belong to grad_clip_coef_kernel) -- unless the row lies beyond
// capacity or, with MONITOR, the slot stopped at an earlier step (read before this step's rule runs: the stop step's own row is
// written).  The instances without TRACE do not read the two trailing arguments.
// LRP (the plateau lr rule; only with MONITOR): thread 0 runs lr_plateau_step in place of the bare stop rule -- at
// EVERY step it writes lr_eff[pair] = lr_in[pair * lr_in_stride] * scale (lr_in: the staged per-pair table, stride 1, or the one staged
// lr, stride 0), on counted steps the stop rule follows and the pair's lr record takes its verdict.  The instances without LRP do not
// read the six trailing arguments.
// IMG (the image-space terms): two waves more own terms 6 (total variation, the pair's n_a slots) and 7 (pixel identity,
// its n_b slots); their raw sums go to words 6-7 of the row and of out8 and into the total as fmaf(w_pix, raw_7, fmaf(w_tv, raw_6, total of
// the five)).  The two weights are not in wtab: a sweep's slots share them.  The instances without IMG do not read the two trailing
// arguments and launch with 320 threads, as before.
// LYR (the structure terms over the keys of several ViT blocks): a slot's partials of terms 1 and 2 are n_layers
// ranges of tiles_g / tiles_e slots, one per layer in ascending order.  Each range is added in slot order (ssim_layer_sum, the function
// splice_step_ssim_layer_values reports with), the layers' sums in ascending order, the pair's crops in crop order as before -- so with
// one crop per pair the reported word IS the float32 sum of the reported per-layer values.  The instances without LYR do not read the
// three trailing arguments.
// KG (the key second-moment appearance term): the pair's raw value is read from the term's own buffer, kg_values
// [pairs] (the finish launch of key_gram.hip has summed it), and enters the total last: fmaf(w_kg, raw, total of everything before).  No word
// of the row but word 0 moves.  The instances without KG do not read the two trailing arguments.
__device__ __forceinline__ float ssim_layer_sum(const float* part, int tiles) {
    float acc = 0.f;
    for (int i = 0; i < tiles; ++i) acc += part[i];
    return acc;
}
// NN (the nearest-neighbour key appearance term): its raw value, nn_values[pair] (the finish launch of key_nn.hip), enters
// behind that: fmaf(w_nn, raw, total).  With the key second-moment term off the step launches the KG instance on this term's weight and
// buffer -- the same one fused multiply-add, no new code; with both on, total_loss_nn_kernel below: the same body
// (total_loss_body.h, included into both) with KG and NN, two arguments more.  total_loss_kernel keeps its name, its arguments and its code.
template <bool MONITOR, bool TRACE, bool LRP = false, bool IMG = false, bool LYR = false, bool KG = false>
__global__ __launch_bounds__(IMG ? 448 : 320) void total_loss_kernel(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls,
                                                         float w_id, float* out8, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on,
                                                         int entire, splice_stop_state* stop, const int* dev_t, StopRule rule, splice_best_state* kb,
                                                         float* means, float* trace, int capacity, LrRule lr_rule, splice_lr_state* lr_state, int* lr_cuts,
                                                         const float* lr_in, int lr_in_stride, float* lr_eff, float w_tv, float w_pix, int n_layers,
                                                         int tiles_g, int tiles_e, float w_kg, const float* kg_values) {
    constexpr bool NN = false;
    constexpr float w_nn = 0.f;
    constexpr const float* nn_values = nullptr;
#include "total_loss_body.h"
}
// the instance of a step with both key terms
template <bool MONITOR, bool TRACE, bool LRP = false, bool IMG = false, bool LYR = false>
__global__ __launch_bounds__(IMG ? 448 : 320) void total_loss_nn_kernel(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls,
                                                            float w_id, float* out8, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on,
                                                            int entire, splice_stop_state* stop, const int* dev_t, StopRule rule, splice_best_state* kb,
                                                            float* means, float* trace, int capacity, LrRule lr_rule, splice_lr_state* lr_state, int* lr_cuts,
                                                            const float* lr_in, int lr_in_stride, float* lr_eff, float w_tv, float w_pix, int n_layers,
                                                            int tiles_g, int tiles_e, float w_kg, const float* kg_values, float w_nn, const float* nn_values) {
    constexpr bool KG = true, NN = true;
#include "total_loss_body.h"
}
// the rule alone on a caller's [pairs][8] losses (splice_plateau_update): one thread per slot
__global__ __launch_bounds__(64) void plateau_update_kernel(splice_stop_state* stop, const float* losses8, int pairs, StopRule rule, int step_idx,
                                                            splice_best_state* kb, float* means) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p < pairs)
        plateau_update(stop + p, losses8[(size_t)p * 8], rule, step_idx, kb ? kb + p : nullptr, means ? means + (size_t)p * SPLICE_STOP_HISTORY : nullptr);
}
// the six trailing arguments of a total_loss_kernel launch without the plateau lr rule
#define NO_LR_RULE LrRule{}, (splice_lr_state*)nullptr, (int*)nullptr, (const float*)nullptr, 0, (float*)nullptr
// the two trailing arguments behind them of a launch without the image-space terms
#define NO_IMG_TERMS 0.f, 0.f
// the three trailing arguments behind those of a launch without structure layers
#define NO_SSIM_LAYERS 0, 0, 0
// the two trailing arguments behind those of a launch without the key second-moment term
#define NO_KEY_GRAM 0.f, (const float*)nullptr
// the step's instance by what the handle carries (the lr rule rides on the stop rule)
using TotalLossKernel = decltype(&total_loss_kernel<false, false>);
template <bool IMG, bool LYR = false, bool KG = false>
static TotalLossKernel total_loss_instance(bool lr_rule, bool trace, bool stop) {
    return lr_rule ? (trace ? total_loss_kernel<true, true, true, IMG, LYR, KG> : total_loss_kernel<true, false, true, IMG, LYR, KG>)
           : trace ? (stop ? total_loss_kernel<true, true, false, IMG, LYR, KG> : total_loss_kernel<false, true, false, IMG, LYR, KG>)
                   : (stop ? total_loss_kernel<true, false, false, IMG, LYR, KG> : total_loss_kernel<false, false, false, IMG, LYR, KG>);
}
// ... and by the step's terms: the image-space terms, structure layers, the key second-moment term
template <bool KG>
static TotalLossKernel total_loss_for(bool img, bool layered, bool lr_rule, bool trace, bool stop) {
    return layered ? (img ? total_loss_instance<true, true, KG>(lr_rule, trace, stop) : total_loss_instance<false, true, KG>(lr_rule, trace, stop))
                   : (img ? total_loss_instance<true, false, KG>(lr_rule, trace, stop) : total_loss_instance<false, false, KG>(lr_rule, trace, stop));
}
using TotalLossNnKernel = decltype(&total_loss_nn_kernel<false, false>);
template <bool IMG, bool LYR>
static TotalLossNnKernel total_loss_nn_instance(bool lr_rule, bool trace, bool stop) {
    return lr_rule ? (trace ? total_loss_nn_kernel<true, true, true, IMG, LYR> : total_loss_nn_kernel<true, false, true, IMG, LYR>)
           : trace ? (stop ? total_loss_nn_kernel<true, true, false, IMG, LYR> : total_loss_nn_kernel<false, true, false, IMG, LYR>)
                   : (stop ? total_loss_nn_kernel<true, false, false, IMG, LYR> : total_loss_nn_kernel<false, false, false, IMG, LYR>);
}
static TotalLossNnKernel total_loss_nn_for(bool img, bool layered, bool lr_rule, bool trace, bool stop) {
    return layered ? (img ? total_loss_nn_instance<true, true>(lr_rule, trace, stop) : total_loss_nn_instance<false, true>(lr_rule, trace, stop))
                   : (img ? total_loss_nn_instance<true, false>(lr_rule, trace, stop) : total_loss_nn_instance<false, false>(lr_rule, trace, stop));
}
// one thread per (layer, pair): the pair's crops' sums of layer i's slot range of `term`, added in crop order (splice_step_ssim_layer_values)
__global__ __launch_bounds__(64) void ssim_layer_values_kernel(const float* lbase, size_t lstride, int lp, int term, int n_layers, int tiles, int pairs,
                                                               int n_slots, float* out) {
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id >= n_layers * pairs) return;
    const int i = id / pairs, p = id % pairs;
    float tot = 0.f;
    for (int slot = 0; slot < n_slots; ++slot)
        tot += ssim_layer_sum(lbase + ((size_t)p * n_slots + slot) * lstride + 8 + (size_t)term * lp + (size_t)i * tiles, tiles);
    out[id] = tot;
}
// the two rules alone on a caller's [pairs][8] losses (splice_plateau_update_lr): one thread per slot, the loss kernel's device function
__global__ __launch_bounds__(64) void plateau_update_lr_kernel(splice_stop_state* stop, splice_lr_state* lr_state, int* lr_cuts, const float* losses8, int pairs,
                                                               StopRule rule, LrRule lr_rule, int step_idx, int counted, const float* lr_in, int lr_in_stride,
                                                               float* lr_eff) {
    const int p = blockIdx.x * 64 + threadIdx.x;
    if (p < pairs)
        lr_plateau_step(stop + p, lr_state + p, lr_cuts + (size_t)p * SPLICE_STOP_HISTORY, losses8[(size_t)p * 8], counted != 0, rule, lr_rule, step_idx,
                        lr_in[(size_t)p * lr_in_stride], lr_eff + p);
}
static bool lr_rule_ok(float factor, int patience, float min_scale, const char* who) {
    if (factor > 0.f && factor < 1.f && patience >= 1 && min_scale >= 0.f && min_scale < 1.f) return true;
    splice_set_error("%s: needs 0 < factor < 1, patience >= 1 and 0 <= min_scale < 1, got %g, %d, %g", who, (double)factor, patience, (double)min_scale);
    return false;
}
static bool stop_rule_ok(int window, float rel, int patience, int min_steps, const char* who) {
    if (window >= 0 && rel > 0.f && rel < 1.f && patience >= 1 && min_steps >= 0) return true;
    splice_set_error("%s: needs window >= 0, 0 < rel < 1, patience >= 1 and min_steps >= 0", who);
    return false;
}
// All per-step inputs in ONE eager launch in front of the graph replay (three copies + the Adam step count were four
// launches with ~10-30 us of host/queue gaps between them): up to three fp32 buffers, one int and (fp != null) nf floats, the
// scheduled learning rate (nf = 1) or one per pair (splice_step_set_pair_lr).
struct StageArgs { const float* src[3]; float* dst[3]; unsigned long long n[3]; int* ip; int iv; float* fp; int nf; float fv[SPLICE_STEP_MAX_PAIR_CFGS]; };
__global__ __launch_bounds__(256) void stage_inputs_kernel(StageArgs a) {
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!a.src[k]) continue;
        const size_t n4 = a.n[k] / 4;   // vector body + scalar tail
        const float4* s4 = reinterpret_cast<const float4*>(a.src[k]);
        float4* d4 = reinterpret_cast<float4*>(a.dst[k]);
        const bool vec = ((reinterpret_cast<size_t>(a.src[k]) | reinterpret_cast<size_t>(a.dst[k])) & 15) == 0;
        if (vec) {
            for (size_t i = gid; i < n4; i += stride) d4[i] = s4[i];
            for (size_t i = n4 * 4 + gid; i < a.n[k]; i += stride) a.dst[k][i] = a.src[k][i];
        } else {
            for (size_t i = gid; i < a.n[k]; i += stride) a.dst[k][i] = a.src[k][i];
        }
    }
    if (gid == 0) {
        *a.ip = a.iv;
        if (a.fp) {
#pragma unroll
            for (int k = 0; k < SPLICE_STEP_MAX_PAIR_CFGS; ++k)
                if (k < a.nf) a.fp[k] = a.fv[k];
        }
    }
}
// The gather form of the staging launch (splice_step_set_input_rows): the caller's batches hold pairs_in pairs, the handle's pair
// blockIdx.y takes the block of pair rows[blockIdx.y] -- blk[k] floats of buffer k: its nA A crops, its nB B crops, its one entire
// image.  The staged buffers hold the bytes the flat form would have been handed.  A kernel of its own: stage_inputs_kernel, which
// every handle without a row table launches, keeps its instructions.  16-byte loads and stores when a pair's block is a multiple of 4
// floats and both base pointers are aligned (then every pair's block is), else the scalar path, as the flat kernel.
struct StageRowsArgs { StageArgs a; unsigned long long blk[3]; int rows[SPLICE_STEP_MAX_PAIR_CFGS]; };
__global__ __launch_bounds__(256) void stage_inputs_rows_kernel(StageRowsArgs r) {
    const StageArgs& a = r.a;
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x, stride = (size_t)gridDim.x * 256;
    const size_t row = (size_t)r.rows[blockIdx.y];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!a.src[k]) continue;
        const size_t n = r.blk[k];
        const float* src = a.src[k] + row * n;
        float* dst = a.dst[k] + (size_t)blockIdx.y * n;
        const bool vec = (n & 3) == 0 && ((reinterpret_cast<size_t>(a.src[k]) | reinterpret_cast<size_t>(a.dst[k])) & 15) == 0;
        if (vec) {
            const float4* s4 = reinterpret_cast<const float4*>(src);
            float4* d4 = reinterpret_cast<float4*>(dst);
            for (size_t i = gid; i < n / 4; i += stride) d4[i] = s4[i];
        } else {
            for (size_t i = gid; i < n; i += stride) dst[i] = src[i];
        }
    }
    if (gid == 0 && blockIdx.y == 0) {
        *a.ip = a.iv;
        if (a.fp) {
#pragma unroll
            for (int k = 0; k < SPLICE_STEP_MAX_PAIR_CFGS; ++k)
                if (k < a.nf) a.fp[k] = a.fv[k];
        }
    }
}
static int tri_tiles(int T) { const int nt = (T + 63) / 64; return nt * (nt + 1) / 2; }   // upper-triangular 64 x 64 tiles of a [T][T] matrix
static float* loss_part(SpliceStep* st, int slot) { return st->losses + 8 + (size_t)slot * st->lp; }   // pair 0; pair p at + p * lstride

// `n_img` images [3][h][w] -> [3][oh][ow] each (contiguous batches on both sides)
static int place_images(const float* src, int h, int w, float* dst, int oh, int ow, int n_img, hipStream_t s) {
    if (src == dst) return SPLICE_OK;   // identity Resize with the producer writing the ViT context's image slot itself (step_ptrs)
    if (h == oh && w == ow) {   // Resize returns its input when the shorter edge already matches
        RC(dev_copy_launch(dst, src, (size_t)n_img * 3 * h * w * sizeof(float), s));
        return SPLICE_OK;
    }
    return resize_bilinear_fwd_launch(src, dst, 3 * n_img, h, w, oh, ow, s);
}
static int unplace_grads(const float* dsrc, int oh, int ow, float* ddst, int h, int w, int n_img, hipStream_t s) {
    if (dsrc == ddst) return SPLICE_OK;
    if (h == oh && w == ow) {
        RC(dev_copy_launch(ddst, dsrc, (size_t)n_img * 3 * h * w * sizeof(float), s));
        return SPLICE_OK;
    }
    return resize_bilinear_bwd_launch(dsrc, ddst, 3 * n_img, h, w, oh, ow, s);
}

// Where the step's images live.  With an identity Resize (crop size == ViT input size: the benchmark's 224 x 224 pair, and
// every size-matched crop of train_model) the staged inputs, the generator outputs and their gradients ARE the image slots
// of the ViT context -- the generator reads and writes them in place, no copy kernels on either chain (4 + 2 launches per
// step, 3 of them on the critical chain).  Otherwise the private buffers + resize_bilinear_* as before.
struct StepPtrs { float *a_in, *b_in, *e_in, *x, *y, *xe, *dx, *dy, *dxe; };
static StepPtrs step_ptrs(SpliceStep* st) {
    const splice_step_config& c = st->cfg;
    VitView& vg = st->vg;
    const size_t vimg = (size_t)3 * vg.H * vg.W;
    const int pA = 0, pB = st->Pa, pX = st->Pa + st->Pb, pY = 2 * st->Pa + st->Pb;
    const bool ida = c.crop_h == vg.H && c.crop_w == vg.W, idb = st->cropb_h == vg.H && st->cropb_w == vg.W;
    StepPtrs p;
    p.a_in = ida ? vg.imgs + pA * vimg : st->gen_in;
    p.x = ida ? vg.imgs + pX * vimg : st->gen_out;
    p.dx = ida ? vg.d_imgs + pX * vimg : st->d_gen_out;
    p.b_in = idb ? vg.imgs + pB * vimg : st->in_b;
    p.y = idb ? vg.imgs + pY * vimg : st->gen_out_b;
    p.dy = idb ? vg.d_imgs + pY * vimg : st->d_gen_out_b;
    p.e_in = st->ent_in; p.xe = st->ent_out; p.dxe = st->d_ent_out;
    if (st->plan_e) {
        VitView& ve = st->ve;
        if (c.ent_h == ve.H && c.ent_w == ve.W) {
            const size_t eimg = (size_t)3 * ve.H * ve.W;
            p.e_in = ve.imgs; p.xe = ve.imgs + st->pairs * eimg; p.dxe = ve.d_imgs + st->pairs * eimg;
        }
    }
    return p;
}

// fp32 keys of pass b (view into the last layer's raw qkv): pointer + leading dimension 3D
static const float* keys_ptr(const VitView& v, const float* qkv_last, int pass) { return qkv_last + (size_t)pass * v.Tld * 3 * v.D + v.D; }

// What one step does about each loss term (index L_*), decided once per step_body from the lambda schedule (ssim_on, entire) and either cfg's
// scalar lambdas or the per-pair tables.  on: the term's kernels launch (per-pair: when any pair needs them; a pair whose weight is 0
// returns early in the kernel).  lambda: the scalar weight, 0 when the schedule gates the term off.  tab: the term's PW_* row, or null.
struct Term { bool on; float lambda; const float* tab; };
static void step_terms(const SpliceStep* st, bool ssim_on, bool entire, Term t[L_TERMS]) {
    const splice_step_config& c = st->cfg;
    const float lambda[L_TERMS] = {0.f, c.lambda_global_ssim, c.lambda_entire_ssim, c.lambda_entire_cls, c.lambda_global_cls, c.lambda_global_identity};
    const bool sched[L_TERMS] = {false, ssim_on, entire, entire, true, ssim_on};
    for (int k = 1; k < L_TERMS; ++k) {
        t[k].lambda = sched[k] ? lambda[k] : 0.f;
        t[k].on = st->pw ? sched[k] && st->pw_any[TERM_LAM[k]] : t[k].lambda > 0.f;
        t[k].tab = st->pw ? st->pw + (size_t)TERM_ROW[k] * st->P : nullptr;
    }
}

// The structure term of P pairs (util/losses.py:74-83): targets = passes [pass_tgt, pass_tgt + P), generated = passes
// [pass_x, pass_x + P) of view v.  `b` is carved over st->ssim_ws for v's token count.
// `tab` (a handle with splice_step_set_ssim_layers): entry i = the same operands of block ssim_layers[i] -- its qkv and transposed copy, the
// workspace and key-gradient buffer of its own, its weight; the launchers then take every operand pointer from the table.
static int ssim_batch(SpliceStep* st, VitView& v, int pass_tgt, int pass_x, int count, const Term& term, int slot, SelfSimBatch* b,
                      SelfSimLayers* tab = nullptr) {
    bf16_t *qkv = nullptr, *qkvT = nullptr;
    if (tab) {
        tab->n = st->ssim_list.n;
        const size_t pass_rows = (size_t)v.Tld * 3 * v.D;
        for (int i = 0; i < tab->n; ++i) {
            const int l = st->ssim_list.layers[i];
            SelfSimBatch w = {};
            RC(splice_vit_get_tensor(v.ctx, 1, l, (void**)&qkv));
            RC(splice_vit_get_tensor(v.ctx, 8, l, (void**)&qkvT));
            selfsim_batch_carve(st->ssim_ws_layer[i], v.T, v.D, count, &w);
            SelfSimLayer& e = tab->e[i];
            e.k_tgt = qkv + (size_t)pass_tgt * pass_rows + v.D;
            e.k_x = qkv + (size_t)pass_x * pass_rows + v.D;
            e.kT_x = qkvT + (size_t)v.D * v.rows + (size_t)pass_x * v.Tld;
            e.S_tgt = w.S_tgt; e.wmat = w.wmat; e.norm_x = w.norm_x; e.rpart = w.rpart;
            e.dk = v.dk_layer[i] + (size_t)pass_x * v.Tld * v.D;
            e.weight = st->ssim_list.weights[i];
        }
    }
    RC(splice_vit_get_tensor(v.ctx, 1, v.depth - 1, (void**)&qkv));
    RC(splice_vit_get_tensor(v.ctx, 6, v.depth - 1, (void**)&qkvT));
    selfsim_batch_carve(st->ssim_ws, v.T, v.D, count, b);
    const size_t pass_rows = (size_t)v.Tld * 3 * v.D;
    b->ldk = 3 * v.D; b->ldt = v.rows; b->k_pstride = pass_rows; b->kT_pstride = (size_t)v.Tld;
    b->k_tgt = qkv + (size_t)pass_tgt * pass_rows + v.D;
    b->k_x = qkv + (size_t)pass_x * pass_rows + v.D;
    b->kT_x = qkvT + (size_t)v.D * v.rows + (size_t)pass_x * v.Tld;
    b->loss_part = loss_part(st, slot); b->part_pstride = st->lstride;
    b->dk = v.d_keys + (size_t)pass_x * v.Tld * v.D; b->dk_pstride = (size_t)v.Tld * v.D; b->lddk = v.D;
    b->eps = 1e-8f;
    b->fp8 = st->cfg.fp8_selfsim && v.D % 128 == 0;
    b->loss_scale = 1.0f / ((float)v.T * (float)v.T);
    b->e_scale = 4.0f * term.lambda * b->loss_scale;
    b->e_scale_tab = term.tab;
    return SPLICE_OK;
}

// The appearance term over the handle's [CLS] layers (splice_step_set_cls_layers): the table of one launch.  Generated rows: passes pass_x,
// pass_x + x_step, ... of view vx; targets: passes pass_t, pass_t + t_step, ... of the global view.  Entry i reads block cls_layers[i]'s output
// on both sides and seeds the view's buffer of that block -- the top block row 0 of d_block, as the plain path does.
static int cls_table(SpliceStep* st, VitView& vx, int pass_x, int x_step, int pass_t, int t_step, ClsLayers* tab) {
    VitView& vg = st->vg;
    const size_t xpass = (size_t)vx.Tld * vx.D, tpass = (size_t)vg.Tld * vg.D;
    tab->n = st->cls_list.n; tab->D = vx.D;
    tab->x_ps = (size_t)x_step * xpass; tab->t_ps = (size_t)t_step * tpass; tab->seed_step = x_step;
    for (int i = 0; i < tab->n; ++i) {
        float *bx = nullptr, *bt = nullptr;
        RC(splice_vit_get_tensor(vx.ctx, 0, st->cls_list.layers[i], (void**)&bx));
        RC(splice_vit_get_tensor(vg.ctx, 0, st->cls_list.layers[i], (void**)&bt));
        ClsLayer& e = tab->e[i];
        e.x = bx + (size_t)pass_x * xpass; e.tgt = bt + (size_t)pass_t * tpass;
        if (vx.cls_seed[i]) { e.seed = vx.cls_seed[i] + (size_t)pass_x * vx.D; e.seed_ps = (size_t)vx.D; }
        else { e.seed = vx.d_block + (size_t)pass_x * xpass; e.seed_ps = xpass; }
        e.weight = st->cls_list.weights[i];
    }
    return SPLICE_OK;
}

// The identity term over the handle's identity layers (splice_step_set_id_layers): the table of its two launches.  Generated keys: the y'
// passes pass_y, pass_y + 1, ... of the global view; targets: its B' passes from pass_b on.  The top block's entry points into the key
// columns of qkv_last_f32 (ld 3D) and d_keys, as the plain path does; a lower block's into its [rows][D] fp32 key buffer and its
// key-gradient buffer.
static int id_table(SpliceStep* st, int pass_y, int pass_b, IdLayers* tab) {
    VitView& v = st->vg;
    tab->n = st->id_list.n; tab->T = v.T; tab->D = v.D;
    tab->x_rs = tab->t_rs = tab->g_rs = (size_t)v.Tld;
    for (int i = 0; i < tab->n; ++i) {
        const int l = st->id_list.layers[i];
        IdLayer& e = tab->e[i];
        float* k = nullptr;
        if (l == v.depth - 1) {
            RC(splice_vit_get_tensor(v.ctx, 3, l, (void**)&k));
            e.x = keys_ptr(v, k, pass_y); e.tgt = keys_ptr(v, k, pass_b); e.ldx = e.ldt = 3 * v.D;
        } else {
            RC(splice_vit_get_tensor(v.ctx, 9, l, (void**)&k));
            e.x = k + (size_t)pass_y * v.Tld * v.D; e.tgt = k + (size_t)pass_b * v.Tld * v.D; e.ldx = e.ldt = v.D;
        }
        e.grad = v.dk_id[i] + (size_t)pass_y * v.Tld * v.D; e.ldg = v.D;
        e.weight = st->id_list.weights[i];
    }
    return SPLICE_OK;
}

extern "C" {

int splice_step_create(const splice_step_config* cfg, void* vit_ctx_global, void* vit_ctx_entire, void* gen_plan_a, void* gen_plan_b,
                       void* gen_plan_entire, void** out) {
    if (!cfg || !vit_ctx_global || !gen_plan_a || !gen_plan_b || !out) return SPLICE_ERR_ARG;
    // every failure below leaves through splice_step_destroy, which frees whatever exists of the half-built handle by then
    std::unique_ptr<SpliceStep, void (*)(void*)> guard(new SpliceStep(), splice_step_destroy);
    SpliceStep* st = guard.get();
    st->cfg = *cfg;
    st->crops_mode = cfg->n_crops > 1 || cfg->n_crops_b > 1;
    const int pairs = st->pairs = cfg->pairs > 1 ? cfg->pairs : 1;
    // crops mode: the reference zips the crop lists (util/losses.py:76,87,98) -- the structure term runs over the A crops, the
    // identity term over the B crops, the appearance term over min(nA, nB) pairs -- while netG's BatchNorm sees every crop of
    // its call (models/model.py:15-23): the two plans may hold different numbers of images
    const int nb_crops = cfg->n_crops_b > 0 ? cfg->n_crops_b : cfg->n_crops;
    if (st->crops_mode && (nb_crops < 1 || nb_crops > 8 || cfg->n_crops > 8)) { splice_set_error("splice_step_create: 1..8 crops per side"); return SPLICE_ERR_ARG; }
    // several pairs with n_crops > 1 each: pair p's crops are images [p n, (p + 1) n) of each side, one netG call per pair (grouped plans)
    const int na = st->na = st->crops_mode ? cfg->n_crops : 1, nb = st->nb = st->crops_mode ? nb_crops : 1;
    if (st->crops_mode && pairs > 1 && pairs * (na > nb ? na : nb) > SPLICE_STEP_MAX_GROUP_IMAGES) {
        splice_set_error("splice_step_create: %d pairs x %d crops = %d images per side, at most %d", pairs, na > nb ? na : nb, pairs * (na > nb ? na : nb),
                         SPLICE_STEP_MAX_GROUP_IMAGES);
        return SPLICE_ERR_ARG;
    }
    const int Pa = st->Pa = pairs * na;
    const int Pb = st->Pb = pairs * nb;
    const int P = st->P = Pa > Pb ? Pa : Pb;
    st->max_crop_h = cfg->crop_h; st->max_crop_w = cfg->crop_w;
    st->cropb_h = cfg->crop_h; st->cropb_w = cfg->crop_w;
    int rc = SPLICE_OK;   // (plain returns, not RC(): the callee's message stays the last error)
    if ((rc = view_init(st, st->vg, vit_ctx_global, 2 * (Pa + Pb))) != SPLICE_OK) return rc;
    if (st->vg.H != cfg->vit_h || st->vg.W != cfg->vit_w) { splice_set_error("splice_step_create: global ViT context shape mismatch"); return SPLICE_ERR_ARG; }
    int n, h, w;
    for (int k = 0; k < 2; ++k) {
        void* plan = k ? gen_plan_b : gen_plan_a;
        const int want = k ? Pb : Pa;
        if ((rc = splice_gen_plan_dims(plan, &n, &h, &w, &st->nparams)) != SPLICE_OK) return rc;
        if (n != want || h != cfg->crop_h || w != cfg->crop_w) { splice_set_error("splice_step_create: the crop generator plans must hold %d / %d image(s) at the crop size", Pa, Pb); return SPLICE_ERR_ARG; }
    }
    st->plan_a = gen_plan_a; st->plan_b = gen_plan_b;
    if (pairs > 1) {
        if (cfg->arena_stride < st->nparams) { splice_set_error("splice_step_create: pairs > 1 needs arena_stride >= the parameter count"); return SPLICE_ERR_ARG; }
        st->astride = (size_t)cfg->arena_stride;
    }
    const size_t crop = (size_t)3 * cfg->crop_h * cfg->crop_w;
    for (float** q : {&st->gen_in, &st->in_b, &st->gen_out, &st->gen_out_b, &st->d_gen_out, &st->d_gen_out_b})
        if ((rc = salloc(st, q, P * crop)) != SPLICE_OK) return rc;
    if ((rc = salloc(st, &st->grads_b, arena_floats(st))) != SPLICE_OK) return rc;
    // the backward writes nparams floats per pair; the <= 63 floats of padding between two arenas are read by the whole-range
    // add / Adam and must never hold garbage
    if (hipMemset(st->grads_b, 0, arena_floats(st) * sizeof(float)) != hipSuccess) return SPLICE_ERR_HIP;
    int Tmax = st->vg.T;
    if (cfg->ent_h > 0) {   // the entire-image branch: one image per pair (netG(A) is one image in crops mode too)
        if (!vit_ctx_entire || !gen_plan_entire) { splice_set_error("splice_step_create: entire-image branch needs its ViT context and generator plan"); return SPLICE_ERR_ARG; }
        if ((rc = view_init(st, st->ve, vit_ctx_entire, 2 * pairs)) != SPLICE_OK) return rc;
        if (st->ve.H != cfg->ent_vit_h || st->ve.W != cfg->ent_vit_w) { splice_set_error("splice_step_create: entire ViT context shape mismatch"); return SPLICE_ERR_ARG; }
        if ((rc = splice_gen_plan_dims(gen_plan_entire, &n, &h, &w, nullptr)) != SPLICE_OK) return rc;
        if (n != pairs || h != cfg->ent_h || w != cfg->ent_w) { splice_set_error("splice_step_create: the entire generator plan must hold %d image(s) at the entire-image size", pairs); return SPLICE_ERR_ARG; }
        st->plan_e = gen_plan_entire;
        const size_t ent = (size_t)3 * cfg->ent_h * cfg->ent_w;
        for (float** q : {&st->ent_in, &st->ent_out, &st->d_ent_out})
            if ((rc = salloc(st, q, pairs * ent)) != SPLICE_OK) return rc;
        if (st->ve.T > Tmax) Tmax = st->ve.T;
    }
    char* wsb = nullptr;
    if ((rc = salloc(st, &wsb, selfsim_batch_ws_bytes(Tmax, st->vg.D, P))) != SPLICE_OK) return rc;
    st->ssim_ws = wsb;
    {   // per-term partial slots: the MSE kernels use up to SPLICE_MSE_PARTIALS workgroups, the structure term one per upper-triangular tile
        const size_t nt = (Tmax + 63) / 64, tri = nt * (nt + 1) / 2;
        st->lp = tri > SPLICE_MSE_PARTIALS ? tri : SPLICE_MSE_PARTIALS;
        st->lstride = 8 + 8 * st->lp;
    }
    if ((rc = salloc(st, &st->losses, P * st->lstride)) != SPLICE_OK) return rc;
    if ((rc = salloc(st, &st->dev_t, 4)) != SPLICE_OK) return rc;
    if ((rc = salloc(st, &st->dev_lr, 1)) != SPLICE_OK) return rc;
    if ((rc = salloc(st, &st->stop, (size_t)pairs)) != SPLICE_OK) return rc;
    {
        const std::vector<splice_stop_state> z((size_t)pairs, splice_stop_state{0.f, 0, 0, 0.f, 0, -1});
        if (hipMemcpy(st->stop, z.data(), z.size() * sizeof(splice_stop_state), hipMemcpyHostToDevice) != hipSuccess) return SPLICE_ERR_HIP;
    }
    if (P > 1 && !st->crops_mode) {
        if ((rc = salloc(st, &st->dev_lrs, SPLICE_STEP_MAX_PAIR_CFGS)) != SPLICE_OK) return rc;
        if ((rc = salloc(st, &st->pw_tab_alloc, (size_t)PW_ROWS * P)) != SPLICE_OK) return rc;
    }
    st->opt_hp0 = cfg->beta1; st->opt_hp1 = cfg->beta2; st->opt_eps = cfg->eps;
    if (const char* e = getenv("SPLICE_STEP_GRAPH")) st->use_graph = atoi(e);
    if (const char* e = getenv("SPLICE_STEP_SYNC")) st->dbg_sync = atoi(e);
    if (const char* e = getenv("SPLICE_STEP_OVERLAP")) st->overlap = atoi(e);
#ifdef SPLICE_DEV_SWITCHES   // scratch builds only (make DEV=1): the work-skipping timing switch is not part of the product library
    if (const char* e = getenv("SPLICE_STEP_ABLATE")) st->ablate = atoi(e);
#endif
    if (hipStreamCreateWithFlags(&st->own_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&st->side_stream, hipStreamNonBlocking) != hipSuccess ||
        !create_events(st)) {
        splice_set_error("splice_step_create: stream/event creation failed");
        return SPLICE_ERR_HIP;
    }
    *out = guard.release();
    return SPLICE_OK;
}

// (also the teardown of a handle whose creation failed half-way: every member is null until it exists)
void splice_step_destroy(void* h) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return;
    st->graphs.retire();
    if (st->own_stream) { (void)hipStreamSynchronize(st->own_stream); (void)hipStreamDestroy(st->own_stream); }
    if (st->side_stream) { (void)hipStreamSynchronize(st->side_stream); (void)hipStreamDestroy(st->side_stream); }
    for (auto& set : st->evs)
        for (hipEvent_t e : set)
            if (e) (void)hipEventDestroy(e);
    for (void* q : st->allocs) (void)hipFree(q);
    delete st;
}

// Pointers to the generator outputs of the last step (device, valid until the next run):
// which 0: x_global [P][3][a_h][a_w], 1: x_entire [P][3][ent_h][ent_w], 2: y_global [P][3][b_h][b_w]
int splice_step_output(void* h, int which, float** out) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || !out) return SPLICE_ERR_ARG;
    const StepPtrs p = step_ptrs(st);
    *out = which == 0 ? p.x : which == 1 ? p.xe : which == 2 ? p.y : nullptr;
    return *out ? SPLICE_OK : SPLICE_ERR_STATE;
}

// Crop sizes of the NEXT steps (<= the creation size): the reference's data feed draws size ~ U(min_cover*h, h) per step
// and image (data/transforms.py:21-22, data/Dataset.py:66-67); the ViT input size (after Resize) is unchanged for square
// crops.  All pairs of a batch share the two sizes.
int splice_step_set_crops(void* h, int a_h, int a_w, int b_h, int b_w) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (a_h > st->max_crop_h || a_w > st->max_crop_w || b_h > st->max_crop_h || b_w > st->max_crop_w) { splice_set_error("splice_step_set_crops: larger than the creation size"); return SPLICE_ERR_ARG; }
    RC(splice_gen_plan_resize(st->plan_a, a_h, a_w));
    RC(splice_gen_plan_resize(st->plan_b, b_h, b_w));
    st->cfg.crop_h = a_h; st->cfg.crop_w = a_w; st->cropb_h = b_h; st->cropb_w = b_w;
    return SPLICE_OK;
}

// The first rule the handle carries that rides in its own update, so that it runs whole steps only (neither gradient-only nor phase
// mode), named for an error text; null: none.
static const char* whole_step_rule(const SpliceStep* st) {
    return st->stop_rule.window > 0 ? "with a stop rule" : st->ema ? "with a weight average" : st->clip ? "with gradient clipping"
           : st->best ? "that keeps the best weights" : st->trace ? "with a loss trace"
           : (st->lambda_tv > 0.f || st->lambda_pix > 0.f) ? "with image-space loss terms"
           : st->ssim_list.n > 0 ? "with structure layers" : st->cls_list.n > 0 ? "with [CLS] layers"
           : st->id_list.n > 0 ? "with identity layers" : st->kg_lambda > 0.f ? "with the key second-moment term"
           : st->nn_lambda > 0.f ? "with the nearest-neighbour key term" : nullptr;
}
// The shared opening of the rule setters below: before the first step only (`what` of the rule, for the error text), and not on a
// gradient-only or phase-mode handle.  Callers return its code plainly, not through RC(): the message stays the last error.
static int rule_setter_ok(const SpliceStep* st, const char* who, const char* what) {
    if (st->runs > 0) { splice_set_error("%s: %s before the first step", who, what); return SPLICE_ERR_STATE; }
    if (st->skip_adam || st->phases != 7 || st->leader) {
        splice_set_error("%s: not on a handle in gradient-only (splice_step_set_mode) or phase mode (splice_step_set_phases)", who);
        return SPLICE_ERR_STATE;
    }
    return SPLICE_OK;
}

// skip_adam != 0: the step stops after backward -- `grads` holds the gradient of this step's loss (+= its previous content
// when accumulate != 0) and the parameters are untouched; the caller sums several losses that way (e.g. the same crops seen
// at several ViT input scales) and applies splice_adam_step once.
int splice_step_set_mode(void* h, int skip_adam, int accumulate) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || (accumulate && !skip_adam)) return SPLICE_ERR_ARG;
    const char* rule = skip_adam ? whole_step_rule(st) : nullptr;
    if (rule) { splice_set_error("splice_step_set_mode: a handle %s runs whole steps (no gradient-only mode)", rule); return SPLICE_ERR_STATE; }
    if (st->skip_adam != (skip_adam ? 1 : 0) || st->accumulate != (accumulate ? 1 : 0)) st->graphs.retire();
    st->skip_adam = skip_adam ? 1 : 0; st->accumulate = accumulate ? 1 : 0;
    return SPLICE_OK;
}
// The optimiser of the step's update (util/util.py:28-39): kind 0 Adam (hp0 = beta1, hp1 = beta2), 1 RMSprop (hp0 = alpha; the v arena
// holds square_avg, m is not touched), 2 SGD (no moment arena).  Default: Adam with cfg.beta1 / beta2 / eps.  A change drops the
// handle's graphs.
int splice_step_set_optimizer(void* h, int kind, float hp0, float hp1, float eps) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || kind < SPLICE_OPT_ADAM || kind > SPLICE_OPT_SGD) return SPLICE_ERR_ARG;
    if (st->opt_kind != kind || st->opt_hp0 != hp0 || st->opt_hp1 != hp1 || st->opt_eps != eps) st->graphs.retire();
    st->opt_kind = kind; st->opt_hp0 = hp0; st->opt_hp1 = hp1; st->opt_eps = eps;
    return SPLICE_OK;
}
// The extended rules of the step's update (include/splice_hip.h states them): the update launch of every later step is the extended instance
// of the handle's kind, with `w` as its third moment arena.  The record is checked by the launcher at the first step (it knows the kind's
// rules); here only what the handle itself needs.  Before the first step only: the moments belong to a run from step 0.
int splice_step_set_optimizer_ext(void* h, const splice_optim_ext* options, float* w) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!options) { splice_set_error("splice_step_set_optimizer_ext: needs the option record"); return SPLICE_ERR_ARG; }
    if ((options->amsgrad || options->centered) && !w) {
        splice_set_error("splice_step_set_optimizer_ext: amsgrad / centered need the w arena");
        return SPLICE_ERR_ARG;
    }
    if (int rc = rule_setter_ok(st, "splice_step_set_optimizer_ext", "the options are set")) return rc;
    st->graphs.retire();
    st->opt_ext_on = 1; st->opt_ext = *options; st->opt_w = w;
    return SPLICE_OK;
}
// The learning rate of the next splice_step_run (a schedule: scheduler.step(), train.py:80).  It is staged into device memory by the
// step's input-staging launch and read by the optimiser kernel, so a captured graph replays with the lr of every step.  Until the
// first call the handle keeps cfg.lr as a kernel argument; the first call drops the handle's graphs.
int splice_step_set_lr(void* h, float lr) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!st->lr_set) st->graphs.retire();
    st->lr_set = 1; st->lr = lr;
    return SPLICE_OK;
}
static int pair_cfgs_ok(SpliceStep* st, const void* host, const char* who) {
    if (!st || !host) return SPLICE_ERR_ARG;
    if (st->P < 2 || st->crops_mode || !st->pw_tab_alloc || st->P > SPLICE_STEP_MAX_PAIR_CFGS) {
        splice_set_error("%s: per-pair configs need 2 .. %d pairs (pairs mode, not n_crops)", who, SPLICE_STEP_MAX_PAIR_CFGS);
        return SPLICE_ERR_ARG;
    }
    return SPLICE_OK;
}
// Per-pair loss weights: lambdas = host [P][5] {global_cls, global_ssim, global_identity, entire_cls, entire_ssim} (LAM_*).  The device tables
// hold what the scalar path computes from cfg, with the same fp32 expressions in the same order: e_scale = 4 lambda * loss_scale of the
// view (ssim_batch), lambda / (float)(rows * cols) of each MSE term (mse_batched_launch), and the lambdas of the total.
int splice_step_set_pair_weights(void* h, const float* lambdas) {
    SpliceStep* st = (SpliceStep*)h;
    RC(pair_cfgs_ok(st, lambdas, "splice_step_set_pair_weights"));
    const int P = st->P;
    for (int i = 0; i < 5 * P; ++i)
        if (!(lambdas[i] >= 0.f)) { splice_set_error("splice_step_set_pair_weights: lambdas must be >= 0"); return SPLICE_ERR_ARG; }
    std::vector<float> t((size_t)PW_ROWS * P, 0.f);
    const VitView &vg = st->vg, &ve = st->ve;
    const float ls_g = 1.0f / ((float)vg.T * (float)vg.T);
    const float ls_e = st->plan_e ? 1.0f / ((float)ve.T * (float)ve.T) : 0.f;
    const size_t n_cls = (size_t)1 * vg.D, n_id = (size_t)vg.T * vg.D, n_ecls = (size_t)1 * ve.D;
    for (int k = 0; k < 5; ++k) st->pw_any[k] = 0;
    for (int p = 0; p < P; ++p) {
        const float* l = lambdas + (size_t)p * 5;
        for (int k = 0; k < 5; ++k) st->pw_any[k] |= l[k] > 0.f;
        t[PW_ESCALE_G * P + p] = 4.0f * l[LAM_SSIM] * ls_g;
        if (st->plan_e) t[PW_ESCALE_E * P + p] = 4.0f * l[LAM_ESSIM] * ls_e;
        t[PW_CLS * P + p] = l[LAM_CLS] / (float)n_cls;
        t[PW_ID * P + p] = l[LAM_ID] / (float)n_id;           // (keys)
        if (st->plan_e) t[PW_ECLS * P + p] = l[LAM_ECLS] / (float)n_ecls;
        for (int k = 0; k < 5; ++k) t[PW_LAMBDAS * P + (size_t)p * 5 + k] = l[k];
    }
    st->graphs.retire();
    HIPCHK(hipDeviceSynchronize());   // (a running step may still read the tables)
    HIPCHK(hipMemcpy(st->pw_tab_alloc, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
    st->pw = st->pw_tab_alloc;
    return SPLICE_OK;
}
// Per-pair learning rates of the next splice_step_run and every later one until the next call (the per-pair form of splice_step_set_lr):
// staged by the input-staging launch, read by the optimiser as lr[element / arena_stride].  The first call drops the handle's graphs.
int splice_step_set_pair_lr(void* h, const float* lr) {
    SpliceStep* st = (SpliceStep*)h;
    RC(pair_cfgs_ok(st, lr, "splice_step_set_pair_lr"));
    if (st->astride % 4) { splice_set_error("splice_step_set_pair_lr: the arena stride must be a multiple of 4"); return SPLICE_ERR_ARG; }
    if (!st->pair_lr) st->graphs.retire();
    st->pair_lr = 1;
    for (int p = 0; p < st->P; ++p) st->lrs[p] = lr[p];
    return SPLICE_OK;
}
// Run only part of a step: phases is a mask of 1 = generator forward (and input staging), 2 = ViT forward, losses and ViT backward
// down to the gradient of the generated images, 4 = generator backward (+ Adam unless splice_step_set_mode says otherwise).
// With `leader` (another step handle, same image shapes; phases must be 2) this handle is a FOLLOWER: it reads the leader's
// staged inputs and generator outputs instead of running the generator, and ADDS its image gradients to the leader's.  That
// is the several-scales step (BASELINE configs[4]) with one generator pass: leader 1|2, followers 2, leader 4 -- the generator
// backward is linear in the image gradient, so backpropagating the sum equals summing the backpropagations.
int splice_step_set_phases(void* h, int phases, void* leader) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || phases <= 0 || phases > 7 || leader == h || (leader && phases != 2) || (leader && ((SpliceStep*)leader)->leader)) return SPLICE_ERR_ARG;
    const char* rule = phases != 7 || leader ? whole_step_rule(st) : nullptr;
    if (rule) { splice_set_error("splice_step_set_phases: a handle %s runs whole steps (no phase mode)", rule); return SPLICE_ERR_STATE; }
    if (st->leader != (SpliceStep*)leader) st->graphs.retire();
    st->phases = phases;
    st->leader = (SpliceStep*)leader;
    return SPLICE_OK;
}

// The plateau stop rule of every pair of the handle (plateau.h; include/splice_hip.h has the rule).  Before the first step only: the state
// records belong to a run from step 0.  Not on a gradient-only or phase-mode handle: the update the rule freezes is not this handle's.
int splice_step_set_stop_rule(void* h, int window, float rel, int patience, int min_steps) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!stop_rule_ok(window, rel, patience, min_steps, "splice_step_set_stop_rule")) return SPLICE_ERR_ARG;
    if (int rc = rule_setter_ok(st, "splice_step_set_stop_rule", "the rule is set")) return rc;
    if (window == 0 && st->best) { splice_set_error("splice_step_set_stop_rule: a handle that keeps the best weights needs its rule (window > 0)"); return SPLICE_ERR_STATE; }
    if (window == 0 && st->lr_state) { splice_set_error("splice_step_set_stop_rule: a handle with the plateau lr rule needs its windows (window > 0)"); return SPLICE_ERR_STATE; }
    if ((window > 0) != (st->stop_rule.window > 0)) st->graphs.retire();
    st->stop_rule = StopRule{window, rel, patience, min_steps};
    return SPLICE_OK;
}
// The weight average of every pair of the handle (include/splice_hip.h has the rule): `ema` is written by the step's optimiser launch.  Before
// the first step only: the average belongs to a run from step 0.  Not on a gradient-only or phase-mode handle: the update it rides in is
// not this handle's.
int splice_step_set_ema(void* h, float* ema, float decay, int start) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!ema || !(decay > 0.f && decay < 1.f) || start < 0) {
        splice_set_error("splice_step_set_ema: needs the ema arena, 0 < decay < 1 and start >= 0");
        return SPLICE_ERR_ARG;
    }
    if (int rc = rule_setter_ok(st, "splice_step_set_ema", "the average is set")) return rc;
    if (st->best) { splice_set_error("splice_step_set_ema: the average is set before splice_step_set_keep_best (which takes its best arena)"); return SPLICE_ERR_STATE; }
    st->graphs.retire();
    st->ema = ema; st->ema_decay = decay; st->ema_start = start;
    return SPLICE_OK;
}
// Gradient clipping of every pair of the handle (include/splice_hip.h has the rule): the step's two norm launches write `state`, its optimiser
// launch reads it.  Before the first step only, and not on a gradient-only or phase-mode handle, as the weight average.
int splice_step_set_grad_clip(void* h, float max_norm, splice_clip_state* state) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!state || !(max_norm > 0.f) || !(max_norm <= 3.402823466e+38f)) {
        splice_set_error("splice_step_set_grad_clip: needs the state records and a finite max_norm > 0, got %g", (double)max_norm);
        return SPLICE_ERR_ARG;
    }
    if (int rc = rule_setter_ok(st, "splice_step_set_grad_clip", "the rule is set")) return rc;
    if (st->clip_rule.records) { splice_set_error("splice_step_set_grad_clip: the handle clips against the running norm (splice_step_set_grad_clip_auto); a handle takes one of the two"); return SPLICE_ERR_STATE; }
    if (st->astride % 4) { splice_set_error("splice_step_set_grad_clip: the arena stride must be a multiple of 4"); return SPLICE_ERR_ARG; }
    if (!st->clip_partials) RC(salloc(st, &st->clip_partials, (size_t)st->pairs * (((size_t)st->nparams + SPLICE_CLIP_CHUNK - 1) / SPLICE_CLIP_CHUNK)));
    st->graphs.retire();
    st->clip = state; st->clip_norm = max_norm;
    return SPLICE_OK;
}
// Gradient clipping of every pair against its own running norm (include/splice_hip.h has the rule): splice_step_set_grad_clip with the second
// records, which the second norm launch keeps in its AUTO instance.  max_norm is the optional cap (0: none).  The regime is not set here:
// step_body knows it per launch sequence.
int splice_step_set_grad_clip_auto(void* h, float max_norm, float k, float beta, int warmup, splice_clip_state* state, splice_clip_auto_state* auto_state) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!state || !auto_state || !(max_norm >= 0.f) || !(max_norm <= 3.402823466e+38f)) {
        splice_set_error("splice_step_set_grad_clip_auto: needs both state records and a finite max_norm >= 0 (0: no cap), got %g", (double)max_norm);
        return SPLICE_ERR_ARG;
    }
    if (!(k >= 1.f) || !(k <= 3.402823466e+38f) || !(beta >= 0.f && beta < 1.f) || warmup < 1) {
        splice_set_error("splice_step_set_grad_clip_auto: needs a finite k >= 1, 0 <= beta < 1 and warmup >= 1, got k %g, beta %g, warmup %d", (double)k, (double)beta, warmup);
        return SPLICE_ERR_ARG;
    }
    if (int rc = rule_setter_ok(st, "splice_step_set_grad_clip_auto", "the rule is set")) return rc;
    if (st->clip && !st->clip_rule.records) { splice_set_error("splice_step_set_grad_clip_auto: the handle clips to a fixed norm (splice_step_set_grad_clip); a handle takes one of the two"); return SPLICE_ERR_STATE; }
    if (st->astride % 4) { splice_set_error("splice_step_set_grad_clip_auto: the arena stride must be a multiple of 4"); return SPLICE_ERR_ARG; }
    if (!st->clip_partials) RC(salloc(st, &st->clip_partials, (size_t)st->pairs * (((size_t)st->nparams + SPLICE_CLIP_CHUNK - 1) / SPLICE_CLIP_CHUNK)));
    st->graphs.retire();
    st->clip = state; st->clip_norm = max_norm;
    st->clip_rule = ClipAutoRule{k, beta, warmup, 0, auto_state};
    return SPLICE_OK;
}
// Keep every pair's best-window weights (include/splice_hip.h has the rule): the loss kernel's rule writes `state` and `means`, the optimiser
// launch of the same step reads the record and writes the best arena(s).  Before the first step only, behind the stop rule (and the
// average, which decides whether best_ema is due), and not on a gradient-only or phase-mode handle, as the weight average.
int splice_step_set_keep_best(void* h, float* best_params, float* best_ema, splice_best_state* state, float* means) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!best_params || !state || !means) {
        splice_set_error("splice_step_set_keep_best: needs the best arena, the state records and the window means");
        return SPLICE_ERR_ARG;
    }
    if (int rc = rule_setter_ok(st, "splice_step_set_keep_best", "the best weights are kept from")) return rc;
    if (st->stop_rule.window <= 0) { splice_set_error("splice_step_set_keep_best: needs a handle with a stop rule (splice_step_set_stop_rule, window > 0)"); return SPLICE_ERR_STATE; }
    if ((best_ema != nullptr) != (st->ema != nullptr)) {
        splice_set_error("splice_step_set_keep_best: best_ema goes with a weight average (splice_step_set_ema): given exactly when the handle keeps one");
        return SPLICE_ERR_ARG;
    }
    if (st->astride % 4) { splice_set_error("splice_step_set_keep_best: the arena stride must be a multiple of 4"); return SPLICE_ERR_ARG; }
    st->graphs.retire();
    st->best = state; st->best_means = means; st->best_p = best_params; st->best_ema = best_ema;
    return SPLICE_OK;
}
// The per-step loss trace of every pair of the handle (include/splice_hip.h has the row): the step's loss kernel writes words 0-5 of row
// step_idx, with gradient clipping its norm launch words 6-7.  Before the first step only: the rows belong to a run from step 0.  Not on a
// gradient-only or phase-mode handle: such a handle's step is one of several that share a step index.
int splice_step_set_loss_trace(void* h, float* trace, int capacity) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!trace || capacity < 1) {
        splice_set_error("splice_step_set_loss_trace: needs the trace rows and a capacity >= 1, got %d", capacity);
        return SPLICE_ERR_ARG;
    }
    if (int rc = rule_setter_ok(st, "splice_step_set_loss_trace", "the trace is set")) return rc;
    st->graphs.retire();
    st->trace = trace; st->trace_cap = capacity;
    return SPLICE_OK;
}
// The plateau lr rule of every pair of the handle (include/splice_hip.h has the rule): the step's loss kernel writes `state`, `cut_steps` and
// the handle's lr_eff table, the optimiser launch of the same step reads the table.  Before the first step only, behind the stop rule,
// and not on a gradient-only or phase-mode handle, as that rule.
int splice_step_set_lr_plateau(void* h, float factor, int patience, float min_scale, splice_lr_state* state, int* cut_steps) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!state || !cut_steps) { splice_set_error("splice_step_set_lr_plateau: needs the state records and the cut-step rows"); return SPLICE_ERR_ARG; }
    if (!lr_rule_ok(factor, patience, min_scale, "splice_step_set_lr_plateau")) return SPLICE_ERR_ARG;
    if (int rc = rule_setter_ok(st, "splice_step_set_lr_plateau", "the rule is set")) return rc;
    if (st->stop_rule.window <= 0) { splice_set_error("splice_step_set_lr_plateau: needs a handle with a stop rule (splice_step_set_stop_rule, window > 0)"); return SPLICE_ERR_STATE; }
    if (st->astride % 4) { splice_set_error("splice_step_set_lr_plateau: the arena stride must be a multiple of 4"); return SPLICE_ERR_ARG; }
    if (!st->lr_eff) RC(salloc(st, &st->lr_eff, (size_t)st->pairs));
    st->graphs.retire();
    st->lr_rule = LrRule{factor, patience, min_scale}; st->lr_state = state; st->lr_cuts = cut_steps;
    return SPLICE_OK;
}
// The image-space loss terms of every pair of the handle (include/splice_hip.h has the terms): one value launch at the loss stage, one
// gradient-add launch per backward chain whose weight is > 0, and the IMG instance of the loss kernel.  Before the first step only, and not
// on a gradient-only or phase-mode handle: a follower adds its image gradients into its leader's, which would count the terms once per
// follower.  The value kernel writes one partial per IMAGE_TERMS_CHUNK floats of an image: a handle whose largest crop needs more slots
// than the other terms do gets a wider partials buffer here (zeros added to a fixed-order sum change no bit of the other terms).
int splice_step_set_image_terms(void* h, float lambda_tv, float lambda_pix) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!(lambda_tv >= 0.f) || !(lambda_tv <= 3.402823466e+38f) || !(lambda_pix >= 0.f) || !(lambda_pix <= 3.402823466e+38f)) {
        splice_set_error("splice_step_set_image_terms: needs finite lambda_tv >= 0 and lambda_pix >= 0, got %g, %g", (double)lambda_tv, (double)lambda_pix);
        return SPLICE_ERR_ARG;
    }
    if (int rc = rule_setter_ok(st, "splice_step_set_image_terms", "the terms are set")) return rc;
    const size_t chunks = ((size_t)3 * st->max_crop_h * st->max_crop_w + IMAGE_TERMS_CHUNK - 1) / IMAGE_TERMS_CHUNK;
    if ((lambda_tv > 0.f || lambda_pix > 0.f) && chunks > st->lp) {
        float* wider = nullptr;
        RC(salloc(st, &wider, (size_t)st->P * (8 + 8 * chunks)));
        st->losses = wider; st->lp = chunks; st->lstride = 8 + 8 * chunks;   // (the narrower buffer stays with the handle until it goes)
    }
    st->graphs.retire();
    st->lambda_tv = lambda_tv; st->lambda_pix = lambda_pix;
    return SPLICE_OK;
}
// ---- what the four per-layer terms share on the host (DESIGN.md section 9k has the overview): the record above, the argument checks of
// their setters, the hash their graph keys are built from, the key-gradient buffers of the two terms that add into a chain's table, and the
// host copy of their per-layer values.
// The argument checks of a layer list for `who`: n in 1..min(depth, most), ascending distinct blocks of a depth-block ViT, finite weights > 0.
static bool layer_list_check(const char* who, int depth, int most, int n, const int* layers, const float* weights) {
    if (n < 1 || n > depth || n > most) { splice_set_error("%s: needs 1..%d layers, got %d", who, depth < most ? depth : most, n); return false; }
    for (int i = 0; i < n; ++i) {
        if (layers[i] < 0 || layers[i] >= depth || (i > 0 && layers[i] <= layers[i - 1])) {
            splice_set_error("%s: layers must be ascending distinct block indices in [0, %d), got layers[%d] = %d", who, depth, i, layers[i]);
            return false;
        }
        if (!(weights[i] > 0.f) || !(weights[i] <= 3.402823466e+38f)) {
            splice_set_error("%s: weights must be finite and > 0, got weights[%d] = %g", who, i, (double)weights[i]);
            return false;
        }
    }
    return true;
}
static const unsigned long long FNV_BASIS = 1469598103934665603ull;
static unsigned long long fnv1a_word(unsigned long long h, unsigned long long v) {   // the eight bytes of v, low byte first
    for (int k = 0; k < 8; ++k) { h ^= (v >> (8 * k)) & 0xff; h *= 1099511628211ull; }
    return h;
}
// FNV-1a from `basis` over (block, weight bits) in list order.  head >= 0 (the key second-moment list): every entry opens with a word more,
// `head` at entry 0 and 0 at the later ones.
static unsigned long long layer_list_hash(const LayerList& list, unsigned long long basis, long long head = -1) {
    unsigned long long h = basis;
    for (int i = 0; i < list.n; ++i) {
        unsigned w;
        memcpy(&w, &list.weights[i], sizeof(w));
        if (head >= 0) h = fnv1a_word(h, i == 0 ? (unsigned long long)head : 0);
        h = fnv1a_word(fnv1a_word(h, (unsigned long long)list.layers[i]), (unsigned long long)w);
    }
    return h;
}
// The key-gradient buffers of a term that ADDS into the blocks `layers` of one chain of the global view (the identity list on the y' chain,
// the key second-moment term on the x' chain): dk[i] = the buffer pk already has for the block (d_keys at the top, the structure list's),
// else a zeroed one of the handle's own -- then also in dk_own[i], for the step's zeroing of the chain's passes, and in `tab`, the chain's
// table, which starts as a copy of pk.
static int key_grad_buffers(SpliceStep* st, VitView& v, int n, const int* layers, float** dk, float** dk_own, std::vector<const float*>& tab) {
    tab = v.pk;
    for (int i = 0; i < n; ++i) {
        const int l = layers[i];
        if (v.pk[l]) { dk[i] = const_cast<float*>(v.pk[l]); continue; }
        RC(salloc(st, &dk_own[i], (size_t)v.rows * v.D));
        HIPCHK(hipMemset(dk_own[i], 0, (size_t)v.rows * v.D * sizeof(float)));   // padding rows and every other chain's passes read as zero gradient for good
        tab[l] = dk[i] = dk_own[i];
    }
    return SPLICE_OK;
}
// `count` floats of a term's values to the HOST behind a device-wide wait (the *_values readers)
static int values_to_host(float* out, const float* dev, size_t count) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, dev, count * sizeof(float), hipMemcpyDeviceToHost));
    return SPLICE_OK;
}
static unsigned long long ssim_layers_salt(const SpliceStep* st) {
    if (!st->ssim_list.n) return 0;
    const unsigned long long h = layer_list_hash(st->ssim_list, FNV_BASIS);
    return ((h ^ (h >> 15) ^ (h >> 30) ^ (h >> 45)) & 0x7fffull) << 40 | 1ull << 55;
}
// The blocks whose keys the two structure terms read, and their weights (include/splice_hip.h has the term): n ascending distinct block
// indices, n finite weights > 0.  The three self-similarity launches of a structure term then cover every named block (grid z), the ViT
// contexts write the transposed qkv copy of each, every block gets a key-gradient buffer and a workspace of its own for both views, and
// the ViT backward adds each block's dK where it always could (pk[l]).  Before the first step only; not on a gradient-only or phase-mode
// handle (such a handle in turn refuses splice_step_set_mode / splice_step_set_phases); not with fp8_selfsim (the table carries no e4m3
// workspace).  A layer list needs n tiles slots of a term's partial row: a handle whose row is narrower gets a wider partials buffer
// here -- the appended slots are zero, and in total_loss_kernel's lane-strided walk (slot i on lane i % 64, ascending) they reach each
// lane behind its existing addends, so no bit of any other term moves.
int splice_step_set_ssim_layers(void* h, int n, const int* layers, const float* weights) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_set_ssim_layers";
    if (!st || !layers || !weights) return SPLICE_ERR_ARG;
    if (!layer_list_check(who, st->vg.depth, SELFSIM_MAX_LAYERS, n, layers, weights)) return SPLICE_ERR_ARG;
    if (int rc = rule_setter_ok(st, who, "the layers are set")) return rc;
    if (st->cfg.fp8_selfsim) { splice_set_error("%s: not with fp8_selfsim (the e4m3 Gram path reads the top block alone)", who); return SPLICE_ERR_STATE; }
    if (st->ssim_list.n) { splice_set_error("%s: the layers are set once", who); return SPLICE_ERR_STATE; }
    if (st->id_list.n) { splice_set_error("%s: call it in front of splice_step_set_id_layers (the identity term shares this list's key-gradient buffers)", who); return SPLICE_ERR_STATE; }
    if (st->kg_lambda > 0.f) { splice_set_error("%s: call it in front of splice_step_set_key_gram (that term shares this list's key-gradient buffers)", who); return SPLICE_ERR_STATE; }
    if (st->nn_lambda > 0.f) { splice_set_error("%s: call it in front of splice_step_set_key_nn (that term shares this list's key-gradient buffers)", who); return SPLICE_ERR_STATE; }
    const int Tmax = st->plan_e && st->ve.T > st->vg.T ? st->ve.T : st->vg.T;
    for (VitView* v : {&st->vg, &st->ve}) {
        if (!v->ctx) continue;
        RC(splice_vit_ctx_set_transposed_layers(v->ctx, n, layers));
        for (int i = 0; i < n; ++i) {
            if (layers[i] == v->depth - 1) { v->dk_layer[i] = v->d_keys; continue; }
            RC(salloc(st, &v->dk_layer[i], (size_t)v->rows * v->D));
            HIPCHK(hipMemset(v->dk_layer[i], 0, (size_t)v->rows * v->D * sizeof(float)));   // padding rows read as zero gradient
        }
        for (int i = 0; i < n; ++i) v->pk[layers[i]] = v->dk_layer[i];   // (the top block's entry stays: the key-identity term seeds it whatever is named)
    }
    for (int i = 0; i < n; ++i) {
        if (i == 0) { st->ssim_ws_layer[0] = st->ssim_ws; continue; }
        char* ws = nullptr;
        RC(salloc(st, &ws, selfsim_batch_ws_bytes(Tmax, st->vg.D, st->P)));
        st->ssim_ws_layer[i] = ws;
    }
    const size_t need = (size_t)n * tri_tiles(Tmax);
    if (need > st->lp) {
        float* wider = nullptr;
        RC(salloc(st, &wider, (size_t)st->P * (8 + 8 * need)));
        st->losses = wider; st->lp = need; st->lstride = 8 + 8 * need;   // (the narrower buffer stays with the handle until it goes)
    }
    st->graphs.retire();
    st->ssim_list.set(n, layers, weights);
    return SPLICE_OK;
}
// The per-layer values of the last step's structure term `term` (1: global, 2: entire-image): out[i * pairs + p] (device, [n][pairs]) =
// pair p's sum of layer i's slot range of the term's partial row, added in slot order, the pair's crops in crop order -- the addends
// w_i mse(S_i, S*_i) whose ascending sum total_loss_kernel reports as word `term` of the losses row.
int splice_step_ssim_layer_values(void* h, int term, float* out, splice_stream_t stream) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_ssim_layer_values";
    if (!st || !out || (term != L_GLOBAL_SSIM && term != L_ENTIRE_SSIM)) { splice_set_error("%s: needs a handle, out and term 1 or 2", who); return SPLICE_ERR_ARG; }
    if (!st->ssim_list.n) { splice_set_error("%s: the handle has no structure layers (splice_step_set_ssim_layers)", who); return SPLICE_ERR_STATE; }
    if (term == L_ENTIRE_SSIM && !st->plan_e) { splice_set_error("%s: the handle has no entire-image branch", who); return SPLICE_ERR_STATE; }
    const int n = st->ssim_list.n, tiles = tri_tiles(term == L_GLOBAL_SSIM ? st->vg.T : st->ve.T);
    const int n_slots = term == L_GLOBAL_SSIM && st->crops_mode ? (st->pairs > 1 ? st->na : st->P) : 1;
    SPLICE_LAUNCH(ssim_layer_values_kernel, dim3((n * st->pairs + 63) / 64), dim3(64), 0, (hipStream_t)stream, (const float*)st->losses, st->lstride, (int)st->lp, term, n,
                  tiles, st->pairs, n_slots, out);
    return SPLICE_OK;
}
static unsigned long long cls_layers_salt(const SpliceStep* st) {
    if (!st->cls_list.n) return 0;
    return layer_list_hash(st->cls_list, FNV_BASIS) | 1ull;   // (never 0: a handle with layers is never keyed like one without)
}
// The blocks whose [CLS] row the two appearance terms read, and their weights (include/splice_hip.h has the term): n ascending distinct
// block indices, n finite weights > 0.  One launch per appearance term then covers every named block (cls_layers.hip) in place of the
// term's mse_batched_launch; a block below the top gets a [CLS]-row seed buffer [B][D] per view, set to zero (-0.0f) here once -- the loss kernel
// overwrites the rows it owns each step, no step writes the rows of other passes -- which the ViT backward of the x' chain (global view) and
// of the x_entire' chain (entire view) adds in front of the block (splice_vit_ctx_set_cls_seeds).  The top block, when named, keeps row 0 of
// d_block and the [CLS]-only tail; when it is not, that row stays at the zero the step's zeroing wrote.  Before the first step only; not on
// a gradient-only or phase-mode handle (which in turn refuses those calls); not with fp8_selfsim; not a second time.
int splice_step_set_cls_layers(void* h, int n, const int* layers, const float* weights) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_set_cls_layers";
    if (!st || !layers || !weights) return SPLICE_ERR_ARG;
    if (!layer_list_check(who, st->vg.depth, CLS_MAX_LAYERS, n, layers, weights)) return SPLICE_ERR_ARG;
    if (int rc = rule_setter_ok(st, who, "the layers are set")) return rc;
    if (st->cfg.fp8_selfsim) { splice_set_error("%s: not with fp8 (the e4m3 forward is validated against the top block's [CLS] row alone)", who); return SPLICE_ERR_STATE; }
    if (st->cls_list.n) { splice_set_error("%s: the layers are set once", who); return SPLICE_ERR_STATE; }
    for (VitView* v : {&st->vg, &st->ve}) {
        if (!v->ctx) continue;
        v->cls_seed_tab.assign(v->depth, nullptr);
        for (int i = 0; i < n; ++i) {
            if (layers[i] == v->depth - 1) continue;
            RC(salloc(st, &v->cls_seed[i], (size_t)v->B * v->D));
            // (-0.0f, the identity of the backward's g += seed for every g: a row no loss launch ever writes -- another chain's pass, a sweep
            // slot whose lambda is 0 -- leaves even the sign of a zero alone)
            HIPCHK(hipMemsetD32((hipDeviceptr_t)v->cls_seed[i], (int)0x80000000u, (size_t)v->B * v->D));
            v->cls_seed_tab[layers[i]] = v->cls_seed[i];
        }
        RC(salloc(st, &v->cls_values, (size_t)st->P * n));
        HIPCHK(hipMemset(v->cls_values, 0, (size_t)st->P * n * sizeof(float)));
    }
    st->graphs.retire();
    st->cls_list.set(n, layers, weights);
    return SPLICE_OK;
}
// The per-layer addends of the appearance term of the last step that computed it (entire = 0: loss_global_cls, word 4; else
// loss_entire_cls, word 3), copied to the HOST behind a device-wide wait: out[s * n + i] = slot s's w_i * mse of block i's [CLS] rows, n the
// layer count; slots = the pairs (entire, or one crop per pair), else pairs * min(nA, nB) pair-crops in pair-major order.  cap: floats
// `out` holds.  A slot's partial is the float32 sum of its row, ascending, exactly; a slot that never took part reads zeros.
int splice_step_cls_layer_values(void* h, int entire, float* out, int cap) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_cls_layer_values";
    if (!st || !out) { splice_set_error("%s: needs a handle and out", who); return SPLICE_ERR_ARG; }
    if (!st->cls_list.n) { splice_set_error("%s: the handle has no [CLS] layers (splice_step_set_cls_layers)", who); return SPLICE_ERR_STATE; }
    if (entire && !st->plan_e) { splice_set_error("%s: the handle has no entire-image branch", who); return SPLICE_ERR_STATE; }
    const int nc = st->na < st->nb ? st->na : st->nb, slots = entire ? st->pairs : st->pairs * nc;
    if (cap < slots * st->cls_list.n) { splice_set_error("%s: out holds %d floats, needs %d", who, cap, slots * st->cls_list.n); return SPLICE_ERR_ARG; }
    return values_to_host(out, entire ? st->ve.cls_values : st->vg.cls_values, (size_t)slots * st->cls_list.n);
}
static unsigned long long id_layers_salt(const SpliceStep* st) {
    if (!st->id_list.n) return 0;
    // (from a basis of its own; never 0: a handle with layers is never keyed like one without)
    return layer_list_hash(st->id_list, FNV_BASIS ^ 0x9e3779b97f4a7c15ull) | 2ull;
}
// The blocks whose keys the identity term reads, and their weights (include/splice_hip.h has the term): n ascending distinct block indices,
// n finite weights > 0.  Two launches then cover every named block (id_layers.hip) in place of the term's mse_batched_launch; the global
// ViT context writes the fp32 keys of each named block below the top (splice_vit_ctx_set_key_f32_layers).  Key-gradient buffers are per
// BLOCK: the top block's is d_keys, a block the structure list names too shares that list's buffer -- the structure term writes its x'
// passes, this term its y' passes, the way d_keys is shared at the top -- and any other block gets one of its own, zeroed here (padding rows
// read as zero gradient for good) and over its y' passes at every step (DESIGN.md section 9m says why).  The y' chain's backward reads
// pk_y = pk + the identity blocks; the x' chain and the entire-image chain keep pk, so a block named only here adds no launch to them.
// Before the first step only; not on a gradient-only or phase-mode handle (which in turn refuses those calls); not with fp8_selfsim; not
// a second time; and behind splice_step_set_ssim_layers where both are called, so that the shared buffers exist.
int splice_step_set_id_layers(void* h, int n, const int* layers, const float* weights) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_set_id_layers";
    if (!st || !layers || !weights) return SPLICE_ERR_ARG;
    VitView& v = st->vg;
    if (!layer_list_check(who, v.depth, ID_MAX_LAYERS, n, layers, weights)) return SPLICE_ERR_ARG;
    if (int rc = rule_setter_ok(st, who, "the layers are set")) return rc;
    if (st->cfg.fp8_selfsim) { splice_set_error("%s: not with fp8 (the e4m3 forward keeps fp32 keys of the top block alone)", who); return SPLICE_ERR_STATE; }
    if (st->id_list.n) { splice_set_error("%s: the layers are set once", who); return SPLICE_ERR_STATE; }
    if (st->nn_lambda > 0.f) { splice_set_error("%s: call it in front of splice_step_set_key_nn", who); return SPLICE_ERR_STATE; }
    if (v.D % 4) { splice_set_error("%s: needs an embedding width that is a multiple of 4, got %d", who, v.D); return SPLICE_ERR_ARG; }
    RC(splice_vit_ctx_set_key_f32_layers(v.ctx, n, layers));
    if (int rc = key_grad_buffers(st, v, n, layers, v.dk_id, v.dk_id_own, v.pk_y)) return rc;
    const int G = id_layers_wg(v.T, v.D, 0);
    RC(salloc(st, &st->id_scratch, (size_t)st->Pb * n * G));
    RC(salloc(st, &st->id_values, (size_t)st->Pb * n));
    HIPCHK(hipMemset(st->id_scratch, 0, (size_t)st->Pb * n * G * sizeof(float)));
    HIPCHK(hipMemset(st->id_values, 0, (size_t)st->Pb * n * sizeof(float)));
    st->graphs.retire();
    st->id_list.set(n, layers, weights);
    return SPLICE_OK;
}
// The per-layer addends of the identity term (loss_global_id_B, word 5) of the last step that computed it, copied to the HOST behind a
// device-wide wait: out[s * n + i] = slot s's w_i * mse of block i's keys, n the layer count; the slots are the B crops, pairs * nB of
// them in pair-major order.  cap: floats `out` holds.  A slot's partial -- with one crop per pair the reported word -- is the float32 sum
// of its row, ascending, exactly; a slot that never took part reads zeros.
int splice_step_id_layer_values(void* h, float* out, int cap) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_id_layer_values";
    if (!st || !out) { splice_set_error("%s: needs a handle and out", who); return SPLICE_ERR_ARG; }
    if (!st->id_list.n) { splice_set_error("%s: the handle has no identity layers (splice_step_set_id_layers)", who); return SPLICE_ERR_STATE; }
    if (cap < st->Pb * st->id_list.n) { splice_set_error("%s: out holds %d floats, needs %d", who, cap, st->Pb * st->id_list.n); return SPLICE_ERR_ARG; }
    return values_to_host(out, st->id_values, (size_t)st->Pb * st->id_list.n);
}
static unsigned long long key_gram_salt(const SpliceStep* st) {
    if (!(st->kg_lambda > 0.f)) return 0;
    unsigned w;
    memcpy(&w, &st->kg_lambda, sizeof(w));
    // FNV-1a over (block, weight bits), from a basis of its own; then the list, headed by its length and flag
    const unsigned long long h = fnv1a_word(fnv1a_word(FNV_BASIS ^ 0xc2b2ae3d27d4eb4full, (unsigned long long)st->kg_layer), (unsigned long long)w);
    return layer_list_hash(st->kg_list, h, 0x100 + 2 * st->kg_list.n + st->kg_centered) | 4ull;   // (never 0: a handle with the term is never keyed like one without)
}
// The key second-moment appearance term (include/splice_hip.h has the term): its weight, finite and > 0, and its block.  The global ViT
// context writes the transposed bf16 copy of a block below the top (splice_vit_ctx_set_transposed_layers: a repeated call before the
// first forward adds to the blocks already named, so the context ends up with the union of this block and the structure list).  The
// key gradient is ADDED into the block's buffer of the x' chain: pk's where the block has one (d_keys at the top, the structure
// list's), else a buffer of its own, zeroed here (padding rows and every other chain's passes read as zero gradient for good) and over
// its x' passes at every step the term runs; only the x' chain's backward then reads it (pk_x).  Before the first step only; not on a
// gradient-only or phase-mode handle (which in turn refuses those calls); not with fp8_selfsim; not with several pairs of nA != nB
// crops; not a second time; and behind splice_step_set_ssim_layers where both are called, so that the shared buffer exists.
int splice_step_set_key_gram(void* h, float lambda, int layer) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_set_key_gram";
    if (!st) return SPLICE_ERR_ARG;
    VitView& v = st->vg;
    if (!(lambda > 0.f) || !(lambda <= 3.402823466e+38f)) { splice_set_error("%s: lambda must be finite and > 0, got %g", who, (double)lambda); return SPLICE_ERR_ARG; }
    if (layer < 0 || layer >= v.depth) { splice_set_error("%s: layer must be a block index in [0, %d), got %d", who, v.depth, layer); return SPLICE_ERR_ARG; }
    if (int rc = rule_setter_ok(st, who, "the term is set")) return rc;
    if (st->cfg.fp8_selfsim) { splice_set_error("%s: not with fp8_selfsim (the term reads the bf16 key copies of a bf16 forward)", who); return SPLICE_ERR_STATE; }
    if (st->kg_lambda > 0.f) { splice_set_error("%s: the term is set once", who); return SPLICE_ERR_STATE; }
    if (st->nn_lambda > 0.f) { splice_set_error("%s: call it in front of splice_step_set_key_nn (that term shares this one's key-gradient buffers)", who); return SPLICE_ERR_STATE; }
    if (v.D % 64) { splice_set_error("%s: needs an embedding width that is a multiple of 64, got %d", who, v.D); return SPLICE_ERR_ARG; }
    if (st->pairs > 1 && st->na != st->nb) { splice_set_error("%s: not with several pairs of nA != nB crops (%d, %d)", who, st->na, st->nb); return SPLICE_ERR_STATE; }
    if (layer != v.depth - 1) RC(splice_vit_ctx_set_transposed_layers(v.ctx, 1, &layer));
    if (int rc = key_grad_buffers(st, v, 1, &layer, v.dk_kgl, v.dk_kgl_own, v.pk_x)) return rc;   // (a list of the one block: entry 0)
    const int slots = st->pairs * (st->na < st->nb ? st->na : st->nb), tiles = key_gram_tiles(v.D);
    RC(salloc(st, &st->kg_delta, (size_t)slots * v.D * v.D));
    RC(salloc(st, &st->kg_part, (size_t)slots * tiles));
    RC(salloc(st, &st->kg_value, (size_t)st->pairs));
    HIPCHK(hipMemset(st->kg_delta, 0, (size_t)slots * v.D * v.D * sizeof(bf16_t)));
    HIPCHK(hipMemset(st->kg_part, 0, (size_t)slots * tiles * sizeof(float)));
    HIPCHK(hipMemset(st->kg_value, 0, (size_t)st->pairs * sizeof(float)));
    st->graphs.retire();
    st->kg_lambda = lambda; st->kg_layer = layer;
    return SPLICE_OK;
}
// The raw key second-moment term of the last step that computed it, copied to the HOST behind a device-wide wait: out[p] = pair p's
// value, `pairs` floats; zeros before the first such step.
int splice_step_key_gram_values(void* h, float* out) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_key_gram_values";
    if (!st || !out) { splice_set_error("%s: needs a handle and out", who); return SPLICE_ERR_ARG; }
    if (!(st->kg_lambda > 0.f)) { splice_set_error("%s: the handle has no key second-moment term (splice_step_set_key_gram)", who); return SPLICE_ERR_STATE; }
    return values_to_host(out, st->kg_value, (size_t)st->pairs);
}
// The key second-moment term over several blocks, optionally centred (include/splice_hip.h has the term): the list version of
// splice_step_set_key_gram, with its refusals; the two exclude each other in either order ("the term is set once").  Every named block
// below the top gets its transposed bf16 copy (splice_vit_ctx_set_transposed_layers adds to the blocks already named).  Key-gradient
// buffers are per block as there: pk's where the block has one (d_keys at the top, the structure list's: that term stores, this one adds),
// else one of its own, zeroed here and over its x' passes on the steps the term runs; only the x' chain's table (pk_x) carries those.
int splice_step_set_key_gram_layers(void* h, float lambda, int n, const int* layers, const float* weights, int centered) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_set_key_gram_layers";
    if (!st || !layers || !weights) return SPLICE_ERR_ARG;
    VitView& v = st->vg;
    const int depth = v.depth;
    if (!(lambda > 0.f) || !(lambda <= 3.402823466e+38f)) { splice_set_error("%s: lambda must be finite and > 0, got %g", who, (double)lambda); return SPLICE_ERR_ARG; }
    if (!layer_list_check(who, depth, KEY_GRAM_MAX_LAYERS, n, layers, weights)) return SPLICE_ERR_ARG;
    if (centered != 0 && centered != 1) { splice_set_error("%s: centered must be 0 or 1, got %d", who, centered); return SPLICE_ERR_ARG; }
    if (int rc = rule_setter_ok(st, who, "the term is set")) return rc;
    if (st->cfg.fp8_selfsim) { splice_set_error("%s: not with fp8_selfsim (the term reads the bf16 key copies of a bf16 forward)", who); return SPLICE_ERR_STATE; }
    if (st->kg_lambda > 0.f) { splice_set_error("%s: the term is set once", who); return SPLICE_ERR_STATE; }
    if (st->nn_lambda > 0.f) { splice_set_error("%s: call it in front of splice_step_set_key_nn (that term shares this one's key-gradient buffers)", who); return SPLICE_ERR_STATE; }
    if (v.D % 64) { splice_set_error("%s: needs an embedding width that is a multiple of 64, got %d", who, v.D); return SPLICE_ERR_ARG; }
    if (st->pairs > 1 && st->na != st->nb) { splice_set_error("%s: not with several pairs of nA != nB crops (%d, %d)", who, st->na, st->nb); return SPLICE_ERR_STATE; }
    int below[KEY_GRAM_MAX_LAYERS], nbelow = 0;
    for (int i = 0; i < n; ++i)
        if (layers[i] != depth - 1) below[nbelow++] = layers[i];
    if (nbelow) RC(splice_vit_ctx_set_transposed_layers(v.ctx, nbelow, below));
    if (int rc = key_grad_buffers(st, v, n, layers, v.dk_kgl, v.dk_kgl_own, v.pk_x)) return rc;
    const size_t slots = (size_t)st->pairs * (st->na < st->nb ? st->na : st->nb), tiles = key_gram_tiles(v.D);
    RC(salloc(st, &st->kg_delta, n * slots * v.D * v.D));
    RC(salloc(st, &st->kg_part, n * slots * tiles));
    RC(salloc(st, &st->kg_value, (size_t)st->pairs));
    RC(salloc(st, &st->kg_values, (size_t)st->pairs * n));
    HIPCHK(hipMemset(st->kg_delta, 0, n * slots * v.D * v.D * sizeof(bf16_t)));
    HIPCHK(hipMemset(st->kg_part, 0, n * slots * tiles * sizeof(float)));
    HIPCHK(hipMemset(st->kg_value, 0, (size_t)st->pairs * sizeof(float)));
    HIPCHK(hipMemset(st->kg_values, 0, (size_t)st->pairs * n * sizeof(float)));
    if (centered) {
        RC(salloc(st, &st->kg_mu, n * slots * 2 * v.D));
        HIPCHK(hipMemset(st->kg_mu, 0, n * slots * 2 * v.D * sizeof(float)));
    }
    st->graphs.retire();
    st->kg_lambda = lambda; st->kg_layer = layers[n - 1]; st->kg_centered = centered;
    st->kg_list.set(n, layers, weights);
    return SPLICE_OK;
}
// The per-layer addends of the term of the last step that computed it, copied to the HOST behind a device-wide wait:
// out[p * n + i], pairs * n floats; zeros before the first such step.
int splice_step_key_gram_layer_values(void* h, float* out) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_key_gram_layer_values";
    if (!st || !out) { splice_set_error("%s: needs a handle and out", who); return SPLICE_ERR_ARG; }
    if (!kg_listed(st)) { splice_set_error("%s: the handle has no key second-moment layers (splice_step_set_key_gram_layers)", who); return SPLICE_ERR_STATE; }
    return values_to_host(out, st->kg_values, (size_t)st->pairs * st->kg_list.n);
}
static unsigned long long key_nn_salt(const SpliceStep* st) {
    if (!(st->nn_lambda > 0.f)) return 0;
    unsigned w;
    memcpy(&w, &st->nn_lambda, sizeof(w));
    // FNV-1a over (block, weight bits), from a basis of its own
    return fnv1a_word(fnv1a_word(FNV_BASIS ^ 0x165667b19e3779f9ull, (unsigned long long)st->nn_layer), (unsigned long long)w) | 8ull;   // (never 0)
}
// The nearest-neighbour key appearance term (include/splice_hip.h has the term): its weight, finite and > 0, and its block.  It reads the
// row-major bf16 qkv of the block, which every block keeps for its backward: the ViT context needs no call.  The key gradient is ADDED
// into the block's buffer of the x' chain: pk_x's where the block has one (pk's -- d_keys at the top, the structure list's -- or the key
// second-moment term's own), else a buffer of its own, zeroed here and over its x' passes at every step the term runs; only the x' chain's
// backward reads it (pk_x).  Before the first step only; not on a gradient-only or phase-mode handle (which in turn refuses those calls);
// not with fp8_selfsim; not with several pairs of nA != nB crops; not a second time; and behind the setters of the structure, identity
// and key second-moment layers where they are called, so that the shared buffers exist.
int splice_step_set_key_nn(void* h, float lambda, int layer) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_set_key_nn";
    if (!st) return SPLICE_ERR_ARG;
    VitView& v = st->vg;
    if (!(lambda > 0.f) || !(lambda <= 3.402823466e+38f)) { splice_set_error("%s: lambda must be finite and > 0, got %g", who, (double)lambda); return SPLICE_ERR_ARG; }
    if (layer < 0 || layer >= v.depth) { splice_set_error("%s: layer must be a block index in [0, %d), got %d", who, v.depth, layer); return SPLICE_ERR_ARG; }
    if (int rc = rule_setter_ok(st, who, "the term is set")) return rc;
    if (st->cfg.fp8_selfsim) { splice_set_error("%s: not with fp8_selfsim (the term reads the bf16 keys of a bf16 forward)", who); return SPLICE_ERR_STATE; }
    if (st->nn_lambda > 0.f) { splice_set_error("%s: the term is set once", who); return SPLICE_ERR_STATE; }
    if (v.D % 64) { splice_set_error("%s: needs an embedding width that is a multiple of 64, got %d", who, v.D); return SPLICE_ERR_ARG; }
    if (st->pairs > 1 && st->na != st->nb) { splice_set_error("%s: not with several pairs of nA != nB crops (%d, %d)", who, st->na, st->nb); return SPLICE_ERR_STATE; }
    if (v.pk_x.empty()) v.pk_x = v.pk;
    if (v.pk_x[layer]) v.dk_nn = const_cast<float*>(v.pk_x[layer]);
    else {
        RC(salloc(st, &v.dk_nn_own, (size_t)v.rows * v.D));
        HIPCHK(hipMemset(v.dk_nn_own, 0, (size_t)v.rows * v.D * sizeof(float)));   // padding rows and every other chain's passes read as zero gradient for good
        v.pk_x[layer] = v.dk_nn = v.dk_nn_own;
    }
    const size_t slots = (size_t)st->pairs * (st->na < st->nb ? st->na : st->nb), parts = (size_t)key_nn_parts(v.T);
    const size_t ws = key_nn_ws_bytes(v.T, v.D, (int)slots) / sizeof(float);
    RC(salloc(st, &st->nn_match, slots * v.T));
    RC(salloc(st, &st->nn_cos, slots * v.T));
    RC(salloc(st, &st->nn_part, slots * parts));
    RC(salloc(st, &st->nn_value, (size_t)st->pairs));
    RC(salloc(st, &st->nn_ws, ws));
    HIPCHK(hipMemset(st->nn_match, 0, slots * v.T * sizeof(int)));
    HIPCHK(hipMemset(st->nn_cos, 0, slots * v.T * sizeof(float)));
    HIPCHK(hipMemset(st->nn_part, 0, slots * parts * sizeof(float)));
    HIPCHK(hipMemset(st->nn_value, 0, (size_t)st->pairs * sizeof(float)));
    HIPCHK(hipMemset(st->nn_ws, 0, ws * sizeof(float)));
    st->graphs.retire();
    st->nn_lambda = lambda; st->nn_layer = layer;
    return SPLICE_OK;
}
// The raw nearest-neighbour term of the last step that computed it, copied to the HOST behind a device-wide wait: out[p] = pair p's
// value, `pairs` floats; zeros before the first such step.
int splice_step_key_nn_values(void* h, float* out) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_key_nn_values";
    if (!st || !out) { splice_set_error("%s: needs a handle and out", who); return SPLICE_ERR_ARG; }
    if (!(st->nn_lambda > 0.f)) { splice_set_error("%s: the handle has no nearest-neighbour key term (splice_step_set_key_nn)", who); return SPLICE_ERR_STATE; }
    return values_to_host(out, st->nn_value, (size_t)st->pairs);
}
// ... and its assignment: match / cos, [pairs][crops][T] each (either may be null)
int splice_step_key_nn_match(void* h, int* match, float* cos) {
    SpliceStep* st = (SpliceStep*)h;
    const char* who = "splice_step_key_nn_match";
    if (!st || (!match && !cos)) { splice_set_error("%s: needs a handle and match or cos", who); return SPLICE_ERR_ARG; }
    if (!(st->nn_lambda > 0.f)) { splice_set_error("%s: the handle has no nearest-neighbour key term (splice_step_set_key_nn)", who); return SPLICE_ERR_STATE; }
    const size_t n = (size_t)st->pairs * (st->na < st->nb ? st->na : st->nb) * st->vg.T;
    HIPCHK(hipDeviceSynchronize());
    if (match) HIPCHK(hipMemcpy(match, st->nn_match, n * sizeof(int), hipMemcpyDeviceToHost));
    if (cos) HIPCHK(hipMemcpy(cos, st->nn_cos, n * sizeof(float), hipMemcpyDeviceToHost));
    return SPLICE_OK;
}
// Start the handle at step next_step_idx of a run other handles carried so far (a resumed run, a compacted engine; DESIGN.md section
// 9g).  What a handle keeps from one step to the next, and this call therefore sets, is two things: ssim_id_on, which only the run of step
// cls_warmup switches on, and the stop records.  Nothing else in the handle is state: dev_t and the lr(s) are staged by every step's
// first launch, lr_eff is written by each step's loss kernel before the update of that step reads it, the clip partials and the loss
// partials are scratch of one step, the graphs are captured once the shapes have repeated, and the arenas, the BatchNorm buffers and
// the other rules' records are the caller's.  stop: host, [pairs] records, given exactly when the handle has the stop rule.  After
// the rule setters, before the first splice_step_run.
int splice_step_restore(void* h, int next_step_idx, const splice_stop_state* stop, splice_stream_t stream) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || next_step_idx < 0) return SPLICE_ERR_ARG;
    if (st->runs > 0) { splice_set_error("splice_step_restore: a handle is restored before its first step"); return SPLICE_ERR_STATE; }
    if ((stop != nullptr) != (st->stop_rule.window > 0)) {
        splice_set_error("splice_step_restore: the stop records go with the stop rule (splice_step_set_stop_rule): given exactly when the handle has it");
        return SPLICE_ERR_ARG;
    }
    if (stop) {
        HIPCHK(hipMemcpyAsync(st->stop, stop, (size_t)st->pairs * sizeof(splice_stop_state), hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));   // (the caller's records may go away)
    }
    st->ssim_id_on = next_step_idx > st->cfg.cls_warmup ? 1 : 0;
    return SPLICE_OK;
}
// The gather form of the input staging: the caller's crop batches and entire images hold pairs_in pairs, pair p of the handle is pair
// rows[p] of them (strictly increasing, < pairs_in <= SPLICE_STEP_MAX_PAIR_CFGS).  The table rides in the staging launch's by-value
// arguments: no device table, no launch more, no synchronisation; the staged bytes -- all a captured graph sees -- are those of a flat
// copy of the gathered batches.  rows NULL: off.
int splice_step_set_input_rows(void* h, int pairs_in, const int* rows) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (!rows) { st->pairs_in = 0; return SPLICE_OK; }
    if (st->leader) { splice_set_error("splice_step_set_input_rows: a follower stages no inputs"); return SPLICE_ERR_STATE; }
    if (pairs_in < st->pairs || pairs_in > SPLICE_STEP_MAX_PAIR_CFGS) {
        splice_set_error("splice_step_set_input_rows: the caller's %d pairs must be at least the handle's %d and at most %d", pairs_in, st->pairs, SPLICE_STEP_MAX_PAIR_CFGS);
        return SPLICE_ERR_ARG;
    }
    for (int p = 0; p < st->pairs; ++p)
        if (rows[p] < 0 || rows[p] >= pairs_in || (p > 0 && rows[p] <= rows[p - 1])) {
            splice_set_error("splice_step_set_input_rows: rows must be strictly increasing in [0, %d), got rows[%d] = %d", pairs_in, p, rows[p]);
            return SPLICE_ERR_ARG;
        }
    st->pairs_in = pairs_in;
    for (int p = 0; p < st->pairs; ++p) st->in_rows[p] = rows[p];
    return SPLICE_OK;
}
int splice_step_stop_state(void* h, splice_stop_state* out, splice_stream_t stream) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || !out) return SPLICE_ERR_ARG;
    HIPCHK(hipMemcpyAsync(out, st->stop, (size_t)st->pairs * sizeof(splice_stop_state), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    return SPLICE_OK;
}
int splice_plateau_update(splice_stop_state* state, const float* losses8, int pairs, int window, float rel, int patience, int min_steps, int step_idx,
                          int counted, splice_stream_t stream) {
    if (!state || !losses8 || pairs < 1 || step_idx < 0) return SPLICE_ERR_ARG;
    if (!stop_rule_ok(window, rel, patience, min_steps, "splice_plateau_update")) return SPLICE_ERR_ARG;
    if (!counted || window == 0) return SPLICE_OK;
    SPLICE_LAUNCH(plateau_update_kernel, dim3((pairs + 63) / 64), dim3(64), 0, (hipStream_t)stream, state, losses8, pairs, StopRule{window, rel, patience, min_steps}, step_idx,
                  (splice_best_state*)nullptr, (float*)nullptr);
    return SPLICE_OK;
}
// the same kernel, the same device function, with the keep-best record and the window means
int splice_plateau_update_best(splice_stop_state* state, splice_best_state* best, float* means, const float* losses8, int pairs, int window, float rel,
                               int patience, int min_steps, int step_idx, int counted, splice_stream_t stream) {
    if (!state || !best || !means || !losses8 || pairs < 1 || step_idx < 0) return SPLICE_ERR_ARG;
    if (!stop_rule_ok(window, rel, patience, min_steps, "splice_plateau_update_best")) return SPLICE_ERR_ARG;
    if (!counted || window == 0) return SPLICE_OK;
    SPLICE_LAUNCH(plateau_update_kernel, dim3((pairs + 63) / 64), dim3(64), 0, (hipStream_t)stream, state, losses8, pairs, StopRule{window, rel, patience, min_steps}, step_idx,
                  best, means);
    return SPLICE_OK;
}
// the loss kernel's device function for both rules; launched at uncounted steps too (lr_eff is written at every step)
int splice_plateau_update_lr(splice_stop_state* state, splice_lr_state* lr_state, int* cut_steps, const float* losses8, const float* lr_in, int per_pair,
                             float* lr_eff, int pairs, int window, float rel, int patience, int min_steps, float factor, int lr_patience, float min_scale,
                             int step_idx, int counted, splice_stream_t stream) {
    if (!state || !lr_state || !cut_steps || !losses8 || !lr_in || !lr_eff || pairs < 1 || step_idx < 0) return SPLICE_ERR_ARG;
    if (!stop_rule_ok(window, rel, patience, min_steps, "splice_plateau_update_lr")) return SPLICE_ERR_ARG;
    if (window < 1) { splice_set_error("splice_plateau_update_lr: the lr rule needs the stop rule's windows (window >= 1)"); return SPLICE_ERR_ARG; }
    if (!lr_rule_ok(factor, lr_patience, min_scale, "splice_plateau_update_lr")) return SPLICE_ERR_ARG;
    SPLICE_LAUNCH(plateau_update_lr_kernel, dim3((pairs + 63) / 64), dim3(64), 0, (hipStream_t)stream, state, lr_state, cut_steps, losses8, pairs,
                  StopRule{window, rel, patience, min_steps}, LrRule{factor, lr_patience, min_scale}, step_idx, counted, lr_in, per_pair ? 1 : 0, lr_eff);
    return SPLICE_OK;
}
// test hook: the step's total-loss launch (the instance without the stop rule) on a caller's partials buffer
int splice_total_loss_pairs(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls, float w_id, float* out8,
                            int pairs, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on, int entire, splice_stream_t stream) {
    if (!lbase || pairs < 1 || lp < 1 || lstride < 8 + (size_t)L_TERMS * lp || n_a < 1 || n_b < 1 || n_c < 1 || n_e < 1) {
        splice_set_error("splice_total_loss_pairs: invalid argument");
        return SPLICE_ERR_ARG;
    }
    const auto kernel = total_loss_kernel<false, false>;
    SPLICE_LAUNCH(kernel, dim3(pairs), dim3(320), 0, (hipStream_t)stream, lbase, lstride, lp, w_ssim, w_essim, w_ecls, w_cls, w_id, out8,
                  n_a, n_b, n_c, n_e, wtab, ssim_on, entire, (splice_stop_state*)nullptr, (const int*)nullptr, StopRule{}, (splice_best_state*)nullptr,
                  (float*)nullptr, (float*)nullptr, 0, NO_LR_RULE, NO_IMG_TERMS, NO_SSIM_LAYERS, NO_KEY_GRAM);
    return SPLICE_OK;
}
// test hook: the same launch with the image-space terms (the IMG instance, 448 threads): terms 6 / 7 of the partials (lstride >= 8 + 8 lp)
int splice_total_loss_pairs_img(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls, float w_id, float* out8,
                                int pairs, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on, int entire, float w_tv, float w_pix,
                                splice_stream_t stream) {
    if (!lbase || pairs < 1 || lp < 1 || lstride < 8 + (size_t)8 * lp || n_a < 1 || n_b < 1 || n_c < 1 || n_e < 1 || !(w_tv >= 0.f) || !(w_pix >= 0.f)) {
        splice_set_error("splice_total_loss_pairs_img: invalid argument");
        return SPLICE_ERR_ARG;
    }
    const auto kernel = total_loss_kernel<false, false, false, true>;
    SPLICE_LAUNCH(kernel, dim3(pairs), dim3(448), 0, (hipStream_t)stream, lbase, lstride, lp, w_ssim, w_essim, w_ecls, w_cls, w_id, out8,
                  n_a, n_b, n_c, n_e, wtab, ssim_on, entire, (splice_stop_state*)nullptr, (const int*)nullptr, StopRule{}, (splice_best_state*)nullptr,
                  (float*)nullptr, (float*)nullptr, 0, NO_LR_RULE, w_tv, w_pix, NO_SSIM_LAYERS, NO_KEY_GRAM);
    return SPLICE_OK;
}
// test hook: the same launch with the loss trace (the TRACE instances): dev_t holds step index + 1 on the device; stop (optional, with its
// rule: the MONITOR instance, as a handle with the stop rule launches it) the [pairs] records
int splice_total_loss_pairs_trace(float* lbase, size_t lstride, int lp, float w_ssim, float w_essim, float w_ecls, float w_cls, float w_id, float* out8,
                                  int pairs, int n_a, int n_b, int n_c, int n_e, const float* wtab, int ssim_on, int entire, splice_stop_state* stop,
                                  int window, float rel, int patience, int min_steps, const int* dev_t, float* trace, int capacity,
                                  splice_stream_t stream) {
    if (!lbase || pairs < 1 || lp < 1 || lstride < 8 + (size_t)L_TERMS * lp || n_a < 1 || n_b < 1 || n_c < 1 || n_e < 1 || !dev_t || !trace || capacity < 1) {
        splice_set_error("splice_total_loss_pairs_trace: invalid argument");
        return SPLICE_ERR_ARG;
    }
    if (stop && (window < 1 || !stop_rule_ok(window, rel, patience, min_steps, "splice_total_loss_pairs_trace"))) {
        if (window < 1) splice_set_error("splice_total_loss_pairs_trace: stop records go with their rule (window >= 1)");
        return SPLICE_ERR_ARG;
    }
    const auto kernel = stop ? total_loss_kernel<true, true> : total_loss_kernel<false, true>;
    SPLICE_LAUNCH(kernel, dim3(pairs), dim3(320), 0, (hipStream_t)stream, lbase, lstride, lp, w_ssim, w_essim, w_ecls, w_cls, w_id, out8, n_a, n_b, n_c, n_e, wtab,
                  ssim_on, entire, stop, dev_t, stop ? StopRule{window, rel, patience, min_steps} : StopRule{}, (splice_best_state*)nullptr, (float*)nullptr, trace,
                  capacity, NO_LR_RULE, NO_IMG_TERMS, NO_SSIM_LAYERS, NO_KEY_GRAM);
    return SPLICE_OK;
}

// BatchNorm running statistics (models/unet/common.py:95-96): when set, every step applies the momentum-0.1 update of its
// netG calls in the reference's order (A_global, A on entire steps, B_global; models/model.py:15-23) to the caller's
// buffer arena(s) (layout: splice_gen_buffer_info; pair p at running + p * stride).  NULL switches tracking off.
int splice_step_set_running_stats(void* h, float* running, long long stride) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || (running && st->P > 1 && stride <= 0)) return SPLICE_ERR_ARG;
    st->running = running; st->running_stride = stride;
    return SPLICE_OK;
}

// `n` images src [3][h][w] -> passes [pass, pass + n) of view v's image batch (Resize; the Normalize is fused into the ViT patch gather)
static int place_passes(VitView& v, const float* src, int h, int w, int pass, int n, hipStream_t s) {
    return place_images(src, h, w, v.imgs + (size_t)pass * 3 * v.H * v.W, v.H, v.W, n, s);
}
// zero the two seed planes (block output, keys) of passes [pass, pass + n): the loss kernels write only the rows they own
static int zero_seeds(VitView& v, int pass, int n, hipStream_t s) {
    const size_t passD = (size_t)v.Tld * v.D;
    RC(dev_zero_launch(v.d_block + pass * passD, n * passD * sizeof(float), s));
    for (float* dk : v.dk_layer)   // the lower blocks of splice_step_set_ssim_layers (the top block's entry is d_keys itself)
        if (dk && dk != v.d_keys) RC(dev_zero_launch(dk + pass * passD, n * passD * sizeof(float), s));
    return dev_zero_launch(v.d_keys + pass * passD, n * passD * sizeof(float), s);
}

// ---- the launch sequence of one step (capturable: no allocation, no host sync, internal pointers only)
static int step_body(SpliceStep* st, float* params, float* grads, float* m, float* v, bool ssim_on, bool entire, hipStream_t s) {
    const splice_step_config& c = st->cfg;
    VitView &vg = st->vg, &ve = st->ve;
    const int P = st->P, Pa = st->Pa, Pb = st->Pb, pairs = st->pairs;
    const int nc = st->na < st->nb ? st->na : st->nb, Pc = pairs * nc;   // Pc: pairs of the appearance term (zip of x' and B' within each pair)
    Term t[L_TERMS] = {};
    step_terms(st, ssim_on, entire, t);
    const StepPtrs ip = step_ptrs(st);
    // a follower (splice_step_set_phases) sees the leader's images and adds its image gradients to the leader's
    const StepPtrs src = st->leader ? step_ptrs(st->leader) : ip;
    const bool img_on = st->lambda_tv > 0.f || st->lambda_pix > 0.f;   // (whole-step handles without a leader only: src == ip)
    const bool do_gf = (st->phases & 1) != 0, do_v = (st->phases & 2) != 0, do_gb = (st->phases & 4) != 0;
    const bool gen_fwd = do_gf && !(st->ablate & 1), gen_bwd = do_gb && !(st->ablate & 2);
    // Backward of one image chain on stream q: ViT data gradient of passes [p0, p1) of view vw (`vit`), un-resized into the gradient d_img of
    // the chain's generated images [h][w], added to the leader's d_lead by a follower; then (`gen`) the generator backward of `plan` into `arena`.
    // `img_term` (L_GLOBAL_TV on the x' chain, L_GLOBAL_PIX on the y' chain, 0 on the entire-image chain): with that term's weight > 0 its
    // gradient is added into d_img in place, one launch, from the chain's saved generator output.
    // `pk`: the chain's key-gradient table -- the view's, or on the y' chain of a step whose identity term ran over named blocks that table plus
    // those blocks (pk_y).
    // `cls_term` ([CLS] layers only; L_GLOBAL_CLS on the x' chain, L_ENTIRE_CLS on the entire-image chain, 0 on the y' chain): the chain's passes
    // are armed with the view's seed buffers when that term ran this step, and disarmed otherwise -- a chain without seeds gains no launch.
    auto chain_bwd = [&](VitView& vw, int p0, int p1, bool vit, float* d_img, int h, int w, float* d_lead, void* plan, float* arena, int accumulate,
                         bool gen, int img_term, int cls_term, const std::vector<const float*>& pk, hipStream_t q) -> int {
        if (do_v) {
            if (vit && st->cls_list.n) RC(splice_vit_ctx_set_cls_seeds(vw.ctx, cls_term && t[cls_term].on ? vw.cls_seed_tab.data() : nullptr, p0, p1));
            if (vit) RC(splice_vit_backward(vw.ctx, p0, p1, vw.pb.data(), nullptr, pk.data(), vw.d_imgs, 1, q));
            RC(unplace_grads(vw.d_imgs + (size_t)p0 * 3 * vw.H * vw.W, vw.H, vw.W, d_img, h, w, p1 - p0, q));
            if (st->leader) RC(add_f32_launch(d_lead, d_img, (size_t)(p1 - p0) * 3 * h * w, q));
            if (img_term == L_GLOBAL_TV && st->lambda_tv > 0.f) RC(image_tv_grad_add_launch(ip.x, d_img, p1 - p0, h, w, st->lambda_tv, q));
            if (img_term == L_GLOBAL_PIX && st->lambda_pix > 0.f) RC(image_pix_grad_add_launch(ip.y, ip.b_in, d_img, p1 - p0, h, w, st->lambda_pix, q));
        }
        if (gen) RC(splice_gen_backward(plan, params, d_img, arena, accumulate, q));
        return SPLICE_OK;
    };
    // pass layout of the global context: [0, Pa) A'   [Pa, Pa + Pb) B'   then x' = G(A crops) (Pa passes), y' = G(B crops) (Pb passes)
    const int pA = 0, pB = Pa, pX = Pa + Pb, pY = 2 * Pa + Pb, pEnd = 2 * (Pa + Pb);
    // ---- the no-grad target passes A', B' (util/losses.py:79,91,101) do not depend on the generator: their ViT forward
    // runs on a side stream beside the generator forward (hundreds of small latency-bound launches that leave most
    // CUs idle); inside a capture this becomes a fork/join of the graph.  The instrumented (profiling) path stays serial.
    const bool overlap = st->overlap && !splice_prof_active();
    hipStream_t s2 = overlap ? st->side_stream : s;
    if (overlap) {
        HIPCHK(hipEventRecord(st->ev(SpliceStep::EV_FORK), s));
        HIPCHK(hipStreamWaitEvent(s2, st->ev(SpliceStep::EV_FORK), 0));
    }
    // The generator runs as one plan per crop kind (A crops | B crops: the reference draws their sizes independently,
    // data/Dataset.py:66-67); G(B_crop) goes first on the side stream so that it runs beside G(A_crop) instead of behind it
    if (gen_fwd) {
        RC(splice_gen_forward_borrowed(st->plan_b, params, src.b_in, ip.y, s2));
        if (overlap) HIPCHK(hipEventRecord(st->ev(SpliceStep::EV_GB), s2));
    }
    float *blk_g = nullptr, *qkv_g = nullptr;
    RC(splice_vit_get_tensor(vg.ctx, 0, vg.depth - 1, (void**)&blk_g));
    RC(splice_vit_get_tensor(vg.ctx, 3, vg.depth - 1, (void**)&qkv_g));
    const size_t passD = (size_t)vg.Tld * vg.D;
    SelfSimBatch sb = {};
    // structure layers (splice_step_set_ssim_layers): the tables of the two views' launches; null: the top block alone, the plain launches
    SelfSimLayers sl = {}, sle = {};
    const bool layered = st->ssim_list.n > 0;
    IdLayers idt = {};   // identity layers (splice_step_set_id_layers): the table of the term's two launches
    const bool id_layered = do_v && t[L_GLOBAL_ID].on && st->id_list.n > 0;
    // the key second-moment term (splice_step_set_key_gram): on the steps of the structure and identity terms, entire-image steps included
    const bool kg_on = do_v && ssim_on && st->kg_lambda > 0.f;
    // the nearest-neighbour key term (splice_step_set_key_nn): on the same steps
    const bool nn_on = do_v && ssim_on && st->nn_lambda > 0.f;
    if (do_v) {
        RC(place_passes(vg, src.a_in, c.crop_h, c.crop_w, pA, Pa, s2));
        RC(place_passes(vg, src.b_in, st->cropb_h, st->cropb_w, pB, Pb, s2));
        if (!(st->ablate & 8)) RC(splice_vit_forward_passes(vg.ctx, vg.imgs, 1, pX, pA, pX, s2));
        // everything of the loss stage that does not need the generated images also runs here, off the critical path
        RC(dev_zero_launch(st->losses, (size_t)P * st->lstride * sizeof(float), s2));
        RC(zero_seeds(vg, pX, Pa + Pb, s2));
        for (float* dk : vg.dk_id_own)   // the blocks only the identity list names: their y' passes alone (no x' chain reads them)
            if (dk) RC(dev_zero_launch(dk + pY * passD, Pb * passD * sizeof(float), s2));
        // the blocks only the key second-moment term names: their x' passes alone (no other chain reads them), on the steps the term adds into them
        if (kg_on)
            for (float* dk : vg.dk_kgl_own)
                if (dk) RC(dev_zero_launch(dk + pX * passD, Pa * passD * sizeof(float), s2));
        if (nn_on && vg.dk_nn_own) RC(dev_zero_launch(vg.dk_nn_own + pX * passD, Pa * passD * sizeof(float), s2));   // likewise the nearest-neighbour term's
        if (t[L_GLOBAL_SSIM].on) {   // target self-similarity S* of A' (util/losses.py:79)
            RC(ssim_batch(st, vg, pA, pX, Pa, t[L_GLOBAL_SSIM], L_GLOBAL_SSIM, &sb, layered ? &sl : nullptr));
            RC(selfsim_target_launch(sb, s2, layered ? &sl : nullptr));
        }
    }
    if (overlap) HIPCHK(hipEventRecord(st->ev(SpliceStep::EV_JOIN), s2));
    // ---- Model.forward: x_global = G(A_crop), y_global = G(B_crop) [, x_entire = G(A)]
    if (gen_fwd) {
        RC(splice_gen_forward_borrowed(st->plan_a, params, src.a_in, ip.x, s));
        if (overlap) HIPCHK(hipStreamWaitEvent(s, st->ev(SpliceStep::EV_GB), 0));
    }
    if (do_v) {
        RC(place_passes(vg, src.x, c.crop_h, c.crop_w, pX, Pa, s));
        RC(place_passes(vg, src.y, st->cropb_h, st->cropb_w, pY, Pb, s));
        if (!(st->ablate & 16)) RC(splice_vit_forward_passes(vg.ctx, vg.imgs, 1, pX, pX, pEnd, s));
    }
    if (overlap) HIPCHK(hipStreamWaitEvent(s, st->ev(SpliceStep::EV_JOIN), 0));
    // ---- losses on the global batch
    if (do_v) {
        if (t[L_GLOBAL_SSIM].on) RC(selfsim_loss_launch(sb, s, layered ? &sl : nullptr));
        if (kg_on && kg_listed(st)) {   // the term over its list of blocks: one table, the layer a grid dimension
            KeyGramLayers kt = {};
            kt.n = st->kg_list.n; kt.centered = st->kg_centered;
            kt.ldt_x = kt.ldt_b = vg.rows; kt.tx_ps = kt.tb_ps = (size_t)vg.Tld; kt.ldk = 3 * vg.D; kt.k_ps = (size_t)vg.Tld * 3 * vg.D;
            kt.T = vg.T; kt.D = vg.D; kt.part_ps = (size_t)key_gram_tiles(vg.D); kt.lddk = vg.D; kt.dk_ps = passD;
            kt.values = st->kg_values; kt.value = st->kg_value; kt.mu = st->kg_mu;
            const size_t slots = (size_t)pairs * nc;
            const float c0 = 4.0f * st->kg_lambda / ((float)vg.T * (float)vg.D * (float)vg.D);
            for (int i = 0; i < st->kg_list.n; ++i) {
                const int l = st->kg_list.layers[i];
                bf16_t *qkv = nullptr, *qkvT = nullptr;
                RC(splice_vit_get_tensor(vg.ctx, 1, l, (void**)&qkv));
                RC(splice_vit_get_tensor(vg.ctx, l == vg.depth - 1 ? 6 : 8, l, (void**)&qkvT));
                KeyGramLayer& e = kt.e[i];
                e.kT_x = qkvT + (size_t)vg.D * vg.rows + (size_t)pX * vg.Tld; e.kT_b = qkvT + (size_t)vg.D * vg.rows + (size_t)pB * vg.Tld;
                e.k_x = qkv + (size_t)pX * vg.Tld * 3 * vg.D + vg.D;
                e.delta = st->kg_delta + i * slots * vg.D * vg.D; e.part = st->kg_part + i * slots * kt.part_ps;
                e.dk = vg.dk_kgl[i] + pX * passD;
                e.weight = st->kg_list.weights[i]; e.scale = c0 * e.weight;   // (one rounding more than the one-block scale; weight 1: its bits)
            }
            RC(key_gram_layers_loss_launch(kt, pairs, nc, s));
            RC(key_gram_layers_dk_launch(kt, pairs, nc, s));
        } else if (kg_on) {   // keys of x' against keys of B', crop i with crop i, through their D x D second moments; behind selfsim_dk_kernel: that stores, this adds
            const int l = st->kg_layer;
            bf16_t *qkv = nullptr, *qkvT = nullptr;
            RC(splice_vit_get_tensor(vg.ctx, 1, l, (void**)&qkv));
            RC(splice_vit_get_tensor(vg.ctx, l == vg.depth - 1 ? 6 : 8, l, (void**)&qkvT));
            KeyGram kg = {};
            kg.kT_x = qkvT + (size_t)vg.D * vg.rows + (size_t)pX * vg.Tld; kg.kT_b = qkvT + (size_t)vg.D * vg.rows + (size_t)pB * vg.Tld;
            kg.ldt_x = kg.ldt_b = vg.rows; kg.tx_ps = kg.tb_ps = (size_t)vg.Tld;
            kg.k_x = qkv + (size_t)pX * vg.Tld * 3 * vg.D + vg.D; kg.ldk = 3 * vg.D; kg.k_ps = (size_t)vg.Tld * 3 * vg.D;
            kg.T = vg.T; kg.D = vg.D;
            kg.delta = st->kg_delta; kg.part = st->kg_part; kg.part_ps = (size_t)key_gram_tiles(vg.D); kg.value = st->kg_value;
            kg.dk = vg.dk_kgl[0] + pX * passD; kg.lddk = vg.D; kg.dk_ps = passD;
            kg.scale = 4.0f * st->kg_lambda / ((float)vg.T * (float)vg.D * (float)vg.D);
            RC(key_gram_loss_launch(kg, pairs, nc, s));
            RC(key_gram_dk_launch(kg, pairs, nc, s));
        }
        if (nn_on) {   // every key of x' towards its nearest key of B', crop i with crop i; behind the structure term's store and the key second-moment add
            bf16_t* qkv = nullptr;
            RC(splice_vit_get_tensor(vg.ctx, 1, st->nn_layer, (void**)&qkv));
            KeyNn kn = {};
            kn.k_x = qkv + (size_t)pX * vg.Tld * 3 * vg.D + vg.D; kn.k_b = qkv + (size_t)pB * vg.Tld * 3 * vg.D + vg.D;
            kn.ldk = 3 * vg.D; kn.kx_ps = kn.kb_ps = (size_t)vg.Tld * 3 * vg.D;
            kn.T = vg.T; kn.D = vg.D; kn.scale = st->nn_lambda / (float)vg.T; kn.eps = 1e-8f; kn.inv_t = 1.0f / (float)vg.T;
            kn.match = st->nn_match; kn.cos = st->nn_cos; kn.part = st->nn_part; kn.part_ps = (size_t)key_nn_parts(vg.T); kn.value = st->nn_value;
            kn.dk = vg.dk_nn + pX * passD; kn.lddk = vg.D; kn.dk_ps = passD; kn.ws = st->nn_ws;
            RC(key_nn_launch(kn, pairs, nc, s));
        }
        if (t[L_GLOBAL_CLS].on && st->cls_list.n) {   // [CLS] of the named blocks: one launch for all of them, the call structure of the plain path below
            const int n = st->cls_list.n;
            const float g = t[L_GLOBAL_CLS].lambda / (float)(size_t)vg.D;
            ClsLayers ct = {};
            if (pairs > 1 && st->na != st->nb) {
                for (int i = 0; i < nc; ++i) {
                    RC(cls_table(st, vg, pX + i, st->na, pB + i, st->nb, &ct));
                    RC(cls_layers_launch(ct, pairs, g, nullptr, loss_part(st, L_GLOBAL_CLS) + (size_t)i * st->lstride, (size_t)nc * st->lstride,
                                         vg.cls_values + (size_t)i * n, (size_t)nc * n, s));
                }
            } else {
                RC(cls_table(st, vg, pX, 1, pB, 1, &ct));
                RC(cls_layers_launch(ct, Pc, g, t[L_GLOBAL_CLS].tab, loss_part(st, L_GLOBAL_CLS), st->lstride, vg.cls_values, (size_t)n, s));
            }
        } else if (t[L_GLOBAL_CLS].on) {   // [CLS] of block 11, before the final LayerNorm (util/losses.py:90-93)
            if (pairs > 1 && st->na != st->nb) {
                // several pairs with nA != nB crops: one launch per crop index i (pair p's x'_i against its B'_i into slot p nc + i); every
                // pair-crop is its own workgroups, as in one launch
                for (int i = 0; i < nc; ++i)
                    RC(mse_batched_launch(blk_g + (pX + i) * passD, vg.D, st->na * passD, blk_g + (pB + i) * passD, vg.D, st->nb * passD, 1, vg.D, 1.0f,
                                          t[L_GLOBAL_CLS].lambda, loss_part(st, L_GLOBAL_CLS) + (size_t)i * st->lstride, (size_t)nc * st->lstride,
                                          vg.d_block + (pX + i) * passD, vg.D, st->na * passD, pairs, s, nullptr));
            } else {
                RC(mse_batched_launch(blk_g + pX * passD, vg.D, passD, blk_g + pB * passD, vg.D, passD, 1, vg.D, 1.0f, t[L_GLOBAL_CLS].lambda,
                                      loss_part(st, L_GLOBAL_CLS), st->lstride, vg.d_block + pX * passD, vg.D, passD, Pc, s, t[L_GLOBAL_CLS].tab));
            }
        }
        if (t[L_GLOBAL_ID].on && st->id_list.n) {   // keys of the named blocks: one launch for all of them; its finish launch rides in bookkeeping
            RC(id_table(st, pY, pB, &idt));
            RC(id_layers_launch(idt, Pb, t[L_GLOBAL_ID].lambda / (float)((size_t)vg.T * vg.D), t[L_GLOBAL_ID].tab, st->id_scratch, 0, s));
        } else if (t[L_GLOBAL_ID].on)    // keys of y' against keys of B' (util/losses.py:96-105): mean over h*T*d = T*D
            RC(mse_batched_launch(keys_ptr(vg, qkv_g, pY), 3 * vg.D, 3 * passD, keys_ptr(vg, qkv_g, pB), 3 * vg.D, 3 * passD, vg.T, vg.D, 1.0f, t[L_GLOBAL_ID].lambda,
                                  loss_part(st, L_GLOBAL_ID), st->lstride, vg.d_keys + pY * passD, vg.D, passD, Pb, s, t[L_GLOBAL_ID].tab));
        // the image-space terms, at the crops' own resolution: image i's partials into terms 6 / 7 of slot i, every step (no schedule)
        if (img_on)
            RC(image_terms_value_launch(st->lambda_tv > 0.f ? ip.x : nullptr, Pa, c.crop_h, c.crop_w, loss_part(st, L_GLOBAL_TV),
                                        st->lambda_pix > 0.f ? ip.y : nullptr, ip.b_in, Pb, st->cropb_h, st->cropb_w, loss_part(st, L_GLOBAL_PIX),
                                        st->lstride, st->lp, s));
    }
    // ---- entire-image branch (every entire_every-th step): passes [0, pairs) A_entire', [pairs, 2 pairs) x_entire'
    if (entire) {
        if (do_gf) RC(splice_gen_forward_borrowed(st->plan_e, params, src.e_in, ip.xe, s));
        if (do_v) {
            RC(place_passes(ve, src.e_in, c.ent_h, c.ent_w, 0, pairs, s));
            RC(place_passes(ve, src.xe, c.ent_h, c.ent_w, pairs, pairs, s));
            RC(splice_vit_forward_ex(ve.ctx, ve.imgs, 1, pairs, s));
            float* blk_e = nullptr;
            RC(splice_vit_get_tensor(ve.ctx, 0, ve.depth - 1, (void**)&blk_e));
            const size_t epassD = (size_t)ve.Tld * ve.D;
            RC(zero_seeds(ve, pairs, pairs, s));
            if (t[L_ENTIRE_SSIM].on) {
                SelfSimBatch se = {};
                RC(ssim_batch(st, ve, 0, pairs, pairs, t[L_ENTIRE_SSIM], L_ENTIRE_SSIM, &se, layered ? &sle : nullptr));
                RC(selfsim_target_launch(se, s, layered ? &sle : nullptr));
                RC(selfsim_loss_launch(se, s, layered ? &sle : nullptr));
            }
            if (t[L_ENTIRE_CLS].on && st->cls_list.n) {   // the same over the named blocks (one launch)
                ClsLayers ct = {};
                RC(cls_table(st, ve, pairs, 1, pB, st->nb, &ct));
                RC(cls_layers_launch(ct, pairs, t[L_ENTIRE_CLS].lambda / (float)(size_t)ve.D, t[L_ENTIRE_CLS].tab, loss_part(st, L_ENTIRE_CLS), st->lstride,
                                     ve.cls_values, (size_t)st->cls_list.n, s));
            } else if (t[L_ENTIRE_CLS].on)   // target is the B_global crop's CLS (util/losses.py:60; with n_crops > 1 the zip pairs x_entire with the FIRST crop of its pair)
                RC(mse_batched_launch(blk_e + pairs * epassD, ve.D, epassD, blk_g + pB * passD, vg.D, st->nb * passD, 1, ve.D, 1.0f, t[L_ENTIRE_CLS].lambda,
                                      loss_part(st, L_ENTIRE_CLS), st->lstride, ve.d_block + pairs * epassD, ve.D, epassD, pairs, s, t[L_ENTIRE_CLS].tab));
        }
    }
    // The reported loss values and the BatchNorm running statistics (reference's call order) depend on nothing downstream: with a side
    // stream they run at the tail of its chain instead of between the generator backward and Adam on the critical one, else at the end.
    const bool stop_on = st->stop_rule.window > 0;   // the plateau stop rule: monitor in the loss kernel, frozen slots masked out of the two updates
    auto bookkeeping = [&](hipStream_t q) -> int {
        if (do_v) {
            // slots per pair and term: 1 (pairs mode); the slot count for every term (one pair with n_crops: unused slots hold zeros); the
            // term's crops per pair (several pairs with n_crops)
            const bool grouped = st->crops_mode && pairs > 1;
            const int n1 = st->crops_mode ? P : 1;
            // (the rule and the trace ride in the launch: no node more)
            const bool lrp = st->lr_state != nullptr, trc = st->trace != nullptr;
            // the identity layers' finish launch: the slots' addends, and their sum into partial slot 0 of the term's zeroed row
            if (id_layered)
                RC(id_layers_finish_launch(idt, Pb, t[L_GLOBAL_ID].tab, st->id_scratch, 0, st->id_values, (size_t)st->id_list.n, loss_part(st, L_GLOBAL_ID),
                                           st->lstride, q));
            // the trailing pair (weight, values) of the one key term that is on: the nearest-neighbour term alone rides on the KG instance
            const bool key_one = kg_on != nn_on;
            const float w_key = kg_on ? st->kg_lambda : nn_on ? st->nn_lambda : st->kg_lambda;
            const float* v_key = kg_on ? st->kg_value : nn_on ? st->nn_value : st->kg_value;
#define TOTAL_LOSS_STEP_ARGS                                                                                                                                         \
    st->losses, st->lstride, (int)st->lp, t[L_GLOBAL_SSIM].lambda, t[L_ENTIRE_SSIM].lambda, t[L_ENTIRE_CLS].lambda, t[L_GLOBAL_CLS].lambda, t[L_GLOBAL_ID].lambda, \
        st->losses_out, grouped ? st->na : n1, grouped ? st->nb : n1, grouped ? nc : n1, grouped ? 1 : n1, st->pw ? st->pw + (size_t)PW_LAMBDAS * P : nullptr,     \
        (int)ssim_on, (int)entire, st->stop, st->dev_t, st->stop_rule, st->best, st->best_means, st->trace, st->trace_cap, st->lr_rule, st->lr_state, st->lr_cuts, \
        (const float*)(st->pair_lr ? st->dev_lrs : st->dev_lr), st->pair_lr ? 1 : 0, st->lr_eff, st->lambda_tv, st->lambda_pix, st->ssim_list.n, tri_tiles(vg.T),  \
        st->plan_e ? tri_tiles(ve.T) : 0, w_key, v_key
            if (kg_on && nn_on) {
                const auto kernel = total_loss_nn_for(img_on, layered, lrp, trc, stop_on);
                SPLICE_LAUNCH(kernel, dim3(pairs), dim3(img_on ? 448 : 320), 0, q, TOTAL_LOSS_STEP_ARGS, st->nn_lambda, (const float*)st->nn_value);
            } else {
                const auto kernel = key_one ? total_loss_for<true>(img_on, layered, lrp, trc, stop_on) : total_loss_for<false>(img_on, layered, lrp, trc, stop_on);
                SPLICE_LAUNCH(kernel, dim3(pairs), dim3(img_on ? 448 : 320), 0, q, TOTAL_LOSS_STEP_ARGS);
            }
#undef TOTAL_LOSS_STEP_ARGS
        }
        if (!st->running || !gen_fwd) return SPLICE_OK;
        void* plans[3] = {st->plan_a, st->plan_b, nullptr};
        if (entire) { plans[1] = st->plan_e; plans[2] = st->plan_b; }   // (A_global, A on entire steps, B_global)
        // (a slot that stops at THIS step is not frozen yet: the order against the loss kernel above does not matter)
        return gen_running_stats_update(plans, entire ? 3 : 2, st->running, st->running_stride, 0.1f, stop_on ? st->stop : nullptr, st->dev_t, q);
    };
    // ---- backward (train.py:78): ViT dgrad for the generated images only, then the generator
    // the x' and y' passes are independent chains until the generator: one per stream (every launch of a
    // dependent chain pays ~8 us of fixed latency; two chains in flight hide each other's), each into its
    // own generator plan and gradient arena (no cross-chain accumulation)
    const bool side_tail = overlap && !(st->ablate & 4);
    const float* adam_g2 = nullptr;
    if (!(st->ablate & 4)) {   // (the same launches whether or not the second stream is used: results are bit-identical)
        if (overlap) {
            HIPCHK(hipEventRecord(st->ev(SpliceStep::EV_FORK2), s));
            HIPCHK(hipStreamWaitEvent(s2, st->ev(SpliceStep::EV_FORK2), 0));
        }
        RC(chain_bwd(vg, pY, pEnd, !(st->ablate & 32), ip.dy, st->cropb_h, st->cropb_w, src.dy, st->plan_b, st->grads_b, 0, gen_bwd, L_GLOBAL_PIX, 0, id_layered ? vg.pk_y : vg.pk, s2));
        if (side_tail) {
            RC(bookkeeping(s2));
            HIPCHK(hipEventRecord(st->ev(SpliceStep::EV_JOIN2), s2));
        }
        RC(chain_bwd(vg, pX, pY, true, ip.dx, c.crop_h, c.crop_w, src.dx, st->plan_a, grads, st->accumulate, gen_bwd, L_GLOBAL_TV, L_GLOBAL_CLS, kg_on || nn_on ? vg.pk_x : vg.pk, s));
        if (overlap) HIPCHK(hipStreamWaitEvent(s, st->ev(SpliceStep::EV_JOIN2), 0));
        // grads = g(A) + g(B): folded into the Adam kernel on ordinary steps; a separate add when the entire-image branch
        // still has to accumulate into the sum (same association order either way)
        if (gen_bwd) {
            if (entire || st->skip_adam) RC(add_f32_launch(grads, st->grads_b, arena_floats(st), s));
            else adam_g2 = st->grads_b;
        }
    }
    if (entire) RC(chain_bwd(ve, pairs, 2 * pairs, true, ip.dxe, c.ent_h, c.ent_w, src.dxe, st->plan_e, grads, 1, do_gb, 0, L_ENTIRE_CLS, ve.pk, s));
    if (!side_tail) RC(bookkeeping(s));
    // ---- optimizer.step() (train.py:79) over every pair's arena; Adam's step count (>= 1) and a scheduled lr are read from the device at
    // execution time
    SPLICE_DEV_REGION(21);
    if (do_gb && !st->skip_adam) {
        OptimArgs a = {};
        a.kind = st->opt_kind; a.p = params; a.g = grads; a.g2 = adam_g2; a.m = m; a.v = v;
        a.n = arena_floats(st);
        a.lr = c.lr; a.hp0 = st->opt_hp0; a.hp1 = st->opt_hp1; a.eps = st->opt_eps; a.step_dev = st->dev_t;
        // per-pair lrs (splice_step_set_pair_lr): pair p's arena reads dev_lrs[p]
        a.lr_dev = st->pair_lr ? st->dev_lrs : st->lr_set ? st->dev_lr : nullptr;
        a.lr_stride = st->pair_lr ? st->astride : 0;
        // the plateau lr rule: the learning rate(s) THIS step's loss kernel wrote, lr_in * scale -- that kernel always precedes this launch
        // (the order keep-best relies on, below): on the side stream's tail, in front of the EV_JOIN2 wait above, or on the main stream in
        // front of this launch.  One arena reads lr_eff[0] as a scheduled lr, several the per-pair instances (no other kernel than a sweep's)
        if (st->lr_state) { a.lr_dev = st->lr_eff; a.lr_stride = st->pairs > 1 ? st->astride : 0; }
        if (stop_on) { a.mask = st->stop; a.mask_step = st->dev_t; a.mask_stride = st->astride; }
        if (st->ema) { a.ema = st->ema; a.ema_decay = st->ema_decay; a.ema_start = st->ema_start; }   // (another kernel: the graph pool keys on it)
        if (st->clip) {   // two launches more: the norm of the gradient the update is about to read, frozen slots left out
            // the running-norm rule keeps one reference per regime of the step -- before cls_warmup (none), entire-image, ordinary -- baked
            // into the launch sequence like the loss kernel's "counted": a by-value kernel argument, which an update of a pooled executable rewrites
            ClipAutoRule rule = st->clip_rule;
            rule.regime = !ssim_on ? -1 : entire ? 1 : 0;
            RC(grad_norm_launch(grads, adam_g2, st->pairs, st->astride, (size_t)st->nparams, st->clip_norm, st->clip_partials, st->clip,
                                stop_on ? st->stop : nullptr, st->dev_t, s, st->trace, st->trace_cap, rule.records ? &rule : nullptr));
            a.clip = st->clip; a.clip_stride = st->astride;
        }
        // keep-best: the record this launch reads was written by THIS step's loss kernel -- on the side stream's tail, in front of the
        // EV_JOIN2 wait above, or on the main stream in front of this launch -- so the update of the step that closes a best window sees it
        if (st->best) { a.best = st->best; a.best_p = st->best_p; a.best_ema = st->best_ema; }   // (another kernel, as with the average)
        if (st->opt_ext_on) { a.ext = &st->opt_ext; a.w = st->opt_w; }   // (another kernel again: the graph pool keys on the rule it selects)
        RC(optim_launch(a, s));
    }
    return SPLICE_OK;
}

// One step of every pair.  step_idx is the reference's data step counter (0-based, data/Dataset.py:57,63).
// params/grads/m/v: the generator arenas, [P][arena_stride] (one flat arena when P = 1).  A_crop / B_crop: [P][3][h][w]
// at the current crop sizes; A_entire [P][3][ent_h][ent_w] (may be NULL on steps where step_idx % entire_every != 0).
// losses_out: device fp32 [P][8], per pair {loss, loss_global_ssim, loss_entire_ssim, loss_entire_cls, loss_global_cls,
// loss_global_id_B, loss_global_tv, loss_global_pix_id_B} (inactive terms are 0; the last two only with splice_step_set_image_terms).
// The launch sequence (~500 kernels) is captured once per regime (first step / ordinary / entire-image) into a hipGraph
// and replayed; inputs are staged into handle-owned buffers first so the graph only ever sees the same pointers.
int splice_step_run(void* h, float* params, float* grads, float* m, float* v, const float* A_crop, const float* B_crop,
                    const float* A_entire, int step_idx, float* losses_out, splice_stream_t stream) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || !params || !grads || !m || !v || !A_crop || !B_crop || step_idx < 0) return SPLICE_ERR_ARG;
#ifdef SPLICE_DEV_SWITCHES
    ++g_splice_dev_steps;
#endif
    hipStream_t caller = (hipStream_t)stream;
    const splice_step_config& c = st->cfg;
    const int P = st->P;
    st->ev_slot = (st->ev_slot + 1) % SpliceStep::EV_RING;   // this call's set of cross-stream events
    ++st->runs;
    // ---- lambda schedule (util/losses.py:34-44)
    if (step_idx == c.cls_warmup) st->ssim_id_on = 1;
    const bool entire = c.ent_h > 0 && c.entire_every > 0 && (step_idx % c.entire_every == 0);
    if (entire && !A_entire) { splice_set_error("splice_step_run: step %d needs the entire structure image", step_idx); return SPLICE_ERR_ARG; }
    // Graphs pay off only while the launch sequence repeats: with random crop sizes (data/transforms.py:21) nearly every
    // step has new shapes, and re-capturing + instantiating ~600 nodes costs as much as the step itself (9.9 vs 5.8 ms
    // measured).  So a step whose arenas / crop sizes differ from the previous step's runs eagerly (same kernels, same
    // results) and a graph is captured only once the shapes have repeated (below).
    {
        void* ptrs[6] = {params, grads, m, v, losses_out, st->running};
        st->losses_out = losses_out;
        const int crops[4] = {c.crop_h, c.crop_w, st->cropb_h, st->cropb_w};
        if (memcmp(ptrs, st->graph_ptrs, sizeof(ptrs)) || memcmp(crops, st->graph_crops, sizeof(crops))) {
            st->graphs.retire();
            memcpy(st->graph_ptrs, ptrs, sizeof(ptrs));
            memcpy(st->graph_crops, crops, sizeof(crops));
            st->shape_repeats = 0;
            st->repeat_step = step_idx;
        } else if (step_idx != st->repeat_step) {
            // a step split into several calls (splice_step_set_phases: MultiScaleEngine runs phases 1|2, then 4, with identical
            // pointers and crop sizes) is ONE step: its later calls inherit the first call's eager / graph decision instead
            // of looking like a repeat and capturing a graph that the next step's new crop sizes drop again
            if (st->shape_repeats < 2) ++st->shape_repeats;
            st->repeat_step = step_idx;
        }
    }
    // (from the THIRD consecutive step with identical shapes on: under random crop sizes two equal steps in a row happen ~14 times
    // per 2000 steps, each time capturing ~600 nodes for ONE replay before the next size drops the graph again)
    const bool graph = st->use_graph && !splice_prof_active() && st->shape_repeats >= 2;
    hipStream_t s = caller;
    if (graph) {   // graphs cannot be captured on the legacy default stream: run on the handle's own stream, fenced by events
        s = st->own_stream;
        HIPCHK(hipEventRecord(st->ev(SpliceStep::EV_IN), caller));
        HIPCHK(hipStreamWaitEvent(s, st->ev(SpliceStep::EV_IN), 0));
    }
    if (st->leader) {
        const SpliceStep* ld = st->leader;
        if (ld->P != P || ld->Pa != st->Pa || ld->Pb != st->Pb || ld->pairs != st->pairs || ld->cfg.crop_h != c.crop_h || ld->cfg.crop_w != c.crop_w ||
            ld->cropb_h != st->cropb_h || ld->cropb_w != st->cropb_w || ld->cfg.ent_h != c.ent_h || ld->cfg.ent_w != c.ent_w) {
            splice_set_error("splice_step_run: a follower's images must have the leader's shapes");
            return SPLICE_ERR_ARG;
        }
    }
    // ---- stage the inputs (eager; with the generator forward: the other phases of the step see the same staged images)
    if (st->phases & 1) {
        StageArgs sa = {};
        const StepPtrs ip = step_ptrs(st);
        sa.src[0] = A_crop; sa.dst[0] = ip.a_in; sa.n[0] = (size_t)st->Pa * 3 * c.crop_h * c.crop_w;
        sa.src[1] = B_crop; sa.dst[1] = ip.b_in; sa.n[1] = (size_t)st->Pb * 3 * st->cropb_h * st->cropb_w;
        if (entire) { sa.src[2] = A_entire; sa.dst[2] = ip.e_in; sa.n[2] = (size_t)st->pairs * 3 * c.ent_h * c.ent_w; }
        sa.ip = st->dev_t; sa.iv = step_idx + 1;
        if (st->pair_lr) {
            sa.fp = st->dev_lrs; sa.nf = P;
            for (int p = 0; p < P; ++p) sa.fv[p] = st->lrs[p];
        } else if (st->lr_set || st->lr_state) {   // (the plateau lr rule reads its lr_in on the device: without a setter the handle stages cfg.lr itself)
            sa.fp = st->dev_lr; sa.nf = 1; sa.fv[0] = st->lr_set ? st->lr : c.lr;
        }
        if (st->pairs_in > 0) {   // the caller's batches hold pairs_in pairs: gather this handle's (same launch count, same staged bytes)
            StageRowsArgs ra = {};
            ra.a = sa;
            ra.blk[0] = (size_t)st->na * 3 * c.crop_h * c.crop_w;
            ra.blk[1] = (size_t)st->nb * 3 * st->cropb_h * st->cropb_w;
            ra.blk[2] = (size_t)3 * c.ent_h * c.ent_w;
            for (int p = 0; p < st->pairs; ++p) ra.rows[p] = st->in_rows[p];
            const int per_pair = st->na > st->nb ? st->na : st->nb;
            SPLICE_LAUNCH(stage_inputs_rows_kernel, dim3(128 * (per_pair > 4 ? 4 : per_pair), st->pairs), dim3(256), 0, s, ra);
        } else {
            SPLICE_LAUNCH(stage_inputs_kernel, dim3(128 * (P > 4 ? 4 : P)), dim3(256), 0, s, sa);
        }
    }
    // Steps whose shapes differ from the previous step's (the reference's random crop sizes) are launched eagerly.  Capturing EVERY such step into a
    // rotation of executables updated in place was built in round 5, is bit-equal and SLOWER (272.1 -> 265.9 steps/s: recording ~600 nodes +
    // hipGraphExecUpdate costs more host time than ~600 launches; profiles/r05_graph_every_step.txt); it left the library in round 6.
    if (!graph) {
        RC(step_body(st, params, grads, m, v, st->ssim_id_on != 0, entire, s));
    } else {
        const int variant = (st->ssim_id_on ? 1 : 0) | (entire ? 2 : 0) | (st->phases << 2);
        hipGraphExec_t ex = st->graphs.find(variant);
        if (!ex) {
            hipGraph_t g = nullptr;
            HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
            const int rc = step_body(st, params, grads, m, v, st->ssim_id_on != 0, entire, s);
            const hipError_t ee = hipStreamEndCapture(s, &g);
            if (rc != SPLICE_OK || ee != hipSuccess || !g) {
                if (g) (void)hipGraphDestroy(g);
                if (rc == SPLICE_OK) splice_set_error("splice_step_run: graph capture failed (%s)", hipGetErrorString(ee));
                return rc != SPLICE_OK ? rc : SPLICE_ERR_HIP;
            }
            // several pairs with n_crops: the layout is part of the pool key (other keys unchanged)
            const bool grouped = st->crops_mode && st->pairs > 1;
            // ... and so is the stop rule: its loss-kernel and update nodes are other kernels than those of a handle without it; and the
            // plateau lr rule, whose loss-kernel node is another kernel again
            const unsigned long long salt = (grouped ? ((unsigned long long)st->pairs << 32) | ((unsigned long long)st->na << 16) | (unsigned long long)st->nb : 0) |
                                            (st->stop_rule.window > 0 ? 1ull << 63 : 0) | (st->lr_state ? 1ull << 62 : 0) |
                                            // ... and the two image-space terms, a launch each (and another loss-kernel instance)
                                            (st->lambda_tv > 0.f ? 1ull << 61 : 0) | (st->lambda_pix > 0.f ? 1ull << 60 : 0) |
                                            // ... and the structure layers (bits 40-55: bit 55 on, 15 bits of a hash of the blocks and their weights): another
                                            // grid, other zeroing launches and key-gradient adds, another loss-kernel instance
                                            ssim_layers_salt(st) |
                                            // ... and the extended rule of the update (bits 56-59: off, or 1 + kind with the arenas it walks)
                                            (st->opt_ext_on ? (unsigned long long)(1 + st->opt_kind + 3 * ((st->opt_ext.momentum > 0.f ? 1 : 0) + 2 * (st->opt_ext.amsgrad || st->opt_ext.centered ? 1 : 0))) << 56 : 0);
            // ... and the [CLS] layers: a 64-bit hash of the blocks and their weight bits folded over the word (another loss launch, the seed adds)
            // ... and the identity layers, likewise (two other loss launches, the key-gradient tables of the y' chain, a zeroing launch per own block)
            // ... and the key second-moment term: its block and weight bits (three launches more, a zeroing launch and the x' chain's table)
            ex = st->graphs.adopt(variant, g, salt ^ cls_layers_salt(st) ^ id_layers_salt(st) ^ key_gram_salt(st) ^ key_nn_salt(st));
            if (!ex) return SPLICE_ERR_HIP;
        }
        HIPCHK(hipGraphLaunch(ex, s));
    }
    if (graph) {
        HIPCHK(hipEventRecord(st->ev(SpliceStep::EV_OUT), s));
        HIPCHK(hipStreamWaitEvent(caller, st->ev(SpliceStep::EV_OUT), 0));
    }
    if (st->dbg_sync) HIPCHK(hipStreamSynchronize(s));
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { splice_set_error("splice_step_run: %s", hipGetErrorString(e)); return SPLICE_ERR_HIP; }
    return SPLICE_OK;
}

// out[0..2] = captures that updated a pooled executable in place / updates the runtime refused (executable parked for good) / executables instantiated, by this handle
int splice_step_graph_stats(void* h, long long* out) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st || !out) return SPLICE_ERR_ARG;
    out[0] = st->graphs.updates; out[1] = st->graphs.refusals; out[2] = st->graphs.instantiations;
    return SPLICE_OK;
}

// 1 = replay captured hipGraphs (default), 0 = launch every kernel eagerly
int splice_step_use_graph(void* h, int on) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    st->use_graph = on ? 1 : 0;
    return SPLICE_OK;
}
// 1 = the independent chains of a step run on two streams (default), 0 = everything on one stream.  The results are
// bit-identical either way (every kernel is deterministic and owns its outputs); captured graphs are dropped.
int splice_step_use_overlap(void* h, int on) {
    SpliceStep* st = (SpliceStep*)h;
    if (!st) return SPLICE_ERR_ARG;
    if (st->overlap != (on ? 1 : 0)) st->graphs.retire();
    st->overlap = on ? 1 : 0;
    return SPLICE_OK;
}
}
