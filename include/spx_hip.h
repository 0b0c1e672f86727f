/*
 * spx_hip.h — C ABI of libspx_hip.so: the MI355X (gfx950) implementation of
 * ScaleProtoSeg's prototype-distance hot path.
 *
 * The reference has no FFI: its boundary for this path is the Python surface of
 * the PPNetMultiScale nn.Module.  The entry points below are the
 * device-side operators that surface needs; the Python package
 * `scaleprotoseg_amd` binds them with ctypes and mirrors the reference's
 * module/function names above them.  Each entry point cites the reference
 * code it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless named host_*; the caller owns and
 *    allocates every buffer (torch.empty); nothing is retained after return;
 *  - `stream` is a hipStream_t passed as void* (0 = default stream); calls only
 *    enqueue work, they never synchronise;
 *  - return 0 on success, non-zero on error; spx_last_error() gives the message
 *    of the last failing call of the calling thread;
 *  - tensors are dense, row-major, in the reference's layouts:
 *      features X   [B, C, H*W]      bf16 (x_dtype 0) or fp32 (x_dtype 1), C = S*Cs; the reference feeds a Sigmoid's
 *                                    output (values in (0, 1)).  The prototype gradient's product runs in fp16: features are
 *                                    taken exactly for 2^-14 <= |x| < 65520 and saturate at +-65504 beyond (never inf)
 *      bank         [P, Cs]          fp32   (prototype_vectors.view(P, Cs))
 *      distances    [B, P, H*W]      fp32
 *      activations  [B*H*W, P]       fp32   (NHWC pixel order)
 *      logits       [B*H*W, K]       fp32
 *      last layer W [K, P]           fp32
 */
#ifndef SPX_HIP_H
#define SPX_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SPX_MAX_PANELS 64   /* (scale, <=192-prototype block) work units per pixel tile */
#define SPX_ABI_VERSION 17
#define SPX_PRUNE_MAX_K 64   /* largest k of spx_prune_merge */

/* How the prototype bank is cut into MFMA panels.  Filled by spx_make_plan(). */
typedef struct spx_plan {
    int32_t num_prototypes;        /* P */
    int32_t num_classes;           /* K */
    int32_t num_scales;            /* S */
    int32_t channels_per_scale;    /* Cs (multiple of 16) */
    int32_t kc;                    /* channels staged per LDS step (32; a 16-channel tail is zero-filled) */
    int32_t npb;                   /* 32-prototype blocks per panel (2, 4 or 6) */
    int32_t ncb;                   /* 32-class blocks of the head (1, 2 or 5) */
    int32_t npanels;
    int32_t panel_ch0[SPX_MAX_PANELS];  /* first feature channel of the panel's scale */
    int32_t panel_p0[SPX_MAX_PANELS];   /* first prototype row of the panel */
    int32_t panel_np[SPX_MAX_PANELS];   /* prototypes in the panel (<= 32*npb) */
} spx_plan;

int spx_version(void);
const char* spx_last_error(void);

/* Build the panel plan from the module's scale table
 * (scale_num_prototypes, segmentation/model/model_multiscale.py:146-149, re-packed by
 * prune_prototypes :408-423).  host_scale_lo/hi: S entries each, HOST memory. */
int spx_make_plan(int32_t P, int32_t K, int32_t S, int32_t Cs,
                  const int32_t* host_scale_lo, const int32_t* host_scale_hi, spx_plan* out);

/* Sizes (bytes) of the packed operand buffers for a plan. */
size_t spx_packed_bank_bytes(const spx_plan* plan);   /* bf16 MFMA A-fragments of the bank          */
size_t spx_packed_bankT_bytes(const spx_plan* plan);  /* bf16 A-fragments of -2 bank^T (backward dX) */
size_t spx_packed_p2_bytes(const spx_plan* plan);     /* fp32 |p|^2 per padded prototype            */
size_t spx_packed_head_bytes(const spx_plan* plan);   /* split-bf16 (hi,lo) fragments of W          */
size_t spx_packed_headT_bytes(const spx_plan* plan);  /* split-bf16 fragments of W^T (backward)     */

/* Re-pack the fp32 bank into bf16 MFMA fragment order and compute |p|^2
 * (replaces the per-forward p**2 / sum of model_multiscale.py:270-274).
 * packed_bankT may be NULL when no backward is needed. */
int spx_pack_bank(const spx_plan* plan, const float* bank, void* packed_bank, void* packed_bankT,
                  float* packed_p2, void* stream);

/* Re-pack a dense [K, P] head matrix (last_layer.weight, model_multiscale.py:225; or the dense
 * form of the grouping projections) into split-bf16 fragments.  packed_headT may be NULL. */
int spx_pack_head(const spx_plan* plan, const float* W, void* packed_head, void* packed_headT, void* stream);

/* Everything one forward (+ backward) needs in ONE launch: spx_pack_bank + spx_pack_head (+ spx_pack_group_tail, and then the
 * head^T in the unit order of spx_pack_headT_units) - the per-step form for training, where every parameter changes between
 * steps and four small launches cost more than the packing itself.  W / Wg and their outputs may be NULL (no head / no
 * grouping tail); packed_bankT, packed_headT, packed_tailT NULL = no backward.  Same buffers and sizes as the single calls. */
int spx_pack_all(const spx_plan* plan, const float* bank, const float* W, const float* Wg, int32_t K2, void* packed_bank,
                 void* packed_bankT, float* packed_p2, void* packed_head, void* packed_headT, void* packed_tail,
                 void* packed_tailT, void* stream);

/* Fused forward: distances -> similarity -> linear head.
 * Replaces _scale_l2_convolution + _l2_convolution (model_multiscale.py:255-317),
 * distance_2_similarity (:324-330), the permute/contiguous/reshape (:369-370) and
 * run_last_layer (:243-244).  Any of distances/activations/logits may be NULL (not written).
 * act_fn: 0 = "log" (log((d+1)/(d+eps))), 1 = "linear" (-d). */
int spx_dist_fwd(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                 const void* packed_bank, const float* packed_p2, const void* packed_head,
                 float* distances, float* activations, float* logits,
                 float epsilon, int32_t act_fn, void* stream);

/* Backward, pixel side: recomputes the distance tile, forms
 *   G = (dDist + (dAct + dLogits.W) * act'(d)) * [d > 0]
 * and writes dX = 2 (rowsum_s(G) x - G.P) in X's dtype, plus two scratch buffers for spx_bank_bwd, both opaque to the caller:
 *   g_out  spx_bwd_scratch_bytes(): G as fp16 MFMA fragments with one power-of-two scale per 128-pixel tile;
 *   a_out  spx_bwd_head_scratch_bytes(): what d_W = dLogits^T . A needs - for heads of at most 32 rows the product itself,
 *          formed in this kernel as one fp32 partial per (panel, tile, 32-prototype block); for wider heads the activations
 *          as block-scaled int16 MFMA fragments.
 * Replaces autograd through model_multiscale.py:255-281,324-330,243-244.  d_dist / d_act / d_logits may be NULL (treated as
 * 0); dx may be NULL (X frozen); g_out / a_out may be NULL when the bank / head are frozen.
 *   dx_acc spx_bwd_dx_scratch_bytes() (0 for most plans -> NULL): a scale of more than 192 prototypes is walked as several
 *          panels, each adding its share of dX; with bf16 features that sum runs in this fp32 scratch and dX is rounded
 *          once (NULL: the partial sums pass through the bf16 dX, one rounding per panel). */
int spx_dist_bwd(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                 const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                 const void* packed_headT,
                 const float* d_dist, const float* d_act, const float* d_logits,
                 void* dx, void* dx_acc, void* g_out, void* a_out,
                 float epsilon, int32_t act_fn, void* stream);

/* Class-gathered variants: instead of the P-wide distance map, every pixel keeps only the
 * distances to the prototypes of ITS OWN class - the only entries KLDLoss reads for that pixel
 * (segmentation/model/loss.py:89-107; caller segmentation/model/module_multiscale.py:239-242) - so the fp32 map
 * and its gradient never cross HBM.
 *   labels     int32 [B, HW]: class 0..K-1 of the pixel; any other value = no class (its slots read 0)
 *   proto_key  uint32 [npanels * 32*npb], in the plan's padded row order: (class << 16) | slot, slot < J =
 *              rank of the prototype among its class's prototypes (ascending index); 0xFFFFFFFF = none / padding
 *   class_distances fp32 [B, J, HW] (slot planes): entry (slot, px) = distance of pixel px to prototype `slot` of class
 *              labels[px]; entries that no prototype maps to (every slot of a pixel without a class, the slots past its class's
 *              prototype count) are written as 0 by the kernel for classes below 1024 - the planes may arrive uninitialised;
 *              tables with larger class ids: the caller zero-fills.
 * Everything else as in spx_dist_fwd / spx_dist_bwd. */
int spx_dist_fwd_cls(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                     const void* packed_bank, const float* packed_p2, const void* packed_head,
                     const int32_t* labels, const uint32_t* proto_key, int32_t J,
                     float* class_distances, float* activations, float* logits,
                     float epsilon, int32_t act_fn, void* stream);
int spx_dist_bwd_cls(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                     const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                     const void* packed_headT,
                     const int32_t* labels, const uint32_t* proto_key, int32_t J,
                     const float* d_class_distances, const float* d_act, const float* d_logits,
                     void* dx, void* dx_acc, void* g_out, void* a_out,
                     float epsilon, int32_t act_fn, void* stream);

/* Scale-parallel forward for pixel grids that do not fill the chip (the reference trains on crops: 10 x 65 x 65 latent
 * pixels = 331 tiles for 512+ workgroup slots, each tile walking every scale's panels one after the other).  The scales
 * are independent work (segmentation/model/model_multiscale.py:283-317 is a Python loop over them), so each runs as its
 * own workgroup; only the logits - a sum over ALL prototypes - need the per-scale partials summed, in scale order, by a
 * second small kernel.  spx_fwd_split_groups(): how many groups the library uses for this problem (1 = the single walk);
 * spx_dist_fwd_ws = spx_dist_fwd / spx_dist_fwd_cls (labels_cls / proto_key NULL = the P-wide map) with a workspace of
 * spx_fwd_split_workspace_bytes() for those partials (NULL or 0 bytes: the single walk).  Launches without a logits
 * output (and the pixel-side backward, which has no cross-scale term at all) split on their own. */
int32_t spx_fwd_split_groups(const spx_plan* plan, int32_t B, int32_t HW);
size_t spx_fwd_split_workspace_bytes(const spx_plan* plan, int32_t B, int32_t HW);
int spx_dist_fwd_ws(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                    const void* packed_bank, const float* packed_p2, const void* packed_head,
                    const int32_t* labels_cls, const uint32_t* proto_key, int32_t J, float* class_distances,
                    float* distances, float* activations, float* logits, void* split_workspace,
                    float epsilon, int32_t act_fn, void* stream);

/* Pixel-wise cross entropy on the path's logits (segmentation/model/loss.py:9-48, caller
 * segmentation/model/module_multiscale.py:239): CE = mean over the non-ignored pixels of
 * logsumexp_k(logits[px]) - logits[px, label[px]].
 *   labels    int32 [B*HW]: class 0..K-1 of the pixel (the reference's target - 1); any other value = ignored
 *   lse       fp32  [B*HW]: per-pixel logsumexp (forward output, backward input)
 *   pred      int32 [B*HW]: argmax class, lowest index on ties (optional forward output: `correct`, loss.py:43-46)
 *   partials  fp32  [2 * spx_ce_partials(...)]: (sum of the per-pixel losses, number of non-ignored pixels) pairs, one
 *             per wave; the caller sums them (fixed shape, fixed order: deterministic) and divides
 *   logits    the forward's logits (backward input)
 *   coef      DEVICE scalar: dLoss/dCE / number of non-ignored pixels
 *   d_logits_out fp32 [B*HW, K]: coef * (softmax - onehot) (0 on ignored pixels), formed by the pixel-side backward for
 *             spx_bank_bwd's d_logits operand
 * spx_dist_fwd_ce = spx_dist_fwd / spx_dist_fwd_cls (labels_cls / proto_key NULL = the P-wide map) with the CE
 * statistics computed on the logits tile while it is still in registers (8 B/px of extra output instead of separate
 * log_softmax / nll passes over the [B*HW, K] tensor); spx_dist_bwd_ce = spx_dist_bwd / spx_dist_bwd_cls taking
 * (logits, lse, labels, coef) in place of d_logits.  spx_ce_fwd / spx_ce_bwd are the same arithmetic as stand-alone
 * kernels over any [M, K] logits (heads the fused kernels do not carry: more than 160 classes, the grouping tail). */
typedef struct spx_ce {
    const int32_t* labels;
    float* lse;
    int32_t* pred;
    float* partials;
    const float* logits;
    const float* coef;
    float* d_logits_out;
} spx_ce;
size_t spx_ce_partials(int32_t B, int32_t HW);       /* (sum, count) pairs the fused forward writes */
size_t spx_ce_partials_flat(int64_t M);              /* ... and spx_ce_fwd */
int spx_dist_fwd_ce(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                    const void* packed_bank, const float* packed_p2, const void* packed_head,
                    const int32_t* labels_cls, const uint32_t* proto_key, int32_t J, float* class_distances,
                    float* distances, float* activations, float* logits, const spx_ce* ce,
                    float epsilon, int32_t act_fn, void* stream);
int spx_dist_bwd_ce(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                    const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                    const void* packed_headT,
                    const int32_t* labels_cls, const uint32_t* proto_key, int32_t J,
                    const float* d_dist, const float* d_class_distances, const float* d_act, const spx_ce* ce,
                    void* dx, void* dx_acc, void* g_out, void* a_out,
                    float epsilon, int32_t act_fn, void* stream);
int spx_ce_fwd(const float* logits, const int32_t* labels, int64_t M, int32_t K, float* lse, int32_t* pred,
               float* partials, void* stream);
int spx_ce_bwd(const float* logits, const float* lse, const int32_t* labels, const float* coef, int64_t M, int32_t K,
               float* d_logits, void* stream);
/* mean loss -> loss[0], (count, loss sum) -> count_sum[0..1] from the (sum, count) partial pairs the cross-entropy kernels leave
 * (spx_ce_fwd / the fused epilogues / the grouping tail): one launch, fixed summation order; 0 / 0 = nan as torch's mean over
 * no pixel (loss.py:36-40).  spx_shift_labels: out = labels - 1 as int32 (loss.py:32) from int64 (is_int64 = 1) or int32 labels. */
int spx_ce_finish(const float* partials, int64_t n_pairs, float* loss, float* count_sum, void* stream);
int spx_shift_labels(const void* labels, int32_t is_int64, int64_t n, int32_t* out, void* stream);

/* Segmented cross entropy: S <= 16 row ranges of ONE [M, K] logits tensor (the packed MSC training maps: the four maps'
 * logits of one distance launch), each with its own mean and its own backward coefficient, in one forward, one finish and
 * one backward launch.  Segment k is the rows [off[k], off[k+1]); off[0] = 0, off[S] = M, every segment non-empty.  The
 * table is copied into the kernel arguments: no device table, and a captured launch keeps the layout it was captured with.
 *   spx_ce_seg_partials  number of (loss sum, valid count, correct count) fp32 triples the forward writes: 4 per started
 *                        block of 256 rows of every segment (0 with spx_last_error() for a bad table)
 *   spx_ce_seg_fwd       lse [M], pred [M] (may be NULL) and the triples; block j of segment k starts at row off[k] + 256 j,
 *                        so no wave holds rows of two segments
 *   spx_ce_seg_finish    losses[k] = sum_k / count_k (0 / 0 = nan), mean[0] = (((l_0 + l_1) + l_2) + ...) / S, count[k] the fp32
 *                        divisor, valid[k] / correct[k] int32 (correct: a valid row whose pred equals its label)
 *   spx_ce_seg_bwd       d_logits[m, :] = c_k (softmax - onehot) on the valid rows of segment k and exactly 0 on the ignored
 *                        ones, c_k = (g_losses[k] + g_mean[0] / S) / count[k]; g_losses / g_mean are DEVICE arrays, NULL = 0
 * For every segment losses[k], the lse / pred rows, the counts and d_logits carry the bits spx_ce_fwd / spx_ce_finish /
 * spx_ce_bwd give on the contiguous slice with coef = g / count: the same lanes, the same summation order.  No float
 * atomics, no workspace besides the triples, no host read. */
typedef struct spx_ce_segments {
    int32_t S;
    int64_t off[17];
} spx_ce_segments;
size_t spx_ce_seg_partials(const spx_ce_segments* seg);
int spx_ce_seg_fwd(const float* logits, const int32_t* labels, const spx_ce_segments* seg, int32_t K, float* lse, int32_t* pred,
                   float* partials, void* stream);
int spx_ce_seg_finish(const float* partials, const spx_ce_segments* seg, float* losses, float* mean, float* count, int32_t* valid,
                      int32_t* correct, void* stream);
int spx_ce_seg_bwd(const float* logits, const float* lse, const int32_t* labels, const spx_ce_segments* seg, const float* count,
                   const float* g_losses, const float* g_mean, int32_t K, float* d_logits, void* stream);

/* out [n1, n2] = a^T . b for tall-skinny fp32 operands a [M, n1], b [M, n2] with n1 * n2 <= 8192: the d W_g = d_logits^T . g
 * product of the grouping tail (segmentation/model/model_multiscale_group.py:305-308 through autograd) and its relatives.
 * Deterministic (per-workgroup partials summed in workgroup order).  workspace: spx_pixel_outer_workspace_bytes(). */
size_t spx_pixel_outer_workspace_bytes(int64_t M, int32_t n1, int32_t n2);
int spx_pixel_outer(const float* a, const float* b, int64_t M, int32_t n1, int32_t n2, float* out, void* workspace, void* stream);

/* Heads wider than the distance kernels carry (more than 160 rows: scaleproto_coco.gin's 182 classes, the 450 / 546 grouping
 * units of group_scaleproto_ade.gin / _coco.gin; a grouping tail over more than 32 classes) and the head behind a user-supplied
 * similarity: the three products of the reference's nn.Linear (segmentation/model/model_multiscale.py:243-244,
 * model_multiscale_group.py:283-308, and their autograd) as ONE fp32 MFMA kernel family on row-major device tensors,
 *     C[i][j] = sum_k A(i, k) * B(j, k),   A(i, k) = A[i * a_row_stride + k * a_k_stride]  (B alike),
 * for i < M, j < N, k < K; per operand one of the two strides must be 1.  y = a . w^T: (a, P, 1), (w, P, 1); d_a = g . w:
 * (g, N, 1), (w, 1, P); d_w = g^T . a: (g, 1, N), (a, 1, P).  flags: 1 = A elements enter as exp(A) and 2 = B elements as exp(B)
 * (the grouping tail's exp(units)), 4 = C[i][j] is multiplied by exp(E[i * lde + j]) (its backward d_units).  fp32 operands and
 * accumulation (v_mfma_f32_32x32x2_f32); long contractions over few output tiles are split into workspace slabs summed in a fixed
 * order (deterministic).  workspace: spx_rows_gemm_workspace_bytes() (may be 0 -> NULL accepted). */
size_t spx_rows_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t flags);
int spx_rows_gemm(const float* A, int64_t a_row_stride, int64_t a_k_stride, const float* B, int64_t b_row_stride,
                  int64_t b_k_stride, float* C, int64_t ldc, int32_t M, int32_t N, int32_t K, int32_t flags, const float* E,
                  int64_t lde, void* workspace, void* stream);

/* Grouping head with the tail as its own kernel: the unit product runs in the distance kernel, then a small fp32 kernel
 * forms g = exp(units), logits = W_g . g and - when `ce` is given - the cross-entropy statistics of the logits it has just
 * formed (partials: spx_ce_partials_flat(B*HW) pairs).  Wg: the RAW last_layer_group.weight [K2, U] fp32.
 * workspace: spx_group_tail_workspace_bytes().  spx_dist_bwd_group_ce = spx_dist_bwd_group with (logits, lse, labels,
 * coef) in place of d_logits; d_logits_out then carries the formed [B*HW, K2] gradient (for d_W_g = d_logits^T . g). */
size_t spx_group_tail_workspace_bytes(const spx_plan* plan, int32_t B, int32_t HW);
int spx_dist_fwd_group_ws(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                          const void* packed_bank, const float* packed_p2, const void* packed_head,
                          const float* Wg, int32_t K2, float* distances, float* activations,
                          float* group_activations, float* logits, const spx_ce* ce, void* workspace,
                          float epsilon, int32_t act_fn, void* stream);
int spx_dist_bwd_group_ce(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                          const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                          const void* packed_headT_units, const void* packed_tailT, int32_t K2,
                          const float* group_activations, const float* d_dist, const float* d_act,
                          const spx_ce* ce, const float* d_group_activations, float* d_units, void* dx, void* dx_acc, void* g_out,
                          void* a_out, float epsilon, int32_t act_fn, void* stream);

/* Grouping head with its tail fused (segmentation/model/model_multiscale_group.py:283-308, run_last_layer):
 *   units = act . Wd^T   (Wd = the dense [U = G*K', P] form of the per-class group_projection matrices, packed with
 *                         spx_pack_head for a plan whose num_classes = U)
 *   g = exp(units);  logits = g . W_g^T   (W_g = last_layer_group.weight [K2, U], K2 <= 32)
 * spx_pack_group_tail re-packs W_g (packed_tail: forward, packed_tailT: backward, spx_packed_tail_bytes() each);
 * spx_pack_headT_units is spx_pack_head's transposed output with the unit index in accumulator order (the
 * backward builds its dUnits operand in registers): spx_packed_headT_bytes().
 * Forward: logits [B*HW, K2]; group_activations [B*HW, U] = g (optional output, required by the backward).
 * Backward: d_logits [B*HW, K2] in, optionally d_group_activations [B*HW, U] (a gradient on g itself: KLDLossGroup on
 * compute_group's list, segmentation/model/module_multiscale_group_train.py:242-262; NULL = none); d_units [B*HW, U] =
 * (d_logits . W_g + d_group_activations) * g out (the d_logits operand of spx_bank_bwd, which then yields d_Wd);
 * d_W_g = d_logits^T . g is a [K2, U] product left to the caller.
 * spx_exp / spx_exp_bwd: y = exp(x) and dx = g * y over n fp32 elements - the same g for heads the fused kernels do not
 * carry, and for compute_group() on activations that did not come out of the fused forward. */
/* Dense [U, P] head matrix of the grouping head from the per-class projection weights (group_projection[j].weight [g_j, n_j],
 * segmentation/model/model_multiscale_group.py:249-269): out[u][p] = W_j[row_local[u]][col_local[p]] where row_block[u] ==
 * col_block[p] == j, 0 elsewhere (one launch; every element written).  block_ptrs / block_cols: HOST arrays of nblocks (<= 192)
 * DEVICE pointers / column counts n_j; row_block, row_local [U] and col_block, col_local [P]: device int32 tables (block -1 =
 * belongs to no class present).  spx_group_dense_bwd: the adjoint - d_flat[i] = d_out[flat_row[i]][flat_col[i]] for the n weight
 * elements in block order (the caller hands out views of d_flat as the weights' gradients). */
int spx_group_dense(const float* const* block_ptrs, const int32_t* block_cols, int32_t nblocks, const int32_t* row_block,
                    const int32_t* row_local, const int32_t* col_block, const int32_t* col_local, int32_t U, int32_t P, float* out,
                    void* stream);
int spx_group_dense_bwd(const float* d_out, const int32_t* flat_row, const int32_t* flat_col, int64_t n, int32_t P, float* d_flat,
                        void* stream);
/* In-place Euclidean projection of every ROW of the group projections onto the simplex {w >= 0, sum w = z} in one launch
 * (segmentation/utils.py:113-124 projection_simplex_sort, once per class after every optimizer step of the group phase,
 * segmentation/model/module_multiscale_group_train.py:337-338).  block_ptrs / block_rows / block_cols: HOST arrays of nblocks
 * DEVICE pointers to contiguous fp32 matrices [G_j, n_j], their row counts G_j and column counts n_j.  Per row: u = the row in
 * descending order; css_k = fp32(sum_{i<=k} u_i) - z, the sum kept in float64, added in order, rounded per element; rho = the
 * largest k with u_k - css_k / k > 0 (fp32); theta = css_rho / rho; w = v - theta where that is not below 0, else 0.  Bit-identical
 * to the stock formula on a CPU copy of the row; no atomics, run-to-run identical.  A row holding a NaN comes back all NaN, the
 * other rows are untouched by it.  Enqueues on `stream` only.  Limits: 1 <= nblocks <= 192, G_j >= 1, 1 <= n_j <= 1024, at
 * most 2^31 - 1 rows; a violation or a NULL pointer returns non-zero and launches nothing. */
int spx_simplex_project(float* const* block_ptrs, const int32_t* block_rows, const int32_t* block_cols, int32_t nblocks, float z,
                        void* stream);
size_t spx_packed_tail_bytes(const spx_plan* plan);
int spx_pack_group_tail(const spx_plan* plan, const float* Wg, int32_t K2, void* packed_tail, void* packed_tailT,
                        void* stream);
int spx_pack_headT_units(const spx_plan* plan, const float* W, void* packed_headT_units, void* stream);
int spx_dist_fwd_group(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                       const void* packed_bank, const float* packed_p2, const void* packed_head,
                       const void* packed_tail, int32_t K2,
                       float* distances, float* activations, float* group_activations, float* logits,
                       float epsilon, int32_t act_fn, void* stream);
int spx_dist_bwd_group(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                       const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                       const void* packed_headT_units, const void* packed_tailT, int32_t K2,
                       const float* group_activations, const float* d_dist, const float* d_act,
                       const float* d_logits, const float* d_group_activations, float* d_units, void* dx, void* dx_acc, void* g_out,
                       void* a_out, float epsilon, int32_t act_fn, void* stream);
int spx_exp(const float* x, float* y, int64_t n, void* stream);
int spx_exp_bwd(const float* g, const float* y, float* dx, int64_t n, void* stream);

/* Bytes of the g_out and of the a_out scratch of spx_dist_bwd. */
size_t spx_bwd_scratch_bytes(const spx_plan* plan, int32_t B, int32_t HW);
size_t spx_bwd_head_scratch_bytes(const spx_plan* plan, int32_t B, int32_t HW);
size_t spx_bwd_dx_scratch_bytes(const spx_plan* plan, int32_t x_dtype, int32_t B, int32_t HW);

/* Backward, parameter side: d_bank [P, Cs] = 2 (p colsum(G) - G^T X) as a pixel-split MFMA reduction with per-workgroup
 * fp32 partial slabs, and d_W [K, P] = dLogits^T A from spx_dist_bwd's a_out (the tile partials of a head of at most 32 rows
 * are summed; for a wider head the product is formed here from the activation fragments and d_logits, which may be NULL
 * otherwise).  Every sum runs in a fixed order (no float atomics: replicas stay bit-identical).
 * workspace: spx_bank_bwd_workspace_bytes().  d_bank / d_W may be NULL. */
size_t spx_bank_bwd_workspace_bytes(const spx_plan* plan, int32_t B, int32_t HW);
int spx_bank_bwd(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                 const float* bank, const void* g_in, const void* a_in, const float* d_logits,
                 float* d_bank, float* d_W, void* workspace, void* stream);

/* Class-masked per-prototype argmin over the latent grid (prototype push).
 * Replaces the one_hot / matmul / masked add / two min() reductions of
 * segmentation/push_multiscale_optimization.py:74-91.  labels: int32 [B, HW], already resized with
 * resize_label (dataset.py:22-30); label == void_class (or outside 0..K) matches no prototype;
 * void_class < 0 means labels are 0..K-1 with no void.  class_identity: fp32 [P, K].
 * Outputs: indices int64 [B, P] (flat i*W+j, lowest index on ties), values fp32 [B, P].
 * scratch: uint64 [B*P]. */
int spx_push_argmin(const float* distances, const int32_t* labels, const float* class_identity,
                    int32_t B, int32_t P, int32_t K, int32_t HW, int32_t void_class, float max_dist,
                    int64_t* indices, float* values, uint64_t* scratch, void* stream);

/* The same reduction FUSED into the distance kernel (the P-wide distance map is never written): features in, per
 * (image, prototype) minimum + flat index out.  labels / void_class / K: exactly as spx_push_argmin takes them (raw int32
 * [B, HW] labels; label == void_class or outside the K classes matches no prototype; void_class < 0: labels are 0..K-1);
 * proto_key: the (class << 16 | slot) table of spx_dist_fwd_cls (class of every padded prototype row) in place of the
 * fp32 class_identity - i.e. a one-hot prototype_class_identity, which is what the reference builds
 * (model_multiscale.py:89-97).
 * Arithmetic and tie rule as spx_push_argmin (distances as spx_dist_fwd computes them; d + max_dist * (1 - mask) rounded
 * as the reference rounds it; lowest flat index on ties; absent class -> (0, max_dist)).  Integer atomic minima:
 * run-to-run identical.  scratch: uint64 [B*P]. */
int spx_dist_push_min(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                      const float* packed_p2, const int32_t* labels, int32_t void_class, int32_t K, const uint32_t* proto_key,
                      float max_dist, int64_t* indices, float* values, uint64_t* scratch, void* stream);

/* Lexicographic (value, image) argmin over images per prototype: tot_dist.argmin(dim=0),
 * push_multiscale_optimization.py:135-137.  values fp32 [N, P] -> best int64 [P]. */
int spx_argmin_images(const float* values, int32_t N, int32_t P, int64_t* best, void* stream);

/* KLD loss over class-gathered distances (segmentation/model/loss.py:51-146).  vals fp32 [B, J, HW]
 * (the slot planes of spx_dist_fwd_cls), labels int32 [B, HW].  A segment = (image, class).  Four streaming passes,
 * each reading vals once; all segment reductions use integer atomics (run-to-run identical results):
 *   spx_kld_segment_max    smax_keys uint32 [B, K, J] (caller zero-fills): ordered key of max_px vals over the segment
 *                          (key k -> float: k & 0x80000000 ? k ^ 0x80000000 : ~k); counts uint32 [B, K] (zero-filled,
 *                          may be NULL): pixels per segment (loss.py:113-127 skips segments of fewer than two);
 *                          range_keys uint32 [2] (zero-filled, may be NULL): ordered keys of max(v) and max(-v) over
 *                          every value that enters a segment (the value range the fixed-point scale below is sized for)
 *   spx_kld_segment_sumexp ssum_fx uint64 [B, K, J] (zero-filled): sum_px exp(vals - smax) * 2^40, smax from the keys
 *   spx_kld_segment_lse    lse fp32 [n = B*K*J]: smax + log(ssum_fx / 2^40), 0 for a segment without pixels; with `scale`
 *                          (ONE double in device memory; needs range_keys and HW) also the fixed-point scale of the
 *                          pair sums: the power of two 2^floor(log2(2^61 / (HW * (max - min + 32)))) - no host sync
 *   spx_kld_pair_sums      a_fx int64 [B, K, J, J] (zero-filled): sum_px p_j * (l_k - l_j) * scale = -KL(j || k) of the
 *                          segment, i.e. the Gram matrix sum_px p_j l_k minus its row's diagonal entry (diagonal 0);
 *                          scale: ONE double in DEVICE memory, so the caller can derive it from the data without a
 *                          host sync; l = vals - lse (the log_softmax over the segment's pixels, loss.py:110), p = exp(l).
 *   spx_kld_backward       grad fp32 [B, J, HW] = dLoss/dvals given A = a_fx / scale and Cf = dLoss/dA [B, K, J, J]
 *                          (diagonal entries of Cf are not read: A's diagonal is identically 0)
 * W (the three reduction passes): row length of the pixel grid (must divide HW) lets a wave take the pixels as compact
 * 16 x 4 blocks down a 16-pixel column strip, which cross fewer class boundaries than a row segment (partial results are
 * published per class run); 0 = unknown
 * (linear walk).  W changes only the rounding of fp32 partial sums.
 *   spx_kld_gram_loss      the [B, K, J, J]-sized algebra between the passes (loss.py:113-142), one workgroup per segment
 *                          + a one-workgroup finish: A = a_fx / scale [nseg = B*K, J, J]; kld_jk = (A_jj + A_kk - A_jk -
 *                          A_kj) / 2; an entry is valid when pair_ok[class][j][k] (uint8 [K, J, J]: j < k, both slots exist,
 *                          same scale) and the segment has >= 2 pixels; loss[0] = mean over the valid entries of exp(-kld)
 *                          (0 if none), loss[1] = 1 / max(number of valid entries, 1); Cf = dLoss/dA WITHOUT that factor
 *                          (spx_kld_backward applies it: cf_scale); partials: double [2 * nseg] scratch.  Fixed-order sums.
 *   spx_kld_backward       cf_scale: ONE float in device memory that multiplies Cf (NULL = 1): the caller's
 *                          dLoss_total/dLoss times loss[1], formed on the device
 * J <= 16 and K*J*J*8 bytes must fit the LDS table (~60 KiB). */
int spx_kld_segment_max(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t W, int32_t K,
                        uint32_t* smax_keys, uint32_t* counts, uint32_t* range_keys, void* stream);
int spx_kld_segment_sumexp(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t W, int32_t K,
                           const uint32_t* smax_keys, uint64_t* ssum_fx, void* stream);
int spx_kld_segment_lse(const uint32_t* smax_keys, const uint64_t* ssum_fx, int32_t n, float* lse, const uint32_t* range_keys,
                        int32_t HW, double* scale, void* stream);
int spx_kld_gram_loss(const int64_t* a_fx, const double* scale, const uint32_t* counts, const uint8_t* pair_ok, int32_t nseg, int32_t K,
                      int32_t J, float* A, float* Cf, double* partials, float* loss, void* stream);
int spx_kld_pair_sums(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t W, int32_t K,
                      const float* lse, const double* scale, int64_t* a_fx, void* stream);
int spx_kld_backward(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t K,
                     const float* lse, const float* A, const float* Cf, const float* cf_scale, float* grad, void* stream);

/* Evaluation maps: F.interpolate(src, size=(H, W), mode="bilinear", align_corners=False) followed
 * by argmin (take_max = 0) or argmax (take_max = 1) over the channel dimension, without materialising the
 * upsampled [N, C, H, W] tensor (segmentation/eval_valid_multiscale.py:229-234, :375-383: nearest prototype per
 * full-resolution pixel from the distance map, predicted class from the logits).  src fp32 [N, C, h, w];
 * indices int64 [N, H, W] (lowest channel on ties); values fp32 [N, H, W] (the extremum; may be NULL). */
int spx_upsample_argext(const float* src, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                        int32_t take_max, int64_t* indices, float* values, void* stream);

/* Evaluation metrics: the counters segmentation/eval_valid_multiscale.py:229-269 derives from the
 * full-resolution maps above, accumulated without writing those maps.  Per image n, on the bilinear maps of
 * spx_upsample_argext's arithmetic: pred = argmax_c logits, near = argmin_p distances (lowest index on ties).
 * Counters are int64 and ADDED to (zero them once, call once per batch).
 *   logits     fp32 [N, h, w, K] addressed through host_logit_strides = element strides of (n, k, y, x)
 *   distances  fp32 [N, P, h, w] addressed through host_dist_strides  = element strides of (n, p, y, x); may be NULL
 *   labels     [N, H, W] contiguous, label_bytes 1 (uint8), 4 (int32) or 8 (int64); 0 = void, c + 1 = class c, any
 *              other non-zero value is non-void and matches no class (the reference's `ann != 0`)
 *   proto_class int32 [P]: cls(p), the first argmax of prototype_class_identity[p] (:109-112)
 *   conf       [K + 1, K]: conf[r, pred] += 1 per non-void pixel, r = ann - 1 for 1 <= ann <= K, else K (:236-243)
 *   hits       [P]: hits[near] += 1 per pixel (void included) with cls(near) == pred (:245-253)
 * Sizes: K <= 1024, P <= 4096, N*H*W < 2^31.  Entries of proto_class outside [0, K) match no class. */
int spx_eval_accumulate(const float* logits, const int64_t* host_logit_strides, const float* distances,
                        const int64_t* host_dist_strides, const int32_t* proto_class, const void* labels, int32_t label_bytes,
                        int32_t N, int32_t K, int32_t P, int32_t h, int32_t w, int32_t H, int32_t W, int64_t* conf,
                        int64_t* hits, void* stream);
/* Top-k class purity of sample pixels (:255-269).  samples [N, S, 2] = (y, x) per image, int32 (sample_bytes 4) or int64
 * (sample_bytes 8), duplicates allowed, N*S < 2^24.  Per
 * sample: the P interpolated distances in ascending order, ties by lower index (stable), hit_j = cls(order_j) == pred;
 * topk[k] += sum_{j <= k} hit_j for k < P; seen (int64 [1], may be NULL) += 1.  Samples outside [0, H) x [0, W) are
 * skipped and not counted. */
int spx_eval_topk(const float* logits, const int64_t* host_logit_strides, const float* distances, const int64_t* host_dist_strides,
                  const int32_t* proto_class, const void* samples, int32_t sample_bytes, int32_t N, int32_t S, int32_t K,
                  int32_t P, int32_t h, int32_t w, int32_t H, int32_t W, int64_t* topk, int64_t* seen, void* stream);
/* Host-side check of a proto_class table before it is uploaded: every entry in [0, K) (non-zero status otherwise). */
int spx_eval_check_classes(const int32_t* host_classes, int32_t P, int32_t K);

/* Prototype pruning: the k nearest training patches of every prototype (find_nearest.py:88-225 with full_save=True, as
 * prune.py:22-30 calls it).  Per image and prototype the nearest latent pixel is kept as one 64-bit key:
 *   bits 63..32 = float bits of d | void << 31, bits 31..0 = flat latent index i*W + j.
 * d >= 0, so the bits order as the value; void = the pixel's label equals void_label.  The minimum key is the reference's
 * np.amin / np.argmin of `proto_dist_ + 10e6 * (interpolated_y == -1)` (:118-142, a float64 sum): the nearest non-void
 * pixel of an image with any; for an all-void image the nearest pixel, ranked after every non-void candidate; the
 * lowest flat index on ties (first occurrence).  Integer atomic minima: run-to-run identical.
 * spx_prune_argmin: on a distance map fp32 [B, P, HW] already in HBM (as spx_push_argmin serves the push); labels
 * int32 [B, HW] at the latent resolution (resize_label, dataset.py:22-30); keys uint64 [B, P] written here. */
int spx_prune_argmin(const float* distances, const int32_t* labels, int32_t void_label, int32_t B, int32_t P, int32_t HW,
                     uint64_t* keys, void* stream);
/* The same keys FUSED into the distance kernel (the P-wide map is never written), bit-identical to spx_prune_argmin on the
 * map spx_dist_fwd writes.  Arguments as spx_dist_push_min; proto_key: any table of the plan's padded rows (read, not
 * used for masking).  keys uint64 [B, P] written here. */
int spx_dist_prune_min(const spx_plan* plan, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                       const float* packed_p2, const int32_t* labels, int32_t void_label, const uint32_t* proto_key, uint64_t* keys,
                       void* stream);
/* Footprint of every key's latent cell (i, j) = (flat / W, flat % W) in the full-resolution label (:145-158), computed in
 * float64 exactly as written: ph = Hf / H, pw = Wf / W; box = (int(i*ph), int((i+1)*ph), int(j*pw), int((j+1)*pw)),
 * stops clamped to Hf / Wf as a NumPy slice clamps them.  labels int32 [B, Hf, Wf] in the reference's convention there
 * (convert_targets(target) - 1: void = -1); target_class int32 [P] = argmax of prototype_class_identity[p] (0 for an
 * all-zero row).  Outputs: box int32 [B, P, 4] (h0, h1, w0, w1; zero area = empty footprint, the candidate the
 * reference skips, :168-169) and label int32 [B, P] (:206-213): target_class[p] if any footprint pixel equals it, else
 * the most frequent value, the smallest value on a count tie (np.unique + argmax); 0 for an empty footprint.  Any int32
 * value counts as a value; values -1 .. 1022 are counted in an LDS histogram, others pairwise. */
int spx_prune_footprint(const int32_t* labels, int32_t B, int32_t Hf, int32_t Wf, int32_t H, int32_t W, int32_t P,
                        const uint64_t* keys, const int32_t* target_class, int32_t* label, int32_t* box, void* stream);
/* Merge the candidates of B consecutive images (global indices image0 .. image0 + B - 1, later than every image already in
 * the table) into the running table of the k nearest per prototype (:222-225), 1 <= k <= SPX_PRUNE_MAX_K.  Table rows
 * [P, k]: table_key uint64 (a key above), table_image int64 (-1 = empty slot; empty slots come last), table_label int32,
 * table_box int32 [.., 4], table_cell int32 [.., 2] = (i, j) for a grid of width W.  Initialise key to all ones and image
 * to -1.  Candidates with an empty footprint are skipped.  A row holds the k smallest candidates by (key bits 63..32,
 * image), in that order: a candidate replaces the last kept one only if its key is strictly smaller, so on an equal
 * distance the earlier image stays (heapq.heappushpop).  The reference evicts whichever of several entries tied at the
 * k-th distance sits at its heap's root; this rule keeps the earliest of them.  box / table_box 16-byte aligned. */
int spx_prune_merge(const uint64_t* keys, const int32_t* label, const int32_t* box, int32_t B, int32_t P, int32_t W, int64_t image0,
                    int32_t k, uint64_t* table_key, int64_t* table_image, int32_t* table_label, int32_t* table_box, int32_t* table_cell,
                    void* stream);

/* Weight-side regularisers of the training objective (additive to ABI 17).  For class block j (the j-th class that owns
 * prototypes), G groups, n_j columns, w[g][c] = wd[u0_j + g][flat_col[off_j + c]]:
 *   term 0 EntropyGroup      mean_(j,g) -sum_c w log(w + eps) / log(n_j)               (segmentation/model/loss.py:398-426)
 *   term 1 CrossEntropyGroup -mean_(j,i!=l) -sum_c w[i,c] log(max(w[l,c], eps))        (:429-464)
 *   term 2 ScaleMax          -mean_(j,s: span non-empty) mean_g max_(c in span(j,s)) w  (:351-395; gradient to the first max)
 *   term 3 L1                sum |head[k][u] (1 - ident[u][k])|                         (module_multiscale.py:260-261,
 *                                                                                        module_multiscale_group_train.py:283-285)
 * total = ((weights[3] l1 + weights[1] t1) + weights[2] t2) + weights[0] t0, the reference's order (:288-297).  Bit b of
 * `terms` enables term b; a disabled term is 0 and gets no gradient.  Group terms need wd and the GroupTables; L1 needs head
 * and ident.  Limits: nblocks <= 192, 1 <= G <= 16, 1 <= S <= 16, n_j <= 4096, U*P and K*Uh < 2^31.  No float atomics:
 * fixed-order reductions in float64, run-to-run bit-identical. */
#define SPX_REG_ENT 1
#define SPX_REG_CEG 2
#define SPX_REG_SMAX 4
#define SPX_REG_L1 8
typedef struct spx_reg {
    const float* wd;                 /* [U, P] dense group matrix (spx_group_dense) */
    int32_t U, P;
    const int32_t *row_block, *row_local, *col_block, *col_local;   /* the GroupTables of spx_group_dense */
    const int32_t* flat_col;         /* prototype column of every weight element in block order (spx_group_dense_bwd) */
    const int32_t* block_info;       /* [nblocks][4]: off_j (first flat element), n_j, u0_j (first unit row), 0 */
    const int32_t* spans;            /* [nblocks][S][2]: local columns [c0, c1) of scale s; c0 == c1: no prototype there */
    int32_t nblocks, G, S, nspans;   /* nspans: non-empty spans (ScaleMax's mean count) */
    const float* head;               /* [K, Uh] last_layer(_group).weight */
    const float* ident;              /* [Uh, K] prototype / group class identity, fp32 */
    int32_t K, Uh;
    float epsilon;
    float weights[4];
    int32_t terms;
} spx_reg;
/* Forward, one launch: terms fp32 [4] and total fp32 [1].  workspace: spx_reg_workspace_bytes, ZERO-FILLED before its first
 * use; every call leaves it zeroed again (its first word is the last-workgroup ticket).  One call at a time per workspace. */
size_t spx_reg_workspace_bytes(const spx_reg* r);
int spx_reg_fwd(const spx_reg* r, float* total, float* terms, void* workspace, void* stream);
/* Backward, one launch: upstream of term b = g_total[0] * weights[b] + g_terms[b] (either pointer may be NULL = 0), read
 * on the device.  d_wd [U, P] (every element written; 0 outside the blocks) when group terms are on, d_head [K, Uh] when
 * L1 is on.  Gradients as torch's autograd of the reference forms (clamp passes where w >= eps, sgn(0) = 0). */
int spx_reg_bwd(const spx_reg* r, const float* g_total, const float* g_terms, float* d_wd, float* d_head, void* stream);

/* Activation losses of the labelled pixels over class-gathered planes (additive to ABI 17; segmentation/model/loss.py:149-348).
 * vals fp32 [B, J, HW] slot planes (spx_dist_fwd_cls, or gathered activations), labels int32 [B, HW] (class 0..K-1, anything
 * else = no class), slot_scale int32 [K, J]: scale id of (class, slot), -1 = the class has no such slot, -2 = a slot that lies
 * in no scale.  A segment is (image, class) with n pixels and Jc slots; a = activation of a pixel for a slot (mode 0: vals;
 * mode 1: log((vals + 1) / (vals + epsilon)); mode 2: -vals; applied at load, the gradient is with respect to vals).
 *   term 0 spatial entropy  mean over segments with n >= 2 of mean_j H_j / ln n, H_j = entropy of the softmax of a_j over the
 *                           segment's pixels (ln n is a constant of the gradient)                              (:149-211)
 *   term 1 sample entropy   mean over items (segment, scale) with n >= 1 and ns >= 2 slots of that scale of the pixel mean of
 *                           the entropy of the softmax over the ns slots / ln ns; an item with ns < 2 is skipped  (:214-284)
 *   term 2 norm             mean over segments with n >= 1 of mean_j (sum_px |a| / n) (norm_type 0, l1) or mean_j max_px |a|
 *                           (norm_type 1, linf; the gradient is shared evenly by the pixels at the maximum)      (:287-348)
 * A term without a segment / item is 0 with zero gradient.  Bit b of `terms` enables term b; a disabled term is 0, takes no
 * part in the total and gets no gradient.  Call order: zero-fill `workspace` (spx_actloss_workspace_bytes), segment_max,
 * segment_sums, finish; then backward any number of times.  Integer atomics and fixed-order sums only: run-to-run bit-identical.
 * Limits: those of the spx_kld_* reduction passes (J <= 16, K*J*12 + K*4 + 8 <= 60 KiB), HW < 2^29. */
#define SPX_ACT_SPAT 1
#define SPX_ACT_SAMPL 2
#define SPX_ACT_NORM 4
typedef struct spx_actloss {
    const float* vals;
    const int32_t* labels;
    const int32_t* slot_scale;
    int32_t B, J, HW, W, K;          /* W: row length of the pixel grid (a traversal hint), 0 or a divisor of HW */
    int32_t mode, terms, norm_type;
    float epsilon;
    float weights[3];
} spx_actloss;
size_t spx_actloss_workspace_bytes(const spx_actloss* a);
int spx_actloss_segment_max(const spx_actloss* a, void* workspace, void* stream);
int spx_actloss_segment_sums(const spx_actloss* a, void* workspace, void* stream);
/* out fp32 [7]: the three terms, 1 / max(1, number of segments or items) of each, total = sum of weights[b] * term b.
 * coef fp32 [B*K, 6, J]: what the backward reads per (segment, slot). */
int spx_actloss_finish(const spx_actloss* a, void* workspace, float* coef, float* out, void* stream);
/* grad fp32 [B, J, HW] = d/dvals, every element written.  Upstream of term b = g_total[0] * weights[b] + g_terms[b] (either
 * pointer may be NULL = 0), read on the device. */
int spx_actloss_backward(const spx_actloss* a, const float* coef, const float* g_total, const float* g_terms, float* grad,
                         void* stream);

/* Activation-overlap metrics (additive to ABI 17; segmentation/analysis/prototype_overlap.py:28-92, group_overlap.py:28-87):
 * how much the high-activation regions of one class's prototypes (or groups) overlap.
 *   planes     fp32 [N, C, h, w] activation planes, addressed through host_strides = element strides of (n, c, y, x)
 *   u[n,c,Y,X] the plane upsampled to H x W as OpenCV INTER_CUBIC / F.interpolate(mode="bicubic", align_corners=False) define
 *              it: source coordinate (X + 0.5) * w / W - 0.5, four taps per axis, Keys' kernel with a = -0.75, tap indices
 *              clamped to the grid; computed in fp32 and never written to memory
 *   T[n,c]     np.quantile(u[n,c], q), linear method: the caller passes k = floor(q * (H*W - 1)) and gamma = the fractional part
 *              (float64 on the host, gamma rounded to fp32); with v = the sorted values, d = v[k+1] - v[k]:
 *              T = gamma >= 0.5 ? v[k+1] - d * (1 - gamma) : v[k] + d * gamma in fp32 (numpy's _lerp)
 *   mask       u > T (strict: a constant plane has an empty mask)
 * spx_overlap_thresholds writes T fp32 [N, C], found by an exact radix select (integer histograms: run-to-run identical).
 * spx_overlap_accumulate ADDS, for image n and every class k with a pixel labels[n] == k + 1 (labels as spx_eval_accumulate
 * takes them), over the slots j of slot_table int32 [K, J] (channel of (class, slot); outside [0, C) = no such slot):
 *   area[k, j] += |mask_j|;   inter[k, j, j'] += |mask_j & mask_j'| for j < j';   images[k] += 1
 * (int64 [K, J], [K, J, J], [K]; the union of a pair is area_j + area_j' - inter).  thresholds: what spx_overlap_thresholds
 * wrote for the same planes and size.  workspace: spx_overlap_workspace_bytes(N, C, K) bytes (independent of H and W; 0 and
 * spx_last_error for bad sizes), no initialisation needed, one call at a time per workspace.
 * Limits: J <= 32, K <= 1024, C <= 4096, N <= 65535, H*W < 2^31, H and W <= 32768, h <= 16384, w <= 1638. */
size_t spx_overlap_workspace_bytes(int32_t N, int32_t C, int32_t K);
int spx_overlap_thresholds(const float* planes, const int64_t* host_strides, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H,
                           int32_t W, int64_t k, float gamma, void* workspace, float* thresholds, void* stream);
int spx_overlap_accumulate(const float* planes, const int64_t* host_strides, const float* thresholds, const void* labels,
                           int32_t label_bytes, const int32_t* slot_table, int32_t N, int32_t C, int32_t K, int32_t J, int32_t h,
                           int32_t w, int32_t H, int32_t W, int64_t* inter, int64_t* area, int64_t* images, void* workspace,
                           void* stream);

/* Push bounding boxes (additive to ABI 17; segmentation/push_multiscale_optimization.py:416-497, helpers.py:53-87): for every
 * pushed prototype the box of its latent patch in image pixels and the rectangle of the highly activated region around it.
 *   planes, host_strides, u, labels   as spx_overlap_accumulate takes them (labels [N, H, W]: 0 = void, k + 1 = class k)
 *   rows        int32 [R, 4] on the device = (n, c, class k, flat latent index f): plane (n, c), the prototype's class, the pushed
 *               latent pixel.  host_rows: the same table in host memory, or NULL.  Given, every row is checked on the host
 *               (0 <= n < N, 0 <= c < C, k >= 0, 0 <= f < h*w) and a bad one refuses the call; with NULL the kernel writes -1 to
 *               the eight outputs of such a row and reads nothing for it.
 *   thresholds  fp32 [N, C]; only the entries the rows name are read.  The reference's threshold is np.percentile(u, 95) =
 *               spx_overlap_thresholds at q = 0.95 for the same planes and size.
 *   rf box      ph = H / h, pw = W / w, i = f / w, j = f % w, in double as Python's floats:
 *               rf = [int(i*ph), int(i*ph + ph) + 1, int(j*pw), int(j*pw + pw) + 1]; the ends may exceed H, W and are stored so
 *   hit(Y, X)   labels[n, Y, X] == k + 1 ? u[n, c, Y, X] >= T : 0 >= T   (non-strict; with T <= 0 every pixel outside the class hits)
 *   crop        from (sh, eh, sw, ew) = rf with four sticky `stopped` flags, until all are set, a pass does in this order, each step
 *               on the box as the step before left it:
 *                 0: not stopped[0], sh > 0     and a hit in row sh - 1, columns sw..ew (clipped to W - 1): sh -= 1, else stopped[0]
 *                 1: not stopped[1], eh < H - 1 and a hit in row eh + 1, the same columns:                  eh += 1, else stopped[1]
 *                 2: not stopped[2], sw > 0     and a hit in column sw - 1, rows sh..eh (clipped to H - 1): sw -= 1, else stopped[2]
 *                 3: not stopped[3], ew < W - 1 and a hit in column ew + 1, the same rows:                  ew += 1, else stopped[3]
 *               then m = add_margin: crop = (max(sh - m, 0), min(eh + m, H - 1) + 1, max(sw - m, 0), min(ew + m, W - 1) + 1)
 * Outputs int32 [R, 4] each: rf_boxes and crops, (h0, h1, w0, w1) with exclusive ends.  Integer results of a serial walk: run-to-run
 * identical.  One launch of R workgroups, no workspace.  Limits: those of spx_overlap_accumulate, R <= 2^24, 0 <= add_margin <= 32768. */
int spx_push_boxes(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                   const int32_t* host_rows, const float* thresholds, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H,
                   int32_t W, int32_t add_margin, int32_t* rf_boxes, int32_t* crops, void* stream);

/* Per-row thresholds for the push boxes (additive to ABI 17): spx_push_boxes with T = row_thresholds[r], fp32 [R], in place of
 * thresholds[n, c] - the same rows, walk and outputs.  A host row may name class -1, which masks on label 0: what the reference
 * does for a patch whose majority label is void (nearest_img.py:283, patch_class + 1 == 0).  T = +inf or NaN hits nowhere: the crop
 * is the patch box plus the margin. */
int spx_push_boxes_rows(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                        const int32_t* host_rows, const float* row_thresholds, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w,
                        int32_t H, int32_t W, int32_t add_margin, int32_t* rf_boxes, int32_t* crops, void* stream);

/* Class-restricted thresholds (additive to ABI 17; segmentation/analysis/nearest_img.py:292-300, push_multiscale_optimization.py:
 * 476-484, the reference's threshold_gt): T[r] = np.percentile(u[n, c][labels[n] == L], 100 q) with u as spx_overlap_thresholds
 * defines it.
 *   rows      int32 [R, 3] on the device = (n, c, label value L).  host_rows: the same table in host memory, or NULL.  Given,
 *             every row is checked on the host (0 <= n < N, 0 <= c < C, L >= 0) and a bad one refuses the call; with NULL such a
 *             row gets NaN and nothing is read for it.
 *   rank      on the device, in float64 as numpy forms it: count = |{labels[n] == L}|, virtual = q (count - 1), k = floor(virtual),
 *             gamma = (float)(virtual - k) clamped below 1, k1 = min(k + 1, count - 1);  T = numpy's _lerp(v[k], v[k1], gamma) in
 *             fp32 over the sorted fp32 values v of the class's pixels.  count == 0: T = +inf (the reference's np.inf).
 * The select is spx_overlap_thresholds' (three histogram rounds over values recomputed by the same function, integer
 * histograms: exact and run-to-run identical), so with every pixel in the class T equals spx_overlap_thresholds' bit for bit.
 * No host read, no synchronisation; every launch goes to `stream`.  workspace: spx_masked_workspace_bytes(R) bytes (0 and
 * spx_last_error for a bad R), no initialisation needed, one call at a time per workspace.  Limits: those of
 * spx_overlap_thresholds, R <= 4096, 0 < q < 1. */
size_t spx_masked_workspace_bytes(int32_t R);
int spx_masked_thresholds(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                          const int32_t* host_rows, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, double q,
                          void* workspace, float* thresholds, void* stream);

/* Majority label of a patch box (additive to ABI 17; nearest_img.py:258-264, nearest_proto.py:242-244):
 * majority[r] = np.bincount(labels[n][h0:h1, w0:w1].ravel()).argmax() for row (n, flat latent index f) of rows int32 [R, 2], with
 * (h0, h1, w0, w1) the rf box of spx_push_boxes for a latent grid h x w, clipped to the image as a NumPy slice clips it; the smallest
 * label on a tie.  Labels [N, H, W] hold 0 .. num_labels - 1 (num_labels <= 1024: the histogram lives in LDS); a value outside is
 * not counted.  host_rows as above (0 <= n < N, 0 <= f < h*w), or NULL: such a row gets -1.  majority int32 [R]. */
int spx_patch_majority(const void* labels, int32_t label_bytes, const int32_t* rows, const int32_t* host_rows, int32_t R, int32_t N,
                       int32_t h, int32_t w, int32_t H, int32_t W, int32_t num_labels, int32_t* majority, void* stream);

/* Nearest prototypes of chosen pixels (additive to ABI 17; segmentation/analysis/nearest_proto.py:54-66).  distances fp32
 * [B, P, h, w] contiguous; queries int32 [Q, 3] on the device = (n, y, x), host_queries the same in host memory (every query
 * checked, a bad one refuses the call) or NULL (a bad query gets no entry).  Per query the k <= 64 smallest distances[n, :, y, x]
 * in ascending (distance, prototype) order under the total order of the fp32 bits (-0 below +0, NaN last): index int64 [Q, k],
 * value fp32 [Q, k], missing entries -1 / +inf.  include: uint8 [P] or NULL; a prototype with a zero byte is no candidate.
 * window = 0: the k nearest candidates.  window > 0, the reference's rule: the `window` nearest of ALL prototypes, of which the
 * included ones are kept, k at the most.  One wave per query, no atomics: run-to-run identical. */
int spx_nearest_protos(const float* distances, const int32_t* queries, const int32_t* host_queries, const uint8_t* include, int32_t Q,
                       int32_t B, int32_t P, int32_t h, int32_t w, int32_t k, int32_t window, int64_t* index, float* value, void* stream);

/* Single-pass push (additive to ABI 17; segmentation/push_multiscale_optimization.py:135-137, :162-188): merge the per-image
 * minima of B consecutive images (global indices image0 .. image0 + B - 1, later than every image already merged - the
 * precondition of spx_prune_merge) into the running winner of every prototype, and gather the winner's feature vector while the
 * batch's features are still on the device.
 *   indices int64 [B, P], values fp32 [B, P]   what spx_dist_push_min / spx_push_argmin wrote for the batch
 *   x            [B, C, HW] contiguous NCHW features of the batch; x_dtype 0 = bf16, 1 = fp32 (as spx_dist_push_min)
 *   proto_scale  int32 [P]: channel block of every prototype (the reference's p / (P / S)); block s is channels s*Cs .. s*Cs + Cs - 1
 * State, owned by the caller and updated in place: best_value fp32 [P] (initialise to +inf), best_image int64 [P] (-1),
 * best_flat int64 [P] (0), best_patch fp32 [P, Cs] (0).
 * Rule, per prototype p: (v, b) = the lexicographic minimum of (values[b, p], b) over b under fp32 `<` (the lowest image of the
 * batch on ties; a NaN is never below anything and never wins).  If v < best_value[p], strictly:
 *   best_value[p] = v;  best_image[p] = image0 + b;  best_flat[p] = f = indices[b, p];
 *   best_patch[p, c] = (float) x[b, proto_scale[p] * Cs + c, f] for c < Cs   (bf16 -> fp32 widens exactly)
 * otherwise nothing of row p is written, not even the same bits.  Because batches arrive in image order and an equal value
 * does not replace, the state after all batches is values.argmin(dim=0) over all images with the lowest image on ties (:135-137)
 * and the patches the reference gathers from it (:162-188); a prototype whose class never appears ends at image 0, flat 0, value
 * max_dist.  Preconditions: 0 <= indices < HW (true of the two producers) and (proto_scale[p] + 1) * Cs <= C; a row that breaks
 * one is left unchanged and nothing is read for it.  One wave per prototype: no atomics, run-to-run identical.  One launch, no
 * workspace, nothing allocated. */
int spx_push_merge(const int64_t* indices, const float* values, const void* x, int32_t x_dtype, int32_t B, int32_t P, int32_t C,
                   int32_t HW, int32_t Cs, const int32_t* proto_scale, int64_t image0, float* best_value, int64_t* best_image,
                   int64_t* best_flat, float* best_patch, void* stream);

/* Explanation maps (additive to ABI 17; segmentation/analysis/sample_activations_prototype.py:71-133,
 * sample_activations_group.py:72-131): the normalised heat map of an activation plane over one class of an image, and the map of
 * the slot that dominates each pixel of the class, as one byte per pixel.
 *   planes, host_strides, u, labels   as spx_overlap_accumulate takes them (labels [N, H, W]: 0 = void, k + 1 = class k)
 *   heat rows   int32 [R, 3] on the device = (n, c, class k): plane (n, c) over class k.  host_rows: the same table in host
 *               memory, required: every row is checked on the host (0 <= n < N, 0 <= c < C, k >= 0) and a bad one refuses
 *               the call before any launch.
 *   m           labels[n] == k + 1 ? u[n, c] : 0;   lo = min m, hi = max m over the H*W pixels;   d = hi - lo (fp32)
 *   heat        (uint8) trunc(255 * ((m - lo) / d)), every operation in fp32 and rounded on its own, the division correctly
 *               rounded: NumPy's np.uint8(255 * ((m - amin) / amax(m - amin))) on float32.  Where d == 0 (a constant plane, a
 *               class absent from the image) the row is all zeros; NumPy divides 0 by 0 there and its bytes are undefined.
 * spx_explain_range writes the order-preserving uint32 keys of lo and hi into workspace (8 R bytes, no initialisation needed,
 * one call at a time per workspace): integer min / max atomics, run-to-run identical.  spx_explain_heat, given the same
 * arguments and that workspace, writes heat uint8 [R, H, W] and ranges fp32 [R, 2] = (lo, hi).
 *   dominant rows  int32 [R, 2] on the device = (n, class k), host_rows as above (0 <= n < N, 0 <= k < K)
 *   dom            labels[n] == k + 1 ? argmax over j of weights[k, j] * u[n, slot_table[k, j]] : 255, the product in fp32, over
 *                  the slots with a channel in [0, C); the first maximum on ties and a NaN counts as a maximum (np.argmax);
 *                  the value is the column j of slot_table int32 [K, J]; a class without a slot gives 255 everywhere.
 *                  weights fp32 [K, J] on the device, or NULL = 1.
 * spx_explain_dominant writes dom uint8 [R, H, W].  heat and dom may have any alignment; every byte is written exactly once.
 * Each call enqueues on `stream` only.  Limits: those of spx_overlap_accumulate, R <= 65535. */
int spx_explain_range(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                      const int32_t* host_rows, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                      void* workspace, void* stream);
int spx_explain_heat(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                     const int32_t* host_rows, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                     const void* workspace, uint8_t* heat, float* ranges, void* stream);
int spx_explain_dominant(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                         const int32_t* host_rows, const int32_t* slot_table, const float* weights, int32_t R, int32_t N, int32_t C,
                         int32_t K, int32_t J, int32_t h, int32_t w, int32_t H, int32_t W, uint8_t* dom, void* stream);

/* Failure cases (additive to ABI 17; segmentation/analysis/failure_cases.py, segmentation/eval_test.py:99-111): predicted label
 * maps as bytes with a confusion matrix per image, the table of failing (image, class) pairs, and the heat maps of two classes'
 * slots over the failing class.
 *
 * spx_predict_accumulate: logits fp32 [N, h, w, K] through host_logit_strides = (n, channel, y, x) as spx_eval_accumulate takes
 * them, 1 <= K <= 256.  k* = the first argmax over the classes of the bilinear (align_corners = False) upsample to H x W, with the
 * bits of spx_upsample_argext.  At least one of:
 *   pred  uint8 [N, H, W], any alignment: id_map[k*] (id_map uint8 [K] on the device), or k* when id_map is NULL; every byte is
 *         written exactly once, as packed dwords wherever four bytes of a row share an aligned dword.
 *   conf  int64 [N, K+1, K], ADDED to: conf[n, r, k*] += 1 per pixel with label != 0, r = label - 1 for 1 <= label <= K, else K
 *         (spx_eval_accumulate's rule, per image).  Needs labels [N, H, W] (label_bytes 1 / 4 / 8); labels may be NULL without it.
 * One launch; counters privatised per workgroup in LDS and flushed with 64-bit atomics whenever a workgroup's image changes.
 *
 * spx_failure_table: one launch over conf int64 [N, K+1, K], no host read.  For image n and class k:
 *   present = sum_j conf[n, k, j] > 0;  I = conf[n, k, k];  U = sum_j conf[n, k, j] + sum_{r = 0..K} conf[n, r, k] - I
 *   iou  f64 [N, K]    I / U, the division correctly rounded; NaN for a class that is not present
 *   fail uint8 [N, K]  iou < threshold (strict, float64); 0 for a class that is not present
 *   miss int32 [N, K]  argmax over j != k of conf[n, k, j]: the lowest j among equal counts, -1 when all are zero or the class is
 *                      not present
 *
 * spx_paired_range / spx_paired_heat: planes, host_strides, labels, u as spx_explain_range takes them.  rows int32 [R, 4] on the
 * device = (n, c, class a, range slot q), host_rows the same table in host memory, required and checked before any launch: every
 * field in range (0 <= q < Q), every slot 0 .. Q-1 named, rows of one slot name one (n, a).
 *   m      labels[n] == a + 1 ? u[n, c] : 0;   lo_q = min m, hi_q = max m over all pixels of all rows naming slot q
 *   heat   (uint8) trunc(255 * ((m - lo_q) / hi_q)) in fp32, every operation rounded on its own, the division correctly rounded
 *          (np.uint8(255 * ((m - min) / max)) on float32); 255 where 255 x >= 256 (possible only when lo_q < 0); a slot with
 *          hi_q <= 0 gives all-zero rows.
 * spx_paired_range writes the keys of lo and hi into workspace (8 Q bytes, no initialisation needed); spx_paired_heat, given the
 * same arguments and that workspace, writes heat uint8 [R, H, W] (any alignment, every byte once) and ranges fp32 [Q, 2].
 * Integer min / max atomics: run-to-run identical.  Limits: those of spx_explain_range; Q <= R <= 65535. */
int spx_predict_accumulate(const float* logits, const int64_t* host_logit_strides, const void* labels, int32_t label_bytes,
                           const uint8_t* id_map, int32_t N, int32_t K, int32_t h, int32_t w, int32_t H, int32_t W, uint8_t* pred,
                           int64_t* conf, void* stream);
int spx_failure_table(const int64_t* conf, int32_t N, int32_t K, double threshold, double* iou, int32_t* miss, uint8_t* fail_out,
                      void* stream);
int spx_paired_range(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                     const int32_t* host_rows, int32_t R, int32_t Q, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                     void* workspace, void* stream);
int spx_paired_heat(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                    const int32_t* host_rows, int32_t R, int32_t Q, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                    const void* workspace, uint8_t* heat, float* ranges, void* stream);

/* Cross-scale feature aggregation (additive to ABI 17; the reference's WeightedAgg, segmentation/model/scale_head.py, called at
 * model_multiscale.py:306-314): the features of one scale are combined with the activations of the scale above it,
 *     a = similarity(source)   source fp32 [B, Pn, HW]: source_kind 0 = ready activations, 1 = distances under 'log'
 *                              (log((d + 1) / (d + epsilon)), the bits the distance kernels emit), 2 = distances under 'linear' (-d)
 *     s[b][c][px] = sum_p proto[p][c] * a[b][p][px]          proto fp32 [Pn, Cs], Cs a multiple of 16, Pn >= 1
 *     out = s (mode 0)  |  (x + s) / 2 (mode 1)  |  sqrt(x * s) (mode 2)          out fp32 [B, Cs, HW]
 * x: [B, Cs, HW] planes of x_dtype (0 bf16, 1 fp32) with channel stride HW and batch stride x_bstride elements (a channel slice
 * of [B, S * Cs, H, W] is passed in place); ignored (NULL accepted) in mode 0.  The product runs on v_mfma_f32_32x32x2_f32:
 * fp32 operands and accumulation.  One launch, no workspace.
 *
 * spx_scale_agg_bwd: g = dL/dout fp32 [B, Cs, HW].  s is recomputed, never saved.  Outputs, each optional (NULL = not wanted):
 *   dx       [B, Cs, HW] contiguous, x's dtype (bf16: round to nearest even); not written in mode 0
 *   dsource  fp32 [B, Pn, HW]; for a distance source it carries the similarity's derivative
 *            (-(1 - epsilon) / ((d + 1)(d + epsilon)) resp. -1)
 *   dproto   fp32 [Pn, Cs]: per-workgroup partials over slabs of 256 pixels, summed in slab order by a second kernel
 * mode 2 follows dx = g s / (2 out), ds = g x / (2 out) in IEEE arithmetic (x s <= 0 gives what that gives).
 * workspace: spx_scale_agg_workspace_bytes(B, Cs, Pn, HW) bytes, no initialisation needed.  No float atomics: run-to-run identical. */
#define SPX_SAGG_NONE 0
#define SPX_SAGG_SUM 1
#define SPX_SAGG_MULT 2
#define SPX_SAGG_ACTIVATIONS 0
#define SPX_SAGG_DIST_LOG 1
#define SPX_SAGG_DIST_LINEAR 2
size_t spx_scale_agg_workspace_bytes(int32_t B, int32_t Cs, int32_t Pn, int32_t HW);
int spx_scale_agg_fwd(const void* x, int32_t x_dtype, int64_t x_bstride, const float* source, int32_t source_kind, const float* proto,
                      float* out, int32_t B, int32_t Cs, int32_t Pn, int32_t HW, int32_t mode, float epsilon, void* stream);
int spx_scale_agg_bwd(const void* x, int32_t x_dtype, int64_t x_bstride, const float* source, int32_t source_kind, const float* proto,
                      const float* g, void* dx, float* dsource, float* dproto, void* workspace, int32_t B, int32_t Cs, int32_t Pn,
                      int32_t HW, int32_t mode, float epsilon, void* stream);

/* Part consistency and stability (additive to ABI 17; segmentation/analysis/metrics/consistency.py:186-270 and :165-178,
 * stability.py:169-175): which prototypes or groups of a class fire at the centroids of the annotated object parts.
 *   labels [N, H, W] (label_bytes 1 / 4 / 8): 0 = void, k + 1 = class k < K, anything else no class
 *   parts  [N, H, W] (part_bytes 1 / 4 / 8): t in 1..M = part t, anything else no part (the reference raises above M)
 *   B_t = (labels == k + 1) & (parts == t); a pixel's key (k, t) is k * M + t - 1.
 *
 * spx_part_components: the 8-connected components of every B_t of every image in one labelling over the joint key (neighbours
 * are joined when their keys are equal): union-find, 32 x 32 tiles labelled in LDS, a border-merge launch, a flatten launch.
 * Every parent is at most its own pixel index and only atomicMin lowers it, so every find / union loop ends; no workgroup waits
 * for another, kernel boundaries order the launches, and every cross-workgroup access to a parent is an agent-scope atomic.
 *   workspace  spx_part_components_workspace_bytes(N, H, W) bytes (0 and spx_last_error for bad sizes), no initialisation needed,
 *              and the result: [sumx uint64 N*H*W | sumy uint64 N*H*W | parent uint32 N*H*W | count uint32 N*H*W].
 *              parent[n][i] = the smallest pixel index Y * W + X of the pixel's component (0xffffffff: no key); at that root
 *              count / sumx / sumy = the component's pixels and the integer sums of their X and Y; 0 at every other pixel.
 *   totals     uint64 [N, K, M, 3] = (count, sum X, sum Y) of B_t: the complement's centroid follows by subtraction.
 * Integer atomics only: two runs agree bit for bit.
 *
 * spx_part_thresholds: T[n, k, j] fp32 [N, K, J] for the slots of slot_table int32 [K, J] (channel or -1) of
 *   u[Y, X] = labels[n, Y, X] == k + 1 ? a[n, c, sy(Y), sx(X)] : +0,   sx(X) = min(floor(X * (1.0 / (W / w))), w - 1) in float64
 *   (the source index of OpenCV's INTER_NEAREST, sy alike with H / h; planes / host_strides as spx_overlap_thresholds takes them)
 *   mode SPX_PART_IMAGE    np.quantile(u, q) over all H * W values
 *   mode SPX_PART_NONZERO  np.quantile(u[u != 0], q); +inf when there is none
 * with the rank formed on the device in float64 as spx_masked_thresholds forms it and numpy's fp32 _lerp.  One pass over the labels
 * counts the pixels of every class per latent cell; one workgroup per (n, k, j) then selects over the h * w cell values with those
 * multiplicities (and the zero, H * W - n_k times, in image mode).  The [H, W] plane is never formed.  A slot without a channel in
 * [0, C) and a class with skip[k] != 0 (skip uint8 [K] or NULL) get NaN.  workspace: spx_part_thresholds_workspace_bytes(N, K, h, w)
 * bytes, no initialisation needed.
 *
 * spx_part_presence: given the labelling (comp_workspace, totals) and thresholds fp32 [N, K, J] of the same labels,
 *   valid uint8 [N, K]           1 when class k is not skipped and some B_t of image n is not empty
 *   table uint8 [N, K, J, M + 1] 255 (absent) in a row that is not valid, for a slot without a channel, in column 0 and for an empty
 *                                B_t; else 1 when u[cy, cx] > T (strict) at the centroid of any component of B_t or of the
 *                                complement of B_t within the image (the label-0 row of cv2.connectedComponentsWithStats, which
 *                                consistency.py:264 walks too; none when B_t is the whole image), else 0.
 *   centroid = (rint(sum X / count), rint(sum Y / count)), the quotients in float64: np.round, half to even.
 * Every byte is written by an initialising launch; later launches store only the byte 1.
 *
 * spx_part_fold_consistency: counters int64 [ones K*J*(M+1) | times present K*J*(M+1) | rows K*J], ADDED to, over the valid rows
 * of the batch and the slots with a channel.  spx_part_fold_stability: counters int64 [stable rows, valid rows], ADDED to: a valid
 * row is stable when all M + 1 entries of the two tables agree with absent read as 0 (stability.py:242).
 * No host read, no synchronisation; every launch goes to `stream`.  Limits: N <= 65535, K <= 1024, J <= 32, 1 <= M <= 254, the
 * map limits of spx_overlap_accumulate. */
#define SPX_PART_IMAGE 0
#define SPX_PART_NONZERO 1
size_t spx_part_components_workspace_bytes(int32_t N, int32_t H, int32_t W);
int spx_part_components(const void* labels, int32_t label_bytes, const void* parts, int32_t part_bytes, int32_t N, int32_t K, int32_t M,
                        int32_t H, int32_t W, void* workspace, uint64_t* totals, void* stream);
size_t spx_part_thresholds_workspace_bytes(int32_t N, int32_t K, int32_t h, int32_t w);
int spx_part_thresholds(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* slot_table,
                        const uint8_t* skip, int32_t N, int32_t C, int32_t K, int32_t J, int32_t h, int32_t w, int32_t H, int32_t W,
                        double q, int32_t mode, void* workspace, float* thresholds, void* stream);
int spx_part_presence(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const void* parts,
                      int32_t part_bytes, const int32_t* slot_table, const uint8_t* skip, const float* thresholds,
                      const void* comp_workspace, const uint64_t* totals, int32_t N, int32_t C, int32_t K, int32_t J, int32_t M, int32_t h,
                      int32_t w, int32_t H, int32_t W, uint8_t* table, uint8_t* valid, void* stream);
int spx_part_fold_consistency(const uint8_t* table, const uint8_t* valid, const int32_t* slot_table, int32_t N, int32_t C, int32_t K,
                              int32_t J, int32_t M, int64_t* counters, void* stream);
int spx_part_fold_stability(const uint8_t* clean, const uint8_t* noisy, const uint8_t* valid, const int32_t* slot_table, int32_t N, int32_t C,
                            int32_t K, int32_t J, int32_t M, int64_t* counters, void* stream);

/* Training-batch preparation (additive to ABI 17; segmentation/data/dataset.py:143-186, resize_label of dataset.py:22-30 and its
 * per-step use in module_multiscale.py:234-236): from raw uint8 HWC images and integer labels already on the device, ONE launch
 * writes the scaled, padded, cropped, flipped and normalised window batch, the window labels and the latent labels of up to
 * SPX_BATCH_MAX_GRIDS grids.  No workspace, no atomics, no host read; every thread writes its own elements, so two runs agree bit
 * for bit.
 *
 * One spx_batch_sample per sample, in DEVICE memory.  The scaled image is never formed: window pixel (y, x) of a sample is
 *   x' = flip ? Wc - 1 - x : x,   (sy, sx) = (y0 + y, x0 + x')        the position in the scaled, padded image
 * pad region (sy >= hs or sx >= ws, or a negative position):
 *   image  0 when normalising (the reference pads with `mean` and normalises afterwards), mean[c] otherwise,
 *          rint(mean[c] * 255) saturated to 0..255 for uint8 output;   label 0
 * inside, image: bilinear at the sample position of OpenCV's INTER_LINEAR, every operation in fp32 in this order (the library is
 * built with -ffp-contract=off; tests/batch_restatement.py restates it in NumPy float32 and matches bit for bit):
 *   rx = float(w) / float(ws);  fx = (sx + 0.5f) * rx - 0.5f, raised to 0 when negative;  x0 = floor(fx);  a = fx - x0;
 *   x1 = min(x0 + 1, w - 1);  x0 >= w - 1: x0 = x1 = w - 1, a = 0;      the same in y with b
 *   v = (p00 * (1 - a) + p01 * a) * (1 - b) + (p10 * (1 - a) + p11 * a) * b         p = the source bytes as fp32
 *   r = round_u8 ? rintf(v) : v
 *   fp32 output  normalize ? (r / 255.0f - mean[c]) / std[c] : r / 255.0f;      uint8 output (needs round_u8): the byte r
 * OpenCV's own INTER_LINEAR works in 11-bit fixed point: it was never run against this rule.
 * inside, label: src[index[row_tab + sy]][index[col_tab + sx]] - the caller's tables of PIL's NEAREST rule, h -> hs and w -> ws -
 * then id_map[raw] when an id table is given (a raw value outside 0..L-1 becomes 0; dataset.py:134 `convert_targets`).
 * latent labels of grid g: the window label at (index[grid_rt[g] + y], index[grid_ct[g] + x]), the tables Hc -> grid_h[g] and
 * Wc -> grid_w[g] shared by all samples: resize_label of the window, as composing index tables equals resampling twice.
 * latent[g] int64 [B, grid_h, grid_w] in the reference's convention (0 = void); latent0[g] int32, the same minus one under the
 * rule of spx_shift_labels (a value whose v - 1 leaves int32 is -1).  Either may be NULL.
 * A table entry is clamped into the source and a sample whose tables do not lie inside `index` (n_index entries) is written as
 * pad, so no descriptor can make the kernel read outside `index`; the image and label pointers are the caller's promise.
 *
 * spx_resize_labels: the latent-label half alone for labels [B, Hc, Wc] already on the device (labels_in, labels_dtype): reads
 * `index`, `id_map`, the grids and latent / latent0; `samples`, `image_out` and `window_labels` are not read.
 * Limits: 1 <= B <= 65535, Hc * Wc < 2^31 - 256 and the same for every grid, G <= 4 (at least one output in all), L >= 0. */
#define SPX_BATCH_MAX_GRIDS 4
#define SPX_LABEL_U8 1      /* label dtype codes: the element's size in bytes */
#define SPX_LABEL_I16 2
#define SPX_LABEL_I32 4
#define SPX_LABEL_I64 8
typedef struct spx_batch_sample {
    const void* image;          /* uint8, channel stride 1: pixel (Y, X) at image + Y * image_row_stride + X * image_pixel_stride */
    const void* label;          /* [h, w], element stride 1 within a row */
    int64_t image_row_stride;   /* bytes */
    int64_t label_row_stride;   /* elements */
    int32_t image_pixel_stride; /* bytes (3 for packed HWC) */
    int32_t label_dtype;        /* SPX_LABEL_* */
    int32_t h, w;               /* source size */
    int32_t hs, ws;             /* scaled size, both >= 1 */
    int32_t y0, x0;             /* crop origin in the scaled, padded image */
    int32_t flip;
    int32_t row_tab, col_tab;   /* offsets into `index`: hs entries in 0..h-1, ws entries in 0..w-1 */
    int32_t reserved;
} spx_batch_sample;             /* 80 bytes */
typedef struct spx_batch {
    const spx_batch_sample* samples;    /* DEVICE [B] */
    const int32_t* index;               /* DEVICE [n_index] */
    const int32_t* id_map;              /* DEVICE [L] or NULL */
    const void* labels_in;              /* spx_resize_labels only: [B, Hc, Wc] */
    void* image_out;                    /* [B, 3, Hc, Wc] fp32 or uint8, or NULL */
    int64_t* window_labels;             /* [B, Hc, Wc] or NULL */
    int64_t* latent[SPX_BATCH_MAX_GRIDS];
    int32_t* latent0[SPX_BATCH_MAX_GRIDS];
    int32_t n_index, L, labels_dtype, B, Hc, Wc, G;
    int32_t grid_h[SPX_BATCH_MAX_GRIDS], grid_w[SPX_BATCH_MAX_GRIDS];
    int32_t grid_rt[SPX_BATCH_MAX_GRIDS], grid_ct[SPX_BATCH_MAX_GRIDS];     /* offsets into `index` */
    int32_t normalize, round_u8, out_u8;
    float mean[3], std[3];
} spx_batch;
int spx_batch_prepare(const spx_batch* args, void* stream);
int spx_resize_labels(const spx_batch* args, void* stream);

/* ---- multi-scale input fusion: the pixel-wise maximum of MSC (segmentation/utils.py:71-111) in one launch --------------------
 * K maps [B, C, h_k, w_k] (1 <= K <= 8), all bf16 (dtype code 0) or all fp32 (1); maps[0] fixes the output grid (H, W) = (h_0,
 * w_0).  Element (b, c, i, j) of map k is at data + b * batch_stride + c * channel_stride + i * w_k + j (strides in elements: a
 * channel slice is read in place; the h_k x w_k plane is contiguous).  out is contiguous [B, C, H, W] in out_dtype.
 *   u_0 = maps[0];   u_k[Y][X], k >= 1: bilinear with align_corners = False, every operation in fp32 in this order
 *     r = float(h_k) / float(H);  s = r * (Y + 0.5f) - 0.5f, raised to 0 when negative;  i0 = min(floor(s), h_k - 1);
 *     i1 = min(i0 + 1, h_k - 1);  ly = s - i0;   the same along the columns with lx
 *     u = (1 - ly) * ((1 - lx) * v00 + lx * v01) + ly * ((1 - lx) * v10 + lx * v11)        (no contraction into fma)
 *   z = max_k u_k, the lowest k among equal values; a NaN candidate wins and keeps the first NaN's k (torch.max(dim=0));
 *   activation 0: y = z;  1: y = 1 / (1 + expf(-z));   a bf16 y is the fp32 y rounded to nearest even.
 * spx_msc_max_fwd writes out and, when index is not NULL, the winning k per element (uint8 [B, C, H, W]).
 * spx_msc_max_bwd reads g = dL/dout (g_dtype, contiguous [B, C, H, W]), index (may be NULL when K = 1) and, under activation 1,
 * out (the derivative is y (1 - y) of the SAVED y in out_dtype); of the maps it reads the sizes h, w only; it writes grads[k] (contiguous [B, C, h_k, w_k] in the maps'
 * dtype) for every k whose pointer is not NULL: one thread per source element gathers g * wy * wx over the destination pixels
 * whose footprint holds it and whose index is k, in ascending (Y, X) order.  No atomics, no workspace: run-to-run identical.
 * Both are one launch on `stream` and read nothing on the host.  Limits: 1 <= B <= 65535, C >= 1, H * W < 2^31 and h_k * w_k <
 * 2^31, B * C * H * W < 2^40, fewer than 2^39 gradient elements in one backward; out, g and the grads are aligned to their
 * element size. */
#define SPX_MSC_MAX_MAPS 8
typedef struct spx_msc_map {
    const void* data;
    int64_t batch_stride, channel_stride;   /* elements */
    int32_t h, w;
} spx_msc_map;
typedef struct spx_msc {
    spx_msc_map maps[SPX_MSC_MAX_MAPS];
    void* grads[SPX_MSC_MAX_MAPS];          /* backward only */
    void* out;
    uint8_t* index;
    const void* g;                          /* backward only */
    int32_t K, B, C;
    int32_t in_dtype, out_dtype, g_dtype;   /* 0 = bf16, 1 = fp32 */
    int32_t activation;                     /* 0 = none, 1 = sigmoid */
    int32_t reserved;
} spx_msc;
int spx_msc_max_fwd(const spx_msc* args, void* stream);
int spx_msc_max_bwd(const spx_msc* args, void* stream);

/* ---- the packed training maps: MSC's training list [full] + pyramid + [max] on ONE pixel axis, one launch ---------------------
 * The same K maps (spx_msc, same stride rules, same dtype codes).  out is ONE contiguous buffer [C, M] in out_dtype with
 * nseg = K + (with_max ? 1 : 0) segments side by side and no padding: pixel (b, i) of segment q (i = row * w_q + column) is
 * column off_q + b * h_q * w_q + i of every channel row, off_q = sum_{j < q} B * h_j * w_j, M = off_nseg.
 *   segment q < K   act(maps[q]) at the map's own grid (h_q, w_q);
 *   segment K       (with_max != 0) act(max_k u_k) at (H, W) = (h_0, w_0): the candidates u_k, the tie and NaN rules, the
 *                   activation and the bf16 rounding are spx_msc_max_fwd's, above, operation for operation; index (uint8
 *                   [B, C, H, W], the usual layout, not packed) receives the winning k when it is not NULL.
 * Taken as features [1, C, 1, M] the buffer is what the distance entry points read (B = 1, HW = M): their workgroup tiles
 * straddle segment and image boundaries, which changes nothing, as every quantity of theirs is per pixel.  With with_max = 0
 * any K maps of a common B and C form a ragged batch.  Stores are 8- / 16-byte vectors when M is a multiple of 4 and out is
 * aligned to them, element stores otherwise (any M, any element-aligned out).
 * spx_msc_pack_bwd reads g = dL/dout (g_dtype, contiguous [C, M]), index (with_max; may be NULL when K = 1) and, under activation
 * 1, out; it writes grads[k] (contiguous [B, C, h_k, w_k] in the maps' dtype) for every k whose pointer is not NULL, one thread
 * per source element: first the element's own segment, g * y (1 - y) (or g), then the gather over segment K in
 * spx_msc_max_bwd's ascending (Y, X) order, all added in fp32 in that order and rounded once.  No atomics, no workspace:
 * run-to-run identical.  Both are one launch on `stream`; offsets and sizes travel in the kernel arguments, nothing is read
 * on the host.  Limits: those of spx_msc_max_fwd / _bwd per map, and M < 2^31, C * M < 2^40. */
int spx_msc_pack_fwd(const spx_msc* args, int with_max, void* stream);
int spx_msc_pack_bwd(const spx_msc* args, int with_max, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPX_HIP_H */
