// Kernel argument blocks + launcher prototypes shared by the kernel translation units and the C ABI.
#pragma once
#include "spx_common.h"
#include <type_traits>

struct SpxFwdArgs {
    spx_plan plan;
    const void* x;
    const char* packed_bank;
    const float* p2;
    const char* packed_head;
    float* dist;
    float* act;
    float* logits;
    int B, HW, vec_ok;              // vec_ok: the launcher's spx_x_stage_mode(HW); the kernels do not read it
    int tile_first, tiles_launch;   // this launch covers tiles [tile_first, tile_first + tiles_launch) of every image (always all: tile_first = 0)
    int tile_mul;                   // block -> tile permutation: tile = (block * tile_mul) mod tiles_launch (1 = identity), see spx_tile_mul
    int dist_vec;              // distances 16-B aligned and HW % 4 == 0: 16-B stores of 4 pixels of a row
    // class-gathered distances (spx_dist_fwd_cls): every pixel keeps only the distances to its own class's prototypes
    const int32_t* labels;     // [B, HW] class per pixel (anything outside 0..0xFFFD = none)
    const uint32_t* proto_key; // [npanels][32 npb] (class << 16) | slot per padded prototype row, 0xFFFFFFFF = none
    float* cls_dist;           // [B, J, HW] slot planes
    int J;
    // fused prototype push (spx_dist_push_min): instead of the slot planes, the class-masked minimum of every prototype's
    // distance row over the image, as (ordered float key << 32 | flat pixel index) integer minima
    unsigned long long* push_keys;   // [B, P], caller-initialised to all ones; NULL = off
    float push_max;                  // the reference's max_dist (1e10)
    int push_void, push_K;           // label decode of spx_push_argmin: labels are raw (void_class dropped from 0..K), see spx_hip.h
    // prune mode of the same epilogue (spx_dist_prune_min): no class mask; a pixel whose label is push_void ranks after every
    // other pixel (key: float bits of d | void << 31, see spx_prune.hip); push_max / push_K unused
    int push_prune;
    // grouping-head tail (spx_dist_fwd_group): logits = W_g . exp(units), units = the head product
    const char* packed_tail;   // W_g A-fragments (spx_pack_group_tail); NULL = no tail
    float* gact;               // [B*HW, U] exp(units) (optional)
    int K2;                    // classes of the tail (<= 32)
    // scale-parallel launch for small pixel grids (grid.y = scale group): workgroup (tile, g) walks only the panels
    // [group_first[g], group_first[g+1]) of scale g and writes its partial logits to logits + g * logits_group_stride
    int ngroups;               // 1 = off
    size_t logits_group_stride;
    int32_t group_first[SPX_MAX_PANELS + 1];
    // fused cross entropy (spx_dist_fwd_ce): statistics of the logits tile, see spx_hip.h
    const int32_t* ce_labels;  // [B, HW]; NULL = off
    float* ce_lse;             // [B*HW]
    int32_t* ce_pred;          // [B*HW] or NULL
    float* ce_partials;        // [tiles * 4 waves][2]
    float eps;
    int act_fn;
    unsigned long long* dbg;   // diagnostic builds only (SPX_DIAG_STAMPS): per-workgroup phase clocks
};
struct SpxBwdArgs {
    spx_plan plan;
    const void* x;
    const char* packed_bank;
    const char* packed_bankT;
    const float* p2;
    const char* packed_headT;
    const float* d_dist;
    const float* d_act;
    const float* d_logits;
    const int32_t* labels;      // class-gathered mode (spx_dist_bwd_cls): see SpxFwdArgs
    const uint32_t* proto_key;
    const float* d_cls_dist;    // [B, J, HW]
    int J;
    // grouping-head tail (spx_dist_bwd_group): d_logits is [B*HW, K2]; dUnits = (W_g^T . dLogits) * exp(units)
    const char* packed_tailT;   // W_g^T A-fragments; NULL = no tail
    const float* gact;          // [B*HW, U] exp(units) of the forward
    float* d_units;             // [B*HW, U] written for the parameter kernel
    const float* d_gact;        // [B*HW, U] gradient on g = exp(units) itself (may be NULL)
    int K2;
    int ngroups;                // scale-parallel launch (see SpxFwdArgs); 1 = off
    int32_t group_first[SPX_MAX_PANELS + 1];
    // fused cross entropy (spx_dist_bwd_ce): d_logits = coef * (softmax(logits) - onehot(label)) formed in the prologue
    const int32_t* ce_labels;   // [B, HW]; NULL = off (then d_logits above is used)
    const float* ce_logits;     // [B*HW, K] the forward's logits
    const float* ce_lse;        // [B*HW]
    const float* ce_coef;       // device scalar
    float* ce_dlogits_out;      // [B*HW, K] written for the parameter kernel (may be NULL)
    void* dx;
    float* dx_acc;              // fp32 [B][C][HW rounded up to 4]: partial dX of scales that span several panels (bf16 features); may be NULL
    uint16_t* g_out;
    uint16_t* a_out;            // head-gradient scratch (spx_common.h): fp32 d_W tile partials (one class block) or the activation blob
    int B, HW, vec_ok;              // vec_ok: the launcher's spx_x_stage_mode(HW); the kernels do not read it
    int tile_first, tiles_launch;   // this launch covers tiles [tile_first, tile_first + tiles_launch) of every image (always all: tile_first = 0)
    int tile_mul;                   // see SpxFwdArgs
    float eps;
    int act_fn;
    unsigned long long* dbg;
};
struct SpxBankBwdArgs {
    spx_plan plan;
    const void* x;
    const float* bank;
    const uint16_t* g_in;
    const uint16_t* a_in;       // kernel 1's head-gradient scratch
    const float* d_logits;
    float* d_bank;
    float* d_W;
    float* workspace;
    int B, HW, vec_ok, nsplit;
    int ci_first, nci_launch;   // this launch covers chunks [ci_first, ci_first + nci_launch) of every image ...
    int slab_first, nslabs;     // ... with nslabs workgroups writing slabs [slab_first, slab_first + nslabs); nsplit = all slabs
};
// Slot (16-B unit) of lane (r = pixel, h) inside the 1-KiB fragment blob of k-step s2.  Kernel 2 copies the blobs
// verbatim into LDS and reads them back with ds_read_b64_tr_b16 (pixel = k): the 32 lanes of a half-wave then
// touch 4 consecutive pixels x both lane halves x both k-steps, which this permutation spreads over all 16
// 16-B bank groups (the plain slot r + 32 h would put them 4-way on the same banks).
__host__ __device__ inline uint32_t spx_blob_slot(int r, int h, int s2) {
    return (uint32_t)(((r >> 2) * 8 + (r & 3) + 4 * h + 8 * s2) & 63);
}

// Staging mode of the X tiles (template parameter VM of the kernels): 0 = element-wise loads (images of fewer than 8 pixels),
// 1 = 16-B vector loads, 2 = vector loads with a ragged image end (H*W % 8 != 0), see SpxXStager
inline int spx_x_stage_mode(int HW) { return HW < 8 ? 0 : (HW % 8 == 0 ? 1 : 2); }
// The run-time pair (x_dtype, staging mode) as compile-time constants: f(std::bool_constant<XF32>, std::integral_constant<int, VM>)
template <typename F>
static inline void spx_dispatch_x(int x_dtype, int vm, F f) {
    auto with_vm = [&](auto xf32) {
        if (vm == 2) f(xf32, std::integral_constant<int, 2>{});
        else if (vm) f(xf32, std::integral_constant<int, 1>{});
        else f(xf32, std::integral_constant<int, 0>{});
    };
    if (x_dtype == 1) with_vm(std::true_type{});
    else with_vm(std::false_type{});
}

int spx_tile_mul(int tiles_launch, long long plane_bytes);
hipError_t spx_launch_fwd(const SpxFwdArgs& a, int x_dtype, hipStream_t s);        // a.labels != NULL: class-gathered variant
hipError_t spx_launch_bwd(const SpxBwdArgs& a, int x_dtype, hipStream_t s);
hipError_t spx_launch_bank_bwd(const SpxBankBwdArgs& a, int x_dtype, hipStream_t s);
int spx_bank_bwd_nsplit(const spx_plan& pl, int B, int HW);
size_t spx_bwd_scratch_elems(const spx_plan& pl, int B, int HW);
size_t spx_bank_bwd_ws_floats(const spx_plan& pl, int nsplit);
hipError_t spx_launch_pack_bank(const spx_plan& pl, const float* bank, void* pb, void* pbT, float* p2, hipStream_t s);
hipError_t spx_launch_pack_head(const spx_plan& pl, const float* W, void* ph, void* phT, hipStream_t s);
hipError_t spx_launch_pack_tail(const spx_plan& pl, const float* Wg, int K2, void* pt, void* ptT, hipStream_t s);
hipError_t spx_launch_pack_headT_units(const spx_plan& pl, const float* W, void* phT, hipStream_t s);
// every operand of one forward (+ backward) in one launch (spx_pack_all); the nb_* workgroup ranges are filled by the launcher
struct SpxPackAllArgs {
    spx_plan plan;
    const float* bank;
    const float* W;            // head [K, P] or NULL
    const float* Wg;           // group tail [K2, K] or NULL
    int K2, headT_units;       // headT_units: head^T with the unit index in accumulator order (grouping backward)
    void *packed_bank, *packed_bankT;
    float* p2;
    void *packed_head, *packed_headT, *packed_tail, *packed_tailT;
    int nb_bank, nb_head, nb_headT;
};
hipError_t spx_launch_pack_all(SpxPackAllArgs a, hipStream_t s);
hipError_t spx_launch_ce_finish(const float* partials, long long n, float* loss, float* aux, hipStream_t s);
hipError_t spx_launch_shift_labels(const void* in, int is64, long long n, int32_t* out, hipStream_t s);
// dense form of the per-class group projections (spx_group_dense)
#define SPX_GROUP_BLOCKS_MAX 192
struct SpxGroupDenseArgs {
    const float* ptrs[SPX_GROUP_BLOCKS_MAX];     // device pointer of every block's weight [g_j, n_j]
    int ncols[SPX_GROUP_BLOCKS_MAX];             // n_j
    const int32_t *row_block, *row_local, *col_block, *col_local;
    int U, P;
    float* out;
};
hipError_t spx_launch_group_dense(const SpxGroupDenseArgs& a, hipStream_t s);
hipError_t spx_launch_group_dense_bwd(const float* d_out, const int32_t* rows, const int32_t* cols, long long n, int P, float* d_flat,
                                      hipStream_t s);
// in-place simplex projection of the group projections' rows (spx_simplex_project): one workgroup per row
#define SPX_SIMPLEX_MAX_COLS 1024
struct SpxSimplexArgs {
    float* ptrs[SPX_GROUP_BLOCKS_MAX];           // device pointer of every block's weight [G_j, n_j]
    int cols[SPX_GROUP_BLOCKS_MAX];              // n_j
    int row0[SPX_GROUP_BLOCKS_MAX + 1];          // first row of block j in the launch's row order; row0[nblocks] = all rows
    int nblocks;
    float z;
};
hipError_t spx_launch_simplex(const SpxSimplexArgs& a, hipStream_t s);
hipError_t spx_launch_push_argmin(const float* dist, const int32_t* labels, const float* ident, int B, int P, int K,
                                  int HW, int void_class, float max_dist, int64_t* idx, float* val,
                                  uint64_t* scratch, hipStream_t s);
hipError_t spx_launch_argmin_images(const float* values, int N, int P, int64_t* best, hipStream_t s);
hipError_t spx_launch_push_merge(const int64_t* indices, const float* values, const void* x, int x_dtype, int B, int P, int C, int HW,
                                 int Cs, const int32_t* proto_scale, long long image0, float* best_value, int64_t* best_image,
                                 int64_t* best_flat, float* best_patch, hipStream_t s);
hipError_t spx_launch_upsample_argext(const float* src, int N, int C, int h, int w, int H, int W, int take_max,
                                      int64_t* idx, float* val, hipStream_t s);
hipError_t spx_launch_eval_accumulate(const float* logits, const long long* lst, const float* dist, const long long* dst,
                                      const int32_t* pcls, const void* labels, int label_bytes, int N, int K, int P, int h, int w,
                                      int H, int W, unsigned long long* conf, unsigned long long* hits, hipStream_t s);
hipError_t spx_launch_eval_topk(const float* logits, const long long* lst, const float* dist, const long long* dst,
                                const int32_t* pcls, const void* samples, int sample_bytes, int N, int S, int K, int P, int h,
                                int w, int H, int W, unsigned long long* topk, unsigned long long* seen, hipStream_t s);
hipError_t spx_launch_sum_groups(const float* parts, size_t n, int groups, float* out, hipStream_t s);
int spx_split_groups(const spx_plan& pl, int B, int HW, int32_t* group_first);
hipError_t spx_launch_group_tail(const float* parts, int groups, long long M, int U, const float* Wg, int K2, float* gact,
                                 float* logits, const int32_t* labels, float* lse, int32_t* pred, float* partials, hipStream_t s);
hipError_t spx_launch_push_finalize(const uint64_t* scratch, int n, int64_t* idx, float* val, hipStream_t s);
hipError_t spx_launch_prune_argmin(const float* dist, const int32_t* labels, int void_label, int B, int P, int HW,
                                   uint64_t* keys, hipStream_t s);
hipError_t spx_launch_prune_footprint(const int32_t* labels, int B, int Hf, int Wf, int H, int W, int P, const uint64_t* keys,
                                      const int32_t* target_class, int32_t* label, int32_t* box, hipStream_t s);
hipError_t spx_launch_prune_merge(const uint64_t* keys, const int32_t* label, const int32_t* box, int B, int P, int W, long long image0,
                                  int k, uint64_t* tkey, int64_t* timg, int32_t* tlabel, int32_t* tbox, int32_t* tcell, hipStream_t s);
// weight-side regularisers (spx_reg.hip)
size_t spx_reg_workspace(const spx_reg& r);
hipError_t spx_launch_reg_fwd(const spx_reg& r, float* total, float* terms, void* workspace, hipStream_t s);
hipError_t spx_launch_reg_bwd(const spx_reg& r, const float* g_total, const float* g_terms, float* d_wd, float* d_head,
                              hipStream_t s);
#ifdef SPX_DIAG
void spx_gemm_force(int wm, int splits);
#endif
size_t spx_gemm_workspace(int M, int N, int K, int flags);
hipError_t spx_launch_gemm(const float* A, long long ras, long long kas, const float* B, long long rbs, long long kbs,
                           float* C, long long ldc, int M, int N, int K, int flags, const float* E, long long lde,
                           float* ws, hipStream_t s);
int spx_pixel_outer_blocks(long long M);
hipError_t spx_launch_pixel_outer(const float* a, const float* b, long long M, int n1, int n2, float* out, float* parts, hipStream_t s);
hipError_t spx_launch_ce_fwd(const float* logits, const int32_t* labels, long long M, int K, float* lse, int32_t* pred,
                             float* partials, hipStream_t s);
hipError_t spx_launch_ce_bwd(const float* logits, const float* lse, const int32_t* labels, const float* coef, long long M, int K,
                             float* d_logits, hipStream_t s);
// segmented cross entropy (spx_ce_seg_*): the table by value
long long spx_ce_seg_blocks(const spx_ce_segments& seg);
hipError_t spx_launch_ce_seg_fwd(const float* logits, const int32_t* labels, const spx_ce_segments& seg, int K, float* lse, int32_t* pred,
                                 float* partials, hipStream_t s);
hipError_t spx_launch_ce_seg_finish(const float* partials, const spx_ce_segments& seg, float* losses, float* mean, float* count,
                                    int32_t* valid, int32_t* correct, hipStream_t s);
hipError_t spx_launch_ce_seg_bwd(const float* logits, const float* lse, const int32_t* labels, const spx_ce_segments& seg,
                                 const float* count, const float* g_losses, const float* g_mean, int K, float* d_logits, hipStream_t s);
hipError_t spx_launch_exp(const float* x, const float* g, const float* y, float* out, long long n, hipStream_t s);
hipError_t spx_launch_kld_lse(const uint32_t* keys, const uint64_t* ssum_fx, int n, float* lse, const uint32_t* range_keys, int HW,
                              double* scale_out, hipStream_t s);
hipError_t spx_launch_kld_gram_loss(const int64_t* a_fx, const double* scale, const uint32_t* counts, const uint8_t* pair_ok, int nseg, int K,
                                    int J, float* A, float* Cf, double* part, float* loss, hipStream_t s);
// activation-overlap metrics (spx_overlap.hip)
size_t spx_overlap_ws_bytes(int N, int C, int K);
hipError_t spx_launch_overlap_thresholds(const float* planes, const long long* st, int N, int C, int h, int w, int H, int W,
                                         long long k, float gamma, void* workspace, float* thresholds, hipStream_t s);
hipError_t spx_launch_overlap_accumulate(const float* planes, const long long* st, const float* thresholds, const void* labels,
                                         int label_bytes, const int32_t* table, int N, int C, int K, int J, int h, int w, int H, int W,
                                         unsigned long long* inter, unsigned long long* area, unsigned long long* images,
                                         void* workspace, hipStream_t s);
// push bounding boxes (spx_pushbox.hip)
hipError_t spx_launch_push_boxes(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                 const float* thresholds, int per_row, int R, int N, int C, int h, int w, int H, int W, int add_margin,
                                 int32_t* rf_boxes, int32_t* crops, hipStream_t s);
// class-restricted thresholds (spx_masked_select.hip)
size_t spx_masked_ws_bytes(int R);
hipError_t spx_launch_masked_thresholds(const float* planes, const long long* st, const void* labels, int label_bytes,
                                        const int32_t* rows, int R, int N, int C, int h, int w, int H, int W, double q, void* workspace,
                                        float* thresholds, hipStream_t s);
// nearest-image / nearest-prototype analysis (spx_nearest.hip)
hipError_t spx_launch_patch_majority(const void* labels, int label_bytes, const int32_t* rows, int R, int N, int h, int w, int H, int W,
                                     int bins, int32_t* majority, hipStream_t s);
hipError_t spx_launch_nearest_protos(const float* distances, const int32_t* queries, const uint8_t* include, int Q, int B, int P, int h,
                                     int w, int k, int window, long long* index, float* value, hipStream_t s);
// explanation maps (spx_explain.hip)
hipError_t spx_launch_explain_range(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                    int R, int N, int C, int h, int w, int H, int W, void* workspace, hipStream_t s);
hipError_t spx_launch_explain_heat(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                   int R, int N, int C, int h, int w, int H, int W, const void* workspace, uint8_t* heat, float* ranges,
                                   hipStream_t s);
hipError_t spx_launch_explain_dominant(const float* planes, const long long* st, const void* labels, int label_bytes,
                                       const int32_t* rows, const int32_t* table, const float* weights, int R, int N, int C, int K, int J,
                                       int h, int w, int H, int W, uint8_t* dom, hipStream_t s);
hipError_t spx_launch_predict_accumulate(const float* logits, const long long* lst, const void* labels, int label_bytes,
                                         const uint8_t* id_map, int N, int K, int h, int w, int H, int W, uint8_t* pred,
                                         unsigned long long* conf, hipStream_t s);
hipError_t spx_launch_failure_table(const long long* conf, int N, int K, double threshold, double* iou, int32_t* miss, uint8_t* fail,
                                    hipStream_t s);
hipError_t spx_launch_paired_range(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                   int R, int Q, int N, int C, int h, int w, int H, int W, void* workspace, hipStream_t s);
hipError_t spx_launch_paired_heat(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                  int R, int Q, int N, int C, int h, int w, int H, int W, const void* workspace, uint8_t* heat,
                                  float* ranges, hipStream_t s);
size_t spx_actloss_ws_bytes(int B, int K, int J);
hipError_t spx_launch_actloss_max(const spx_actloss* p, void* workspace, hipStream_t s);
hipError_t spx_launch_actloss_sums(const spx_actloss* p, void* workspace, hipStream_t s);
hipError_t spx_launch_actloss_finish(const spx_actloss* p, void* workspace, float* coef, float* out, hipStream_t s);
hipError_t spx_launch_actloss_backward(const spx_actloss* p, const float* coef, const float* g_total, const float* g_terms, float* grad,
                                       hipStream_t s);
// the four streaming passes of the KLD loss (spx_kld.hip)
hipError_t spx_launch_kld_max(const float* vals, const int32_t* labels, int B, int J, int HW, int W, int K, uint32_t* smax_keys,
                              uint32_t* counts, uint32_t* range_keys, hipStream_t s);
hipError_t spx_launch_kld_sumexp(const float* vals, const int32_t* labels, int B, int J, int HW, int W, int K, const uint32_t* smax_keys,
                                 uint64_t* ssum_fx, hipStream_t s);
hipError_t spx_launch_kld_pairs(const float* vals, const int32_t* labels, int B, int J, int HW, int W, int K, const float* lse,
                                const double* scale, int64_t* a_fx, hipStream_t s);
hipError_t spx_launch_kld_backward(const float* vals, const int32_t* labels, int B, int J, int HW, int K, const float* lse, const float* A,
                                   const float* Cf, const float* cf_scale, float* grad, hipStream_t s);
// cross-scale feature aggregation (spx_scale_agg.hip)
size_t spx_scale_agg_workspace(int B, int Cs, int Pn, int HW);
hipError_t spx_launch_scale_agg_fwd(const void* x, int x_bf16, long long x_bstride, const float* src, int src_kind, const float* proto,
                                    float* out, int B, int Cs, int Pn, int HW, int mode, float eps, hipStream_t s);
hipError_t spx_launch_scale_agg_bwd(const void* x, int x_bf16, long long x_bstride, const float* src, int src_kind, const float* proto,
                                    const float* g, void* dx, float* dsrc, float* dproto, void* ws, int B, int Cs, int Pn, int HW,
                                    int mode, float eps, hipStream_t s);
// part consistency / stability (spx_parts.hip)
size_t spx_parts_comp_ws_bytes(int N, int H, int W);
size_t spx_parts_thr_ws_bytes(int N, int K, int h, int w);
hipError_t spx_launch_part_components(const void* labels, int label_bytes, const void* parts, int part_bytes, int N, int K, int M, int H,
                                      int W, void* workspace, unsigned long long* totals, hipStream_t s);
hipError_t spx_launch_part_thresholds(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* table,
                                      const uint8_t* skip, int N, int C, int K, int J, int h, int w, int H, int W, double q, int mode,
                                      void* workspace, float* thresholds, hipStream_t s);
hipError_t spx_launch_part_presence(const float* planes, const long long* st, const void* labels, int label_bytes, const void* parts,
                                    int part_bytes, const int32_t* table, const uint8_t* skip, const float* thresholds,
                                    const void* comp_workspace, const unsigned long long* totals, int N, int C, int K, int J, int M, int h,
                                    int w, int H, int W, uint8_t* out, uint8_t* valid, hipStream_t s);
hipError_t spx_launch_part_fold_consistency(const uint8_t* tab, const uint8_t* valid, const int32_t* table, int N, int C, int K, int J, int M,
                                            long long* counters, hipStream_t s);
hipError_t spx_launch_part_fold_stability(const uint8_t* clean, const uint8_t* noisy, const uint8_t* valid, const int32_t* table, int N, int C,
                                          int K, int J, int M, unsigned long long* counters, hipStream_t s);
// training-batch preparation (spx_batch.hip)
hipError_t spx_launch_batch_prepare(const spx_batch& a, hipStream_t s);
hipError_t spx_launch_resize_labels(const spx_batch& a, hipStream_t s);
// multi-scale input fusion (spx_msc.hip)
hipError_t spx_launch_msc_max_fwd(const spx_msc& a, hipStream_t s);
hipError_t spx_launch_msc_max_bwd(const spx_msc& a, hipStream_t s);
hipError_t spx_launch_msc_pack_fwd(const spx_msc& a, int with_max, hipStream_t s);
hipError_t spx_launch_msc_pack_bwd(const spx_msc& a, int with_max, hipStream_t s);
