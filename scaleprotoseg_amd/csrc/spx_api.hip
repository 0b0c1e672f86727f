// C ABI of libspx_hip.so (see include/spx_hip.h).  Host-side validation + kernel launches; no torch types,
// no allocation, no synchronisation (graph-capturable).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "spx_args.h"

static thread_local char g_err[512] = "";
#ifdef SPX_DIAG
// diagnostic builds only (-DSPX_DIAG, never the product library: include/spx_hip.h promises no process-global state): the
// buffer of the in-kernel phase clocks (SPX_DIAG_STAMPS) and overrides of the tile permutation / product-kernel tiling
static unsigned long long* g_dbg = nullptr;
static int g_tile_mul_req = 0;                 // 0 = automatic (below), 1 = identity, > 1 = that multiplier
#else
static constexpr unsigned long long* g_dbg = nullptr;
static constexpr int g_tile_mul_req = 0;
#endif

// Block -> tile permutation of the pixel kernels: tile = (block * mul) mod tiles with mul coprime to the tile count, so that
// the workgroups running at one time are spread over the whole pixel range instead of covering one contiguous stretch of every
// feature plane (see profiles/EXPERIMENTS.md, plane strides).
static int gcd_i(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
int spx_tile_mul(int tiles_launch, long long plane_bytes) {
    // Automatic: only where the feature planes are a multiple of 1 MiB apart (power-of-two grids such as 1024 x 2048: plane
    // stride 4 MiB).  There neighbouring tiles of all channels fall on the same few DRAM banks at the same time and spreading
    // the co-running tiles 64 KiB apart measured -3.5 % (forward) / -1.6 % (pixel backward); on every other stride tried it
    // changed nothing or cost up to 15 % (1016 x 2048), so it stays off there (tools/probes/stride_sweep.py).
    int m = g_tile_mul_req;
    if (m == 0) m = (plane_bytes > 0 && plane_bytes % (1ll << 20) == 0) ? 257 : 1;
    if (m <= 1 || tiles_launch < 4 * m) return 1;
    while (gcd_i(m, tiles_launch) != 1) ++m;
    return m;
}

static int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
static int hip_status(hipError_t e, const char* what) {
    if (e == hipSuccess) return 0;
    return fail("%s: %s", what, hipGetErrorString(e));
}
static int check_plan(const spx_plan* pl) {
    if (!pl) return fail("plan is NULL");
    if (pl->npanels < 1 || pl->npanels > SPX_MAX_PANELS) return fail("plan: npanels %d out of range", pl->npanels);
    if (pl->kc != 32) return fail("plan: kc %d", pl->kc);
    if (pl->npb != 2 && pl->npb != 4 && pl->npb != 6) return fail("plan: npb %d (must be 2, 4 or 6)", pl->npb);
    if (pl->ncb != 1 && pl->ncb != 2 && pl->ncb != 5) return fail("plan: ncb %d (must be 1, 2 or 5)", pl->ncb);
    return 0;
}

// Scale-parallel launch (grid.y = scale): for pixel grids that do not fill the chip (the reference's training crops:
// 10 x 65 x 65 px = 331 tiles on 512-768 workgroup slots, each walking every panel of every scale serially) the
// panels of different scales are independent work - different channels of X and dX, different prototype rows - and run
// as separate workgroups.  Only the logits (a sum over all prototypes) need a second step, a fixed-order sum of the
// per-scale partials.  Returns the number of groups (1 = keep the single walk) and their first panels.
#define SPX_SPLIT_MAX_TILES 1024
int spx_split_groups(const spx_plan& pl, int B, int HW, int32_t* group_first) {
    const long long tiles = (long long)B * ((HW + SPX_TILE_PX - 1) / SPX_TILE_PX);
    int g = 0;
    for (int q = 0; q < pl.npanels; ++q)
        if (q == 0 || pl.panel_ch0[q] != pl.panel_ch0[q - 1]) group_first[g++] = q;
    group_first[g] = pl.npanels;
    if (g < 2 || tiles > SPX_SPLIT_MAX_TILES) {
        group_first[0] = 0;
        group_first[1] = pl.npanels;
        return 1;
    }
    return g;
}

hipError_t spx_launch_fwd_npb2(const SpxFwdArgs& a, int x_dtype, hipStream_t s);
hipError_t spx_launch_fwd_npb4(const SpxFwdArgs& a, int x_dtype, hipStream_t s);
hipError_t spx_launch_fwd_npb6(const SpxFwdArgs& a, int x_dtype, hipStream_t s);
hipError_t spx_launch_bwd_npb2(const SpxBwdArgs& a, int x_dtype, hipStream_t s);
hipError_t spx_launch_bwd_npb4(const SpxBwdArgs& a, int x_dtype, hipStream_t s);
hipError_t spx_launch_bwd_npb6(const SpxBwdArgs& a, int x_dtype, hipStream_t s);
hipError_t spx_launch_fwd(const SpxFwdArgs& a, int x_dtype, hipStream_t s) {
    return a.plan.npb == 2 ? spx_launch_fwd_npb2(a, x_dtype, s) : a.plan.npb == 4 ? spx_launch_fwd_npb4(a, x_dtype, s) : spx_launch_fwd_npb6(a, x_dtype, s);
}
hipError_t spx_launch_bwd(const SpxBwdArgs& a, int x_dtype, hipStream_t s) {
    return a.plan.npb == 2 ? spx_launch_bwd_npb2(a, x_dtype, s) : a.plan.npb == 4 ? spx_launch_bwd_npb4(a, x_dtype, s) : spx_launch_bwd_npb6(a, x_dtype, s);
}

extern "C" {

int spx_version(void) { return SPX_ABI_VERSION; }
#ifdef SPX_DIAG
void spx_diag_set_debug_buffer(void* p) { g_dbg = (unsigned long long*)p; }
void spx_diag_set_tile_mul(int m) { g_tile_mul_req = m; }       /* 1 = identity */
void spx_diag_set_gemm(int wm, int splits) { spx_gemm_force(wm, splits); }     /* 0 = the shape-derived default */
#endif
const char* spx_last_error(void) { return g_err; }

int spx_make_plan(int32_t P, int32_t K, int32_t S, int32_t Cs, const int32_t* lo, const int32_t* hi, spx_plan* out) {
    if (!out || !lo || !hi) return fail("spx_make_plan: NULL argument");
    if (P < 1 || K < 1 || S < 1 || Cs < 1) return fail("spx_make_plan: non-positive size (P=%d K=%d S=%d Cs=%d)", P, K, S, Cs);
    if (Cs % 16) return fail("spx_make_plan: channels per scale (%d) must be a multiple of 16 (MFMA k-step)", Cs);
    if (K > 160) return fail("spx_make_plan: num_classes %d > 160 not supported by the fused head", K);
    memset(out, 0, sizeof(*out));
    out->num_prototypes = P;
    out->num_classes = K;
    out->num_scales = S;
    out->channels_per_scale = Cs;
    out->kc = 32;                              /* chunks of 32 channels; a 16-channel tail is zero-filled */
    out->ncb = (K <= 32) ? 1 : (K <= 64) ? 2 : 5;   /* the kernels are specialised for 1, 2 or 5 class blocks */
    int per_max = 1, covered = 0;
    for (int s = 0; s < S; ++s) {
        const int n = hi[s] - lo[s];
        if (lo[s] < 0 || hi[s] > P || n < 0) return fail("spx_make_plan: scale %d range (%d,%d) outside [0,%d]", s, lo[s], hi[s], P);
        if (s && lo[s] != hi[s - 1]) return fail("spx_make_plan: scale ranges must be contiguous");
        covered += n;
        if (n == 0) continue;
        const int np_s = (n + 191) / 192;
        const int per = (n + np_s - 1) / np_s;
        if (per > per_max) per_max = per;
    }
    // the reference's F.linear rejects a distance map narrower than the head (P % S != 0): same here
    if (covered != P) return fail("spx_make_plan: scale table covers %d prototypes but the bank has %d (reference needs P %% S == 0)", covered, P);
    out->npb = ((per_max + 63) / 64) * 2;      /* panel height in 32-prototype blocks: 2, 4 or 6 */
    const int cap = out->npb * 32;
    int q = 0;
    for (int s = 0; s < S; ++s) {
        for (int p = lo[s]; p < hi[s]; p += cap) {
            if (q >= SPX_MAX_PANELS) return fail("spx_make_plan: more than %d panels", SPX_MAX_PANELS);
            out->panel_ch0[q] = s * Cs;
            out->panel_p0[q] = p;
            out->panel_np[q] = (hi[s] - p < cap) ? hi[s] - p : cap;
            ++q;
        }
    }
    if (q == 0) return fail("spx_make_plan: empty bank");
    out->npanels = q;
    return 0;
}

size_t spx_bwd_scratch_bytes(const spx_plan* pl, int32_t B, int32_t HW) { return spx_bwd_scratch_elems(*pl, B, HW) * 2; }
size_t spx_bwd_dx_scratch_bytes(const spx_plan* pl, int32_t x_dtype, int32_t B, int32_t HW) {
    if (x_dtype != 0) return 0;                                     /* fp32 features accumulate in dX itself */
    for (int q = 1; q < pl->npanels; ++q)
        if (pl->panel_ch0[q] == pl->panel_ch0[q - 1])               /* some scale spans several panels */
            return (size_t)B * pl->num_scales * pl->channels_per_scale * (((size_t)HW + 3) / 4 * 4) * sizeof(float);
    return 0;
}
size_t spx_bwd_head_scratch_bytes(const spx_plan* pl, int32_t B, int32_t HW) {
    if (pl->ncb != 1) return spx_bwd_scratch_elems(*pl, B, HW) * 2;              /* the activation blob */
    const size_t tiles = (size_t)B * ((HW + SPX_TILE_PX - 1) / SPX_TILE_PX);
    return spx_dw_partial_bytes(pl->npanels, tiles, pl->npb, pl->num_classes) + 16;   /* d_W tile partials + the head scale */
}

size_t spx_packed_bank_bytes(const spx_plan* pl) {
    return (size_t)pl->npanels * pl->npb * 32 * (((pl->channels_per_scale + 31) / 32) * 32) * 2;
}
size_t spx_packed_bankT_bytes(const spx_plan* pl) {
    return (size_t)pl->npanels * pl->npb * 2 * ((pl->channels_per_scale + 31) / 32) * 1024;
}
size_t spx_packed_p2_bytes(const spx_plan* pl) { return (size_t)pl->npanels * pl->npb * 32 * 4; }
size_t spx_packed_head_bytes(const spx_plan* pl) { return (size_t)pl->ncb * pl->npanels * pl->npb * 2 * 2048; }
size_t spx_packed_headT_bytes(const spx_plan* pl) { return (size_t)pl->npanels * pl->npb * (pl->ncb * 2) * 2048; }

int spx_pack_bank(const spx_plan* pl, const float* bank, void* pb, void* pbT, float* p2, void* stream) {
    if (check_plan(pl)) return 1;
    if (!bank || !pb || !p2) return fail("spx_pack_bank: NULL buffer");
    return hip_status(spx_launch_pack_bank(*pl, bank, pb, pbT, p2, (hipStream_t)stream), "spx_pack_bank");
}

int spx_pack_head(const spx_plan* pl, const float* W, void* ph, void* phT, void* stream) {
    if (check_plan(pl)) return 1;
    if (!W || !ph) return fail("spx_pack_head: NULL buffer");
    return hip_status(spx_launch_pack_head(*pl, W, ph, phT, (hipStream_t)stream), "spx_pack_head");
}

size_t spx_packed_tail_bytes(const spx_plan* pl) { return (size_t)pl->ncb * 2 * 2048; }

int spx_pack_all(const spx_plan* pl, const float* bank, const float* W, const float* Wg, int32_t K2, void* packed_bank,
                 void* packed_bankT, float* p2, void* packed_head, void* packed_headT, void* packed_tail, void* packed_tailT,
                 void* stream) {
    if (check_plan(pl)) return 1;
    if (!bank || !packed_bank || !p2) return fail("spx_pack_all: NULL bank buffer");
    if ((packed_head || packed_headT) && !W) return fail("spx_pack_all: head outputs without a head");
    if (packed_headT && !packed_head) return fail("spx_pack_all: packed_headT without packed_head");
    if ((packed_tail || packed_tailT) && (!Wg || !W || !packed_tail)) return fail("spx_pack_all: tail outputs need W, Wg and packed_tail");
    if (packed_tail && (K2 < 1 || K2 > 32)) return fail("spx_pack_all: %d tail classes (the fused tail carries at most 32)", K2);
    SpxPackAllArgs a{};
    a.plan = *pl;
    a.bank = bank; a.W = W; a.Wg = Wg; a.K2 = K2;
    a.headT_units = packed_tail != nullptr;      // the grouping backward reads head^T in accumulator (unit) order
    a.packed_bank = packed_bank; a.packed_bankT = packed_bankT; a.p2 = p2;
    a.packed_head = packed_head; a.packed_headT = packed_headT; a.packed_tail = packed_tail; a.packed_tailT = packed_tailT;
    return hip_status(spx_launch_pack_all(a, (hipStream_t)stream), "spx_pack_all");
}

int spx_pack_group_tail(const spx_plan* pl, const float* Wg, int32_t K2, void* packed_tail, void* packed_tailT, void* stream) {
    if (check_plan(pl)) return 1;
    if (!Wg || !packed_tail) return fail("spx_pack_group_tail: NULL buffer");
    if (K2 < 1 || K2 > 32) return fail("spx_pack_group_tail: %d classes (the fused tail carries at most 32)", K2);
    return hip_status(spx_launch_pack_tail(*pl, Wg, K2, packed_tail, packed_tailT, (hipStream_t)stream), "spx_pack_group_tail");
}

int spx_pack_headT_units(const spx_plan* pl, const float* W, void* packed_headT_units, void* stream) {
    if (check_plan(pl)) return 1;
    if (!W || !packed_headT_units) return fail("spx_pack_headT_units: NULL buffer");
    return hip_status(spx_launch_pack_headT_units(*pl, W, packed_headT_units, (hipStream_t)stream), "spx_pack_headT_units");
}

struct SpxTailFwd { const void* packed_tail; int32_t K2; float* gact; };
struct SpxTailBwd { const void* packed_tailT; int32_t K2; const float* gact; float* d_units; const float* d_gact; };

static int dist_fwd_impl(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                         const void* packed_bank, const float* packed_p2, const void* packed_head, float* distances,
                         const int32_t* labels, const uint32_t* proto_key, int32_t J, float* cls_dist,
                         float* activations, float* logits, float epsilon, int32_t act_fn, void* stream,
                         SpxTailFwd tail = SpxTailFwd{nullptr, 0, nullptr}, const spx_ce* ce = nullptr, void* split_ws = nullptr,
                         bool keep_partials = false, unsigned long long* push_keys = nullptr, float push_max = 0.0f, int push_void = -1, int push_K = 0,
                         int push_prune = 0) {
    if (check_plan(pl)) return 1;
    if (!x || !packed_bank || !packed_p2) return fail("spx_dist_fwd: NULL operand");
    if (x_dtype != 0 && x_dtype != 1) return fail("spx_dist_fwd: x_dtype %d (0 = bf16, 1 = fp32)", x_dtype);
    if (B < 1 || HW < 1) return fail("spx_dist_fwd: empty input (B=%d HW=%d)", B, HW);
    if (act_fn != 0 && act_fn != 1) return fail("spx_dist_fwd: act_fn %d", act_fn);
    if (logits && !packed_head) return fail("spx_dist_fwd: logits requested without a packed head");
    const long long tiles = (long long)B * ((HW + SPX_TILE_PX - 1) / SPX_TILE_PX);
    if (tiles > 0x7fffffffLL) return fail("spx_dist_fwd: too many pixel tiles");
    if ((long long)pl->num_prototypes * HW >= (1LL << 29)) return fail("spx_dist_fwd: P*HW too large for 32-bit offsets");
    if ((long long)pl->num_scales * pl->channels_per_scale * HW * (x_dtype ? 4 : 2) >= (1LL << 32)) return fail("spx_dist_fwd: one image of features exceeds 4 GiB");
    SpxFwdArgs a;
    a.plan = *pl;
    a.x = x;
    a.packed_bank = (const char*)packed_bank;
    a.p2 = packed_p2;
    a.packed_head = (const char*)packed_head;
    a.dist = distances;
    a.act = activations;
    a.logits = logits;
    a.B = B;
    a.HW = HW;
    a.labels = labels;
    a.proto_key = proto_key;
    a.cls_dist = cls_dist;
    a.J = J;
    a.push_keys = push_keys;
    a.push_max = push_max;
    a.push_void = push_void;
    a.push_K = push_K;
    a.push_prune = push_prune;
    a.packed_tail = (const char*)tail.packed_tail;
    a.gact = tail.gact;
    a.K2 = tail.K2;
    a.dist_vec = distances && ((uintptr_t)distances & 15) == 0 && HW % 4 == 0;
    a.ce_labels = nullptr;
    a.ce_lse = nullptr;
    a.ce_pred = nullptr;
    a.ce_partials = nullptr;
    if (ce) {
        if (!logits) return fail("spx_dist_fwd_ce: the cross entropy needs the logits output");
        if (!ce->labels || !ce->lse || !ce->partials) return fail("spx_dist_fwd_ce: NULL labels / lse / partials");
        a.ce_labels = ce->labels;
        a.ce_lse = ce->lse;
        a.ce_pred = ce->pred;
        a.ce_partials = ce->partials;
    }
    a.eps = epsilon;
    a.act_fn = act_fn;
    a.dbg = g_dbg;
    // scale-parallel launch: always when no logits are asked for; with logits when the caller brought the workspace for
    // the per-scale partials (and neither a grouping tail nor the fused cross entropy rides on the logits tile)
    a.ngroups = 1;
    a.logits_group_stride = 0;
    const int groups = spx_split_groups(*pl, B, HW, a.group_first);
    if (groups > 1 && !tail.packed_tail && !ce && (!logits || split_ws)) {
        a.ngroups = groups;
        if (logits) {
            a.logits = (float*)split_ws;
            a.logits_group_stride = (size_t)B * HW * pl->num_classes;
        }
    }
    if (hip_status(spx_launch_fwd(a, x_dtype, (hipStream_t)stream), "spx_dist_fwd")) return 1;
    if (a.ngroups > 1 && logits && !keep_partials)
        return hip_status(spx_launch_sum_groups((const float*)split_ws, a.logits_group_stride, groups, logits, (hipStream_t)stream), "spx_dist_fwd (sum of the scale partials)");
    return 0;
}

int spx_dist_fwd(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                 const float* packed_p2, const void* packed_head, float* distances, float* activations,
                 float* logits, float epsilon, int32_t act_fn, void* stream) {
    return dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, packed_head, distances, nullptr, nullptr, 0,
                         nullptr, activations, logits, epsilon, act_fn, stream);
}

int spx_dist_fwd_group(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                       const void* packed_bank, const float* packed_p2, const void* packed_head,
                       const void* packed_tail, int32_t K2, float* distances, float* activations,
                       float* group_activations, float* logits, float epsilon, int32_t act_fn, void* stream) {
    if (!packed_head || !packed_tail || !logits) return fail("spx_dist_fwd_group: NULL head / tail / logits");
    if (K2 < 1 || K2 > 32) return fail("spx_dist_fwd_group: %d classes (at most 32)", K2);
    return dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, packed_head, distances, nullptr, nullptr, 0,
                         nullptr, activations, logits, epsilon, act_fn, stream, SpxTailFwd{packed_tail, K2, group_activations});
}

static int check_cls(const char* who, const int32_t* labels, const uint32_t* proto_key, int32_t J, int32_t HW) {
    if (!labels || !proto_key) return fail("%s: NULL labels / proto_key", who);
    if (J < 1 || J > 0xFFFF) return fail("%s: J %d out of range", who, J);
    if ((long long)HW * J >= (1LL << 29)) return fail("%s: HW*J too large for 32-bit offsets", who);
    return 0;
}

size_t spx_group_tail_workspace_bytes(const spx_plan* pl, int32_t B, int32_t HW) {
    return pl ? (size_t)B * HW * pl->num_classes * sizeof(float) : 0;
}

int spx_dist_fwd_group_ws(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                          const void* packed_bank, const float* packed_p2, const void* packed_head,
                          const float* Wg, int32_t K2, float* distances, float* activations,
                          float* group_activations, float* logits, const spx_ce* ce, void* workspace,
                          float epsilon, int32_t act_fn, void* stream) {
    if (!packed_head || !Wg || !logits || !workspace) return fail("spx_dist_fwd_group_ws: NULL head / W_g / logits / workspace");
    if (K2 < 1 || K2 > 32) return fail("spx_dist_fwd_group_ws: %d classes (at most 32)", K2);
    if (check_plan(pl)) return 1;
    if (ce && (!ce->labels || !ce->lse || !ce->partials)) return fail("spx_dist_fwd_group_ws: NULL labels / lse / partials");
    // the unit product as the kernel's \"logits\" into the workspace, then the tail kernel.  NOT scale-parallel: measured on
    // the Cityscapes crops (10 x 65 x 65, 57 units) the per-scale partial units cost more traffic (4 x [M][57] written and
    // re-read: +30 us) than the shorter panel walk saves
    const int groups = 1;
    float* const parts = (float*)workspace;
    if (dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, packed_head, distances, nullptr, nullptr, 0, nullptr,
                      activations, parts, epsilon, act_fn, stream, SpxTailFwd{nullptr, 0, nullptr}, nullptr, nullptr, true))
        return 1;
    const long long M = (long long)B * HW;
    // the tail writes one (sum, count) pair per 64 pixels and clears the rest of the spx_ce_partials_flat(M) pairs itself
    return hip_status(spx_launch_group_tail(parts, groups, M, pl->num_classes, Wg, K2, group_activations, logits,
                                            ce ? ce->labels : nullptr, ce ? ce->lse : nullptr, ce ? ce->pred : nullptr,
                                            ce ? ce->partials : nullptr, (hipStream_t)stream), "spx_dist_fwd_group_ws (tail)");
}

int spx_dist_fwd_cls(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                     const void* packed_bank, const float* packed_p2, const void* packed_head,
                     const int32_t* labels, const uint32_t* proto_key, int32_t J, float* class_distances,
                     float* activations, float* logits, float epsilon, int32_t act_fn, void* stream) {
    if (check_cls("spx_dist_fwd_cls", labels, proto_key, J, HW)) return 1;
    if (!class_distances) return fail("spx_dist_fwd_cls: NULL class_distances");
    return dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, packed_head, nullptr, labels, proto_key, J,
                         class_distances, activations, logits, epsilon, act_fn, stream);
}

int spx_dist_push_min(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                      const float* packed_p2, const int32_t* labels, int32_t void_class, int32_t K, const uint32_t* proto_key,
                      float max_dist, int64_t* indices, float* values, uint64_t* scratch, void* stream) {
    if (check_cls("spx_dist_push_min", labels, proto_key, 1, HW)) return 1;
    if (K < 1 || K > 0xFFFD) return fail("spx_dist_push_min: K %d out of range", K);
    if (!indices || !values || !scratch) return fail("spx_dist_push_min: NULL output / scratch");
    if (check_plan(pl)) return 1;
    const size_t n = (size_t)B * pl->num_prototypes;
    if (hip_status(hipMemsetAsync(scratch, 0xFF, n * sizeof(uint64_t), (hipStream_t)stream), "spx_dist_push_min (scratch fill)")) return 1;
    if (dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, nullptr, nullptr, labels, proto_key, 1, nullptr, nullptr, nullptr,
                      1e-4f, 0, stream, SpxTailFwd{nullptr, 0, nullptr}, nullptr, nullptr, false, (unsigned long long*)scratch, max_dist, void_class, K))
        return 1;
    return hip_status(spx_launch_push_finalize(scratch, (int)n, indices, values, (hipStream_t)stream), "spx_dist_push_min (decode)");
}

int spx_dist_prune_min(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                       const float* packed_p2, const int32_t* labels, int32_t void_label, const uint32_t* proto_key, uint64_t* keys,
                       void* stream) {
    if (check_cls("spx_dist_prune_min", labels, proto_key, 1, HW)) return 1;
    if (!keys) return fail("spx_dist_prune_min: NULL keys");
    if (check_plan(pl)) return 1;
    if (B < 1 || B > 65535) return fail("spx_dist_prune_min: B %d out of range", B);
    const size_t n = (size_t)B * pl->num_prototypes;
    if (hip_status(hipMemsetAsync(keys, 0xFF, n * sizeof(uint64_t), (hipStream_t)stream), "spx_dist_prune_min (key fill)")) return 1;
    return dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, nullptr, nullptr, labels, proto_key, 1, nullptr, nullptr,
                         nullptr, 1e-4f, 0, stream, SpxTailFwd{nullptr, 0, nullptr}, nullptr, nullptr, false,
                         (unsigned long long*)keys, 0.0f, void_label, 1, 1);
}

static int dist_bwd_impl(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                         const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                         const void* packed_headT, const float* d_dist, const int32_t* labels,
                         const uint32_t* proto_key, int32_t J, const float* d_cls_dist, const float* d_act,
                         const float* d_logits, void* dx, void* dx_acc, void* g_out, void* a_out, float epsilon, int32_t act_fn,
                         void* stream, SpxTailBwd tail = SpxTailBwd{nullptr, 0, nullptr, nullptr, nullptr}, const spx_ce* ce = nullptr) {
    if (check_plan(pl)) return 1;
    if (!x || !packed_bank || !packed_p2) return fail("spx_dist_bwd: NULL operand");
    if (x_dtype != 0 && x_dtype != 1) return fail("spx_dist_bwd: x_dtype %d", x_dtype);
    if (B < 1 || HW < 1) return fail("spx_dist_bwd: empty input");
    if (dx && !packed_bankT) return fail("spx_dist_bwd: dx requested without packed bank^T");
    if ((d_logits || ce) && !packed_headT) return fail("spx_dist_bwd: d_logits given without packed head^T");
    if (ce && d_logits) return fail("spx_dist_bwd_ce: the fused cross entropy replaces d_logits");
    if (ce && (!ce->labels || !ce->lse || !ce->logits || !ce->coef)) return fail("spx_dist_bwd_ce: NULL labels / lse / logits / coef");
    if ((long long)pl->num_prototypes * HW >= (1LL << 29)) return fail("spx_dist_bwd: P*HW too large for 32-bit offsets");
    const long long tiles = (long long)B * ((HW + SPX_TILE_PX - 1) / SPX_TILE_PX);
    if (tiles > 0x7fffffffLL) return fail("spx_dist_bwd: too many pixel tiles");
    if ((long long)pl->num_scales * pl->channels_per_scale * HW * (x_dtype ? 4 : 2) >= (1LL << 32)) return fail("spx_dist_bwd: one image of features exceeds 4 GiB");
    if (g_out && pl->channels_per_scale > 256) return fail("spx_dist_bwd: G scratch requested but spx_bank_bwd supports channels_per_scale <= 256 (got %d)", pl->channels_per_scale);
    SpxBwdArgs a;
    a.plan = *pl;
    a.x = x;
    a.packed_bank = (const char*)packed_bank;
    a.packed_bankT = (const char*)packed_bankT;
    a.p2 = packed_p2;
    a.packed_headT = (const char*)packed_headT;
    a.d_dist = d_dist;
    a.d_act = d_act;
    a.d_logits = d_logits;
    a.labels = labels;
    a.proto_key = proto_key;
    a.d_cls_dist = d_cls_dist;
    a.J = J;
    a.packed_tailT = (const char*)tail.packed_tailT;
    a.gact = tail.gact;
    a.d_units = tail.d_units;
    a.d_gact = tail.d_gact;
    a.K2 = tail.K2;
    a.ce_labels = ce ? ce->labels : nullptr;
    a.ce_logits = ce ? ce->logits : nullptr;
    a.ce_lse = ce ? ce->lse : nullptr;
    a.ce_coef = ce ? ce->coef : nullptr;
    a.ce_dlogits_out = ce ? ce->d_logits_out : nullptr;
    a.dx = dx;
    a.dx_acc = (float*)dx_acc;
    a.g_out = (uint16_t*)g_out;
    a.a_out = (uint16_t*)a_out;
    a.B = B;
    a.HW = HW;
    a.eps = epsilon;
    a.act_fn = act_fn;
    a.dbg = g_dbg;
    a.ngroups = spx_split_groups(*pl, B, HW, a.group_first);      // the backward needs no cross-scale step at all
    return hip_status(spx_launch_bwd(a, x_dtype, (hipStream_t)stream), "spx_dist_bwd");
}

int spx_dist_bwd(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                 const void* packed_bankT, const float* packed_p2, const void* packed_headT, const float* d_dist,
                 const float* d_act, const float* d_logits, void* dx, void* dx_acc, void* g_out, void* a_out, float epsilon,
                 int32_t act_fn, void* stream) {
    return dist_bwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_bankT, packed_p2, packed_headT, d_dist, nullptr,
                         nullptr, 0, nullptr, d_act, d_logits, dx, dx_acc, g_out, a_out, epsilon, act_fn, stream);
}

int spx_dist_bwd_group(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                       const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                       const void* packed_headT_units, const void* packed_tailT, int32_t K2,
                       const float* group_activations, const float* d_dist, const float* d_act,
                       const float* d_logits, const float* d_group_activations, float* d_units, void* dx, void* dx_acc, void* g_out,
                       void* a_out, float epsilon, int32_t act_fn, void* stream) {
    if (!packed_headT_units || !packed_tailT || !group_activations || !d_logits || !d_units)
        return fail("spx_dist_bwd_group: NULL tail operand");
    if (K2 < 1 || K2 > 32) return fail("spx_dist_bwd_group: %d classes (at most 32)", K2);
    return dist_bwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_bankT, packed_p2, packed_headT_units, d_dist,
                         nullptr, nullptr, 0, nullptr, d_act, d_logits, dx, dx_acc, g_out, a_out, epsilon, act_fn, stream,
                         SpxTailBwd{packed_tailT, K2, group_activations, d_units, d_group_activations});
}

int spx_dist_bwd_group_ce(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                          const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                          const void* packed_headT_units, const void* packed_tailT, int32_t K2,
                          const float* group_activations, const float* d_dist, const float* d_act, const spx_ce* ce,
                          const float* d_group_activations, float* d_units, void* dx, void* dx_acc, void* g_out, void* a_out, float epsilon,
                          int32_t act_fn, void* stream) {
    if (!ce) return fail("spx_dist_bwd_group_ce: NULL ce");
    if (!packed_headT_units || !packed_tailT || !group_activations || !d_units)
        return fail("spx_dist_bwd_group_ce: NULL tail operand");
    if (K2 < 1 || K2 > 32) return fail("spx_dist_bwd_group_ce: %d classes (at most 32)", K2);
    return dist_bwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_bankT, packed_p2, packed_headT_units, d_dist,
                         nullptr, nullptr, 0, nullptr, d_act, nullptr, dx, dx_acc, g_out, a_out, epsilon, act_fn, stream,
                         SpxTailBwd{packed_tailT, K2, group_activations, d_units, d_group_activations}, ce);
}

int spx_dist_bwd_cls(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW,
                     const void* packed_bank, const void* packed_bankT, const float* packed_p2,
                     const void* packed_headT, const int32_t* labels, const uint32_t* proto_key, int32_t J,
                     const float* d_class_distances, const float* d_act, const float* d_logits, void* dx,
                     void* dx_acc, void* g_out, void* a_out, float epsilon, int32_t act_fn, void* stream) {
    if (check_cls("spx_dist_bwd_cls", labels, proto_key, J, HW)) return 1;
    // d_class_distances may be NULL (no gradient reaches the gathered distances)
    return dist_bwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_bankT, packed_p2, packed_headT, nullptr,
                         d_class_distances ? labels : nullptr, proto_key, J, d_class_distances, d_act, d_logits, dx, dx_acc,
                         g_out, a_out, epsilon, act_fn, stream);
}

int32_t spx_fwd_split_groups(const spx_plan* pl, int32_t B, int32_t HW) {
    int32_t gf[SPX_MAX_PANELS + 1];
    return pl ? spx_split_groups(*pl, B, HW, gf) : 1;
}
size_t spx_fwd_split_workspace_bytes(const spx_plan* pl, int32_t B, int32_t HW) {
    const int g = spx_fwd_split_groups(pl, B, HW);
    return g > 1 ? (size_t)g * B * HW * pl->num_classes * sizeof(float) : 0;
}
int spx_dist_fwd_ws(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                    const float* packed_p2, const void* packed_head, const int32_t* labels_cls, const uint32_t* proto_key,
                    int32_t J, float* class_distances, float* distances, float* activations, float* logits,
                    void* split_workspace, float epsilon, int32_t act_fn, void* stream) {
    if (labels_cls) {
        if (check_cls("spx_dist_fwd_ws", labels_cls, proto_key, J, HW)) return 1;
        if (!class_distances) return fail("spx_dist_fwd_ws: NULL class_distances");
        if (distances) return fail("spx_dist_fwd_ws: class-gathered and P-wide distances are exclusive");
    }
    return dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, packed_head, distances, labels_cls, proto_key,
                         labels_cls ? J : 0, labels_cls ? class_distances : nullptr, activations, logits, epsilon, act_fn,
                         stream, SpxTailFwd{nullptr, 0, nullptr}, nullptr, split_workspace);
}

size_t spx_ce_partials(int32_t B, int32_t HW) { return (size_t)B * ((HW + SPX_TILE_PX - 1) / SPX_TILE_PX) * 4; }
size_t spx_ce_partials_flat(int64_t M) { return (size_t)((M + 255) / 256) * 4; }

int spx_dist_fwd_ce(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                    const float* packed_p2, const void* packed_head, const int32_t* labels_cls, const uint32_t* proto_key,
                    int32_t J, float* class_distances, float* distances, float* activations, float* logits,
                    const spx_ce* ce, float epsilon, int32_t act_fn, void* stream) {
    if (!ce) return fail("spx_dist_fwd_ce: NULL ce");
    if (labels_cls) {
        if (check_cls("spx_dist_fwd_ce", labels_cls, proto_key, J, HW)) return 1;
        if (!class_distances) return fail("spx_dist_fwd_ce: NULL class_distances");
        if (distances) return fail("spx_dist_fwd_ce: class-gathered and P-wide distances are exclusive");
    }
    return dist_fwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_p2, packed_head, distances, labels_cls, proto_key,
                         labels_cls ? J : 0, labels_cls ? class_distances : nullptr, activations, logits, epsilon, act_fn,
                         stream, SpxTailFwd{nullptr, 0, nullptr}, ce);
}

int spx_dist_bwd_ce(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const void* packed_bank,
                    const void* packed_bankT, const float* packed_p2, const void* packed_headT, const int32_t* labels_cls,
                    const uint32_t* proto_key, int32_t J, const float* d_dist, const float* d_class_distances,
                    const float* d_act, const spx_ce* ce, void* dx, void* dx_acc, void* g_out, void* a_out, float epsilon,
                    int32_t act_fn, void* stream) {
    if (!ce) return fail("spx_dist_bwd_ce: NULL ce");
    if (labels_cls && check_cls("spx_dist_bwd_ce", labels_cls, proto_key, J, HW)) return 1;
    if (labels_cls && d_dist) return fail("spx_dist_bwd_ce: class-gathered and P-wide distance gradients are exclusive");
    return dist_bwd_impl(pl, x, x_dtype, B, HW, packed_bank, packed_bankT, packed_p2, packed_headT, d_dist,
                         (labels_cls && d_class_distances) ? labels_cls : nullptr, proto_key, labels_cls ? J : 0,
                         labels_cls ? d_class_distances : nullptr, d_act, nullptr, dx, dx_acc, g_out, a_out, epsilon, act_fn, stream,
                         SpxTailBwd{nullptr, 0, nullptr, nullptr, nullptr}, ce);
}

size_t spx_pixel_outer_workspace_bytes(int64_t M, int32_t n1, int32_t n2) {
    return (size_t)spx_pixel_outer_blocks(M) * n1 * n2 * sizeof(float);
}
int spx_pixel_outer(const float* a, const float* b, int64_t M, int32_t n1, int32_t n2, float* out, void* workspace, void* stream) {
    if (!a || !b || !out || !workspace) return fail("spx_pixel_outer: NULL buffer");
    if (M < 1 || n1 < 1 || n2 < 1 || (long long)n1 * n2 > 8192) return fail("spx_pixel_outer: bad sizes (M=%lld, %d x %d; n1*n2 <= 8192)", (long long)M, n1, n2);
    return hip_status(spx_launch_pixel_outer(a, b, M, n1, n2, out, (float*)workspace, (hipStream_t)stream), "spx_pixel_outer");
}

size_t spx_rows_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K, int32_t flags) {
    if (M < 1 || N < 1 || K < 1) return 0;
    return spx_gemm_workspace(M, N, K, flags);
}
int spx_rows_gemm(const float* A, int64_t ras, int64_t kas, const float* B, int64_t rbs, int64_t kbs, float* C, int64_t ldc,
                  int32_t M, int32_t N, int32_t K, int32_t flags, const float* E, int64_t lde, void* workspace, void* stream) {
    if (!A || !B || !C) return fail("spx_rows_gemm: NULL operand");
    if (M < 1 || N < 1 || K < 1) return fail("spx_rows_gemm: bad sizes (M=%d N=%d K=%d)", M, N, K);
    if ((ras != 1 && kas != 1) || (rbs != 1 && kbs != 1) || ras < 1 || kas < 1 || rbs < 1 || kbs < 1)
        return fail("spx_rows_gemm: each operand needs one unit stride (A: %lld, %lld; B: %lld, %lld)", (long long)ras, (long long)kas,
                    (long long)rbs, (long long)kbs);
    if (ldc < N) return fail("spx_rows_gemm: ldc (%lld) < N (%d)", (long long)ldc, N);
    if (flags & ~7) return fail("spx_rows_gemm: unknown flags 0x%x", flags);
    if ((flags & 4) && (!E || lde < N)) return fail("spx_rows_gemm: flag 4 needs E with lde >= N");
    if (spx_gemm_workspace(M, N, K, flags) && !workspace) return fail("spx_rows_gemm: workspace needed (spx_rows_gemm_workspace_bytes)");
    return hip_status(spx_launch_gemm(A, ras, kas, B, rbs, kbs, C, ldc, M, N, K, flags, E, lde, (float*)workspace, (hipStream_t)stream),
                      "spx_rows_gemm");
}

int spx_exp(const float* x, float* y, int64_t n, void* stream) {
    if (!x || !y || n < 1 || (n + 255) / 256 > 0x7fffffffLL) return fail("spx_exp: bad arguments");
    return hip_status(spx_launch_exp(x, nullptr, nullptr, y, n, (hipStream_t)stream), "spx_exp");
}
int spx_exp_bwd(const float* g, const float* y, float* dx, int64_t n, void* stream) {
    if (!g || !y || !dx || n < 1 || (n + 255) / 256 > 0x7fffffffLL) return fail("spx_exp_bwd: bad arguments");
    return hip_status(spx_launch_exp(nullptr, g, y, dx, n, (hipStream_t)stream), "spx_exp_bwd");
}

int spx_group_dense(const float* const* block_ptrs, const int32_t* block_cols, int32_t nblocks, const int32_t* row_block,
                    const int32_t* row_local, const int32_t* col_block, const int32_t* col_local, int32_t U, int32_t P, float* out,
                    void* stream) {
    if (!block_ptrs || !block_cols || !row_block || !row_local || !col_block || !col_local || !out) return fail("spx_group_dense: NULL buffer");
    if (nblocks < 1 || nblocks > SPX_GROUP_BLOCKS_MAX) return fail("spx_group_dense: %d blocks (1..%d)", nblocks, SPX_GROUP_BLOCKS_MAX);
    if (U < 1 || P < 1 || (long long)U * P > 0x7fffffffLL) return fail("spx_group_dense: bad sizes (U=%d P=%d)", U, P);
    SpxGroupDenseArgs a{};
    for (int j = 0; j < nblocks; ++j) {
        if (!block_ptrs[j] || block_cols[j] < 1) return fail("spx_group_dense: block %d is empty", j);
        a.ptrs[j] = block_ptrs[j];
        a.ncols[j] = block_cols[j];
    }
    a.row_block = row_block; a.row_local = row_local; a.col_block = col_block; a.col_local = col_local;
    a.U = U; a.P = P; a.out = out;
    return hip_status(spx_launch_group_dense(a, (hipStream_t)stream), "spx_group_dense");
}
int spx_group_dense_bwd(const float* d_out, const int32_t* flat_row, const int32_t* flat_col, int64_t n, int32_t P, float* d_flat,
                        void* stream) {
    if (!d_out || !flat_row || !flat_col || !d_flat) return fail("spx_group_dense_bwd: NULL buffer");
    if (n < 1 || P < 1 || (n + 255) / 256 > 0x7fffffffLL) return fail("spx_group_dense_bwd: bad sizes");
    return hip_status(spx_launch_group_dense_bwd(d_out, flat_row, flat_col, n, P, d_flat, (hipStream_t)stream), "spx_group_dense_bwd");
}

int spx_simplex_project(float* const* block_ptrs, const int32_t* block_rows, const int32_t* block_cols, int32_t nblocks, float z,
                        void* stream) {
    static const char* who = "spx_simplex_project";
    if (!block_ptrs || !block_rows || !block_cols) return fail("%s: NULL table", who);
    if (nblocks < 1 || nblocks > SPX_GROUP_BLOCKS_MAX) return fail("%s: %d blocks (1..%d)", who, nblocks, SPX_GROUP_BLOCKS_MAX);
    SpxSimplexArgs a{};
    long long rows = 0;
    for (int j = 0; j < nblocks; ++j) {
        if (!block_ptrs[j]) return fail("%s: block %d is NULL", who, j);
        if (block_rows[j] < 1) return fail("%s: block %d has %d rows (>= 1)", who, j, block_rows[j]);
        if (block_cols[j] < 1 || block_cols[j] > SPX_SIMPLEX_MAX_COLS)
            return fail("%s: block %d has %d columns (1..%d)", who, j, block_cols[j], SPX_SIMPLEX_MAX_COLS);
        a.ptrs[j] = block_ptrs[j];
        a.cols[j] = block_cols[j];
        a.row0[j] = (int)rows;
        rows += block_rows[j];
        if (rows > 0x7fffffffLL) return fail("%s: more than 2^31 - 1 rows", who);
    }
    a.row0[nblocks] = (int)rows;
    a.nblocks = nblocks;
    a.z = z;
    return hip_status(spx_launch_simplex(a, (hipStream_t)stream), who);
}

int spx_ce_fwd(const float* logits, const int32_t* labels, int64_t M, int32_t K, float* lse, int32_t* pred, float* partials,
               void* stream) {
    if (!logits || !labels || !lse || !partials) return fail("spx_ce_fwd: NULL buffer");
    if (M < 1 || K < 1 || (M + 255) / 256 > 0x7fffffffLL) return fail("spx_ce_fwd: bad sizes (M=%lld K=%d)", (long long)M, K);
    return hip_status(spx_launch_ce_fwd(logits, labels, M, K, lse, pred, partials, (hipStream_t)stream), "spx_ce_fwd");
}
int spx_ce_finish(const float* partials, int64_t n_pairs, float* loss, float* count_sum, void* stream) {
    if (!partials || !loss || !count_sum || n_pairs < 1) return fail("spx_ce_finish: bad arguments");
    return hip_status(spx_launch_ce_finish(partials, n_pairs, loss, count_sum, (hipStream_t)stream), "spx_ce_finish");
}
int spx_shift_labels(const void* labels, int32_t is_int64, int64_t n, int32_t* out, void* stream) {
    if (!labels || !out || n < 1 || (n + 255) / 256 > 0x7fffffffLL) return fail("spx_shift_labels: bad arguments");
    return hip_status(spx_launch_shift_labels(labels, is_int64, n, out, (hipStream_t)stream), "spx_shift_labels");
}
int spx_ce_bwd(const float* logits, const float* lse, const int32_t* labels, const float* coef, int64_t M, int32_t K,
               float* d_logits, void* stream) {
    if (!logits || !lse || !labels || !coef || !d_logits) return fail("spx_ce_bwd: NULL buffer");
    if (M < 1 || K < 1 || (M * K + 255) / 256 > 0x7fffffffLL) return fail("spx_ce_bwd: bad sizes (M=%lld K=%d)", (long long)M, K);
    return hip_status(spx_launch_ce_bwd(logits, lse, labels, coef, M, K, d_logits, (hipStream_t)stream), "spx_ce_bwd");
}

// segmented cross entropy: the table is checked on every call (it is all the kernels know about the buffers' sizes)
static int check_ce_segments(const spx_ce_segments* seg, const char* who) {
    if (!seg) return fail("%s: NULL segment table", who);
    if (seg->S < 1 || seg->S > 16) return fail("%s: %d segments (1..16)", who, seg->S);
    if (seg->off[0] != 0) return fail("%s: off[0] = %lld (must be 0)", who, (long long)seg->off[0]);
    for (int k = 0; k < seg->S; ++k)
        if (seg->off[k + 1] <= seg->off[k])
            return fail("%s: segment %d is empty or the table is not increasing (off %lld .. %lld)", who, k, (long long)seg->off[k],
                        (long long)seg->off[k + 1]);
    if (seg->off[seg->S] > (1LL << 40) || spx_ce_seg_blocks(*seg) > 0x7fffffffLL)
        return fail("%s: %lld rows are too many", who, (long long)seg->off[seg->S]);
    return 0;
}
size_t spx_ce_seg_partials(const spx_ce_segments* seg) {
    if (check_ce_segments(seg, "spx_ce_seg_partials")) return 0;
    return (size_t)spx_ce_seg_blocks(*seg) * 4;
}
int spx_ce_seg_fwd(const float* logits, const int32_t* labels, const spx_ce_segments* seg, int32_t K, float* lse, int32_t* pred,
                   float* partials, void* stream) {
    if (check_ce_segments(seg, "spx_ce_seg_fwd")) return 1;
    if (!logits || !labels || !lse || !partials) return fail("spx_ce_seg_fwd: NULL buffer");
    if (K < 1) return fail("spx_ce_seg_fwd: K = %d", K);
    return hip_status(spx_launch_ce_seg_fwd(logits, labels, *seg, K, lse, pred, partials, (hipStream_t)stream), "spx_ce_seg_fwd");
}
int spx_ce_seg_finish(const float* partials, const spx_ce_segments* seg, float* losses, float* mean, float* count, int32_t* valid,
                      int32_t* correct, void* stream) {
    if (check_ce_segments(seg, "spx_ce_seg_finish")) return 1;
    if (!partials || !losses || !mean || !count || !valid || !correct) return fail("spx_ce_seg_finish: NULL buffer");
    return hip_status(spx_launch_ce_seg_finish(partials, *seg, losses, mean, count, valid, correct, (hipStream_t)stream),
                      "spx_ce_seg_finish");
}
int spx_ce_seg_bwd(const float* logits, const float* lse, const int32_t* labels, const spx_ce_segments* seg, const float* count,
                   const float* g_losses, const float* g_mean, int32_t K, float* d_logits, void* stream) {
    if (check_ce_segments(seg, "spx_ce_seg_bwd")) return 1;
    if (!logits || !lse || !labels || !count || !d_logits) return fail("spx_ce_seg_bwd: NULL buffer");
    if (K < 1 || seg->off[seg->S] > (0x7fffffffLL * 256 - 255) / K)                 /* the grid: one thread per element */
        return fail("spx_ce_seg_bwd: bad sizes (M=%lld K=%d)", (long long)seg->off[seg->S], K);
    return hip_status(spx_launch_ce_seg_bwd(logits, lse, labels, *seg, count, g_losses, g_mean, K, d_logits, (hipStream_t)stream),
                      "spx_ce_seg_bwd");
}

size_t spx_bank_bwd_workspace_bytes(const spx_plan* pl, int32_t B, int32_t HW) {
    const int nsplit = spx_bank_bwd_nsplit(*pl, B, HW);
    return spx_bank_bwd_ws_floats(*pl, nsplit) * sizeof(float);
}

int spx_bank_bwd(const spx_plan* pl, const void* x, int32_t x_dtype, int32_t B, int32_t HW, const float* bank,
                 const void* g_in, const void* a_in, const float* d_logits, float* d_bank, float* d_W,
                 void* workspace, void* stream) {
    if (check_plan(pl)) return 1;
    if (!x || !bank || !workspace) return fail("spx_bank_bwd: NULL operand");
    if (x_dtype != 0 && x_dtype != 1) return fail("spx_bank_bwd: x_dtype %d", x_dtype);
    if (d_bank && !g_in) return fail("spx_bank_bwd: d_bank requested without G");
    if (d_W && !a_in) return fail("spx_bank_bwd: d_W requested without the head-gradient scratch of spx_dist_bwd");
    if (d_W && pl->ncb > 1 && !d_logits) return fail("spx_bank_bwd: d_W of a head wider than 32 rows needs d_logits");
    if (pl->channels_per_scale > 256) return fail("spx_bank_bwd: Cs %d > 256 not supported", pl->channels_per_scale);
    SpxBankBwdArgs a;
    a.plan = *pl;
    a.x = x;
    a.bank = bank;
    a.g_in = (const uint16_t*)g_in;
    a.a_in = (const uint16_t*)a_in;
    a.d_logits = d_logits;
    a.d_bank = d_bank;
    a.d_W = d_W;
    a.workspace = (float*)workspace;
    a.B = B;
    a.HW = HW;
    a.nsplit = spx_bank_bwd_nsplit(*pl, B, HW);
    return hip_status(spx_launch_bank_bwd(a, x_dtype, (hipStream_t)stream), "spx_bank_bwd");
}

int spx_push_argmin(const float* distances, const int32_t* labels, const float* class_identity, int32_t B, int32_t P,
                    int32_t K, int32_t HW, int32_t void_class, float max_dist, int64_t* indices, float* values,
                    uint64_t* scratch, void* stream) {
    if (!distances || !labels || !class_identity || !indices || !values || !scratch)
        return fail("spx_push_argmin: NULL buffer");
    if (B < 1 || P < 1 || K < 1 || HW < 1) return fail("spx_push_argmin: empty input");
    if (K > 160) return fail("spx_push_argmin: num_classes %d > 160", K);
    if (P > 65535 || B > 65535) return fail("spx_push_argmin: grid too large");
    return hip_status(spx_launch_push_argmin(distances, labels, class_identity, B, P, K, HW, void_class, max_dist,
                                             indices, values, scratch, (hipStream_t)stream),
                      "spx_push_argmin");
}

int spx_prune_argmin(const float* distances, const int32_t* labels, int32_t void_label, int32_t B, int32_t P, int32_t HW,
                     uint64_t* keys, void* stream) {
    if (!distances || !labels || !keys) return fail("spx_prune_argmin: NULL buffer");
    if (B < 1 || P < 1 || HW < 1) return fail("spx_prune_argmin: empty input (B=%d P=%d HW=%d)", B, P, HW);
    if (P > 0x7FFF8 || B > 65535) return fail("spx_prune_argmin: grid too large (B=%d P=%d)", B, P);
    return hip_status(spx_launch_prune_argmin(distances, labels, void_label, B, P, HW, keys, (hipStream_t)stream), "spx_prune_argmin");
}

int spx_prune_footprint(const int32_t* labels, int32_t B, int32_t Hf, int32_t Wf, int32_t H, int32_t W, int32_t P,
                        const uint64_t* keys, const int32_t* target_class, int32_t* label, int32_t* box, void* stream) {
    if (!labels || !keys || !target_class || !label || !box) return fail("spx_prune_footprint: NULL buffer");
    if (B < 1 || P < 1 || Hf < 1 || Wf < 1 || H < 1 || W < 1)
        return fail("spx_prune_footprint: empty input (B=%d P=%d Hf=%d Wf=%d H=%d W=%d)", B, P, Hf, Wf, H, W);
    if (B > 65535 || P > 0x7FFFFFFF / 4) return fail("spx_prune_footprint: grid too large (B=%d P=%d)", B, P);
    if ((long long)H * W >= (1LL << 31)) return fail("spx_prune_footprint: latent grid too large");
    return hip_status(spx_launch_prune_footprint(labels, B, Hf, Wf, H, W, P, keys, target_class, label, box, (hipStream_t)stream),
                      "spx_prune_footprint");
}

int spx_prune_merge(const uint64_t* keys, const int32_t* label, const int32_t* box, int32_t B, int32_t P, int32_t W, int64_t image0,
                    int32_t k, uint64_t* table_key, int64_t* table_image, int32_t* table_label, int32_t* table_box, int32_t* table_cell,
                    void* stream) {
    if (!keys || !label || !box || !table_key || !table_image || !table_label || !table_box || !table_cell)
        return fail("spx_prune_merge: NULL buffer");
    if (B < 1 || P < 1 || W < 1) return fail("spx_prune_merge: empty input (B=%d P=%d W=%d)", B, P, W);
    if (k < 1 || k > SPX_PRUNE_MAX_K) return fail("spx_prune_merge: k %d outside 1..%d", k, SPX_PRUNE_MAX_K);
    if (image0 < 0) return fail("spx_prune_merge: negative image index");
    if ((((uintptr_t)box) | ((uintptr_t)table_box)) & 15) return fail("spx_prune_merge: box tables must be 16-byte aligned");
    return hip_status(spx_launch_prune_merge(keys, label, box, B, P, W, image0, k, table_key, table_image, table_label, table_box,
                                             table_cell, (hipStream_t)stream), "spx_prune_merge");
}

int spx_argmin_images(const float* values, int32_t N, int32_t P, int64_t* best, void* stream) {
    if (!values || !best) return fail("spx_argmin_images: NULL buffer");
    if (N < 1 || P < 1) return fail("spx_argmin_images: empty input");
    return hip_status(spx_launch_argmin_images(values, N, P, best, (hipStream_t)stream), "spx_argmin_images");
}

int spx_push_merge(const int64_t* indices, const float* values, const void* x, int32_t x_dtype, int32_t B, int32_t P, int32_t C,
                   int32_t HW, int32_t Cs, const int32_t* proto_scale, int64_t image0, float* best_value, int64_t* best_image,
                   int64_t* best_flat, float* best_patch, void* stream) {
    static const char* who = "spx_push_merge";
    if (!indices || !values || !x || !proto_scale) return fail("%s: NULL candidates / features / scale table", who);
    if (!best_value || !best_image || !best_flat || !best_patch) return fail("%s: NULL state", who);
    if (x_dtype != 0 && x_dtype != 1) return fail("%s: feature dtype code %d (0 = bf16, 1 = fp32)", who, x_dtype);
    if (B < 1 || P < 1 || C < 1 || HW < 1 || Cs < 1) return fail("%s: empty input (B=%d P=%d C=%d HW=%d Cs=%d)", who, B, P, C, HW, Cs);
    if (Cs > C) return fail("%s: %d channels per scale, features have %d", who, Cs, C);
    if (image0 < 0 || image0 > INT64_MAX - B) return fail("%s: image index %lld outside 0 .. 2^63 - 1 - B", who, (long long)image0);
    return hip_status(spx_launch_push_merge(indices, values, x, x_dtype, B, P, C, HW, Cs, proto_scale, image0, best_value, best_image,
                                            best_flat, best_patch, (hipStream_t)stream), who);
}

int spx_upsample_argext(const float* src, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                        int32_t take_max, int64_t* indices, float* values, void* stream) {
    if (!src || !indices) return fail("spx_upsample_argext: NULL buffer");
    if (N < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail("spx_upsample_argext: empty input");
    if ((long long)h * w >= (1LL << 31) || (long long)N > 65535) return fail("spx_upsample_argext: map too large");
    return hip_status(spx_launch_upsample_argext(src, N, C, h, w, H, W, take_max ? 1 : 0, indices, values,
                                                 (hipStream_t)stream), "spx_upsample_argext");
}

// ---- full-resolution map operators: evaluation metrics, activation overlap, push bounding boxes, explanation maps ----------
#define SPX_EVAL_MAX_CLASSES 1024
#define SPX_EVAL_MAX_PROTOTYPES 4096
#define SPX_OVL_MAX_SLOTS 32
#define SPX_OVL_MAX_OUT 32768
#define SPX_OVL_MAX_ROWS 16384
#define SPX_OVL_MAX_COLS 1638
#define SPX_PBX_MAX_ROWS (1 << 24)
#define SPX_EXP_MAX_ROWS 65535

static int check_label_bytes(const char* who, int32_t code) {
    if (code != 1 && code != 4 && code != 8) return fail("%s: label byte code %d (1 = uint8, 4 = int32, 8 = int64)", who, code);
    return 0;
}

// strides st = (n, channel, y, x) of a [N, C, h, w] tensor of `noun` ("" = the planes): none negative, and one image within
// 2^31 elements, since the kernels address inside one image with 32-bit offsets
static int check_image_strides(const char* who, const char* noun, const int64_t* st, int32_t C, int32_t h, int32_t w) {
    const char* sep = *noun ? " " : "";
    for (int i = 0; i < 4; ++i)
        if (st[i] < 0) return fail("%s: negative %s%sstride", who, noun, sep);
    if ((long long)(C - 1) * st[1] + (long long)(h - 1) * st[2] + (long long)(w - 1) * st[3] >= (1LL << 31))
        return fail("%s: one %s%simage spans more than 2^31 elements", who, noun, sep);
    return 0;
}

int spx_eval_check_classes(const int32_t* host_classes, int32_t P, int32_t K) {
    if (!host_classes) return fail("spx_eval_check_classes: NULL table");
    if (P < 1 || P > SPX_EVAL_MAX_PROTOTYPES || K < 1 || K > SPX_EVAL_MAX_CLASSES)
        return fail("spx_eval_check_classes: bad sizes (P=%d K=%d; P <= %d, K <= %d)", P, K, SPX_EVAL_MAX_PROTOTYPES, SPX_EVAL_MAX_CLASSES);
    for (int p = 0; p < P; ++p)
        if (host_classes[p] < 0 || host_classes[p] >= K)
            return fail("spx_eval_check_classes: prototype %d has class %d outside [0, %d)", p, host_classes[p], K);
    return 0;
}

static int eval_check(const char* who, const float* logits, const int64_t* lst, const float* dist, const int64_t* dst,
                      int32_t N, int32_t K, int32_t P, int32_t h, int32_t w, int32_t H, int32_t W) {
    if (!logits || !lst) return fail("%s: NULL logits / logit strides", who);
    if (N < 1 || K < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail("%s: empty input (N=%d K=%d h=%d w=%d H=%d W=%d)", who, N, K, h, w, H, W);
    if (K > SPX_EVAL_MAX_CLASSES) return fail("%s: %d classes (at most %d)", who, K, SPX_EVAL_MAX_CLASSES);
    if ((long long)N * H * W >= (1LL << 31) || (long long)h * w >= (1LL << 31)) return fail("%s: maps too large", who);
    if (int e = check_image_strides(who, "logit", lst, K, h, w)) return e;
    if (dist) {
        if (!dst) return fail("%s: NULL distance strides", who);
        if (P < 1 || P > SPX_EVAL_MAX_PROTOTYPES) return fail("%s: %d prototypes (1..%d)", who, P, SPX_EVAL_MAX_PROTOTYPES);
        if (int e = check_image_strides(who, "distance", dst, P, h, w)) return e;
    }
    return 0;
}

int spx_eval_accumulate(const float* logits, const int64_t* host_logit_strides, const float* distances,
                        const int64_t* host_dist_strides, const int32_t* proto_class, const void* labels, int32_t label_bytes,
                        int32_t N, int32_t K, int32_t P, int32_t h, int32_t w, int32_t H, int32_t W, int64_t* conf,
                        int64_t* hits, void* stream) {
    static const char* who = "spx_eval_accumulate";
    if (!labels || !conf) return fail("%s: NULL labels / confusion counters", who);
    if (distances && (!proto_class || !hits)) return fail("%s: distances without prototype classes / hit counters", who);
    if (int e = check_label_bytes(who, label_bytes)) return e;
    if (int e = eval_check(who, logits, host_logit_strides, distances, host_dist_strides, N, K, P, h, w, H, W)) return e;
    return hip_status(spx_launch_eval_accumulate(logits, (const long long*)host_logit_strides, distances,
                                                 (const long long*)host_dist_strides, proto_class, labels, label_bytes, N, K, P,
                                                 h, w, H, W, (unsigned long long*)conf, (unsigned long long*)hits,
                                                 (hipStream_t)stream), who);
}

int spx_eval_topk(const float* logits, const int64_t* host_logit_strides, const float* distances, const int64_t* host_dist_strides,
                  const int32_t* proto_class, const void* samples, int32_t sample_bytes, int32_t N, int32_t S, int32_t K,
                  int32_t P, int32_t h, int32_t w, int32_t H, int32_t W, int64_t* topk, int64_t* seen, void* stream) {
    static const char* who = "spx_eval_topk";
    if (!distances || !proto_class || !samples || !topk) return fail("%s: NULL distances / prototype classes / samples / counters", who);
    if (sample_bytes != 4 && sample_bytes != 8) return fail("%s: sample byte code %d (4 = int32, 8 = int64)", who, sample_bytes);
    // a workgroup's u32 top-k copy grows by at most P per sample: with N*S < 2^24 spread over min(N*S, 256) workgroups it
    // takes at most 2^16 samples, 2^16 * 4096 < 2^32
    if (S < 1 || (long long)N * S >= (1LL << 24)) return fail("%s: bad sample count (N=%d S=%d; N*S < 2^24)", who, N, S);
    if (int e = eval_check(who, logits, host_logit_strides, distances, host_dist_strides, N, K, P, h, w, H, W)) return e;
    return hip_status(spx_launch_eval_topk(logits, (const long long*)host_logit_strides, distances, (const long long*)host_dist_strides,
                                           proto_class, samples, sample_bytes, N, S, K, P, h, w, H, W, (unsigned long long*)topk,
                                           (unsigned long long*)seen, (hipStream_t)stream), who);
}

static int overlap_check(const char* who, const float* planes, const int64_t* st, int32_t N, int32_t C, int32_t h, int32_t w,
                         int32_t H, int32_t W, const void* workspace) {
    if (!planes || !st || !workspace) return fail("%s: NULL planes / strides / workspace", who);
    if (N < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail("%s: empty input (N=%d C=%d h=%d w=%d H=%d W=%d)", who, N, C, h, w, H, W);
    if (N > 65535 || C > SPX_EVAL_MAX_PROTOTYPES) return fail("%s: bad sizes (N=%d C=%d; N <= 65535, C <= %d)", who, N, C, SPX_EVAL_MAX_PROTOTYPES);
    if ((long long)H * W >= (1LL << 31) || H > SPX_OVL_MAX_OUT || W > SPX_OVL_MAX_OUT)
        return fail("%s: output %d x %d too large (H*W < 2^31, H and W <= %d)", who, H, W, SPX_OVL_MAX_OUT);
    if (h > SPX_OVL_MAX_ROWS || w > SPX_OVL_MAX_COLS)
        return fail("%s: latent grid %d x %d too large (h <= %d, w <= %d)", who, h, w, SPX_OVL_MAX_ROWS, SPX_OVL_MAX_COLS);
    return check_image_strides(who, "", st, C, h, w);
}

size_t spx_overlap_workspace_bytes(int32_t N, int32_t C, int32_t K) {
    if (N < 1 || N > 65535 || C < 1 || C > SPX_EVAL_MAX_PROTOTYPES || K < 1 || K > SPX_EVAL_MAX_CLASSES) {
        fail("spx_overlap_workspace_bytes: bad sizes (N=%d C=%d K=%d; N <= 65535, C <= %d, K <= %d)", N, C, K, SPX_EVAL_MAX_PROTOTYPES,
             SPX_EVAL_MAX_CLASSES);
        return 0;
    }
    return spx_overlap_ws_bytes(N, C, K);
}

int spx_overlap_thresholds(const float* planes, const int64_t* host_strides, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H,
                           int32_t W, int64_t k, float gamma, void* workspace, float* thresholds, void* stream) {
    static const char* who = "spx_overlap_thresholds";
    if (!thresholds) return fail("%s: NULL thresholds", who);
    if (int e = overlap_check(who, planes, host_strides, N, C, h, w, H, W, workspace)) return e;
    // 0 < q < 1: the lower order statistic is never the last one, the weight of the upper one is a proper fraction
    const long long HW = (long long)H * W;
    if (k < 0 || k > (HW > 1 ? HW - 2 : 0) || !(gamma >= 0.0f && gamma < 1.0f))
        return fail("%s: rank %lld / weight %g outside a quantile 0 < q < 1 of %lld values", who, (long long)k, (double)gamma, HW);
    return hip_status(spx_launch_overlap_thresholds(planes, (const long long*)host_strides, N, C, h, w, H, W, k, gamma, workspace,
                                                    thresholds, (hipStream_t)stream), who);
}

int spx_overlap_accumulate(const float* planes, const int64_t* host_strides, const float* thresholds, const void* labels,
                           int32_t label_bytes, const int32_t* slot_table, int32_t N, int32_t C, int32_t K, int32_t J, int32_t h,
                           int32_t w, int32_t H, int32_t W, int64_t* inter, int64_t* area, int64_t* images, void* workspace,
                           void* stream) {
    static const char* who = "spx_overlap_accumulate";
    if (!thresholds || !labels || !slot_table || !inter || !area || !images)
        return fail("%s: NULL thresholds / labels / slot table / counters", who);
    if (int e = check_label_bytes(who, label_bytes)) return e;
    if (K < 1 || K > SPX_EVAL_MAX_CLASSES || J < 1 || J > SPX_OVL_MAX_SLOTS)
        return fail("%s: bad sizes (K=%d J=%d; K <= %d, J <= %d)", who, K, J, SPX_EVAL_MAX_CLASSES, SPX_OVL_MAX_SLOTS);
    if (int e = overlap_check(who, planes, host_strides, N, C, h, w, H, W, workspace)) return e;
    return hip_status(spx_launch_overlap_accumulate(planes, (const long long*)host_strides, thresholds, labels, label_bytes, slot_table,
                                                    N, C, K, J, h, w, H, W, (unsigned long long*)inter, (unsigned long long*)area,
                                                    (unsigned long long*)images, workspace, (hipStream_t)stream), who);
}

// what spx_push_boxes and spx_push_boxes_rows check alike; min_class: the lowest class a host row may name
static int push_boxes_check(const char* who, const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes,
                            const int32_t* rows, const int32_t* host_rows, const float* thresholds, int32_t R, int32_t N, int32_t C,
                            int32_t h, int32_t w, int32_t H, int32_t W, int32_t add_margin, const int32_t* rf_boxes, const int32_t* crops,
                            int32_t min_class) {
    if (!labels || !rows || !thresholds || !rf_boxes || !crops) return fail("%s: NULL labels / rows / thresholds / boxes", who);
    if (int e = check_label_bytes(who, label_bytes)) return e;
    if (R < 1 || R > SPX_PBX_MAX_ROWS) return fail("%s: %d rows (1..%d)", who, R, SPX_PBX_MAX_ROWS);
    if (add_margin < 0 || add_margin > SPX_OVL_MAX_OUT) return fail("%s: add_margin %d outside 0..%d", who, add_margin, SPX_OVL_MAX_OUT);
    if (int e = overlap_check(who, planes, host_strides, N, C, h, w, H, W, rows)) return e;
    if (host_rows)
        for (int r = 0; r < R; ++r) {
            const int32_t* q = host_rows + 4 * (size_t)r;
            if (q[0] < 0 || q[0] >= N || q[1] < 0 || q[1] >= C || q[2] < min_class || q[3] < 0 || q[3] >= h * w)
                return fail("%s: row %d = (n %d, c %d, class %d, flat index %d) out of range (N=%d C=%d, class >= %d, h*w=%d)", who, r,
                            q[0], q[1], q[2], q[3], N, C, min_class, h * w);
        }
    return 0;
}

int spx_push_boxes(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                   const int32_t* host_rows, const float* thresholds, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H,
                   int32_t W, int32_t add_margin, int32_t* rf_boxes, int32_t* crops, void* stream) {
    static const char* who = "spx_push_boxes";
    if (int e = push_boxes_check(who, planes, host_strides, labels, label_bytes, rows, host_rows, thresholds, R, N, C, h, w, H, W,
                                 add_margin, rf_boxes, crops, 0))
        return e;
    return hip_status(spx_launch_push_boxes(planes, (const long long*)host_strides, labels, label_bytes, rows, thresholds, 0, R, N, C, h,
                                            w, H, W, add_margin, rf_boxes, crops, (hipStream_t)stream), who);
}

int spx_push_boxes_rows(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                        const int32_t* host_rows, const float* row_thresholds, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w,
                        int32_t H, int32_t W, int32_t add_margin, int32_t* rf_boxes, int32_t* crops, void* stream) {
    static const char* who = "spx_push_boxes_rows";
    if (int e = push_boxes_check(who, planes, host_strides, labels, label_bytes, rows, host_rows, row_thresholds, R, N, C, h, w, H, W,
                                 add_margin, rf_boxes, crops, -1))
        return e;
    return hip_status(spx_launch_push_boxes(planes, (const long long*)host_strides, labels, label_bytes, rows, row_thresholds, 1, R, N, C,
                                            h, w, H, W, add_margin, rf_boxes, crops, (hipStream_t)stream), who);
}

#define SPX_MSK_MAX_ROWS 4096
size_t spx_masked_workspace_bytes(int32_t R) {
    if (R < 1 || R > SPX_MSK_MAX_ROWS) {
        fail("spx_masked_workspace_bytes: %d rows (1..%d)", R, SPX_MSK_MAX_ROWS);
        return 0;
    }
    return spx_masked_ws_bytes(R);
}

int spx_masked_thresholds(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                          const int32_t* host_rows, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W, double q,
                          void* workspace, float* thresholds, void* stream) {
    static const char* who = "spx_masked_thresholds";
    if (!labels || !rows || !thresholds) return fail("%s: NULL labels / rows / thresholds", who);
    if (int e = check_label_bytes(who, label_bytes)) return e;
    if (R < 1 || R > SPX_MSK_MAX_ROWS) return fail("%s: %d rows (1..%d)", who, R, SPX_MSK_MAX_ROWS);
    if (!(q > 0.0 && q < 1.0)) return fail("%s: quantile %g outside 0 < q < 1", who, q);
    if (int e = overlap_check(who, planes, host_strides, N, C, h, w, H, W, workspace)) return e;
    if (host_rows)
        for (int r = 0; r < R; ++r) {
            const int32_t* p = host_rows + 3 * (size_t)r;
            if (p[0] < 0 || p[0] >= N || p[1] < 0 || p[1] >= C || p[2] < 0)
                return fail("%s: row %d = (n %d, c %d, label %d) out of range (N=%d C=%d, label >= 0)", who, r, p[0], p[1], p[2], N, C);
        }
    return hip_status(spx_launch_masked_thresholds(planes, (const long long*)host_strides, labels, label_bytes, rows, R, N, C, h, w, H, W,
                                                   q, workspace, thresholds, (hipStream_t)stream), who);
}

#define SPX_NEAR_MAX_K 64
int spx_patch_majority(const void* labels, int32_t label_bytes, const int32_t* rows, const int32_t* host_rows, int32_t R, int32_t N,
                       int32_t h, int32_t w, int32_t H, int32_t W, int32_t num_labels, int32_t* majority, void* stream) {
    static const char* who = "spx_patch_majority";
    if (!labels || !rows || !majority) return fail("%s: NULL labels / rows / output", who);
    if (int e = check_label_bytes(who, label_bytes)) return e;
    if (R < 1 || R > SPX_PBX_MAX_ROWS) return fail("%s: %d rows (1..%d)", who, R, SPX_PBX_MAX_ROWS);
    if (N < 1 || h < 1 || w < 1 || H < 1 || W < 1) return fail("%s: empty input (N=%d h=%d w=%d H=%d W=%d)", who, N, h, w, H, W);
    if ((long long)H * W >= (1LL << 31) || (long long)h * w >= (1LL << 31) || H > SPX_OVL_MAX_OUT || W > SPX_OVL_MAX_OUT)
        return fail("%s: maps too large (H*W, h*w < 2^31, H and W <= %d)", who, SPX_OVL_MAX_OUT);
    if (num_labels < 1 || num_labels > SPX_EVAL_MAX_CLASSES)
        return fail("%s: %d label values 0..K (K + 1 <= %d: the histogram lives in LDS)", who, num_labels, SPX_EVAL_MAX_CLASSES);
    if (host_rows)
        for (int r = 0; r < R; ++r) {
            const int32_t* p = host_rows + 2 * (size_t)r;
            if (p[0] < 0 || p[0] >= N || p[1] < 0 || p[1] >= h * w)
                return fail("%s: row %d = (n %d, flat index %d) out of range (N=%d h*w=%d)", who, r, p[0], p[1], N, h * w);
        }
    return hip_status(spx_launch_patch_majority(labels, label_bytes, rows, R, N, h, w, H, W, num_labels, majority, (hipStream_t)stream), who);
}

int spx_nearest_protos(const float* distances, const int32_t* queries, const int32_t* host_queries, const uint8_t* include, int32_t Q,
                       int32_t B, int32_t P, int32_t h, int32_t w, int32_t k, int32_t window, int64_t* index, float* value, void* stream) {
    static const char* who = "spx_nearest_protos";
    if (!distances || !queries || !index || !value) return fail("%s: NULL distances / queries / outputs", who);
    if (Q < 1 || Q > SPX_PBX_MAX_ROWS) return fail("%s: %d queries (1..%d)", who, Q, SPX_PBX_MAX_ROWS);
    if (B < 1 || P < 1 || h < 1 || w < 1) return fail("%s: empty input (B=%d P=%d h=%d w=%d)", who, B, P, h, w);
    if ((long long)P * h * w >= (1LL << 31)) return fail("%s: one image's map spans more than 2^31 elements", who);
    if (k < 1 || k > SPX_NEAR_MAX_K) return fail("%s: k %d outside 1..%d", who, k, SPX_NEAR_MAX_K);
    if (window < 0) return fail("%s: negative window", who);
    if (host_queries)
        for (int r = 0; r < Q; ++r) {
            const int32_t* p = host_queries + 3 * (size_t)r;
            if (p[0] < 0 || p[0] >= B || p[1] < 0 || p[1] >= h || p[2] < 0 || p[2] >= w)
                return fail("%s: query %d = (n %d, y %d, x %d) out of range (B=%d h=%d w=%d)", who, r, p[0], p[1], p[2], B, h, w);
        }
    return hip_status(spx_launch_nearest_protos(distances, queries, include, Q, B, P, h, w, k, window, (long long*)index, value,
                                                (hipStream_t)stream), who);
}

// what the three explanation-map entry points check alike
static int explain_check(const char* who, const float* planes, const int64_t* st, const void* labels, int32_t label_bytes,
                         const int32_t* rows, const int32_t* host_rows, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H,
                         int32_t W) {
    if (!labels || !rows || !host_rows) return fail("%s: NULL labels / rows / host rows", who);
    if (int e = check_label_bytes(who, label_bytes)) return e;
    if (R < 1 || R > SPX_EXP_MAX_ROWS) return fail("%s: %d rows (1..%d)", who, R, SPX_EXP_MAX_ROWS);
    return overlap_check(who, planes, st, N, C, h, w, H, W, rows);
}
static int explain_heat_rows(const char* who, const int32_t* host_rows, int32_t R, int32_t N, int32_t C) {
    for (int r = 0; r < R; ++r) {
        const int32_t* q = host_rows + 3 * (size_t)r;
        if (q[0] < 0 || q[0] >= N || q[1] < 0 || q[1] >= C || q[2] < 0)
            return fail("%s: row %d = (n %d, c %d, class %d) out of range (N=%d C=%d, class >= 0)", who, r, q[0], q[1], q[2], N, C);
    }
    return 0;
}

int spx_explain_range(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                      const int32_t* host_rows, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                      void* workspace, void* stream) {
    static const char* who = "spx_explain_range";
    if (!workspace) return fail("%s: NULL workspace", who);
    if (int e = explain_check(who, planes, host_strides, labels, label_bytes, rows, host_rows, R, N, C, h, w, H, W)) return e;
    if (int e = explain_heat_rows(who, host_rows, R, N, C)) return e;
    return hip_status(spx_launch_explain_range(planes, (const long long*)host_strides, labels, label_bytes, rows, R, N, C, h, w, H, W,
                                               workspace, (hipStream_t)stream), who);
}

int spx_explain_heat(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                     const int32_t* host_rows, int32_t R, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                     const void* workspace, uint8_t* heat, float* ranges, void* stream) {
    static const char* who = "spx_explain_heat";
    if (!workspace || !heat || !ranges) return fail("%s: NULL workspace / heat / ranges", who);
    if (int e = explain_check(who, planes, host_strides, labels, label_bytes, rows, host_rows, R, N, C, h, w, H, W)) return e;
    if (int e = explain_heat_rows(who, host_rows, R, N, C)) return e;
    return hip_status(spx_launch_explain_heat(planes, (const long long*)host_strides, labels, label_bytes, rows, R, N, C, h, w, H, W,
                                              workspace, heat, ranges, (hipStream_t)stream), who);
}

int spx_explain_dominant(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                         const int32_t* host_rows, const int32_t* slot_table, const float* weights, int32_t R, int32_t N, int32_t C,
                         int32_t K, int32_t J, int32_t h, int32_t w, int32_t H, int32_t W, uint8_t* dom, void* stream) {
    static const char* who = "spx_explain_dominant";
    if (!slot_table || !dom) return fail("%s: NULL slot table / output", who);
    if (K < 1 || K > SPX_EVAL_MAX_CLASSES || J < 1 || J > SPX_OVL_MAX_SLOTS)
        return fail("%s: bad sizes (K=%d J=%d; K <= %d, J <= %d)", who, K, J, SPX_EVAL_MAX_CLASSES, SPX_OVL_MAX_SLOTS);
    if (int e = explain_check(who, planes, host_strides, labels, label_bytes, rows, host_rows, R, N, C, h, w, H, W)) return e;
    for (int r = 0; r < R; ++r) {
        const int32_t* q = host_rows + 2 * (size_t)r;
        if (q[0] < 0 || q[0] >= N || q[1] < 0 || q[1] >= K)
            return fail("%s: row %d = (n %d, class %d) out of range (N=%d K=%d)", who, r, q[0], q[1], N, K);
    }
    return hip_status(spx_launch_explain_dominant(planes, (const long long*)host_strides, labels, label_bytes, rows, slot_table, weights,
                                                  R, N, C, K, J, h, w, H, W, dom, (hipStream_t)stream), who);
}

// ---- failure cases: label maps with per-image confusion, the failure table, paired heat maps -------------------------------
#define SPX_PRED_MAX_CLASSES 256

int spx_predict_accumulate(const float* logits, const int64_t* host_logit_strides, const void* labels, int32_t label_bytes,
                           const uint8_t* id_map, int32_t N, int32_t K, int32_t h, int32_t w, int32_t H, int32_t W, uint8_t* pred,
                           int64_t* conf, void* stream) {
    static const char* who = "spx_predict_accumulate";
    if (!pred && !conf) return fail("%s: NULL pred and conf: nothing to write", who);
    if (conf && !labels) return fail("%s: NULL labels with confusion counters", who);
    if (labels)
        if (int e = check_label_bytes(who, label_bytes)) return e;
    if (K > SPX_PRED_MAX_CLASSES) return fail("%s: %d classes (at most %d: a prediction is one byte)", who, K, SPX_PRED_MAX_CLASSES);
    if (int e = eval_check(who, logits, host_logit_strides, nullptr, nullptr, N, K, 0, h, w, H, W)) return e;
    return hip_status(spx_launch_predict_accumulate(logits, (const long long*)host_logit_strides, conf ? labels : nullptr, label_bytes,
                                                    id_map, N, K, h, w, H, W, pred, (unsigned long long*)conf, (hipStream_t)stream), who);
}

int spx_failure_table(const int64_t* conf, int32_t N, int32_t K, double threshold, double* iou, int32_t* miss, uint8_t* fail_out,
                      void* stream) {
    static const char* who = "spx_failure_table";
    if (!conf || !iou || !miss || !fail_out) return fail("%s: NULL conf / iou / miss / fail", who);
    if (N < 1 || K < 1) return fail("%s: empty input (N=%d K=%d)", who, N, K);
    if (K > SPX_EVAL_MAX_CLASSES || (long long)N * K >= (1LL << 31))
        return fail("%s: bad sizes (N=%d K=%d; K <= %d, N*K < 2^31)", who, N, K, SPX_EVAL_MAX_CLASSES);
    if (threshold != threshold) return fail("%s: the threshold is NaN", who);
    return hip_status(spx_launch_failure_table((const long long*)conf, N, K, threshold, iou, miss, fail_out, (hipStream_t)stream), who);
}

// what the two paired-map entry points check alike: every field of every row, every slot used, one (image, class) per slot
static int paired_check(const char* who, const float* planes, const int64_t* st, const void* labels, int32_t label_bytes,
                        const int32_t* rows, const int32_t* host_rows, int32_t R, int32_t Q, int32_t N, int32_t C, int32_t h, int32_t w,
                        int32_t H, int32_t W, const void* workspace) {
    if (!workspace) return fail("%s: NULL workspace", who);
    if (int e = explain_check(who, planes, st, labels, label_bytes, rows, host_rows, R, N, C, h, w, H, W)) return e;
    if (Q < 1 || Q > R) return fail("%s: %d range slots for %d rows (1..R)", who, Q, R);
    std::vector<int32_t> first;                                  // host memory, at most 4 Q <= 256 KiB: the first row of each slot
    try {
        first.assign((size_t)Q, -1);
    } catch (...) {
        return fail("%s: out of host memory for the table of %d range slots", who, Q);
    }
    for (int r = 0; r < R; ++r) {
        const int32_t* p = host_rows + 4 * (size_t)r;
        if (p[0] < 0 || p[0] >= N || p[1] < 0 || p[1] >= C || p[2] < 0 || p[3] < 0 || p[3] >= Q)
            return fail("%s: row %d = (n %d, c %d, class %d, slot %d) out of range (N=%d C=%d Q=%d, class >= 0)", who, r, p[0], p[1], p[2],
                        p[3], N, C, Q);
        int32_t& f = first[(size_t)p[3]];
        if (f < 0) f = r;
        else if (host_rows[4 * (size_t)f] != p[0] || host_rows[4 * (size_t)f + 2] != p[2])
            return fail("%s: row %d = (n %d, class %d) shares slot %d with row %d = (n %d, class %d)", who, r, p[0], p[2], p[3], f,
                        host_rows[4 * (size_t)f], host_rows[4 * (size_t)f + 2]);
    }
    for (int q = 0; q < Q; ++q)
        if (first[(size_t)q] < 0) return fail("%s: no row names range slot %d of %d", who, q, Q);
    return 0;
}

int spx_paired_range(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                     const int32_t* host_rows, int32_t R, int32_t Q, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                     void* workspace, void* stream) {
    static const char* who = "spx_paired_range";
    if (int e = paired_check(who, planes, host_strides, labels, label_bytes, rows, host_rows, R, Q, N, C, h, w, H, W, workspace)) return e;
    return hip_status(spx_launch_paired_range(planes, (const long long*)host_strides, labels, label_bytes, rows, R, Q, N, C, h, w, H, W,
                                              workspace, (hipStream_t)stream), who);
}

int spx_paired_heat(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* rows,
                    const int32_t* host_rows, int32_t R, int32_t Q, int32_t N, int32_t C, int32_t h, int32_t w, int32_t H, int32_t W,
                    const void* workspace, uint8_t* heat, float* ranges, void* stream) {
    static const char* who = "spx_paired_heat";
    if (!heat || !ranges) return fail("%s: NULL heat / ranges", who);
    if (int e = paired_check(who, planes, host_strides, labels, label_bytes, rows, host_rows, R, Q, N, C, h, w, H, W, workspace)) return e;
    return hip_status(spx_launch_paired_heat(planes, (const long long*)host_strides, labels, label_bytes, rows, R, Q, N, C, h, w, H, W,
                                             workspace, heat, ranges, (hipStream_t)stream), who);
}

static int kld_check(const char* who, const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t K,
                     const void* out, int pairs) {
    if (!vals || !labels || !out) return fail("%s: NULL buffer", who);
    if (B < 1 || B > 65535 || HW < 1 || K < 1 || J < 1 || J > 16) return fail("%s: bad sizes (B=%d HW=%d K=%d J=%d; J <= 16)", who, B, HW, K, J);
    if ((long long)J * HW >= (1LL << 31)) return fail("%s: J*HW too large", who);
    (void)pairs;        // (the pair and gradient passes tile their per-class tables over class blocks: no K * J * J limit)
    if ((long long)K * J * 12 + (long long)K * 4 + 8 > 60 * 1024) return fail("%s: K*J = %d exceeds the segment tables of the reduction passes", who, K * J);
    return 0;
}

static int kld_check_w(const char* fn, int32_t HW, int32_t W) {
    if (W < 0 || (W > 0 && HW % W != 0)) return fail("%s: W must be 0 or divide HW", fn);
    return 0;
}
int spx_kld_segment_max(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t W, int32_t K,
                        uint32_t* smax_keys, uint32_t* counts, uint32_t* range_keys, void* stream) {
    if (kld_check("spx_kld_segment_max", vals, labels, B, J, HW, K, smax_keys, 0) || kld_check_w("spx_kld_segment_max", HW, W)) return 1;
    return hip_status(spx_launch_kld_max(vals, labels, B, J, HW, W, K, smax_keys, counts, range_keys, (hipStream_t)stream), "spx_kld_segment_max");
}
int spx_kld_segment_sumexp(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t W, int32_t K,
                           const uint32_t* smax_keys, uint64_t* ssum_fx, void* stream) {
    if (kld_check("spx_kld_segment_sumexp", vals, labels, B, J, HW, K, ssum_fx, 0) || !smax_keys) return smax_keys ? 1 : fail("spx_kld_segment_sumexp: NULL smax_keys");
    if (kld_check_w("spx_kld_segment_sumexp", HW, W)) return 1;
    return hip_status(spx_launch_kld_sumexp(vals, labels, B, J, HW, W, K, smax_keys, ssum_fx, (hipStream_t)stream), "spx_kld_segment_sumexp");
}
int spx_kld_segment_lse(const uint32_t* smax_keys, const uint64_t* ssum_fx, int32_t n, float* lse, const uint32_t* range_keys, int32_t HW,
                        double* scale, void* stream) {
    if (!smax_keys || !ssum_fx || !lse) return fail("spx_kld_segment_lse: NULL pointer");
    if (n < 0) return fail("spx_kld_segment_lse: n < 0");
    if (scale && (!range_keys || HW < 1)) return fail("spx_kld_segment_lse: the scale needs range_keys and HW");
    if (n == 0) return 0;
    return hip_status(spx_launch_kld_lse(smax_keys, ssum_fx, n, lse, range_keys, HW, scale, (hipStream_t)stream), "spx_kld_segment_lse");
}
int spx_kld_gram_loss(const int64_t* a_fx, const double* scale, const uint32_t* counts, const uint8_t* pair_ok, int32_t nseg, int32_t K,
                      int32_t J, float* A, float* Cf, double* partials, float* loss, void* stream) {
    if (!a_fx || !scale || !counts || !pair_ok || !A || !Cf || !partials || !loss) return fail("spx_kld_gram_loss: NULL pointer");
    if (nseg < 1 || K < 1 || J < 1 || J > 16 || nseg % K) return fail("spx_kld_gram_loss: bad sizes (nseg=%d K=%d J=%d)", nseg, K, J);
    return hip_status(spx_launch_kld_gram_loss(a_fx, scale, counts, pair_ok, nseg, K, J, A, Cf, partials, loss, (hipStream_t)stream), "spx_kld_gram_loss");
}
int spx_kld_pair_sums(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t W, int32_t K,
                      const float* lse, const double* scale, int64_t* a_fx, void* stream) {
    if (kld_check("spx_kld_pair_sums", vals, labels, B, J, HW, K, a_fx, 1) || !lse || !scale) return (lse && scale) ? 1 : fail("spx_kld_pair_sums: NULL lse / scale");
    if (kld_check_w("spx_kld_pair_sums", HW, W)) return 1;
    return hip_status(spx_launch_kld_pairs(vals, labels, B, J, HW, W, K, lse, scale, a_fx, (hipStream_t)stream), "spx_kld_pair_sums");
}
int spx_kld_backward(const float* vals, const int32_t* labels, int32_t B, int32_t J, int32_t HW, int32_t K,
                     const float* lse, const float* A, const float* Cf, const float* cf_scale, float* grad, void* stream) {
    if (kld_check("spx_kld_backward", vals, labels, B, J, HW, K, grad, 1)) return 1;
    if (!lse || !A || !Cf) return fail("spx_kld_backward: NULL table");
    return hip_status(spx_launch_kld_backward(vals, labels, B, J, HW, K, lse, A, Cf, cf_scale, grad, (hipStream_t)stream), "spx_kld_backward");
}

// ptrs = 0: the workspace query, which needs the sizes only
static int actloss_check(const char* who, const spx_actloss* a, int planes) {
    if (!a) return fail("%s: NULL descriptor", who);
    if (!a->slot_scale) return fail("%s: NULL slot_scale", who);
    if (planes && (!a->vals || !a->labels)) return fail("%s: NULL buffer", who);
    if (a->mode < 0 || a->mode > 2) return fail("%s: mode %d (0 activations, 1 log, 2 linear)", who, a->mode);
    if (a->terms < 1 || a->terms > (SPX_ACT_SPAT | SPX_ACT_SAMPL | SPX_ACT_NORM)) return fail("%s: terms %d", who, a->terms);
    if (a->norm_type != 0 && a->norm_type != 1) return fail("%s: norm_type %d (0 l1, 1 linf)", who, a->norm_type);
    if (a->HW >= (1 << 29)) return fail("%s: HW too large", who);
    // sizes: the domain of the KLD reduction passes
    if (kld_check(who, (const float*)a->slot_scale, a->slot_scale, a->B, a->J, a->HW, a->K, a->slot_scale, 0)) return 1;
    return kld_check_w(who, a->HW, a->W);
}
size_t spx_actloss_workspace_bytes(const spx_actloss* a) {
    if (actloss_check("spx_actloss_workspace_bytes", a, 0)) return 0;
    return spx_actloss_ws_bytes(a->B, a->K, a->J);
}
int spx_actloss_segment_max(const spx_actloss* a, void* workspace, void* stream) {
    if (actloss_check("spx_actloss_segment_max", a, 1)) return 1;
    if (!workspace) return fail("spx_actloss_segment_max: NULL workspace");
    return hip_status(spx_launch_actloss_max(a, workspace, (hipStream_t)stream), "spx_actloss_segment_max");
}
int spx_actloss_segment_sums(const spx_actloss* a, void* workspace, void* stream) {
    if (actloss_check("spx_actloss_segment_sums", a, 1)) return 1;
    if (!workspace) return fail("spx_actloss_segment_sums: NULL workspace");
    return hip_status(spx_launch_actloss_sums(a, workspace, (hipStream_t)stream), "spx_actloss_segment_sums");
}
int spx_actloss_finish(const spx_actloss* a, void* workspace, float* coef, float* out, void* stream) {
    if (actloss_check("spx_actloss_finish", a, 0)) return 1;
    if (!workspace || !coef || !out) return fail("spx_actloss_finish: NULL buffer");
    return hip_status(spx_launch_actloss_finish(a, workspace, coef, out, (hipStream_t)stream), "spx_actloss_finish");
}
int spx_actloss_backward(const spx_actloss* a, const float* coef, const float* g_total, const float* g_terms, float* grad, void* stream) {
    if (actloss_check("spx_actloss_backward", a, 1)) return 1;
    if (!coef || !grad) return fail("spx_actloss_backward: NULL buffer");
    return hip_status(spx_launch_actloss_backward(a, coef, g_total, g_terms, grad, (hipStream_t)stream), "spx_actloss_backward");
}

static int reg_check(const char* who, const spx_reg* r, int ptrs = 1) {
    if (!r) return fail("%s: NULL descriptor", who);
    if (r->terms < 1 || r->terms > 15) return fail("%s: term mask %d (1..15)", who, r->terms);
    if (r->terms & (SPX_REG_ENT | SPX_REG_CEG | SPX_REG_SMAX)) {
        if (ptrs && (!r->wd || !r->row_block || !r->row_local || !r->col_block || !r->col_local || !r->flat_col || !r->block_info || !r->spans))
            return fail("%s: group terms need wd and the group tables", who);
        if (r->U < 1 || r->P < 1 || (long long)r->U * r->P >= (1LL << 31)) return fail("%s: bad group sizes (U=%d P=%d)", who, r->U, r->P);
        if (r->nblocks < 1 || r->nblocks > SPX_GROUP_BLOCKS_MAX) return fail("%s: %d blocks (1..%d)", who, r->nblocks, SPX_GROUP_BLOCKS_MAX);
        if (r->G < 1 || r->G > 16 || r->S < 1 || r->S > 16) return fail("%s: G=%d S=%d (1..16 each)", who, r->G, r->S);
        if ((long long)r->nblocks * r->G > r->U) return fail("%s: %d blocks of %d rows exceed U=%d", who, r->nblocks, r->G, r->U);
        if ((r->terms & SPX_REG_CEG) && r->G < 2) return fail("%s: the group cross entropy needs G >= 2", who);
        if ((r->terms & SPX_REG_SMAX) && r->nspans < 1) return fail("%s: ScaleMax without a non-empty span", who);
    }
    if (r->terms & SPX_REG_L1) {
        if (ptrs && (!r->head || !r->ident)) return fail("%s: L1 needs the head and the identity", who);
        if (r->K < 1 || r->Uh < 1 || (long long)r->K * r->Uh >= (1LL << 31)) return fail("%s: bad head sizes (K=%d Uh=%d)", who, r->K, r->Uh);
    }
    return 0;
}
size_t spx_reg_workspace_bytes(const spx_reg* r) {
    if (reg_check("spx_reg_workspace_bytes", r, 0)) return 0;
    return spx_reg_workspace(*r);
}
int spx_reg_fwd(const spx_reg* r, float* total, float* terms, void* workspace, void* stream) {
    if (reg_check("spx_reg_fwd", r)) return 1;
    if (!total || !terms || !workspace) return fail("spx_reg_fwd: NULL output / workspace");
    return hip_status(spx_launch_reg_fwd(*r, total, terms, workspace, (hipStream_t)stream), "spx_reg_fwd");
}
int spx_reg_bwd(const spx_reg* r, const float* g_total, const float* g_terms, float* d_wd, float* d_head, void* stream) {
    if (reg_check("spx_reg_bwd", r)) return 1;
    if ((r->terms & (SPX_REG_ENT | SPX_REG_CEG | SPX_REG_SMAX)) && !d_wd) return fail("spx_reg_bwd: NULL d_wd");
    if ((r->terms & SPX_REG_L1) && !d_head) return fail("spx_reg_bwd: NULL d_head");
    return hip_status(spx_launch_reg_bwd(*r, g_total, g_terms, d_wd, d_head, (hipStream_t)stream), "spx_reg_bwd");
}

}  // extern "C"

static int scale_agg_check(const char* who, const void* x, int32_t x_dtype, int64_t x_bstride, const float* source, int32_t source_kind,
                           const float* proto, int32_t B, int32_t Cs, int32_t Pn, int32_t HW, int32_t mode) {
    if (!source || !proto) return fail("%s: NULL source / proto", who);
    if (mode != SPX_SAGG_NONE && mode != SPX_SAGG_SUM && mode != SPX_SAGG_MULT) return fail("%s: mode %d (0 none, 1 sum, 2 mult)", who, mode);
    if (source_kind < SPX_SAGG_ACTIVATIONS || source_kind > SPX_SAGG_DIST_LINEAR)
        return fail("%s: source_kind %d (0 activations, 1 distances/log, 2 distances/linear)", who, source_kind);
    if (B < 1 || HW < 1) return fail("%s: empty input (B=%d HW=%d)", who, B, HW);
    if (Pn < 1) return fail("%s: empty scale: the aggregated scale has %d prototypes", who, Pn);
    if (Cs < 16 || Cs % 16) return fail("%s: channels per scale %d must be a positive multiple of 16", who, Cs);
    if ((long long)B * (Cs > Pn ? Cs : Pn) * HW >= (1LL << 40)) return fail("%s: tensor too large", who);
    if (mode != SPX_SAGG_NONE) {
        if (!x) return fail("%s: NULL x (modes sum / mult combine with it)", who);
        if (x_dtype != 0 && x_dtype != 1) return fail("%s: x_dtype %d (0 bf16, 1 fp32)", who, x_dtype);
        if (x_bstride < (int64_t)Cs * HW) return fail("%s: x batch stride %lld below Cs * HW", who, (long long)x_bstride);
    }
    return 0;
}

size_t spx_scale_agg_workspace_bytes(int32_t B, int32_t Cs, int32_t Pn, int32_t HW) {
    if (B < 1 || Cs < 1 || Pn < 1 || HW < 1) return 0;
    return spx_scale_agg_workspace(B, Cs, Pn, HW);
}

int spx_scale_agg_fwd(const void* x, int32_t x_dtype, int64_t x_bstride, const float* source, int32_t source_kind, const float* proto,
                      float* out, int32_t B, int32_t Cs, int32_t Pn, int32_t HW, int32_t mode, float epsilon, void* stream) {
    static const char* who = "spx_scale_agg_fwd";
    if (int e = scale_agg_check(who, x, x_dtype, x_bstride, source, source_kind, proto, B, Cs, Pn, HW, mode)) return e;
    if (!out) return fail("%s: NULL out", who);
    return hip_status(spx_launch_scale_agg_fwd(x, x_dtype == 0, x_bstride, source, source_kind, proto, out, B, Cs, Pn, HW, mode, epsilon,
                                               (hipStream_t)stream), who);
}

int spx_scale_agg_bwd(const void* x, int32_t x_dtype, int64_t x_bstride, const float* source, int32_t source_kind, const float* proto,
                      const float* g, void* dx, float* dsource, float* dproto, void* workspace, int32_t B, int32_t Cs, int32_t Pn,
                      int32_t HW, int32_t mode, float epsilon, void* stream) {
    static const char* who = "spx_scale_agg_bwd";
    if (int e = scale_agg_check(who, x, x_dtype, x_bstride, source, source_kind, proto, B, Cs, Pn, HW, mode)) return e;
    if (!g || !workspace) return fail("%s: NULL g / workspace", who);
    return hip_status(spx_launch_scale_agg_bwd(x, x_dtype == 0, x_bstride, source, source_kind, proto, g, dx, dsource, dproto, workspace,
                                               B, Cs, Pn, HW, mode, epsilon, (hipStream_t)stream), who);
}

// what the part-metric entry points check alike: the maps [N, H, W] and the (class, part) key space
#define SPX_PRT_MAX_PARTS 254
static int parts_maps_check(const char* who, const void* labels, int32_t label_bytes, int32_t N, int32_t K, int32_t M, int32_t H,
                            int32_t W) {
    if (!labels) return fail("%s: NULL labels", who);
    if (int e = check_label_bytes(who, label_bytes)) return e;
    if (N < 1 || N > 65535 || K < 1 || K > SPX_EVAL_MAX_CLASSES)
        return fail("%s: bad sizes (N=%d K=%d; 1 <= N <= 65535, 1 <= K <= %d)", who, N, K, SPX_EVAL_MAX_CLASSES);
    if (M < 1 || M > SPX_PRT_MAX_PARTS) return fail("%s: max_parts %d outside 1..%d", who, M, SPX_PRT_MAX_PARTS);
    if (H < 1 || W < 1 || (long long)H * W >= (1LL << 31) || H > SPX_OVL_MAX_OUT || W > SPX_OVL_MAX_OUT)
        return fail("%s: maps %d x %d (1 <= H, W <= %d, H*W < 2^31)", who, H, W, SPX_OVL_MAX_OUT);
    return 0;
}
static int parts_slots_check(const char* who, const int32_t* slot_table, int32_t J) {
    if (!slot_table) return fail("%s: NULL slot table", who);
    if (J < 1 || J > SPX_OVL_MAX_SLOTS) return fail("%s: %d slots per class (1..%d)", who, J, SPX_OVL_MAX_SLOTS);
    return 0;
}

size_t spx_part_components_workspace_bytes(int32_t N, int32_t H, int32_t W) {
    if (N < 1 || N > 65535 || H < 1 || W < 1 || (long long)H * W >= (1LL << 31)) {
        fail("spx_part_components_workspace_bytes: bad sizes (N=%d H=%d W=%d)", N, H, W);
        return 0;
    }
    return spx_parts_comp_ws_bytes(N, H, W);
}

int spx_part_components(const void* labels, int32_t label_bytes, const void* parts, int32_t part_bytes, int32_t N, int32_t K, int32_t M,
                        int32_t H, int32_t W, void* workspace, uint64_t* totals, void* stream) {
    static const char* who = "spx_part_components";
    if (!parts || !workspace || !totals) return fail("%s: NULL parts / workspace / totals", who);
    if (int e = check_label_bytes(who, part_bytes)) return e;
    if (int e = parts_maps_check(who, labels, label_bytes, N, K, M, H, W)) return e;
    return hip_status(spx_launch_part_components(labels, label_bytes, parts, part_bytes, N, K, M, H, W, workspace,
                                                 (unsigned long long*)totals, (hipStream_t)stream), who);
}

size_t spx_part_thresholds_workspace_bytes(int32_t N, int32_t K, int32_t h, int32_t w) {
    if (N < 1 || N > 65535 || K < 1 || K > SPX_EVAL_MAX_CLASSES || h < 1 || w < 1 || (long long)h * w >= (1LL << 31)) {
        fail("spx_part_thresholds_workspace_bytes: bad sizes (N=%d K=%d h=%d w=%d)", N, K, h, w);
        return 0;
    }
    return spx_parts_thr_ws_bytes(N, K, h, w);
}

int spx_part_thresholds(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const int32_t* slot_table,
                        const uint8_t* skip, int32_t N, int32_t C, int32_t K, int32_t J, int32_t h, int32_t w, int32_t H, int32_t W,
                        double q, int32_t mode, void* workspace, float* thresholds, void* stream) {
    static const char* who = "spx_part_thresholds";
    if (!thresholds) return fail("%s: NULL thresholds", who);
    if (mode != SPX_PART_IMAGE && mode != SPX_PART_NONZERO) return fail("%s: mode %d (0 image, 1 nonzero)", who, mode);
    if (!(q > 0.0 && q < 1.0)) return fail("%s: quantile %g outside 0 < q < 1", who, q);
    if (int e = parts_maps_check(who, labels, label_bytes, N, K, 1, H, W)) return e;
    if (int e = parts_slots_check(who, slot_table, J)) return e;
    if (int e = overlap_check(who, planes, host_strides, N, C, h, w, H, W, workspace)) return e;
    return hip_status(spx_launch_part_thresholds(planes, (const long long*)host_strides, labels, label_bytes, slot_table, skip, N, C, K, J,
                                                 h, w, H, W, q, mode, workspace, thresholds, (hipStream_t)stream), who);
}

int spx_part_presence(const float* planes, const int64_t* host_strides, const void* labels, int32_t label_bytes, const void* parts,
                      int32_t part_bytes, const int32_t* slot_table, const uint8_t* skip, const float* thresholds,
                      const void* comp_workspace, const uint64_t* totals, int32_t N, int32_t C, int32_t K, int32_t J, int32_t M, int32_t h,
                      int32_t w, int32_t H, int32_t W, uint8_t* table, uint8_t* valid, void* stream) {
    static const char* who = "spx_part_presence";
    if (!parts || !thresholds || !totals || !table || !valid) return fail("%s: NULL parts / thresholds / totals / outputs", who);
    if (int e = check_label_bytes(who, part_bytes)) return e;
    if (int e = parts_maps_check(who, labels, label_bytes, N, K, M, H, W)) return e;
    if (int e = parts_slots_check(who, slot_table, J)) return e;
    if (int e = overlap_check(who, planes, host_strides, N, C, h, w, H, W, comp_workspace)) return e;
    return hip_status(spx_launch_part_presence(planes, (const long long*)host_strides, labels, label_bytes, parts, part_bytes, slot_table,
                                               skip, thresholds, comp_workspace, (const unsigned long long*)totals, N, C, K, J, M, h, w, H,
                                               W, table, valid, (hipStream_t)stream), who);
}

static int parts_fold_check(const char* who, const void* a, const void* b, const void* valid, const int32_t* slot_table, const void* counters,
                            int32_t N, int32_t C, int32_t K, int32_t J, int32_t M) {
    if (!a || !b || !valid || !counters) return fail("%s: NULL table / valid flags / counters", who);
    if (int e = parts_slots_check(who, slot_table, J)) return e;
    if (N < 1 || N > 65535 || C < 1 || K < 1 || K > SPX_EVAL_MAX_CLASSES || M < 1 || M > SPX_PRT_MAX_PARTS)
        return fail("%s: bad sizes (N=%d C=%d K=%d max_parts=%d)", who, N, C, K, M);
    return 0;
}

int spx_part_fold_consistency(const uint8_t* table, const uint8_t* valid, const int32_t* slot_table, int32_t N, int32_t C, int32_t K,
                              int32_t J, int32_t M, int64_t* counters, void* stream) {
    static const char* who = "spx_part_fold_consistency";
    if (int e = parts_fold_check(who, table, table, valid, slot_table, counters, N, C, K, J, M)) return e;
    return hip_status(spx_launch_part_fold_consistency(table, valid, slot_table, N, C, K, J, M, (long long*)counters, (hipStream_t)stream), who);
}

int spx_part_fold_stability(const uint8_t* clean, const uint8_t* noisy, const uint8_t* valid, const int32_t* slot_table, int32_t N, int32_t C,
                            int32_t K, int32_t J, int32_t M, int64_t* counters, void* stream) {
    static const char* who = "spx_part_fold_stability";
    if (int e = parts_fold_check(who, clean, noisy, valid, slot_table, counters, N, C, K, J, M)) return e;
    return hip_status(spx_launch_part_fold_stability(clean, noisy, valid, slot_table, N, C, K, J, M, (unsigned long long*)counters,
                                                     (hipStream_t)stream), who);
}

// what the two batch entry points check alike: the sizes, the id table, the grids and their tables, the latent outputs
static int batch_check(const char* who, const spx_batch* a) {
    if (!a) return fail("%s: NULL arguments", who);
    if (!a->index || a->n_index < 1) return fail("%s: NULL or empty index buffer", who);
    if (a->B < 1 || a->B > 65535) return fail("%s: batch %d outside 1..65535", who, a->B);
    if (a->Hc < 1 || a->Wc < 1 || (long long)a->Hc * a->Wc >= (1LL << 31) - 256)
        return fail("%s: window %d x %d (both >= 1, Hc * Wc < 2^31 - 256)", who, a->Hc, a->Wc);
    if (a->L < 0 || (a->L > 0 && !a->id_map) || (a->id_map && a->L < 1))
        return fail("%s: id table of %d entries (NULL with 0, a pointer with L >= 1)", who, a->L);
    if (a->G < 0 || a->G > SPX_BATCH_MAX_GRIDS) return fail("%s: %d latent grids (0..%d)", who, a->G, SPX_BATCH_MAX_GRIDS);
    for (int g = 0; g < a->G; ++g) {
        if (a->grid_h[g] < 1 || a->grid_w[g] < 1 || (long long)a->grid_h[g] * a->grid_w[g] >= (1LL << 31) - 256)
            return fail("%s: latent grid %d is %d x %d", who, g, a->grid_h[g], a->grid_w[g]);
        if (a->grid_rt[g] < 0 || a->grid_ct[g] < 0 || (long long)a->grid_rt[g] + a->grid_h[g] > a->n_index ||
            (long long)a->grid_ct[g] + a->grid_w[g] > a->n_index)
            return fail("%s: the index tables of latent grid %d leave the index buffer", who, g);
        if (!a->latent[g] && !a->latent0[g]) return fail("%s: latent grid %d has no output", who, g);
    }
    return 0;
}

int spx_batch_prepare(const spx_batch* a, void* stream) {
    static const char* who = "spx_batch_prepare";
    if (int e = batch_check(who, a)) return e;
    if (!a->samples) return fail("%s: NULL sample descriptors", who);
    if (!a->image_out && !a->window_labels && a->G == 0) return fail("%s: no output requested", who);
    if (a->image_out) {
        if (a->out_u8 && !a->round_u8) return fail("%s: uint8 output needs round_u8", who);
        for (int c = 0; c < 3; ++c) {
            if (!(a->mean[c] == a->mean[c]) || !(a->std[c] == a->std[c])) return fail("%s: NaN in mean / std", who);
            if (a->normalize && !a->out_u8 && a->std[c] == 0.0f) return fail("%s: std[%d] is zero", who, c);
        }
    }
    return hip_status(spx_launch_batch_prepare(*a, (hipStream_t)stream), who);
}

int spx_resize_labels(const spx_batch* a, void* stream) {
    static const char* who = "spx_resize_labels";
    if (int e = batch_check(who, a)) return e;
    if (!a->labels_in) return fail("%s: NULL labels", who);
    if (a->G < 1) return fail("%s: no latent grid", who);
    const int d = a->labels_dtype;
    if (d != SPX_LABEL_U8 && d != SPX_LABEL_I16 && d != SPX_LABEL_I32 && d != SPX_LABEL_I64)
        return fail("%s: label dtype code %d (1 = uint8, 2 = int16, 4 = int32, 8 = int64)", who, d);
    return hip_status(spx_launch_resize_labels(*a, (hipStream_t)stream), who);
}

// what the two MSC entry points check alike: the maps, their common batch and channel counts, the dtype codes
static int msc_check(const char* who, const spx_msc* a, bool forward) {
    if (!a) return fail("%s: NULL arguments", who);
    if (a->K < 1 || a->K > SPX_MSC_MAX_MAPS) return fail("%s: %d maps (1..%d)", who, a->K, SPX_MSC_MAX_MAPS);
    if (a->B < 1 || a->B > 65535 || a->C < 1) return fail("%s: batch %d (1..65535), channels %d (>= 1)", who, a->B, a->C);
    if ((a->in_dtype | 1) != 1 || (a->out_dtype | 1) != 1) return fail("%s: dtype codes %d / %d (0 = bf16, 1 = fp32)", who, a->in_dtype, a->out_dtype);
    if ((a->activation | 1) != 1) return fail("%s: activation code %d (0 = none, 1 = sigmoid)", who, a->activation);
    for (int k = 0; k < a->K; ++k) {
        const spx_msc_map& m = a->maps[k];
        if (forward && !m.data) return fail("%s: map %d is NULL", who, k);
        if (m.h < 1 || m.w < 1 || (long long)m.h * m.w >= (1LL << 31)) return fail("%s: map %d is %d x %d (both >= 1, h * w < 2^31)", who, k, m.h, m.w);
        if (forward && (m.batch_stride < 0 || m.channel_stride < 0)) return fail("%s: map %d has a negative stride", who, k);
        if (forward && (uintptr_t)m.data % (a->in_dtype == 0 ? 2 : 4)) return fail("%s: map %d is not aligned to its element size", who, k);
    }
    if ((long long)a->B * a->C > ((1LL << 40) - 1) / ((long long)a->maps[0].h * a->maps[0].w)) return fail("%s: B * C * H * W >= 2^40", who);
    if (!a->out && (forward || a->activation == 1)) return fail("%s: NULL output", who);
    if (a->out && (uintptr_t)a->out % (a->out_dtype == 0 ? 2 : 4)) return fail("%s: the output is not aligned to its element size", who);
    return 0;
}

int spx_msc_max_fwd(const spx_msc* a, void* stream) {
    static const char* who = "spx_msc_max_fwd";
    if (int e = msc_check(who, a, true)) return e;
    return hip_status(spx_launch_msc_max_fwd(*a, (hipStream_t)stream), who);
}

// what the two MSC backward entry points check alike: the upstream gradient, the index, the gradient buffers
static int msc_bwd_check(const char* who, const spx_msc* a, bool need_index) {
    if (!a->g) return fail("%s: NULL upstream gradient", who);
    if ((a->g_dtype | 1) != 1) return fail("%s: g_dtype code %d (0 = bf16, 1 = fp32)", who, a->g_dtype);
    if (need_index && !a->index) return fail("%s: NULL index with %d maps", who, a->K);
    const size_t gsz = a->g_dtype == 0 ? 2 : 4, msz = a->in_dtype == 0 ? 2 : 4;
    if ((uintptr_t)a->g % gsz) return fail("%s: the upstream gradient is not aligned to its element size", who);
    long long total = 0;
    for (int k = 0; k < a->K; ++k) {
        if ((uintptr_t)a->grads[k] % msz) return fail("%s: gradient %d is not aligned to its element size", who, k);
        if (!a->grads[k]) continue;
        const long long planes = (long long)a->B * a->C, hw = (long long)a->maps[k].h * a->maps[k].w;
        if (planes > ((1LL << 39) - 1 - total) / hw) return fail("%s: 2^39 or more gradient elements in one launch", who);
        total += planes * hw;
    }
    return 0;
}

int spx_msc_max_bwd(const spx_msc* a, void* stream) {
    static const char* who = "spx_msc_max_bwd";
    if (int e = msc_check(who, a, false)) return e;
    if (int e = msc_bwd_check(who, a, a->K > 1)) return e;
    return hip_status(spx_launch_msc_max_bwd(*a, (hipStream_t)stream), who);
}

// the packed axis: M = sum over the segments of B * h * w below 2^31, C * M below 2^40
static int msc_pack_check(const char* who, const spx_msc* a, int with_max) {
    long long M = 0;
    for (int k = 0; k < a->K + (with_max ? 1 : 0); ++k) {
        const spx_msc_map& m = a->maps[k < a->K ? k : 0];
        M += (long long)a->B * m.h * m.w;                  // (each term below 2^47: msc_check)
    }
    if (M >= (1LL << 31)) return fail("%s: %lld packed pixels (M < 2^31)", who, M);
    if ((long long)a->C > ((1LL << 40) - 1) / M) return fail("%s: C * M >= 2^40", who);
    return 0;
}

int spx_msc_pack_fwd(const spx_msc* a, int with_max, void* stream) {
    static const char* who = "spx_msc_pack_fwd";
    if (int e = msc_check(who, a, true)) return e;
    if (int e = msc_pack_check(who, a, with_max)) return e;
    return hip_status(spx_launch_msc_pack_fwd(*a, with_max, (hipStream_t)stream), who);
}

int spx_msc_pack_bwd(const spx_msc* a, int with_max, void* stream) {
    static const char* who = "spx_msc_pack_bwd";
    if (int e = msc_check(who, a, false)) return e;
    if (int e = msc_pack_check(who, a, with_max)) return e;
    if (int e = msc_bwd_check(who, a, with_max && a->K > 1)) return e;
    return hip_status(spx_launch_msc_pack_bwd(*a, with_max, (hipStream_t)stream), who);
}
