// The pixel walk, the one-step-ahead fetch and the fixed-order wave reductions of the segment passes over class-gathered
// planes [B, J, HW]: shared by the KLD loss (spx_kld.hip) and the activation losses (spx_actloss.hip).
#pragma once
#include "spx_common.h"
#include <algorithm>
#include <type_traits>

#define SPX_KLD_TABLE_LDS (60 * 1024)      // LDS budget of the per-class tables of the pair and gradient passes (class blocks beyond it)

#define SPX_KLD_MIN_WGS 512      // tile rows shrink (64 -> 32 -> 16) until the reduction passes launch at least this many workgroups
#define SPX_KLD_THREADS 256
#define SPX_KLD_PX_PER_WG 2048
#define SPX_KLD_MAXJ 16
#define SPX_KLD_TILE 64                 // W given: a workgroup's tile (64 x 64 pixels: four 16-column strips of 16 steps of 4 rows)

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int lo = __shfl_xor((int)__double2loint(v), m), hi = __shfl_xor((int)__double2hiint(v), m);
        v += __hiloint2double(hi, lo);
    }
    return v;      // fixed butterfly order: deterministic
}
// Sum over the 64 lanes in a fixed order without the LDS crossbar: four DPP adds leave every lane of a 16-lane row with its
// row's sum, the four row sums are read back and added in row order.  ~8 vector instructions per value, against 12
// ds_bpermute + 6 double adds for the butterfly above: the pair pass publishes 132 such sums per class run.
__device__ __forceinline__ float wave_sum_f32(float v) {
    auto dpp_add = [](float x, auto ctrl) {
        return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xF, 0xF, true));
    };
    v = dpp_add(v, std::integral_constant<int, 0xB1>{});     // quad_perm [1,0,3,2]
    v = dpp_add(v, std::integral_constant<int, 0x4E>{});     // quad_perm [2,3,0,1]
    v = dpp_add(v, std::integral_constant<int, 0x141>{});    // row_half_mirror
    v = dpp_add(v, std::integral_constant<int, 0x140>{});    // row_mirror
    const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 0));
    const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 16));
    const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 32));
    const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 48));
    return ((r0 + r1) + r2) + r3;
}
__device__ __forceinline__ float wave_max_f32(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m));
    return v;
}

// The pixels a wave visits in the reduction passes.  W > 0: the pixels are rows of W and a wave walks DOWN a 16-pixel-wide
// column strip in steps of 16 x 4 pixel blocks (label maps are coherent in both directions; a compact block crosses far
// fewer class boundaries than the same pixels taken along one row).  W == 0: a linear walk.  This lane's pixel of step s is
// first + s*stride (s < nsteps, real for s < nvalid).  The passes keep per-thread partial results while all 64 pixels of a
// step share one class and reduce + publish them (wave butterfly, one LDS integer atomic per entry) only when the class
// changes or the walk ends; steps whose pixels are not all of one class take the per-lane atomic path (spx_segment_walk).
// The J plane values of one pixel, loaded UNCONDITIONALLY (a padded slot re-reads slot J-1, a lane without a pixel reads
// pixel `px_safe`): a load under a per-lane condition becomes its own basic block with a full s_waitcnt in front of
// its use, i.e. one exposed memory round trip per slot instead of one per pixel step (measured: 10 round trips per
// step made the pair-sum pass 170 us for 84 MB).
template <int JT>
__device__ __forceinline__ void spx_kld_load_planes(float (&raw)[JT], const float* __restrict__ v, int J, int HW, int px_safe) {
#pragma unroll
    for (int j = 0; j < JT; ++j) raw[j] = v[(size_t)min(j, J - 1) * HW + px_safe];
}

struct SpxKldWalk {
    int first, stride, nsteps, nvalid;
};
__device__ __forceinline__ SpxKldWalk spx_kld_walk(int HW, int W, int trows, int lane, int wave) {
    SpxKldWalk w;
    if (W > 0) {
        // a step of a wave = a 16-column x 4-row block, the wave walks DOWN its 16-column strip (trows rows: 64 = 16 steps on
        // large maps, fewer on small ones so that the chip fills), the four waves of a workgroup sit side by side.  A compact block lies inside ONE label region far more often
        // than a 64 x 1 row segment does (a 64-pixel row of a map with 16-pixel regions is never of one class; 613 us -> see
        // profiles/EXPERIMENTS.md for the pair pass at 2 Mpx), and every load instruction still moves four whole 64-B pieces.
        const int tiles_x = (W + SPX_KLD_TILE - 1) / SPX_KLD_TILE, H = HW / W;
        const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
        const int col = tx * SPX_KLD_TILE + wave * 16 + (lane & 15), row = ty * trows + (lane >> 4);
        const int hend = min(H, (ty + 1) * trows);
        w.nsteps = (hend - ty * trows + 3) / 4;
        if (tx * SPX_KLD_TILE + wave * 16 >= W) w.nsteps = 0;             // wave-uniform
        w.first = row * W + col;
        w.stride = 4 * W;
        w.nvalid = (col < W && row < hend) ? (hend - row + 3) / 4 : 0;
    } else {
        constexpr int PX_PER_WAVE = SPX_KLD_PX_PER_WG / (SPX_KLD_THREADS / 64);
        const int px0 = blockIdx.x * SPX_KLD_PX_PER_WG + wave * PX_PER_WAVE;
        w.nsteps = px0 < HW ? min(PX_PER_WAVE / 64, (HW - px0 + 63) / 64) : 0;
        w.first = px0 + lane;
        w.stride = 64;
        w.nvalid = w.first < HW ? (HW - w.first + 63) / 64 : 0;
    }
    return w;
}

// One step's inputs of a lane: its pixel's label and J plane values.  Fetched UNCONDITIONALLY (a lane without a pixel at that
// step reads pixel 0 and ignores it) and ONE STEP AHEAD: the label and the planes leave together, and the next step's round
// trip runs under this step's arithmetic - a wave's walk was a chain of two dependent round trips per step (label, then
// planes) with nothing else to issue.
template <int JT>
struct SpxKldStep {
    int c;
    float d[JT];
};
template <int JT>
__device__ __forceinline__ void spx_kld_fetch(SpxKldStep<JT>& o, const float* __restrict__ v, const int32_t* __restrict__ lab,
                                              const SpxKldWalk& w, int step, int J, int HW) {
    const int px = step < w.nvalid ? w.first + step * w.stride : 0;
    o.c = lab[px];
    spx_kld_load_planes(o.d, v, J, HW, px);
}

#define SPX_WALK_INLINE __attribute__((always_inline))       // on every closure handed to spx_segment_walk
// The walk of one wave in the reduction passes, stated once.  (spx_kld_max_kernel, spx_kld_pairs_kernel and
// spx_act_sums_kernel keep a copy of the loop, each with its reason: profiles/segment_walk_summary.md.)  The kernel keeps
// its tables, accumulators and arithmetic and hands in four callables (closures of the kernel, inlined by force: a closure left as a call keeps its captured
// accumulator arrays in memory - profiles/EXPERIMENTS.md):
//   prep(raw, c, ok)   form the step's values of this lane from the planes `raw`, its class c and whether it has one
//   accumulate(okm)    a uniform step: add the step's values to the per-thread partial results (okm: the lanes with a class)
//   lane_path(c)       a mixed step, called on the lanes that have a class: one LDS integer atomic per entry
//   publish(cur)       reduce the partial results of class `cur` over the wave, publish them and reset them
// Classes are relative to `c_lo`, the origin of the workgroup's class block (0 in the passes without class blocks): a pixel
// of a class outside [c_lo, c_lo + K) is a pixel without a class here.
// Lanes without a class (void pixels, lanes past the map) contribute neutral values either way: a step is uniform when
// the lanes that HAVE a class agree on it (void borders and ragged tile edges do not send it down the per-lane path).  A step
// without a class pixel is skipped before its values are formed.
template <int JT, typename Prep, typename Accumulate, typename LanePath, typename Publish>
__device__ __forceinline__ void spx_segment_walk(const float* __restrict__ v, const int32_t* __restrict__ lab, const SpxKldWalk& w, int J,
                                                 int HW, int c_lo, int K, Prep prep, Accumulate accumulate, LanePath lane_path,
                                                 Publish publish) {
    int cur = -1;                                          // class of the partial results (wave-uniform)
    SpxKldStep<JT> nx;
    spx_kld_fetch(nx, v, lab, w, 0, J, HW);
    for (int step = 0; step < w.nsteps; ++step) {
        const SpxKldStep<JT> cs = nx;
        spx_kld_fetch(nx, v, lab, w, step + 1, J, HW);
        const int c = step < w.nvalid ? cs.c - c_lo : -1;
        const bool ok = c >= 0 && c < K;
        const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
        const int c0 = okm ? __builtin_amdgcn_readlane(c, __builtin_ffsll((long long)okm) - 1) : -1;
        const bool uniform = __builtin_amdgcn_ballot_w64(ok && c != c0) == 0;
        if (okm == 0) continue;                            // a step without a class pixel
        prep(cs.d, c, ok);
        if (uniform) {
            if (c0 != cur) {
                if (cur >= 0) publish(cur);
                cur = c0;
            }
            accumulate(okm);
        } else if (ok) {
            lane_path(c);
        }
    }
    if (cur >= 0) publish(cur);
}

// ---- launch geometry of the segment passes (host)
// Rows of a workgroup's tile and the grid (x, y) of the reduction passes.
// rows of a workgroup's tile: 64 (16 steps per wave) on large maps; on small ones (training crops) 32 or 16, so that there
// are enough workgroups to fill the chip.  (Two workgroups per CU are enough since the passes fetch a step ahead: at 2 Mpx
// 64-row tiles = 512 workgroups run the max / sum-exp / pair passes in 27 / 22 / 39 us, 32-row tiles = 1024 in 39 / 25 / 52 -
// half the class-run publishes per pixel; 128-row tiles = 256 workgroups in 35 / 38 / 59.)
static inline int spx_segment_tile_rows(int B, int HW, int W, dim3& grid) {
    int trows = SPX_KLD_TILE;
    grid = dim3((unsigned)((HW + SPX_KLD_PX_PER_WG - 1) / SPX_KLD_PX_PER_WG), (unsigned)B);
    if (W > 0) {
        const int tiles_x = (W + SPX_KLD_TILE - 1) / SPX_KLD_TILE, H = HW / W;
        while (trows > 16 && (long long)B * tiles_x * ((H + trows - 1) / trows) < SPX_KLD_MIN_WGS) trows >>= 1;
        grid.x = (unsigned)(tiles_x * ((H + trows - 1) / trows));
    }
    return trows;
}
// Pixels per workgroup of the gradient passes.
// pixels per workgroup: 2048 on large maps; small maps (training crops) get enough workgroups to fill the chip - a thread
// then takes one pixel instead of walking eight in sequence behind the table set-up (80 -> ~20 us at 10 x 65 x 65)
// (2 Mpx, same box: 512 / 1024 / 2048 / 4096 / 8192 pixels per workgroup = 65 / 51 / 45 / 55 / 82 us)
static inline int spx_segment_px_per_wg(int B, int HW) {
    int ppw = SPX_KLD_PX_PER_WG;
    while (ppw > SPX_KLD_THREADS && (long long)B * ((HW + ppw - 1) / ppw) < 512) ppw >>= 1;
    return ppw;
}
// Classes per class block (grid.z) so that a block's tables of `per_class` bytes each fit `budget` bytes of LDS.
static inline int spx_segment_class_block(int K, size_t per_class, size_t budget) {
    return (int)std::min<size_t>((size_t)K, std::max<size_t>(1, budget / per_class));
}
// The run-time slot count J as the compile-time width JT (J rounded up to a multiple of 4): f(std::integral_constant<int, JT>)
template <typename F>
static inline void spx_dispatch_jt(int J, F f) {
    if (J <= 4) f(std::integral_constant<int, 4>{});
    else if (J <= 8) f(std::integral_constant<int, 8>{});
    else if (J <= 12) f(std::integral_constant<int, 12>{});
    else f(std::integral_constant<int, 16>{});
}
