// Activation-overlap metrics (segmentation/analysis/prototype_overlap.py:28-92, group_overlap.py:28-87): every activation
// plane of a class is upsampled to the label size (OpenCV INTER_CUBIC), thresholded at its own q-quantile, and the
// intersections of the binary masks of one class's planes are counted.  The upsampled [C, H, W] tensor (1.9 GB per Cityscapes
// image) is never written: every pass recomputes a pixel's value from the latent plane with ovl_value() (spx_overlap_sample.h),
// and because that is ONE function compiled with -ffp-contract=off the value of a pixel is the same bits in every pass - the
// selection that finds the threshold and the comparison that builds the mask agree on every pixel.
//
//   spx_overlap_thresholds   the radix select of spx_overlap_sample.h for the order statistics v[k], v[k1] of every plane over
//                            all its pixels, the ranks given by the host; T = numpy's _lerp(v[k], v[k1], gamma) in fp32.
//   spx_overlap_accumulate   class presence from the labels, then per (image, present class, pixel tile): one ballot per
//                            slot, popcount(b_j & b_j') per slot pair (j == j': the mask's area), 64-bit integer atomics.
#include "spx_overlap_sample.h"

#define OVL_MAX_J 32
#define OVL_MAX_PAIRS (OVL_MAX_J * (OVL_MAX_J + 1) / 2)
#define OVL_PAIR_REGS ((OVL_MAX_PAIRS + 63) / 64)
#define OVL_CNT_ROWS 64           // output rows of a counting tile (64 columns wide): 16 per wave

// ---- selection -------------------------------------------------------------------------------------------------------
// Workspace: state uint32 [N*C][4], hist uint32 [N*C][2][OVL_BINS] (the select's, per plane); presence int32 [N][K].  Nothing
// depends on H or W.
static inline size_t ovl_state_bytes(long long planes) { return (size_t)planes * 16; }
static inline size_t ovl_hist_bytes(long long planes) { return (size_t)planes * 2 * OVL_BINS * 4; }

__global__ __launch_bounds__(OVL_THREADS) void spx_overlap_init_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                                                                       uint32_t k0, uint32_t k1) {
    const size_t plane = blockIdx.x;
    ovl_clear_hist(hist + plane * 2 * OVL_BINS);
    if (threadIdx.x == 0) {
        state[plane * 4 + 0] = 0u;
        state[plane * 4 + 1] = k0;
        state[plane * 4 + 2] = 0u;
        state[plane * 4 + 3] = k1;
    }
}

// band blockIdx.x of plane (blockIdx.z, blockIdx.y), every pixel
__global__ __launch_bounds__(OVL_THREADS) void spx_overlap_hist_kernel(SpxPlanes a, int C, int h, int w, int H, int W, int band_rows,
                                                                       int round, const uint32_t* __restrict__ state,
                                                                       uint32_t* __restrict__ hist) {
    const int c = blockIdx.y, n = blockIdx.z;
    const size_t plane = (size_t)n * C + c;
    ovl_hist_round<false>(a, n, c, h, w, H, W, band_rows, round, state + plane * 4, hist + plane * 2 * OVL_BINS, OvlClass{});
}

// plane blockIdx.x; the ranks are in the state from the start
__global__ __launch_bounds__(OVL_THREADS) void spx_overlap_scan_kernel(int round, uint32_t* __restrict__ state, uint32_t* __restrict__ hist,
                                                                       float gamma, float* __restrict__ thresholds) {
    const size_t plane = blockIdx.x;
    uint32_t* st = state + plane * 4;
    ovl_scan_round(round, st, hist + plane * 2 * OVL_BINS, [&](int r) { return st[2 * r + 1]; });
    if (round == 2 && threadIdx.x == 0) thresholds[plane] = ovl_lerp(ovl_unkey(st[0]), ovl_unkey(st[2]), gamma);
}

size_t spx_overlap_ws_bytes(int N, int C, int K) {
    const long long planes = (long long)N * C;
    return ovl_state_bytes(planes) + ovl_hist_bytes(planes) + (((size_t)N * K * 4 + 255) & ~(size_t)255);
}

hipError_t spx_launch_overlap_thresholds(const float* planes, const long long* st, int N, int C, int h, int w, int H, int W,
                                         long long k, float gamma, void* workspace, float* thresholds, hipStream_t s) {
    const long long np = (long long)N * C, HW = (long long)H * W;
    uint32_t* state = (uint32_t*)workspace;
    uint32_t* hist = (uint32_t*)((char*)workspace + ovl_state_bytes(np));
    const long long k1 = k + 1 < HW ? k + 1 : HW - 1;
    const int band = ovl_band_plan(h, w, H);
    if (!band) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spx_overlap_init_kernel, dim3((unsigned)np), dim3(OVL_THREADS), 0, s, state, hist, (uint32_t)k, (uint32_t)k1);
    const dim3 grid((unsigned)((H + band - 1) / band), (unsigned)C, (unsigned)N);
    const SpxPlanes a = spx_planes(planes, st);
    for (int round = 0; round < 3; ++round) {
        hipLaunchKernelGGL(spx_overlap_hist_kernel, grid, dim3(OVL_THREADS), 0, s, a, C, h, w, H, W, band, round, state, hist);
        hipLaunchKernelGGL(spx_overlap_scan_kernel, dim3((unsigned)np), dim3(OVL_THREADS), 0, s, round, state, hist, gamma, thresholds);
    }
    return hipGetLastError();
}

// ---- counting --------------------------------------------------------------------------------------------------------

// presence[n][k] = 1 where class k (label k + 1) occurs in image n; presence is zeroed before the launch
__global__ __launch_bounds__(OVL_THREADS) void spx_overlap_presence_kernel(const void* __restrict__ labels, int label_bytes, int K,
                                                                           long long HW, int32_t* __restrict__ presence) {
    __shared__ int s_seen[1024];
    const int tid = threadIdx.x, n = blockIdx.y;
    for (int i = tid; i < K; i += OVL_THREADS) s_seen[i] = 0;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * OVL_THREADS + tid; i < HW; i += (long long)gridDim.x * OVL_THREADS) {
        const long long ann = spx_label(labels, label_bytes, (size_t)n * HW + i);
        if (ann >= 1 && ann <= K) s_seen[ann - 1] = 1;
    }
    __syncthreads();
    for (int i = tid; i < K; i += OVL_THREADS)
        if (s_seen[i]) presence[(size_t)n * K + i] = 1;
}

// One tile of 64 columns x OVL_CNT_ROWS rows of image blockIdx.z for class blockIdx.y; a workgroup of an absent class leaves
// at once.  Lane l owns column l of the tile, wave v the rows v, v + 4, ...; per row and slot one ballot of (u > T), kept in
// LDS (every lane writes the same word); then lane l adds popcount(b_j & b_j') of the pairs l, l + 64, ... (j <= j' in
// row-major order; j == j' is the area) to its registers.  Rows without any pixel above a threshold (most of them at
// q = 0.95) skip the pairs.
__global__ __launch_bounds__(OVL_THREADS) void spx_overlap_count_kernel(
    SpxPlanes a, const float* __restrict__ thresholds, const int32_t* __restrict__ table, const int32_t* __restrict__ presence, int C,
    int K, int J, int h, int w, int H, int W, int tiles_x, unsigned long long* __restrict__ inter, unsigned long long* __restrict__ area,
    unsigned long long* __restrict__ images) {
    __shared__ unsigned long long s_b[4][OVL_MAX_J];
    __shared__ unsigned short s_pair[OVL_MAX_PAIRS];
    __shared__ int s_ch[OVL_MAX_J];
    __shared__ float s_T[OVL_MAX_J];
    const int tid = threadIdx.x, k = blockIdx.y, n = blockIdx.z;
    if (!presence[(size_t)n * K + k]) return;                    // workgroup-uniform
    if (blockIdx.x == 0 && tid == 0) atomicAdd(&images[k], 1ull);
    const int npairs = J * (J + 1) / 2;
    for (int p = tid; p < npairs; p += OVL_THREADS) {
        int j = 0, rem = p;
        while (rem >= J - j) {
            rem -= J - j;
            ++j;
        }
        s_pair[p] = (unsigned short)(j | ((j + rem) << 8));
    }
    if (tid < J) {
        const int ch = table[(size_t)k * J + tid];
        const bool ok = ch >= 0 && ch < C;                       // anything else: the class has no such slot
        s_ch[tid] = ok ? ch : -1;
        s_T[tid] = ok ? thresholds[(size_t)n * C + ch] : 0.0f;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int X = tx * 64 + lane;
    const bool col_ok = X < W;
    int ox[4], oy[4];
    float wx[4], wy[4];
    ovl_axis(col_ok ? X : W - 1, w, W, 0, (int)a.sx, ox, wx);
    const float* img = a.p + (long long)n * a.sn;
    uint32_t acc[OVL_PAIR_REGS];
#pragma unroll
    for (int i = 0; i < OVL_PAIR_REGS; ++i) acc[i] = 0u;
    const int Yend = min(H, (ty + 1) * OVL_CNT_ROWS);
    for (int Y = ty * OVL_CNT_ROWS + wave; Y < Yend; Y += 4) {
        ovl_axis(Y, h, H, 0, (int)a.sy, oy, wy);
        unsigned long long any = 0ull;
        for (int j = 0; j < J; ++j) {
            const int ch = s_ch[j];
            unsigned long long b = 0ull;
            if (ch >= 0) {                                       // wave-uniform
                const float v = ovl_value(img + (long long)ch * a.sc, oy, wy, ox, wx);
                b = __ballot(col_ok && v > s_T[j]);
            }
            s_b[wave][j] = b;
            any |= b;
        }
        if (any) {
#pragma unroll
            for (int i = 0; i < OVL_PAIR_REGS; ++i) {
                const int p = lane + 64 * i;
                if (p < npairs) {
                    const unsigned pr = s_pair[p];
                    acc[i] += (uint32_t)__popcll(s_b[wave][pr & 255u] & s_b[wave][pr >> 8]);
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < OVL_PAIR_REGS; ++i) {
        const int p = lane + 64 * i;
        if (p < npairs && acc[i]) {
            const unsigned pr = s_pair[p];
            const int j = (int)(pr & 255u), j2 = (int)(pr >> 8);
            if (j == j2) atomicAdd(&area[(size_t)k * J + j], (unsigned long long)acc[i]);
            else atomicAdd(&inter[((size_t)k * J + j) * J + j2], (unsigned long long)acc[i]);
        }
    }
}

hipError_t spx_launch_overlap_accumulate(const float* planes, const long long* st, const float* thresholds, const void* labels,
                                         int label_bytes, const int32_t* table, int N, int C, int K, int J, int h, int w, int H, int W,
                                         unsigned long long* inter, unsigned long long* area, unsigned long long* images,
                                         void* workspace, hipStream_t s) {
    const long long np = (long long)N * C, HW = (long long)H * W;
    int32_t* presence = (int32_t*)((char*)workspace + ovl_state_bytes(np) + ovl_hist_bytes(np));
    hipError_t e = hipMemsetAsync(presence, 0, (size_t)N * K * 4, s);
    if (e != hipSuccess) return e;
    const long long chunks = (HW + OVL_THREADS * 16 - 1) / (OVL_THREADS * 16);
    hipLaunchKernelGGL(spx_overlap_presence_kernel, dim3((unsigned)(chunks < 1024 ? chunks : 1024), (unsigned)N), dim3(OVL_THREADS), 0, s,
                       labels, label_bytes, K, HW, presence);
    const int tiles_x = (W + 63) / 64, tiles_y = (H + OVL_CNT_ROWS - 1) / OVL_CNT_ROWS;
    hipLaunchKernelGGL(spx_overlap_count_kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)K, (unsigned)N), dim3(OVL_THREADS), 0, s,
                       spx_planes(planes, st), thresholds, table, presence, C, K, J, h, w, H, W, tiles_x, inter, area, images);
    return hipGetLastError();
}
