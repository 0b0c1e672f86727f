// Class-restricted activation thresholds (segmentation/analysis/nearest_img.py:292-300, push_multiscale_optimization.py:476-484):
// T = np.percentile(u[labels == L], 100 q) of an activation plane upsampled to the label size, the reference's `threshold_gt`.
// The radix select of spx_overlap_sample.h (ovl_hist_round, ovl_scan_round: a pixel has the same bits here, in the select over
// all pixels and in the crop walk) in its masked form: a round samples and counts only the pixels whose label is L, and because
// their number is known only on the device the ranks are formed there, in float64 as numpy forms them on the host:
//
//   row r = (n, c, L);  count = |{labels[n] == L}|;  virtual = q (count - 1);  k = floor(virtual);  gamma = float(virtual - k),
//   clamped below 1;  k1 = min(k + 1, count - 1);  T = numpy's _lerp(v[k], v[k1], gamma) in fp32;  count == 0: T = +inf.
//
// Workspace per row: the select's state and hist, and count uint32.
// A row out of range (the host entry point refuses it when it is given the table's host copy) gets NaN and reads nothing.
#include "spx_overlap_sample.h"

static inline size_t msk_state_bytes(long long rows) { return (size_t)rows * 16; }
static inline size_t msk_count_bytes(long long rows) { return ((size_t)rows * 4 + 255) & ~(size_t)255; }
static inline size_t msk_hist_bytes(long long rows) { return (size_t)rows * 2 * OVL_BINS * 4; }

__device__ __forceinline__ bool msk_row_ok(const int32_t* __restrict__ rows, size_t row, int N, int C) {
    return ovl_plane_ok(rows[row * 3 + 0], rows[row * 3 + 1], N, C) && rows[row * 3 + 2] >= 0;
}

// (k, gamma) of numpy's linear quantile of `count` >= 1 values, in float64; overlap._rank on the host
__device__ __forceinline__ void msk_rank(double q, uint32_t count, uint32_t& k, uint32_t& k1, float& gamma) {
    const double virt = q * (double)(count - 1u);
    const double fl = floor(virt);
    k = (uint32_t)fl;
    gamma = (float)(virt - fl);
    if (gamma >= 1.0f) gamma = 1.0f - 5.9604644775390625e-08f;       // 1 - 2^-24
    k1 = k + 1u < count ? k + 1u : count - 1u;
}

__global__ __launch_bounds__(OVL_THREADS) void spx_masked_init_kernel(uint32_t* __restrict__ state, uint32_t* __restrict__ count,
                                                                      uint32_t* __restrict__ hist) {
    const size_t row = blockIdx.x;
    ovl_clear_hist(hist + row * 2 * OVL_BINS);
    if (threadIdx.x < 4) state[row * 4 + threadIdx.x] = 0u;
    if (threadIdx.x == 4) count[row] = 0u;
}

// band blockIdx.x of row blockIdx.y, the pixels of the row's class; round 0 also counts them
__global__ __launch_bounds__(OVL_THREADS) void spx_masked_hist_kernel(SpxPlanes a, const void* __restrict__ labels, int label_bytes,
                                                                      const int32_t* __restrict__ rows, int N, int C, int h, int w, int H,
                                                                      int W, int band_rows, int round, const uint32_t* __restrict__ state,
                                                                      uint32_t* __restrict__ count, uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_count;
    const size_t row = blockIdx.y;
    if (!msk_row_ok(rows, row, N, C)) return;                    // workgroup-uniform
    if (round > 0 && count[row] == 0u) return;                   // workgroup-uniform: the class is absent from the image
    const OvlClass cls = {labels, label_bytes, rows[row * 3 + 2], count + row, &s_count};
    ovl_hist_round<true>(a, rows[row * 3 + 0], rows[row * 3 + 1], h, w, H, W, band_rows, round, state + row * 4,
                         hist + row * 2 * OVL_BINS, cls);
}

// row blockIdx.x; the ranks of round 0 are formed here from the row's count.  +inf for an absent class, NaN for a row out of range.
__global__ __launch_bounds__(OVL_THREADS) void spx_masked_scan_kernel(int round, const int32_t* __restrict__ rows, int N, int C, double q,
                                                                      uint32_t* __restrict__ state, const uint32_t* __restrict__ count,
                                                                      uint32_t* __restrict__ hist, float* __restrict__ thresholds) {
    const size_t row = blockIdx.x;
    const bool ok = msk_row_ok(rows, row, N, C);
    const uint32_t cnt_all = ok ? count[row] : 0u;
    if (cnt_all == 0u) {                                         // workgroup-uniform; nothing was counted, the histograms are zero
        if (round == 2 && threadIdx.x == 0) thresholds[row] = ok ? __uint_as_float(0x7f800000u) : __uint_as_float(0x7fc00000u);
        return;
    }
    uint32_t k0, k1;
    float gamma;
    msk_rank(q, cnt_all, k0, k1, gamma);
    uint32_t* st = state + row * 4;
    ovl_scan_round(round, st, hist + row * 2 * OVL_BINS, [&](int r) { return round == 0 ? (r == 0 ? k0 : k1) : st[2 * r + 1]; });
    if (round == 2 && threadIdx.x == 0) thresholds[row] = ovl_lerp(ovl_unkey(st[0]), ovl_unkey(st[2]), gamma);
}

size_t spx_masked_ws_bytes(int R) { return msk_state_bytes(R) + msk_count_bytes(R) + msk_hist_bytes(R); }

hipError_t spx_launch_masked_thresholds(const float* planes, const long long* st, const void* labels, int label_bytes,
                                        const int32_t* rows, int R, int N, int C, int h, int w, int H, int W, double q, void* workspace,
                                        float* thresholds, hipStream_t s) {
    uint32_t* state = (uint32_t*)workspace;
    uint32_t* count = (uint32_t*)((char*)workspace + msk_state_bytes(R));
    uint32_t* hist = (uint32_t*)((char*)workspace + msk_state_bytes(R) + msk_count_bytes(R));
    const int band = ovl_band_plan(h, w, H);
    if (!band) return hipErrorInvalidValue;
    hipLaunchKernelGGL(spx_masked_init_kernel, dim3((unsigned)R), dim3(OVL_THREADS), 0, s, state, count, hist);
    const dim3 grid((unsigned)((H + band - 1) / band), (unsigned)R);
    const SpxPlanes a = spx_planes(planes, st);
    for (int round = 0; round < 3; ++round) {
        hipLaunchKernelGGL(spx_masked_hist_kernel, grid, dim3(OVL_THREADS), 0, s, a, labels, label_bytes, rows, N, C, h, w, H, W, band,
                           round, state, count, hist);
        hipLaunchKernelGGL(spx_masked_scan_kernel, dim3((unsigned)R), dim3(OVL_THREADS), 0, s, round, rows, N, C, q, state, count, hist,
                           thresholds);
    }
    return hipGetLastError();
}
