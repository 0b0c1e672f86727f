// Class-restricted activation thresholds (segmentation/analysis/nearest_img.py:292-300, push_multiscale_optimization.py:476-484):
// T = np.percentile(u[labels == L], 100 q) of an activation plane upsampled to the label size, the reference's `threshold_gt`.
// The select is the one of spx_overlap.hip - the order-preserving key, three histogram rounds of 11 / 11 / 10 key bits over
// values recomputed with ovl_value() (spx_overlap_sample.h: a pixel has the same bits here, in the unmasked select and in the
// crop walk of spx_pushbox.hip) - with two differences: only the pixels whose label is L are counted, and because their number
// is known only on the device the rank is formed there, in float64 as numpy forms it on the host:
//
//   row r = (n, c, L);  count = |{labels[n] == L}|;  virtual = q (count - 1);  k = floor(virtual);  gamma = float(virtual - k),
//   clamped below 1;  k1 = min(k + 1, count - 1);  T = numpy's _lerp(v[k], v[k1], gamma) in fp32;  count == 0: T = +inf.
//
// Workspace per row: state uint32 [4] = (prefix, rank) of the two order statistics, count uint32, hist uint32 [2][OVL_BINS].
// A row out of range (the host entry point refuses it when it is given the table's host copy) gets NaN and reads nothing.
#include "spx_overlap_sample.h"

static inline size_t msk_state_bytes(long long rows) { return (size_t)rows * 16; }
static inline size_t msk_count_bytes(long long rows) { return ((size_t)rows * 4 + 255) & ~(size_t)255; }
static inline size_t msk_hist_bytes(long long rows) { return (size_t)rows * 2 * OVL_BINS * 4; }

__device__ __forceinline__ bool msk_row_ok(const int32_t* __restrict__ rows, size_t row, int N, int C) {
    const int n = rows[row * 3 + 0], c = rows[row * 3 + 1], L = rows[row * 3 + 2];
    return n >= 0 && n < N && c >= 0 && c < C && L >= 0;
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
    uint32_t* hq = hist + row * 2 * OVL_BINS;
    for (int i = threadIdx.x; i < 2 * OVL_BINS; i += OVL_THREADS) hq[i] = 0u;
    if (threadIdx.x < 4) state[row * 4 + threadIdx.x] = 0u;
    if (threadIdx.x == 4) count[row] = 0u;
}

// Histogram round `round` of the band of output rows blockIdx.x of row blockIdx.y: spx_overlap_hist_kernel over the pixels
// whose label is L (the label is read first; a pixel outside the class is not sampled).  Round 0 also counts them.
__global__ __launch_bounds__(OVL_THREADS) void spx_masked_hist_kernel(SpxPlanes a, const void* __restrict__ labels, int label_bytes,
                                                                      const int32_t* __restrict__ rows, int N, int C, int h, int w, int H,
                                                                      int W, int band_rows, int round, const uint32_t* __restrict__ state,
                                                                      uint32_t* __restrict__ count, uint32_t* __restrict__ hist) {
    __shared__ float s_stage[OVL_STAGE];
    __shared__ uint32_t s_hist[2 * OVL_BINS];
    __shared__ int s_oy[OVL_BAND * 4];
    __shared__ float s_wy[OVL_BAND * 4];
    __shared__ uint32_t s_count;
    const int tid = threadIdx.x;
    const size_t row = blockIdx.y;
    if (!msk_row_ok(rows, row, N, C)) return;                    // workgroup-uniform
    const int n = rows[row * 3 + 0], c = rows[row * 3 + 1];
    const long long want = rows[row * 3 + 2];
    if (round > 0 && count[row] == 0u) return;                   // workgroup-uniform: the class is absent from the image
    const int Y0 = blockIdx.x * band_rows, Y1 = min(H, Y0 + band_rows), nrows = Y1 - Y0;
    int i0, i1;
    float t;
    ovl_coord(Y0, h, H, i0, t);
    ovl_coord(Y1 - 1, h, H, i1, t);
    const int lo = ovl_clamp(i0 - 1, h - 1), hi = ovl_clamp(i1 + 2, h - 1);
    const int nstage = (hi - lo + 1) * w;                       // <= OVL_STAGE: ovl_band_rows, checked again at the launch
    for (int i = tid; i < 2 * OVL_BINS; i += OVL_THREADS) s_hist[i] = 0u;
    if (tid == 0) s_count = 0u;
    for (int r = tid; r < nrows; r += OVL_THREADS) ovl_axis(Y0 + r, h, H, lo, w, &s_oy[4 * r], &s_wy[4 * r]);
    const float* src = a.p + (long long)n * a.sn + (long long)c * a.sc;
    for (int i = tid; i < nstage; i += OVL_THREADS) {
        const int y = i / w, x = i - y * w;
        s_stage[i] = src[(long long)(lo + y) * a.sy + (long long)x * a.sx];
    }
    __syncthreads();
    const uint32_t p0 = state[row * 4 + 0], p1 = state[row * 4 + 2];
    const int wave = tid >> 6, lane = tid & 63;
    const size_t label0 = (size_t)n * H * W;
    int cur0 = 0, cur1 = 0;
    uint32_t run0 = 0u, run1 = 0u, mine = 0u;
    for (int X = lane; X < W; X += 64) {
        int ox[4];
        float wx[4];
        ovl_axis(X, w, W, 0, 1, ox, wx);
        for (int r = wave; r < nrows; r += 4) {
            if (spx_label(labels, label_bytes, label0 + (size_t)(Y0 + r) * W + X) != want) continue;
            const uint32_t key = ovl_key(ovl_value(s_stage, &s_oy[4 * r], &s_wy[4 * r], ox, wx));
            if (round == 0) {
                ++mine;
                ovl_count(s_hist, cur0, run0, (int)(key >> 21));
            } else if (round == 1) {
                if ((key >> 21) == p0) ovl_count(s_hist, cur0, run0, (int)((key >> 10) & 2047u));
                if ((key >> 21) == p1) ovl_count(s_hist + OVL_BINS, cur1, run1, (int)((key >> 10) & 2047u));
            } else {
                if ((key >> 10) == p0) ovl_count(s_hist, cur0, run0, (int)(key & 1023u));
                if ((key >> 10) == p1) ovl_count(s_hist + OVL_BINS, cur1, run1, (int)(key & 1023u));
            }
        }
    }
    if (run0) atomicAdd(&s_hist[cur0], run0);
    if (run1) atomicAdd(&s_hist[OVL_BINS + cur1], run1);
    if (mine) atomicAdd(&s_count, mine);
    __syncthreads();
    uint32_t* hq = hist + row * 2 * OVL_BINS;
    for (int i = tid; i < 2 * OVL_BINS; i += OVL_THREADS) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&hq[i], v);
    }
    if (tid == 0 && s_count) atomicAdd(&count[row], s_count);
}

// Between the rounds, one workgroup per row: spx_overlap_scan_kernel with the ranks of round 0 formed here from the row's count.
// After the last round T = numpy's _lerp of the two values; +inf for an absent class, NaN for a row out of range.
__global__ __launch_bounds__(OVL_THREADS) void spx_masked_scan_kernel(int round, const int32_t* __restrict__ rows, int N, int C, double q,
                                                                      uint32_t* __restrict__ state, const uint32_t* __restrict__ count,
                                                                      uint32_t* __restrict__ hist, float* __restrict__ thresholds) {
    __shared__ uint32_t s_sum[OVL_THREADS];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const bool ok = msk_row_ok(rows, row, N, C);
    const uint32_t cnt_all = ok ? count[row] : 0u;
    if (cnt_all == 0u) {                                         // workgroup-uniform; nothing was counted, the histograms are zero
        if (round == 2 && tid == 0) thresholds[row] = ok ? __uint_as_float(0x7f800000u) : __uint_as_float(0x7fc00000u);
        return;
    }
    uint32_t k0, k1;
    float gamma;
    msk_rank(q, cnt_all, k0, k1, gamma);
    const int bits = round == 2 ? 10 : 11, per = (1 << bits) / OVL_THREADS;     // 8 or 4 consecutive bins per thread
    uint32_t* hq = hist + row * 2 * OVL_BINS;
    for (int r = 0; r < 2; ++r) {
        const uint32_t* hr = hq + (round == 0 ? 0 : r * OVL_BINS);              // round 0: one histogram serves both ranks
        uint32_t mine = 0u;
        for (int i = 0; i < per; ++i) mine += hr[tid * per + i];
        s_sum[tid] = mine;
        __syncthreads();
        for (int off = 1; off < OVL_THREADS; off <<= 1) {
            const uint32_t add = tid >= off ? s_sum[tid - off] : 0u;
            __syncthreads();
            s_sum[tid] += add;
            __syncthreads();
        }
        const uint32_t rank = round == 0 ? (r == 0 ? k0 : k1) : state[row * 4 + 2 * r + 1];
        uint32_t below = s_sum[tid] - mine;
        __syncthreads();                                                         // every thread has read its rank and sums
        if (rank >= below && rank < below + mine) {                              // exactly one thread
            int b = tid * per;
            for (;; ++b) {
                const uint32_t cnt = hr[b];
                if (rank < below + cnt) break;
                below += cnt;
            }
            state[row * 4 + 2 * r] = (state[row * 4 + 2 * r] << bits) | (uint32_t)b;
            state[row * 4 + 2 * r + 1] = rank - below;
        }
        __syncthreads();
    }
    for (int i = tid; i < 2 * OVL_BINS; i += OVL_THREADS) hq[i] = 0u;
    if (round == 2 && tid == 0) {
        const float lo = ovl_unkey(state[row * 4 + 0]), hi = ovl_unkey(state[row * 4 + 2]);
        const float d = hi - lo;
        thresholds[row] = gamma >= 0.5f ? hi - d * (1.0f - gamma) : lo + d * gamma;
    }
}

size_t spx_masked_ws_bytes(int R) { return msk_state_bytes(R) + msk_count_bytes(R) + msk_hist_bytes(R); }

hipError_t spx_launch_masked_thresholds(const float* planes, const long long* st, const void* labels, int label_bytes,
                                        const int32_t* rows, int R, int N, int C, int h, int w, int H, int W, double q, void* workspace,
                                        float* thresholds, hipStream_t s) {
    uint32_t* state = (uint32_t*)workspace;
    uint32_t* count = (uint32_t*)((char*)workspace + msk_state_bytes(R));
    uint32_t* hist = (uint32_t*)((char*)workspace + msk_state_bytes(R) + msk_count_bytes(R));
    const int band = ovl_band_rows(h, w, H);
    if (band < 1 || (long long)ovl_max_staged_rows(h, H, band) * w > OVL_STAGE) return hipErrorInvalidValue;
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
