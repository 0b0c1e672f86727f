// The two small kernels of the nearest-image / nearest-prototype analysis (segmentation/analysis/nearest_img.py:258-264,
// nearest_proto.py:54-66).
//
//   spx_patch_majority   row (n, flat latent index f): the most frequent label of labels[n][h0:h1, w0:w1], the float64 patch box
//                        of spx_pushbox.hip clipped as a NumPy slice clips it: np.bincount(...).argmax(), the smallest label on
//                        a tie.  One workgroup per row, the histogram in LDS.
//   spx_nearest_protos   query (n, y, x): the k prototypes with the smallest distances[n, :, y, x] in ascending (distance,
//                        prototype) order.  One wave per query; every round takes the wave-wide minimum of the 64-bit words
//                        (order-preserving key of the distance << 32 | prototype) above the word taken last.
#include "spx_overlap_sample.h"

#define NEAR_THREADS 256
#define NEAR_MAX_BINS 1024

__global__ __launch_bounds__(NEAR_THREADS) void spx_patch_majority_kernel(const void* __restrict__ labels, int label_bytes,
                                                                          const int32_t* __restrict__ rows, int N, int h, int w, int H,
                                                                          int W, int bins, int32_t* __restrict__ majority) {
    __shared__ uint32_t s_hist[NEAR_MAX_BINS];
    __shared__ unsigned long long s_best[NEAR_THREADS / 64];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const int n = rows[row * 2 + 0], f = rows[row * 2 + 1];
    if (n < 0 || n >= N || f < 0 || f >= h * w) {                // workgroup-uniform
        if (tid == 0) majority[row] = -1;
        return;
    }
    for (int i = tid; i < bins; i += NEAR_THREADS) s_hist[i] = 0u;
    __syncthreads();
    const double ph = (double)H / (double)h, pw = (double)W / (double)w;
    const int pi = f / w, pj = f - pi * w;
    const int h0 = (int)((double)pi * ph), h1 = min((int)((double)pi * ph + ph) + 1, H);     // h0 < H, w0 < W: pi < h, pj < w
    const int w0 = (int)((double)pj * pw), w1 = min((int)((double)pj * pw + pw) + 1, W);
    const int bw = w1 - w0, cells = (h1 - h0) * bw;
    const size_t label0 = (size_t)n * H * W;
    for (int i = tid; i < cells; i += NEAR_THREADS) {
        const int y = i / bw, x = i - y * bw;
        const long long v = spx_label(labels, label_bytes, label0 + (size_t)(h0 + y) * W + (w0 + x));
        if (v >= 0 && v < bins) atomicAdd(&s_hist[(int)v], 1u);
    }
    __syncthreads();
    // the largest (count, bins - 1 - label): the highest count, the smallest label among equals
    unsigned long long best = 0ull;
    for (int i = tid; i < bins; i += NEAR_THREADS) {
        const unsigned long long word = ((unsigned long long)s_hist[i] << 32) | (unsigned)(bins - 1 - i);
        best = word > best ? word : best;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long other = __shfl_xor(best, off);
        best = other > best ? other : best;
    }
    if ((tid & 63) == 0) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < NEAR_THREADS / 64; ++v) best = s_best[v] > best ? s_best[v] : best;
        majority[row] = bins - 1 - (int)(best & 0xffffffffull);
    }
}

hipError_t spx_launch_patch_majority(const void* labels, int label_bytes, const int32_t* rows, int R, int N, int h, int w, int H, int W,
                                     int bins, int32_t* majority, hipStream_t s) {
    hipLaunchKernelGGL(spx_patch_majority_kernel, dim3((unsigned)R), dim3(NEAR_THREADS), 0, s, labels, label_bytes, rows, N, h, w, H, W,
                       bins, majority);
    return hipGetLastError();
}

// window == 0: the k nearest among the included prototypes (all of them without a mask).  window > 0, the reference's rule
// (nearest_proto.py:61-63): the `window` nearest of ALL prototypes, of which the included ones are kept, k at the most.
__global__ __launch_bounds__(NEAR_THREADS) void spx_nearest_protos_kernel(const float* __restrict__ distances,
                                                                          const int32_t* __restrict__ queries,
                                                                          const uint8_t* __restrict__ include, int Q, int B, int P, int h,
                                                                          int w, int k, int window, long long* __restrict__ index,
                                                                          float* __restrict__ value) {
    const int lane = threadIdx.x & 63;
    const long long query = (long long)blockIdx.x * (NEAR_THREADS / 64) + (threadIdx.x >> 6);
    if (query >= Q) return;                                      // wave-uniform; no barrier follows
    const int n = queries[query * 3 + 0], y = queries[query * 3 + 1], x = queries[query * 3 + 2];
    const bool ok = n >= 0 && n < B && y >= 0 && y < h && x >= 0 && x < w;
    const size_t hw = (size_t)h * w;
    const float* col = distances + ((size_t)(ok ? n : 0) * P) * hw + (size_t)(ok ? y : 0) * w + (ok ? x : 0);
    const bool filter_late = window > 0;
    const int rounds = !ok ? 0 : (filter_late ? min(window, P) : P);
    const unsigned long long none = ~0ull;
    unsigned long long last = 0ull;
    bool first = true;
    int emitted = 0;
    for (int round = 0; round < rounds && emitted < k; ++round) {
        unsigned long long best = none;
        for (int p = lane; p < P; p += 64) {
            if (!filter_late && include && !include[p]) continue;
            const unsigned long long word = ((unsigned long long)ovl_key(col[(size_t)p * hw]) << 32) | (unsigned)p;
            if ((first || word > last) && word < best) best = word;
        }
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long other = __shfl_xor(best, off);
            best = other < best ? other : best;
        }
        if (best == none) break;                                 // wave-uniform: every candidate is taken
        last = best;
        first = false;
        const int p = (int)(best & 0xffffffffull);
        if (!filter_late || !include || include[p]) {
            if (lane == 0) {
                index[query * k + emitted] = p;
                value[query * k + emitted] = ovl_unkey((uint32_t)(best >> 32));
            }
            ++emitted;
        }
    }
    for (int i = emitted + lane; i < k; i += 64) {
        index[query * k + i] = -1;
        value[query * k + i] = __uint_as_float(0x7f800000u);
    }
}

hipError_t spx_launch_nearest_protos(const float* distances, const int32_t* queries, const uint8_t* include, int Q, int B, int P, int h,
                                     int w, int k, int window, long long* index, float* value, hipStream_t s) {
    const int per = NEAR_THREADS / 64;
    hipLaunchKernelGGL(spx_nearest_protos_kernel, dim3((unsigned)((Q + per - 1) / per)), dim3(NEAR_THREADS), 0, s, distances, queries,
                       include, Q, B, P, h, w, k, window, index, value);
    return hipGetLastError();
}
