// Row-wise Euclidean projection onto the simplex {w >= 0, sum w = z}, in place, for every group projection of the model in ONE
// launch (segmentation/utils.py:113-124 projection_simplex_sort, called once per class after every optimizer step of the group
// phase, segmentation/model/module_multiscale_group_train.py:337-338).  The stock formula is about fifteen small launches per
// class; the rows are tiny ([3, 12] per class), so the work is launch latency and nothing else.
//
// One 64-lane workgroup per row, the row in LDS:
//   1. rank      element i goes to place #{j < i: v_j >= v_i} + #{j > i: v_j > v_i} of the descending order (a stable counting
//                rank: a permutation whatever the ties; every lane reads the same v_j, an LDS broadcast)
//   2. prefix    css_k = fp32(sum_{i<=k} u_i) - z with the running sum in float64, added to in index order by ONE lane and
//                rounded per element: torch's CPU cumsum.  Sequential on purpose - a tree would round differently.
//   3. rho       the largest k with u_k - css_k / k > 0 (fp32, IEEE division, no contraction); an integer maximum over lanes
//   4. write     w_i = v_i - theta, theta = css_rho / rho, negative results replaced by 0 (torch.clamp: -0 and NaN pass)
// The result equals projection_simplex_sort on a CPU copy of the row bit for bit.  No atomics; no floating-point reduction across
// lanes.  A row with a NaN is all NaN by the formula (the NaN sorts first, every css is NaN, rho = 0, theta = NaN / 0): it is
// written as NaN without being ranked.  rho = 0 otherwise needs a +inf in the row; theta is then css_1 / 0, as torch gathers it.
#include "spx_args.h"
#include "spx_common.h"

#define SPX_SIMPLEX_THREADS 64

__global__ __launch_bounds__(SPX_SIMPLEX_THREADS) void spx_simplex_kernel(const SpxSimplexArgs a) {
    __shared__ float s_v[SPX_SIMPLEX_MAX_COLS], s_u[SPX_SIMPLEX_MAX_COLS], s_c[SPX_SIMPLEX_MAX_COLS];
    const int lane = threadIdx.x, row = blockIdx.x;
    int lo = 0, hi = a.nblocks;                                 // the block of this row: the last b with row0[b] <= row
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.row0[mid] <= row) lo = mid; else hi = mid;
    }
    const int n = a.cols[lo];
    float* __restrict__ p = a.ptrs[lo] + (size_t)(row - a.row0[lo]) * n;

    bool nan = false;
    for (int i = lane; i < n; i += SPX_SIMPLEX_THREADS) {
        const float x = p[i];
        s_v[i] = x;
        nan |= x != x;
    }
    if (__any(nan)) {                                           // workgroup-uniform: the workgroup is one wave
        for (int i = lane; i < n; i += SPX_SIMPLEX_THREADS) p[i] = __builtin_nanf("");
        return;
    }
    __syncthreads();
    for (int i = lane; i < n; i += SPX_SIMPLEX_THREADS) {
        const float x = s_v[i];
        int r = 0;
        for (int j = 0; j < i; ++j) r += s_v[j] >= x;
        for (int j = i + 1; j < n; ++j) r += s_v[j] > x;
        s_u[r] = x;
    }
    __syncthreads();
    if (lane == 0) {
        double acc = 0.0;
        for (int k = 0; k < n; ++k) {
            acc += (double)s_u[k];
            s_c[k] = (float)acc - a.z;
        }
    }
    __syncthreads();
    int rho = 0;
    for (int k = lane; k < n; k += SPX_SIMPLEX_THREADS)
        if (s_u[k] - s_c[k] / (float)(k + 1) > 0.0f) rho = k + 1;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) rho = max(rho, __shfl_xor(rho, off));
    const float theta = s_c[rho > 0 ? rho - 1 : 0] / (float)rho;
    for (int i = lane; i < n; i += SPX_SIMPLEX_THREADS) {
        const float w = s_v[i] - theta;
        p[i] = w < 0.0f ? 0.0f : w;
    }
}

hipError_t spx_launch_simplex(const SpxSimplexArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(spx_simplex_kernel, dim3((unsigned)a.row0[a.nblocks]), dim3(SPX_SIMPLEX_THREADS), 0, s, a);
    return hipGetLastError();
}
