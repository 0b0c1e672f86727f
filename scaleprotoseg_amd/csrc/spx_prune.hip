// Prototype pruning: the k nearest training patches of every prototype (find_nearest.py:88-225 with full_save=True, as
// prune.py:22-30 calls it) without the per-image copy of the distance map to the host.
//   spx_prune_argmin_kernel     void-masked per-prototype minimum of a distance map already in HBM (:118-142)
//   spx_prune_footprint_kernel  the winner's footprint box in the full-resolution label and its label (:145-158, :206-213)
//   spx_prune_merge_kernel      the running [P, k] nearest table, B new images per launch (:222-225)
// The fused variant of the first step (features in, no map written) is the prune mode of the fused push epilogue in
// spx_fwd_impl.h.  Both produce the same 64-bit key per (image, prototype):
//   bits 63..32  float bits of d | void << 31   (d >= 0: the bits order as the value; a void pixel ranks after every
//                                                non-void one, as d + 1e7 does in the reference's float64 map)
//   bits 31..0   flat latent index i*W + j     (lowest on ties: np.argmin's first occurrence)
// so that the minimum is one integer minimum and run-to-run identical.
#include "spx_common.h"

#define SPX_PRUNE_PB 8          // prototype rows per workgroup of the map reduction
#define SPX_PRUNE_CHUNK 4096    // pixels per workgroup of the map reduction
#define SPX_PRUNE_BINS 1024     // LDS histogram of the footprint mode: labels -1 .. 1022; others are counted pairwise

__device__ __forceinline__ uint32_t prune_dist_key(float d, bool is_void) {
    // + 0.0f: -0.0 and +0.0 get one key; fmaxf(d, 0) maps NaN to 0 (the distance kernel's relu does the same)
    return __float_as_uint(fmaxf(d, 0.0f) + 0.0f) | (is_void ? 0x80000000u : 0u);
}

// grid (chunks, ceil(P / PB), B), 256 threads.  A thread reads each label once for PB rows.
__global__ __launch_bounds__(256) void spx_prune_argmin_kernel(const float* __restrict__ dist, const int32_t* __restrict__ labels,
                                                               int void_label, int P, int HW,
                                                               unsigned long long* __restrict__ keys) {
    __shared__ unsigned long long s_min[4][SPX_PRUNE_PB];
    const int p0 = blockIdx.y * SPX_PRUNE_PB, b = blockIdx.z, tid = threadIdx.x;
    const int32_t* lab = labels + (size_t)b * HW;
    const float* rows[SPX_PRUNE_PB];
#pragma unroll
    for (int pp = 0; pp < SPX_PRUNE_PB; ++pp) rows[pp] = dist + ((size_t)b * P + min(p0 + pp, P - 1)) * HW;
    unsigned long long best[SPX_PRUNE_PB];
#pragma unroll
    for (int pp = 0; pp < SPX_PRUNE_PB; ++pp) best[pp] = ~0ull;
    const int begin = blockIdx.x * SPX_PRUNE_CHUNK;
    const int end = min(begin + SPX_PRUNE_CHUNK, HW);
    for (int i = begin + tid; i < end; i += 256) {
        const bool v = lab[i] == void_label;
#pragma unroll
        for (int pp = 0; pp < SPX_PRUNE_PB; ++pp) {
            const unsigned long long key = ((unsigned long long)prune_dist_key(rows[pp][i], v) << 32) | (uint32_t)i;
            best[pp] = key < best[pp] ? key : best[pp];
        }
    }
#pragma unroll
    for (int pp = 0; pp < SPX_PRUNE_PB; ++pp) {
        unsigned long long m = best[pp];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const unsigned long long o = shfl_xor_u64(m, s);
            m = o < m ? o : m;
        }
        if ((tid & 63) == 0) s_min[tid >> 6][pp] = m;
    }
    __syncthreads();
    if (tid < SPX_PRUNE_PB && p0 + tid < P) {
        unsigned long long v = s_min[0][tid];
        for (int w = 1; w < 4; ++w) v = s_min[w][tid] < v ? s_min[w][tid] : v;
        atomicMin(keys + (size_t)b * P + p0 + tid, v);
    }
}

// One workgroup per (prototype, image): grid (P, B), 256 threads.  Box in float64 exactly as find_nearest.py:145-158
// writes it (patch_height = Hf / H; int(i * patch_height), int((i + 1) * patch_height)); then the label of :206-213:
// the prototype's class if any footprint pixel has it, else the most frequent value, the smallest value on a count tie.
// Values -1 .. SPX_PRUNE_BINS - 2 are counted in an LDS histogram; any other value is counted pairwise over the footprint.
__global__ __launch_bounds__(256) void spx_prune_footprint_kernel(const int32_t* __restrict__ labels, int Hf, int Wf, int H, int W, int P,
                                                                  const unsigned long long* __restrict__ keys,
                                                                  const int32_t* __restrict__ target_class,
                                                                  int32_t* __restrict__ out_label, int32_t* __restrict__ out_box) {
    __shared__ uint32_t hist[SPX_PRUNE_BINS];
    __shared__ unsigned long long s_best[4];
    const int p = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const size_t o = (size_t)b * P + p;
    const uint32_t flat = (uint32_t)keys[o];
    const int i = (int)(flat / (uint32_t)W), j = (int)(flat % (uint32_t)W);
    const double ph = (double)Hf / (double)H, pw = (double)Wf / (double)W;
    // numpy slicing clamps the stop at the array's end
    const int h0 = min((int)((double)i * ph), Hf), h1 = min((int)((double)(i + 1) * ph), Hf);
    const int w0 = min((int)((double)j * pw), Wf), w1 = min((int)((double)(j + 1) * pw), Wf);
    if (tid == 0) {
        out_box[4 * o + 0] = h0;
        out_box[4 * o + 1] = h1;
        out_box[4 * o + 2] = w0;
        out_box[4 * o + 3] = w1;
    }
    const int bh = h1 - h0, bw = w1 - w0;
    if (bh <= 0 || bw <= 0) {                  // empty footprint: the candidate is skipped (:168-169)
        if (tid == 0) out_label[o] = 0;
        return;
    }
    const int n = bh * bw;
    const int tc = target_class[p];
    const int32_t* img = labels + (size_t)b * Hf * Wf;
    for (int t = tid; t < SPX_PRUNE_BINS; t += 256) hist[t] = 0;
    __syncthreads();
    int found = 0, wide = 0;
    for (int t = tid; t < n; t += 256) {
        const int v = img[(size_t)(h0 + t / bw) * Wf + w0 + t % bw];
        found |= v == tc;
        const unsigned u = (unsigned)(v + 1);
        if (u < (unsigned)SPX_PRUNE_BINS) atomicAdd(hist + u, 1u);
        else wide = 1;
    }
    found = __syncthreads_or(found);
    if (found) {
        if (tid == 0) out_label[o] = tc;
        return;
    }
    wide = __syncthreads_or(wide);
    // (count, smallest value) as one maximum: count above, the complement of the order-preserving value bits below
    unsigned long long best = 0;
    for (int t = tid; t < SPX_PRUNE_BINS; t += 256) {
        const uint32_t c = hist[t];
        if (c) best = max(best, ((unsigned long long)c << 32) | (0xFFFFFFFFu - ((uint32_t)(t - 1) ^ 0x80000000u)));
    }
    if (wide) {
        for (int t = tid; t < n; t += 256) {
            const int v = img[(size_t)(h0 + t / bw) * Wf + w0 + t % bw];
            if ((unsigned)(v + 1) < (unsigned)SPX_PRUNE_BINS) continue;
            uint32_t c = 0;
            for (int q = 0; q < n; ++q) c += img[(size_t)(h0 + q / bw) * Wf + w0 + q % bw] == v;
            best = max(best, ((unsigned long long)c << 32) | (0xFFFFFFFFu - ((uint32_t)v ^ 0x80000000u)));
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long x = shfl_xor_u64(best, s);
        best = x > best ? x : best;
    }
    if ((tid & 63) == 0) s_best[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long v = s_best[0];
        for (int w = 1; w < 4; ++w) v = s_best[w] > v ? s_best[w] : v;
        out_label[o] = (int32_t)((0xFFFFFFFFu - (uint32_t)v) ^ 0x80000000u);
    }
}

// One thread per prototype.  The table row [k] is sorted by (distance key, image); empty slots carry image -1 at the end.
// Candidates of images image0 .. image0 + B - 1 are inserted in image order: a candidate enters a full row only when its
// key is strictly below the last entry's (every kept image is earlier, so an equal key keeps the earlier image), and goes
// after the entries with an equal key.  Result: the k smallest candidates by (key, image).
__global__ __launch_bounds__(256) void spx_prune_merge_kernel(const unsigned long long* __restrict__ ckey, const int32_t* __restrict__ clabel,
                                                              const int32_t* __restrict__ cbox, int B, int P, int W, long long image0, int k,
                                                              unsigned long long* __restrict__ tkey, long long* __restrict__ timg,
                                                              int32_t* __restrict__ tlabel, int32_t* __restrict__ tbox,
                                                              int32_t* __restrict__ tcell) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    unsigned long long* rk = tkey + (size_t)p * k;
    long long* ri = timg + (size_t)p * k;
    int32_t* rl = tlabel + (size_t)p * k;
    int32_t* rb = tbox + (size_t)p * k * 4;
    int32_t* rc = tcell + (size_t)p * k * 2;
    int cnt = 0;
    while (cnt < k && ri[cnt] >= 0) ++cnt;
    for (int b = 0; b < B; ++b) {
        const size_t o = (size_t)b * P + p;
        const int4 box = *(const int4*)(cbox + 4 * o);
        if (box.y <= box.x || box.w <= box.z) continue;             // empty footprint: skipped, as the reference does
        const unsigned long long key = ckey[o];
        const uint32_t hi = (uint32_t)(key >> 32);
        if (cnt == k && hi >= (uint32_t)(rk[k - 1] >> 32)) continue;
        int pos = cnt < k ? cnt : k - 1;                            // the slot freed at the end
        while (pos > 0 && (uint32_t)(rk[pos - 1] >> 32) > hi) {
            rk[pos] = rk[pos - 1];
            ri[pos] = ri[pos - 1];
            rl[pos] = rl[pos - 1];
            *(int4*)(rb + 4 * pos) = *(const int4*)(rb + 4 * (pos - 1));
            rc[2 * pos] = rc[2 * pos - 2];
            rc[2 * pos + 1] = rc[2 * pos - 1];
            --pos;
        }
        rk[pos] = key;
        ri[pos] = image0 + b;
        rl[pos] = clabel[o];
        *(int4*)(rb + 4 * pos) = box;
        const uint32_t flat = (uint32_t)key;
        rc[2 * pos] = (int32_t)(flat / (uint32_t)W);
        rc[2 * pos + 1] = (int32_t)(flat % (uint32_t)W);
        if (cnt < k) ++cnt;
    }
}

hipError_t spx_launch_prune_argmin(const float* dist, const int32_t* labels, int void_label, int B, int P, int HW,
                                   uint64_t* keys, hipStream_t s) {
    hipError_t e = hipMemsetAsync(keys, 0xFF, (size_t)B * P * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    dim3 grid((HW + SPX_PRUNE_CHUNK - 1) / SPX_PRUNE_CHUNK, (P + SPX_PRUNE_PB - 1) / SPX_PRUNE_PB, B);
    hipLaunchKernelGGL(spx_prune_argmin_kernel, grid, dim3(256), 0, s, dist, labels, void_label, P, HW, (unsigned long long*)keys);
    return hipGetLastError();
}

hipError_t spx_launch_prune_footprint(const int32_t* labels, int B, int Hf, int Wf, int H, int W, int P, const uint64_t* keys,
                                      const int32_t* target_class, int32_t* label, int32_t* box, hipStream_t s) {
    hipLaunchKernelGGL(spx_prune_footprint_kernel, dim3(P, B), dim3(256), 0, s, labels, Hf, Wf, H, W, P,
                       (const unsigned long long*)keys, target_class, label, box);
    return hipGetLastError();
}

hipError_t spx_launch_prune_merge(const uint64_t* keys, const int32_t* label, const int32_t* box, int B, int P, int W, long long image0,
                                  int k, uint64_t* tkey, int64_t* timg, int32_t* tlabel, int32_t* tbox, int32_t* tcell, hipStream_t s) {
    hipLaunchKernelGGL(spx_prune_merge_kernel, dim3((P + 255) / 256), dim3(256), 0, s, (const unsigned long long*)keys, label, box, B,
                       P, W, image0, k, (unsigned long long*)tkey, (long long*)timg, tlabel, tbox, tcell);
    return hipGetLastError();
}
