// Part consistency and stability (segmentation/analysis/metrics/consistency.py:186-270, stability.py): connected components of
// the part annotations with their centroids, the quantile threshold of every class-masked, nearest-upsampled activation plane,
// and the presence of every (class, slot) at every part's centroids.  include/spx_hip.h states the contract.
//
// 1. Components.  A pixel's key is (class k, part t) = k * M + t - 1 when labels == k + 1 with 0 <= k < K and 1 <= parts <= M, else
//    none.  Two pixels are joined when they are 8-neighbours with the same key.  Union-find over parent[n][i], i = Y * W + X:
//      prt_tile_kernel   labels a 32 x 32 tile in LDS, writes parent = the image index of the tile-local root, and at that root
//                        the tile-local count / sum X / sum Y (zero elsewhere); adds them to the totals of (n, key);
//      prt_merge_kernel  unions every pair of neighbours that lies across a tile border;
//      prt_flatten_kernel points every keyed pixel at its root and moves the tile-local sums to the root.
//    INVARIANT: parent[i] <= i, always.  The tile kernel writes the index of the smallest pixel of the tile-local component (the
//    local order ly * 32 + lx and the image order agree inside a tile); afterwards a parent only changes by atomicMin with a value
//    below the pixel it is stored at.
//    WHY EVERY LOOP ENDS.  find(a) follows a = parent[a] while parent[a] != a: by the invariant a strictly decreases, and it is
//    bounded by 0.  union(a, b) repeats { a = find(a); b = find(b); stop if equal; order them a > b; old = atomicMin(&parent[a], b);
//    stop if old == a; a = old }: when it does not stop, old < a (the invariant, and old != a) and b < a, so max(a, b) strictly
//    decreases from one round to the next.  Neither loop waits for another thread: a concurrent atomicMin can only lower a parent,
//    which shortens nobody's walk below its bound.  No workgroup waits on another; what one kernel wrote is visible to the next by
//    the kernel boundary.  Inside the merge and flatten kernels every access to parent[] is an agent-scope atomic (load, min or
//    store), so no stale line of a CU's L1 is ever read.
//    The sums are integers added with integer atomics: the order of arrival does not change them, two runs agree bit for bit.
// 2. Thresholds.  u[Y, X] = labels == k + 1 ? a[sy(Y), sx(X)] : +0 takes at most h * w + 1 distinct values: prt_count_kernel counts,
//    in one pass over the labels, how many pixels of every class fall on every latent cell, and prt_threshold_kernel (one
//    workgroup per (n, k, slot), no traffic between workgroups) runs the radix select of spx_overlap_sample.h over the cells'
//    values with those multiplicities, histograms in LDS.  The [H, W] plane is never formed.
// 3. Presence.  prt_presence_init_kernel writes every byte of the table (0 for a part that occurs, 255 otherwise) and the valid
//    flags; the two presence kernels then store the byte 1, and nothing else, where an activation beats its threshold at a
//    centroid: whichever of several equal stores lands last, the byte is the same.
#include "spx_overlap_sample.h"

#define PRT_TILE 32
#define PRT_TILE_PX (PRT_TILE * PRT_TILE)
#define PRT_THREADS 256
#define PRT_NONE 0xffffffffu

// ---- what the kernels share ----------------------------------------------------------------------------------------------
// the key of pixel o of the flat label / part maps, or -1
__device__ __forceinline__ int prt_key(const void* labels, int label_bytes, const void* parts, int part_bytes, size_t o, int K, int M) {
    const long long lab = spx_label(labels, label_bytes, o);
    if (lab < 1 || lab > K) return -1;
    const long long t = spx_label(parts, part_bytes, o);
    if (t < 1 || t > M) return -1;
    return (int)(lab - 1) * M + (int)(t - 1);
}
// source index of OpenCV's INTER_NEAREST: min(floor(d * inv), in - 1) with inv = 1.0 / (out / in) formed in float64 on the host
__device__ __forceinline__ int prt_src(int d, double inv, int in) {
    const int s = (int)floor((double)d * inv);
    return s < in - 1 ? s : in - 1;
}
// (k, gamma) of numpy's linear quantile of `count` >= 1 values in float64 (overlap._rank; msk_rank of spx_masked_select.hip)
__device__ __forceinline__ void prt_rank(double q, uint32_t count, uint32_t& k, uint32_t& k1, float& gamma) {
    const double virt = q * (double)(count - 1u);
    const double fl = floor(virt);
    k = (uint32_t)fl;
    gamma = (float)(virt - fl);
    if (gamma >= 1.0f) gamma = 1.0f - 5.9604644775390625e-08f;       // 1 - 2^-24
    k1 = k + 1u < count ? k + 1u : count - 1u;
}
// np.round of a centroid coordinate: the float64 quotient of the integer sums, rounded half to even
__device__ __forceinline__ int prt_centroid(unsigned long long sum, unsigned long long count) {
    return (int)rint((double)sum / (double)count);
}

// ---- union-find in LDS (workgroup scope) and in memory (agent scope) -----------------------------------------------------------
__device__ __forceinline__ uint32_t prt_lds_find(uint32_t* lab, uint32_t a) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(&lab[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == a) return a;
        a = p;                                                       // p < a
    }
}
__device__ __forceinline__ void prt_lds_union(uint32_t* lab, uint32_t a, uint32_t b) {
    for (;;) {
        a = prt_lds_find(lab, a);
        b = prt_lds_find(lab, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = __hip_atomic_fetch_min(&lab[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;                                                     // old < a and b < a: the larger of the pair went down
    }
}
__device__ __forceinline__ uint32_t prt_find(uint32_t* par, uint32_t a) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(&par[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (p == a) return a;
        a = p;
    }
}
__device__ __forceinline__ void prt_union(uint32_t* par, uint32_t a, uint32_t b) {
    for (;;) {
        a = prt_find(par, a);
        b = prt_find(par, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = __hip_atomic_fetch_min(&par[a], b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;
    }
}

// ---- 1. components ---------------------------------------------------------------------------------------------------------
struct PrtComp {                  // the component workspace of N images of HW pixels
    uint32_t* parent;             // [N, HW]  PRT_NONE for a pixel without a key
    uint32_t* count;              // [N, HW]  pixels of the component at its root, 0 elsewhere
    unsigned long long* sumx;     // [N, HW]
    unsigned long long* sumy;     // [N, HW]
};
static inline size_t prt_comp_bytes(long long N, long long HW) { return (size_t)N * HW * 24; }
static inline PrtComp prt_comp(void* ws, long long N, long long HW) {
    PrtComp c;
    c.sumx = (unsigned long long*)ws;
    c.sumy = c.sumx + N * HW;
    c.parent = (uint32_t*)(c.sumy + N * HW);
    c.count = c.parent + N * HW;
    return c;
}

// tile (blockIdx.x, blockIdx.y) of image blockIdx.z
__global__ __launch_bounds__(PRT_THREADS) void prt_tile_kernel(const void* __restrict__ labels, int label_bytes, const void* __restrict__ parts,
                                                               int part_bytes, int K, int M, int H, int W, PrtComp comp,
                                                               unsigned long long* __restrict__ totals) {
    __shared__ int s_key[PRT_TILE_PX];
    __shared__ uint32_t s_lab[PRT_TILE_PX], s_cnt[PRT_TILE_PX], s_sx[PRT_TILE_PX], s_sy[PRT_TILE_PX];
    const int tid = threadIdx.x, X0 = blockIdx.x * PRT_TILE, Y0 = blockIdx.y * PRT_TILE;
    const size_t n = blockIdx.z, HW = (size_t)H * W;
    constexpr int PER = PRT_TILE_PX / PRT_THREADS;
    for (int p = tid; p < PRT_TILE_PX; p += PRT_THREADS) {
        const int Y = Y0 + (p >> 5), X = X0 + (p & 31);
        s_key[p] = (Y < H && X < W) ? prt_key(labels, label_bytes, parts, part_bytes, n * HW + (size_t)Y * W + X, K, M) : -1;
        s_lab[p] = (uint32_t)p;
        s_cnt[p] = 0u;
        s_sx[p] = 0u;
        s_sy[p] = 0u;
    }
    __syncthreads();
    for (int p = tid; p < PRT_TILE_PX; p += PRT_THREADS) {           // the four neighbours before p in raster order
        const int key = s_key[p];
        if (key < 0) continue;
        const int ly = p >> 5, lx = p & 31;
        if (lx > 0 && s_key[p - 1] == key) prt_lds_union(s_lab, p, p - 1);
        if (ly > 0) {
            if (lx > 0 && s_key[p - PRT_TILE - 1] == key) prt_lds_union(s_lab, p, p - PRT_TILE - 1);
            if (s_key[p - PRT_TILE] == key) prt_lds_union(s_lab, p, p - PRT_TILE);
            if (lx < PRT_TILE - 1 && s_key[p - PRT_TILE + 1] == key) prt_lds_union(s_lab, p, p - PRT_TILE + 1);
        }
    }
    __syncthreads();
    uint32_t root[PER];                                              // no union runs any more: the roots are final
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = tid + i * PRT_THREADS;
        root[i] = PRT_NONE;
        if (s_key[p] < 0) continue;
        const uint32_t r = prt_lds_find(s_lab, p);
        root[i] = r;
        atomicAdd(&s_cnt[r], 1u);
        atomicAdd(&s_sx[r], (uint32_t)(X0 + (p & 31)));              // at most 1024 * 32767: fits
        atomicAdd(&s_sy[r], (uint32_t)(Y0 + (p >> 5)));
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int p = tid + i * PRT_THREADS;
        const int Y = Y0 + (p >> 5), X = X0 + (p & 31);
        if (Y >= H || X >= W) continue;
        const size_t o = n * HW + (size_t)Y * W + X;
        const uint32_t r = root[i];
        const bool is_root = r == (uint32_t)p;
        comp.parent[o] = r == PRT_NONE ? PRT_NONE : (uint32_t)((Y0 + (int)(r >> 5)) * W + X0 + (int)(r & 31u));
        comp.count[o] = is_root ? s_cnt[p] : 0u;
        comp.sumx[o] = is_root ? s_sx[p] : 0ull;
        comp.sumy[o] = is_root ? s_sy[p] : 0ull;
        if (is_root) {
            unsigned long long* t = totals + (n * (size_t)K * M + (size_t)s_key[p]) * 3;
            atomicAdd(&t[0], (unsigned long long)s_cnt[p]);
            atomicAdd(&t[1], (unsigned long long)s_sx[p]);
            atomicAdd(&t[2], (unsigned long long)s_sy[p]);
        }
    }
}

// Every pair of 8-neighbours in different tiles: a pixel on the first column of a tile column (X % 32 == 0, X > 0) looks at its
// three left neighbours, a pixel on the first row of a tile row at its three upper neighbours.  A pair that crosses a vertical
// border is seen from its right pixel, any other pair that crosses a horizontal border from its lower pixel.
__global__ __launch_bounds__(PRT_THREADS) void prt_merge_kernel(const void* __restrict__ labels, int label_bytes, const void* __restrict__ parts,
                                                                int part_bytes, int K, int M, int H, int W, PrtComp comp) {
    const int nvb = (W - 1) / PRT_TILE, nhb = (H - 1) / PRT_TILE;
    const long long id = (long long)blockIdx.x * PRT_THREADS + threadIdx.x;
    const size_t n = blockIdx.y, HW = (size_t)H * W;
    int X, Y, dx[3], dy[3];
    if (id < (long long)nvb * H) {
        X = ((int)(id / H) + 1) * PRT_TILE;
        Y = (int)(id % H);
        for (int i = 0; i < 3; ++i) { dx[i] = -1; dy[i] = i - 1; }
    } else if (id < (long long)nvb * H + (long long)nhb * W) {
        const long long e = id - (long long)nvb * H;
        Y = ((int)(e / W) + 1) * PRT_TILE;
        X = (int)(e % W);
        for (int i = 0; i < 3; ++i) { dx[i] = i - 1; dy[i] = -1; }
    } else {
        return;
    }
    const int key = prt_key(labels, label_bytes, parts, part_bytes, n * HW + (size_t)Y * W + X, K, M);
    if (key < 0) return;
    uint32_t* par = comp.parent + n * HW;
    for (int i = 0; i < 3; ++i) {
        const int x = X + dx[i], y = Y + dy[i];
        if (x < 0 || x >= W || y < 0 || y >= H) continue;
        if (prt_key(labels, label_bytes, parts, part_bytes, n * HW + (size_t)y * W + x, K, M) != key) continue;
        prt_union(par, (uint32_t)(Y * W + X), (uint32_t)(y * W + x));
    }
}

// Pixel blockIdx.x * 256 + threadIdx.x of image blockIdx.y.  No union runs in this launch, so the roots are final; a pixel's parent
// is overwritten with its root while others may walk through it, and both the old parent and the root are its ancestors.  Only
// the thread of pixel i reads or writes count / sumx / sumy [i] of a pixel that is not a root (nothing is added there), and only
// atomics add to those of a root, whose own thread adds nothing.
__global__ __launch_bounds__(PRT_THREADS) void prt_flatten_kernel(int H, int W, PrtComp comp) {
    const size_t HW = (size_t)H * W, i = (size_t)blockIdx.x * PRT_THREADS + threadIdx.x, n = blockIdx.y;
    if (i >= HW) return;
    uint32_t* par = comp.parent + n * HW;
    const uint32_t p = __hip_atomic_load(&par[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == PRT_NONE) return;
    const uint32_t r = prt_find(par, p);
    if (r != p) __hip_atomic_store(&par[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r == (uint32_t)i) return;
    const size_t o = n * HW + i, ro = n * HW + r;
    const uint32_t c = comp.count[o];
    if (c == 0u) return;                                             // not the root of a tile-local component
    atomicAdd(&comp.count[ro], c);
    atomicAdd(&comp.sumx[ro], comp.sumx[o]);
    atomicAdd(&comp.sumy[ro], comp.sumy[o]);
    comp.count[o] = 0u;
    comp.sumx[o] = 0ull;
    comp.sumy[o] = 0ull;
}

size_t spx_parts_comp_ws_bytes(int N, int H, int W) { return prt_comp_bytes(N, (long long)H * W); }

hipError_t spx_launch_part_components(const void* labels, int label_bytes, const void* parts, int part_bytes, int N, int K, int M, int H,
                                      int W, void* workspace, unsigned long long* totals, hipStream_t s) {
    const long long HW = (long long)H * W;
    const PrtComp comp = prt_comp(workspace, N, HW);
    hipError_t e = hipMemsetAsync(totals, 0, (size_t)N * K * M * 3 * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const dim3 tiles((unsigned)((W + PRT_TILE - 1) / PRT_TILE), (unsigned)((H + PRT_TILE - 1) / PRT_TILE), (unsigned)N);
    hipLaunchKernelGGL(prt_tile_kernel, tiles, dim3(PRT_THREADS), 0, s, labels, label_bytes, parts, part_bytes, K, M, H, W, comp, totals);
    const long long border = (long long)((W - 1) / PRT_TILE) * H + (long long)((H - 1) / PRT_TILE) * W;
    if (border > 0)
        hipLaunchKernelGGL(prt_merge_kernel, dim3((unsigned)((border + PRT_THREADS - 1) / PRT_THREADS), (unsigned)N), dim3(PRT_THREADS), 0,
                           s, labels, label_bytes, parts, part_bytes, K, M, H, W, comp);
    hipLaunchKernelGGL(prt_flatten_kernel, dim3((unsigned)((HW + PRT_THREADS - 1) / PRT_THREADS), (unsigned)N), dim3(PRT_THREADS), 0, s, H,
                       W, comp);
    return hipGetLastError();
}

// ---- 2. thresholds ---------------------------------------------------------------------------------------------------------
// mult[n][k][cell]: the pixels of class k of image n whose nearest source is the latent cell.  A thread walks 8 consecutive
// pixels of row blockIdx.y and adds each run of equal (class, cell) once.
#define PRT_RUN 8
__global__ __launch_bounds__(PRT_THREADS) void prt_count_kernel(const void* __restrict__ labels, int label_bytes, int K, int h, int w, int H,
                                                                int W, double inv_y, double inv_x, uint32_t* __restrict__ mult) {
    const int Y = blockIdx.y, X0 = (blockIdx.x * PRT_THREADS + threadIdx.x) * PRT_RUN;
    if (X0 >= W) return;
    const size_t n = blockIdx.z, hw = (size_t)h * w;
    const size_t row = (n * H + Y) * (size_t)W;
    uint32_t* m = mult + n * K * hw;
    const int cy = prt_src(Y, inv_y, h);
    long long cur = -1;
    uint32_t run = 0u;
    for (int X = X0; X < W && X < X0 + PRT_RUN; ++X) {
        const long long lab = spx_label(labels, label_bytes, row + X);
        if (lab < 1 || lab > K) continue;
        const long long at = (long long)((lab - 1) * hw) + (long long)cy * w + prt_src(X, inv_x, w);
        if (at != cur) {
            if (run) atomicAdd(&m[cur], run);
            cur = at;
            run = 0u;
        }
        ++run;
    }
    if (run) atomicAdd(&m[cur], run);
}

// Slot blockIdx.x of class blockIdx.y of image blockIdx.z.  mode 0 ("image"): all H * W values of u, the pixels outside the class
// as +0 with multiplicity H * W - n_k.  mode 1 ("nonzero"): the values of u that are not zero; none: T = +inf.  A slot without a
// channel in [0, C) and a skipped class get NaN.
__global__ __launch_bounds__(OVL_THREADS) void prt_threshold_kernel(SpxPlanes a, const int32_t* __restrict__ table, const uint8_t* __restrict__ skip,
                                                                    const uint32_t* __restrict__ mult, int C, int K, int J, int h, int w,
                                                                    long long HWout, double q, int mode, float* __restrict__ thresholds) {
    __shared__ uint32_t s_hist[2 * OVL_BINS];
    __shared__ uint32_t s_st[4];
    __shared__ uint32_t s_count, s_class;
    const int tid = threadIdx.x, j = blockIdx.x, k = blockIdx.y;
    const size_t n = blockIdx.z, hw = (size_t)h * w;
    const size_t row = (n * K + k) * J + j;
    const int c = table[k * J + j];
    if (c < 0 || c >= C || (skip && skip[k])) {                      // workgroup-uniform
        if (tid == 0) thresholds[row] = __uint_as_float(0x7fc00000u);
        return;
    }
    const uint32_t* m = mult + (n * K + k) * hw;
    const float* src = a.p + (long long)n * a.sn + (long long)c * a.sc;
    auto value = [&](int i) {
        const int y = i / w, x = i - y * w;
        return src[(long long)y * a.sy + (long long)x * a.sx];
    };
    ovl_clear_hist(s_hist);
    if (tid < 4) s_st[tid] = 0u;
    if (tid == 0) { s_count = 0u; s_class = 0u; }
    __syncthreads();
    uint32_t mine = 0u, mine_class = 0u;
    for (int i = tid; i < (int)hw; i += OVL_THREADS) {
        const uint32_t wgt = m[i];
        mine_class += wgt;
        if (wgt && (mode == 0 || value(i) != 0.0f)) mine += wgt;
    }
    if (mine) atomicAdd(&s_count, mine);
    if (mine_class) atomicAdd(&s_class, mine_class);
    __syncthreads();
    const uint32_t zeros = mode == 0 ? (uint32_t)(HWout - (long long)s_class) : 0u;
    const uint32_t count = s_count + zeros;
    if (count == 0u) {                                               // workgroup-uniform
        if (tid == 0) thresholds[row] = __uint_as_float(0x7f800000u);
        return;
    }
    uint32_t k0, k1;
    float gamma;
    prt_rank(q, count, k0, k1, gamma);
    const uint32_t zero_key = ovl_key(0.0f);
    for (int round = 0; round < 3; ++round) {
        const uint32_t p0 = s_st[0], p1 = s_st[2];
        __syncthreads();                                             // the prefixes are read before the scan rewrites them
        auto add = [&](uint32_t key, uint32_t wgt) {
            if (round == 0) {
                atomicAdd(&s_hist[key >> 21], wgt);
            } else if (round == 1) {
                if ((key >> 21) == p0) atomicAdd(&s_hist[(key >> 10) & 2047u], wgt);
                if ((key >> 21) == p1) atomicAdd(&s_hist[OVL_BINS + ((key >> 10) & 2047u)], wgt);
            } else {
                if ((key >> 10) == p0) atomicAdd(&s_hist[key & 1023u], wgt);
                if ((key >> 10) == p1) atomicAdd(&s_hist[OVL_BINS + (key & 1023u)], wgt);
            }
        };
        for (int i = tid; i < (int)hw; i += OVL_THREADS) {
            const uint32_t wgt = m[i];
            if (!wgt) continue;
            const float v = value(i);
            if (mode == 1 && !(v != 0.0f)) continue;
            add(ovl_key(v), wgt);
        }
        if (tid == 0 && zeros) add(zero_key, zeros);
        __syncthreads();
        ovl_scan_round(round, s_st, s_hist, [&](int r) { return round == 0 ? (r == 0 ? k0 : k1) : s_st[2 * r + 1]; });
        __syncthreads();
    }
    if (tid == 0) thresholds[row] = ovl_lerp(ovl_unkey(s_st[0]), ovl_unkey(s_st[2]), gamma);
}

size_t spx_parts_thr_ws_bytes(int N, int K, int h, int w) { return (size_t)N * K * h * w * sizeof(uint32_t); }

hipError_t spx_launch_part_thresholds(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* table,
                                      const uint8_t* skip, int N, int C, int K, int J, int h, int w, int H, int W, double q, int mode,
                                      void* workspace, float* thresholds, hipStream_t s) {
    uint32_t* mult = (uint32_t*)workspace;
    hipError_t e = hipMemsetAsync(mult, 0, spx_parts_thr_ws_bytes(N, K, h, w), s);
    if (e != hipSuccess) return e;
    const double inv_y = 1.0 / ((double)H / (double)h), inv_x = 1.0 / ((double)W / (double)w);
    const dim3 cgrid((unsigned)((W + PRT_THREADS * PRT_RUN - 1) / (PRT_THREADS * PRT_RUN)), (unsigned)H, (unsigned)N);
    hipLaunchKernelGGL(prt_count_kernel, cgrid, dim3(PRT_THREADS), 0, s, labels, label_bytes, K, h, w, H, W, inv_y, inv_x, mult);
    hipLaunchKernelGGL(prt_threshold_kernel, dim3((unsigned)J, (unsigned)K, (unsigned)N), dim3(OVL_THREADS), 0, s, spx_planes(planes, st),
                       table, skip, mult, C, K, J, h, w, (long long)H * W, q, mode, thresholds);
    return hipGetLastError();
}

// ---- 3. presence -----------------------------------------------------------------------------------------------------------
struct PrtPresence {
    SpxPlanes a;
    const void* labels;
    int label_bytes;
    const int32_t* table;         // [K, J]
    const uint8_t* skip;          // [K] or NULL
    const float* thresholds;      // [N, K, J]
    int C, K, J, M, h, w, H, W;
    double inv_y, inv_x;
    uint8_t* out;                 // [N, K, J, M + 1]
};

// every slot of class k of image n at the centroid (cx, cy) of part t
__device__ __forceinline__ void prt_test(const PrtPresence& p, size_t n, int k, int t, int cx, int cy) {
    const bool inside = spx_label(p.labels, p.label_bytes, (n * p.H + cy) * (size_t)p.W + cx) == (long long)k + 1;
    const float* cell = p.a.p + (long long)n * p.a.sn + (long long)prt_src(cy, p.inv_y, p.h) * p.a.sy + (long long)prt_src(cx, p.inv_x, p.w) * p.a.sx;
    for (int j = 0; j < p.J; ++j) {
        const int c = p.table[k * p.J + j];
        if (c < 0 || c >= p.C) continue;
        const size_t row = (n * p.K + k) * p.J + j;
        const float v = inside ? cell[(long long)c * p.a.sc] : 0.0f;
        if (v > p.thresholds[row]) p.out[row * (p.M + 1) + t] = (uint8_t)1;
    }
}

// element blockIdx.x * 256 + threadIdx.x of the table [N, K, J, M + 1]; the element (j, t) = (0, 0) also writes valid[n, k]
__global__ __launch_bounds__(PRT_THREADS) void prt_presence_init_kernel(const int32_t* __restrict__ table, const uint8_t* __restrict__ skip,
                                                                        const unsigned long long* __restrict__ totals, int N, int C, int K,
                                                                        int J, int M, uint8_t* __restrict__ out, uint8_t* __restrict__ valid) {
    const size_t e = (size_t)blockIdx.x * PRT_THREADS + threadIdx.x;
    if (e >= (size_t)N * K * J * (M + 1)) return;
    const int t = (int)(e % (M + 1)), j = (int)(e / (M + 1) % J), k = (int)(e / (M + 1) / J % K);
    const size_t n = e / (M + 1) / J / K;
    const unsigned long long* tot = totals + (n * K + k) * (size_t)M * 3;
    bool any = false;
    for (int i = 0; i < M; ++i) any = any || tot[3 * i] != 0ull;
    const bool ok = any && !(skip && skip[k]);
    const int c = table[k * J + j];
    out[e] = (ok && c >= 0 && c < C && t > 0 && tot[3 * (t - 1)] != 0ull) ? (uint8_t)0 : (uint8_t)255;
    if (j == 0 && t == 0) valid[n * K + k] = ok ? (uint8_t)1 : (uint8_t)0;
}

// pixel blockIdx.x * 256 + threadIdx.x of image blockIdx.y: the root of a component tests at the component's centroid
__global__ __launch_bounds__(PRT_THREADS) void prt_presence_comp_kernel(PrtPresence p, const void* __restrict__ parts, int part_bytes,
                                                                        PrtComp comp) {
    const size_t HW = (size_t)p.H * p.W, i = (size_t)blockIdx.x * PRT_THREADS + threadIdx.x, n = blockIdx.y;
    if (i >= HW) return;
    const uint32_t cnt = comp.count[n * HW + i];
    if (cnt == 0u) return;
    const int key = prt_key(p.labels, p.label_bytes, parts, part_bytes, n * HW + i, p.K, p.M);
    if (key < 0) return;                                             // (a root always has a key)
    const int k = key / p.M, t = key % p.M + 1;
    if (p.skip && p.skip[k]) return;
    prt_test(p, n, k, t, prt_centroid(comp.sumx[n * HW + i], cnt), prt_centroid(comp.sumy[n * HW + i], cnt));
}

// (n, k, t) = element blockIdx.x * 256 + threadIdx.x of [N, K, M]: the complement of B_t within the image, from the totals
__global__ __launch_bounds__(PRT_THREADS) void prt_presence_rest_kernel(PrtPresence p, int N, const unsigned long long* __restrict__ totals) {
    const size_t e = (size_t)blockIdx.x * PRT_THREADS + threadIdx.x;
    if (e >= (size_t)N * p.K * p.M) return;
    const int t = (int)(e % p.M) + 1, k = (int)(e / p.M % p.K);
    const size_t n = e / p.M / p.K;
    const unsigned long long HW = (unsigned long long)p.H * p.W, cnt = totals[3 * e];
    if (cnt == 0ull || cnt >= HW || (p.skip && p.skip[k])) return;
    const unsigned long long allx = (unsigned long long)p.H * ((unsigned long long)p.W * (p.W - 1) / 2);
    const unsigned long long ally = (unsigned long long)p.W * ((unsigned long long)p.H * (p.H - 1) / 2);
    prt_test(p, n, k, t, prt_centroid(allx - totals[3 * e + 1], HW - cnt), prt_centroid(ally - totals[3 * e + 2], HW - cnt));
}

hipError_t spx_launch_part_presence(const float* planes, const long long* st, const void* labels, int label_bytes, const void* parts,
                                    int part_bytes, const int32_t* table, const uint8_t* skip, const float* thresholds,
                                    const void* comp_workspace, const unsigned long long* totals, int N, int C, int K, int J, int M, int h,
                                    int w, int H, int W, uint8_t* out, uint8_t* valid, hipStream_t s) {
    const long long HW = (long long)H * W;
    const PrtComp comp = prt_comp((void*)comp_workspace, N, HW);
    PrtPresence p;
    p.a = spx_planes(planes, st);
    p.labels = labels;
    p.label_bytes = label_bytes;
    p.table = table;
    p.skip = skip;
    p.thresholds = thresholds;
    p.C = C; p.K = K; p.J = J; p.M = M; p.h = h; p.w = w; p.H = H; p.W = W;
    p.inv_y = 1.0 / ((double)H / (double)h);
    p.inv_x = 1.0 / ((double)W / (double)w);
    p.out = out;
    const long long elems = (long long)N * K * J * (M + 1), rest = (long long)N * K * M;
    hipLaunchKernelGGL(prt_presence_init_kernel, dim3((unsigned)((elems + PRT_THREADS - 1) / PRT_THREADS)), dim3(PRT_THREADS), 0, s, table,
                       skip, totals, N, C, K, J, M, out, valid);
    hipLaunchKernelGGL(prt_presence_comp_kernel, dim3((unsigned)((HW + PRT_THREADS - 1) / PRT_THREADS), (unsigned)N), dim3(PRT_THREADS), 0, s,
                       p, parts, part_bytes, comp);
    hipLaunchKernelGGL(prt_presence_rest_kernel, dim3((unsigned)((rest + PRT_THREADS - 1) / PRT_THREADS)), dim3(PRT_THREADS), 0, s, p, N,
                       totals);
    return hipGetLastError();
}

// ---- counters --------------------------------------------------------------------------------------------------------------
// consistency: counters int64 [ones K J (M+1) | times present K J (M+1) | rows K J].  One thread per (k, j, t) walks the images in
// order: no atomics.
__global__ __launch_bounds__(PRT_THREADS) void prt_fold_consistency_kernel(const uint8_t* __restrict__ tab, const uint8_t* __restrict__ valid,
                                                                           const int32_t* __restrict__ table, int N, int C, int K, int J, int M,
                                                                           long long* __restrict__ counters) {
    const size_t e = (size_t)blockIdx.x * PRT_THREADS + threadIdx.x, per = (size_t)K * J * (M + 1);
    if (e >= per) return;
    const int t = (int)(e % (M + 1)), j = (int)(e / (M + 1) % J), k = (int)(e / (M + 1) / J);
    const int c = table[k * J + j];
    if (c < 0 || c >= C) return;
    long long ones = 0, times = 0, rows = 0;
    for (int n = 0; n < N; ++n) {
        if (!valid[(size_t)n * K + k]) continue;
        const uint8_t v = tab[(size_t)n * per + e];
        ones += v == 1;
        times += v != 255;
        ++rows;
    }
    counters[e] += ones;
    counters[per + e] += times;
    if (t == 0) counters[2 * per + (size_t)k * J + j] += rows;
}

// stability: counters int64 [stable rows | valid rows].  One thread per (n, k, j); a workgroup adds its two sums once.
__global__ __launch_bounds__(PRT_THREADS) void prt_fold_stability_kernel(const uint8_t* __restrict__ clean, const uint8_t* __restrict__ noisy,
                                                                         const uint8_t* __restrict__ valid, const int32_t* __restrict__ table,
                                                                         int N, int C, int K, int J, int M, unsigned long long* __restrict__ counters) {
    __shared__ uint32_t s_stable, s_rows;
    if (threadIdx.x == 0) { s_stable = 0u; s_rows = 0u; }
    __syncthreads();
    const size_t e = (size_t)blockIdx.x * PRT_THREADS + threadIdx.x;
    if (e < (size_t)N * K * J) {
        const int j = (int)(e % J), k = (int)(e / J % K);
        const size_t n = e / J / K;
        const int c = table[k * J + j];
        if (c >= 0 && c < C && valid[n * K + k]) {
            bool same = true;
            for (int t = 0; t <= M; ++t) same = same && (clean[e * (M + 1) + t] == 1) == (noisy[e * (M + 1) + t] == 1);
            atomicAdd(&s_rows, 1u);
            if (same) atomicAdd(&s_stable, 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_rows) {
        atomicAdd(&counters[0], (unsigned long long)s_stable);
        atomicAdd(&counters[1], (unsigned long long)s_rows);
    }
}

hipError_t spx_launch_part_fold_consistency(const uint8_t* tab, const uint8_t* valid, const int32_t* table, int N, int C, int K, int J, int M,
                                            long long* counters, hipStream_t s) {
    const long long per = (long long)K * J * (M + 1);
    hipLaunchKernelGGL(prt_fold_consistency_kernel, dim3((unsigned)((per + PRT_THREADS - 1) / PRT_THREADS)), dim3(PRT_THREADS), 0, s, tab,
                       valid, table, N, C, K, J, M, counters);
    return hipGetLastError();
}

hipError_t spx_launch_part_fold_stability(const uint8_t* clean, const uint8_t* noisy, const uint8_t* valid, const int32_t* table, int N, int C,
                                          int K, int J, int M, unsigned long long* counters, hipStream_t s) {
    const long long rows = (long long)N * K * J;
    hipLaunchKernelGGL(prt_fold_stability_kernel, dim3((unsigned)((rows + PRT_THREADS - 1) / PRT_THREADS)), dim3(PRT_THREADS), 0, s, clean,
                       noisy, valid, table, N, C, K, J, M, counters);
    return hipGetLastError();
}
