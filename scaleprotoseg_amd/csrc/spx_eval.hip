// Evaluation-time full-resolution maps: bilinear upsample (align_corners = False) of a
// [N, C, h, w] map to [H, W] fused with the per-pixel argmin / argmax over C - the reference materialises the
// upsampled [C, H, W] tensor (1.6-1.9 GB per Cityscapes image) and copies it to the host first
// (segmentation/eval_valid_multiscale.py:229-234, :375-383).  The source map (<= tens of MB) stays cache-resident:
// every output pixel reads its 4 neighbours of each channel; neighbouring outputs share them.
#include "spx_planes.h"

// torch's area_pixel_compute_source_index for align_corners = False (no explicit scale factor): scale = in / out,
// src = scale * (dst + 0.5) - 0.5 clamped at 0; i0 = floor, i1 = min(i0 + 1, in - 1), lambda1 = src - i0.
// The arithmetic is the CPU kernel's OPERATION BY OPERATION, fused multiply-adds where the shipped x86 builds have them
// (aten/src/ATen/native/cpu/UpSampleKernel.cpp; restated and pinned bit for bit in oracle/ppnet_oracle.py::
// upsample_bilinear_restated): the values, and with them the arg{min,max} indices, are bit-identical to the reference's
// F.interpolate + min / max on the host (this library is compiled with -ffp-contract=off: every fma below is explicit).
__device__ __forceinline__ void src_index(int dst, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float s = __builtin_fmaf(scale, (float)dst + 0.5f, -0.5f);
    s = s < 0.0f ? 0.0f : s;
    i0 = (int)s;
    if (i0 > in_size - 1) i0 = in_size - 1;
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = s - (float)i0;
    l0 = 1.0f - l1;
}

__global__ __launch_bounds__(256) void spx_upsample_argext_kernel(const float* __restrict__ src, int C, int h, int w,
                                                                  int H, int W, float sh, float sw, int take_max,
                                                                  int64_t* __restrict__ idx, float* __restrict__ val) {
    const int ox = blockIdx.x * 64 + (threadIdx.x & 63);
    const int oy = blockIdx.y * 4 + (threadIdx.x >> 6);
    const int n = blockIdx.z;
    if (ox >= W || oy >= H) return;
    int y0, y1, x0, x1;
    float ly0, ly1, lx0, lx1;
    src_index(oy, sh, h, y0, y1, ly0, ly1);
    src_index(ox, sw, w, x0, x1, lx0, lx1);
    const float* base = src + (size_t)n * C * h * w;
    const int o00 = y0 * w + x0, o01 = y0 * w + x1, o10 = y1 * w + x0, o11 = y1 * w + x1;
    float best = 0.0f;
    int bi = 0;
    const int hw = h * w;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        const float* p = base + (size_t)c * hw;
        // rows first (t0, t1), then the two rows blended; in each blend the first product is fused, the second rounded
        const float t0 = __builtin_fmaf(p[o00], lx0, p[o01] * lx1), t1 = __builtin_fmaf(p[o10], lx0, p[o11] * lx1);
        const float v = __builtin_fmaf(t0, ly0, t1 * ly1);
        const bool better = take_max ? (v > best) : (v < best);
        if (c == 0 || better) {      // strict comparison: ties keep the lowest channel index
            best = v;
            bi = c;
        }
    }
    const size_t o = ((size_t)n * H + oy) * W + ox;
    idx[o] = bi;
    if (val) val[o] = best;
}

hipError_t spx_launch_upsample_argext(const float* src, int N, int C, int h, int w, int H, int W, int take_max,
                                      int64_t* idx, float* val, hipStream_t s) {
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    dim3 grid((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4), (unsigned)N);
    hipLaunchKernelGGL(spx_upsample_argext_kernel, grid, dim3(256), 0, s, src, C, h, w, H, W, sh, sw, take_max, idx, val);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Evaluation metrics (segmentation/eval_valid_multiscale.py:229-269): the same bilinear arithmetic and
// arg-reductions as above, but the per-pixel pred / near stay in registers and only integer counters leave the chip:
//   conf [K+1, K]  conf[r, pred] += 1 per non-void pixel, r = ann - 1 for 1 <= ann <= K, else K (":236-243")
//   hits [P]       hits[near] += 1 where cls(near) == pred, void pixels included (":245-253")
//   topk [P]       per sample pixel: stable ascending order of the P distances, topk[k] += #hits among the first k+1
//                  (":255-269"); seen += 1 per sample taken.
// Counters are privatised per workgroup in LDS (u32) and flushed once per workgroup with 64-bit global atomics (only the
// non-zero words).  The accumulate grid is persistent (a few workgroups per CU, each walking many 64 x 16 pixel tiles),
// so the zeroing and the flush are paid a few times per CU, not per tile.  The confusion matrix is held whole in LDS
// when (K+1)*K <= SPX_EVAL_FULL_CONF_WORDS; above that (ADE 150, COCO 182) only its diagonal is - a good model's
// pixels land there - and the off-diagonal cells go straight to global 64-bit atomics.  Exact either way.

#define SPX_EVAL_THREADS 256
#define SPX_EVAL_FULL_CONF_WORDS 8192

__device__ __forceinline__ float bilerp(const float* __restrict__ q, unsigned o00, unsigned o01, unsigned o10, unsigned o11,
                                        float lx0, float lx1, float ly0, float ly1) {
    const float t0 = __builtin_fmaf(q[o00], lx0, q[o01] * lx1), t1 = __builtin_fmaf(q[o10], lx0, q[o11] * lx1);
    return __builtin_fmaf(t0, ly0, t1 * ly1);
}

// arg{max,min} over C channels of the interpolated map at one output pixel (strict comparison: lowest index on ties).
// q: the image's channel 0 (workgroup-uniform); o**: 32-bit in-image offsets of the 4 neighbours; sc: channel stride.
template <bool MAX, typename T>
__device__ __forceinline__ int argext_at(const float* __restrict__ q, T sc, int C, unsigned o00, unsigned o01, unsigned o10,
                                         unsigned o11, float lx0, float lx1, float ly0, float ly1) {
    float best = 0.0f;
    int bi = 0;
#pragma unroll 4
    for (int c = 0; c < C; ++c) {
        const float v = bilerp(q, o00, o01, o10, o11, lx0, lx1, ly0, ly1);
        q += sc;
        const bool better = MAX ? (v > best) : (v < best);
        if (c == 0 || better) {
            best = v;
            bi = c;
        }
    }
    return bi;
}

// the same scan over channels c0 .. c0 + nc - 1 of a longer run: best / bi carry over from the previous chunk, so the
// chunked scan makes exactly the comparisons of one scan
template <bool MAX>
__device__ __forceinline__ void argext_run(const float* __restrict__ q, int sc, int c0, int nc, unsigned o00, unsigned o01,
                                           unsigned o10, unsigned o11, float lx0, float lx1, float ly0, float ly1, float& best,
                                           int& bi) {
#pragma unroll 4
    for (int j = 0; j < nc; ++j) {
        const float v = bilerp(q, o00, o01, o10, o11, lx0, lx1, ly0, ly1);
        q += sc;
        const bool better = MAX ? (v > best) : (v < best);
        if (c0 + j == 0 || better) {
            best = v;
            bi = c0 + j;
        }
    }
}

// Logits arrive pixel-major ([N, h, w, K]): read straight from memory, the 64 lanes of a wave touch ~9 source pixels
// K * 4 bytes apart, i.e. ~9 cache lines per load instead of the one line of a channel-major map.  So each tile first
// copies its source footprint (rows ya..yb, columns xa..xb, all K channels; ~2 x 9 pixels at x8) to LDS channel-major
// with coalesced reads, and the K-channel scan reads LDS.  A footprint above SPX_EVAL_STAGE floats (strong
// down-sampling) is read from memory directly.  The values are the same floats either way.
// The distance map is channel-major, but read from memory its 912 loads per pixel (228 channels x 4 neighbours) keep
// the texture-address path busy at ~5 cycles per wave-load; from LDS the same reads are broadcasts.  Its footprint is
// staged in chunks of SPX_EVAL_DCHUNK channels, each a padded 4 x 16 block (rows x columns, so the staging index is
// shifts and masks), whenever the tile's footprint fits that block (up-sampling by ~x4.6 or more: all the reference's
// evaluation shapes); otherwise the distances are read from memory directly.
#define SPX_EVAL_STAGE 4096
#define SPX_EVAL_TILE_H 16                                    // output rows per tile: a tile is 64 x SPX_EVAL_TILE_H pixels,
                                                              // one per thread (4 / 8 / 16 rows: profiles/eval_metrics_summary.md)
#define SPX_EVAL_ACC_THREADS (64 * SPX_EVAL_TILE_H)
#define SPX_EVAL_DCHUNK (SPX_EVAL_STAGE / 64)

__global__ __launch_bounds__(SPX_EVAL_ACC_THREADS) void spx_eval_accumulate_kernel(
    SpxPlanes lg, SpxPlanes ds, const int32_t* __restrict__ pcls, const void* __restrict__ labels, int label_bytes, int N, int K,
    int P, int h, int w, int H, int W, float sh, float sw, int tiles_x, int tiles_y, int full_conf,
    unsigned long long* __restrict__ conf, unsigned long long* __restrict__ hits) {
    extern __shared__ unsigned int s_eval[];
    const int tid = threadIdx.x;
    const bool with_d = ds.p != nullptr;
    const int nconf = full_conf ? (K + 1) * K : K;
    unsigned int* s_conf = s_eval;
    unsigned int* s_hits = s_eval + nconf;
    int* s_cls = (int*)(s_hits + P);
    float* s_lg = (float*)(s_cls + P);
    for (int i = tid; i < nconf + (with_d ? P : 0); i += SPX_EVAL_ACC_THREADS) s_eval[i] = 0u;
    if (with_d)
        for (int p = tid; p < P; p += SPX_EVAL_ACC_THREADS) s_cls[p] = pcls[p];
    __syncthreads();

    const long long ntiles = (long long)N * tiles_y * tiles_x;
    for (long long t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int tx = (int)(t % tiles_x);
        const long long r = t / tiles_x;
        const int ty = (int)(r % tiles_y), n = (int)(r / tiles_y);
        const int ox = tx * 64 + (tid & 63), oy = ty * SPX_EVAL_TILE_H + (tid >> 6);
        const bool active = ox < W && oy < H;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        src_index(active ? oy : ty * SPX_EVAL_TILE_H, sh, h, y0, y1, ly0, ly1);
        src_index(active ? ox : tx * 64, sw, w, x0, x1, lx0, lx1);
        // the tile's source footprint (src_index is monotone in dst): workgroup-uniform
        int ya, yb, xa, xb, d0, d1;
        float f0, f1;
        src_index(ty * SPX_EVAL_TILE_H, sh, h, ya, d0, f0, f1);
        src_index(min(ty * SPX_EVAL_TILE_H + SPX_EVAL_TILE_H - 1, H - 1), sh, h, d0, yb, f0, f1);
        src_index(tx * 64, sw, w, xa, d0, f0, f1);
        src_index(min(tx * 64 + 63, W - 1), sw, w, d0, xb, f0, f1);
        const int nfx = xb - xa + 1, nfy = yb - ya + 1, nf = nfx * nfy;
        const float* lq = lg.p + (long long)n * lg.sn;
        int pred;
        if (nf * K <= SPX_EVAL_STAGE) {
            __syncthreads();                                   // the previous tile's scan is done with s_lg
            for (int i = tid; i < nf * K; i += SPX_EVAL_ACC_THREADS) {
                const int c = i % K, px = i / K, fx = px % nfx, fy = px / nfx;
                s_lg[c * nf + px] = lq[c * lg.sc + (ya + fy) * lg.sy + (xa + fx) * lg.sx];
            }
            __syncthreads();
            const unsigned r0 = (unsigned)((y0 - ya) * nfx), r1 = (unsigned)((y1 - ya) * nfx);
            pred = argext_at<true>(s_lg, nf, K, r0 + (x0 - xa), r0 + (x1 - xa), r1 + (x0 - xa), r1 + (x1 - xa), lx0, lx1, ly0, ly1);
        } else {
            const unsigned r0 = (unsigned)(y0 * lg.sy), r1 = (unsigned)(y1 * lg.sy), c0 = (unsigned)(x0 * lg.sx),
                           c1 = (unsigned)(x1 * lg.sx);
            pred = argext_at<true>(lq, lg.sc, K, r0 + c0, r0 + c1, r1 + c0, r1 + c1, lx0, lx1, ly0, ly1);
        }
        if (active) {
            const long long ann = spx_label(labels, label_bytes, ((size_t)n * H + oy) * W + ox);
            if (ann != 0) {
                const int row = (ann >= 1 && ann <= K) ? (int)(ann - 1) : K;
                if (full_conf) atomicAdd(&s_conf[row * K + pred], 1u);
                else if (row == pred) atomicAdd(&s_conf[pred], 1u);
                else atomicAdd(&conf[(size_t)row * K + pred], 1ull);
            }
        }
        if (with_d) {
            const float* dq = ds.p + (long long)n * ds.sn;
            int near = 0;
            if (nfx <= 16 && nfy <= 4) {                       // workgroup-uniform: every thread takes the barriers
                const unsigned r0 = (unsigned)((y0 - ya) * 16), r1 = (unsigned)((y1 - ya) * 16);
                const unsigned e00 = r0 + (x0 - xa), e01 = r0 + (x1 - xa), e10 = r1 + (x0 - xa), e11 = r1 + (x1 - xa);
                float best = 0.0f;
                for (int c0 = 0; c0 < P; c0 += SPX_EVAL_DCHUNK) {
                    const int nc = min(SPX_EVAL_DCHUNK, P - c0);
                    __syncthreads();                           // the previous chunk's (or the logits') scan is done
                    for (int i = tid; i < nc * 64; i += SPX_EVAL_ACC_THREADS) {
                        const int fx = i & 15, fy = (i >> 4) & 3, c = i >> 6;
                        if (fx < nfx && fy < nfy) s_lg[i] = dq[(long long)(c0 + c) * ds.sc + (ya + fy) * ds.sy + (xa + fx) * ds.sx];
                    }
                    __syncthreads();
                    argext_run<false>(s_lg, 64, c0, nc, e00, e01, e10, e11, lx0, lx1, ly0, ly1, best, near);
                }
            } else {
                const unsigned r0 = (unsigned)(y0 * ds.sy), r1 = (unsigned)(y1 * ds.sy), c0 = (unsigned)(x0 * ds.sx),
                               c1 = (unsigned)(x1 * ds.sx);
                near = argext_at<false>(dq, ds.sc, P, r0 + c0, r0 + c1, r1 + c0, r1 + c1, lx0, lx1, ly0, ly1);
            }
            if (active && s_cls[near] == pred) atomicAdd(&s_hits[near], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < nconf; i += SPX_EVAL_ACC_THREADS) {
        const unsigned int v = s_conf[i];
        if (v) atomicAdd(&conf[full_conf ? (size_t)i : (size_t)i * K + i], (unsigned long long)v);
    }
    if (with_d)
        for (int p = tid; p < P; p += SPX_EVAL_ACC_THREADS) {
            const unsigned int v = s_hits[p];
            if (v) atomicAdd(&hits[p], (unsigned long long)v);
        }
}

// One sample pixel per loop trip of a workgroup: its K logits and P distances interpolated into LDS, pred by the same
// strict scan as above, every distance ranked by counting (rank = #{q : d_q < d_p or (d_q == d_p and q < p)}, the stable
// ascending order), hit_rank = (cls(p) == pred), then an inclusive prefix sum of the hits added to the workgroup's
// topk copy.  Samples outside [0, H) x [0, W) are skipped and not counted as seen.
__global__ __launch_bounds__(SPX_EVAL_THREADS) void spx_eval_topk_kernel(
    SpxPlanes lg, SpxPlanes ds, const int32_t* __restrict__ pcls, const void* __restrict__ samples, int sample_bytes, int N, int S,
    int K, int P, int h, int w, int H, int W, float sh, float sw, unsigned long long* __restrict__ topk,
    unsigned long long* __restrict__ seen) {
    extern __shared__ unsigned int s_eval[];
    __shared__ int s_part[SPX_EVAL_THREADS];
    __shared__ int s_pred;
    const int tid = threadIdx.x;
    float* s_d = (float*)s_eval;
    unsigned int* s_acc = s_eval + P;
    int* s_hit = (int*)(s_acc + P);
    float* s_l = (float*)(s_hit + P);
    for (int p = tid; p < P; p += SPX_EVAL_THREADS) s_acc[p] = 0u;
    const int chunk = (P + SPX_EVAL_THREADS - 1) / SPX_EVAL_THREADS;
    const int k0 = tid * chunk < P ? tid * chunk : P, k1 = k0 + chunk < P ? k0 + chunk : P;
    unsigned int taken = 0;

    const long long total = (long long)N * S;
    for (long long s = blockIdx.x; s < total; s += gridDim.x) {
        const int n = (int)(s / S);
        long long yl, xl;
        if (sample_bytes == 4) {
            yl = ((const int32_t*)samples)[2 * s];
            xl = ((const int32_t*)samples)[2 * s + 1];
        } else {
            yl = ((const long long*)samples)[2 * s];
            xl = ((const long long*)samples)[2 * s + 1];
        }
        if (yl < 0 || yl >= H || xl < 0 || xl >= W) continue;   // uniform over the workgroup
        const int y = (int)yl, x = (int)xl;
        ++taken;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        src_index(y, sh, h, y0, y1, ly0, ly1);
        src_index(x, sw, w, x0, x1, lx0, lx1);
        {
            const float* q = lg.p + (long long)n * lg.sn;
            const unsigned o00 = (unsigned)(y0 * lg.sy + x0 * lg.sx), o01 = (unsigned)(y0 * lg.sy + x1 * lg.sx),
                           o10 = (unsigned)(y1 * lg.sy + x0 * lg.sx),
                           o11 = (unsigned)(y1 * lg.sy + x1 * lg.sx);
            for (int c = tid; c < K; c += SPX_EVAL_THREADS) s_l[c] = bilerp(q + c * lg.sc, o00, o01, o10, o11, lx0, lx1, ly0, ly1);
        }
        {
            const float* q = ds.p + (long long)n * ds.sn;
            const unsigned o00 = (unsigned)(y0 * ds.sy + x0 * ds.sx), o01 = (unsigned)(y0 * ds.sy + x1 * ds.sx),
                           o10 = (unsigned)(y1 * ds.sy + x0 * ds.sx),
                           o11 = (unsigned)(y1 * ds.sy + x1 * ds.sx);
            for (int p = tid; p < P; p += SPX_EVAL_THREADS) {
                s_d[p] = bilerp(q + p * ds.sc, o00, o01, o10, o11, lx0, lx1, ly0, ly1);
                s_hit[p] = 0;
            }
        }
        __syncthreads();
        if (tid == 0) {
            float best = 0.0f;
            int bi = 0;
            for (int c = 0; c < K; ++c) {
                const float v = s_l[c];
                if (c == 0 || v > best) {
                    best = v;
                    bi = c;
                }
            }
            s_pred = bi;
        }
        __syncthreads();
        const int pred = s_pred;
        for (int p = tid; p < P; p += SPX_EVAL_THREADS) {
            const float v = s_d[p];
            int rank = 0;
#pragma unroll 8
            for (int q = 0; q < P; ++q) {
                const float u = s_d[q];
                rank += (u < v) || (u == v && q < p);
            }
            // rank <= P - 1 always (p never counts itself); NaN distances may collide, never leave the array
            if (pcls[p] == pred) s_hit[rank] = 1;
        }
        __syncthreads();
        int sum = 0;
        for (int k = k0; k < k1; ++k) sum += s_hit[k];
        s_part[tid] = sum;
        __syncthreads();
        for (int off = 1; off < SPX_EVAL_THREADS; off <<= 1) {
            const int add = tid >= off ? s_part[tid - off] : 0;
            __syncthreads();
            s_part[tid] += add;
            __syncthreads();
        }
        int run = s_part[tid] - sum;
        for (int k = k0; k < k1; ++k) {
            run += s_hit[k];
            s_acc[k] += (unsigned int)run;
        }
        __syncthreads();                                        // before the next sample overwrites s_d / s_hit / s_l
    }
    __syncthreads();
    for (int p = tid; p < P; p += SPX_EVAL_THREADS) {
        const unsigned int v = s_acc[p];
        if (v) atomicAdd(&topk[p], (unsigned long long)v);
    }
    if (tid == 0 && seen && taken) atomicAdd(seen, (unsigned long long)taken);
}

// the whole matrix in LDS when it fits beside the hit counters, the class table and the staging area in 64 KiB
static int spx_eval_full_conf(int K, int P) {
    return (long long)(K + 1) * K <= SPX_EVAL_FULL_CONF_WORDS && (long long)(K + 1) * K + 2 * P + SPX_EVAL_STAGE <= 16384 ? 1 : 0;
}

hipError_t spx_launch_eval_accumulate(const float* logits, const long long* lst, const float* dist, const long long* dst,
                                      const int32_t* pcls, const void* labels, int label_bytes, int N, int K, int P, int h, int w,
                                      int H, int W, unsigned long long* conf, unsigned long long* hits, hipStream_t s) {
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int tiles_x = (W + 63) / 64, tiles_y = (H + SPX_EVAL_TILE_H - 1) / SPX_EVAL_TILE_H;
    const long long ntiles = (long long)N * tiles_y * tiles_x;
    const int full = spx_eval_full_conf(K, dist ? P : 0);
    const size_t lds = sizeof(unsigned int) * ((size_t)(full ? (K + 1) * K : K) + (dist ? 2 * (size_t)P : 0) + SPX_EVAL_STAGE);
    // persistent: as many workgroups as fit on the device at once (occupancy x CUs), each walking >= 1 tile
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 256;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, spx_eval_accumulate_kernel, SPX_EVAL_ACC_THREADS, lds) != hipSuccess || per_cu < 1)
        per_cu = 2;
    const long long cap = (long long)per_cu * cus;
    const unsigned grid = (unsigned)(ntiles < cap ? ntiles : cap);
    hipLaunchKernelGGL(spx_eval_accumulate_kernel, dim3(grid), dim3(SPX_EVAL_ACC_THREADS), lds, s, spx_planes(logits, lst),
                       spx_planes(dist, dst), pcls, labels, label_bytes, N, K, dist ? P : 0, h, w, H, W, sh, sw, tiles_x, tiles_y,
                       full, conf, hits);
    return hipGetLastError();
}

hipError_t spx_launch_eval_topk(const float* logits, const long long* lst, const float* dist, const long long* dst,
                                const int32_t* pcls, const void* samples, int sample_bytes, int N, int S, int K, int P, int h,
                                int w, int H, int W, unsigned long long* topk, unsigned long long* seen, hipStream_t s) {
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const long long total = (long long)N * S;
    const unsigned grid = (unsigned)(total < 256 ? total : 256);
    const size_t lds = sizeof(unsigned int) * (3 * (size_t)P + (size_t)K);
    hipLaunchKernelGGL(spx_eval_topk_kernel, dim3(grid), dim3(SPX_EVAL_THREADS), lds, s, spx_planes(logits, lst), spx_planes(dist, dst), pcls,
                       samples, sample_bytes, N, S, K, P, h, w, H, W, sh, sw, topk, seen);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// Label maps and per-image confusion (segmentation/eval_test.py:99-111, segmentation/analysis/failure_cases.py:96-141):
// the pass of spx_eval_accumulate_kernel over the logits (the same tiles, the same staged footprint, the same scan, so
// pred carries the bits of spx_upsample_argext), with two other outputs:
//   pred [N, H, W] uint8   id_map[k*], or k* without a map: one byte per pixel
//   conf [N, K+1, K]       the rule of spx_eval_accumulate per image
// A wave is one row of a tile.  Its 64 bytes are gathered with lane shuffles into the aligned dwords of memory they fall
// into (lane l forms the dword 4 l bytes above the row's address rounded down to a dword), whole dwords are stored as
// such and the ends of the row byte by byte: every byte is written exactly once whatever W and the pointer are.
// A workgroup walks a contiguous run of tiles (tiles are numbered image by image), so the counters it holds in LDS belong
// to one image; they are flushed and zeroed when the image changes and at the end.

__device__ __forceinline__ void spx_predict_flush(unsigned int* s_conf, int nconf, int K, int full_conf,
                                                  unsigned long long* __restrict__ conf_n) {
    for (int i = threadIdx.x; i < nconf; i += SPX_EVAL_ACC_THREADS) {
        const unsigned int v = s_conf[i];
        if (v && conf_n) atomicAdd(&conf_n[full_conf ? (size_t)i : (size_t)i * K + i], (unsigned long long)v);
        s_conf[i] = 0u;
    }
}

__global__ __launch_bounds__(SPX_EVAL_ACC_THREADS) void spx_predict_accumulate_kernel(
    SpxPlanes lg, const void* __restrict__ labels, int label_bytes, const uint8_t* __restrict__ id_map, int N, int K, int h, int w,
    int H, int W, float sh, float sw, int tiles_x, int tiles_y, long long chunk, int full_conf, uint8_t* __restrict__ pred_out,
    unsigned long long* __restrict__ conf) {
    extern __shared__ unsigned int s_eval[];
    const int tid = threadIdx.x;
    const int nconf = conf ? (full_conf ? (K + 1) * K : K) : 0;
    unsigned int* s_conf = s_eval;
    float* s_lg = (float*)(s_eval + nconf);
    const size_t conf_image = (size_t)(K + 1) * K;

    const long long ntiles = (long long)N * tiles_y * tiles_x;
    const long long t0 = (long long)blockIdx.x * chunk, t1 = min(t0 + chunk, ntiles);
    int held = -1;                                             // the image whose counters s_conf holds
    for (long long t = t0; t < t1; ++t) {
        const int tx = (int)(t % tiles_x);
        const long long r = t / tiles_x;
        const int ty = (int)(r % tiles_y), n = (int)(r / tiles_y);
        if (conf && n != held) {                               // workgroup-uniform
            __syncthreads();                                   // the previous tile's counts are in
            spx_predict_flush(s_conf, nconf, K, full_conf, held >= 0 ? conf + (size_t)held * conf_image : nullptr);
            __syncthreads();
            held = n;
        }
        const int ox = tx * 64 + (tid & 63), oy = ty * SPX_EVAL_TILE_H + (tid >> 6);
        const bool active = ox < W && oy < H;
        int y0, y1, x0, x1;
        float ly0, ly1, lx0, lx1;
        src_index(active ? oy : ty * SPX_EVAL_TILE_H, sh, h, y0, y1, ly0, ly1);
        src_index(active ? ox : tx * 64, sw, w, x0, x1, lx0, lx1);
        // the tile's source footprint (src_index is monotone in dst): workgroup-uniform
        int ya, yb, xa, xb, d0;
        float f0, f1;
        src_index(ty * SPX_EVAL_TILE_H, sh, h, ya, d0, f0, f1);
        src_index(min(ty * SPX_EVAL_TILE_H + SPX_EVAL_TILE_H - 1, H - 1), sh, h, d0, yb, f0, f1);
        src_index(tx * 64, sw, w, xa, d0, f0, f1);
        src_index(min(tx * 64 + 63, W - 1), sw, w, d0, xb, f0, f1);
        const int nfx = xb - xa + 1, nfy = yb - ya + 1, nf = nfx * nfy;
        const float* lq = lg.p + (long long)n * lg.sn;
        int pred;
        if (nf * K <= SPX_EVAL_STAGE) {
            __syncthreads();                                   // the previous tile's scan is done with s_lg
            for (int i = tid; i < nf * K; i += SPX_EVAL_ACC_THREADS) {
                const int c = i % K, px = i / K, fx = px % nfx, fy = px / nfx;
                s_lg[c * nf + px] = lq[c * lg.sc + (ya + fy) * lg.sy + (xa + fx) * lg.sx];
            }
            __syncthreads();
            const unsigned r0 = (unsigned)((y0 - ya) * nfx), r1 = (unsigned)((y1 - ya) * nfx);
            pred = argext_at<true>(s_lg, nf, K, r0 + (x0 - xa), r0 + (x1 - xa), r1 + (x0 - xa), r1 + (x1 - xa), lx0, lx1, ly0, ly1);
        } else {
            const unsigned r0 = (unsigned)(y0 * lg.sy), r1 = (unsigned)(y1 * lg.sy), c0 = (unsigned)(x0 * lg.sx),
                           c1 = (unsigned)(x1 * lg.sx);
            pred = argext_at<true>(lq, lg.sc, K, r0 + c0, r0 + c1, r1 + c0, r1 + c1, lx0, lx1, ly0, ly1);
        }
        if (conf && active) {
            const long long ann = spx_label(labels, label_bytes, ((size_t)n * H + oy) * W + ox);
            if (ann != 0) {
                const int row = (ann >= 1 && ann <= K) ? (int)(ann - 1) : K;
                if (full_conf) atomicAdd(&s_conf[row * K + pred], 1u);
                else if (row == pred) atomicAdd(&s_conf[pred], 1u);
                else atomicAdd(&conf[(size_t)n * conf_image + (size_t)row * K + pred], 1ull);
            }
        }
        if (pred_out && oy < H) {                              // wave-uniform: the wave's row of the tile is in the image
            const int lane = tid & 63, ncols = min(64, W - tx * 64);
            uint8_t* a0 = pred_out + ((size_t)n * H + oy) * W + (size_t)tx * 64;
            const int mis = (int)((uintptr_t)a0 & 3u);
            const int byte = id_map ? (int)id_map[pred] : pred;
            uint32_t word = 0u;
            int have = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int col = 4 * lane + j - mis;            // the tile column of byte j of this lane's dword
                const int v = __shfl(byte, col & 63);
                if (col >= 0 && col < ncols) {
                    word |= ((uint32_t)v & 255u) << (8 * j);
                    have |= 1 << j;
                }
            }
            uint8_t* q = a0 - mis + 4 * lane;                  // dword-aligned
            if (have == 15) {
                *(uint32_t*)q = word;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((have >> j) & 1) q[j] = (uint8_t)(word >> (8 * j));
            }
        }
    }
    if (conf && held >= 0) {
        __syncthreads();
        spx_predict_flush(s_conf, nconf, K, full_conf, conf + (size_t)held * conf_image);
    }
}

hipError_t spx_launch_predict_accumulate(const float* logits, const long long* lst, const void* labels, int label_bytes,
                                         const uint8_t* id_map, int N, int K, int h, int w, int H, int W, uint8_t* pred,
                                         unsigned long long* conf, hipStream_t s) {
    const float sh = (float)h / (float)H, sw = (float)w / (float)W;
    const int tiles_x = (W + 63) / 64, tiles_y = (H + SPX_EVAL_TILE_H - 1) / SPX_EVAL_TILE_H;
    const long long ntiles = (long long)N * tiles_y * tiles_x;
    const int full = spx_eval_full_conf(K, 0);
    const size_t lds = sizeof(unsigned int) * ((size_t)(conf ? (full ? (K + 1) * K : K) : 0) + SPX_EVAL_STAGE);
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
            cus = 256;
    }
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, spx_predict_accumulate_kernel, SPX_EVAL_ACC_THREADS, lds) != hipSuccess || per_cu < 1)
        per_cu = 2;
    // one contiguous run of tiles per workgroup, as many workgroups as the device holds at once
    const long long cap = (long long)per_cu * cus;
    const long long chunk = (ntiles + cap - 1) / cap;
    const unsigned grid = (unsigned)((ntiles + chunk - 1) / chunk);
    hipLaunchKernelGGL(spx_predict_accumulate_kernel, dim3(grid), dim3(SPX_EVAL_ACC_THREADS), lds, s, spx_planes(logits, lst), labels,
                       label_bytes, id_map, N, K, h, w, H, W, sh, sw, tiles_x, tiles_y, chunk, full, pred, conf);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------------
// The failure table (failure_cases.py:131-160) from the per-image confusion, one thread per (image, class):
//   present = sum_j conf[n, k, j] > 0;  I = conf[n, k, k];  U = sum_j conf[n, k, j] + sum_{r <= K} conf[n, r, k] - I
//   iou = I / U in float64 (the division correctly rounded), fail = iou < threshold (strict),
//   miss = the lowest j != k with the largest conf[n, k, j] > 0, or -1;  a class that is not present: NaN, -1, 0.
__global__ __launch_bounds__(SPX_EVAL_THREADS) void spx_failure_table_kernel(const long long* __restrict__ conf, int N, int K,
                                                                             double threshold, double* __restrict__ iou,
                                                                             int32_t* __restrict__ miss, uint8_t* __restrict__ fail) {
    const long long i = (long long)blockIdx.x * SPX_EVAL_THREADS + threadIdx.x;
    if (i >= (long long)N * K) return;
    const int n = (int)(i / K), k = (int)(i - (long long)n * K);
    const long long* cn = conf + (size_t)n * (K + 1) * K;
    long long row = 0, col = 0, top = 0;
    int arg = -1;
    for (int j = 0; j < K; ++j) {
        const long long v = cn[(size_t)k * K + j];
        row += v;
        if (j != k && v > top) {                               // strict: the lowest class among equal counts
            top = v;
            arg = j;
        }
    }
    for (int r = 0; r <= K; ++r) col += cn[(size_t)r * K + k];
    if (row > 0) {
        const long long I = cn[(size_t)k * K + k];
        const double v = (double)I / (double)(row + col - I);
        iou[i] = v;
        miss[i] = arg;
        fail[i] = v < threshold ? 1 : 0;
    } else {
        iou[i] = __longlong_as_double(0x7ff8000000000000LL);
        miss[i] = -1;
        fail[i] = 0;
    }
}

hipError_t spx_launch_failure_table(const long long* conf, int N, int K, double threshold, double* iou, int32_t* miss, uint8_t* fail,
                                    hipStream_t s) {
    const long long total = (long long)N * K;
    hipLaunchKernelGGL(spx_failure_table_kernel, dim3((unsigned)((total + SPX_EVAL_THREADS - 1) / SPX_EVAL_THREADS)),
                       dim3(SPX_EVAL_THREADS), 0, s, conf, N, K, threshold, iou, miss, fail);
    return hipGetLastError();
}
