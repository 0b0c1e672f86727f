// Explanation maps (segmentation/analysis/sample_activations_prototype.py:71-133, sample_activations_group.py:72-131): the
// two pictures a user looks at, as bytes.  The reference resizes every activation plane to the image (OpenCV INTER_CUBIC) on
// the host, masks it with the class, min-max normalises it, converts with np.uint8(255 * x), and takes an argmax over the
// stacked planes of the class.  Here every pass recomputes a pixel from the latent plane with ovl_value()
// (spx_overlap_sample.h; ONE function, compiled with -ffp-contract=off, so the range pass and the byte pass see the same bits)
// and the fp32 [H, W] map is never written: one byte per pixel leaves the chip.
//
//   heat row r = (n, c, class k):   m = labels[n] == k + 1 ? u[n, c] : 0;  lo = min m, hi = max m over the image;
//                                   d = hi - lo;  heat = (uint8) trunc(255 * ((m - lo) / d)) in fp32;  d == 0: all zeros
//   dominant row r = (n, class k):  dom = labels[n] == k + 1 ? the first argmax over the class's slots j of wgt[k, j] * u_j : 255
//
//   spx_explain_range     lo / hi of every heat row: the staged bands of output rows and their pixel walk of
//                         spx_overlap_sample.h (ovl_stage_band, ovl_walk_band), minima and maxima of the order-preserving
//                         uint32 key folded by wave shuffles, then integer atomics per row (min and max do not depend on the
//                         order: run-to-run identical, no float atomics).
//   spx_explain_heat      the bytes of every heat row.
//   spx_explain_dominant  the bytes of every dominant row: the taps of a pixel are formed once, the slots change the plane only.
// The two byte kernels share exp_store(): lanes are assigned by the ADDRESS of the output dword, so each lane forms four
// consecutive bytes and stores them as one dword whatever W and the output pointer are; the dwords that straddle the ends of
// an image are written byte by byte by the image each byte belongs to.  Every output byte is written exactly once.
//
// At the end of the file: the paired heat maps of the failure cases (failure_cases.py:188-420), spx_paired_range and
// spx_paired_heat, which look like the heat maps above and are not: another mask, shared ranges, another divisor.
#include "spx_overlap_sample.h"

#define EXP_THREADS 256
#define EXP_BAND 32               // most output rows of one band of the range pass: many bands per image, a row table has few rows
#define EXP_DWORDS 4              // output dwords per lane of a byte kernel: 4 KiB per workgroup
#define EXP_OFF 255u              // the dominant map outside the class

struct ExpLabels {
    const void* p;
    int bytes;
};

// ---- range -------------------------------------------------------------------------------------------------------------
// Band blockIdx.x of heat row blockIdx.y.  keys uint32 [2][R]: running minimum (initialised to all ones) and maximum (zero) of
// float_key(m).  The labels are read along X, as the walk goes.
__global__ __launch_bounds__(EXP_THREADS) void spx_explain_range_kernel(SpxPlanes a, ExpLabels labels, const int32_t* __restrict__ rows,
                                                                        int R, int N, int C, int h, int w, int H, int W, int band_rows,
                                                                        uint32_t* __restrict__ keys) {
    __shared__ float s_stage[OVL_STAGE];
    __shared__ int s_oy[EXP_BAND * 4];
    __shared__ float s_wy[EXP_BAND * 4];
    __shared__ uint32_t s_lo[EXP_THREADS / 64], s_hi[EXP_THREADS / 64];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int n = rows[r * 3 + 0], c = rows[r * 3 + 1];
    const long long want = (long long)rows[r * 3 + 2] + 1;
    if (!ovl_plane_ok(n, c, N, C)) return;                      // workgroup-uniform; the entry point has refused such a row
    const int Y0 = blockIdx.x * band_rows, nrows = min(H, Y0 + band_rows) - Y0;
    ovl_stage_band<EXP_THREADS>(a, n, c, h, w, H, Y0, nrows, s_oy, s_wy, s_stage, nullptr, 0);
    const int wave = tid >> 6, lane = tid & 63;
    const size_t label0 = (size_t)n * H * W;
    uint32_t klo = 0xffffffffu, khi = 0u;
    ovl_walk_band<EXP_THREADS>(w, W, nrows, [&](int i, int X, const int* ox, const float* wx) {
        float m = 0.0f;
        if (spx_label(labels.p, labels.bytes, label0 + (size_t)(Y0 + i) * W + X) == want)
            m = ovl_value(s_stage, &s_oy[4 * i], &s_wy[4 * i], ox, wx);
        const uint32_t key = float_key(m);
        klo = min(klo, key);
        khi = max(khi, key);
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        klo = min(klo, (uint32_t)__shfl_xor(klo, off));
        khi = max(khi, (uint32_t)__shfl_xor(khi, off));
    }
    if (lane == 0) {
        s_lo[wave] = klo;
        s_hi[wave] = khi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < EXP_THREADS / 64; ++v) {
            klo = min(klo, s_lo[v]);
            khi = max(khi, s_hi[v]);
        }
        atomicMin(&keys[r], klo);
        atomicMax(&keys[(size_t)R + r], khi);
    }
}

hipError_t spx_launch_explain_range(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                    int R, int N, int C, int h, int w, int H, int W, void* workspace, hipStream_t s) {
    const int band = ovl_band_plan(h, w, H, EXP_BAND);
    if (!band) return hipErrorInvalidValue;
    uint32_t* keys = (uint32_t*)workspace;
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)R * 4, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(keys + R, 0, (size_t)R * 4, s);
    if (e != hipSuccess) return e;
    const ExpLabels lab = {labels, label_bytes};
    hipLaunchKernelGGL(spx_explain_range_kernel, dim3((unsigned)((H + band - 1) / band), (unsigned)R), dim3(EXP_THREADS), 0, s,
                       spx_planes(planes, st), lab, rows, R, N, C, h, w, H, W, band, keys);
    return hipGetLastError();
}

// ---- bytes -------------------------------------------------------------------------------------------------------------
// The workgroup's share of output image `row` (the H*W bytes from out + row * H*W).  Addresses are counted from `out` rounded
// down to a dword, so a dword index names an aligned dword of memory; dword q of the image holds the bytes [4q, 4q + 4) of that
// count, of which [first, last) are the image's.  px(Y, X) is the byte of a pixel; it is called with X ascending inside a row.
template <class Pixel>
__device__ __forceinline__ void exp_store(uint8_t* __restrict__ out, size_t row, int H, int W, Pixel& px) {
    const long long HW = (long long)H * W;
    const long long mis = (long long)((uintptr_t)out & 3u);
    uint8_t* base = out - mis;                                   // dword-aligned
    const long long b0 = (long long)row * HW + mis, b1 = b0 + HW;
#pragma unroll 1
    for (int it = 0; it < EXP_DWORDS; ++it) {
        const long long f0 = ((b0 >> 2) + ((long long)blockIdx.x * EXP_DWORDS + it) * EXP_THREADS + threadIdx.x) * 4;
        if (f0 >= b1) break;
        const long long first = f0 > b0 ? f0 : b0, last = f0 + 4 < b1 ? f0 + 4 : b1;
        const int local = (int)(first - b0);                     // < H*W < 2^31
        int Y = local / W, X = local - Y * W;
        uint32_t word = 0u;
        for (long long f = first; f < last; ++f) {
            word |= (px(Y, X) & 255u) << (8 * (int)(f - f0));
            if (++X == W) {
                X = 0;
                ++Y;
            }
        }
        if (last - first == 4) {
            *(uint32_t*)(base + f0) = word;
        } else {
            for (long long f = first; f < last; ++f) base[f] = (uint8_t)(word >> (8 * (int)(f - f0)));
        }
    }
}
// dwords that can touch one image, whatever its misalignment
static inline long long exp_image_dwords(int H, int W) { return ((long long)H * W + 6) / 4; }

// the taps of a pixel with global strides; the y taps are kept while Y stays
struct ExpTaps {
    int Y, oy[4], ox[4];
    float wy[4], wx[4];
    __device__ __forceinline__ void at(const SpxPlanes& a, int h, int w, int H, int W, int Yn, int Xn) {
        if (Yn != Y) {
            ovl_axis(Yn, h, H, 0, (int)a.sy, oy, wy);
            Y = Yn;
        }
        ovl_axis(Xn, w, W, 0, (int)a.sx, ox, wx);
    }
};

// np.uint8(255 * ((m - lo) / d)) in float32: every operation rounded on its own, the division correctly rounded
__device__ __forceinline__ uint32_t exp_heat_byte(float m, float lo, float d) {
    const float r = m - lo;
    const float x = r / d;
    return (uint32_t)(int)(255.0f * x);
}

struct ExpHeatPixel {
    SpxPlanes a;
    ExpLabels labels;
    const float* plane;
    size_t label0;
    long long want;
    float lo, d;
    uint32_t outside;             // the byte of m = 0
    int h, w, H, W;
    ExpTaps taps;
    __device__ __forceinline__ uint32_t operator()(int Y, int X) {
        if (d == 0.0f) return 0u;
        if (spx_label(labels.p, labels.bytes, label0 + (size_t)Y * W + X) != want) return outside;
        taps.at(a, h, w, H, W, Y, X);
        return exp_heat_byte(ovl_value(plane, taps.oy, taps.wy, taps.ox, taps.wx), lo, d);
    }
};

__global__ __launch_bounds__(EXP_THREADS) void spx_explain_heat_kernel(SpxPlanes a, ExpLabels labels, const int32_t* __restrict__ rows,
                                                                       int R, int N, int C, int h, int w, int H, int W,
                                                                       const uint32_t* __restrict__ keys, uint8_t* __restrict__ heat,
                                                                       float* __restrict__ ranges) {
    const int r = blockIdx.y;
    const int n = rows[r * 3 + 0], c = rows[r * 3 + 1];
    if (!ovl_plane_ok(n, c, N, C)) return;                      // workgroup-uniform; the entry point has refused such a row
    ExpHeatPixel px;
    px.a = a;
    px.labels = labels;
    px.plane = a.p + (long long)n * a.sn + (long long)c * a.sc;
    px.label0 = (size_t)n * H * W;
    px.want = (long long)rows[r * 3 + 2] + 1;
    px.lo = key_float(keys[r]);
    const float hi = key_float(keys[(size_t)R + r]);
    px.d = hi - px.lo;
    px.outside = px.d == 0.0f ? 0u : exp_heat_byte(0.0f, px.lo, px.d);
    px.h = h;
    px.w = w;
    px.H = H;
    px.W = W;
    px.taps.Y = -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        ranges[(size_t)r * 2 + 0] = px.lo;
        ranges[(size_t)r * 2 + 1] = hi;
    }
    exp_store(heat, (size_t)r, H, W, px);
}

hipError_t spx_launch_explain_heat(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                   int R, int N, int C, int h, int w, int H, int W, const void* workspace, uint8_t* heat, float* ranges,
                                   hipStream_t s) {
    const long long per = (long long)EXP_THREADS * EXP_DWORDS;
    const ExpLabels lab = {labels, label_bytes};
    hipLaunchKernelGGL(spx_explain_heat_kernel, dim3((unsigned)((exp_image_dwords(H, W) + per - 1) / per), (unsigned)R), dim3(EXP_THREADS),
                       0, s, spx_planes(planes, st), lab, rows, R, N, C, h, w, H, W, (const uint32_t*)workspace, heat, ranges);
    return hipGetLastError();
}

struct ExpDominantPixel {
    SpxPlanes a;
    ExpLabels labels;
    const float* image;           // a.p + n * sn
    const int32_t* slots;         // the class's row of the slot table
    const float* weights;         // the class's row of the weights, or NULL = 1
    size_t label0;
    long long want;
    int C, J, h, w, H, W;
    ExpTaps taps;
    __device__ __forceinline__ uint32_t operator()(int Y, int X) {
        if (spx_label(labels.p, labels.bytes, label0 + (size_t)Y * W + X) != want) return EXP_OFF;
        taps.at(a, h, w, H, W, Y, X);
        uint32_t best = EXP_OFF;
        float top = 0.0f;
        for (int j = 0; j < J; ++j) {
            const int ch = slots[j];                             // wave-uniform
            if (ch < 0 || ch >= C) continue;
            const float v = (weights ? weights[j] : 1.0f) * ovl_value(image + (long long)ch * a.sc, taps.oy, taps.wy, taps.ox, taps.wx);
            // np.argmax: the first maximum, and a NaN counts as one
            if (best == EXP_OFF || v > top || (v != v && top == top)) {
                best = (uint32_t)j;
                top = v;
            }
        }
        return best;
    }
};

__global__ __launch_bounds__(EXP_THREADS) void spx_explain_dominant_kernel(SpxPlanes a, ExpLabels labels, const int32_t* __restrict__ rows,
                                                                           const int32_t* __restrict__ table,
                                                                           const float* __restrict__ weights, int N, int C, int K, int J,
                                                                           int h, int w, int H, int W, uint8_t* __restrict__ dom) {
    const int r = blockIdx.y;
    const int n = rows[r * 2 + 0], k = rows[r * 2 + 1];
    if (n < 0 || n >= N || k < 0 || k >= K) return;             // workgroup-uniform; the entry point has refused such a row
    ExpDominantPixel px;
    px.a = a;
    px.labels = labels;
    px.image = a.p + (long long)n * a.sn;
    px.slots = table + (size_t)k * J;
    px.weights = weights ? weights + (size_t)k * J : nullptr;
    px.label0 = (size_t)n * H * W;
    px.want = (long long)k + 1;
    px.C = C;
    px.J = J;
    px.h = h;
    px.w = w;
    px.H = H;
    px.W = W;
    px.taps.Y = -1;
    exp_store(dom, (size_t)r, H, W, px);
}

hipError_t spx_launch_explain_dominant(const float* planes, const long long* st, const void* labels, int label_bytes,
                                       const int32_t* rows, const int32_t* table, const float* weights, int R, int N, int C, int K, int J,
                                       int h, int w, int H, int W, uint8_t* dom, hipStream_t s) {
    const long long per = (long long)EXP_THREADS * EXP_DWORDS;
    const ExpLabels lab = {labels, label_bytes};
    hipLaunchKernelGGL(spx_explain_dominant_kernel, dim3((unsigned)((exp_image_dwords(H, W) + per - 1) / per), (unsigned)R),
                       dim3(EXP_THREADS), 0, s, spx_planes(planes, st), lab, rows, table, weights, N, C, K, J, h, w, H, W, dom);
    return hipGetLastError();
}

// ---- paired heat maps (segmentation/analysis/failure_cases.py:188-420) ----------------------------------------------------
// The failure cases draw the slots of two classes over the pixels of ONE of them, on a range shared between rows, and divide by
// the maximum, not by the width of the range:
//   row r = (n, c, a, q):   m = labels[n] == a + 1 ? u[n, c] : 0;   lo_q = min m, hi_q = max m over all pixels of all rows of slot q;
//                           x = (m - lo_q) / hi_q in fp32;  heat = (uint8) trunc(255 * x), 255 where 255 x >= 256 (only when
//                           lo_q < 0);  hi_q <= 0: all zeros
// The two kernels are the range and heat kernels above with the slot between the row and its range: keys uint32 [2][Q].
__global__ __launch_bounds__(EXP_THREADS) void spx_paired_range_kernel(SpxPlanes a, ExpLabels labels, const int32_t* __restrict__ rows,
                                                                       int Q, int N, int C, int h, int w, int H, int W, int band_rows,
                                                                       uint32_t* __restrict__ keys) {
    __shared__ float s_stage[OVL_STAGE];
    __shared__ int s_oy[EXP_BAND * 4];
    __shared__ float s_wy[EXP_BAND * 4];
    __shared__ uint32_t s_lo[EXP_THREADS / 64], s_hi[EXP_THREADS / 64];
    const int tid = threadIdx.x, r = blockIdx.y;
    const int n = rows[r * 4 + 0], c = rows[r * 4 + 1], q = rows[r * 4 + 3];
    const long long want = (long long)rows[r * 4 + 2] + 1;
    if (!ovl_plane_ok(n, c, N, C) || q < 0 || q >= Q) return;   // workgroup-uniform; the entry point has refused such a row
    const int Y0 = blockIdx.x * band_rows, nrows = min(H, Y0 + band_rows) - Y0;
    ovl_stage_band<EXP_THREADS>(a, n, c, h, w, H, Y0, nrows, s_oy, s_wy, s_stage, nullptr, 0);
    const int wave = tid >> 6, lane = tid & 63;
    const size_t label0 = (size_t)n * H * W;
    uint32_t klo = 0xffffffffu, khi = 0u;
    ovl_walk_band<EXP_THREADS>(w, W, nrows, [&](int i, int X, const int* ox, const float* wx) {
        float m = 0.0f;
        if (spx_label(labels.p, labels.bytes, label0 + (size_t)(Y0 + i) * W + X) == want)
            m = ovl_value(s_stage, &s_oy[4 * i], &s_wy[4 * i], ox, wx);
        const uint32_t key = float_key(m);
        klo = min(klo, key);
        khi = max(khi, key);
    });
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        klo = min(klo, (uint32_t)__shfl_xor(klo, off));
        khi = max(khi, (uint32_t)__shfl_xor(khi, off));
    }
    if (lane == 0) {
        s_lo[wave] = klo;
        s_hi[wave] = khi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int v = 1; v < EXP_THREADS / 64; ++v) {
            klo = min(klo, s_lo[v]);
            khi = max(khi, s_hi[v]);
        }
        atomicMin(&keys[q], klo);
        atomicMax(&keys[(size_t)Q + q], khi);
    }
}

hipError_t spx_launch_paired_range(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                   int R, int Q, int N, int C, int h, int w, int H, int W, void* workspace, hipStream_t s) {
    const int band = ovl_band_plan(h, w, H, EXP_BAND);
    if (!band) return hipErrorInvalidValue;
    uint32_t* keys = (uint32_t*)workspace;
    hipError_t e = hipMemsetAsync(keys, 0xff, (size_t)Q * 4, s);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(keys + Q, 0, (size_t)Q * 4, s);
    if (e != hipSuccess) return e;
    const ExpLabels lab = {labels, label_bytes};
    hipLaunchKernelGGL(spx_paired_range_kernel, dim3((unsigned)((H + band - 1) / band), (unsigned)R), dim3(EXP_THREADS), 0, s,
                       spx_planes(planes, st), lab, rows, Q, N, C, h, w, H, W, band, keys);
    return hipGetLastError();
}

// np.uint8(255 * ((m - lo) / hi)) in float32, with the conversion's undefined case defined: 255 from 256 up
__device__ __forceinline__ uint32_t exp_paired_byte(float m, float lo, float hi) {
    const float r = m - lo;
    const float x = r / hi;
    const float v = 255.0f * x;
    return v >= 256.0f ? 255u : (uint32_t)(int)v;
}

struct ExpPairedPixel {
    SpxPlanes a;
    ExpLabels labels;
    const float* plane;
    size_t label0;
    long long want;
    float lo, hi;
    uint32_t outside;             // the byte of m = 0
    int h, w, H, W;
    ExpTaps taps;
    __device__ __forceinline__ uint32_t operator()(int Y, int X) {
        if (!(hi > 0.0f)) return 0u;
        if (spx_label(labels.p, labels.bytes, label0 + (size_t)Y * W + X) != want) return outside;
        taps.at(a, h, w, H, W, Y, X);
        return exp_paired_byte(ovl_value(plane, taps.oy, taps.wy, taps.ox, taps.wx), lo, hi);
    }
};

__global__ __launch_bounds__(EXP_THREADS) void spx_paired_heat_kernel(SpxPlanes a, ExpLabels labels, const int32_t* __restrict__ rows,
                                                                      int Q, int N, int C, int h, int w, int H, int W,
                                                                      const uint32_t* __restrict__ keys, uint8_t* __restrict__ heat,
                                                                      float* __restrict__ ranges) {
    const int r = blockIdx.y;
    const int n = rows[r * 4 + 0], c = rows[r * 4 + 1], q = rows[r * 4 + 3];
    if (!ovl_plane_ok(n, c, N, C) || q < 0 || q >= Q) return;   // workgroup-uniform; the entry point has refused such a row
    ExpPairedPixel px;
    px.a = a;
    px.labels = labels;
    px.plane = a.p + (long long)n * a.sn + (long long)c * a.sc;
    px.label0 = (size_t)n * H * W;
    px.want = (long long)rows[r * 4 + 2] + 1;
    px.lo = key_float(keys[q]);
    px.hi = key_float(keys[(size_t)Q + q]);
    px.outside = px.hi > 0.0f ? exp_paired_byte(0.0f, px.lo, px.hi) : 0u;
    px.h = h;
    px.w = w;
    px.H = H;
    px.W = W;
    px.taps.Y = -1;
    if (blockIdx.x == 0 && threadIdx.x == 0) {                  // every row of the slot writes the same two floats
        ranges[(size_t)q * 2 + 0] = px.lo;
        ranges[(size_t)q * 2 + 1] = px.hi;
    }
    exp_store(heat, (size_t)r, H, W, px);
}

hipError_t spx_launch_paired_heat(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                  int R, int Q, int N, int C, int h, int w, int H, int W, const void* workspace, uint8_t* heat,
                                  float* ranges, hipStream_t s) {
    const long long per = (long long)EXP_THREADS * EXP_DWORDS;
    const ExpLabels lab = {labels, label_bytes};
    hipLaunchKernelGGL(spx_paired_heat_kernel, dim3((unsigned)((exp_image_dwords(H, W) + per - 1) / per), (unsigned)R), dim3(EXP_THREADS),
                       0, s, spx_planes(planes, st), lab, rows, Q, N, C, h, w, H, W, (const uint32_t*)workspace, heat, ranges);
    return hipGetLastError();
}
