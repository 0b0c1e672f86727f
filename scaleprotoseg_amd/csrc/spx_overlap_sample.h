// What the activation-overlap metrics (spx_overlap.hip), the class-restricted thresholds (spx_masked_select.hip), the push
// bounding boxes (spx_pushbox.hip) and the explanation maps (spx_explain.hip) share: the upsampled value of a pixel recomputed
// from the latent plane, the bands of output rows that stage their latent rows in LDS (their plan, staging and pixel walk) and
// the radix select (its key, histogram round, scan round and lerp), each stated once (the strided view of the planes and the
// label read come from spx_planes.h).  ONE function, compiled with -ffp-contract=off, gives a pixel the same bits in every pass
// of every file.
#ifndef SPX_OVERLAP_SAMPLE_H
#define SPX_OVERLAP_SAMPLE_H
#include "spx_planes.h"

// ---- the upsampled value ---------------------------------------------------------------------------------------------
// Source coordinate of output index d for `in` source and `out` output samples: s = (d + 0.5) * in / out - 0.5, taken
// EXACTLY as the fraction num / den with num = (2d + 1) * in - out, den = 2 * out: i = floor(s), t = s - i = r / den with one
// rounding (fits int32: the entry points bound out <= 32768, in <= 16384).  Taps i - 1 .. i + 2, clamped to the grid.
__device__ __forceinline__ void ovl_coord(int d, int in, int out, int& i, float& t) {
    const int num = (2 * d + 1) * in - out, den = 2 * out;
    int r;
    if (num < 0) {                // only -out < num < 0: i = -1
        i = -1;
        r = num + den;
    } else {
        i = (int)((unsigned)num / (unsigned)den);
        r = num - i * den;
    }
    t = (float)r / (float)den;
}
// Keys' cubic convolution weights at a = -0.75 (OpenCV's INTER_CUBIC, torch's bicubic) for the taps at distance
// t + 1, t, 1 - t, 2 - t.
__device__ __forceinline__ float ovl_cc1(float x) { return ((1.25f * x - 2.25f) * x) * x + 1.0f; }            // |x| <= 1
__device__ __forceinline__ float ovl_cc2(float x) { return ((-0.75f * x + 3.75f) * x - 6.0f) * x + 3.0f; }    // 1 < |x| < 2
__device__ __forceinline__ void ovl_weights(float t, float* wgt) {
    wgt[0] = ovl_cc2(t + 1.0f);
    wgt[1] = ovl_cc1(t);
    wgt[2] = ovl_cc1(1.0f - t);
    wgt[3] = ovl_cc2(2.0f - t);
}
__device__ __forceinline__ int ovl_clamp(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }
// taps of one axis: element offsets (clamped index - origin) * stride and the four weights
__device__ __forceinline__ void ovl_axis(int d, int in, int out, int origin, int stride, int* off, float* wgt) {
    int i;
    float t;
    ovl_coord(d, in, out, i, t);
    ovl_weights(t, wgt);
#pragma unroll
    for (int a = 0; a < 4; ++a) off[a] = (ovl_clamp(i - 1 + a, in - 1) - origin) * stride;
}
// THE value of an upsampled pixel: rows first, left to right, then the four rows top to bottom.  p may point to LDS or to
// memory; the arithmetic is the same sequence of fp32 operations either way.
__device__ __forceinline__ float ovl_value(const float* p, const int* oy, const float* wy, const int* ox, const float* wx) {
    float v = 0.0f;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float* q = p + oy[a];
        const float row = ((q[ox[0]] * wx[0] + q[ox[1]] * wx[1]) + q[ox[2]] * wx[2]) + q[ox[3]] * wx[3];
        v = a == 0 ? row * wy[0] : v + row * wy[a];
    }
    return v;
}

// ---- bands of output rows whose latent footprint is staged in LDS --------------------------------------------------------
#define OVL_STAGE 8192            // floats of latent rows staged per band (32 KiB)
#define OVL_BAND 256              // most output rows of one band (the y-tap table's size)

// rows of a band so that its latent footprint (rows i_first - 1 .. i_last + 2) fits the stage
static inline int ovl_band_rows(int h, int w, int H) {
    const int cap = OVL_STAGE / w;                               // >= 5: the entry point bounds w
    if (cap >= h) return H < OVL_BAND ? H : OVL_BAND;
    // (r - 1) * h / H <= cap - 5, so first and last row of a band are at most cap - 4 latent rows apart (the floors of two
    // coordinates x apart differ by at most ceil(x)) and with the taps -1 .. +2 at most cap rows are staged
    const long long r = 1 + (long long)(cap - 5) * H / h;
    return (int)(r < OVL_BAND ? r : OVL_BAND);
}
// the most latent rows any band of `band` output rows stages, by the kernel's own coordinate rule (host copy of ovl_coord's
// integer part): the launch refuses a band that would not fit instead of trusting the bound above
static inline int ovl_max_staged_rows(int h, int H, int band) {
    int most = 0;
    for (int Y0 = 0; Y0 < H; Y0 += band) {
        const int Y1 = Y0 + band < H ? Y0 + band : H;
        const long long n0 = (2LL * Y0 + 1) * h - H, n1 = (2LL * (Y1 - 1) + 1) * h - H, den = 2LL * H;
        const int i0 = n0 < 0 ? -1 : (int)(n0 / den), i1 = n1 < 0 ? -1 : (int)(n1 / den);
        const int lo = i0 - 1 < 0 ? 0 : (i0 - 1 > h - 1 ? h - 1 : i0 - 1), hi = i1 + 2 > h - 1 ? h - 1 : (i1 + 2 < 0 ? 0 : i1 + 2);
        if (hi - lo + 1 > most) most = hi - lo + 1;
    }
    return most;
}
// output rows per band, at most `most` (the size of the kernel's y-tap table), or 0: no band fits the stage, the launch fails
static inline int ovl_band_plan(int h, int w, int H, int most = OVL_BAND) {
    const int rows = ovl_band_rows(h, w, H), band = rows < most ? rows : most;
    return band >= 1 && (long long)ovl_max_staged_rows(h, H, band) * w <= OVL_STAGE ? band : 0;
}

__device__ __forceinline__ bool ovl_plane_ok(int n, int c, int N, int C) { return n >= 0 && n < N && c >= 0 && c < C; }

// The workgroup of THREADS threads stages the output rows Y0 .. Y0 + nrows - 1 of plane (n, c): the latent rows of their taps,
// halo included, densely into s_stage (at most OVL_STAGE floats: ovl_band_plan), and the y taps of row Y0 + r, as offsets into
// s_stage, into s_oy / s_wy [4 r ..].  It also zeroes the nzero LDS words at s_zero that the caller accumulates into (none:
// nullptr, 0), after the band's bounds and before the tap table: the place where the kernels measure as before.  Ends with a
// barrier: the band is there for every thread.
template <int THREADS>
__device__ __forceinline__ void ovl_stage_band(const SpxPlanes& a, int n, int c, int h, int w, int H, int Y0, int nrows, int* s_oy,
                                               float* s_wy, float* s_stage, uint32_t* s_zero, int nzero) {
    const int tid = threadIdx.x;
    int i0, i1;
    float t;
    ovl_coord(Y0, h, H, i0, t);
    ovl_coord(Y0 + nrows - 1, h, H, i1, t);
    const int lo = ovl_clamp(i0 - 1, h - 1), hi = ovl_clamp(i1 + 2, h - 1);
    const int nstage = (hi - lo + 1) * w;
    for (int i = tid; i < nzero; i += THREADS) s_zero[i] = 0u;
    for (int r = tid; r < nrows; r += THREADS) ovl_axis(Y0 + r, h, H, lo, w, &s_oy[4 * r], &s_wy[4 * r]);
    const float* src = a.p + (long long)n * a.sn + (long long)c * a.sc;
    for (int i = tid; i < nstage; i += THREADS) {
        const int y = i / w, x = i - y * w;
        s_stage[i] = src[(long long)(lo + y) * a.sy + (long long)x * a.sx];
    }
    __syncthreads();
}
// The walk over a staged band: lane l takes the columns X = l, l + 64, ..., wave v the band's rows r = v, v + THREADS / 64, ...
// of each; px(r, X, ox, wx) gets the x taps for ovl_value(s_stage, &s_oy[4 * r], &s_wy[4 * r], ox, wx).  A thread sees the rows
// of a column one after the other: the runs of ovl_count rest on that.
template <int THREADS, class Pixel>
__device__ __forceinline__ void ovl_walk_band(int w, int W, int nrows, Pixel&& px) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int X = lane; X < W; X += 64) {
        int ox[4];
        float wx[4];
        ovl_axis(X, w, W, 0, 1, ox, wx);
        for (int r = wave; r < nrows; r += THREADS / 64) px(r, X, ox, wx);
    }
}

// ---- the exact radix select over the upsampled values (spx_overlap.hip, spx_masked_select.hip) ---------------------------
// Three histogram rounds of 11 / 11 / 10 bits of the order-preserving uint32 key of the fp32 value, a one-workgroup scan after
// each.  Per selected row: state uint32 [4] = (key prefix, rank inside it) of the two order statistics, with zero prefixes
// before round 0, and hist uint32 [2][OVL_BINS], zero before every round.
#define OVL_THREADS 256
#define OVL_BINS 2048             // bins of a histogram round (the last round uses 1024)

// order-preserving key of an fp32 value (-0.0 sorts directly below +0.0, NaNs at the two ends) and its inverse
__device__ __forceinline__ uint32_t ovl_key(float v) {
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ovl_unkey(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// one run of equal bins per thread: consecutive rows of a column mostly fall into one bin of the coarse rounds
__device__ __forceinline__ void ovl_count(uint32_t* hist, int& cur, uint32_t& run, int bin) {
    if (bin != cur) {
        if (run) atomicAdd(&hist[cur], run);
        cur = bin;
        run = 0u;
    }
    ++run;
}
__device__ __forceinline__ void ovl_clear_hist(uint32_t* hq) {
    for (int i = threadIdx.x; i < 2 * OVL_BINS; i += OVL_THREADS) hq[i] = 0u;
}

struct OvlClass {                 // what a round over the pixels of one class reads and counts; unused by a round over all pixels
    const void* labels;
    int label_bytes;
    long long want;               // the label of the class
    uint32_t* count;              // the row's number of such pixels: round 0 adds to it
    uint32_t* s_count;            // one LDS word of the kernel
};

// Histogram round `round` (0, 1, 2) of the band of output rows blockIdx.x of plane (n, c) into the row's histograms hq; st is
// the row's state.  MASKED: only the pixels whose label is cls.want are sampled and counted (the label is read first).
template <bool MASKED>
__device__ __forceinline__ void ovl_hist_round(const SpxPlanes& a, int n, int c, int h, int w, int H, int W, int band_rows, int round,
                                               const uint32_t* st, uint32_t* hq, const OvlClass& cls) {
    __shared__ float s_stage[OVL_STAGE];
    __shared__ uint32_t s_hist[2 * OVL_BINS];
    __shared__ int s_oy[OVL_BAND * 4];
    __shared__ float s_wy[OVL_BAND * 4];
    const int tid = threadIdx.x;
    const int Y0 = blockIdx.x * band_rows, nrows = min(H, Y0 + band_rows) - Y0;
    if (MASKED && tid == 0) *cls.s_count = 0u;
    ovl_stage_band<OVL_THREADS>(a, n, c, h, w, H, Y0, nrows, s_oy, s_wy, s_stage, s_hist, 2 * OVL_BINS);
    // the thread's pixels and the runs it carries; a struct, because with a lambda that captured the run counters by reference
    // this kernel kept them in scratch (12 bytes per lane)
    struct {
        OvlClass cls;
        size_t label0;            // of image n
        int W, Y0, round;
        uint32_t p0, p1;
        int cur0, cur1;
        uint32_t run0, run1, mine;
        __device__ __forceinline__ void operator()(int r, int X, const int* ox, const float* wx) {
            if constexpr (MASKED) {
                if (spx_label(cls.labels, cls.label_bytes, label0 + (size_t)(Y0 + r) * W + X) != cls.want) return;
            }
            const uint32_t key = ovl_key(ovl_value(s_stage, &s_oy[4 * r], &s_wy[4 * r], ox, wx));
            if (round == 0) {
                if constexpr (MASKED) ++mine;
                ovl_count(s_hist, cur0, run0, (int)(key >> 21));
            } else if (round == 1) {
                if ((key >> 21) == p0) ovl_count(s_hist, cur0, run0, (int)((key >> 10) & 2047u));
                if ((key >> 21) == p1) ovl_count(s_hist + OVL_BINS, cur1, run1, (int)((key >> 10) & 2047u));
            } else {
                if ((key >> 10) == p0) ovl_count(s_hist, cur0, run0, (int)(key & 1023u));
                if ((key >> 10) == p1) ovl_count(s_hist + OVL_BINS, cur1, run1, (int)(key & 1023u));
            }
        }
    } px = {cls, (size_t)n * H * W, W, Y0, round, st[0], st[2], 0, 0, 0u, 0u, 0u};
    ovl_walk_band<OVL_THREADS>(w, W, nrows, px);
    if (px.run0) atomicAdd(&s_hist[px.cur0], px.run0);
    if (px.run1) atomicAdd(&s_hist[OVL_BINS + px.cur1], px.run1);
    if (MASKED && px.mine) atomicAdd(cls.s_count, px.mine);
    __syncthreads();
    for (int i = tid; i < 2 * OVL_BINS; i += OVL_THREADS) {
        const uint32_t v = s_hist[i];
        if (v) atomicAdd(&hq[i], v);
    }
    if (MASKED && tid == 0 && *cls.s_count) atomicAdd(cls.count, *cls.s_count);
}

// After a round, one workgroup per row: for each of the two ranks (rank(0), rank(1): where the kernel keeps them) the bin that
// holds it (the first bin whose running count exceeds the rank), the rank inside that bin, the key prefix extended by the bin;
// the histograms zeroed for the next round.  After round 2 the keys in st[0], st[2] are complete.
template <class Rank>
__device__ __forceinline__ void ovl_scan_round(int round, uint32_t* st, uint32_t* hq, Rank rank_of) {
    __shared__ uint32_t s_sum[OVL_THREADS];
    const int tid = threadIdx.x;
    const int bits = round == 2 ? 10 : 11, per = (1 << bits) / OVL_THREADS;     // 8 or 4 consecutive bins per thread
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
        const uint32_t rank = rank_of(r);
        uint32_t below = s_sum[tid] - mine;
        __syncthreads();                                                         // every thread has read its rank and sums
        if (rank >= below && rank < below + mine) {                              // exactly one thread
            int b = tid * per;
            for (;; ++b) {
                const uint32_t cnt = hr[b];
                if (rank < below + cnt) break;
                below += cnt;
            }
            st[2 * r] = (st[2 * r] << bits) | (uint32_t)b;
            st[2 * r + 1] = rank - below;
        }
        __syncthreads();
    }
    ovl_clear_hist(hq);
}
// numpy's _lerp of the two order statistics, in fp32
__device__ __forceinline__ float ovl_lerp(float lo, float hi, float gamma) {
    const float d = hi - lo;
    return gamma >= 0.5f ? hi - d * (1.0f - gamma) : lo + d * gamma;
}

#endif  // SPX_OVERLAP_SAMPLE_H
