// What the activation-overlap metrics (spx_overlap.hip), the class-restricted thresholds (spx_masked_select.hip), the push
// bounding boxes (spx_pushbox.hip) and the explanation maps (spx_explain.hip) share: the upsampled value of a pixel recomputed
// from the latent plane, the bands of output rows that stage their latent rows in LDS and the key and run counter of the radix
// select (the strided view of the planes and the label read come from spx_planes.h).  ONE function, compiled with
// -ffp-contract=off, gives a pixel the same bits in every pass of every file.
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

// ---- the exact radix select over the upsampled values (spx_overlap.hip, spx_masked_select.hip) ---------------------------
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

#endif  // SPX_OVERLAP_SAMPLE_H
