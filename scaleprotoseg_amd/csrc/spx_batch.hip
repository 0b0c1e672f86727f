// Training-batch preparation (segmentation/data/dataset.py:143-186 and the per-step resize_label of module_multiscale.py:234-236):
// the augmented, normalised window batch, the window labels and the latent labels of every grid in ONE launch, from raw uint8
// HWC images and integer labels on the device.  include/spx_hip.h states the arithmetic; this file keeps its operation order.
//
//   spx_batch_prepare_kernel   grid (window blocks + latent blocks of every grid, B).  The window of a sample is walked as one flat
//                              run of Hc * Wc pixels, BATCH_THREADS per workgroup, so a wave's 64 lanes store 256 contiguous bytes
//                              into each of the three CHW planes and 512 into the int64 labels whatever Wc is (513 is odd: no
//                              wider store is aligned), and read about 64 neighbouring 3-byte pixels of one or two source rows, each
//                              lane its two horizontal neighbours as ONE unaligned 8-byte load per row.
//                              The latent blocks read the labels straight from the source through the composed tables: no block
//                              waits for another, nothing is read back that this launch wrote.
//   spx_resize_labels_kernel   the latent blocks alone, over a dense [B, H, W] label tensor.
// The descriptor of a sample is read through wave-uniform addresses (blockIdx.y), i.e. by scalar loads.
#include "spx_args.h"

#define BATCH_THREADS 256

__device__ __forceinline__ long long batch_raw_label(const void* p, int dtype, long long at) {
    switch (dtype) {
        case SPX_LABEL_U8: return (long long)((const uint8_t*)p)[at];
        case SPX_LABEL_I16: return (long long)((const int16_t*)p)[at];
        case SPX_LABEL_I32: return (long long)((const int32_t*)p)[at];
        default: return ((const long long*)p)[at];
    }
}
// Loads are issued for every lane from an address clamped into the buffer and the result is selected afterwards: a load under a
// per-lane condition is a basic block with its own wait, one exposed memory round trip each.
__device__ __forceinline__ long long batch_map_label(long long raw, const int32_t* __restrict__ id_map, int L) {
    if (!id_map) return raw;                                        // wave-uniform
    const bool known = raw >= 0 && raw < (long long)L;
    const long long v = (long long)id_map[known ? raw : 0];
    return known ? v : 0ll;
}
__device__ __forceinline__ int batch_clamp(int v, int n) { return v < 0 ? 0 : (v > n - 1 ? n - 1 : v); }
__device__ __forceinline__ int batch_clamp_ll(long long v, int n) { return v < 0 ? 0 : (v > (long long)(n - 1) ? n - 1 : (int)v); }
__device__ __forceinline__ int32_t batch_shift(long long v) {                      // the rule of spx_shift_labels_kernel
    const long long w = v - 1;
    return (w < -2147483647LL || w > 2147483647LL) ? -1 : (int32_t)w;
}
// do the sample's two tables lie inside the index buffer?  (wave-uniform)
__device__ __forceinline__ bool batch_tables_ok(const spx_batch_sample& s, int n_index) {
    return s.hs >= 1 && s.ws >= 1 && s.h >= 1 && s.w >= 1 && s.row_tab >= 0 && s.col_tab >= 0 &&
           (long long)s.row_tab + s.hs <= (long long)n_index && (long long)s.col_tab + s.ws <= (long long)n_index;
}
// the window label at (y, x) of a sample whose tables are ok: 0 in the pad
__device__ __forceinline__ long long batch_window_label(const spx_batch& a, const spx_batch_sample& s, int y, int x) {
    const int xf = s.flip ? a.Wc - 1 - x : x;
    const long long sy = (long long)s.y0 + y, sx = (long long)s.x0 + xf;
    const bool inside = sy >= 0 && sx >= 0 && sy < s.hs && sx < s.ws;
    const int cy = batch_clamp_ll(sy, s.hs), cx = batch_clamp_ll(sx, s.ws);
    const int Y = batch_clamp(a.index[s.row_tab + cy], s.h), X = batch_clamp(a.index[s.col_tab + cx], s.w);
    const long long v = batch_map_label(batch_raw_label(s.label, s.label_dtype, (long long)Y * s.label_row_stride + X), a.id_map, a.L);
    return inside ? v : 0ll;
}

// source position of OpenCV's INTER_LINEAR along one axis, fp32 (include/spx_hip.h)
__device__ __forceinline__ void batch_axis(int d, int n_in, int n_out, int& i0, int& i1, float& frac) {
    const float r = (float)n_in / (float)n_out;
    float f = ((float)d + 0.5f) * r - 0.5f;
    f = f < 0.0f ? 0.0f : f;
    const float fl = floorf(f);
    i0 = (int)fl;
    frac = f - fl;
    i1 = i0 + 1 < n_in - 1 ? i0 + 1 : n_in - 1;
    if (i0 >= n_in - 1) {
        i0 = i1 = n_in - 1;
        frac = 0.0f;
    }
}

// The two horizontal neighbours X0, X1 of one source row as fp32, p[0..2] and p[3..5].  Packed pixels (stride 3, w >= 3; wave-
// uniform): X1 is X0 + 1, or X0 itself at the right edge where its weight is exactly 0, so the six bytes from X0 on are fetched
// as ONE unaligned 8-byte load that is moved left to end with the row and shifted back; bytes past the row come out as 0.
__device__ __forceinline__ void batch_pair(const uint8_t* row, long long X0, long long X1, int w, int pixel_stride, float* p) {
    if (pixel_stride == 3 && w >= 3) {
        const long long o0 = X0 * 3, last = (long long)w * 3 - 8;
        const long long base = o0 < last ? o0 : last;
        unsigned long long q;
        __builtin_memcpy(&q, row + base, 8);
        q >>= 8 * (int)(o0 - base);
#pragma unroll
        for (int c = 0; c < 6; ++c) p[c] = (float)(unsigned)((q >> (8 * c)) & 0xffull);
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            p[c] = (float)row[X0 * pixel_stride + c];
            p[3 + c] = (float)row[X1 * pixel_stride + c];
        }
    }
}

// which latent grid a block of the latent range belongs to: blocks of grid 0 first
__device__ __forceinline__ int batch_latent_grid(const spx_batch& a, int& block) {
    int g = 0;
    for (; g < a.G - 1; ++g) {
        const int nb = (a.grid_h[g] * a.grid_w[g] + BATCH_THREADS - 1) / BATCH_THREADS;
        if (block < nb) break;
        block -= nb;
    }
    return g;
}
__device__ __forceinline__ void batch_store_latent(const spx_batch& a, int g, size_t at, long long v) {
    if (a.latent[g]) a.latent[g][at] = v;
    if (a.latent0[g]) a.latent0[g][at] = batch_shift(v);
}

__global__ __launch_bounds__(BATCH_THREADS) void spx_batch_prepare_kernel(const spx_batch a, const int window_blocks) {
    const int b = blockIdx.y;
    const spx_batch_sample s = a.samples[b];
    const bool ok = batch_tables_ok(s, a.n_index);                  // wave-uniform, as every branch below but the bounds checks
    int block = blockIdx.x;
    if (block >= window_blocks) {                                   // no barrier in this kernel
        block -= window_blocks;
        const int g = batch_latent_grid(a, block);
        const int hg = a.grid_h[g], wg = a.grid_w[g];
        const int j = block * BATCH_THREADS + threadIdx.x;
        if (j >= hg * wg) return;
        const int ly = j / wg, lx = j - ly * wg;
        const int y = batch_clamp(a.index[a.grid_rt[g] + ly], a.Hc), x = batch_clamp(a.index[a.grid_ct[g] + lx], a.Wc);
        batch_store_latent(a, g, (size_t)b * hg * wg + j, ok ? batch_window_label(a, s, y, x) : 0ll);
        return;
    }
    const int HW = a.Hc * a.Wc;
    const int i = block * BATCH_THREADS + threadIdx.x;
    if (i >= HW) return;
    const int y = i / a.Wc, x = i - y * a.Wc;
    const int xf = s.flip ? a.Wc - 1 - x : x;
    const long long sy = (long long)s.y0 + y, sx = (long long)s.x0 + xf;
    const bool inside = ok && sy >= 0 && sx >= 0 && sy < s.hs && sx < s.ws;
    float r[3] = {0.0f, 0.0f, 0.0f};
    long long lab = 0ll;
    if (ok) {
        // the image's loads first: they do not depend on the index tables, so they are in flight with the tables' round trip
        if (a.image_out) {
            int X0, X1, Y0, Y1;
            float fa, fb;
            batch_axis(batch_clamp_ll(sx, s.ws), s.w, s.ws, X0, X1, fa);
            batch_axis(batch_clamp_ll(sy, s.hs), s.h, s.hs, Y0, Y1, fb);
            float top[6], bot[6];
            batch_pair((const uint8_t*)s.image + (long long)Y0 * s.image_row_stride, X0, X1, s.w, s.image_pixel_stride, top);
            batch_pair((const uint8_t*)s.image + (long long)Y1 * s.image_row_stride, X0, X1, s.w, s.image_pixel_stride, bot);
            if (a.window_labels) lab = batch_window_label(a, s, y, x);
            const float ia = 1.0f - fa, ib = 1.0f - fb;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const float v = (top[c] * ia + top[3 + c] * fa) * ib + (bot[c] * ia + bot[3 + c] * fa) * fb;
                r[c] = a.round_u8 ? rintf(v) : v;
            }
        } else if (a.window_labels) {
            lab = batch_window_label(a, s, y, x);
        }
    }
    if (a.window_labels) a.window_labels[(size_t)b * HW + i] = lab;
    if (!a.image_out) return;
    const size_t plane = (size_t)HW;
    if (a.out_u8) {
        uint8_t* out = (uint8_t*)a.image_out + (size_t)b * 3 * plane + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = inside ? r[c] : rintf(a.mean[c] * 255.0f);
            v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
            out[c * plane] = (uint8_t)v;
        }
    } else {
        float* out = (float*)a.image_out + (size_t)b * 3 * plane + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float v = r[c] / 255.0f;
            if (a.normalize) v = (v - a.mean[c]) / a.std[c];
            out[c * plane] = inside ? v : (a.normalize ? 0.0f : a.mean[c]);
        }
    }
}

__global__ __launch_bounds__(BATCH_THREADS) void spx_resize_labels_kernel(const spx_batch a) {
    const int b = blockIdx.y;
    int block = blockIdx.x;
    const int g = batch_latent_grid(a, block);
    const int hg = a.grid_h[g], wg = a.grid_w[g];
    const int j = block * BATCH_THREADS + threadIdx.x;
    if (j >= hg * wg) return;
    const int ly = j / wg, lx = j - ly * wg;
    const int y = batch_clamp(a.index[a.grid_rt[g] + ly], a.Hc), x = batch_clamp(a.index[a.grid_ct[g] + lx], a.Wc);
    const long long raw = batch_raw_label(a.labels_in, a.labels_dtype, ((long long)b * a.Hc + y) * a.Wc + x);
    batch_store_latent(a, g, (size_t)b * hg * wg + j, batch_map_label(raw, a.id_map, a.L));
}

static unsigned batch_latent_blocks(const spx_batch& a) {
    unsigned n = 0;
    for (int g = 0; g < a.G; ++g) n += (unsigned)((a.grid_h[g] * a.grid_w[g] + BATCH_THREADS - 1) / BATCH_THREADS);
    return n;
}

hipError_t spx_launch_batch_prepare(const spx_batch& a, hipStream_t s) {
    const bool window = a.image_out || a.window_labels;
    const int window_blocks = window ? (a.Hc * a.Wc + BATCH_THREADS - 1) / BATCH_THREADS : 0;
    const unsigned blocks = (unsigned)window_blocks + batch_latent_blocks(a);
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(spx_batch_prepare_kernel, dim3(blocks, (unsigned)a.B), dim3(BATCH_THREADS), 0, s, a, window_blocks);
    return hipGetLastError();
}

hipError_t spx_launch_resize_labels(const spx_batch& a, hipStream_t s) {
    const unsigned blocks = batch_latent_blocks(a);
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(spx_resize_labels_kernel, dim3(blocks, (unsigned)a.B), dim3(BATCH_THREADS), 0, s, a);
    return hipGetLastError();
}
