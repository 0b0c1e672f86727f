// Cross-scale feature aggregation (the reference's WeightedAgg, segmentation/model/scale_head.py, used at
// model_multiscale.py:306-314): scale i's features are combined with the activations of scale i + 1,
//     a[b][p][px] = similarity(source[b][p][px])                      (or the source itself: ready activations)
//     s[b][c][px] = sum_p proto[p][c] . a[b][p][px]                   [B, Cs, HW]
//     out         = s  |  (x + s) / 2  |  sqrt(x . s)
// The reference forms s through a [B, Pn, Cs, H, W] temporary; here it is a pixel-tile product on the fp32 matrix pipe
// (v_mfma_f32_32x32x2_f32: fp32 operands, fp32 accumulation, no bf16 rounding anywhere) with the similarity applied while the
// source is loaded and the combine in the epilogue.
//
// Operand roles are chosen so that NO activation ever passes through LDS: in D = A . B lane l supplies A[row l & 31][k l >> 5]
// and B[k l >> 5][column l & 31]; with the pixels as the COLUMNS a wave's B operand is source[p0 + (l >> 5)][px0 + (l & 31)] -
// two 128-B row pieces straight from global memory - and the accumulator (register r of lane l = row (r & 3) + 8 (r >> 2) +
// 4 (l >> 5), column l & 31) is stored as 128-B pieces along the pixels of NCHW planes.  Only the small operand (the
// prototype sub-bank) is staged in LDS, in panels.
//
//   forward / backward step 1 (spx_sagg_s_kernel):  workgroup = 4 waves = 128 pixels x 64 channels (grid.y = channel chunks), wave = 32 pixels
//       x 2 channel tiles; the [Pn][64] bank chunk walks through LDS in panels of 64 prototypes (row stride 96 floats: the two
//       k rows of a fragment read fall on disjoint banks).  Backward epilogue: dx and ds = dL/ds (fp32, workspace).
//   backward step 2 (spx_sagg_dsrc_kernel):  dsource[p][px] = act'(d) . sum_c proto[p][c] ds[c][px]: rows = prototypes (64 per
//       workgroup, LDS image [p][c] with an odd stride), columns = pixels, ds straight from global memory.
//   backward step 3 (spx_sagg_dproto_kernel + spx_sagg_reduce_kernel):  dproto[p][c] = sum_{b, px} a[p][px] ds[c][px]: the pixels are the
//       contraction index, both operands pass LDS ([row][32 px], stride 33); every workgroup owns a 64 x 64 block of dproto over
//       a slab of 256 pixels of one image and writes its partial; a second kernel sums the slabs in slab order.  No float
//       atomics: two runs agree bit for bit.
#include "spx_args.h"
#include "spx_common.h"

#define SAGG_PX 128            // pixels per workgroup (4 waves x 32)
#define SAGG_CC 64             // channels per workgroup of the s kernel
#define SAGG_PK 64             // prototypes per LDS panel of the s kernel
#define SAGG_LDP 96            // its row stride in floats
#define SAGG_PR 64             // prototype rows per workgroup of the dsource / dproto kernels
#define SAGG_KC 64             // channels per LDS chunk of the dsource kernel
#define SAGG_LDC 65
#define SAGG_SLAB 256          // pixels per slab of the dproto kernel
#define SAGG_KP 32             // pixels per LDS chunk of the dproto kernel
#define SAGG_LDX 33

struct SpxSaggArgs {
    const void* x; long long x_bstride; int x_bf16;
    const float* src; int src_kind;          // 0 activations, 1 distances under 'log', 2 distances under 'linear'
    const float* proto;
    float* out;                              // forward
    const float* g; void* dx; float* ds;     // backward
    float* dsrc; float* part; float* dproto;
    int B, Cs, Pn, HW, mode, nslab;
    float eps;
};

__device__ __forceinline__ float sagg_act(float v, int kind, float eps) {
    return kind == 1 ? act_log(v, eps) : (kind == 2 ? -v : v);
}
__device__ __forceinline__ float sagg_load_x(const void* x, int bf16, long long i) {
    if (bf16) return __uint_as_float((uint32_t)((const uint16_t*)x)[i] << 16);
    return ((const float*)x)[i];
}

template <bool BWD>
__global__ __launch_bounds__(256) void spx_sagg_s_kernel(const SpxSaggArgs a) {
    __shared__ float ps[SAGG_PK * SAGG_LDP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tiles = (a.HW + SAGG_PX - 1) / SAGG_PX;
    const int b = blockIdx.x / tiles, px = (blockIdx.x % tiles) * SAGG_PX + wave * 32 + (lane & 31);
    const int c0 = blockIdx.y * SAGG_CC;
    const bool px_ok = px < a.HW;
    // backward in the modes 'none' / 'sum': ds does not depend on s, the product is skipped
    const bool need_s = !BWD || a.mode == SPX_SAGG_MULT;

    f32x16 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;

    if (need_s) {
        const float* const sp = a.src + ((long long)b * a.Pn) * a.HW + px;
        for (int p0 = 0; p0 < a.Pn; p0 += SAGG_PK) {
            __syncthreads();                      // the previous panel's fragment reads are done
            // panel image [64 p][64 c], zero outside the bank: thread -> (row tid >> 6 + 4 i, channel tid & 63)
#pragma unroll
            for (int i = 0; i < SAGG_PK / 4; ++i) {
                const int pr = (tid >> 6) + 4 * i, c = c0 + (tid & 63), p = p0 + pr;
                ps[pr * SAGG_LDP + (tid & 63)] = (p < a.Pn && c < a.Cs) ? a.proto[(long long)p * a.Cs + c] : 0.0f;
            }
            __syncthreads();
            const int pend = a.Pn - p0 < SAGG_PK ? a.Pn - p0 : SAGG_PK;       // rows of this panel inside the bank
            for (int k0 = 0; k0 < pend; k0 += 16) {
                float av[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int p = p0 + k0 + 2 * j + (lane >> 5);
                    av[j] = (px_ok && p < a.Pn) ? sp[(long long)p * a.HW] : 0.0f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const int p = p0 + k0 + 2 * j + (lane >> 5);
                    // (a row past the bank or a pixel past the image contributes an exact zero, never act(garbage))
                    const float act = (px_ok && p < a.Pn) ? sagg_act(av[j], a.src_kind, a.eps) : 0.0f;
                    const float* const pp = ps + (k0 + 2 * j + (lane >> 5)) * SAGG_LDP + (lane & 31);
#pragma unroll
                    for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(pp[32 * u], act, acc[u], 0, 0, 0);
                }
            }
        }
    }

    if (!px_ok) return;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = c0 + 32 * u + acc_row(r, lane >> 5);
            if (c >= a.Cs) continue;
            const float s = acc[u][r];
            const long long o = ((long long)b * a.Cs + c) * a.HW + px;
            const float xv = a.mode == SPX_SAGG_NONE ? 0.0f : sagg_load_x(a.x, a.x_bf16, (long long)b * a.x_bstride + (long long)c * a.HW + px);
            if (!BWD) {
                float v = s;
                if (a.mode == SPX_SAGG_SUM) v = (xv + s) / 2.0f;
                else if (a.mode == SPX_SAGG_MULT) v = sqrtf(xv * s);
                a.out[o] = v;
            } else {
                const float g = a.g[o];
                float dxv = 0.0f, dsv = g;
                if (a.mode == SPX_SAGG_SUM) {
                    dxv = g / 2.0f;
                    dsv = g / 2.0f;
                } else if (a.mode == SPX_SAGG_MULT) {
                    const float den = 2.0f * sqrtf(xv * s);
                    dxv = g * s / den;
                    dsv = g * xv / den;
                }
                a.ds[o] = dsv;
                if (a.mode != SPX_SAGG_NONE && a.dx) {
                    if (a.x_bf16) ((__bf16*)a.dx)[o] = (__bf16)dxv;           // round to nearest even
                    else ((float*)a.dx)[o] = dxv;
                }
            }
        }
}

__global__ __launch_bounds__(256) void spx_sagg_dsrc_kernel(const SpxSaggArgs a) {
    __shared__ float ps[SAGG_PR * SAGG_LDC];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int tiles = (a.HW + SAGG_PX - 1) / SAGG_PX;
    const int b = blockIdx.x / tiles, px = (blockIdx.x % tiles) * SAGG_PX + wave * 32 + (lane & 31);
    const int p0 = blockIdx.y * SAGG_PR;
    const bool px_ok = px < a.HW;

    f32x16 acc[2];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[u][r] = 0.0f;

    const float* const dp = a.ds + ((long long)b * a.Cs) * a.HW + px;
    for (int cc = 0; cc < a.Cs; cc += SAGG_KC) {
        __syncthreads();
        // chunk image [64 p][64 c]: thread -> (row tid >> 6 + 4 i, channel tid & 63): 256-B row pieces of the bank
#pragma unroll
        for (int i = 0; i < SAGG_PR / 4; ++i) {
            const int pr = (tid >> 6) + 4 * i, c = cc + (tid & 63), p = p0 + pr;
            ps[pr * SAGG_LDC + (tid & 63)] = (p < a.Pn && c < a.Cs) ? a.proto[(long long)p * a.Cs + c] : 0.0f;
        }
        __syncthreads();
        const int cend = a.Cs - cc < SAGG_KC ? a.Cs - cc : SAGG_KC;           // a multiple of 16
        for (int k0 = 0; k0 < cend; k0 += 16) {
            float dv[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int c = cc + k0 + 2 * j + (lane >> 5);
                dv[j] = (px_ok && c < a.Cs) ? dp[(long long)c * a.HW] : 0.0f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float* const pp = ps + (lane & 31) * SAGG_LDC + k0 + 2 * j + (lane >> 5);
#pragma unroll
                for (int u = 0; u < 2; ++u) acc[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(pp[32 * u * SAGG_LDC], dv[j], acc[u], 0, 0, 0);
            }
        }
    }

    if (!px_ok) return;
    const float c1 = -(1.0f - a.eps);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int p = p0 + 32 * u + acc_row(r, lane >> 5);
            if (p >= a.Pn) continue;
            const long long o = ((long long)b * a.Pn + p) * a.HW + px;
            float v = acc[u][r];
            if (a.src_kind == 1) {
                const float d = a.src[o];
                v = v * (c1 / ((d + 1.0f) * (d + a.eps)));
            } else if (a.src_kind == 2) {
                v = -v;
            }
            a.dsrc[o] = v;
        }
}

// block (p chunk, c chunk) of dproto over one slab of pixels of one image -> part[slab][Pn][Cs]
__global__ __launch_bounds__(256) void spx_sagg_dproto_kernel(const SpxSaggArgs a) {
    __shared__ float as[SAGG_PR * SAGG_LDX];
    __shared__ float gs[SAGG_PR * SAGG_LDX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int spi = (a.HW + SAGG_SLAB - 1) / SAGG_SLAB;           // slabs per image
    const int slab = blockIdx.x, b = slab / spi;
    const int s0 = (slab % spi) * SAGG_SLAB;
    const int send = s0 + SAGG_SLAB < a.HW ? s0 + SAGG_SLAB : a.HW;
    const int ncc = (a.Cs + 63) / 64;
    const int p0 = ((int)blockIdx.y / ncc) * SAGG_PR, c0 = ((int)blockIdx.y % ncc) * 64;
    const int wp = wave >> 1, wc = wave & 1;                      // the wave's 32 x 32 tile of the block

    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.0f;

    const float* const sp = a.src + ((long long)b * a.Pn) * a.HW;
    const float* const dp = a.ds + ((long long)b * a.Cs) * a.HW;
    for (int q0 = s0; q0 < send; q0 += SAGG_KP) {
        __syncthreads();
        // thread -> (row tid >> 5 + 8 i, pixel tid & 31): 128-B row pieces
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = (tid >> 5) + 8 * i, q = q0 + (tid & 31);
            const int p = p0 + row, c = c0 + row;
            const bool qok = q < send;
            as[row * SAGG_LDX + (tid & 31)] = (qok && p < a.Pn) ? sagg_act(sp[(long long)p * a.HW + q], a.src_kind, a.eps) : 0.0f;
            gs[row * SAGG_LDX + (tid & 31)] = (qok && c < a.Cs) ? dp[(long long)c * a.HW + q] : 0.0f;
        }
        __syncthreads();
        const float* const ap = as + (wp * 32 + (lane & 31)) * SAGG_LDX + (lane >> 5);
        const float* const gp = gs + (wc * 32 + (lane & 31)) * SAGG_LDX + (lane >> 5);
#pragma unroll
        for (int kk = 0; kk < SAGG_KP / 2; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ap[2 * kk], gp[2 * kk], acc, 0, 0, 0);
    }

    const int c = c0 + wc * 32 + (lane & 31);
    if (c >= a.Cs) return;
    float* const out = a.part + (long long)slab * a.Pn * a.Cs;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int p = p0 + wp * 32 + acc_row(r, lane >> 5);
        if (p < a.Pn) out[(long long)p * a.Cs + c] = acc[r];
    }
}

// dproto = sum of the slab partials, in slab order
__global__ __launch_bounds__(256) void spx_sagg_reduce_kernel(const float* __restrict__ part, int nslab, int n, float* __restrict__ dproto) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    float s = 0.0f;
    for (int k = 0; k < nslab; ++k) s += part[(long long)k * n + g];
    dproto[g] = s;
}

static int sagg_slabs(int B, int HW) { return B * ((HW + SAGG_SLAB - 1) / SAGG_SLAB); }

// workspace: [ds: B Cs HW floats | slab partials: nslab Pn Cs floats]
size_t spx_scale_agg_workspace(int B, int Cs, int Pn, int HW) {
    return ((size_t)B * Cs * HW + (size_t)sagg_slabs(B, HW) * Pn * Cs) * sizeof(float);
}

hipError_t spx_launch_scale_agg_fwd(const void* x, int x_bf16, long long x_bstride, const float* src, int src_kind, const float* proto,
                                    float* out, int B, int Cs, int Pn, int HW, int mode, float eps, hipStream_t s) {
    SpxSaggArgs a = {};
    a.x = x; a.x_bstride = x_bstride; a.x_bf16 = x_bf16;
    a.src = src; a.src_kind = src_kind; a.proto = proto; a.out = out;
    a.B = B; a.Cs = Cs; a.Pn = Pn; a.HW = HW; a.mode = mode; a.eps = eps;
    const dim3 grid((unsigned)(B * ((HW + SAGG_PX - 1) / SAGG_PX)), (unsigned)((Cs + SAGG_CC - 1) / SAGG_CC));
    hipLaunchKernelGGL(spx_sagg_s_kernel<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t spx_launch_scale_agg_bwd(const void* x, int x_bf16, long long x_bstride, const float* src, int src_kind, const float* proto,
                                    const float* g, void* dx, float* dsrc, float* dproto, void* ws, int B, int Cs, int Pn, int HW,
                                    int mode, float eps, hipStream_t s) {
    SpxSaggArgs a = {};
    a.x = x; a.x_bstride = x_bstride; a.x_bf16 = x_bf16;
    a.src = src; a.src_kind = src_kind; a.proto = proto;
    a.g = g; a.dx = dx; a.dsrc = dsrc; a.dproto = dproto;
    a.ds = (float*)ws;
    a.part = (float*)ws + (size_t)B * Cs * HW;
    a.nslab = sagg_slabs(B, HW);
    a.B = B; a.Cs = Cs; a.Pn = Pn; a.HW = HW; a.mode = mode; a.eps = eps;
    const unsigned tiles = (unsigned)(B * ((HW + SAGG_PX - 1) / SAGG_PX));
    hipLaunchKernelGGL(spx_sagg_s_kernel<true>, dim3(tiles, (unsigned)((Cs + SAGG_CC - 1) / SAGG_CC)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (dsrc) {
        hipLaunchKernelGGL(spx_sagg_dsrc_kernel, dim3(tiles, (unsigned)((Pn + SAGG_PR - 1) / SAGG_PR)), dim3(256), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    if (dproto) {
        const unsigned blocks = (unsigned)(((Pn + SAGG_PR - 1) / SAGG_PR) * ((Cs + 63) / 64));
        hipLaunchKernelGGL(spx_sagg_dproto_kernel, dim3((unsigned)a.nslab, blocks), dim3(256), 0, s, a);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(spx_sagg_reduce_kernel, dim3((unsigned)((Pn * Cs + 255) / 256)), dim3(256), 0, s, (const float*)a.part, a.nslab,
                           Pn * Cs, dproto);
        e = hipGetLastError();
    }
    return e;
}
