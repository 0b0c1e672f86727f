// Multi-scale input fusion: the pixel-wise maximum of the reference's MSC wrapper (segmentation/utils.py:71-111) over the
// full-scale backbone output and the bilinearly resampled outputs of the scaled inputs, with the add-on sigmoid and the cast
// of the deeplab_simple configurations in the same pass.  The rule is stated in include/spx_hip.h (spx_msc_max_fwd).
//
//   forward  (spx_msc_max_fwd_kernel)   a thread owns one group of 4 consecutive columns of one output row and walks a chunk of
//       channels (grid: row groups x channel chunks x batch).  The per-row (i0, i1, ly) of every scaled map is formed once per
//       thread, before the channel loop.  The groups of a row are anchored where the OUTPUT is 16-byte aligned (8 bytes for
//       bf16): the row's first a = 0..3 elements belong to the row's thread 0, every later thread stores one aligned vector and
//       the last one the remainder, element by element - so W, H * W and the output pointer need no alignment and the store of
//       a wave is still one contiguous piece.  The full-scale map is read as a vector when its own address allows it; the scaled
//       maps are at most a few taps per output and are read through the caches, element by element.
//   K = 1    (spx_msc_act_kernel)       the activation and the cast alone: the same groups over a plane taken as one row, four
//       channels per step with their loads issued together (the bandwidth-bound case).
//   backward (spx_msc_max_bwd_kernel)   gather form, all maps in one launch: a thread owns one SOURCE element, finds its map by
//       the descriptor's prefix sums, walks the destination rows and columns whose footprint can hold it (the inverse of s(Y),
//       widened by one; every candidate is tested with the forward's own index function, so rounding can neither drop nor double
//       a contribution) and adds g . wy . wx where the saved index names its map, in ascending (Y, X) order.
//   packed   (spx_msc_pack_fwd / _bwd_kernel)   the K maps and their maximum side by side on one pixel axis; see below.
// Every rule has ONE statement, shared by the plain and the packed kernels: the candidate and the rule of the maximum (msc_tap,
// msc_takes_over), the activation and the stores (msc_sigmoid, msc_store_vector, msc_store), and in the backward the upstream
// term, the decode of a source element and the term of the maximum (msc_upstream, msc_source, msc_max_term).  On the host:
// msc_fill, msc_grad_offsets, msc_channel_chunk.
// No LDS, no atomics, no workspace.
#include "spx_args.h"
#include "spx_common.h"

#define MSC_THREADS 256
#define MSC_VEC 4

// what every kernel's arguments begin with (msc_fill; gofs: msc_grad_offsets)
struct SpxMscCommon {
    spx_msc d;
    float rh[SPX_MSC_MAX_MAPS], rw[SPX_MSC_MAX_MAPS];   // float(h_k) / float(H), float(w_k) / float(W)
    long long gofs[SPX_MSC_MAX_MAPS + 1];               // backward: prefix sums of the elements of the maps that get a gradient
    int H, W;
};
struct SpxMscArgs : SpxMscCommon {
    int groups, cchunk;                                 // forward: groups of a row (ceil(W / 4) + 1), channels per block
    int out_mis;                                        // forward: (out address / element size) & 3
};

// source position of destination index D on an axis of n source elements (ratio r = float(n) / float(destination size))
__device__ __forceinline__ void msc_src(float r, int n, int D, int& i0, int& i1, float& l) {
    float s = r * ((float)D + 0.5f) - 0.5f;
    s = s < 0.0f ? 0.0f : s;
    const int f = (int)floorf(s);
    i0 = f < n - 1 ? f : n - 1;
    i1 = i0 + 1 < n - 1 ? i0 + 1 : n - 1;
    l = s - (float)i0;
}
__device__ __forceinline__ float msc_load(const void* p, bool bf16, long long i) {
    if (bf16) return __uint_as_float((uint32_t)((const uint16_t*)p)[i] << 16);
    return ((const float*)p)[i];
}
__device__ __forceinline__ uint16_t msc_bf16_bits(float v) {
    const __bf16 h = (__bf16)v;                          // round to nearest even
    return *(const uint16_t*)&h;
}
__device__ __forceinline__ void msc_store(void* p, bool bf16, long long i, float v) {
    if (bf16) ((uint16_t*)p)[i] = msc_bf16_bits(v);
    else ((float*)p)[i] = v;
}
// the bilinear candidate of a scaled map: rows r0, r1 (their first elements), columns j0, j1, weights ly, lx
__device__ __forceinline__ float msc_tap(const void* data, bool bf16, long long r0, long long r1, int j0, int j1, float ly, float lx) {
    const float v00 = msc_load(data, bf16, r0 + j0), v01 = msc_load(data, bf16, r0 + j1);
    const float v10 = msc_load(data, bf16, r1 + j0), v11 = msc_load(data, bf16, r1 + j1);
    return (1.0f - ly) * ((1.0f - lx) * v00 + lx * v01) + ly * ((1.0f - lx) * v10 + lx * v11);
}
// torch.max(dim=0): a larger value wins, the first of equals stays, the first NaN wins and stays
__device__ __forceinline__ bool msc_takes_over(float u, float v) { return u > v || (u != u && v == v); }
__device__ __forceinline__ float msc_sigmoid(float v) { return 1.0f / (1.0f + expf(-v)); }
__device__ __forceinline__ void msc_sigmoid(float (&v)[MSC_VEC]) {
#pragma unroll
    for (int j = 0; j < MSC_VEC; ++j) v[j] = msc_sigmoid(v[j]);
}

// one thread's group [xs, xs + 4) of a row of the full-scale map (first element p0 + xs ... clipped to [xb, xe)): a vector
// when the group is whole and its address allows it
template <bool IN_BF16>
__device__ __forceinline__ bool msc_group_vector_ok(const void* data, long long p0, bool full) {
    return full && (((uintptr_t)data + (uintptr_t)p0 * (IN_BF16 ? 2 : 4)) & (IN_BF16 ? 7 : 15)) == 0;
}
template <bool IN_BF16>
__device__ __forceinline__ void msc_load_vector(const void* data, long long p0, float (&v)[MSC_VEC]) {
    if (IN_BF16) {
        const uint2 r = *(const uint2*)((const uint16_t*)data + p0);
        v[0] = __uint_as_float(r.x << 16);
        v[1] = __uint_as_float(r.x & 0xffff0000u);
        v[2] = __uint_as_float(r.y << 16);
        v[3] = __uint_as_float(r.y & 0xffff0000u);
    } else {
        const float4 r = *(const float4*)((const float*)data + p0);
        v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
    }
}
// the cast and the store of a whole group at element o of out, where a vector may go (8 bytes for bf16, 16 for fp32)
template <bool OUT_BF16>
__device__ __forceinline__ void msc_store_vector(void* out, long long o, const float (&v)[MSC_VEC]) {
    if (OUT_BF16) {
        uint2 r;
        r.x = (uint32_t)msc_bf16_bits(v[0]) | ((uint32_t)msc_bf16_bits(v[1]) << 16);
        r.y = (uint32_t)msc_bf16_bits(v[2]) | ((uint32_t)msc_bf16_bits(v[3]) << 16);
        *(uint2*)((uint16_t*)out + o) = r;
    } else {
        *(float4*)((float*)out + o) = make_float4(v[0], v[1], v[2], v[3]);
    }
}
template <bool IN_BF16>
__device__ __forceinline__ void msc_load_group(const void* data, long long p0, int xs, int xb, int xe, float (&v)[MSC_VEC]) {
    if (msc_group_vector_ok<IN_BF16>(data, p0, xe - xb == MSC_VEC)) {
        msc_load_vector<IN_BF16>(data, p0, v);
    } else {
#pragma unroll
        for (int j = 0; j < MSC_VEC; ++j) v[j] = (xs + j >= xb && xs + j < xe) ? msc_load(data, IN_BF16, p0 + j) : 0.0f;
    }
}
// activation, cast and store of a group; o = the row's first element + xs, aligned by the anchoring when the group is whole
template <bool OUT_BF16>
__device__ __forceinline__ void msc_store_group(void* out, uint8_t* index, int activation, long long o, int xs, int xb, int xe,
                                                float (&v)[MSC_VEC], const int (&win)[MSC_VEC]) {
    const bool full = xe - xb == MSC_VEC;
    if (activation == 1) msc_sigmoid(v);
    if (full) {
        msc_store_vector<OUT_BF16>(out, o, v);
    } else {
#pragma unroll
        for (int j = 0; j < MSC_VEC; ++j)
            if (xs + j >= xb && xs + j < xe) msc_store(out, OUT_BF16, o + j, v[j]);
    }
    if (index) {
        uint8_t* const q = index + o;
        if (full && ((uintptr_t)q & 3) == 0) {
            *(uint32_t*)q = (uint32_t)win[0] | ((uint32_t)win[1] << 8) | ((uint32_t)win[2] << 16) | ((uint32_t)win[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < MSC_VEC; ++j)
                if (xs + j >= xb && xs + j < xe) q[j] = (uint8_t)win[j];
        }
    }
}
// the group of thread t in the output row whose first element is e0: [xs, xs + 4) clipped to [xb, xe) (empty: xb >= xe)
__device__ __forceinline__ void msc_group(long long e0, int out_mis, int t, int W, int& xs, int& xb, int& xe) {
    const int head = (int)((MSC_VEC - ((e0 + out_mis) & (MSC_VEC - 1))) & (MSC_VEC - 1));
    xs = head - MSC_VEC + MSC_VEC * t;
    xb = xs < 0 ? 0 : xs;
    xe = xs + MSC_VEC < W ? xs + MSC_VEC : W;
}

template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(MSC_THREADS) void spx_msc_max_fwd_kernel(const SpxMscArgs a) {
    const int H = a.H, W = a.W, K = a.d.K, C = a.d.C;
    const long long task = (long long)blockIdx.x * MSC_THREADS + threadIdx.x;
    if (task >= (long long)H * a.groups) return;
    const int Y = (int)(task / a.groups), t = (int)(task - (long long)Y * a.groups);
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * a.cchunk;
    const int c1 = c0 + a.cchunk < C ? c0 + a.cchunk : C;

    // the rows of every scaled map under this output row, once per thread (constant indices after unrolling: registers)
    int ri0[SPX_MSC_MAX_MAPS], ri1[SPX_MSC_MAX_MAPS];
    float rl[SPX_MSC_MAX_MAPS];
#pragma unroll
    for (int k = 1; k < SPX_MSC_MAX_MAPS; ++k) {
        ri0[k] = ri1[k] = 0;
        rl[k] = 0.0f;
        if (k < K) msc_src(a.rh[k], a.d.maps[k].h, Y, ri0[k], ri1[k], rl[k]);
    }

    const spx_msc_map m0 = a.d.maps[0];
    for (int c = c0; c < c1; ++c) {
        const long long e0 = (((long long)b * C + c) * H + Y) * W;               // the output row's first element
        int xs, xb, xe;
        msc_group(e0, a.out_mis, t, W, xs, xb, xe);
        if (xb >= xe) continue;

        float v[MSC_VEC];
        int win[MSC_VEC];
        msc_load_group<IN_BF16>(m0.data, (long long)b * m0.batch_stride + (long long)c * m0.channel_stride + (long long)Y * W + xs, xs, xb,
                                xe, v);
#pragma unroll
        for (int j = 0; j < MSC_VEC; ++j) win[j] = 0;

#pragma unroll
        for (int k = 1; k < SPX_MSC_MAX_MAPS; ++k) {
            if (k >= K) break;
            const spx_msc_map m = a.d.maps[k];
            const long long pl = (long long)b * m.batch_stride + (long long)c * m.channel_stride;
            const long long r0 = pl + (long long)ri0[k] * m.w, r1 = pl + (long long)ri1[k] * m.w;
#pragma unroll
            for (int j = 0; j < MSC_VEC; ++j) {
                const int X = xs + j;
                if (X < xb || X >= xe) continue;
                int j0, j1;
                float lx;
                msc_src(a.rw[k], m.w, X, j0, j1, lx);
                const float u = msc_tap(m.data, IN_BF16, r0, r1, j0, j1, rl[k], lx);
                if (msc_takes_over(u, v[j])) {
                    v[j] = u;
                    win[j] = k;
                }
            }
        }
        msc_store_group<OUT_BF16>(a.d.out, a.d.index, a.d.activation, e0 + xs, xs, xb, xe, v, win);
    }
}

// K = 1: the activation and the cast alone.  There is no geometry, so a plane is taken as ONE row of H . W elements (the host
// passes H = 1, W = H . W): two threads of a plane at most hold a partial group.  Bandwidth-bound: a thread takes four channels
// per step and, where all four groups are whole vectors (all but the planes' ends), issues the four loads before the first use.
#define MSC_ACT_UNROLL 4
template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(MSC_THREADS) void spx_msc_act_kernel(const SpxMscArgs a) {
    const int W = a.W, C = a.d.C;
    const int t = blockIdx.x * MSC_THREADS + threadIdx.x;
    if (t >= a.groups) return;
    const int b = blockIdx.z;
    const int c0 = blockIdx.y * a.cchunk;
    const int c1 = c0 + a.cchunk < C ? c0 + a.cchunk : C;
    const spx_msc_map m0 = a.d.maps[0];
    const int win[MSC_VEC] = {0, 0, 0, 0};

    for (int c = c0; c < c1; c += MSC_ACT_UNROLL) {
        long long e0[MSC_ACT_UNROLL], p0[MSC_ACT_UNROLL];
        int xs[MSC_ACT_UNROLL], xb[MSC_ACT_UNROLL], xe[MSC_ACT_UNROLL];
        bool fast = c + MSC_ACT_UNROLL <= c1;
#pragma unroll
        for (int u = 0; u < MSC_ACT_UNROLL; ++u) {
            const int cu = c + u < c1 ? c + u : c1 - 1;
            e0[u] = ((long long)b * C + cu) * W;
            msc_group(e0[u], a.out_mis, t, W, xs[u], xb[u], xe[u]);
            p0[u] = (long long)b * m0.batch_stride + (long long)cu * m0.channel_stride + xs[u];
            fast = fast && msc_group_vector_ok<IN_BF16>(m0.data, p0[u], xe[u] - xb[u] == MSC_VEC);
        }
        if (fast) {
            float v[MSC_ACT_UNROLL][MSC_VEC];
#pragma unroll
            for (int u = 0; u < MSC_ACT_UNROLL; ++u) msc_load_vector<IN_BF16>(m0.data, p0[u], v[u]);
            if (a.d.activation == 1) {
#pragma unroll
                for (int u = 0; u < MSC_ACT_UNROLL; ++u) msc_sigmoid(v[u]);
            }
#pragma unroll
            for (int u = 0; u < MSC_ACT_UNROLL; ++u) msc_store_vector<OUT_BF16>(a.d.out, e0[u] + xs[u], v[u]);   // aligned by the anchoring
            if (a.d.index) {
#pragma unroll
                for (int u = 0; u < MSC_ACT_UNROLL; ++u)
#pragma unroll
                    for (int j = 0; j < MSC_VEC; ++j) a.d.index[e0[u] + xs[u] + j] = 0;
            }
        } else {
#pragma unroll
            for (int u = 0; u < MSC_ACT_UNROLL; ++u) {
                if (c + u >= c1 || xb[u] >= xe[u]) continue;
                float v[MSC_VEC];
                msc_load_group<IN_BF16>(m0.data, p0[u], xs[u], xb[u], xe[u], v);
                msc_store_group<OUT_BF16>(a.d.out, a.d.index, a.d.activation, e0[u] + xs[u], xs[u], xb[u], xe[u], v, win);
            }
        }
    }
}

// first and last destination index whose footprint can hold source index i (n source elements, D destination elements)
__device__ __forceinline__ void msc_dst_range(float r, int n, int D, int i, int& lo, int& hi) {
    // s(Y) = r (Y + 0.5) - 0.5 lies in (i - 1, i + 1)  <=>  Y in ((i - 0.5) / r - 0.5, (i + 1.5) / r - 0.5); widened by one.
    // Rows clamped at the borders belong to the border indices: s raised to 0 names i0 = 0 and i1 = 1 (with weight 0 on the
    // latter), i1 held at n - 1 names the last index.
    const float a = ((float)i - 0.5f) / r - 0.5f, b = ((float)i + 1.5f) / r - 0.5f;
    lo = (int)floorf(a) - 1;
    hi = (int)ceilf(b) + 1;
    if (i <= 1 || lo < 0) lo = 0;
    if (i == n - 1 || hi > D - 1) hi = D - 1;
}

// the upstream term at element o of the output: g, under the sigmoid g y (1 - y) at the SAVED y
__device__ __forceinline__ float msc_upstream(const spx_msc& d, long long o) {
    float g = msc_load(d.g, d.g_dtype == 0, o);
    if (d.activation == 1) {
        const float y = msc_load(d.out, d.out_dtype == 0, o);
        g = g * (y * (1.0f - y));
    }
    return g;
}

// The source element a backward thread owns: element `local` = ((b C + c) h + i) w + j of map k, the map whose range of the
// prefix sums holds id (a map without a gradient has an empty range).  off: the first column of every segment (the pack) or null.
struct MscSource {
    int k, h, w, off, i, j;
    float rh, rw;
    long long local, plane;                             // plane = b * C + c
    void* grad;
};
__device__ __forceinline__ MscSource msc_source(const SpxMscCommon& a, const int* off, long long id) {
    MscSource s;
    s.k = s.off = 0;
    s.h = s.w = 1;
    s.rh = s.rw = 1.0f;
    s.local = 0;
    s.grad = nullptr;
#pragma unroll
    for (int q = 0; q < SPX_MSC_MAX_MAPS; ++q) {
        if (q < a.d.K && id >= a.gofs[q] && id < a.gofs[q + 1]) {
            s.k = q;
            s.h = a.d.maps[q].h;
            s.w = a.d.maps[q].w;
            s.rh = a.rh[q];
            s.rw = a.rw[q];
            if (off) s.off = off[q];
            s.local = id - a.gofs[q];
            s.grad = a.d.grads[q];
        }
    }
    s.j = (int)(s.local % s.w);
    s.i = (int)((s.local / s.w) % s.h);
    s.plane = s.local / ((long long)s.w * s.h);
    return s;
}

// The term of the maximum for source element s: the upstream terms of the H x W destination pixels whose index names map s.k,
// added to acc in ascending (Y, X) order.  Map 0 is its own pixel.  A scaled map gathers over the pixels whose footprint can
// hold (i, j), with the forward's weights: acc += g . wy . wx.  Pixel (Y, X) is element gbase + Y W + X of the upstream gradient
// and of the saved output, and element ibase + Y W + X of the index.  has_own: acc holds the element's own term (the pack);
// without one, map 0's term is the result as it stands, not 0 + term (a -0 keeps its sign).
__device__ __forceinline__ float msc_max_term(const SpxMscCommon& a, const MscSource& s, long long gbase, long long ibase, float acc,
                                              bool has_own) {
    const spx_msc& d = a.d;
    const int H = a.H, W = a.W, k = s.k, i = s.i, j = s.j;
    if (k == 0) {
        const long long p = (long long)i * W + j;
        if (d.index && d.index[ibase + p] != 0) return acc;
        const float g = msc_upstream(d, gbase + p);
        return has_own ? acc + g : g;
    }
    int ylo, yhi, xlo, xhi;
    msc_dst_range(s.rh, s.h, H, i, ylo, yhi);
    msc_dst_range(s.rw, s.w, W, j, xlo, xhi);
    for (int Y = ylo; Y <= yhi; ++Y) {
        int i0, i1;
        float ly;
        msc_src(s.rh, s.h, Y, i0, i1, ly);
        const float wy = (i0 == i ? 1.0f - ly : 0.0f) + (i1 == i ? ly : 0.0f);
        if (i0 != i && i1 != i) continue;
        for (int X = xlo; X <= xhi; ++X) {
            int j0, j1;
            float lx;
            msc_src(s.rw, s.w, X, j0, j1, lx);
            if (j0 != j && j1 != j) continue;
            const long long p = (long long)Y * W + X;
            if (d.index[ibase + p] != k) continue;
            const float wx = (j0 == j ? 1.0f - lx : 0.0f) + (j1 == j ? lx : 0.0f);
            acc += msc_upstream(d, gbase + p) * wy * wx;
        }
    }
    return acc;
}

__global__ __launch_bounds__(MSC_THREADS) void spx_msc_max_bwd_kernel(const SpxMscArgs a) {
    const long long id = (long long)blockIdx.x * MSC_THREADS + threadIdx.x;
    if (id >= a.gofs[SPX_MSC_MAX_MAPS]) return;
    const MscSource s = msc_source(a, nullptr, id);
    const long long base = s.plane * a.H * a.W;
    msc_store(s.grad, a.d.in_dtype == 0, s.local, msc_max_term(a, s, base, base, 0.0f, false));
}

// d, H, W and the ratios of every map
static void msc_fill(SpxMscCommon& a, const spx_msc& d) {
    a.d = d;
    a.H = d.maps[0].h;
    a.W = d.maps[0].w;
    for (int k = 0; k < SPX_MSC_MAX_MAPS; ++k) {
        a.rh[k] = a.rw[k] = 1.0f;
        if (k < d.K) {
            a.rh[k] = (float)d.maps[k].h / (float)a.H;
            a.rw[k] = (float)d.maps[k].w / (float)a.W;
        }
    }
}
// gofs of the backward: one thread per element of every map that gets a gradient; returns their number
static long long msc_grad_offsets(SpxMscCommon& a) {
    const spx_msc& d = a.d;
    a.gofs[0] = 0;
    for (int k = 0; k < SPX_MSC_MAX_MAPS; ++k) {
        const long long n = (k < d.K && d.grads[k]) ? (long long)d.B * d.C * d.maps[k].h * d.maps[k].w : 0;
        a.gofs[k + 1] = a.gofs[k] + n;
    }
    return a.gofs[SPX_MSC_MAX_MAPS];
}
// channels per block of a forward whose one pass over the channels takes `blocks` blocks: enough blocks to fill the chip (about
// 8 per CU), then as many channels per block as that leaves, a multiple of `round` - what a thread sets up before its channel
// loop is paid once per block and thread
static int msc_channel_chunk(long long blocks, int C, int round) {
    long long chunks = 2048 / blocks;
    if (chunks < 1) chunks = 1;
    if (chunks > C) chunks = C;
    const int cchunk = (int)((C + chunks - 1) / chunks);
    return (cchunk + round - 1) / round * round;
}

#define MSC_LAUNCH_FWD(kernel)                                                                                   \
    do {                                                                                                         \
        if (d.in_dtype == 0) {                                                                                   \
            if (d.out_dtype == 0) hipLaunchKernelGGL((kernel<true, true>), grid, dim3(MSC_THREADS), 0, s, a);    \
            else hipLaunchKernelGGL((kernel<true, false>), grid, dim3(MSC_THREADS), 0, s, a);                    \
        } else {                                                                                                 \
            if (d.out_dtype == 0) hipLaunchKernelGGL((kernel<false, true>), grid, dim3(MSC_THREADS), 0, s, a);   \
            else hipLaunchKernelGGL((kernel<false, false>), grid, dim3(MSC_THREADS), 0, s, a);                   \
        }                                                                                                        \
    } while (0)

hipError_t spx_launch_msc_max_fwd(const spx_msc& d, hipStream_t s) {
    SpxMscArgs a = {};
    msc_fill(a, d);
    if (d.K == 1) {                 // no geometry: a plane is one row (spx_msc_act_kernel)
        a.W = a.H * a.W;
        a.H = 1;
    }
    a.groups = (a.W + MSC_VEC - 1) / MSC_VEC + 1;
    const size_t esz = d.out_dtype == 0 ? 2 : 4;
    a.out_mis = (int)(((uintptr_t)d.out / esz) & (MSC_VEC - 1));
    const long long tasks = (long long)a.H * a.groups;
    const unsigned bx = (unsigned)((tasks + MSC_THREADS - 1) / MSC_THREADS);
    a.cchunk = msc_channel_chunk((long long)bx * d.B, d.C, d.K == 1 ? MSC_ACT_UNROLL : 1);
    const dim3 grid(bx, (unsigned)((d.C + a.cchunk - 1) / a.cchunk), (unsigned)d.B);
    if (d.K == 1) MSC_LAUNCH_FWD(spx_msc_act_kernel);
    else MSC_LAUNCH_FWD(spx_msc_max_fwd_kernel);
    return hipGetLastError();
}

hipError_t spx_launch_msc_max_bwd(const spx_msc& d, hipStream_t s) {
    SpxMscArgs a = {};
    msc_fill(a, d);
    const long long total = msc_grad_offsets(a);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(spx_msc_max_bwd_kernel, dim3((unsigned)((total + MSC_THREADS - 1) / MSC_THREADS)), dim3(MSC_THREADS), 0, s, a);
    return hipGetLastError();
}

// ---- the packed training maps (spx_msc_pack_fwd / _bwd) ------------------------------------------------------------------------
// The K maps at their own grids and, with_max, their maximum written side by side on ONE pixel axis: out [C, M], pixel (b, i) of
// segment q at column off_q + b . h_q . w_q + i (include/spx_hip.h).  Values, index and rounding are those of the kernels above,
// by the same device functions.
//
//   forward   a thread owns the columns [4 t, 4 t + 4) of a chunk of channels (grid: column groups x channel chunks).  Its four
//       columns are decoded once, before the channel loop: segment, image, pixel.  A group that lies inside one plane of a plain
//       segment, at addresses a vector may take, runs four channels per step with their loads issued together (the K = 1 lesson:
//       the bandwidth-bound case); every other group - the maximum's, those that straddle a segment or an image, those of a
//       buffer whose rows a vector cannot address (M no multiple of 4, a misaligned out) - goes column by column.
//   backward  gather form as above, one thread per source element: first its own segment's term, then the maximum's segment.
struct SpxMscPackArgs : SpxMscCommon {
    int nseg, with_max, off_max, M, cchunk;
    int vec_ok;                                         // forward: M % 4 == 0 and out aligned to a vector
    // first column of every segment; off[nseg] = M.  (Last on purpose: with the scalars behind it the forward kernel spills
    // SGPRs and reserves 36 bytes of scratch per lane.)
    int off[SPX_MSC_MAX_MAPS + 2];
};

struct MscCol {
    const void* data;                                   // plain segment: its map
    long long base;                                     // plain: b . batch_stride + i;  maximum: b
    long long cs;                                       // plain: channel stride
    int seg, b, i;                                      // segment, image, pixel of the plane
};

__device__ __forceinline__ MscCol msc_pack_col(const SpxMscPackArgs& a, int m) {
    MscCol r;
    r.data = nullptr;
    r.base = r.cs = 0;
    r.seg = r.b = r.i = 0;
#pragma unroll
    for (int q = 0; q < SPX_MSC_MAX_MAPS + 1; ++q) {
        if (q < a.nseg && m >= a.off[q] && m < a.off[q + 1]) {
            const bool plain = q < a.d.K;
            const spx_msc_map mp = a.d.maps[q < SPX_MSC_MAX_MAPS ? q : 0];
            const int hw = plain ? mp.h * mp.w : a.H * a.W;
            const int local = m - a.off[q];
            r.seg = q;
            r.b = local / hw;
            r.i = local - r.b * hw;
            r.data = plain ? mp.data : nullptr;
            r.cs = plain ? mp.channel_stride : 0;
            r.base = plain ? (long long)r.b * mp.batch_stride + r.i : (long long)r.b;
        }
    }
    return r;
}

// the value of one column of channel c before the activation; win: the winning map (the maximum's segment only)
template <bool IN_BF16>
__device__ __forceinline__ float msc_pack_value(const SpxMscPackArgs& a, const MscCol& col, int c, int& win) {
    win = 0;
    if (col.seg < a.d.K) return msc_load(col.data, IN_BF16, col.base + (long long)c * col.cs);
    const int W = a.W, K = a.d.K;
    const int Y = col.i / W, X = col.i - Y * W;
    const spx_msc_map m0 = a.d.maps[0];
    float v = msc_load(m0.data, IN_BF16, (long long)col.b * m0.batch_stride + (long long)c * m0.channel_stride + col.i);
    // (a rolled loop on purpose: unrolled, the source positions of 4 columns x 7 maps are hoisted out of the channel loop and
    // take every register the file has; k is uniform, so maps[k] is a scalar load)
#pragma unroll 1
    for (int k = 1; k < K; ++k) {
        const spx_msc_map m = a.d.maps[k];
        int i0, i1, j0, j1;
        float ly, lx;
        msc_src(a.rh[k], m.h, Y, i0, i1, ly);
        msc_src(a.rw[k], m.w, X, j0, j1, lx);
        const long long pl = (long long)col.b * m.batch_stride + (long long)c * m.channel_stride;
        const float u = msc_tap(m.data, IN_BF16, pl + (long long)i0 * m.w, pl + (long long)i1 * m.w, j0, j1, ly, lx);
        if (msc_takes_over(u, v)) {
            v = u;
            win = k;
        }
    }
    return v;
}

template <bool IN_BF16, bool OUT_BF16>
__global__ __launch_bounds__(MSC_THREADS) void spx_msc_pack_fwd_kernel(const SpxMscPackArgs a) {
    const int M = a.M, C = a.d.C;
    const long long first = ((long long)blockIdx.x * MSC_THREADS + threadIdx.x) * MSC_VEC;
    if (first >= M) return;
    const int xs = (int)first;
    const int n = M - xs < MSC_VEC ? M - xs : MSC_VEC;                              // columns [xs, xs + n)
    const int c0 = blockIdx.y * a.cchunk;
    const int c1 = c0 + a.cchunk < C ? c0 + a.cchunk : C;
    const bool sig = a.d.activation == 1;

    MscCol col[MSC_VEC];
    col[0] = msc_pack_col(a, xs);
    col[MSC_VEC - 1] = msc_pack_col(a, xs + n - 1);
    const bool one_plane = n == MSC_VEC && col[0].seg == col[MSC_VEC - 1].seg && col[0].b == col[MSC_VEC - 1].b;
    if (one_plane) {
#pragma unroll
        for (int j = 1; j < MSC_VEC - 1; ++j) {
            col[j] = col[0];
            col[j].i += j;
            if (col[0].seg < a.d.K) col[j].base += j;
        }
    } else {
#pragma unroll
        for (int j = 1; j < MSC_VEC; ++j) col[j] = msc_pack_col(a, xs + j < M ? xs + j : M - 1);
    }

    // whole group in one plane of a plain segment, source and destination addressable as vectors for every channel
    const bool fast = one_plane && a.vec_ok && col[0].seg < a.d.K && (col[0].cs & (MSC_VEC - 1)) == 0 &&
                      msc_group_vector_ok<IN_BF16>(col[0].data, col[0].base, true);
    if (fast) {
        int c = c0;
        for (; c + MSC_ACT_UNROLL <= c1; c += MSC_ACT_UNROLL) {
            float v[MSC_ACT_UNROLL][MSC_VEC];
#pragma unroll
            for (int u = 0; u < MSC_ACT_UNROLL; ++u) msc_load_vector<IN_BF16>(col[0].data, col[0].base + (long long)(c + u) * col[0].cs, v[u]);
            if (sig) {
#pragma unroll
                for (int u = 0; u < MSC_ACT_UNROLL; ++u) msc_sigmoid(v[u]);
            }
#pragma unroll
            for (int u = 0; u < MSC_ACT_UNROLL; ++u) msc_store_vector<OUT_BF16>(a.d.out, (long long)(c + u) * M + xs, v[u]);
        }
        for (; c < c1; ++c) {
            float v[MSC_VEC];
            msc_load_vector<IN_BF16>(col[0].data, col[0].base + (long long)c * col[0].cs, v);
            if (sig) msc_sigmoid(v);
            msc_store_vector<OUT_BF16>(a.d.out, (long long)c * M + xs, v);
        }
        return;
    }

    const long long HW = (long long)a.H * a.W;
    for (int c = c0; c < c1; ++c) {
        float v[MSC_VEC];
        const long long o = (long long)c * M + xs;
#pragma unroll
        for (int j = 0; j < MSC_VEC; ++j) {
            v[j] = 0.0f;
            if (j >= n) continue;
            int win;
            v[j] = msc_pack_value<IN_BF16>(a, col[j], c, win);
            if (sig) v[j] = msc_sigmoid(v[j]);
            if (col[j].seg >= a.d.K && a.d.index) a.d.index[((long long)col[j].b * C + c) * HW + col[j].i] = (uint8_t)win;
        }
        if (a.vec_ok && n == MSC_VEC) {
            msc_store_vector<OUT_BF16>(a.d.out, o, v);
        } else {
#pragma unroll
            for (int j = 0; j < MSC_VEC; ++j)
                if (j < n) msc_store(a.d.out, OUT_BF16, o + j, v[j]);
        }
    }
}

__global__ __launch_bounds__(MSC_THREADS) void spx_msc_pack_bwd_kernel(const SpxMscPackArgs a) {
    const long long id = (long long)blockIdx.x * MSC_THREADS + threadIdx.x;
    if (id >= a.gofs[SPX_MSC_MAX_MAPS]) return;
    const MscSource s = msc_source(a, a.off, id);
    const int C = a.d.C;
    const int b = (int)(s.plane / C), c = (int)(s.plane - (long long)b * C);
    const long long row = (long long)c * a.M;

    // the map's own segment first
    float acc = msc_upstream(a.d, row + s.off + (long long)b * s.h * s.w + (long long)s.i * s.w + s.j);
    if (a.with_max)                                                               // (the index is [B, C, H, W])
        acc = msc_max_term(a, s, row + a.off_max + (long long)b * a.H * a.W, s.plane * a.H * a.W, acc, true);
    msc_store(s.grad, a.d.in_dtype == 0, s.local, acc);
}

static void msc_pack_fill(SpxMscPackArgs& a, const spx_msc& d, int with_max) {
    msc_fill(a, d);
    a.with_max = with_max ? 1 : 0;
    a.nseg = d.K + a.with_max;
    long long m = 0;
    for (int k = 0; k < SPX_MSC_MAX_MAPS + 2; ++k) {
        a.off[k] = (int)m;
        if (k < d.K) m += (long long)d.B * d.maps[k].h * d.maps[k].w;
        else if (k == d.K && with_max) m += (long long)d.B * a.H * a.W;
    }
    a.M = (int)m;                                        // (< 2^31: checked by the entry point)
    a.off_max = a.off[d.K];
}

hipError_t spx_launch_msc_pack_fwd(const spx_msc& d, int with_max, hipStream_t s) {
    SpxMscPackArgs a = {};
    msc_pack_fill(a, d, with_max);
    const size_t vbytes = d.out_dtype == 0 ? 8 : 16;
    a.vec_ok = (a.M % MSC_VEC == 0 && (uintptr_t)d.out % vbytes == 0) ? 1 : 0;
    const long long groups = ((long long)a.M + MSC_VEC - 1) / MSC_VEC;
    const unsigned bx = (unsigned)((groups + MSC_THREADS - 1) / MSC_THREADS);
    a.cchunk = msc_channel_chunk(bx, d.C, MSC_ACT_UNROLL);                        // (the four channels of a step)
    const dim3 grid(bx, (unsigned)((d.C + a.cchunk - 1) / a.cchunk), 1);
    MSC_LAUNCH_FWD(spx_msc_pack_fwd_kernel);
    return hipGetLastError();
}

hipError_t spx_launch_msc_pack_bwd(const spx_msc& d, int with_max, hipStream_t s) {
    SpxMscPackArgs a = {};
    msc_pack_fill(a, d, with_max);
    const long long total = msc_grad_offsets(a);
    if (total == 0) return hipSuccess;
    hipLaunchKernelGGL(spx_msc_pack_bwd_kernel, dim3((unsigned)((total + MSC_THREADS - 1) / MSC_THREADS)), dim3(MSC_THREADS), 0, s, a);
    return hipGetLastError();
}
