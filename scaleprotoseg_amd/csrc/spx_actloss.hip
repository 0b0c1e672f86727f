// Activation losses over class-gathered planes (reference: segmentation/model/loss.py:149-348): spatial entropy, sample entropy
// and activation norm of the labelled pixels, fused.
//
// Input: vals [B, J, HW] (slot planes: activations, or distances with the activation applied at load), labels [B, HW]
// (class 0..K-1, else none), slot_scale [K, J] (scale id of (class, slot); -1 = no such slot, -2 = a slot outside every scale).
// A segment is (image b, class c) with n pixels and Jc slots; a = activation of a pixel of the segment for slot j.
//   spatial entropy  segments with n >= 2:  mean_j H_j / ln n,  H_j = -sum_px p ln p,  p = softmax over the segment's pixels of a_j
//   sample entropy   items (b, c, scale) with n >= 1 and ns >= 2 slots of that scale:  mean_px H_px / ln ns,  H_px = entropy of the
//                    softmax over the ns slots
//   norm             segments with n >= 1:  mean_j (sum_px |a| / n)  (l1)  or  mean_j max_px |a|  (linf)
// each the mean over its segments / items.  Two streaming reduction passes in the manner of spx_kld.hip (same pixel walk, same
// one-step-ahead fetch, per-workgroup LDS tables, INTEGER atomics only: ordered keys for maxima, 64-bit fixed point for sums, so
// the result does not depend on the order of arrival), one single-workgroup finish kernel, one per-pixel gradient pass.
//   pass A  per (b, c, j): max a, max |a|;  per (b, c): n;  the global max |a| (fixed-point scale of the l1 sums)
//   pass B  per (b, c, j): S0 = sum e^(a-m) [2^40], -S1 = -sum (a-m) e^(a-m) [2^32: a term is in [0, 1/e]], sum |a| [scale from
//           the global max: HW terms stay below 2^62], number of pixels with |a| = max |a|;  per (b, c, group): sum_px H_px [2^32:
//           a term is in [0, ln 16]].  Then H_j = ln S0 - S1 / S0, lse_j = m + ln S0.
//   finish  terms, reciprocal item counts, weighted total, and per (segment, slot) the coefficients of the gradient pass
//   backward  d/da = -p (a - lse_j + H_j) cS  +  sample-entropy term recomputed per pixel  +  sign(a) [tie mask] cN, times a'(d)
#include "spx_kld_walk.h"

#define SPX_ACT_TABLE_LDS (60 * 1024)        // LDS budget of the per-class tables of pass B and the gradient pass (class blocks beyond it)
#define SPX_ACT_COEFS 6                      // per (segment, slot): lse, H, max |a|, cS, cN, cG
#define SPX_ACT_FX40 1099511627776.0         // 2^40
#define SPX_ACT_FX32 4294967296.0            // 2^32

extern __shared__ unsigned long long act_smem[];

// the integer tables of one call inside the caller's zero-filled workspace
struct SpxActWs {
    unsigned long long *s0, *s1, *sabs, *samp;            // [B, K, J] each (samp: [B, K, group])
    unsigned int *amax, *absmax, *tie, *counts, *gmax;    // [B, K, J] x 3, [B, K], [1]
};
__host__ __device__ inline SpxActWs spx_act_ws(void* base, int B, int K, int J) {
    const size_t ns = (size_t)B * K * J;
    SpxActWs w;
    unsigned long long* p = (unsigned long long*)base;
    w.s0 = p;
    w.s1 = p + ns;
    w.sabs = p + 2 * ns;
    w.samp = p + 3 * ns;
    unsigned int* q = (unsigned int*)(p + 4 * ns);
    w.amax = q;
    w.absmax = q + ns;
    w.tie = q + 2 * ns;
    w.counts = q + 3 * ns;
    w.gmax = q + 3 * ns + (size_t)B * K;
    return w;
}
size_t spx_actloss_ws_bytes(int B, int K, int J) {
    const size_t ns = (size_t)B * K * J;
    return 4 * ns * 8 + ((3 * ns + (size_t)B * K + 1) * 4 + 7) / 8 * 8;
}

// The sample-entropy groups of a class: the slots of one scale (id >= 0) form a group if there are at least two of them
// (a single slot has entropy 0 / ln 1: skipped); group g = rank of the scale's first slot among the groups.
//   code: 4 bits per slot, the slot's group or 0xF;  nsm1: 4 bits per group, its size - 1;  present: bit j = slot j exists
struct SpxActGroups {
    unsigned long long code;
    unsigned int nsm1, present;
    int ng, Jc;
};
__device__ inline SpxActGroups spx_act_groups(const int32_t* __restrict__ sid, int J) {
    SpxActGroups g{~0ull, 0u, 0u, 0, 0};
    for (int j = 0; j < J; ++j) {
        const int s = sid[j];
        if (s == -1) continue;
        g.present |= 1u << j;
        ++g.Jc;
        if (s < 0) continue;
        int cnt = 0, leader = -1;
        for (int k = 0; k < J; ++k)
            if (sid[k] == s) {
                ++cnt;
                if (leader < 0) leader = k;
            }
        if (cnt < 2) continue;
        int gi;
        if (leader == j) {
            gi = g.ng++;
            g.nsm1 |= (unsigned)(cnt - 1) << (4 * gi);
        } else {
            gi = (int)((g.code >> (4 * leader)) & 0xFull);
        }
        g.code = (g.code & ~(0xFull << (4 * j))) | ((unsigned long long)gi << (4 * j));
    }
    return g;
}
__device__ __forceinline__ unsigned int spx_act_meta(const SpxActGroups& g) { return g.present | ((unsigned)g.ng << 16) | ((unsigned)g.Jc << 20); }

// the activation of a plane value (mode 0: the value itself; 1: log((d+1)/(d+eps)); 2: -d)
template <int JT>
__device__ __forceinline__ void spx_act_apply(float (&a)[JT], const float (&d)[JT], int mode, float eps) {
    if (mode == 1) {
#pragma unroll
        for (int j = 0; j < JT; ++j) a[j] = act_log(d[j], eps);
    } else if (mode == 2) {
#pragma unroll
        for (int j = 0; j < JT; ++j) a[j] = -d[j];
    } else {
#pragma unroll
        for (int j = 0; j < JT; ++j) a[j] = d[j];
    }
}

// fixed-point scale of the l1 sums: a power of two such that HW terms of size <= the global max |a| stay below 2^62
__device__ __forceinline__ double spx_act_l1_scale(unsigned int gmax_key, int HW) {
    const double gm = gmax_key ? fmax((double)key_float(gmax_key), 1e-30) : 1.0;
    return exp2(floor(log2(4611686018427387904.0 / ((double)HW * gm))));
}

// entropy of the softmax over the slots of group g of one pixel (0 where the lane's class has no such group); with WANT_GRAD
// also adds its gradient -p_j (ln p_j + H) * cg[j] to grad[j]
template <int JT, bool WANT_GRAD>
__device__ __forceinline__ float spx_act_group_entropy(const float (&a)[JT], unsigned long long code, int g, const float* cg, float (&grad)[JT]) {
    float m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < JT; ++j) m = (int)((code >> (4 * j)) & 0xFull) == g ? fmaxf(m, a[j]) : m;
    float s0 = 0.0f, s1 = 0.0f, e[JT];
#pragma unroll
    for (int j = 0; j < JT; ++j) {
        const bool in = (int)((code >> (4 * j)) & 0xFull) == g;
        const float t = in ? a[j] - m : 0.0f;
        e[j] = in ? __expf(t) : 0.0f;
        s0 += e[j];
        s1 += in ? t * e[j] : 0.0f;
    }
    if (!(s0 > 0.0f)) return 0.0f;
    const float ls = logf(s0), inv = 1.0f / s0;
    const float H = ls - s1 * inv;
    if (WANT_GRAD) {
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const bool in = (int)((code >> (4 * j)) & 0xFull) == g;
            if (in) grad[j] -= e[j] * inv * ((a[j] - m) - ls + H) * cg[j];
        }
    }
    return H;
}

// pass A
template <int JT>
__global__ __launch_bounds__(SPX_KLD_THREADS) void spx_act_max_kernel(const float* __restrict__ vals, const int32_t* __restrict__ labels,
                                                                     const int32_t* __restrict__ sid, int J, int HW, int W, int trows, int K,
                                                                     int mode, float eps, SpxActWs ws) {
    unsigned int* tmax = (unsigned int*)act_smem;         // [K][J] key of max a
    unsigned int* tabs = tmax + K * J;                    // [K][J] key of max |a|
    unsigned int* cnt = tabs + K * J;                     // [K]
    unsigned int* gmx = cnt + K;                          // [1] key of the largest |a| of all
    unsigned int* pm = gmx + 1;                           // [K] present-slot mask
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 2 * K * J + K + 1; i += SPX_KLD_THREADS) tmax[i] = 0u;
    for (int c = tid; c < K; c += SPX_KLD_THREADS) {
        unsigned int m = 0u;
        for (int j = 0; j < J; ++j) m |= sid[c * J + j] != -1 ? 1u << j : 0u;
        pm[c] = m;
    }
    __syncthreads();
    const float* v = vals + (size_t)b * J * HW;
    const int32_t* lab = labels + (size_t)b * HW;
    const SpxKldWalk w = spx_kld_walk(HW, W, trows, lane, wave);
    float m[JT], ma[JT], gm = 0.0f;
#pragma unroll
    for (int j = 0; j < JT; ++j) {
        m[j] = -3.0e38f;
        ma[j] = 0.0f;
    }
    unsigned int run = 0;
    unsigned int pmc;
    float a[JT], aa[JT];
    spx_segment_walk<JT>(
        v, lab, w, J, HW, 0, K,
        [&](const float (&raw)[JT], int c, bool ok) SPX_WALK_INLINE {
            pmc = ok ? pm[c] : 0u;
            spx_act_apply(a, raw, mode, eps);
#pragma unroll
            for (int j = 0; j < JT; ++j) {
                const bool in = (pmc >> j) & 1u;               // (bits at or beyond J are never set)
                aa[j] = in ? fabsf(a[j]) : 0.0f;
                a[j] = in ? a[j] : -3.0e38f;
                gm = fmaxf(gm, aa[j]);
            }
        },
        [&](unsigned long long okm) SPX_WALK_INLINE {
            run += (unsigned)__builtin_popcountll(okm);
#pragma unroll
            for (int j = 0; j < JT; ++j) {
                m[j] = fmaxf(m[j], a[j]);
                ma[j] = fmaxf(ma[j], aa[j]);
            }
        },
        [&](int c) SPX_WALK_INLINE {
            atomicAdd(&cnt[c], 1u);
#pragma unroll
            for (int j = 0; j < JT; ++j)
                if ((pmc >> j) & 1u) {
                    atomicMax(&tmax[c * J + j], float_key(a[j]));
                    atomicMax(&tabs[c * J + j], float_key(aa[j]));
                }
        },
        [&](int cur) SPX_WALK_INLINE {
            const unsigned int pmc = pm[cur];
#pragma unroll
            for (int j = 0; j < JT; ++j)
                if (j < J && ((pmc >> j) & 1u)) {
                    const float wm = wave_max_f32(m[j]), wa = wave_max_f32(ma[j]);
                    if (lane == 0) {
                        atomicMax(&tmax[cur * J + j], float_key(wm));
                        atomicMax(&tabs[cur * J + j], float_key(wa));
                    }
                    m[j] = -3.0e38f;
                    ma[j] = 0.0f;
                }
            if (lane == 0) atomicAdd(&cnt[cur], run);
            run = 0;
        });
    const float wg = wave_max_f32(gm);
    if (lane == 0 && wg > 0.0f) atomicMax(gmx, float_key(wg));
    __syncthreads();
    const size_t base = (size_t)b * K * J;
    for (int i = tid; i < K * J; i += SPX_KLD_THREADS) {
        if (tmax[i]) atomicMax(&ws.amax[base + i], tmax[i]);
        if (tabs[i]) atomicMax(&ws.absmax[base + i], tabs[i]);
    }
    for (int i = tid; i < K; i += SPX_KLD_THREADS)
        if (cnt[i]) atomicAdd(&ws.counts[(size_t)b * K + i], cnt[i]);
    if (tid == 0 && gmx[0]) atomicMax(ws.gmax, gmx[0]);
}

// pass B.  The tables cover the class block [c_lo, c_lo + K) of blockIdx.z (see spx_kld_pairs_kernel): a pixel of another
// block's class is a pixel without a class here, and every segment is summed by exactly one block.
template <int JT>
__global__ __launch_bounds__(SPX_KLD_THREADS) void spx_act_sums_kernel(const float* __restrict__ vals, const int32_t* __restrict__ labels,
                                                                      const int32_t* __restrict__ sid, int J, int HW, int W, int trows, int Kall,
                                                                      int KB, int mode, float eps, int terms, SpxActWs ws) {
    const int c_lo = blockIdx.z * KB, K = min(KB, Kall - c_lo);
    unsigned long long* t0 = act_smem;                     // [K][J] S0
    unsigned long long* t1 = t0 + KB * J;                  // [K][J] -S1
    unsigned long long* ta = t1 + KB * J;                  // [K][J] sum |a|
    unsigned long long* th = ta + KB * J;                  // [K][group] sum of the pixels' sample entropies
    unsigned long long* gcode = th + KB * J;               // [K]
    double* l1s = (double*)(gcode + KB);                   // [1]
    float* mx = (float*)(l1s + 1);                         // [K][J] max a
    float* amx = mx + KB * J;                              // [K][J] max |a|
    unsigned int* tt = (unsigned int*)(amx + KB * J);      // [K][J] pixels at max |a|
    unsigned int* meta = tt + KB * J;                      // [K]
    const int b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t base = ((size_t)b * Kall + c_lo) * J;
    for (int i = tid; i < K * J; i += SPX_KLD_THREADS) {
        t0[i] = 0ull;
        t1[i] = 0ull;
        ta[i] = 0ull;
        th[i] = 0ull;
        tt[i] = 0u;
        const unsigned int k0 = ws.amax[base + i], k1 = ws.absmax[base + i];
        mx[i] = k0 ? key_float(k0) : 0.0f;
        amx[i] = k1 ? key_float(k1) : 0.0f;
    }
    for (int c = tid; c < K; c += SPX_KLD_THREADS) {
        const SpxActGroups g = spx_act_groups(sid + (size_t)(c_lo + c) * J, J);
        gcode[c] = g.code;
        meta[c] = spx_act_meta(g);
    }
    if (tid == 0) l1s[0] = spx_act_l1_scale(ws.gmax[0], HW);
    __syncthreads();
    const double l1scale = l1s[0];
    const bool want_spat = terms & SPX_ACT_SPAT, want_sampl = terms & SPX_ACT_SAMPL, want_norm = terms & SPX_ACT_NORM;
    const float* v = vals + (size_t)b * J * HW;
    const int32_t* lab = labels + (size_t)b * HW;
    const SpxKldWalk w = spx_kld_walk(HW, W, trows, lane, wave);
    constexpr int GT = JT / 2;                             // at most J / 2 groups of >= 2 slots
    float a0[JT], a1[JT], aa[JT], at[JT], ah[GT];          // <= 16 terms (steps of the walk) each: fp32 is ample
#pragma unroll
    for (int j = 0; j < JT; ++j) a0[j] = a1[j] = aa[j] = at[j] = 0.0f;
#pragma unroll
    for (int g = 0; g < GT; ++g) ah[g] = 0.0f;
    // own copy of spx_segment_walk's loop: on the walker three of the four instances lose an occupancy step (profiles/segment_walk_summary.md)
    int cur = -1;
    auto publish = [&]() {
        if (cur < 0) return;
        const unsigned int mt = meta[cur];
        const int ng = (mt >> 16) & 0xF;
#pragma unroll
        for (int j = 0; j < JT; ++j)
            if (j < J && ((mt >> j) & 1u)) {
                if (want_spat) {
                    const double s0 = wave_sum_f64((double)a0[j]);
                    const double s1 = (double)wave_sum_f32(a1[j]);
                    if (lane == 0) {
                        atomicAdd(&t0[cur * J + j], (unsigned long long)(s0 * SPX_ACT_FX40 + 0.5));
                        atomicAdd(&t1[cur * J + j], (unsigned long long)(s1 * SPX_ACT_FX32 + 0.5));
                    }
                }
                if (want_norm) {
                    const double sa = wave_sum_f64((double)aa[j]);
                    const float st = wave_sum_f32(at[j]);                   // a count <= 1024: exact
                    if (lane == 0) {
                        atomicAdd(&ta[cur * J + j], (unsigned long long)(sa * l1scale + 0.5));
                        atomicAdd(&tt[cur * J + j], (unsigned int)(st + 0.5f));
                    }
                }
                a0[j] = a1[j] = aa[j] = at[j] = 0.0f;
            }
        if (want_sampl) {
#pragma unroll
            for (int g = 0; g < GT; ++g)
                if (g < ng) {
                    const double sh = wave_sum_f64((double)ah[g]);
                    if (lane == 0) atomicAdd(&th[cur * J + g], (unsigned long long)(sh * SPX_ACT_FX32 + 0.5));
                    ah[g] = 0.0f;
                }
        }
    };
    SpxKldStep<JT> nx;
    spx_kld_fetch(nx, v, lab, w, 0, J, HW);
    for (int step = 0; step < w.nsteps; ++step) {
        const SpxKldStep<JT> cs = nx;
        spx_kld_fetch(nx, v, lab, w, step + 1, J, HW);
        const int c = step < w.nvalid ? cs.c - c_lo : -1;
        const bool ok = c >= 0 && c < K;
        const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
        const int c0 = okm ? __builtin_amdgcn_readlane(c, __builtin_ffsll((long long)okm) - 1) : -1;
        const bool uniform = __builtin_amdgcn_ballot_w64(ok && c != c0) == 0;
        if (okm == 0) continue;                            // a step without a pixel of this block's classes
        const int cc = ok ? c : 0;
        const unsigned int mt = ok ? meta[cc] : 0u;
        const unsigned long long code = ok ? gcode[cc] : ~0ull;
        const int ng = (mt >> 16) & 0xF;
        float a[JT], e0[JT], e1[JT], ea[JT], et[JT], eh[GT], unused[JT];
        spx_act_apply(a, cs.d, mode, eps);
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const bool in = (mt >> j) & 1u;
            const int jj = min(j, J - 1);
            const float t = in ? a[j] - mx[cc * J + jj] : 0.0f;
            const float e = (in && want_spat) ? __expf(t) : 0.0f;
            e0[j] = e;
            e1[j] = -t * e;
            ea[j] = (in && want_norm) ? fabsf(a[j]) : 0.0f;
            et[j] = (in && want_norm && fabsf(a[j]) == amx[cc * J + jj]) ? 1.0f : 0.0f;
        }
#pragma unroll
        for (int g = 0; g < GT; ++g) {
            eh[g] = 0.0f;
            if (want_sampl && __builtin_amdgcn_ballot_w64(g < ng) != 0) eh[g] = spx_act_group_entropy<JT, false>(a, code, g, nullptr, unused);
        }
        if (uniform) {
            if (c0 != cur) {
                publish();
                cur = c0;
            }
#pragma unroll
            for (int j = 0; j < JT; ++j) {
                a0[j] += e0[j];
                a1[j] += e1[j];
                aa[j] += ea[j];
                at[j] += et[j];
            }
#pragma unroll
            for (int g = 0; g < GT; ++g) ah[g] += eh[g];
        } else if (ok) {
#pragma unroll
            for (int j = 0; j < JT; ++j)
                if ((mt >> j) & 1u) {
                    if (want_spat) {
                        atomicAdd(&t0[c * J + j], (unsigned long long)((double)e0[j] * SPX_ACT_FX40 + 0.5));
                        atomicAdd(&t1[c * J + j], (unsigned long long)((double)e1[j] * SPX_ACT_FX32 + 0.5));
                    }
                    if (want_norm) {
                        atomicAdd(&ta[c * J + j], (unsigned long long)((double)ea[j] * l1scale + 0.5));
                        if (et[j] != 0.0f) atomicAdd(&tt[c * J + j], 1u);
                    }
                }
            if (want_sampl) {
#pragma unroll
                for (int g = 0; g < GT; ++g)
                    if (g < ng) atomicAdd(&th[c * J + g], (unsigned long long)((double)eh[g] * SPX_ACT_FX32 + 0.5));
            }
        }
    }
    publish();
    __syncthreads();
    for (int i = tid; i < K * J; i += SPX_KLD_THREADS) {
        if (t0[i]) atomicAdd(&ws.s0[base + i], t0[i]);
        if (t1[i]) atomicAdd(&ws.s1[base + i], t1[i]);
        if (ta[i]) atomicAdd(&ws.sabs[base + i], ta[i]);
        if (th[i]) atomicAdd(&ws.samp[base + i], th[i]);
        if (tt[i]) atomicAdd(&ws.tie[base + i], tt[i]);
    }
}

// finish: one workgroup.  out[0..2] = the terms (spatial entropy, sample entropy, norm), out[3..5] = 1 / max(1, number of
// segments / items of the term), out[6] = the weighted total; coef [B*K][SPX_ACT_COEFS][J].  Fixed-order sums.
__global__ __launch_bounds__(256) void spx_act_finish_kernel(const int32_t* __restrict__ sid, int B, int K, int J, int HW, int terms, int norm_type,
                                                             float w0, float w1, float w2, SpxActWs ws, float* __restrict__ coef,
                                                             float* __restrict__ out) {
    __shared__ double red[6][256];
    const int tid = threadIdx.x, nseg = B * K;
    const double l1scale = spx_act_l1_scale(ws.gmax[0], HW);
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // value and count of: spatial, sample, norm
    for (int seg = tid; seg < nseg; seg += 256) {
        const int c = seg % K;
        const SpxActGroups g = spx_act_groups(sid + (size_t)c * J, J);
        const unsigned int n = ws.counts[seg];
        float* cf = coef + (size_t)seg * SPX_ACT_COEFS * J;
        for (int i = 0; i < SPX_ACT_COEFS * J; ++i) cf[i] = 0.0f;
        if (n == 0u || g.Jc == 0) continue;
        double hs = 0.0, nv = 0.0;
        for (int j = 0; j < J; ++j) {
            if (!((g.present >> j) & 1u)) continue;
            const size_t i = (size_t)seg * J + j;
            const double am = (double)key_float(ws.absmax[i]);
            cf[2 * J + j] = (float)am;
            if ((terms & SPX_ACT_SPAT) && n >= 2u) {
                const double S0 = (double)ws.s0[i] * (1.0 / SPX_ACT_FX40), X = (double)ws.s1[i] * (1.0 / SPX_ACT_FX32);
                const double lS = log(S0), H = lS + X / S0;
                cf[j] = (float)((double)key_float(ws.amax[i]) + lS);
                cf[J + j] = (float)H;
                hs += H;
            }
            if (terms & SPX_ACT_NORM) nv += norm_type == 0 ? (double)ws.sabs[i] / l1scale / (double)n : am;
        }
        if ((terms & SPX_ACT_SPAT) && n >= 2u) {
            acc[0] += hs / ((double)g.Jc * log((double)n));
            acc[1] += 1.0;
        }
        if (terms & SPX_ACT_SAMPL)
            for (int q = 0; q < g.ng; ++q) {
                const double ns = (double)(((g.nsm1 >> (4 * q)) & 0xFu) + 1u);
                acc[2] += (double)ws.samp[(size_t)seg * J + q] * (1.0 / SPX_ACT_FX32) / ((double)n * log(ns));
                acc[3] += 1.0;
            }
        if (terms & SPX_ACT_NORM) {
            acc[4] += nv / (double)g.Jc;
            acc[5] += 1.0;
        }
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) red[q][tid] = acc[q];
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (tid < m)
            for (int q = 0; q < 6; ++q) red[q][tid] += red[q][tid + m];
        __syncthreads();
    }
    const double inv_s = 1.0 / fmax(red[1][0], 1.0), inv_i = 1.0 / fmax(red[3][0], 1.0), inv_n = 1.0 / fmax(red[5][0], 1.0);
    if (tid == 0) {
        const float ts = (float)(red[0][0] * inv_s), ti = (float)(red[2][0] * inv_i), tn = (float)(red[4][0] * inv_n);
        out[0] = ts;
        out[1] = ti;
        out[2] = tn;
        out[3] = (float)inv_s;
        out[4] = (float)inv_i;
        out[5] = (float)inv_n;
        float total = 0.0f;                                // (a term that is not computed does not enter, whatever its weight)
        if (terms & SPX_ACT_SPAT) total += w0 * ts;
        if (terms & SPX_ACT_SAMPL) total += w1 * ti;
        if (terms & SPX_ACT_NORM) total += w2 * tn;
        out[6] = total;
    }
    for (int seg = tid; seg < nseg; seg += 256) {
        const int c = seg % K;
        const SpxActGroups g = spx_act_groups(sid + (size_t)c * J, J);
        const unsigned int n = ws.counts[seg];
        if (n == 0u || g.Jc == 0) continue;
        float* cf = coef + (size_t)seg * SPX_ACT_COEFS * J;
        for (int j = 0; j < J; ++j) {
            if (!((g.present >> j) & 1u)) continue;
            if ((terms & SPX_ACT_SPAT) && n >= 2u) cf[3 * J + j] = (float)(inv_s / ((double)g.Jc * log((double)n)));
            if (terms & SPX_ACT_NORM) {
                const double t = norm_type == 0 ? (double)n : (double)max(ws.tie[(size_t)seg * J + j], 1u);
                cf[4 * J + j] = (float)(inv_n / ((double)g.Jc * t));
            }
            const int q = (int)((g.code >> (4 * j)) & 0xFull);
            if ((terms & SPX_ACT_SAMPL) && q != 0xF) {
                const double ns = (double)(((g.nsm1 >> (4 * q)) & 0xFu) + 1u);
                cf[5 * J + j] = (float)(inv_i / ((double)n * log(ns)));
            }
        }
    }
}

// backward: one pass over the pixels, no reduction.  eff_i = g_total * w_i + g_terms[i] is the incoming gradient of term i.
template <int JT>
__global__ __launch_bounds__(SPX_KLD_THREADS) void spx_act_backward_kernel(const float* __restrict__ vals, const int32_t* __restrict__ labels,
                                                                          const int32_t* __restrict__ sid, int J, int HW, int Kall, int KB,
                                                                          int mode, float eps, int terms, int norm_type, float w0, float w1, float w2,
                                                                          const float* __restrict__ coef, const float* __restrict__ g_total,
                                                                          const float* __restrict__ g_terms, int ppw, float* __restrict__ grad) {
    const int c_lo = blockIdx.z * KB, K = min(KB, Kall - c_lo);
    unsigned long long* gcode = act_smem;                  // [K]
    float* sc = (float*)(gcode + KB);                      // [K][SPX_ACT_COEFS][JT], the three gradient coefficients times eff
    unsigned int* meta = (unsigned int*)(sc + KB * SPX_ACT_COEFS * JT);      // [K]
    const int b = blockIdx.y, tid = threadIdx.x;
    const float gt = g_total ? g_total[0] : 0.0f;
    const float e0 = (terms & SPX_ACT_SPAT) ? gt * w0 + (g_terms ? g_terms[0] : 0.0f) : 0.0f;
    const float e1 = (terms & SPX_ACT_SAMPL) ? gt * w1 + (g_terms ? g_terms[1] : 0.0f) : 0.0f;
    const float e2 = (terms & SPX_ACT_NORM) ? gt * w2 + (g_terms ? g_terms[2] : 0.0f) : 0.0f;
    for (int i = tid; i < K * SPX_ACT_COEFS * JT; i += SPX_KLD_THREADS) {
        const int c = i / (SPX_ACT_COEFS * JT), q = (i / JT) % SPX_ACT_COEFS, j = i % JT;
        float x = j < J ? coef[(((size_t)b * Kall + c_lo + c) * SPX_ACT_COEFS + q) * J + j] : 0.0f;
        x *= q == 3 ? e0 : (q == 4 ? e2 : (q == 5 ? e1 : 1.0f));
        sc[i] = x;
    }
    for (int c = tid; c < K; c += SPX_KLD_THREADS) {
        const SpxActGroups g = spx_act_groups(sid + (size_t)(c_lo + c) * J, J);
        gcode[c] = g.code;
        meta[c] = spx_act_meta(g);
    }
    __syncthreads();
    const bool want_spat = terms & SPX_ACT_SPAT, want_sampl = terms & SPX_ACT_SAMPL, want_norm = terms & SPX_ACT_NORM;
    const float* v = vals + (size_t)b * J * HW;
    float* go = grad + (size_t)b * J * HW;
    const int32_t* lab = labels + (size_t)b * HW;
    const int px_end = min(HW, (int)(blockIdx.x + 1) * ppw);
    constexpr int GT = JT / 2;
    int px = blockIdx.x * ppw + tid;
    int craw_n = lab[px < px_end ? px : 0];
    float d_n[JT];
    spx_kld_load_planes(d_n, v, J, HW, px < px_end ? px : 0);
    for (; px < px_end; px += SPX_KLD_THREADS) {
        const int craw = craw_n, c = craw - c_lo;
        float d[JT];
#pragma unroll
        for (int j = 0; j < JT; ++j) d[j] = d_n[j];
        {
            const int pn = px + SPX_KLD_THREADS < px_end ? px + SPX_KLD_THREADS : 0;
            craw_n = lab[pn];
            spx_kld_load_planes(d_n, v, J, HW, pn);
        }
        const bool ok = c >= 0 && c < K;
        if (!ok && !(blockIdx.z == 0 && (craw < 0 || craw >= Kall))) continue;      // another block's pixel
        const int cc = ok ? c : 0;
        const unsigned int mt = ok ? meta[cc] : 0u;
        const unsigned long long code = ok ? gcode[cc] : ~0ull;
        const int ng = (mt >> 16) & 0xF;
        const float* s = sc + cc * SPX_ACT_COEFS * JT;
        float a[JT], g[JT];
        spx_act_apply(a, d, mode, eps);
#pragma unroll
        for (int j = 0; j < JT; ++j) {
            const bool in = (mt >> j) & 1u;
            float r = 0.0f;
            if (want_spat) {
                const float cS = s[3 * JT + j];                           // 0: the segment is not part of the term (no lse either)
                const float l = (in && cS != 0.0f) ? a[j] - s[j] : 0.0f;  // ln p
                r = -__expf(l) * (l + s[JT + j]) * cS;
            }
            if (want_norm) {
                const float sg = a[j] > 0.0f ? 1.0f : (a[j] < 0.0f ? -1.0f : 0.0f);
                const bool hit = norm_type == 0 || fabsf(a[j]) == s[2 * JT + j];
                r += hit ? sg * s[4 * JT + j] : 0.0f;
            }
            g[j] = in ? r : 0.0f;
        }
        if (want_sampl) {
#pragma unroll
            for (int q = 0; q < GT; ++q)
                if (q < ng) spx_act_group_entropy<JT, true>(a, code, q, s + 5 * JT, g);
        }
#pragma unroll
        for (int j = 0; j < JT; ++j)
            if (j < J) {
                float da = 1.0f;                                               // a'(d)
                if (mode == 1) da = 1.0f / (d[j] + 1.0f) - 1.0f / (d[j] + eps);
                if (mode == 2) da = -1.0f;
                const bool in = (mt >> j) & 1u;
                go[(size_t)j * HW + px] = in ? g[j] * da : 0.0f;
            }
    }
}

hipError_t spx_launch_actloss_max(const spx_actloss* p, void* workspace, hipStream_t s) {
    const int B = p->B, J = p->J, HW = p->HW, W = p->W, K = p->K;
    dim3 grid;
    const int trows = spx_segment_tile_rows(B, HW, W, grid);
    const size_t lds = ((size_t)2 * K * J + 2 * K + 1) * 4;
    const SpxActWs ws = spx_act_ws(workspace, B, K, J);
    spx_dispatch_jt(J, [&](auto jt) {
        hipLaunchKernelGGL(spx_act_max_kernel<decltype(jt)::value>, grid, dim3(SPX_KLD_THREADS), lds, s, p->vals, p->labels, p->slot_scale, J, HW, W,
                           trows, K, p->mode, p->epsilon, ws);
    });
    return hipGetLastError();
}

hipError_t spx_launch_actloss_sums(const spx_actloss* p, void* workspace, hipStream_t s) {
    const int B = p->B, J = p->J, HW = p->HW, W = p->W, K = p->K;
    dim3 grid;
    const int trows = spx_segment_tile_rows(B, HW, W, grid);
    const size_t per_class = (size_t)J * (4 * 8 + 3 * 4) + 8 + 4;
    const int KB = spx_segment_class_block(K, per_class, SPX_ACT_TABLE_LDS - 16);
    grid.z = (unsigned)((K + KB - 1) / KB);
    const size_t lds = (size_t)KB * per_class + 16;
    const SpxActWs ws = spx_act_ws(workspace, B, K, J);
    spx_dispatch_jt(J, [&](auto jt) {
        hipLaunchKernelGGL(spx_act_sums_kernel<decltype(jt)::value>, grid, dim3(SPX_KLD_THREADS), lds, s, p->vals, p->labels, p->slot_scale, J, HW, W,
                           trows, K, KB, p->mode, p->epsilon, p->terms, ws);
    });
    return hipGetLastError();
}

hipError_t spx_launch_actloss_finish(const spx_actloss* p, void* workspace, float* coef, float* out, hipStream_t s) {
    const SpxActWs ws = spx_act_ws(workspace, p->B, p->K, p->J);
    hipLaunchKernelGGL(spx_act_finish_kernel, dim3(1), dim3(256), 0, s, p->slot_scale, p->B, p->K, p->J, p->HW, p->terms, p->norm_type,
                       p->weights[0], p->weights[1], p->weights[2], ws, coef, out);
    return hipGetLastError();
}

hipError_t spx_launch_actloss_backward(const spx_actloss* p, const float* coef, const float* g_total, const float* g_terms, float* grad,
                                       hipStream_t s) {
    const int B = p->B, J = p->J, HW = p->HW, K = p->K;
    spx_dispatch_jt(J, [&](auto jt) {
        constexpr int JT = decltype(jt)::value;
        const size_t per_class = (size_t)SPX_ACT_COEFS * JT * 4 + 8 + 4;
        const int KB = spx_segment_class_block(K, per_class, SPX_ACT_TABLE_LDS);
        const int ppw = spx_segment_px_per_wg(B, HW);
        const dim3 grid((unsigned)((HW + ppw - 1) / ppw), (unsigned)B, (unsigned)((K + KB - 1) / KB));
        hipLaunchKernelGGL(spx_act_backward_kernel<JT>, grid, dim3(SPX_KLD_THREADS), (size_t)KB * per_class, s, p->vals, p->labels, p->slot_scale, J,
                           HW, K, KB, p->mode, p->epsilon, p->terms, p->norm_type, p->weights[0], p->weights[1], p->weights[2], coef, g_total,
                           g_terms, ppw, grad);
    });
    return hipGetLastError();
}
