// Weight-side regularisers of the training objective (include/spx_hip.h, spx_reg_fwd / spx_reg_bwd): EntropyGroup,
// CrossEntropyGroup and ScaleMax over the per-class group projections (segmentation/model/loss.py:351-464) and the masked
// L1 of the last layer (module_multiscale.py:260-261, module_multiscale_group_train.py:283-285).
//
// Small data (19 x 3 x 12 to 182 x 3 x 12 weights, heads up to [182, 2054]): the cost is launch latency and the dependent
// reduction chain.  Forward = ONE launch: workgroups of SPX_REG_BPW class blocks (one lane per (block, row), (block, pair) or
// (block, scale) task) and of SPX_REG_L1_CHUNK head elements each write four float64 partial sums; the last workgroup to
// draw the integer ticket adds them in a fixed order and writes the terms and the total.  Backward = ONE elementwise launch
// over d_wd and d_head.  No float atomics: results are bit-identical across calls and graph replays.
#include "spx_args.h"

#define SPX_REG_THREADS 256
#define SPX_REG_BPW 8             // class blocks per group workgroup
#define SPX_REG_L1_PER_THREAD 16
#define SPX_REG_L1_CHUNK (SPX_REG_THREADS * SPX_REG_L1_PER_THREAD)
#define SPX_REG_MAX_G 16
#define SPX_REG_MAX_S 16
// task values of one group workgroup: (b, g) entropies, (b, i, l) cross entropies, (b, s) scale maxima
#define SPX_REG_SLOTS (SPX_REG_BPW * (SPX_REG_MAX_G + SPX_REG_MAX_G * (SPX_REG_MAX_G - 1) + SPX_REG_MAX_S))

int spx_reg_group_wgs(const spx_reg& r) {
    return (r.terms & (SPX_REG_ENT | SPX_REG_CEG | SPX_REG_SMAX)) ? (r.nblocks + SPX_REG_BPW - 1) / SPX_REG_BPW : 0;
}
int spx_reg_l1_wgs(const spx_reg& r) {
    return (r.terms & SPX_REG_L1) ? (int)(((long long)r.K * r.Uh + SPX_REG_L1_CHUNK - 1) / SPX_REG_L1_CHUNK) : 0;
}

__device__ __forceinline__ float reg_clamp_eps(float x, float eps) { return x < eps ? eps : x; }   // torch.clamp: NaN stays NaN

// torch.max(dim) over w[g][c0..c1): the first maximal column; a NaN wins (and the first NaN is kept)
__device__ __forceinline__ int reg_first_max(const spx_reg& r, int off, int u, int c0, int c1, float* best) {
    const float* row = r.wd + (size_t)u * r.P;
    float m = row[r.flat_col[off + c0]];
    int at = c0;
    for (int c = c0 + 1; c < c1; ++c) {
        const float v = row[r.flat_col[off + c]];
        if (m == m && (v > m || v != v)) { m = v; at = c; }
    }
    *best = m;
    return at;
}

__device__ __forceinline__ double reg_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__global__ __launch_bounds__(SPX_REG_THREADS) void spx_reg_fwd_kernel(const spx_reg r, int ngroup_wg, int nwg, float* total,
                                                                       float* terms, unsigned* ticket, double* parts) {
    __shared__ float s_val[SPX_REG_SLOTS];
    __shared__ double s_red[8];          // [0..3] per-wave sums, [4..7] final terms; s_red[0] also carries "I am last"
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wg = blockIdx.x;
    double part[4] = {0.0, 0.0, 0.0, 0.0};
    if (wg < ngroup_wg) {
        const int G = r.G, S = r.S;
        const int b0 = wg * SPX_REG_BPW;
        const int nb = min(SPX_REG_BPW, r.nblocks - b0);
        const int n_ent = nb * G, n_ceg = nb * G * (G - 1), n_sm = nb * S;
        for (int t = tid; t < n_ent + n_ceg + n_sm; t += SPX_REG_THREADS) {
            float v = 0.0f;
            if (t < n_ent) {
                if (r.terms & SPX_REG_ENT) {          // -sum_c w log(w + eps) / log(n), loss.py:419-421
                    const int b = b0 + t / G, g = t % G;
                    const int* bi = r.block_info + 4 * b;
                    const float* row = r.wd + (size_t)(bi[2] + g) * r.P;
                    double s = 0.0;
                    for (int c = 0; c < bi[1]; ++c) {
                        const float w = row[r.flat_col[bi[0] + c]];
                        s += (double)(w * logf(w + r.epsilon));
                    }
                    v = -(float)s / logf((float)bi[1]);
                }
            } else if (t < n_ent + n_ceg) {
                if (r.terms & SPX_REG_CEG) {          // sum_c w[i,c] log(clamp(w[l,c], eps)), loss.py:455-457
                    const int q = t - n_ent, pairs = G * (G - 1);
                    const int b = b0 + q / pairs, pr = q % pairs;
                    const int i = pr / (G - 1), l0 = pr % (G - 1), l = l0 < i ? l0 : l0 + 1;
                    const int* bi = r.block_info + 4 * b;
                    const float* ri = r.wd + (size_t)(bi[2] + i) * r.P;
                    const float* rl = r.wd + (size_t)(bi[2] + l) * r.P;
                    double s = 0.0;
                    for (int c = 0; c < bi[1]; ++c) {
                        const int p = r.flat_col[bi[0] + c];
                        s += (double)(ri[p] * logf(reg_clamp_eps(rl[p], r.epsilon)));
                    }
                    v = (float)s;
                }
            } else if (r.terms & SPX_REG_SMAX) {      // mean_g max_(c in span) w, loss.py:385-387
                const int q = t - n_ent - n_ceg;
                const int b = b0 + q / S, sc = q % S;
                const int* bi = r.block_info + 4 * b;
                const int c0 = r.spans[(b * S + sc) * 2], c1 = r.spans[(b * S + sc) * 2 + 1];
                if (c1 > c0) {
                    float acc = 0.0f;
                    for (int g = 0; g < G; ++g) {
                        float m;
                        reg_first_max(r, bi[0], bi[2] + g, c0, c1, &m);
                        acc += m;
                    }
                    v = acc / (float)G;
                }
            }
            s_val[t] = v;
        }
        __syncthreads();
        // fixed-order block sums: one thread per term
        if (tid < 3) {
            const int lo = tid == 0 ? 0 : (tid == 1 ? n_ent : n_ent + n_ceg);
            const int hi = tid == 0 ? n_ent : (tid == 1 ? n_ent + n_ceg : n_ent + n_ceg + n_sm);
            double s = 0.0;
            for (int t = lo; t < hi; ++t) s += (double)s_val[t];
            part[tid] = s;
        }
    } else {
        // |head * (1 - ident^T)| over this workgroup's chunk of the flat [K, Uh] index
        const long long n = (long long)r.K * r.Uh;
        const long long base = (long long)(wg - ngroup_wg) * SPX_REG_L1_CHUNK + tid;
        double s = 0.0;
#pragma unroll 4
        for (int e = 0; e < SPX_REG_L1_PER_THREAD; ++e) {
            const long long f = base + (long long)e * SPX_REG_THREADS;
            if (f < n) {
                const int k = (int)(f / r.Uh), u = (int)(f - (long long)k * r.Uh);
                s += (double)fabsf(r.head[f] * (1.0f - r.ident[(size_t)u * r.K + k]));
            }
        }
        s = reg_wave_sum(s);
        if (lane == 0) s_red[wave] = s;
        __syncthreads();
        if (tid == 3) part[3] = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
    }
    // publish this workgroup's partials; the last workgroup to arrive adds all of them in workgroup order
    if (tid < 4) parts[(size_t)wg * 4 + tid] = part[tid];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        s_red[0] = (t == (unsigned)(nwg - 1)) ? 1.0 : 0.0;
    }
    __syncthreads();
    if (s_red[0] == 0.0) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    {
        double s = 0.0;
        for (int w = lane; w < nwg; w += 64) s += parts[(size_t)w * 4 + wave];
        s = reg_wave_sum(s);
        if (lane == 0) s_red[4 + wave] = s;
    }
    __syncthreads();
    if (tid == 0) {
        const int G = r.G;
        const float ent = (r.terms & SPX_REG_ENT) ? (float)(s_red[4] / (double)(r.nblocks * G)) : 0.0f;
        const float ceg = (r.terms & SPX_REG_CEG) ? (float)(s_red[5] / (double)(r.nblocks * G * (G - 1))) : 0.0f;
        const float smx = (r.terms & SPX_REG_SMAX) ? -(float)(s_red[6] / (double)r.nspans) : 0.0f;
        const float l1 = (r.terms & SPX_REG_L1) ? (float)s_red[7] : 0.0f;
        terms[0] = ent;
        terms[1] = ceg;
        terms[2] = smx;
        terms[3] = l1;
        total[0] = ((r.weights[3] * l1 + r.weights[1] * ceg) + r.weights[2] * smx) + r.weights[0] * ent;
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next call / replay
    }
}

// Gradients in the order of torch's autograd of the reference forms (so the non-finite cases come out the same):
//   EntropyGroup   gs = -((up / N) / log n);  d w = gs * log(w + eps) + (gs * w) / (w + eps)
//   CrossEntropy   q = -((-up) / N);          d w[i] += q log(clamp(w[l])) (l != i);  d w[l] += [w[l] >= eps] (q w[i]) / clamp(w[l])
//   ScaleMax       d w[g][first max of the span] += ((-up) / N) / G
//   L1             d head = (sgn(head * m) * up) * m,  m = 1 - ident^T
__global__ __launch_bounds__(SPX_REG_THREADS) void spx_reg_bwd_kernel(const spx_reg r, long long n_wd, long long n_head,
                                                                       const float* g_total, const float* g_terms, float* d_wd,
                                                                       float* d_head) {
    const long long i = (long long)blockIdx.x * SPX_REG_THREADS + threadIdx.x;
    if (i >= n_wd + n_head) return;
    float up[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) up[t] = (g_total ? g_total[0] * r.weights[t] : 0.0f) + (g_terms ? g_terms[t] : 0.0f);
    if (i >= n_wd) {
        const long long f = i - n_wd;
        const int k = (int)(f / r.Uh), u = (int)(f - (long long)k * r.Uh);
        const float m = 1.0f - r.ident[(size_t)u * r.K + k];
        const float x = r.head[f] * m;
        const float sg = x != x ? x : (float)((x > 0.0f) - (x < 0.0f));
        d_head[f] = (sg * up[3]) * m;
        return;
    }
    const int u = (int)(i / r.P), p = (int)(i - (long long)u * r.P);
    const int jb = r.row_block[u];
    if (jb < 0 || jb != r.col_block[p]) {
        d_wd[i] = 0.0f;
        return;
    }
    const int G = r.G, g = r.row_local[u], c = r.col_local[p];
    const int* bi = r.block_info + 4 * jb;
    const int n = bi[1], u0 = bi[2];
    const float w = r.wd[i];
    float d = 0.0f;
    if (r.terms & SPX_REG_ENT) {
        const float gs = -((up[0] / (float)(r.nblocks * G)) / logf((float)n));
        const float t = w + r.epsilon;
        d += gs * logf(t) + (gs * w) / t;
    }
    if (r.terms & SPX_REG_CEG) {
        const float q = -((-up[1]) / (float)(r.nblocks * G * (G - 1)));
        const float cw = reg_clamp_eps(w, r.epsilon);
        for (int o = 0; o < G; ++o) {
            if (o == g) continue;
            const float wo = r.wd[(size_t)(u0 + o) * r.P + p];
            d += q * logf(reg_clamp_eps(wo, r.epsilon));            // w as the weighting row i = g, paired with row o
            d += w >= r.epsilon ? (q * wo) / cw : 0.0f;            // w as the clamped row l = g, weighted by row o
        }
    }
    if (r.terms & SPX_REG_SMAX) {
        for (int s = 0; s < r.S; ++s) {
            const int c0 = r.spans[(jb * r.S + s) * 2], c1 = r.spans[(jb * r.S + s) * 2 + 1];
            if (c >= c0 && c < c1) {
                float m;
                if (reg_first_max(r, bi[0], u, c0, c1, &m) == c) d += ((-up[2]) / (float)r.nspans) / (float)G;
                break;
            }
        }
    }
    d_wd[i] = d;
}

hipError_t spx_launch_reg_fwd(const spx_reg& r, float* total, float* terms, void* workspace, hipStream_t s) {
    const int ng = spx_reg_group_wgs(r), nl = spx_reg_l1_wgs(r);
    unsigned* ticket = (unsigned*)workspace;
    double* parts = (double*)((char*)workspace + 64);
    hipLaunchKernelGGL(spx_reg_fwd_kernel, dim3((unsigned)(ng + nl)), dim3(SPX_REG_THREADS), 0, s, r, ng, ng + nl, total, terms,
                       ticket, parts);
    return hipGetLastError();
}
size_t spx_reg_workspace(const spx_reg& r) { return 64 + (size_t)(spx_reg_group_wgs(r) + spx_reg_l1_wgs(r)) * 4 * sizeof(double); }

hipError_t spx_launch_reg_bwd(const spx_reg& r, const float* g_total, const float* g_terms, float* d_wd, float* d_head,
                              hipStream_t s) {
    const long long n_wd = (r.terms & (SPX_REG_ENT | SPX_REG_CEG | SPX_REG_SMAX)) ? (long long)r.U * r.P : 0;
    const long long n_head = (r.terms & SPX_REG_L1) ? (long long)r.K * r.Uh : 0;
    const long long n = n_wd + n_head;
    hipLaunchKernelGGL(spx_reg_bwd_kernel, dim3((unsigned)((n + SPX_REG_THREADS - 1) / SPX_REG_THREADS)), dim3(SPX_REG_THREADS), 0, s,
                       r, n_wd, n_head, g_total, g_terms, d_wd, d_head);
    return hipGetLastError();
}
