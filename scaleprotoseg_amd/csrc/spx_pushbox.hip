// Push bounding boxes (segmentation/push_multiscale_optimization.py:416-497, helpers.py:53-87): for every pushed prototype
// the box of its latent patch in image pixels and the rectangle of the highly activated region around it, found by the
// reference's greedy enlargement.  The reference resizes the activation plane to the image, masks it with the prototype's class
// and walks NumPy rows on the host; here the walk runs on values recomputed from the latent plane with ovl_value() (the
// function the thresholds were selected with: a pixel has the same bits in both), and the [H, W] map is never written.
//
//   row r = (n, c, class k, flat latent index f);  T = thresholds[n, c] (spx_push_boxes) or thresholds[r] (spx_push_boxes_rows:
//           a threshold of the row's own, such as the class-restricted one of spx_masked_select.hip; k = -1 then masks on label 0,
//           what the reference does for a patch whose majority label is void, and T = +inf hits nowhere)
//   rf    = [int(i ph), int(i ph + ph) + 1, int(j pw), int(j pw + pw) + 1] with ph = H / h, pw = W / w, i = f / w, j = f % w,
//           in double as Python computes it (the ends may exceed H, W and are stored as they are)
//   hit(Y, X) = labels[n, Y, X] == k + 1 ? u[n, c, Y, X] >= T : 0 >= T
//   walk  from (sh, eh, sw, ew) = rf with four sticky `stopped` flags, until all are set; one pass is, in this order and each
//         step on the box as the step before left it:
//           up     not stopped, sh > 0     and a hit in row sh - 1, columns sw .. min(ew, W - 1):  sh -= 1, else stopped
//           down   not stopped, eh < H - 1 and a hit in row eh + 1, the same columns:              eh += 1, else stopped
//           left   not stopped, sw > 0     and a hit in column sw - 1, rows sh .. min(eh, H - 1):  sw -= 1, else stopped
//           right  not stopped, ew < W - 1 and a hit in column ew + 1, the same rows:              ew += 1, else stopped
//   crop  = (max(sh - m, 0), min(eh + m, H - 1) + 1, max(sw - m, 0), min(ew + m, W - 1) + 1), m = add_margin
//
// One workgroup per row.  The box and the flags are computed by every thread from the same values (workgroup-uniform), a step
// whose scalar conditions fail costs nothing, and the others are one block-wide "any" over a segment of at most max(H, W) samples:
// lanes stride over the segment, one ballot per wave, one LDS word across the waves, one barrier.
#include "spx_overlap_sample.h"

#define PBX_THREADS 256

struct PbxRow {                   // what the "any" queries of one row share
    const float* plane;           // a.p + n * sn + c * sc
    const void* labels;
    size_t label0;                // n * H * W
    long long want;               // k + 1
    float T;
    int label_bytes, h, w, H, W, sy, sx;
    bool outside_hits;            // 0 >= T: every pixel outside the class is a hit
};

__device__ __forceinline__ bool pbx_hit(const PbxRow& r, int Y, int X) {
    if (spx_label(r.labels, r.label_bytes, r.label0 + (size_t)Y * r.W + X) != r.want) return r.outside_hits;
    int ox[4], oy[4];
    float wx[4], wy[4];
    ovl_axis(Y, r.h, r.H, 0, r.sy, oy, wy);
    ovl_axis(X, r.w, r.W, 0, r.sx, ox, wx);
    return ovl_value(r.plane, oy, wy, ox, wx) >= r.T;
}

// Block-wide any over the pixels (Y0 + t * dY, X0 + t * dX), t = 0 .. count - 1 (count >= 1, all inside the image).  Query q
// answers through word q % 3 of s_any and clears word (q + 1) % 3 for the next query: a thread still reading the answer of q
// is at most one barrier behind the others, and word q % 3 is written again only by query q + 2, two barriers later.
__device__ __forceinline__ bool pbx_any(const PbxRow& r, int Y0, int X0, int dY, int dX, int count, int* s_any, int& q) {
    const int tid = threadIdx.x;
    bool mine = false;
    for (int t = tid; t < count && !mine; t += PBX_THREADS) mine = pbx_hit(r, Y0 + t * dY, X0 + t * dX);
    const int slot = q % 3;
    if (tid == 0) s_any[(q + 1) % 3] = 0;
    if (__ballot(mine) != 0ull && (tid & 63) == 0) s_any[slot] = 1;
    __syncthreads();
    ++q;
    return s_any[slot] != 0;
}

__global__ __launch_bounds__(PBX_THREADS) void spx_push_boxes_kernel(SpxPlanes a, const void* __restrict__ labels, int label_bytes,
                                                                     const int32_t* __restrict__ rows, const float* __restrict__ thresholds,
                                                                     int per_row, int N, int C, int h, int w, int H, int W, int add_margin,
                                                                     int32_t* __restrict__ rf_boxes, int32_t* __restrict__ crops) {
    __shared__ int s_any[3];
    const int tid = threadIdx.x;
    const size_t row = blockIdx.x;
    const int n = rows[row * 4 + 0], c = rows[row * 4 + 1], k = rows[row * 4 + 2], f = rows[row * 4 + 3];
    if (n < 0 || n >= N || c < 0 || c >= C || f < 0 || f >= h * w) {      // workgroup-uniform; the host entry point refuses
        if (tid < 4) {                                                    // such a row when it is given the table's host copy
            rf_boxes[row * 4 + tid] = -1;
            crops[row * 4 + tid] = -1;
        }
        return;
    }
    const double ph = (double)H / (double)h, pw = (double)W / (double)w;
    const int pi = f / w, pj = f - pi * w;
    int sh = (int)((double)pi * ph), eh = (int)((double)pi * ph + ph) + 1;
    int sw = (int)((double)pj * pw), ew = (int)((double)pj * pw + pw) + 1;
    if (tid == 0) {
        rf_boxes[row * 4 + 0] = sh;
        rf_boxes[row * 4 + 1] = eh;
        rf_boxes[row * 4 + 2] = sw;
        rf_boxes[row * 4 + 3] = ew;
        s_any[0] = 0;
    }
    PbxRow r;
    r.plane = a.p + (long long)n * a.sn + (long long)c * a.sc;
    r.labels = labels;
    r.label0 = (size_t)n * H * W;
    r.want = (long long)k + 1;
    r.T = thresholds[per_row ? row : (size_t)n * C + c];
    r.label_bytes = label_bytes;
    r.h = h;
    r.w = w;
    r.H = H;
    r.W = W;
    r.sy = (int)a.sy;
    r.sx = (int)a.sx;
    r.outside_hits = 0.0f >= r.T;
    __syncthreads();
    int q = 0;
    bool stop_up = false, stop_down = false, stop_left = false, stop_right = false;
    // a pass that grows nothing sets all four flags, and the box can grow at most (H - 1) + (W - 1) times: at most H + W passes
    for (int pass = 0; pass < H + W && !(stop_up && stop_down && stop_left && stop_right); ++pass) {
        if (!stop_up && sh > 0 && pbx_any(r, sh - 1, sw, 0, 1, min(ew, W - 1) - sw + 1, s_any, q)) --sh;
        else stop_up = true;
        if (!stop_down && eh < H - 1 && pbx_any(r, eh + 1, sw, 0, 1, min(ew, W - 1) - sw + 1, s_any, q)) ++eh;
        else stop_down = true;
        if (!stop_left && sw > 0 && pbx_any(r, sh, sw - 1, 1, 0, min(eh, H - 1) - sh + 1, s_any, q)) --sw;
        else stop_left = true;
        if (!stop_right && ew < W - 1 && pbx_any(r, sh, ew + 1, 1, 0, min(eh, H - 1) - sh + 1, s_any, q)) ++ew;
        else stop_right = true;
    }
    if (tid == 0) {
        crops[row * 4 + 0] = max(sh - add_margin, 0);
        crops[row * 4 + 1] = min(eh + add_margin, H - 1) + 1;
        crops[row * 4 + 2] = max(sw - add_margin, 0);
        crops[row * 4 + 3] = min(ew + add_margin, W - 1) + 1;
    }
}

hipError_t spx_launch_push_boxes(const float* planes, const long long* st, const void* labels, int label_bytes, const int32_t* rows,
                                 const float* thresholds, int per_row, int R, int N, int C, int h, int w, int H, int W, int add_margin,
                                 int32_t* rf_boxes, int32_t* crops, hipStream_t s) {
    hipLaunchKernelGGL(spx_push_boxes_kernel, dim3((unsigned)R), dim3(PBX_THREADS), 0, s, spx_planes(planes, st), labels, label_bytes,
                       rows, thresholds, per_row, N, C, h, w, H, W, add_margin, rf_boxes, crops);
    return hipGetLastError();
}
