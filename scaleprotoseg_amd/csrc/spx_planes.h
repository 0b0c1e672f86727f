// What every full-resolution map operator (spx_eval.hip, spx_overlap.hip, spx_pushbox.hip, spx_explain.hip) reads its inputs
// through: the strided view of a 4-D fp32 tensor and the label read.  How a pixel is interpolated from the planes is not here:
// the bilinear rule lives in spx_eval.hip, the cubic one in spx_overlap_sample.h.
#ifndef SPX_PLANES_H
#define SPX_PLANES_H
#include "spx_common.h"

struct SpxPlanes {                // element strides of a 4-D fp32 tensor, in (n, channel, y, x) order
    const float* p;
    long long sn, sc, sy, sx;
};

static inline SpxPlanes spx_planes(const float* p, const long long* st) {    // a NULL tensor (no strides either) has zero strides
    SpxPlanes m;
    m.p = p;
    m.sn = p ? st[0] : 0;
    m.sc = p ? st[1] : 0;
    m.sy = p ? st[2] : 0;
    m.sx = p ? st[3] : 0;
    return m;
}

// label_bytes: 1 = uint8, 4 = int32, 8 = int64 (the entry points refuse anything else)
__device__ __forceinline__ long long spx_label(const void* labels, int label_bytes, size_t o) {
    if (label_bytes == 1) return (long long)((const uint8_t*)labels)[o];
    if (label_bytes == 4) return (long long)((const int32_t*)labels)[o];
    return ((const long long*)labels)[o];
}

#endif  // SPX_PLANES_H
