// The lane layout and the segmented scans of the multi-categorical and
// Bernoulli heads of recurrent PPO (recurrent_policy.hip, recurrent_heads.hip).
//
// A 16-row tile of up to 32 logits is spread over all 8 waves of the
// workgroup: 32 lanes per row, two rows per wave, flat logit j in lane j of its
// row.  A component of a multi-categorical head is then a contiguous run of
// lanes, and everything per component (max, sum exp, sum p log p, the Gumbel
// arg-max) is a segmented inclusive scan over the 32 lanes: five steps, d = 1,
// 2, 4, 8, 16, in which a lane combines with lane j - d iff that lane is still
// inside its segment, then one read of the segment's last lane for the total.
// The cost does not depend on the number of components and the order of every
// combination is fixed by (j, d) alone: equal bits on every run.
//
// The kernels get the head as one word, `starts`: bit j is set iff flat logit
// j is the first of its component.  With b = starts & ((2 << j) - 1):
//   component of j   popcount(b) - 1
//   segment's first  the highest set bit of b
//   segment's last   the next set bit above j, less one (A - 1 for the last)
// Lanes at and past A are made segments of their own, so no scan mixes them in.
#pragma once

#include "../../include/agx_multi.h"
#include "agx_common.h"

namespace agx {

// the `starts` word of a checked head (multi_head_check.h's head_width)
inline uint32_t multi_starts(const agx_multi_head &h) {
    uint32_t s = 0;
    int off = 0;
    for (int k = 0; k < h.K; ++k) {
        s |= 1u << off;
        off += h.nvec[k];
    }
    return s;
}

struct SegLane {
    int rl;           // the lane's row of the 16-row tile
    int j;            // its flat logit index, 0 .. 31
    int half;         // the wave lane of its row's logit 0: 0 or 32
    int first, last;  // the flat indices its segment spans
    int k;            // its component (j < A)
    bool on;          // j < A
};

__device__ __forceinline__ SegLane seg_lane(unsigned starts, int A) {
    const int lane = threadIdx.x & 63;
    SegLane s;
    s.rl = 2 * (threadIdx.x >> 6) + (lane >> 5);
    s.j = lane & 31;
    s.half = lane & 32;
    s.on = s.j < A;
    const unsigned st = A < 32 ? starts | (~0u << A) : starts;
    const unsigned below = st & ((2u << s.j) - 1u);  // bit 0 is set: never 0
    const unsigned above = (st >> s.j) >> 1;
    s.first = 31 - __clz((int)below);
    s.last = above ? s.j + __ffs((int)above) - 1 : 31;
    s.k = __popc(below) - 1;
    return s;
}

// the lanes of a Bernoulli head: every bit its own segment
__device__ __forceinline__ SegLane bit_lane(int A) { return seg_lane(~0u, A); }

__device__ __forceinline__ int bperm_i(int lane, int v) { return __builtin_amdgcn_ds_bpermute(lane << 2, v); }

// inclusive scans within the segment; the last lane of a segment ends with its total
__device__ __forceinline__ float seg_scan_sum(const SegLane &s, float v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const float o = bperm((lane - d) & 63, v);
        if (s.j - d >= s.first) v += o;
    }
    return v;
}
__device__ __forceinline__ float seg_scan_max(const SegLane &s, float v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const float o = bperm((lane - d) & 63, v);
        if (s.j - d >= s.first) v = fmaxf(v, o);
    }
    return v;
}
// (score, index) -> the segment's first maximum so far: lane j - d stands for lower indices, so it wins ties
__device__ __forceinline__ void seg_scan_argmax(const SegLane &s, float &sc, int &ix) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 32; d <<= 1) {
        const float os = bperm((lane - d) & 63, sc);
        const int oi = bperm_i((lane - d) & 63, ix);
        if (s.j - d >= s.first && os >= sc) {
            sc = os;
            ix = oi;
        }
    }
}
// a scan's value at the segment's last lane, in every lane of the segment
__device__ __forceinline__ float seg_total(const SegLane &s, float v) { return bperm(s.half + s.last, v); }

// the sum over the 32 lanes of a row, in every lane of it: the 16-lane DPP tree, then the two halves
__device__ __forceinline__ float row32_sum(float v) {
    v = row_sum(v);
    return v + bperm((threadIdx.x & 63) ^ 16, v);
}

}  // namespace agx
