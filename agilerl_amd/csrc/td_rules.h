// What the TD-target kernels (td_targets.hip) and the conservative Q-learning
// loss (cqn.hip) share: torch's NaN rules for min / max / argmax, the row's
// next-state value q_t, the target y, and the fixed-order f64 block sums that
// every mean here is built from.  One definition, so the two kernels' y agree
// bit for bit.
#pragma once

#include "agx_common.h"

namespace agx {

constexpr int kTdBlock = 256;

// The tail of every kernel here: s1 (and s2) summed over the block in f64, an
// xor butterfly per wave, then the waves in ascending order by thread 0.
// True in thread 0, whose s1 / s2 then hold the sums.
template <int THREADS, bool TWO>
__device__ __forceinline__ bool block_sum(double &s1, double &s2) {
    __shared__ double red[TWO ? 2 : 1][THREADS / kWave];
    s1 = wave_sum(s1);
    if (TWO) s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x / 64] = s1;
        if (TWO) red[1][threadIdx.x / 64] = s2;
    }
    __syncthreads();
    if (threadIdx.x != 0) return false;
    s1 = s2 = 0.0;
    for (int w = 0; w < THREADS / kWave; ++w) {
        s1 += red[0][w];
        if (TWO) s2 += red[1][w];
    }
    return true;
}

// The same for three sums: one more pass through block_sum.  The two passes
// are different instantiations (<THREADS, true>, <THREADS, false>), each with
// a red[] array of its own, so thread 0 may still be reading the first pass's
// array while the other threads write the second's.  A kernel that went
// through the SAME instantiation twice would need a __syncthreads() between
// the passes: the second pass's writes would race thread 0's reads of red[].
template <int THREADS>
__device__ __forceinline__ bool block_sum3(double &s1, double &s2, double &s3) {
    double unused = 0.0;
    const bool first = block_sum<THREADS, true>(s1, s2);
    block_sum<THREADS, false>(s3, unused);
    return first;
}

// torch.min / torch.max (and clamp) propagate NaN; fminf / fmaxf do not
__device__ __forceinline__ float nan_min(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return fminf(a, b);
}
__device__ __forceinline__ float nan_max(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return fmaxf(a, b);
}

// torch.argmax walking a row in index order: v replaces the best value bv when
// it is larger, or the row's first NaN (ties and later NaNs keep the earlier index)
__device__ __forceinline__ bool argmax_takes(float v, float bv) { return v > bv || (v != v && bv == bv); }

// q_t of one row, walked by one lane: max_a tn[a], or tn[argmax_a on[a]]
// (double).  A NaN among the values is the maximum, as for torch.max /
// torch.argmax (argmax: the first NaN's index)
__device__ __forceinline__ float row_q_next(const float *__restrict__ on, const float *__restrict__ tn, int A,
                                            int dbl) {
    if (dbl) {
        int best = 0;
        float bv = on[0];
        for (int a = 1; a < A; ++a) {
            const float v = on[a];
            if (argmax_takes(v, bv)) {
                bv = v;
                best = a;
            }
        }
        return tn[best];
    }
    float qt = tn[0];
    for (int a = 1; a < A; ++a) qt = nan_max(qt, tn[a]);
    return qt;
}

// y = r + (gamma * q_t) * (1 - d), one f32 rounding per op
__device__ __forceinline__ float td_y(float r, float g, float qt, float d) { return r + (g * qt) * (1.0f - d); }

}  // namespace agx
