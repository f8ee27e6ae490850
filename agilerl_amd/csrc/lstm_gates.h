// The LSTM gate chains shared by the sequence kernels (lstm.hip) and the fused
// recurrent policy step (recurrent_policy.hip): the MFMA macro, the sigmoid,
// the staging of a step's input tile and the four gates' accumulation over an
// LDS row and a weight row.  Both files accumulate every gate as bias, then k
// ascending over the input, then k ascending over h with these functions, so a
// step taken by either has the other's bits.
#pragma once

#include <cstdint>

#include "agx_common.h"

namespace agx {

namespace lstm {

typedef float f32x4 __attribute__((ext_vector_type(4)));

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

__device__ __forceinline__ bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// Rows b0 .. b0 + 15 of step t of src [B][T][K] into xs [16][ld], zeros for rows past B and columns K .. K16 - 1.
__device__ __forceinline__ void stage_step(float *xs, int ld, const float *src, int B, int64_t T, int64_t t, int K,
                                           int K16, int b0) {
    const int r = threadIdx.x >> 5, c = threadIdx.x & 31;
    const int row = b0 + r;
    const float *p = src + ((int64_t)min(row, B - 1) * T + t) * K;
#pragma unroll 2
    for (int k = c; k < K16; k += 32) xs[r * ld + k] = (row < B && k < K) ? p[k] : 0.f;
}

// The four gates' chains over k < K in ascending 16-deep steps: acc[g][row][unit] += sum_k arow[k] * wrow[g * gs + k].
// arow: this lane's row of an LDS tile, zero-padded to a multiple of 16; wrow: this lane's unit row of gate 0.
// CH steps' operands are requested before their MFMAs (CH * 5 16-byte loads in flight).  K % 4 == 0, rows aligned.
template <int CH>
__device__ __forceinline__ void gates_vec(int K, int q, f32x4 (&acc)[4], const float *arow, const float *wrow,
                                          int64_t gs) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 16 * CH) {
        f32x4 a[CH], w[4][CH];
#pragma unroll
        for (int s = 0; s < CH; ++s) {
            const int k = kc + 16 * s + 4 * q, kk = min(k, K - 4);
            a[s] = *reinterpret_cast<const f32x4 *>(arow + kk);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                w[g][s] = *reinterpret_cast<const f32x4 *>(wrow + g * gs + kk);
                if (k >= K) w[g][s] = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
#pragma unroll
        for (int s = 0; s < CH; ++s)
            if (kc + 16 * s < K) {
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = MFMA(a[s][j], w[g][s][j], acc[g]);
            }
    }
}

// The same chains (same k order, same bits) with 4-byte weight loads: any K, any alignment.
__device__ __forceinline__ void gates_any(int K, int q, f32x4 (&acc)[4], const float *arow, const float *wrow,
                                          int64_t gs) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 16) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(arow + kc + 4 * q);
        float w[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = kc + 4 * q + j, kk = min(k, K - 1);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float v = wrow[g * gs + kk];
                w[g][j] = k < K ? v : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) acc[g] = MFMA(a[j], w[g][j], acc[g]);
    }
}

}  // namespace lstm

}  // namespace agx
