// The LSTM gate chains shared by the sequence kernels (lstm.hip), their split
// per-step form (lstm_split.hip) and the fused recurrent policy step
// (recurrent_policy.hip): the MFMA macro, the sigmoid, the staging of a step's
// input tile, the four gates' accumulation over an LDS row and a weight row,
// and the backward's single-accumulator chain down a weight column.  All files
// accumulate every gate as bias, then k ascending over the input, then k
// ascending over h with these functions, so a step taken by any has the
// others' bits.
#pragma once

#include <cstdint>

#include "agx_common.h"
#include "../../include/agx_lstm.h"

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

// A wave-uniform value the optimiser cannot see through: addresses formed from it are computed where they are used
// instead of being carried through the step loop as one induction pointer per store (which spilled).
__device__ __forceinline__ int64_t opaque(int64_t v) {
    asm volatile("" : "+s"(v));
    return v;
}

__device__ __forceinline__ int opaque_lane(int v) {  // the same for a per-lane value
    asm volatile("" : "+v"(v));
    return v;
}

// acc[row][col] += sum_k arow[k] * wcol[k * ldw], k < K (K % 16 == 0): W read down a column, four steps' operands
// ahead of their MFMAs.
__device__ __forceinline__ f32x4 chain_col(int K, int q, f32x4 acc, const float *arow, const float *wcol, int ldw) {
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 64) {
        f32x4 a[4];
        float w[16];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kc + 16 * s + 4 * q, kk = min(k, K - 4);
            a[s] = *reinterpret_cast<const f32x4 *>(arow + kk);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = wcol[(int64_t)(kk + j) * ldw];
                w[4 * s + j] = k < K ? v : 0.f;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (kc + 16 * s < K) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = MFMA(a[s][j], w[4 * s + j], acc);
            }
    }
    return acc;
}

// `saved`, per layer l at l * 6 * N * H floats: gates [N][4H], c [N][H], h [N][H] (below the top layer)
__host__ __device__ inline int64_t saved_layer(int64_t N, int H, int l) { return (int64_t)l * 6 * N * H; }

// lstm.hip's host side, shared with lstm_split.hip: the descriptor checks (no HIP call) and the two launches of a
// layer's backward that run over all N rows (dw_kernel, then dx_kernel when dX is wanted).
int check_dims(const agx_lstm_desc *d, int64_t B, int64_t T, const char *who);
int check_desc(const agx_lstm_desc *d, int64_t B, int64_t T, bool backward, const char *who);
int launch_dw_dx(const agx_lstm_layer &p, const float *dG, const float *xin, const float *hout, const float *h0, float *dX,
                 int K, int H, int64_t T, int64_t N, hipStream_t s, const char *who);

}  // namespace lstm

}  // namespace agx
