// The dense layers and row passes shared by the fused recurrent policy step
// (recurrent_policy.hip) and the BPTT learner's head kernels
// (recurrent_heads.hip): a 16-row LDS tile through y = x W^T + b on
// v_mfma_f32_16x16x4_f32, and LayerNorm / activation over the tile's rows.
// Both files run 8-wave workgroups and accumulate every output as bias, then k
// ascending, so a row has the same bits in either and whatever its place in
// its tile.
#pragma once

#include "../../include/agx_recurrent.h"

#include "agx_common.h"
#include "lstm_gates.h"

namespace agx {

using lstm::f32x4;

constexpr int kRT = 512;  // threads
constexpr int kRW = 8;    // waves

// acc[row][unit] += sum_k arow[k] * wrow[k], k < K ascending.  arow: this lane's row of an LDS tile zero-padded
// to K16 = the 16-rounded K; wrow: this lane's unit row of W [out][K].  VEC: 16-byte weight loads (K % 4 == 0,
// W 16-byte aligned), else 4-byte loads; the same k order and bits either way.
template <bool VEC>
__device__ __forceinline__ f32x4 chain_row(int K, int q, f32x4 acc, const float *arow, const float *wrow) {
    const int K16 = (K + 15) & ~15;
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 64) {
        f32x4 a[4], w[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kc + 16 * s + 4 * q;
            a[s] = *reinterpret_cast<const f32x4 *>(arow + min(k, K16 - 4));
            if (VEC) {
                w[s] = *reinterpret_cast<const f32x4 *>(wrow + min(k, K - 4));
                if (k >= K) w[s] = f32x4{0.f, 0.f, 0.f, 0.f};
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = wrow[min(k + j, K - 1)];
                    w[s][j] = k + j < K ? v : 0.f;
                }
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (kc + 16 * s < K) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = MFMA(a[s][j], w[s][j], acc);
            }
    }
    return acc;
}

// One 16 x 16 output tile of y = x W^T + b, this wave's: the bias, then k ascending
__device__ __forceinline__ void dense_tile(int tile, const float *X, int ldx, int K, const float *W, const float *b,
                                           int F, float *Y, int ldy) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const bool vec = (K & 3) == 0 && lstm::aligned16(W);
    const int unit = tile * 16 + r, uu = min(unit, F - 1);
    const float bv = b[uu];
    f32x4 acc = {bv, bv, bv, bv};
    const float *wrow = W + (int64_t)uu * K;
    acc = vec ? chain_row<true>(K, q, acc, X + r * ldx, wrow) : chain_row<false>(K, q, acc, X + r * ldx, wrow);
#pragma unroll
    for (int i = 0; i < 4; ++i) Y[(4 * q + i) * ldy + unit] = unit < F ? acc[i] : 0.f;
}

// Y [16][ldy] = X [16][ldx] W^T + b over the 16-rounded width of F, zeros in the columns past F
__device__ __forceinline__ void dense(const float *X, int ldx, int K, const float *W, const float *b, int F, float *Y,
                                      int ldy) {
    const int wave = threadIdx.x >> 6;
    for (int tile = wave; tile < ((F + 15) >> 4); tile += kRW) dense_tile(tile, X, ldx, K, W, b, F, Y, ldy);
}

// One side of a pair of dense layers that advance together (the two heads over a shared latent): where its input
// and output tiles lie; `on`: the side still has a layer at this depth.
struct DenseSide {
    const float *X;
    float *Y;
    int ldx, ldy;
    bool on;

    // the next layer reads what the last one wrote and writes `to`
    __device__ __forceinline__ void advance(float *to, int out) {
        X = Y;
        ldx = ldy;
        Y = to;
        ldy = ((out + 15) & ~15) + 4;
    }
};

// `dense` of both sides' layers la and lc as one tile list, side a's tiles first: the 8 waves share the list, so a
// depth of the pair costs the barriers of one layer.  A tile is still one wave's chain, with the bits `dense`
// gives it.
__device__ __forceinline__ void dense_pair(const agx_recurrent_linear &la, const DenseSide &a,
                                           const agx_recurrent_linear &lc, const DenseSide &c) {
    const int wave = threadIdx.x >> 6;
    const int ta = a.on ? (la.out + 15) >> 4 : 0, tc = c.on ? (lc.out + 15) >> 4 : 0;
    for (int tile = wave; tile < ta + tc; tile += kRW) {
        if (tile < ta)
            dense_tile(tile, a.X, a.ldx, la.in, la.w, la.b, la.out, a.Y, a.ldy);
        else
            dense_tile(tile - ta, c.X, c.ldx, lc.in, lc.w, lc.b, lc.out, c.Y, c.ldy);
    }
}

// the row passes of both sides' layers at once: side a on waves 0 .. 3, side c on waves 4 .. 7
__device__ __forceinline__ void row_pass_pair(const agx_recurrent_linear &la, const DenseSide &a,
                                              const agx_recurrent_linear &lc, const DenseSide &c);

// LayerNorm (affine lnw / lnb, eps 1e-5; null: none) and the activation over the F columns of every row of
// Y [16][ld] in place: waves 0 .. 3, 16 lanes per row.  The loops run to the 16-rounded width, so the row
// reductions see whole DPP rows.  w0 = 4 puts the pass on waves 4 .. 7, beside another tile's pass on waves 0 .. 3.
__device__ __forceinline__ void row_pass(float *Y, int ld, int F, const float *lnw, const float *lnb, int act,
                                         int w0 = 0) {
    const int wave = (int)(threadIdx.x >> 6) - w0, lane = threadIdx.x & 63;
    if (wave < 0 || wave >= 4 || (!lnw && act == AGX_RECURRENT_ACT_NONE)) return;
    const int sub = lane & 15, F16 = (F + 15) & ~15;
    float *y = Y + (4 * wave + (lane >> 4)) * ld;
    float mean = 0.f, rstd = 1.f;
    if (lnw) {
        float s = 0.f;
        for (int j = sub; j < F16; j += 16) s = j < F ? s + y[j] : s;
        mean = row_sum(s) * (1.f / (float)F);
        float vs = 0.f;
        for (int j = sub; j < F16; j += 16) {
            const float d = y[j] - mean;
            vs = j < F ? vs + d * d : vs;
        }
        rstd = 1.f / sqrtf(row_sum(vs) / (float)F + 1e-5f);
    }
    for (int j = sub; j < F; j += 16) {
        float x = y[j];
        if (lnw) x = (x - mean) * rstd * lnw[j] + lnb[j];
        if (act == AGX_RECURRENT_ACT_RELU) x = relu(x);
        if (act == AGX_RECURRENT_ACT_TANH) x = tanhf(x);
        y[j] = x;
    }
}

__device__ __forceinline__ void row_pass_pair(const agx_recurrent_linear &la, const DenseSide &a,
                                              const agx_recurrent_linear &lc, const DenseSide &c) {
    if (a.on) row_pass(a.Y, a.ldy, la.out, la.ln_w, la.ln_b, la.relu ? AGX_RECURRENT_ACT_RELU : AGX_RECURRENT_ACT_NONE);
    if (c.on)
        row_pass(c.Y, c.ldy, lc.out, lc.ln_w, lc.ln_b, lc.relu ? AGX_RECURRENT_ACT_RELU : AGX_RECURRENT_ACT_NONE, 4);
}

}  // namespace agx
