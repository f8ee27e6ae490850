// SimBa encoders (include/agx_simba.h): input Linear, residual blocks
// x + W2 relu(W1 LN(x) + b1) + b2, output LayerNorm -> Linear -> activation;
// blocks + 2 launches forward, blocks + 2 backward, fp32 MFMA throughout.
//
// Every workgroup is 8 waves and works on 16-row tiles.  A tile of rows is
// staged once into LDS (stage_rows: 32 lanes per row, the LayerNorm's mean
// and rstd by two passes over the row in registers, y = xhat * gamma + beta
// rounded op by op), and every GEMM takes its A operand from LDS and its B
// operand straight from the weight matrix in L2.
//
// Block forward (block_fwd_kernel, one workgroup per row tile): the inner
// dimension I = scale * H is walked in chunks of 128 units.  Per chunk each
// wave computes 16 units of u = relu(xn W1^T + b1) as one MFMA chain over H
// (tile_xWt) into LDS, then all waves accumulate y += u W2[:, chunk]^T into
// the H / 16 output tiles they hold across the walk (tiles wave, wave + 8,
// ...: at most four, 16 VGPRs).  u never reaches memory.
//
// Block backward (block_bwd_kernel, three roles in one launch):
//   role W, one workgroup per 32 inner units, loops over the row tiles:
//     recomputes u for its units with the forward's routine (same chain, same
//     bits, so the same ReLU mask), forms du = (dy W2[:, units]) * [u > 0] and
//     accumulates dW1 = du^T xn, dW2 = dy^T u (MFMA over the 16 batch rows of
//     a tile) and db1 in registers; every element is written once.
//   role X, one workgroup per row tile: walks the chunks as the forward does,
//     accumulating dxn = du W1; then the LayerNorm backward (both row sums in
//     one pass), + dy of the residual, and this tile's column sums of the
//     LayerNorm affine gradients as a partial row.
//   role S, one workgroup: db2 = column sums of dy, and the LayerNorm affine
//     gradients of the layer *after* this block from the partial rows the
//     previous launch wrote, in tile order.
// Input layer and tail (lin_fwd_kernel / lin_bwd_kernel) use the same
// routines with flags for the LayerNorm and the ReLU.
#include <cstdint>

#include "agx_common.h"
#include "../../include/agx_simba.h"

namespace agx {

namespace simba {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 512;
constexpr int kWaves = 8;
constexpr int kChunk = 16 * kWaves;  // inner units per step of the forward / role X walk
constexpr int kLdu = kChunk + 4;
constexpr int kUnitsW = 32;          // inner units of a role-W workgroup
constexpr int kLdw = kUnitsW + 4;
constexpr int kLdz = 20;

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

// Rows b0 .. b0 + 15 of src [B][K] into xs [16][ld] (rows past B: zeros, with or without LayerNorm).
// With g: LayerNorm rows, y = ((x - mean) * rstd) * g + bt, each op rounded;
// mean / rstd from st_in [B][2] when given (the backward: the forward's
// values, so y has the forward's bits), else computed (and stored to st_out
// when given).  st [32]: the rows' mean, then rstd.  Ends with a barrier.
__device__ __forceinline__ void stage_rows(float *xs, int ld, const float *src, int B, int K, int b0, const float *g,
                                           const float *bt, float eps, float *st, float *st_out, const float *st_in) {
    const int r = threadIdx.x >> 5, c = threadIdx.x & 31;
    const int row = b0 + r;
    const bool ok = row < B;
    const float *p = src + (int64_t)(ok ? row : 0) * K;
    float s = 0.f;
    for (int k = c; k < K; k += 32) {
        const float v = ok ? p[k] : 0.f;
        xs[r * ld + k] = v;
        s += v;
    }
    if (g) {
        float mean, rs;
        if (st_in) {
            mean = st_in[2 * (ok ? row : 0)];
            rs = st_in[2 * (ok ? row : 0) + 1];
        } else {
            mean = group_sum<32>(s) / (float)K;
            float q = 0.f;
            for (int k = c; k < K; k += 32) {
                const float d = xs[r * ld + k] - mean;
                q += d * d;
            }
            rs = __frsqrt_rn(group_sum<32>(q) / (float)K + eps);
            if (st_out && ok && c == 0) {
                st_out[2 * row] = mean;
                st_out[2 * row + 1] = rs;
            }
        }
        for (int k = c; k < K; k += 32)
            xs[r * ld + k] =
                ok ? __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(xs[r * ld + k], mean), rs), g[k]), bt[k]) : 0.f;
        if (c == 0) {
            st[r] = mean;
            st[16 + r] = rs;
        }
    }
    __syncthreads();
}

// One wave's MFMA chain over k < K in ascending 16-deep steps: acc[row][col] += sum_k a_at(k) * w_at(k), this
// lane's operands (row = lane & 15 for a, col = lane & 15 for w).  Four steps' operands (16 loads of each) are
// requested before their MFMAs, so a chain pays one memory round trip per 64 k instead of one per 16.
template <typename FA, typename FW>
__device__ __forceinline__ f32x4 chain(int K, int q, f32x4 acc, FA a_at, FW w_at) {
    for (int kc = 0; kc < K; kc += 64) {
        float a[16], w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int k = kc + 16 * (u >> 2) + 4 * q + (u & 3), kk = min(k, K - 1);
            a[u] = k < K ? a_at(kk) : 0.f;
            w[u] = k < K ? w_at(kk) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (kc + 16 * (u >> 2) < K) acc = MFMA(a[u], w[u], acc);
    }
    return acc;
}

// The same chain (same k order, so the same bits) with each lane's four consecutive k of a step as one
// 16-byte load: K % 4 == 0 and both rows 16-byte aligned.
__device__ __forceinline__ f32x4 chain4(int K, int q, f32x4 acc, const float *arow, const float *wrow) {
    for (int kc = 0; kc < K; kc += 64) {
        f32x4 a[4], w[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kc + 16 * s + 4 * q, kk = min(k, K - 4);
            a[s] = *reinterpret_cast<const f32x4 *>(arow + kk);
            w[s] = *reinterpret_cast<const f32x4 *>(wrow + kk);
            if (k >= K) a[s] = w[s] = f32x4{0.f, 0.f, 0.f, 0.f};
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

__device__ __forceinline__ bool rows16(const float *a, int lda, const float *w, int ldw, int K) {
    return (((K | lda | ldw) & 3) == 0) && (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(w)) & 15) == 0);
}

// acc += sum_k arow[k] * wrow[k], k < K, both rows contiguous in k
__device__ __forceinline__ f32x4 chain_rows(int K, int q, f32x4 acc, const float *arow, int lda, const float *wrow,
                                            int ldw) {
    if (rows16(arow, lda, wrow, ldw, K)) return chain4(K, q, acc, arow, wrow);
    return chain(K, q, acc, [&](int k) { return arow[k]; }, [&](int k) { return wrow[k]; });
}

// tile[row][col] = sum_k xs[row][k] * W[(n0 + col) * ldw + k], k < K.
// Columns past N repeat column N - 1 (the caller drops them).
__device__ __forceinline__ f32x4 tile_xWt(const float *xs, int ld, const float *W, int ldw, int n0, int N, int K,
                                          int lane) {
    const int r = lane & 15;
    return chain_rows(K, lane >> 4, f32x4{0.f, 0.f, 0.f, 0.f}, xs + r * ld, ld, W + (int64_t)min(n0 + r, N - 1) * ldw,
                      ldw);
}

// tile[row][col] = sum_k xs[row][k] * W[k * ldw + n0 + col], k < K (W read along its rows).
__device__ __forceinline__ f32x4 tile_xW(const float *xs, int ld, const float *W, int ldw, int n0, int N, int K,
                                         int lane) {
    const int r = lane & 15;
    const float *wcol = W + min(n0 + r, N - 1);
    const float *xrow = xs + r * ld;
    return chain(K, lane >> 4, f32x4{0.f, 0.f, 0.f, 0.f}, [&](int k) { return xrow[k]; },
                 [&](int k) { return wcol[(int64_t)k * ldw]; });
}

// LayerNorm backward of the 16 rows whose d/d(normalised row) sits in dn [16][ld]:
// dx = rstd * ((gx - s1 / H) - xhat * (s2 / H)) [+ res], gx = dn * g, s1 = sum gx, s2 = sum gx * xhat,
// xhat recomputed from x and the staged statistics.  Also the tile's column sums of dn * xhat and dn
// (the affine gradients' partial row) into pg / pb [H].  tmp [16][ldt] is scratch (may alias res).
__device__ __forceinline__ void ln_bwd_rows(float *dn, int ld, const float *res, int ldr, float *tmp, int ldt,
                                            const float *x, const float *st, const float *g, int B, int H, int b0,
                                            float *dx, float *pg, float *pb) {
    const int r = threadIdx.x >> 5, c = threadIdx.x & 31;
    const int row = b0 + r;
    const bool ok = row < B;
    const float *xp = x + (int64_t)(ok ? row : 0) * H;
    const float mean = st[r], rs = st[16 + r];
    float s1 = 0.f, s2 = 0.f;
    for (int k = c; k < H; k += 32) {
        const float xh = __fmul_rn(__fsub_rn(xp[k], mean), rs);
        const float gx = dn[r * ld + k] * g[k];
        s1 += gx;
        s2 += gx * xh;
    }
    s1 = group_sum<32>(s1) / (float)H;
    s2 = group_sum<32>(s2) / (float)H;
    for (int k = c; k < H; k += 32) {
        const float xh = __fmul_rn(__fsub_rn(xp[k], mean), rs);
        const float d = dn[r * ld + k];
        float v = rs * ((d * g[k] - s1) - xh * s2);
        if (res) v += res[r * ldr + k];
        if (ok) dx[(int64_t)row * H + k] = v;
        dn[r * ld + k] = ok ? d : 0.f;
        tmp[r * ldt + k] = ok ? d * xh : 0.f;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < H; k += kThreads) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            a += tmp[i * ldt + k];
            b += dn[i * ld + k];
        }
        pg[k] = a;
        pb[k] = b;
    }
}

// role S: column sums in a fixed order
__device__ __forceinline__ void column_sums(const float *src, int rows, int H, float *dst) {
    if (!src) return;
    for (int k = threadIdx.x; k < H; k += kThreads) {
        float a = 0.f;
#pragma unroll 8
        for (int b = 0; b < rows; ++b) a += src[(int64_t)b * H + k];
        dst[k] = a;
    }
}

// ---------------------------------------------------------------------------
struct LinArgs {
    const float *x;        // [B][K]
    const float *ln_g, *ln_b, *w, *b;
    float *out;            // forward: [B][N]
    float *stats;          // [B][2] (with ln_g): written by the forward, read by the backward
    const float *gsrc;     // backward: d/d out [B][N]
    const float *outv;     // backward, relu: the forward's out
    float *gw, *gb, *din;  // din [B][K] (null: none)
    float *pg, *pb;        // with ln_g and din: partial rows [row tiles][K]
    const float *sg, *sb;  // role S: the previous launch's partial rows [row tiles][N] -> g_g, g_b [N]
    float *g_g, *g_b;
    int B, K, N, relu, nW, nX;
    float eps;
};

__global__ __launch_bounds__(kThreads) void lin_fwd_kernel(LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int ld = a.K + 4;
    float *xs = lds, *st = lds + 16 * ld;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b0 = blockIdx.x * 16;
    stage_rows(xs, ld, a.x, a.B, a.K, b0, a.ln_g, a.ln_b, a.eps, st, blockIdx.y == 0 ? a.stats : nullptr, nullptr);
    const int n0 = blockIdx.y * kChunk + wave * 16;
    if (n0 >= a.N) return;
    const f32x4 p = tile_xWt(xs, ld, a.w, a.K, n0, a.N, a.K, lane);
    const int col = n0 + (lane & 15), q = lane >> 4;
    if (col >= a.N) return;
    const float bias = a.b[col];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = b0 + 4 * q + i;
        float v = p[i] + bias;
        if (a.relu) v = relu(v);
        if (row < a.B) a.out[(int64_t)row * a.N + col] = v;
    }
}

__device__ __forceinline__ float dz_at(const LinArgs &a, int row, int n) {
    const int64_t o = (int64_t)row * a.N + n;
    const float d = a.gsrc[o];
    return (a.relu && !(a.outv[o] > 0.f)) ? 0.f : d;
}

__global__ __launch_bounds__(kThreads) void lin_bwd_kernel(LinArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int B = a.B, K = a.K, N = a.N;
    const int ld = K + 4, TK = (K + 15) >> 4;
    const int nrt = (B + 15) >> 4;
    int blk = blockIdx.x;
    if (blk < a.nW) {  // role W: dW[n0 .. n0 + 15][:], db
        float *xs = lds, *st = xs + 16 * ld, *dzs = st + 32;
        const int n0 = blk * 16;
        f32x4 acc[4] = {};
        float sb = 0.f;
        for (int rt = 0; rt < nrt; ++rt) {
            const int b0 = rt * 16;
            if (threadIdx.x < 256) {
                const int rr = threadIdx.x >> 4, cc = threadIdx.x & 15;
                dzs[rr * kLdz + cc] = (b0 + rr < B && n0 + cc < N) ? dz_at(a, b0 + rr, n0 + cc) : 0.f;
            }
            stage_rows(xs, ld, a.x, B, K, b0, a.ln_g, a.ln_b, a.eps, st, nullptr, a.stats);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int kt = wave + kWaves * m;
                if (kt < TK) {
                    const int kcol = min(kt * 16 + r, K - 1);
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[m] = MFMA(dzs[(4 * q + j) * kLdz + r], xs[(4 * q + j) * ld + kcol], acc[m]);
                }
            }
            if (threadIdx.x < 16) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sb += dzs[i * kLdz + threadIdx.x];
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int kt = wave + kWaves * m;
            const int kcol = kt * 16 + r;
            if (kt < TK && kcol < K) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int n = n0 + 4 * q + i;
                    if (n < N) a.gw[(int64_t)n * K + kcol] = acc[m][i];
                }
            }
        }
        if (threadIdx.x < 16 && n0 + (int)threadIdx.x < N) a.gb[n0 + threadIdx.x] = sb;
        return;
    }
    blk -= a.nW;
    if (blk < a.nX) {  // role X: din rows b0 .. b0 + 15
        const int ldn = N + 4;
        float *xs = lds, *st = xs + 16 * ld, *ds = st + 32, *tmp = ds + 16 * ldn;
        const int b0 = blk * 16;
        for (int i = threadIdx.x; i < 16 * N; i += kThreads) {
            const int rr = i / N, n = i - rr * N;
            ds[rr * ldn + n] = b0 + rr < B ? dz_at(a, b0 + rr, n) : 0.f;
        }
        if (a.ln_g && threadIdx.x < 16) {
            const int row = min(b0 + (int)threadIdx.x, B - 1);
            st[threadIdx.x] = a.stats[2 * row];
            st[16 + threadIdx.x] = a.stats[2 * row + 1];
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int kt = wave + kWaves * m;
            if (kt < TK) {
                const f32x4 p = tile_xW(ds, ldn, a.w, K, kt * 16, K, N, lane);
                const int kcol = kt * 16 + r;
                if (kcol < K) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        if (a.ln_g)
                            xs[(4 * q + i) * ld + kcol] = p[i];
                        else if (b0 + 4 * q + i < B)
                            a.din[(int64_t)(b0 + 4 * q + i) * K + kcol] = p[i];
                    }
                }
            }
        }
        if (a.ln_g) {
            __syncthreads();
            ln_bwd_rows(xs, ld, nullptr, 0, tmp, ld, a.x, st, a.ln_g, B, K, b0, a.din, a.pg + (int64_t)blk * K,
                        a.pb + (int64_t)blk * K);
        }
        return;
    }
    column_sums(a.sg, nrt, N, a.g_g);  // role S
    column_sums(a.sb, nrt, N, a.g_b);
}

// ---------------------------------------------------------------------------
struct BlockArgs {
    const float *x;      // block input [B][H]
    const float *ln_g, *ln_b, *w1, *b1, *w2, *b2;
    float *y;            // forward: block output [B][H]
    float *stats;        // [B][2]
    const float *dy;     // backward: d/d y [B][H]
    float *dx;           // [B][H]
    float *g_w1, *g_b1, *g_w2, *g_b2;
    float *pg, *pb;      // role X: partial rows [row tiles][H] of this block's LayerNorm affine gradients
    const float *sg, *sb;  // role S: the previous launch's partial rows -> g_g, g_b (the next LayerNorm's)
    float *g_g, *g_b;
    int B, H, I, nW, nX;
    float eps;
};

// 16 units of one wave: u (or the pre-activation's sign) for rows of xs
__device__ __forceinline__ f32x4 units_pre(const BlockArgs &a, const float *xs, int ld, int u0, int lane) {
    f32x4 p = tile_xWt(xs, ld, a.w1, a.H, u0, a.I, a.H, lane);
    const float bias = a.b1[min(u0 + (lane & 15), a.I - 1)];
#pragma unroll
    for (int i = 0; i < 4; ++i) p[i] = relu(p[i] + bias);
    return p;
}

__global__ __launch_bounds__(kThreads) void block_fwd_kernel(BlockArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int B = a.B, H = a.H, I = a.I;
    const int ld = H + 4, T = (H + 15) >> 4;
    float *xs = lds, *st = xs + 16 * ld, *us = st + 32;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * 16;
    stage_rows(xs, ld, a.x, B, H, b0, a.ln_g, a.ln_b, a.eps, st, a.stats, nullptr);
    f32x4 acc[4] = {};
    for (int c0 = 0; c0 < I; c0 += kChunk) {
        const int u0 = c0 + wave * 16;
        f32x4 u = {0.f, 0.f, 0.f, 0.f};
        if (u0 < I) u = units_pre(a, xs, ld, u0, lane);
        const bool uok = u0 + r < I;
#pragma unroll
        for (int i = 0; i < 4; ++i) us[(4 * q + i) * kLdu + wave * 16 + r] = uok ? u[i] : 0.f;
        __syncthreads();
        const int kn = min(kChunk, I - c0);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int t = wave + kWaves * m;
            if (t < T) {
                const float *w2row = a.w2 + (int64_t)min(t * 16 + r, H - 1) * I + c0;
                const float *urow = us + r * kLdu;
                acc[m] = chain_rows(kn, q, acc[m], urow, kLdu, w2row, I);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int col = (wave + kWaves * m) * 16 + r;
        if (col < H) {
            const float bias = a.b2[col];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = b0 + 4 * q + i;
                if (row < B) a.y[(int64_t)row * H + col] = a.x[(int64_t)row * H + col] + (acc[m][i] + bias);
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void block_bwd_kernel(BlockArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int B = a.B, H = a.H, I = a.I;
    const int ld = H + 4, T = (H + 15) >> 4;
    const int nrt = (B + 15) >> 4;
    float *xs = lds, *st = xs + 16 * ld, *ds = st + 32, *us = ds + 16 * ld;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    int blk = blockIdx.x;
    if (blk < a.nW) {  // role W: 32 inner units, the whole batch
        float *gs = us + 16 * kLdw;  // us: u [16][36], gs: dy W2 [16][36], then du
        const int c0 = blk * kUnitsW;
        const int ut = wave & 1, hb = wave >> 1;  // this wave's dW tiles: unit tile ut, H tiles hb + 4 m
        f32x4 acc1[8] = {}, acc2[8] = {};
        float sb1 = 0.f;
        for (int rt = 0; rt < nrt; ++rt) {
            const int b0 = rt * 16;
            stage_rows(xs, ld, a.x, B, H, b0, a.ln_g, a.ln_b, a.eps, st, nullptr, a.stats);
            stage_rows(ds, ld, a.dy, B, H, b0, nullptr, nullptr, 0.f, st, nullptr, nullptr);
            if (wave < 4) {
                const int u0 = c0 + (wave & 1) * 16;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (u0 < I) v = wave < 2 ? units_pre(a, xs, ld, u0, lane) : tile_xW(ds, ld, a.w2, I, u0, I, H, lane);
                const bool uok = u0 + r < I;
                float *dst = wave < 2 ? us : gs;
#pragma unroll
                for (int i = 0; i < 4; ++i) dst[(4 * q + i) * kLdw + (wave & 1) * 16 + r] = uok ? v[i] : 0.f;
            }
            __syncthreads();
            if (threadIdx.x < 16 * kUnitsW) {  // du = g * [u > 0], in place
                const int rr = threadIdx.x >> 5, cc = threadIdx.x & 31;
                if (!(us[rr * kLdw + cc] > 0.f)) gs[rr * kLdw + cc] = 0.f;
            }
            __syncthreads();
            if (threadIdx.x < kUnitsW) {
#pragma unroll
                for (int i = 0; i < 16; ++i) sb1 += gs[i * kLdw + threadIdx.x];
            }
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int ht = hb + 4 * m;
                if (ht < T) {
                    const int hcol = min(ht * 16 + r, H - 1);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int bb = 4 * q + j;
                        acc1[m] = MFMA(gs[bb * kLdw + ut * 16 + r], xs[bb * ld + hcol], acc1[m]);
                        acc2[m] = MFMA(ds[bb * ld + hcol], us[bb * kLdw + ut * 16 + r], acc2[m]);
                    }
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int ht = hb + 4 * m;
            if (ht < T) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int unit = c0 + ut * 16 + 4 * q + i, h = ht * 16 + r;  // dW1[unit][h]
                    if (unit < I && h < H) a.g_w1[(int64_t)unit * H + h] = acc1[m][i];
                    const int h2 = ht * 16 + 4 * q + i, unit2 = c0 + ut * 16 + r;  // dW2[h2][unit2]
                    if (unit2 < I && h2 < H) a.g_w2[(int64_t)h2 * I + unit2] = acc2[m][i];
                }
            }
        }
        if (threadIdx.x < kUnitsW && c0 + (int)threadIdx.x < I) a.g_b1[c0 + threadIdx.x] = sb1;
        return;
    }
    blk -= a.nW;
    if (blk < a.nX) {  // role X: rows b0 .. b0 + 15
        const int b0 = blk * 16;
        stage_rows(xs, ld, a.x, B, H, b0, a.ln_g, a.ln_b, a.eps, st, nullptr, a.stats);
        stage_rows(ds, ld, a.dy, B, H, b0, nullptr, nullptr, 0.f, st, nullptr, nullptr);
        f32x4 acc[4] = {};
        for (int c0 = 0; c0 < I; c0 += kChunk) {
            const int u0 = c0 + wave * 16;
            f32x4 du = {0.f, 0.f, 0.f, 0.f};
            if (u0 < I) {
                const f32x4 u = units_pre(a, xs, ld, u0, lane);
                const f32x4 g = tile_xW(ds, ld, a.w2, I, u0, I, H, lane);
#pragma unroll
                for (int i = 0; i < 4; ++i) du[i] = u[i] > 0.f ? g[i] : 0.f;
            }
            const bool uok = u0 + r < I;
#pragma unroll
            for (int i = 0; i < 4; ++i) us[(4 * q + i) * kLdu + wave * 16 + r] = uok ? du[i] : 0.f;
            __syncthreads();
            const int kn = min(kChunk, I - c0);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int t = wave + kWaves * m;
                if (t < T) {
                    const float *w1col = a.w1 + (int64_t)c0 * H + min(t * 16 + r, H - 1);
                    const float *urow = us + r * kLdu;
                    acc[m] = chain(kn, q, acc[m], [&](int k) { return urow[k]; },
                                   [&](int k) { return w1col[(int64_t)k * H]; });
                }
            }
            __syncthreads();
        }
        // dxn over the normalised rows (xs is free: the last chunk's barrier is behind every reader)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int col = (wave + kWaves * m) * 16 + r;
            if (col < H) {
#pragma unroll
                for (int i = 0; i < 4; ++i) xs[(4 * q + i) * ld + col] = acc[m][i];
            }
        }
        __syncthreads();
        ln_bwd_rows(xs, ld, ds, ld, ds, ld, a.x, st, a.ln_g, B, H, b0, a.dx, a.pg + (int64_t)blk * H,
                    a.pb + (int64_t)blk * H);
        return;
    }
    column_sums(a.dy, B, H, a.g_b2);  // role S
    column_sums(a.sg, nrt, H, a.g_g);
    column_sums(a.sb, nrt, H, a.g_b);
}

static size_t lin_lds(int K, int N, bool role_x_ln) {
    size_t w = 16 * (K + 4) + 32 + 16 * kLdz;
    size_t x = 16 * (K + 4) + 32 + 16 * (N + 4) + (role_x_ln ? 16 * (K + 4) : 0);
    return (w > x ? w : x) * sizeof(float);
}

static size_t block_lds(int H) {
    const size_t ux = 16 * kLdu, uw = 2 * 16 * kLdw;
    return (2 * 16 * (size_t)(H + 4) + 32 + (ux > uw ? ux : uw)) * sizeof(float);
}

static void allow_lds() {
    static const bool once = [] {
        const int cap = 128 * 1024;
        (void)hipFuncSetAttribute((const void *)lin_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        (void)hipFuncSetAttribute((const void *)lin_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        (void)hipFuncSetAttribute((const void *)block_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        (void)hipFuncSetAttribute((const void *)block_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        return true;
    }();
    (void)once;
}

}  // namespace simba

// ---------------------------------------------------------------------------
static int check_desc(const agx_simba_desc *d, const float *x, int64_t B, bool backward, const char *who) {
    AGX_REQUIRE(d && x, "%s: descriptor / x is NULL", who);
    AGX_REQUIRE(B >= 1 && B <= AGX_SIMBA_MAX_ROWS, "%s: batch %lld outside [1, %d]", who, (long long)B,
                AGX_SIMBA_MAX_ROWS);
    AGX_REQUIRE(d->in >= 1 && d->in <= AGX_SIMBA_MAX_WIDTH && d->H >= 1 && d->H <= AGX_SIMBA_MAX_WIDTH &&
                    d->out_dim >= 1 && d->out_dim <= AGX_SIMBA_MAX_WIDTH,
                "%s: in %d, H %d, out %d outside [1, %d]", who, d->in, d->H, d->out_dim, AGX_SIMBA_MAX_WIDTH);
    AGX_REQUIRE(d->scale >= 1 && (int64_t)d->scale * d->H <= AGX_SIMBA_MAX_INNER, "%s: scale %d * H %d outside [1, %d]",
                who, d->scale, d->H, AGX_SIMBA_MAX_INNER);
    AGX_REQUIRE(d->blocks >= 1 && d->blocks <= AGX_SIMBA_MAX_BLOCKS, "%s: %d blocks outside [1, %d]", who, d->blocks,
                AGX_SIMBA_MAX_BLOCKS);
    AGX_REQUIRE(d->act == AGX_SIMBA_ACT_NONE || d->act == AGX_SIMBA_ACT_RELU, "%s: unknown output activation %d", who,
                d->act);
    AGX_REQUIRE(d->w_in && d->b_in && d->ln_g && d->ln_b && d->w_out && d->b_out && d->acts && d->stats && d->out,
                "%s: a parameter or saved tensor is NULL", who);
    AGX_REQUIRE(!backward || (d->g_w_in && d->g_b_in && d->g_ln_g && d->g_ln_b && d->g_w_out && d->g_b_out),
                "%s: a gradient output is NULL", who);
    for (int i = 0; i < d->blocks; ++i) {
        const agx_simba_block &b = d->blk[i];
        AGX_REQUIRE(b.ln_g && b.ln_b && b.w1 && b.b1 && b.w2 && b.b2, "%s: block %d: a parameter is NULL", who, i);
        AGX_REQUIRE(!backward || (b.g_ln_g && b.g_ln_b && b.g_w1 && b.g_b1 && b.g_w2 && b.g_b2),
                    "%s: block %d: a gradient output is NULL", who, i);
    }
    return AGX_OK;
}

extern "C" int agx_simba_forward(const agx_simba_desc *d, const float *x, int64_t B, void *stream) {
    if (int rc = check_desc(d, x, B, false, "agx_simba_forward")) return rc;
    simba::allow_lds();
    const int H = d->H, I = d->scale * d->H, nrt = (int)ceil_div(B, 16);
    const int64_t BH = B * H;
    hipStream_t s = as_stream(stream);
    simba::LinArgs l{};
    l.x = x;
    l.w = d->w_in;
    l.b = d->b_in;
    l.out = d->acts;
    l.B = (int)B;
    l.K = d->in;
    l.N = H;
    l.eps = d->eps;
    simba::lin_fwd_kernel<<<dim3(nrt, (unsigned)ceil_div(H, simba::kChunk)), simba::kThreads,
                            simba::lin_lds(d->in, H, false), s>>>(l);
    if (int rc = check_launch("agx_simba_forward")) return rc;
    for (int i = 0; i < d->blocks; ++i) {
        const agx_simba_block &b = d->blk[i];
        simba::BlockArgs a{};
        a.x = d->acts + i * BH;
        a.y = d->acts + (i + 1) * BH;
        a.stats = d->stats + i * B * 2;
        a.ln_g = b.ln_g;
        a.ln_b = b.ln_b;
        a.w1 = b.w1;
        a.b1 = b.b1;
        a.w2 = b.w2;
        a.b2 = b.b2;
        a.B = (int)B;
        a.H = H;
        a.I = I;
        a.eps = d->eps;
        simba::block_fwd_kernel<<<nrt, simba::kThreads, simba::block_lds(H), s>>>(a);
        if (int rc = check_launch("agx_simba_forward")) return rc;
    }
    simba::LinArgs t{};
    t.x = d->acts + d->blocks * BH;
    t.stats = d->stats + (int64_t)d->blocks * B * 2;
    t.ln_g = d->ln_g;
    t.ln_b = d->ln_b;
    t.w = d->w_out;
    t.b = d->b_out;
    t.out = d->out;
    t.B = (int)B;
    t.K = H;
    t.N = d->out_dim;
    t.relu = d->act == AGX_SIMBA_ACT_RELU;
    t.eps = d->eps;
    simba::lin_fwd_kernel<<<dim3(nrt, (unsigned)ceil_div(d->out_dim, simba::kChunk)), simba::kThreads,
                            simba::lin_lds(H, d->out_dim, false), s>>>(t);
    return check_launch("agx_simba_forward");
}

extern "C" size_t agx_simba_workspace_bytes(const agx_simba_desc *d, int64_t B) {
    if (!d || B < 1 || d->H < 1) return 0;
    return (size_t)(2 * B * d->H + 4 * ceil_div(B, 16) * d->H) * sizeof(float);
}

extern "C" int agx_simba_backward(const agx_simba_desc *d, const float *x, int64_t B, const float *grad_out,
                                  float *grad_x, void *workspace, void *stream) {
    if (int rc = check_desc(d, x, B, true, "agx_simba_backward")) return rc;
    AGX_REQUIRE(grad_out && workspace, "agx_simba_backward: grad_out / workspace is NULL");
    simba::allow_lds();
    const int H = d->H, I = d->scale * d->H, nrt = (int)ceil_div(B, 16);
    const int64_t BH = B * H;
    hipStream_t s = as_stream(stream);
    float *ws = static_cast<float *>(workspace);
    float *dbuf[2] = {ws, ws + BH};
    float *part[2] = {ws + 2 * BH, ws + 2 * BH + 2 * (int64_t)nrt * H};  // each: pg [nrt][H], pb [nrt][H]
    // tail: d out -> d h_blocks (dbuf[0]), the output LayerNorm's partial rows (part[0])
    simba::LinArgs t{};
    t.x = d->acts + d->blocks * BH;
    t.stats = d->stats + (int64_t)d->blocks * B * 2;
    t.ln_g = d->ln_g;
    t.ln_b = d->ln_b;
    t.w = d->w_out;
    t.gsrc = grad_out;
    t.outv = d->out;
    t.gw = d->g_w_out;
    t.gb = d->g_b_out;
    t.din = dbuf[0];
    t.pg = part[0];
    t.pb = part[0] + (int64_t)nrt * H;
    t.B = (int)B;
    t.K = H;
    t.N = d->out_dim;
    t.relu = d->act == AGX_SIMBA_ACT_RELU;
    t.nW = (int)ceil_div(d->out_dim, 16);
    t.nX = nrt;
    t.eps = d->eps;
    simba::lin_bwd_kernel<<<t.nW + t.nX, simba::kThreads, simba::lin_lds(H, d->out_dim, true), s>>>(t);
    if (int rc = check_launch("agx_simba_backward")) return rc;
    int cur = 0;  // dbuf[cur]: d h_{i + 1}; part[cur]: partial rows of the LayerNorm that reads h_{i + 1}
    for (int i = d->blocks - 1; i >= 0; --i) {
        const agx_simba_block &b = d->blk[i];
        simba::BlockArgs a{};
        a.x = d->acts + i * BH;
        a.stats = d->stats + i * B * 2;
        a.ln_g = b.ln_g;
        a.ln_b = b.ln_b;
        a.w1 = b.w1;
        a.b1 = b.b1;
        a.w2 = b.w2;
        a.b2 = b.b2;
        a.dy = dbuf[cur];
        a.dx = dbuf[cur ^ 1];
        a.g_w1 = b.g_w1;
        a.g_b1 = b.g_b1;
        a.g_w2 = b.g_w2;
        a.g_b2 = b.g_b2;
        a.pg = part[cur ^ 1];
        a.pb = part[cur ^ 1] + (int64_t)nrt * H;
        a.sg = part[cur];
        a.sb = part[cur] + (int64_t)nrt * H;
        a.g_g = i == d->blocks - 1 ? d->g_ln_g : d->blk[i + 1].g_ln_g;
        a.g_b = i == d->blocks - 1 ? d->g_ln_b : d->blk[i + 1].g_ln_b;
        a.B = (int)B;
        a.H = H;
        a.I = I;
        a.nW = (int)ceil_div(I, simba::kUnitsW);
        a.nX = nrt;
        a.eps = d->eps;
        simba::block_bwd_kernel<<<a.nW + a.nX + 1, simba::kThreads, simba::block_lds(H), s>>>(a);
        if (int rc = check_launch("agx_simba_backward")) return rc;
        cur ^= 1;
    }
    // input layer: d h_0 -> dW_in, db_in, d x; block 0's LayerNorm affine gradients from part[cur]
    simba::LinArgs l{};
    l.x = x;
    l.w = d->w_in;
    l.gsrc = dbuf[cur];
    l.gw = d->g_w_in;
    l.gb = d->g_b_in;
    l.din = grad_x;
    l.sg = part[cur];
    l.sb = part[cur] + (int64_t)nrt * H;
    l.g_g = d->blk[0].g_ln_g;
    l.g_b = d->blk[0].g_ln_b;
    l.B = (int)B;
    l.K = d->in;
    l.N = H;
    l.nW = (int)ceil_div(H, 16);
    l.nX = grad_x ? nrt : 0;
    l.eps = d->eps;
    simba::lin_bwd_kernel<<<l.nW + l.nX + 1, simba::kThreads, simba::lin_lds(d->in, H, false), s>>>(l);
    return check_launch("agx_simba_backward");
}

}  // namespace agx
