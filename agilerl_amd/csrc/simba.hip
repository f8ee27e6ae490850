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
//
// Split plans (block_fwd_split_kernel / block_bwd_split_kernel, further down):
// the same routines on a (row groups x inner slices) grid, role W's row tiles
// dealt to Q workgroups per unit range, role S on 64-column workgroups; the
// partial tiles are summed in slice / range order by the last workgroup to
// take a ticket (last_arriver), with no waiting.  Plan (1, 1, 1) launches the
// kernels above.
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

// ---------------------------------------------------------------------------
// Split variants (plan S, R, Q of include/agx_simba.h).  The forward and role X run on a (row group x
// inner slice) grid: a workgroup stages R row tiles, walks only its slice's chunks with every weight
// operand it loads feeding R accumulators (chain_r: the chain above, per tile the same k order and so
// the same bits), and leaves a partial tile in part [S][B][H].  Role W deals the row tiles to Q
// workgroups per unit range, each leaving partial dW1 / dW2 / db1.  The partials are summed by whichever
// workgroup of the group arrives last (last_arriver), in slice / range order; nobody waits.
struct SplitArgs {
    BlockArgs a;
    float *part;         // [S][B][H]: partial y (forward) / dxn (role X)
    float *wpart;        // [Q][2 I H + I]: partial dW1 [I][H], dW2 [H][I], db1 [I]
    unsigned *ctr_rows;  // one ticket counter per row group, zero between launches
    unsigned *ctr_units; // one per role-W unit range
    int S, Q, ngroups, nS;
};

// items [lo, lo + cnt) of n dealt to `parts` in order, as evenly as possible, the extra ones first
__host__ __device__ inline void deal(int n, int parts, int p, int &lo, int &cnt) {
    const int base = n / parts, rem = n % parts;
    cnt = base + (p < rem ? 1 : 0);
    lo = p * base + (p < rem ? p : rem);
}

// After a workgroup's partial stores: every wave releases them at agent scope, one thread takes a ticket,
// and the drawer of the last of n tickets acquires in every wave.  True in that workgroup only; the
// others go on (to their exit) without looking at the counter again.
__device__ __forceinline__ bool last_arriver(unsigned *ctr, unsigned n, int *flag) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __syncthreads();
    if (threadIdx.x == 0)
        *flag = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u == n;
    __syncthreads();
    const bool last = *flag != 0;
    if (last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    return last;
}

// chain for R row tiles sharing the w operand: acc[t] += sum_k a_at(t, k) * w_at(k)
template <int R, typename FA, typename FW>
__device__ __forceinline__ void chain_r(int K, int q, f32x4 (&acc)[R], FA a_at, FW w_at) {
    constexpr int NB = R == 4 ? 8 : 16;  // w operands in flight (R = 4: two steps, for the register budget)
    for (int kc = 0; kc < K; kc += 4 * NB) {
        float w[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const int k = kc + 16 * (u >> 2) + 4 * q + (u & 3);
            w[u] = k < K ? w_at(min(k, K - 1)) : 0.f;
        }
#pragma unroll
        for (int u = 0; u < NB; ++u)
            if (kc + 16 * (u >> 2) < K) {
                const int k = kc + 16 * (u >> 2) + 4 * q + (u & 3);
#pragma unroll
                for (int t = 0; t < R; ++t) acc[t] = MFMA(k < K ? a_at(t, min(k, K - 1)) : 0.f, w[u], acc[t]);
            }
    }
}

// chain4 for R row tiles: tile t's row is arow + t * astride
template <int R>
__device__ __forceinline__ void chain4_r(int K, int q, f32x4 (&acc)[R], const float *arow, int astride,
                                         const float *wrow) {
    for (int kc = 0; kc < K; kc += 64) {
        f32x4 w[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kc + 16 * s + 4 * q;
            w[s] = *reinterpret_cast<const f32x4 *>(wrow + min(k, K - 4));
            if (k >= K) w[s] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (kc + 16 * s < K) {
                const int k = kc + 16 * s + 4 * q;
#pragma unroll
                for (int t = 0; t < R; ++t) {
                    f32x4 av = *reinterpret_cast<const f32x4 *>(arow + t * astride + min(k, K - 4));
                    if (k >= K) av = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[t] = MFMA(av[j], w[s][j], acc[t]);
                }
            }
    }
}

template <int R>
__device__ __forceinline__ void chain_rows_r(int K, int q, f32x4 (&acc)[R], const float *arow, int lda, int astride,
                                             const float *wrow, int ldw) {
    if (rows16(arow, lda | astride, wrow, ldw, K)) return chain4_r<R>(K, q, acc, arow, astride, wrow);
    chain_r<R>(K, q, acc, [&](int t, int k) { return arow[t * astride + k]; }, [&](int k) { return wrow[k]; });
}

// units_pre for the R tiles staged in xs [16 R][ld]
template <int R>
__device__ __forceinline__ void units_pre_r(const BlockArgs &a, const float *xs, int ld, int u0, int lane,
                                            f32x4 (&p)[R]) {
    const int r = lane & 15;
    chain_rows_r<R>(a.H, lane >> 4, p, xs + r * ld, ld, 16 * ld, a.w1 + (int64_t)min(u0 + r, a.I - 1) * a.H, a.H);
    const float bias = a.b1[min(u0 + r, a.I - 1)];
#pragma unroll
    for (int t = 0; t < R; ++t) {
#pragma unroll
        for (int i = 0; i < 4; ++i) p[t][i] = relu(p[t][i] + bias);
    }
}

// this workgroup's slice of the inner units, in whole 16-unit tiles
__device__ __forceinline__ void slice_units(int I, int S, int s, int &u_lo, int &u_hi) {
    int t0, tc;
    deal((I + 15) >> 4, S, s, t0, tc);
    u_lo = t0 * 16;
    u_hi = min(I, (t0 + tc) * 16);
}

// this thread's accumulators acc[m][t] (column tile wave + 8 m, row tile t) -> dst [B][H] rows b0 ..
template <int R>
__device__ __forceinline__ void put_tiles(const f32x4 (&acc)[4][R], float *dst, int B, int H, int b0) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int col = (wave + kWaves * m) * 16 + r;
        if (col < H) {
#pragma unroll
            for (int t = 0; t < R; ++t) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = b0 + 16 * t + 4 * q + i;
                    if (row < B) dst[(int64_t)row * H + col] = acc[m][t][i];
                }
            }
        }
    }
}

// sum over the S partials of element o, in slice order
__device__ __forceinline__ float sum_parts(const float *part, int64_t stride, int S, int64_t o) {
    float v = part[o];
    for (int s = 1; s < S; ++s) v += part[s * stride + o];
    return v;
}

template <int R>
__global__ __launch_bounds__(kThreads) void block_fwd_split_kernel(SplitArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const BlockArgs &a = p.a;
    const int B = a.B, H = a.H, I = a.I;
    const int ld = H + 4, T = (H + 15) >> 4;
    float *xs = lds, *st = xs + 16 * R * ld, *us = st + 32 * R;
    int *flag = reinterpret_cast<int *>(us + 16 * R * kLdu);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int grp = blockIdx.x, s = blockIdx.y;
    const int b0 = grp * 16 * R;
#pragma unroll
    for (int t = 0; t < R; ++t)
        stage_rows(xs + t * 16 * ld, ld, a.x, B, H, b0 + 16 * t, a.ln_g, a.ln_b, a.eps, st + 32 * t,
                   s == 0 ? a.stats : nullptr, nullptr);
    int u_lo, u_hi;
    slice_units(I, p.S, s, u_lo, u_hi);
    f32x4 acc[4][R] = {};
    for (int c0 = u_lo; c0 < u_hi; c0 += kChunk) {
        const int u0 = c0 + wave * 16;
        f32x4 u[R] = {};
        if (u0 < u_hi) units_pre_r<R>(a, xs, ld, u0, lane, u);
        const bool uok = u0 < u_hi && u0 + r < I;
#pragma unroll
        for (int t = 0; t < R; ++t) {
#pragma unroll
            for (int i = 0; i < 4; ++i) us[(16 * t + 4 * q + i) * kLdu + wave * 16 + r] = uok ? u[t][i] : 0.f;
        }
        __syncthreads();
        const int kn = min(kChunk, u_hi - c0);
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int tc = wave + kWaves * m;
            if (tc < T)
                chain_rows_r<R>(kn, q, acc[m], us + r * kLdu, kLdu, 16 * kLdu,
                                a.w2 + (int64_t)min(tc * 16 + r, H - 1) * I + c0, I);
        }
        __syncthreads();
    }
    const int64_t BH = (int64_t)B * H;
    if (p.S == 1) {  // nothing to sum: finish from the registers
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int col = (wave + kWaves * m) * 16 + r;
            if (col < H) {
                const float bias = a.b2[col];
#pragma unroll
                for (int t = 0; t < R; ++t) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = b0 + 16 * t + 4 * q + i;
                        if (row < B) a.y[(int64_t)row * H + col] = a.x[(int64_t)row * H + col] + (acc[m][t][i] + bias);
                    }
                }
            }
        }
        return;
    }
    put_tiles<R>(acc, p.part + s * BH, B, H, b0);
    if (!last_arriver(p.ctr_rows + grp, p.S, flag)) return;
    const int rows = min(16 * R, B - b0);
    for (int i = threadIdx.x; i < rows * H; i += kThreads) {
        const int k = i % H;
        const int64_t o = (int64_t)b0 * H + i;
        a.y[o] = a.x[o] + (sum_parts(p.part, BH, p.S, o) + a.b2[k]);
    }
    if (threadIdx.x == 0) __hip_atomic_store(p.ctr_rows + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// role S of the split backward: 64 columns per workgroup, the rows dealt round the eight waves and the
// waves' sums added in wave order
__device__ __forceinline__ void column_sums_split(const float *src, int rows, int H, int c0, float *dst, float *red) {
    if (!src) return;
    const int c = threadIdx.x & 63, w = threadIdx.x >> 6, col = c0 + c;
    float v = 0.f;
    if (col < H) {
#pragma unroll 4
        for (int b = w; b < rows; b += kWaves) v += src[(int64_t)b * H + col];
    }
    red[w * 64 + c] = v;
    __syncthreads();
    if (w == 0 && col < H) {
        float t = red[c];
#pragma unroll
        for (int j = 1; j < kWaves; ++j) t += red[j * 64 + c];
        dst[col] = t;
    }
    __syncthreads();
}

template <int R>
__global__ __launch_bounds__(kThreads) void block_bwd_split_kernel(SplitArgs p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const BlockArgs &a = p.a;
    const int B = a.B, H = a.H, I = a.I;
    const int ld = H + 4, T = (H + 15) >> 4;
    const int nrt = (B + 15) >> 4;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    int blk = blockIdx.x;
    if (blk < a.nW) {  // role W: 32 inner units, one of Q ranges of the row tiles
        float *xs = lds, *st = xs + 16 * ld, *ds = st + 32, *us = ds + 16 * ld, *gs = us + 16 * kLdw;
        int *flag = reinterpret_cast<int *>(gs + 16 * kLdw);
        const int uw = blk / p.Q, qi = blk - uw * p.Q;
        const int c0 = uw * kUnitsW;
        int rt_lo, rt_n;
        deal(nrt, p.Q, qi, rt_lo, rt_n);
        const int ut = wave & 1, hb = wave >> 1;
        f32x4 acc1[8] = {}, acc2[8] = {};
        float sb1 = 0.f;
        for (int rt = rt_lo; rt < rt_lo + rt_n; ++rt) {
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
            if (threadIdx.x < 16 * kUnitsW) {
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
        const int64_t IH = (int64_t)I * H;
        float *w1 = a.g_w1, *w2 = a.g_w2, *b1 = a.g_b1;
        if (p.Q > 1) {
            w1 = p.wpart + qi * (2 * IH + I);
            w2 = w1 + IH;
            b1 = w2 + IH;
        }
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            const int ht = hb + 4 * m;
            if (ht < T) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int unit = c0 + ut * 16 + 4 * q + i, h = ht * 16 + r;
                    if (unit < I && h < H) w1[(int64_t)unit * H + h] = acc1[m][i];
                    const int h2 = ht * 16 + 4 * q + i, unit2 = c0 + ut * 16 + r;
                    if (unit2 < I && h2 < H) w2[(int64_t)h2 * I + unit2] = acc2[m][i];
                }
            }
        }
        if (threadIdx.x < kUnitsW && c0 + (int)threadIdx.x < I) b1[c0 + threadIdx.x] = sb1;
        if (p.Q == 1 || !last_arriver(p.ctr_units + uw, p.Q, flag)) return;
        const int nu = min(kUnitsW, I - c0);
        const int64_t stride = 2 * IH + I;
        for (int i = threadIdx.x; i < nu * H; i += kThreads) {  // dW1 rows c0 .. c0 + nu - 1 are contiguous
            const int64_t o = (int64_t)c0 * H + i;
            a.g_w1[o] = sum_parts(p.wpart, stride, p.Q, o);
        }
        for (int i = threadIdx.x; i < H * kUnitsW; i += kThreads) {
            const int h = i >> 5, uu = i & 31;
            const int64_t o = (int64_t)h * I + c0 + uu;
            if (uu < nu) a.g_w2[o] = sum_parts(p.wpart + IH, stride, p.Q, o);
        }
        if ((int)threadIdx.x < nu) a.g_b1[c0 + threadIdx.x] = sum_parts(p.wpart + 2 * IH, stride, p.Q, c0 + threadIdx.x);
        if (threadIdx.x == 0) __hip_atomic_store(p.ctr_units + uw, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }
    blk -= a.nW;
    if (blk < a.nX) {  // role X: R row tiles, one inner slice
        float *xs = lds, *st = xs + 16 * R * ld, *ds = st + 32 * R, *us = ds + 16 * R * ld;
        int *flag = reinterpret_cast<int *>(us + 16 * R * kLdu);
        const int s = blk / p.ngroups, grp = blk - s * p.ngroups;
        const int b0 = grp * 16 * R;
#pragma unroll
        for (int t = 0; t < R; ++t) {
            stage_rows(xs + t * 16 * ld, ld, a.x, B, H, b0 + 16 * t, a.ln_g, a.ln_b, a.eps, st + 32 * t, nullptr,
                       a.stats);
            stage_rows(ds + t * 16 * ld, ld, a.dy, B, H, b0 + 16 * t, nullptr, nullptr, 0.f, st, nullptr, nullptr);
        }
        int u_lo, u_hi;
        slice_units(I, p.S, s, u_lo, u_hi);
        f32x4 acc[4][R] = {};
        for (int c0 = u_lo; c0 < u_hi; c0 += kChunk) {
            const int u0 = c0 + wave * 16;
            f32x4 du[R] = {};
            if (u0 < u_hi) {
                f32x4 u[R] = {};
                units_pre_r<R>(a, xs, ld, u0, lane, u);
                const float *wcol = a.w2 + min(u0 + r, I - 1);
                const float *drow = ds + r * ld;
                chain_r<R>(H, q, du, [&](int t, int k) { return drow[t * 16 * ld + k]; },
                           [&](int k) { return wcol[(int64_t)k * I]; });
#pragma unroll
                for (int t = 0; t < R; ++t) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) du[t][i] = u[t][i] > 0.f ? du[t][i] : 0.f;
                }
            }
            const bool uok = u0 < u_hi && u0 + r < I;
#pragma unroll
            for (int t = 0; t < R; ++t) {
#pragma unroll
                for (int i = 0; i < 4; ++i) us[(16 * t + 4 * q + i) * kLdu + wave * 16 + r] = uok ? du[t][i] : 0.f;
            }
            __syncthreads();
            const int kn = min(kChunk, u_hi - c0);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int tc = wave + kWaves * m;
                if (tc < T) {
                    const float *w1col = a.w1 + (int64_t)c0 * H + min(tc * 16 + r, H - 1);
                    const float *urow = us + r * kLdu;
                    chain_r<R>(kn, q, acc[m], [&](int t, int k) { return urow[t * 16 * kLdu + k]; },
                               [&](int k) { return w1col[(int64_t)k * H]; });
                }
            }
            __syncthreads();
        }
        const int64_t BH = (int64_t)B * H;
        if (p.S == 1) {  // dxn over the normalised rows, as in block_bwd_kernel
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int col = (wave + kWaves * m) * 16 + r;
                if (col < H) {
#pragma unroll
                    for (int t = 0; t < R; ++t) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) xs[(16 * t + 4 * q + i) * ld + col] = acc[m][t][i];
                    }
                }
            }
        } else {
            put_tiles<R>(acc, p.part + s * BH, B, H, b0);
            if (!last_arriver(p.ctr_rows + grp, p.S, flag)) return;
            for (int i = threadIdx.x; i < 16 * R * H; i += kThreads) {
                const int rr = i / H, k = i - rr * H;
                xs[rr * ld + k] = b0 + rr < B ? sum_parts(p.part, BH, p.S, (int64_t)(b0 + rr) * H + k) : 0.f;
            }
            if (threadIdx.x == 0) __hip_atomic_store(p.ctr_rows + grp, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < R; ++t) {
            const int rt = grp * R + t;
            if (rt < nrt)
                ln_bwd_rows(xs + t * 16 * ld, ld, ds + t * 16 * ld, ld, ds + t * 16 * ld, ld, a.x, st + 32 * t, a.ln_g, B, H,
                            rt * 16, a.dx, a.pg + (int64_t)rt * H, a.pb + (int64_t)rt * H);
        }
        return;
    }
    blk -= a.nX;  // role S
    column_sums_split(a.dy, B, H, blk * 64, a.g_b2, lds);
    column_sums_split(a.sg, nrt, H, blk * 64, a.g_g, lds);
    column_sums_split(a.sb, nrt, H, blk * 64, a.g_b, lds);
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

constexpr size_t kSplitLdsCap = 160 * 1024;  // gfx950's LDS; the split role X at H = 496, R = 2 needs 141.8 KB

static size_t split_fwd_lds(int H, int R) {
    return ((size_t)16 * R * (H + 4) + 32 * R + 16 * R * kLdu + 4) * sizeof(float);
}

static size_t split_bwd_lds(int H, int R) {
    const size_t x = (size_t)2 * 16 * R * (H + 4) + 32 * R + 16 * R * kLdu + 4;
    const size_t w = (size_t)2 * 16 * (H + 4) + 32 + 2 * 16 * kLdw + 4;
    return (x > w ? x : w) * sizeof(float);
}

static void allow_lds() {
    static const bool once = [] {
        const int cap = 128 * 1024;
        const int scap = (int)kSplitLdsCap;
#define AGX_SPLIT_LDS(R)                                                                                              \
    (void)hipFuncSetAttribute((const void *)block_fwd_split_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize,    \
                              scap);                                                                                  \
    (void)hipFuncSetAttribute((const void *)block_bwd_split_kernel<R>, hipFuncAttributeMaxDynamicSharedMemorySize, scap)
        AGX_SPLIT_LDS(1);
        AGX_SPLIT_LDS(2);
        AGX_SPLIT_LDS(4);
#undef AGX_SPLIT_LDS
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

static const agx_simba_plan kWholePlan = {1, 1, 1};

static bool whole(const agx_simba_plan &p) { return p.slices == 1 && p.row_tiles == 1 && p.w_parts == 1; }

// Dimensions and plan only (no pointers, no HIP call): what agx_simba_choose_plan and the workspace size need.
static int check_plan(const agx_simba_desc *d, int64_t B, const agx_simba_plan *p, bool backward, const char *who) {
    AGX_REQUIRE(d && p, "%s: descriptor / plan is NULL", who);
    AGX_REQUIRE(B >= 1 && B <= AGX_SIMBA_MAX_ROWS, "%s: batch %lld outside [1, %d]", who, (long long)B,
                AGX_SIMBA_MAX_ROWS);
    AGX_REQUIRE(d->H >= 1 && d->H <= AGX_SIMBA_MAX_WIDTH && d->scale >= 1 &&
                    (int64_t)d->scale * d->H <= AGX_SIMBA_MAX_INNER,
                "%s: H %d, scale %d outside the limits", who, d->H, d->scale);
    const int nt = (int)ceil_div((int64_t)d->scale * d->H, 16), nrt = (int)ceil_div(B, 16);
    AGX_REQUIRE(p->slices >= 1 && p->slices <= AGX_SIMBA_MAX_SLICES && p->slices <= nt,
                "%s: %d inner slices outside [1, min(%d, %d unit tiles)]", who, p->slices, AGX_SIMBA_MAX_SLICES, nt);
    AGX_REQUIRE(p->row_tiles == 1 || p->row_tiles == 2 || p->row_tiles == 4, "%s: %d row tiles per workgroup, not 1, 2 or 4",
                who, p->row_tiles);
    AGX_REQUIRE(p->w_parts >= 1 && p->w_parts <= AGX_SIMBA_MAX_W_PARTS && p->w_parts <= nrt,
                "%s: %d role-W row ranges outside [1, min(%d, %d row tiles)]", who, p->w_parts, AGX_SIMBA_MAX_W_PARTS,
                nrt);
    if (whole(*p)) return AGX_OK;
    const size_t lds = backward ? simba::split_bwd_lds(d->H, p->row_tiles) : simba::split_fwd_lds(d->H, p->row_tiles);
    AGX_REQUIRE(lds <= simba::kSplitLdsCap, "%s: %d row tiles of H %d need %zu bytes of LDS, over %zu", who, p->row_tiles,
                d->H, lds, simba::kSplitLdsCap);
    return AGX_OK;
}

extern "C" int agx_simba_choose_plan(const agx_simba_desc *d, int64_t B, agx_simba_plan *plan) {
    AGX_REQUIRE(plan, "agx_simba_choose_plan: plan is NULL");
    *plan = kWholePlan;
    if (int rc = check_plan(d, B, plan, true, "agx_simba_choose_plan")) return rc;
    const int64_t H = d->H, I = (int64_t)d->scale * H;
    if (B <= 256 && d->scale * H * H <= 4 * 224 * 224) return AGX_OK;  // the whole kernels' measured range
    const int nrt = (int)ceil_div(B, 16), nt = (int)ceil_div(I, 16);
    // The fastest candidate of the sweep (tools/simba_time.py --plans) at B = 64 / 256 / 1024
    // and H = 128 .. 496, scale 4; between the measured points the nearest column above.  R = 1 throughout:
    // sharing a weight operand between row tiles was never the fastest.
    int S, Q;
    if (nrt <= 4) {
        S = 8, Q = 1;
    } else if (nrt <= 16) {
        S = H <= 320 ? 4 : 8, Q = H <= 320 ? 4 : 2;
    } else {
        S = H < 320 ? 2 : 4, Q = 4;
    }
    plan->slices = S < nt ? S : nt;
    plan->row_tiles = 1;
    plan->w_parts = Q < nrt ? Q : nrt;
    return AGX_OK;
}

extern "C" size_t agx_simba_split_workspace_bytes(const agx_simba_desc *d, int64_t B, const agx_simba_plan *p,
                                                  int backward) {
    if (check_plan(d, B, p, backward != 0, "agx_simba_split_workspace_bytes")) return 0;
    const int64_t H = d->H, I = (int64_t)d->scale * H;
    int64_t n = p->slices > 1 ? p->slices * B * H : 0;
    if (backward) n += 2 * B * H + 4 * ceil_div(B, 16) * H + (p->w_parts > 1 ? p->w_parts * (2 * I * H + I) : 0);
    return AGX_SIMBA_COUNTER_BYTES + (size_t)n * sizeof(float);
}

static void launch_fwd_split(int R, dim3 grid, size_t lds, hipStream_t s, const simba::SplitArgs &p) {
    if (R == 1) simba::block_fwd_split_kernel<1><<<grid, simba::kThreads, lds, s>>>(p);
    if (R == 2) simba::block_fwd_split_kernel<2><<<grid, simba::kThreads, lds, s>>>(p);
    if (R == 4) simba::block_fwd_split_kernel<4><<<grid, simba::kThreads, lds, s>>>(p);
}

static void launch_bwd_split(int R, dim3 grid, size_t lds, hipStream_t s, const simba::SplitArgs &p) {
    if (R == 1) simba::block_bwd_split_kernel<1><<<grid, simba::kThreads, lds, s>>>(p);
    if (R == 2) simba::block_bwd_split_kernel<2><<<grid, simba::kThreads, lds, s>>>(p);
    if (R == 4) simba::block_bwd_split_kernel<4><<<grid, simba::kThreads, lds, s>>>(p);
}

// ws: the split plans' workspace (counters, then the partials); unused by the whole plan
static int forward_plan(const agx_simba_desc *d, const float *x, int64_t B, const agx_simba_plan &plan, void *ws,
                        void *stream, const char *who) {
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
    if (int rc = check_launch(who)) return rc;
    const int R = plan.row_tiles, groups = (int)ceil_div(nrt, R);
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
        if (whole(plan)) {
            simba::block_fwd_kernel<<<nrt, simba::kThreads, simba::block_lds(H), s>>>(a);
        } else {
            simba::SplitArgs p{};
            p.a = a;
            p.ctr_rows = static_cast<unsigned *>(ws);
            p.part = reinterpret_cast<float *>(static_cast<char *>(ws) + AGX_SIMBA_COUNTER_BYTES);
            p.S = plan.slices;
            p.ngroups = groups;
            launch_fwd_split(R, dim3(groups, plan.slices), simba::split_fwd_lds(H, R), s, p);
        }
        if (int rc = check_launch(who)) return rc;
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
    return check_launch(who);
}

extern "C" int agx_simba_forward(const agx_simba_desc *d, const float *x, int64_t B, void *stream) {
    if (int rc = check_desc(d, x, B, false, "agx_simba_forward")) return rc;
    return forward_plan(d, x, B, kWholePlan, nullptr, stream, "agx_simba_forward");
}

extern "C" int agx_simba_forward_split(const agx_simba_desc *d, const float *x, int64_t B, const agx_simba_plan *plan,
                                       void *workspace, void *stream) {
    if (int rc = check_plan(d, B, plan, false, "agx_simba_forward_split")) return rc;
    if (int rc = check_desc(d, x, B, false, "agx_simba_forward_split")) return rc;
    AGX_REQUIRE(workspace, "agx_simba_forward_split: workspace is NULL");
    return forward_plan(d, x, B, *plan, workspace, stream, "agx_simba_forward_split");
}

extern "C" size_t agx_simba_workspace_bytes(const agx_simba_desc *d, int64_t B) {
    if (!d || B < 1 || d->H < 1) return 0;
    return (size_t)(2 * B * d->H + 4 * ceil_div(B, 16) * d->H) * sizeof(float);
}

// workspace: agx_simba_workspace_bytes' buffers; sws: the split plans' counters, then their partials
static int backward_plan(const agx_simba_desc *d, const float *x, int64_t B, const float *grad_out, float *grad_x,
                         const agx_simba_plan &plan, void *workspace, void *sws, void *stream, const char *who) {
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
    if (int rc = check_launch(who)) return rc;
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
        if (whole(plan)) {
            simba::block_bwd_kernel<<<a.nW + a.nX + 1, simba::kThreads, simba::block_lds(H), s>>>(a);
        } else {
            const int R = plan.row_tiles;
            simba::SplitArgs p{};
            p.S = plan.slices;
            p.Q = plan.w_parts;
            p.ngroups = (int)ceil_div(nrt, R);
            p.nS = (int)ceil_div(H, 64);
            p.ctr_rows = static_cast<unsigned *>(sws);
            p.ctr_units = p.ctr_rows + AGX_SIMBA_COUNTER_BYTES / 8;
            p.part = reinterpret_cast<float *>(static_cast<char *>(sws) + AGX_SIMBA_COUNTER_BYTES);
            p.wpart = p.part + (p.S > 1 ? p.S * BH : 0);
            a.nW *= p.Q;
            a.nX = p.ngroups * p.S;
            p.a = a;
            launch_bwd_split(R, dim3(a.nW + a.nX + p.nS), simba::split_bwd_lds(H, R), s, p);
        }
        if (int rc = check_launch(who)) return rc;
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
    return check_launch(who);
}

extern "C" int agx_simba_backward(const agx_simba_desc *d, const float *x, int64_t B, const float *grad_out,
                                  float *grad_x, void *workspace, void *stream) {
    if (int rc = check_desc(d, x, B, true, "agx_simba_backward")) return rc;
    AGX_REQUIRE(grad_out && workspace, "agx_simba_backward: grad_out / workspace is NULL");
    return backward_plan(d, x, B, grad_out, grad_x, kWholePlan, workspace, nullptr, stream, "agx_simba_backward");
}

extern "C" int agx_simba_backward_split(const agx_simba_desc *d, const float *x, int64_t B, const float *grad_out,
                                        float *grad_x, const agx_simba_plan *plan, void *workspace, void *stream) {
    if (int rc = check_plan(d, B, plan, true, "agx_simba_backward_split")) return rc;
    if (int rc = check_desc(d, x, B, true, "agx_simba_backward_split")) return rc;
    AGX_REQUIRE(grad_out && workspace, "agx_simba_backward_split: grad_out / workspace is NULL");
    // the workspace: counters, the partials, then agx_simba_backward's own buffers
    char *sws = static_cast<char *>(workspace);
    const int64_t H = d->H, I = (int64_t)d->scale * H;
    const int64_t parts = (plan->slices > 1 ? plan->slices * B * H : 0) +
                          (plan->w_parts > 1 ? plan->w_parts * (2 * I * H + I) : 0);
    return backward_plan(d, x, B, grad_out, grad_x, *plan, sws + AGX_SIMBA_COUNTER_BYTES + parts * sizeof(float), sws,
                         stream, "agx_simba_backward_split");
}

}  // namespace agx
