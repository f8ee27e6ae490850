// Stacked LSTM sequences (include/agx_lstm.h): the forward of the whole stack
// in one launch, the backward in three launches per layer, fp32 MFMA.
//
// Every workgroup is 8 waves.  The scans (fwd_kernel, bwd_scan_kernel) give
// one workgroup a 16-row tile of the batch and split the work over its waves
// by hidden unit: wave w owns the 16-unit tiles w, w + 8, ... (NT of them).
// For a tile it accumulates the four gate tiles i, f, g, o with the same A
// operand, so after the MFMA chain lane (r, q) holds all four pre-activations
// of rows 4q .. 4q + 3, unit u0 + r, and the cell update needs no exchange.
//
// Forward, per layer and step t:
//   acc[g] = b_ih + b_hh;  acc[g] += x_t W_ih[g]^T (A: the staged input tile,
//   B: W_ih rows from L2, 16-byte loads batched ahead of their MFMAs);
//   acc[g] += h_{t-1} W_hh[g]^T (A: the h tile in LDS; B: registers for H <=
//   64 (KS > 0), loaded once per layer, else streamed like W_ih);
//   c = f c + i g, h = o tanh(c) in registers; h_t to the other h tile, to
//   the layer's output and, when saving, the gates and c_t to `saved`.
//   The input tile of step t + 1 is staged into the other x tile after the
//   step's math, so a step has one barrier.
// The k order of every accumulator is ascending and the same whatever B, T
// and the row's place in the tile, which makes chunked runs bit-equal.
//
// Backward of a layer:
//   bwd_scan_kernel: the same tiles walk t = T-1 .. 0 with dh and dc in
//     registers (the MFMA output layout is the element-wise layout, so dh
//     needs no LDS); the gate gradients dG_t go to an LDS tile [16][4H] and
//     to the workspace; dh_{t-1} = dG_t W_hh (A: the LDS tile, B: W_hh read
//     down its columns, in registers for H <= 64).
//   dw_kernel: one workgroup per (16 gate rows, 8 column tiles); a wave owns
//     a 16 x 16 tile of [dW_ih | dW_hh | db] and sums it over all B * T rows
//     in ascending order (the bias column is a tile whose B operand is 1).
//   dx_kernel: one workgroup per 16 rows of B * T: dX = dG W_ih, the gradient
//     of the layer below (or of x).
// Nothing waits on another workgroup and no sum is split.
#include <cstdint>

#include "agx_common.h"
#include "lstm_gates.h"
#include "../../include/agx_lstm.h"

namespace agx {

namespace lstm {

constexpr int kThreads = 512;
constexpr int kWaves = 8;

// ---------------------------------------------------------------------------
struct FwdArgs {
    agx_lstm_desc d;
    const float *x, *h0, *c0;
    float *y, *hn, *cn, *saved;
    int B;
    int64_t T;
};

// NT: unit tiles per wave; KS > 0: W_hh in registers, H <= 16 * KS (NT == 1)
template <int NT, int KS, bool SAVE>
__global__ __launch_bounds__(kThreads) void fwd_kernel(FwdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int KR = KS > 0 ? KS : 1;
    const int H = a.d.H, B = a.B, L = a.d.L;
    const int64_t T = a.T, N = (int64_t)B * T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int ldh = H + 4;
    const int kmax = max((a.d.in + 15) & ~15, H), ldx = kmax + 4;
    float *hs = lds;                  // [2][16][ldh]
    float *xs = lds + 2 * 16 * ldh;   // [2][16][ldx]
    const int ntiles = H >> 4;

    for (int li = 0; li < L; ++li) {
        const int l = (int)opaque(li);  // one set of layer pointers live at a time, read from the argument block
        const agx_lstm_layer &p = a.d.layer[l];
        const int K = l ? H : a.d.in, K16 = (K + 15) & ~15;
        float *sv = SAVE ? a.saved + saved_layer(N, H, l) : nullptr;
        float *out = (SAVE && l < L - 1) ? sv + 5 * N * H : a.y;
        const float *src = l == 0 ? a.x : (SAVE ? a.saved + saved_layer(N, H, l - 1) + 5 * N * H : a.y);
        const bool vec_ih = (K & 3) == 0 && aligned16(p.w_ih);
        const bool vec_hh = aligned16(p.w_hh);
        const float *h0 = a.h0 + (int64_t)l * B * H, *c0 = a.c0 + (int64_t)l * B * H;

        // this wave's tiles: the two biases' sum, c_0, and (KS) the W_hh operands
        float bias[NT][4], c[NT][4];
        f32x4 wreg[4][KR];
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            const int unit = min((wave + kWaves * m) * 16 + r, H - 1);
#pragma unroll
            for (int g = 0; g < 4; ++g) bias[m][g] = p.b_ih[g * H + unit] + p.b_hh[g * H + unit];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = b0 + 4 * q + i;
                const float v = c0[(int64_t)min(row, B - 1) * H + unit];
                c[m][i] = row < B ? v : 0.f;
            }
        }
        if (KS > 0) {
            const int unit = min(wave * 16 + r, H - 1);
#pragma unroll
            for (int g = 0; g < 4; ++g)
#pragma unroll
                for (int s = 0; s < KR; ++s)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int k = 16 * s + 4 * q + j;
                        const float v = p.w_hh[((int64_t)g * H + unit) * H + min(k, H - 1)];
                        wreg[g][s][j] = k < H ? v : 0.f;
                    }
        }
        {
            const int rr = threadIdx.x >> 5, cc = threadIdx.x & 31;
            const float *hp = h0 + (int64_t)min(b0 + rr, B - 1) * H;
            for (int k = cc; k < H; k += 32) {
                const float v = hp[k];
                hs[rr * ldh + k] = b0 + rr < B ? v : 0.f;
            }
        }
        stage_step(xs, ldx, src, B, T, 0, K, K16, b0);

        for (int64_t ti = 0; ti < T; ++ti) {
            __syncthreads();
            const int64_t t = opaque(ti);
            const int cur = (int)(t & 1);
            const float *xrow = xs + cur * 16 * ldx + r * ldx;
            const float *hrow = hs + cur * 16 * ldh + r * ldh;
            float *hnext = hs + (cur ^ 1) * 16 * ldh;
#pragma unroll
            for (int m = 0; m < NT; ++m) {
                const int tile = wave + kWaves * m;
                if (tile < ntiles) {
                    const int unit = opaque_lane(tile * 16 + r);
                    f32x4 acc[4];
#pragma unroll
                    for (int g = 0; g < 4; ++g) acc[g] = f32x4{bias[m][g], bias[m][g], bias[m][g], bias[m][g]};
                    const float *wi = p.w_ih + (int64_t)unit * K;
                    if (vec_ih)
                        gates_vec<2>(K, q, acc, xrow, wi, (int64_t)H * K);
                    else
                        gates_any(K, q, acc, xrow, wi, (int64_t)H * K);
                    if (KS > 0) {
#pragma unroll
                        for (int s = 0; s < KR; ++s)
                            if (16 * s < H) {
                                const f32x4 av = *reinterpret_cast<const f32x4 *>(hrow + 16 * s + 4 * q);
#pragma unroll
                                for (int j = 0; j < 4; ++j)
#pragma unroll
                                    for (int g = 0; g < 4; ++g) acc[g] = MFMA(av[j], wreg[g][s][j], acc[g]);
                            }
                    } else {
                        const float *wh = p.w_hh + (int64_t)unit * H;
                        if (vec_hh)
                            gates_vec<2>(H, q, acc, hrow, wh, (int64_t)H * H);
                        else
                            gates_any(H, q, acc, hrow, wh, (int64_t)H * H);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float ig = sigm(acc[0][i]), fg = sigm(acc[1][i]), gg = tanhf(acc[2][i]),
                                    og = sigm(acc[3][i]);
                        const float cv = fg * c[m][i] + ig * gg;
                        const float hv = og * tanhf(cv);
                        c[m][i] = cv;
                        hnext[(4 * q + i) * ldh + unit] = hv;
                        const int row = b0 + 4 * q + i;
                        if (row < B) {
                            const int64_t n = (int64_t)row * T + t;
                            out[n * H + unit] = hv;
                            if (SAVE) {
                                float *gp = sv + n * 4 * H + unit;
                                gp[0] = ig;
                                gp[H] = fg;
                                gp[2 * H] = gg;
                                gp[3 * H] = og;
                                sv[4 * N * H + n * H + unit] = cv;
                            }
                            if (t == T - 1) {
                                a.hn[((int64_t)l * B + row) * H + unit] = hv;
                                a.cn[((int64_t)l * B + row) * H + unit] = cv;
                            }
                        }
                    }
                }
            }
            if (t + 1 < T) stage_step(xs + (cur ^ 1) * 16 * ldx, ldx, src, B, T, t + 1, K, K16, b0);
        }
        __syncthreads();  // the layer's output and both tiles are free before the next layer starts
    }
}

// ---------------------------------------------------------------------------
struct ScanArgs {
    const float *w_hh;           // [4H][H]
    const float *G, *C;          // the forward's gates [N][4H] and c [N][H]
    const float *c0;             // [B][H]
    const float *gy;             // [N][H]
    const float *ghn, *gcn;      // [B][H] or null
    float *dG;                   // [N][4H]
    float *gh0, *gc0;            // [B][H] or null
    int B, H;
    int64_t T;
};

template <int NT, int KS>
__global__ __launch_bounds__(kThreads) void bwd_scan_kernel(ScanArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int KR = KS > 0 ? KS : 1;
    const int H = a.H, B = a.B, H4 = 4 * a.H;
    const int64_t T = a.T;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * 16;
    const int ldg = H4 + 4;
    float *dgs = lds;  // [16][ldg]
    const int ntiles = H >> 4;

    float dh[NT][4], dc[NT][4];
    float wreg[4 * KR][4];  // W_hh[16 s + 4 q + j][unit], s < 4 KS
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        const int unit = min((wave + kWaves * m) * 16 + r, H - 1);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = b0 + 4 * q + i;
            const bool ok = row < B;
            dh[m][i] = (ok && a.ghn) ? a.ghn[(int64_t)row * H + unit] : 0.f;
            dc[m][i] = (ok && a.gcn) ? a.gcn[(int64_t)row * H + unit] : 0.f;
        }
    }
    if (KS > 0) {
        const int unit = min(wave * 16 + r, H - 1);
#pragma unroll
        for (int s = 0; s < 4 * KR; ++s)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = 16 * s + 4 * q + j;
                const float v = a.w_hh[(int64_t)min(k, H4 - 1) * H + unit];
                wreg[s][j] = k < H4 ? v : 0.f;
            }
    }

    for (int64_t ti = T - 1; ti >= 0; --ti) {
        const int64_t t = opaque(ti);
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            const int tile = wave + kWaves * m;
            if (tile < ntiles) {
                const int unit = tile * 16 + r;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int row = b0 + 4 * q + i;
                    float dai = 0.f, daf = 0.f, dag = 0.f, dao = 0.f;
                    if (row < B) {
                        const int64_t n = (int64_t)row * T + t;
                        const float *gp = a.G + n * H4 + unit;
                        const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
                        const float ct = a.C[n * H + unit];
                        const float cp = t > 0 ? a.C[(n - 1) * H + unit] : a.c0[(int64_t)row * H + unit];
                        const float dhv = dh[m][i] + a.gy[n * H + unit];
                        const float tc = tanhf(ct);
                        const float dcv = dc[m][i] + dhv * og * (1.f - tc * tc);
                        dao = dhv * tc * og * (1.f - og);
                        dai = dcv * gg * ig * (1.f - ig);
                        daf = dcv * cp * fg * (1.f - fg);
                        dag = dcv * ig * (1.f - gg * gg);
                        dc[m][i] = dcv * fg;
                        float *dp = a.dG + n * H4 + unit;
                        dp[0] = dai;
                        dp[H] = daf;
                        dp[2 * H] = dag;
                        dp[3 * H] = dao;
                    }
                    float *sp = dgs + (4 * q + i) * ldg + unit;
                    sp[0] = dai;
                    sp[H] = daf;
                    sp[2 * H] = dag;
                    sp[3 * H] = dao;
                }
            }
        }
        __syncthreads();
        const float *arow = dgs + r * ldg;
#pragma unroll
        for (int m = 0; m < NT; ++m) {
            const int tile = wave + kWaves * m;
            if (tile < ntiles) {
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (KS > 0) {
#pragma unroll
                    for (int s = 0; s < 4 * KR; ++s)
                        if (16 * s < H4) {
                            const f32x4 av = *reinterpret_cast<const f32x4 *>(arow + 16 * s + 4 * q);
#pragma unroll
                            for (int j = 0; j < 4; ++j) acc = MFMA(av[j], wreg[s][j], acc);
                        }
                } else {
                    acc = chain_col(H4, q, acc, arow, a.w_hh + tile * 16 + r, H);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) dh[m][i] = acc[i];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        const int tile = wave + kWaves * m;
        if (tile < ntiles) {
            const int unit = tile * 16 + r;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = b0 + 4 * q + i;
                if (row < B) {
                    if (a.gh0) a.gh0[(int64_t)row * H + unit] = dh[m][i];
                    if (a.gc0) a.gc0[(int64_t)row * H + unit] = dc[m][i];
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
struct DwArgs {
    const float *dG;         // [N][4H]
    const float *X;          // the layer's input [N][K]
    const float *hout, *h0;  // the layer's output [N][H] and initial state [B][H]: h_{t-1}
    float *gw_ih, *gw_hh, *gb_ih, *gb_hh;
    int K, H;
    int64_t T, N;
};

__global__ __launch_bounds__(kThreads) void dw_kernel(DwArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int H = a.H, K = a.K, H4 = 4 * a.H;
    const int tx = (K + 15) >> 4, th = H >> 4;
    const int tile = blockIdx.y * kWaves + wave;
    if (tile > tx + th) return;
    const int kind = tile < tx ? 0 : tile < tx + th ? 1 : 2;  // dW_ih, dW_hh, db
    const int col = kind == 0 ? min(tile * 16 + r, K - 1) : kind == 1 ? (tile - tx) * 16 + r : 0;
    const int j0 = blockIdx.x * 16;
    const float *gcol = a.dG + j0 + r;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t n0 = 0; n0 < a.N; n0 += 64) {
        float g[16], w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int64_t n = n0 + 16 * (u >> 2) + 4 * q + (u & 3);
            const bool ok = n < a.N;
            const int64_t nn = ok ? n : a.N - 1;
            g[u] = ok ? gcol[nn * H4] : 0.f;
            if (kind == 0) {
                w[u] = a.X[nn * K + col];
            } else if (kind == 1) {
                const int64_t b = nn / a.T;
                w[u] = nn - b * a.T > 0 ? a.hout[(nn - 1) * H + col] : a.h0[b * H + col];
            } else {
                w[u] = 1.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (n0 + 16 * (u >> 2) < a.N) acc = MFMA(g[u], w[u], acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = j0 + 4 * q + i;
        if (kind == 0) {
            if (tile * 16 + r < K) a.gw_ih[(int64_t)j * K + col] = acc[i];
        } else if (kind == 1) {
            a.gw_hh[(int64_t)j * H + col] = acc[i];
        } else if (r == 0) {
            a.gb_ih[j] = acc[i];
            a.gb_hh[j] = acc[i];
        }
    }
}

struct DxArgs {
    const float *dG, *w_ih;  // [N][4H], [4H][K]
    float *dX;               // [N][K]
    int K, H;
    int64_t N;
};

__global__ __launch_bounds__(kThreads) void dx_kernel(DxArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int K = a.K, H4 = 4 * a.H, ldg = H4 + 4;
    const int64_t n0 = (int64_t)blockIdx.x * 16;
    {
        const int rr = threadIdx.x >> 5, cc = threadIdx.x & 31;
        const bool ok = n0 + rr < a.N;
        const float *p = a.dG + (ok ? n0 + rr : 0) * H4;
        for (int k = cc; k < H4; k += 32) lds[rr * ldg + k] = ok ? p[k] : 0.f;
    }
    __syncthreads();
    const int tk = (K + 15) >> 4;
    for (int kt = wave; kt < tk; kt += kWaves) {
        const int col = kt * 16 + r;
        const f32x4 acc = chain_col(H4, q, f32x4{0.f, 0.f, 0.f, 0.f}, lds + r * ldg, a.w_ih + min(col, K - 1), K);
        if (col < K) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int64_t n = n0 + 4 * q + i;
                if (n < a.N) a.dX[n * K + col] = acc[i];
            }
        }
    }
}

// ---------------------------------------------------------------------------
constexpr int kLdsCap = 160 * 1024;  // gfx950's LDS; the forward at in = H = 512 stages 129 KB, the scans 128.1 KB

static size_t fwd_lds(int in, int H) {
    const int kmax = ((in + 15) & ~15) > H ? ((in + 15) & ~15) : H;
    return ((size_t)2 * 16 * (H + 4) + (size_t)2 * 16 * (kmax + 4)) * sizeof(float);
}

static size_t scan_lds(int H) { return (size_t)16 * (4 * H + 4) * sizeof(float); }

// the instantiation of a width: W_hh in registers up to AGX_LSTM_RESIDENT_H (KS = 2, 4: H <= 32, 64), streamed above
// it with 1, 2 or 4 unit tiles per wave (H <= 128, 256, 512)
#define AGX_LSTM_WIDTHS(X, ...)                      \
    do {                                             \
        if (H <= 32) X(1, 2, __VA_ARGS__);           \
        else if (H <= AGX_LSTM_RESIDENT_H) X(1, 4, __VA_ARGS__); \
        else if (H <= 128) X(1, 0, __VA_ARGS__);     \
        else if (H <= 256) X(2, 0, __VA_ARGS__);     \
        else X(4, 0, __VA_ARGS__);                   \
    } while (0)

static void allow_lds() {
    static const bool once = [] {
#define AGX_LSTM_ALLOW(NT, KS, unused)                                                                             \
    (void)hipFuncSetAttribute((const void *)fwd_kernel<NT, KS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                              kLdsCap);                                                                            \
    (void)hipFuncSetAttribute((const void *)fwd_kernel<NT, KS, true>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                              kLdsCap);                                                                            \
    (void)hipFuncSetAttribute((const void *)bwd_scan_kernel<NT, KS>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap)
        AGX_LSTM_ALLOW(1, 2, 0);
        AGX_LSTM_ALLOW(1, 4, 0);
        AGX_LSTM_ALLOW(1, 0, 0);
        AGX_LSTM_ALLOW(2, 0, 0);
        AGX_LSTM_ALLOW(4, 0, 0);
#undef AGX_LSTM_ALLOW
        (void)hipFuncSetAttribute((const void *)dx_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap);
        return true;
    }();
    (void)once;
}

// ---------------------------------------------------------------------------
int check_dims(const agx_lstm_desc *d, int64_t B, int64_t T, const char *who) {
    AGX_REQUIRE(d, "%s: descriptor is NULL", who);
    AGX_REQUIRE(d->L >= 1 && d->L <= AGX_LSTM_MAX_LAYERS, "%s: %d layers outside [1, %d]", who, d->L,
                AGX_LSTM_MAX_LAYERS);
    AGX_REQUIRE(d->H >= 16 && d->H <= AGX_LSTM_MAX_HIDDEN && d->H % 16 == 0,
                "%s: hidden size %d is not a multiple of 16 in [16, %d]", who, d->H, AGX_LSTM_MAX_HIDDEN);
    AGX_REQUIRE(d->in >= 1 && d->in <= AGX_LSTM_MAX_INPUT, "%s: input size %d outside [1, %d]", who, d->in,
                AGX_LSTM_MAX_INPUT);
    AGX_REQUIRE(B >= 1 && T >= 1, "%s: B %lld, T %lld must be positive", who, (long long)B, (long long)T);
    AGX_REQUIRE(B <= (1 << 24) && T <= (1 << 24) && B * T <= (1 << 24), "%s: B %lld * T %lld above 2^24 rows", who,
                (long long)B, (long long)T);
    return AGX_OK;
}

int check_desc(const agx_lstm_desc *d, int64_t B, int64_t T, bool backward, const char *who) {
    if (int rc = check_dims(d, B, T, who)) return rc;
    for (int l = 0; l < d->L; ++l) {
        const agx_lstm_layer &p = d->layer[l];
        AGX_REQUIRE(p.w_ih && p.w_hh && p.b_ih && p.b_hh, "%s: layer %d: a parameter is NULL", who, l);
        AGX_REQUIRE(!backward || (p.g_w_ih && p.g_w_hh && p.g_b_ih && p.g_b_hh),
                    "%s: layer %d: a gradient output is NULL", who, l);
    }
    return AGX_OK;
}

int launch_dw_dx(const agx_lstm_layer &p, const float *dG, const float *xin, const float *hout, const float *h0, float *dX,
                 int K, int H, int64_t T, int64_t N, hipStream_t s, const char *who) {
    allow_lds();
    const dim3 block(kThreads);
    DwArgs wa{dG, xin, hout, h0, p.g_w_ih, p.g_w_hh, p.g_b_ih, p.g_b_hh, K, H, T, N};
    const int tiles = (K + 15) / 16 + H / 16 + 1;
    hipLaunchKernelGGL(dw_kernel, dim3(4 * H / 16, (unsigned)ceil_div(tiles, kWaves)), block, 0, s, wa);
    if (int rc = check_launch(who)) return rc;
    if (dX) {
        DxArgs xa{dG, p.w_ih, dX, K, H, N};
        hipLaunchKernelGGL(dx_kernel, dim3((unsigned)ceil_div(N, 16)), block, scan_lds(H), s, xa);
        if (int rc = check_launch(who)) return rc;
    }
    return AGX_OK;
}

}  // namespace lstm

using lstm::check_desc;
using lstm::check_dims;

extern "C" size_t agx_lstm_saved_bytes(const agx_lstm_desc *d, int64_t B, int64_t T) {
    if (check_dims(d, B, T, "agx_lstm_saved_bytes")) return 0;
    return (size_t)(B * T) * d->H * (6 * d->L - 1) * sizeof(float);
}

extern "C" size_t agx_lstm_workspace_bytes(const agx_lstm_desc *d, int64_t B, int64_t T) {
    if (check_dims(d, B, T, "agx_lstm_workspace_bytes")) return 0;
    return (size_t)(B * T) * d->H * (d->L > 1 ? 5 : 4) * sizeof(float);
}

extern "C" int agx_lstm_forward(const agx_lstm_desc *d, const float *x, const float *h0, const float *c0, int64_t B,
                                int64_t T, float *y, float *h_n, float *c_n, void *saved, void *stream) {
    const char *who = "agx_lstm_forward";
    if (int rc = check_desc(d, B, T, false, who)) return rc;
    AGX_REQUIRE(x && h0 && c0 && y && h_n && c_n, "%s: an input or output is NULL", who);
    lstm::allow_lds();
    lstm::FwdArgs a{*d, x, h0, c0, y, h_n, c_n, static_cast<float *>(saved), (int)B, T};
    const int H = d->H;
    const dim3 grid((unsigned)ceil_div(B, 16));
    const size_t lds = lstm::fwd_lds(d->in, H);
    hipStream_t s = as_stream(stream);
#define AGX_LSTM_FWD(NT, KS, unused)                                                                \
    do {                                                                                            \
        if (saved)                                                                                  \
            hipLaunchKernelGGL((lstm::fwd_kernel<NT, KS, true>), grid, dim3(lstm::kThreads), lds, s, a);  \
        else                                                                                        \
            hipLaunchKernelGGL((lstm::fwd_kernel<NT, KS, false>), grid, dim3(lstm::kThreads), lds, s, a); \
    } while (0)
    AGX_LSTM_WIDTHS(AGX_LSTM_FWD, 0);
#undef AGX_LSTM_FWD
    return check_launch(who);
}

extern "C" int agx_lstm_backward(const agx_lstm_desc *d, const float *x, const float *h0, const float *c0, int64_t B,
                                 int64_t T, const float *y, const void *saved, const float *gy, const float *gh_n,
                                 const float *gc_n, float *gx, float *gh0, float *gc0, void *workspace, void *stream) {
    const char *who = "agx_lstm_backward";
    if (int rc = check_desc(d, B, T, true, who)) return rc;
    AGX_REQUIRE(x && h0 && c0 && y && saved && gy && workspace, "%s: an input, saved tensor or the workspace is NULL",
                who);
    lstm::allow_lds();
    const int H = d->H, L = d->L;
    const int64_t N = B * T, BH = B * H;
    const float *sv = static_cast<const float *>(saved);
    float *dG = static_cast<float *>(workspace), *dY = dG + 4 * N * H;
    hipStream_t s = as_stream(stream);
    for (int l = L - 1; l >= 0; --l) {
        const agx_lstm_layer &p = d->layer[l];
        const float *svl = sv + lstm::saved_layer(N, H, l);
        const float *hout = l == L - 1 ? y : svl + 5 * N * H;
        const float *xin = l == 0 ? x : sv + lstm::saved_layer(N, H, l - 1) + 5 * N * H;
        const int K = l == 0 ? d->in : H;
        lstm::ScanArgs sa{p.w_hh, svl, svl + 4 * N * H, c0 + l * BH, l == L - 1 ? gy : dY,
                          gh_n ? gh_n + l * BH : nullptr, gc_n ? gc_n + l * BH : nullptr, dG,
                          gh0 ? gh0 + l * BH : nullptr, gc0 ? gc0 + l * BH : nullptr, (int)B, H, T};
        const dim3 sgrid((unsigned)ceil_div(B, 16));
        const size_t slds = lstm::scan_lds(H);
#define AGX_LSTM_SCAN(NT, KS, unused) hipLaunchKernelGGL((lstm::bwd_scan_kernel<NT, KS>), sgrid, dim3(lstm::kThreads), slds, s, sa)
        AGX_LSTM_WIDTHS(AGX_LSTM_SCAN, 0);
#undef AGX_LSTM_SCAN
        if (int rc = check_launch(who)) return rc;
        if (int rc = lstm::launch_dw_dx(p, dG, xin, hout, h0 + l * BH, l == 0 ? gx : dY, K, H, T, N, s, who)) return rc;
    }
    return AGX_OK;
}

}  // namespace agx
