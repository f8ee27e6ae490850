// Stacked LSTM sequences, the split form (include/agx_lstm.h): a layer split by
// hidden unit across the device, one launch per time step, fp32 MFMA.
//
// The whole-sequence kernels (lstm.hip) give a workgroup a 16-row batch tile
// for the whole sequence: B = 128 fills 8 CUs, and above the register-resident
// widths each of them re-reads all of W_ih and W_hh from L2 every step.  Here
// the unit of work is a wave-task, one 16-unit tile x one 16-row batch tile,
// and the step boundary is the launch boundary: nothing waits on another
// workgroup, no sum is split, no atomics.  Every accumulator takes the whole
// kernels' chain (bias, k ascending over the input, k ascending over h, in the
// same 16-deep MFMA steps, through the same functions of lstm_gates.h), so the
// results have the whole kernels' bits.
//
// Forward of a layer, T + 1 launches:
//   xproj_kernel: P[n][4H] = (b_ih + b_hh) + x_n W_ih^T for all N = B T rows.
//     A workgroup owns 128 rows x one unit tile's 64 gate columns, a wave 16 of
//     the rows; the x tile and the W_ih tile pass through LDS in 64-deep k
//     chunks (16-byte row loads, leading dimension 68).  k is not split: the
//     chunks only bound what is staged.  P lies in the layer's gate region of
//     `saved` (the saving form) or in the workspace.
//   step_fwd_kernel, once per t: a workgroup is WV wave-tasks that share a unit
//     tile.  It stages that tile's 64 rows of W_hh and its WV h_{t-1} tiles
//     through LDS in 128-deep k chunks (leading dimension 132), so a weight
//     byte is read from L2 once per workgroup and step, coalesced.  The four
//     accumulators are loaded from P, run the h chain, and the cell update
//     happens in registers; c_t is carried in c_n between launches.
// Backward of a layer, T + 3 launches: step_bwd_kernel for t = T-1 .. 0 and a
//   tail, then lstm.hip's dw_kernel and dx_kernel over all N rows.  The launch
//   for t forms dh_t[:, units] = dG_{t+1} W_hh[:, units] (chain_col's order; A:
//   the dG rows of step t + 1 from the workspace, B: the 4H x 16 column slice
//   of W_hh, both through LDS in 128-deep chunks), adds gy, runs
//   bwd_scan_kernel's formulas, writes dG_t and updates dc in place in a
//   [B][H] buffer.  dh never leaves registers.  The tail does the chain only.
#include <cstdint>
#include <cstdlib>

#include "agx_common.h"
#include "lstm_gates.h"
#include "../../include/agx_lstm.h"

namespace agx {

namespace lstm {

namespace split {

constexpr int kProjKC = 64, kProjRows = 128, kProjThreads = 512;
constexpr int kStepKC = 128;
constexpr int kLdW = 17;  // the backward's W_hh column slice [k][16 + 1]: the four q groups of a read hit 4 banks apart

// dst [rows][KC + 4] <- KC floats of every row at row(i) (nullptr: a row of zeros), zeros from column klen on.
// vec: 16-byte loads (klen % 4 == 0, rows 16-byte aligned).
template <int KC, typename Row>
__device__ __forceinline__ void stage_rows(float *dst, int rows, int klen, bool vec, Row row) {
    constexpr int ld = KC + 4;
    if (vec) {  // four loads in flight per thread before their stores
        const int total = rows * (KC / 4), step = blockDim.x;
        for (int base = threadIdx.x; base < total; base += 4 * step) {
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * step, i = idx / (KC / 4), k = (idx % (KC / 4)) * 4;
                const float *p = idx < total ? row(i) : nullptr;
                v[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (p && k < klen) v[u] = *reinterpret_cast<const f32x4 *>(p + k);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * step, i = idx / (KC / 4), k = (idx % (KC / 4)) * 4;
                if (idx < total) *reinterpret_cast<f32x4 *>(dst + i * ld + k) = v[u];
            }
        }
    } else {
        for (int idx = threadIdx.x; idx < rows * KC; idx += blockDim.x) {
            const int i = idx / KC, k = idx % KC;
            const float *p = row(i);
            dst[i * ld + k] = (p && k < klen) ? p[k] : 0.f;
        }
    }
}

// ---------------------------------------------------------------------------
struct ProjArgs {
    const float *x, *w_ih, *b_ih, *b_hh;  // [N][K], [4H][K], [4H], [4H]
    float *P;                              // [N][4H]
    int K, H;
    int64_t N;
    int vec;
};

__global__ __launch_bounds__(kProjThreads) void xproj_kernel(ProjArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ld = kProjKC + 4;
    float *xs = lds;                    // [128][ld]
    float *ws = lds + kProjRows * ld;   // [64][ld]: row 16 g + u is W_ih[g H + u0 + u]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int K = a.K, H = a.H, K16 = (K + 15) & ~15;
    const int64_t n0 = (int64_t)blockIdx.x * kProjRows;
    const int u0 = blockIdx.y * 16, unit = u0 + r;
    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float b = a.b_ih[g * H + unit] + a.b_hh[g * H + unit];
        acc[g] = f32x4{b, b, b, b};
    }
    for (int k0 = 0; k0 < K16; k0 += kProjKC) {
        const int klen = min(kProjKC, K - k0), kpad = min(kProjKC, K16 - k0);
        __syncthreads();  // the chunk before has been read
        stage_rows<kProjKC>(xs, kProjRows, klen, a.vec, [&](int i) -> const float * {
            return n0 + i < a.N ? a.x + (n0 + i) * K + k0 : nullptr;
        });
        stage_rows<kProjKC>(ws, 64, klen, a.vec, [&](int i) -> const float * {
            return a.w_ih + ((int64_t)(i >> 4) * H + u0 + (i & 15)) * K + k0;
        });
        __syncthreads();
        gates_vec<2>(kpad, q, acc, xs + (wave * 16 + r) * ld, ws + r * ld, 16 * ld);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t n = n0 + wave * 16 + 4 * q + i;
        if (n < a.N) {
            float *pp = a.P + n * 4 * H + unit;
#pragma unroll
            for (int g = 0; g < 4; ++g) pp[g * H] = acc[g][i];
        }
    }
}

// ---------------------------------------------------------------------------
struct StepArgs {
    const float *w_hh;   // [4H][H]
    float *P;            // [N][4H]: the pre-activations so far; SAVE: overwritten by the gates
    const float *hprev;  // row b of h_{t-1} at hprev + b * hstride
    int64_t hstride;
    const float *cprev;  // [B][H]: c0 at t = 0, else cn
    float *out;          // the layer's output [N][H]
    float *C;            // SAVE: [N][H]
    float *hn, *cn;      // [B][H]; hn is written at t = T - 1, cn at every step
    int B, H;
    int64_t T, t;
    int vec;
};

template <bool SAVE>
__global__ __launch_bounds__(512) void step_fwd_kernel(StepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ld = kStepKC + 4;
    const int WV = blockDim.x >> 6;
    float *ws = lds;            // [64][ld]: row 16 g + u is W_hh[g H + u0 + u]
    float *hs = lds + 64 * ld;  // [16 WV][ld]
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int H = a.H, B = a.B;
    const int64_t T = a.T, t = a.t;
    const int64_t bg0 = (int64_t)blockIdx.x * WV * 16, b0 = bg0 + wave * 16;
    const int u0 = blockIdx.y * 16, unit = u0 + r;

    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = b0 + 4 * q + i;
        const float *pp = a.P + ((row < B ? row : B - 1) * T + t) * 4 * H + unit;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float v = pp[g * H];
            acc[g][i] = row < B ? v : 0.f;
        }
    }
    for (int k0 = 0; k0 < H; k0 += kStepKC) {
        const int klen = min(kStepKC, H - k0);
        __syncthreads();  // the chunk before has been read
        stage_rows<kStepKC>(ws, 64, klen, a.vec, [&](int i) -> const float * {
            return a.w_hh + ((int64_t)(i >> 4) * H + u0 + (i & 15)) * H + k0;
        });
        stage_rows<kStepKC>(hs, 16 * WV, klen, a.vec, [&](int i) -> const float * {
            return bg0 + i < B ? a.hprev + (bg0 + i) * a.hstride + k0 : nullptr;
        });
        __syncthreads();
        gates_vec<2>(klen, q, acc, hs + (wave * 16 + r) * ld, ws + r * ld, 16 * ld);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = b0 + 4 * q + i;
        if (row < B) {
            const float ig = sigm(acc[0][i]), fg = sigm(acc[1][i]), gg = tanhf(acc[2][i]), og = sigm(acc[3][i]);
            const float cv = fg * a.cprev[row * H + unit] + ig * gg;
            const float hv = og * tanhf(cv);
            const int64_t n = row * T + t;
            a.out[n * H + unit] = hv;
            a.cn[row * H + unit] = cv;
            if (SAVE) {
                float *gp = a.P + n * 4 * H + unit;
                gp[0] = ig;
                gp[H] = fg;
                gp[2 * H] = gg;
                gp[3 * H] = og;
                a.C[n * H + unit] = cv;
            }
            if (t == T - 1) a.hn[row * H + unit] = hv;
        }
    }
}

// ---------------------------------------------------------------------------
struct BStepArgs {
    const float *w_hh;       // [4H][H]
    const float *G, *C;      // the forward's gates [N][4H] and c [N][H]
    const float *c0;         // [B][H]
    const float *gy;         // [N][H]
    const float *ghn, *gcn;  // [B][H] or null
    float *dG;               // [N][4H]
    float *dc;               // [B][H]: dc_{t+1} f_{t+1} in, dc_t f_t out
    float *gh0, *gc0;        // [B][H] or null (the tail's outputs)
    int B, H;
    int64_t T, t;            // t == -1: the tail
    int vec;
};

__global__ __launch_bounds__(512) void step_bwd_kernel(BStepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    constexpr int ld = kStepKC + 4;
    const int WV = blockDim.x >> 6;
    static_assert(kStepKC * kLdW % 4 == 0, "the dG tile behind the weight slice stays 16-byte aligned");
    float *wt = lds;                     // [128][kLdW]: W_hh[k0 + k][u0 + u]
    float *as = lds + kStepKC * kLdW;    // [16 WV][ld]: rows of dG_{t+1}
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int H = a.H, B = a.B, H4 = 4 * a.H;
    const int64_t T = a.T, t = a.t;
    const int64_t bg0 = (int64_t)blockIdx.x * WV * 16, b0 = bg0 + wave * 16;
    const int u0 = blockIdx.y * 16, unit = u0 + r;
    const bool first = t == T - 1;

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (!first) {
        for (int k0 = 0; k0 < H4; k0 += kStepKC) {
            const int klen = min(kStepKC, H4 - k0);  // a multiple of 64
            __syncthreads();  // the chunk before has been read
            stage_rows<kStepKC>(as, 16 * WV, klen, a.vec, [&](int i) -> const float * {
                return bg0 + i < B ? a.dG + ((bg0 + i) * T + t + 1) * H4 + k0 : nullptr;
            });
            for (int idx = threadIdx.x; idx < klen * 4; idx += blockDim.x) {
                const int k = idx >> 2, c = (idx & 3) * 4;
                const float *p = a.w_hh + (int64_t)(k0 + k) * H + u0 + c;
                f32x4 v;
                if (a.vec) {
                    v = *reinterpret_cast<const f32x4 *>(p);
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = p[j];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) wt[k * kLdW + c + j] = v[j];
            }
            __syncthreads();
            acc = chain_col(klen, q, acc, as + (wave * 16 + r) * ld, wt + r, kLdW);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t row = b0 + 4 * q + i;
        if (row >= B) continue;
        const int64_t e = row * H + unit;
        if (t < 0) {
            if (a.gh0) a.gh0[e] = acc[i];
            if (a.gc0) a.gc0[e] = a.dc[e];
            continue;
        }
        const float dh = first ? (a.ghn ? a.ghn[e] : 0.f) : acc[i];
        const float dcn = first ? (a.gcn ? a.gcn[e] : 0.f) : a.dc[e];
        const int64_t n = row * T + t;
        const float *gp = a.G + n * H4 + unit;
        const float ig = gp[0], fg = gp[H], gg = gp[2 * H], og = gp[3 * H];
        const float ct = a.C[n * H + unit];
        const float cp = t > 0 ? a.C[(n - 1) * H + unit] : a.c0[e];
        const float dhv = dh + a.gy[n * H + unit];
        const float tc = tanhf(ct);
        const float dcv = dcn + dhv * og * (1.f - tc * tc);
        float *dp = a.dG + n * H4 + unit;
        dp[3 * H] = dhv * tc * og * (1.f - og);
        dp[0] = dcv * gg * ig * (1.f - ig);
        dp[H] = dcv * cp * fg * (1.f - fg);
        dp[2 * H] = dcv * ig * (1.f - gg * gg);
        a.dc[e] = dcv * fg;
    }
}

// ---------------------------------------------------------------------------
static size_t proj_lds() { return (size_t)(kProjRows + 64) * (kProjKC + 4) * sizeof(float); }
static size_t fwd_lds(int wv) { return (size_t)(64 + 16 * wv) * (kStepKC + 4) * sizeof(float); }
static size_t bwd_lds(int wv) {
    return ((size_t)kStepKC * kLdW + (size_t)16 * wv * (kStepKC + 4)) * sizeof(float);
}

static void allow_lds() {
    static const bool once = [] {
        const int cap = (int)(fwd_lds(8) > bwd_lds(8) ? fwd_lds(8) : bwd_lds(8));
        (void)hipFuncSetAttribute((const void *)step_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        (void)hipFuncSetAttribute((const void *)step_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        (void)hipFuncSetAttribute((const void *)step_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, cap);
        return true;
    }();
    (void)once;
}

// Wave-tasks per workgroup: 4, the fastest of 2 / 4 / 8 in every measured cell (more waves stage the
// shared weight slice faster and re-read it less, fewer leave more workgroups for the device).
// AGX_LSTM_SPLIT_WAVES=2|4|8 overrides it for measurements; the results do not depend on it.
static int pick_waves() {
    if (const char *e = getenv("AGX_LSTM_SPLIT_WAVES")) {
        const int v = atoi(e);
        if (v == 2 || v == 4 || v == 8) return v;
    }
    return 4;
}

static bool al16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace split

}  // namespace lstm

// ---------------------------------------------------------------------------
// The measured bound (tools/lstm_time.py -> profiles/lstm_time.json): at the measured widths from
// here up (256, 512) the split form's slowest block lay below the whole form's fastest in every sequence cell; at
// 144 it did not in two of sixteen (fwd+bwd, one layer, B = 128), at 128 in none of the fwd+bwd cells.
#define AGX_LSTM_SPLIT_MIN_H 256

extern "C" int agx_lstm_choose_plan(const agx_lstm_desc *d, int64_t B, int64_t T, int32_t *split) {
    AGX_REQUIRE(split, "agx_lstm_choose_plan: split is NULL");
    if (int rc = lstm::check_dims(d, B, T, "agx_lstm_choose_plan")) return rc;
    *split = d->H >= AGX_LSTM_SPLIT_MIN_H;
    return AGX_OK;
}

extern "C" size_t agx_lstm_split_workspace_bytes(const agx_lstm_desc *d, int64_t B, int64_t T, int backward) {
    if (lstm::check_dims(d, B, T, "agx_lstm_split_workspace_bytes")) return 0;
    const size_t NH = (size_t)(B * T) * d->H;
    return (backward ? NH * (d->L > 1 ? 5 : 4) + (size_t)B * d->H : NH * 4) * sizeof(float);
}

extern "C" int agx_lstm_forward_split(const agx_lstm_desc *d, const float *x, const float *h0, const float *c0,
                                      int64_t B, int64_t T, float *y, float *h_n, float *c_n, void *saved,
                                      void *workspace, void *stream) {
    using namespace lstm::split;
    const char *who = "agx_lstm_forward_split";
    if (int rc = lstm::check_desc(d, B, T, false, who)) return rc;
    AGX_REQUIRE(x && h0 && c0 && y && h_n && c_n, "%s: an input or output is NULL", who);
    AGX_REQUIRE(workspace, "%s: the workspace is NULL", who);
    allow_lds();
    const int H = d->H, L = d->L;
    const int64_t N = B * T, BH = B * H;
    float *sv = static_cast<float *>(saved);
    hipStream_t s = as_stream(stream);
    const int wv = pick_waves();
    const dim3 sgrid((unsigned)ceil_div(B, 16 * wv), H / 16), sblock(64 * wv);
    for (int l = 0; l < L; ++l) {
        const agx_lstm_layer &p = d->layer[l];
        const int K = l ? H : d->in;
        float *svl = sv ? sv + lstm::saved_layer(N, H, l) : nullptr;
        float *P = sv ? svl : static_cast<float *>(workspace);
        float *out = (sv && l < L - 1) ? svl + 5 * N * H : y;
        const float *src = l == 0 ? x : (sv ? sv + lstm::saved_layer(N, H, l - 1) + 5 * N * H : y);
        ProjArgs pa{src, p.w_ih, p.b_ih, p.b_hh, P, K, H, N, (K & 3) == 0 && al16(src) && al16(p.w_ih)};
        hipLaunchKernelGGL(xproj_kernel, dim3((unsigned)ceil_div(N, kProjRows), H / 16), dim3(kProjThreads), proj_lds(),
                           s, pa);
        if (int rc = check_launch(who)) return rc;
        const int vec = al16(p.w_hh) && al16(h0) && al16(out);
        for (int64_t t = 0; t < T; ++t) {
            StepArgs sa{p.w_hh, P, t ? out + (t - 1) * H : h0 + l * BH, t ? T * H : H, t ? c_n + l * BH : c0 + l * BH,
                        out, sv ? svl + 4 * N * H : nullptr, h_n + l * BH, c_n + l * BH, (int)B, H, T, t, vec};
            if (sv)
                hipLaunchKernelGGL(step_fwd_kernel<true>, sgrid, sblock, fwd_lds(wv), s, sa);
            else
                hipLaunchKernelGGL(step_fwd_kernel<false>, sgrid, sblock, fwd_lds(wv), s, sa);
            if (int rc = check_launch(who)) return rc;
        }
    }
    return AGX_OK;
}

extern "C" int agx_lstm_backward_split(const agx_lstm_desc *d, const float *x, const float *h0, const float *c0,
                                       int64_t B, int64_t T, const float *y, const void *saved, const float *gy,
                                       const float *gh_n, const float *gc_n, float *gx, float *gh0, float *gc0,
                                       void *workspace, void *stream) {
    using namespace lstm::split;
    const char *who = "agx_lstm_backward_split";
    if (int rc = lstm::check_desc(d, B, T, true, who)) return rc;
    AGX_REQUIRE(x && h0 && c0 && y && saved && gy && workspace, "%s: an input, saved tensor or the workspace is NULL",
                who);
    allow_lds();
    const int H = d->H, L = d->L;
    const int64_t N = B * T, BH = B * H;
    const float *sv = static_cast<const float *>(saved);
    float *dG = static_cast<float *>(workspace), *dY = dG + 4 * N * H;
    float *dc = dG + (L > 1 ? 5 : 4) * N * H;
    hipStream_t s = as_stream(stream);
    const int wv = pick_waves();
    const dim3 sgrid((unsigned)ceil_div(B, 16 * wv), H / 16), sblock(64 * wv);
    for (int l = L - 1; l >= 0; --l) {
        const agx_lstm_layer &p = d->layer[l];
        const float *svl = sv + lstm::saved_layer(N, H, l);
        const float *hout = l == L - 1 ? y : svl + 5 * N * H;
        const float *xin = l == 0 ? x : sv + lstm::saved_layer(N, H, l - 1) + 5 * N * H;
        const int K = l == 0 ? d->in : H;
        const int vec = al16(p.w_hh) && al16(dG);
        const bool tail = gh0 || gc0;
        for (int64_t t = T - 1; t >= (tail ? -1 : 0); --t) {
            BStepArgs ba{p.w_hh, svl, svl + 4 * N * H, c0 + l * BH, l == L - 1 ? gy : dY,
                         gh_n ? gh_n + l * BH : nullptr, gc_n ? gc_n + l * BH : nullptr, dG, dc,
                         gh0 ? gh0 + l * BH : nullptr, gc0 ? gc0 + l * BH : nullptr, (int)B, H, T, t, vec};
            hipLaunchKernelGGL(step_bwd_kernel, sgrid, sblock, bwd_lds(wv), s, ba);
            if (int rc = check_launch(who)) return rc;
        }
        if (int rc = lstm::launch_dw_dx(p, dG, xin, hout, h0 + l * BH, l == 0 ? gx : dY, K, H, T, N, s, who)) return rc;
    }
    return AGX_OK;
}

}  // namespace agx
