// The runtime layer list (include/agx_graph.h) that the runtime-shape learner
// (graph_learner.hip) and the runtime-shape policy step / rollout / evaluation
// (graph_rollout.hip) both interpret: the layer table and its plans, the
// C = A . B^T GEMM, and the forward in its two forms, over global scratch
// (forward_layers) and over 16-row LDS tiles (few_forward).
#pragma once

#include <cmath>
#include <cstdlib>

#include "agx_common.h"
#include "../../include/agx_graph.h"

namespace agx {
namespace {

constexpr int kGT = 256;  // 4 waves, one per SIMD: the whole 512-VGPR file per wave
constexpr int kGW = kGT / kWave;
constexpr int kGL = AGX_PPO_GRAPH_MAX_LAYERS;
constexpr size_t kLdsMax = 160 * 1024;  // LDS per CU (gfx950)

struct GLay {
    int fin, fout, w, b, g, be, ln, relu, src;
    int acc;  // dX goes to the source's second dY buffer (a consumer processed earlier wrote the first)
    // per-agent scratch offsets (floats; -1: not kept): output row-major,
    // output feature-major, xhat, rstd, d(output), d(output) from a second
    // consumer (the latent feeding both heads: the row pass adds the two),
    // transposed weight
    long long yr, yc, xh, rs, dy, dy2, wt;
    long long dyc;  // output layers: d(output) feature-major, written by the loss pass (-1 otherwise)
    int fuse;       // this layer's dX GEMM runs its source's LayerNorm / ReLU backward in the epilogue
    int fused;      // this layer's dZ (and column partials) come from its consumer's dX epilogue
    int ld;         // few-row form: the row stride of the layer's LDS tiles
    long long af;   // few-row form: the LN affine (gamma then beta) copied to LDS, -1: none
};

struct GArgs {
    GLay L[kGL];
    int nl, aout, cout, A, D, n, cstart, bp;
    long long oc, dzr, dzc, dzr1, dzc1, t1, t2, gr, ws_agent;  // dZ buffers by layer parity
    // partnered learner (ppo_learn_graph_part_kernel): K workgroups per agent,
    // R rows of each minibatch per partner; agent stride Q of the block index
    long long ws_part, wt0, wt_agent;  // a partner's scratch, the transposed weights' plan offset / size
    int K, R, Q;
    long long nslab;       // floats per exchange slab: gradient row, loss chunk, partial norms
    float *slabs, *sums;   // [P][2][K][nslab] partial gradients, [P][2][nslab] summed gradients
    float *wtb;            // [P][wt_agent] transposed weights shared by an agent's partners
    unsigned *cnt;         // barrier counters, timeout word, XCC ids (zeroed by the gather)
    unsigned *err;         // caller's sticky error word
    int write_through;     // test hook: the cross-XCD (release-fence) publish form always
    int ld0;               // few-row form: the observation tile's row stride (its offset: oc)
    long long lds_floats;  // few-row form: the LDS tiles' size (dynamic LDS)
    long long *stamps;     // diagnostic phase stamps of the partnered learner (agx_debug_graph_stamps), or null
    float *ws;
    float *params, *m, *v;
    const float *lr;
    float b1, b2, eps;
    long long *step;
    const float *gobs;
    const int *gact;
    const unsigned *gmask;
    const float *grow;
    long long S;
    int E, B, P;
    float clip, vf, ent, max_norm;
    double target_kl;
    const int *batch_p, *epochs_p;
    const float *ent_p;
    float *loss_out, *kl_out;
    int *epochs_out;
    const unsigned *skip;
    int dbg;  // diagnostic phase skips (AGX_GRAPH_DEBUG; timing attribution only, results wrong)
    long long lso;  // Gaussian head: the A log_std floats in the parameter row (gact: float [..][A])
    // multi-categorical head (agx_multi.h): mk components, component k's size in byte k & 3 of
    // mn[k >> 2] (gact: one target word per row, bit off_k + a_k set for every component)
    int mk;
    unsigned mn[AGX_PPO_GRAPH_MAX_ACTIONS / 4];
};

// C[M x N] = A[M x K] . B[N x K]^T, both operands contiguous along k (the
// only operand form the learner needs, see graph_learner.hip), in blocks of
// up to 128 x 128.  The block's A and B panels go through LDS 32 k at a time,
// double-buffered: every global load is a dword load of 64 consecutive lanes
// over 2 rows x 32 contiguous k (two full 128-byte lines), and the next
// chunk's loads fly under the current chunk's MFMAs.  Each wave owns up to 8
// of the block's 16x16 f32 MFMA tiles; MFMA kk takes k = 4kk + q from lane
// group q (LDS rows padded to 36 floats: the 64 lanes' reads hit 64 banks).
// lds: kGemmLds floats.  epi(m, n, c) per element.
constexpr int kBM = 128, kBN = 64, kKC = 32, kLdS = kKC + 4;
constexpr int kRS = kGT / kKC;                           // staging row stride
constexpr int kTPW = (kBM / 16) * (kBN / 16) / kGW;      // tiles per wave
constexpr int kPanel = (kBM + kBN) * kLdS;  // A rows then B rows
constexpr int kGemmLds = 2 * kPanel;        // double-buffered

// LNE: the forward of a layer at most kBN = 64 wide with its LayerNorm(+affine)
// / ReLU in the epilogue.  Each wave then owns WHOLE rows (m-tiles wave and
// wave + kGW, all four n-tile slots), so a row's statistics are register sums
// over the wave's tiles plus one DPP row reduction over the 16 column lanes:
// no separate row pass, no re-read of the pre-activations.  L / base / pr / bp
// describe the layer's outputs (as fwd_rows).
// MODE 2: the dX GEMM of a layer whose source S = L (passed as L) is at most
// kBN wide: the epilogue runs S's ReLU / LayerNorm(+affine) backward on the
// whole rows of dY it holds and writes S's dZ (dzr_s / dzc_s) and per-wave
// bias / LN-affine column partials (colp_s): S needs no row pass of its own.
template <int MODE = 0, class FE>
__device__ __forceinline__ void gemm_nt(const float *A, int lda, const float *B, int ldb, int M, int N, int K,
                                        float *lds, const float *bias, FE epi, const GLay &L,
                                        float *base = nullptr, const float *pr = nullptr, int bp = 0,
                                        float *dzr_s = nullptr, float *dzc_s = nullptr, float *colp_s = nullptr) {
    constexpr bool LNE = MODE == 1, ROWS = MODE != 0;  // ROWS: each wave owns whole rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int lr = tid / kKC, lk = tid % kKC;  // staging: rows lr + kRS i, column lk
    float cb[4] = {0.f, 0.f, 0.f, 0.f}, cg[4] = {0.f, 0.f, 0.f, 0.f}, cbe[4] = {0.f, 0.f, 0.f, 0.f};
    for (int mb = 0; mb < M; mb += kBM)
        for (int nb = 0; nb < N; nb += kBN) {
            const int BM = M - mb < kBM ? M - mb : kBM, BN = N - nb < kBN ? N - nb : kBN;
            const int mtn = (BM + 15) >> 4, ntn = (BN + 15) >> 4, T = mtn * ntn;
            // slot j of this wave -> tile (m0, n0), valid (wave-uniform)
            auto tile = [&](int j, int &m0, int &n0) -> bool {
                if constexpr (ROWS) {
                    const int mt = wave + kGW * (j >> 2), nt = j & 3;
                    m0 = mt << 4;
                    n0 = nt << 4;
                    return mt < mtn && nt < ntn;
                } else {
                    const int t = wave + kGW * j;
                    m0 = (t % mtn) << 4;
                    n0 = (t / mtn) << 4;
                    return t < T;
                }
            };
            const float *Ab = A + (size_t)mb * lda, *Bb = B + (size_t)nb * ldb;
            float ra[kBM / kRS], rb[kBN / kRS];
            auto fetch = [&](int kc) {
                const int k = kc + lk;
                const bool kin = k < K;
                const int kk = kin ? k : 0;
                // unconditional loads from clamped (valid) addresses, then the predicate
#pragma unroll
                for (int i = 0; i < kBM / kRS; ++i) {
                    const int row = lr + kRS * i;
                    const float va = Ab[(size_t)(row < BM ? row : 0) * lda + kk];
                    ra[i] = (row < BM && kin) ? va : 0.f;
                }
#pragma unroll
                for (int i = 0; i < kBN / kRS; ++i) {
                    const int row = lr + kRS * i;
                    const float vb = Bb[(size_t)(row < BN ? row : 0) * ldb + kk];
                    rb[i] = (row < BN && kin) ? vb : 0.f;
                }
            };
            auto commit = [&](int buf) {
                float *As = lds + buf * kPanel, *Bs = As + kBM * kLdS;
#pragma unroll
                for (int i = 0; i < kBM / kRS; ++i) As[(lr + kRS * i) * kLdS + lk] = ra[i];
#pragma unroll
                for (int i = 0; i < kBN / kRS; ++i) Bs[(lr + kRS * i) * kLdS + lk] = rb[i];
            };
            f4 acc[kTPW];
            // per slot: the bias of column n0 + r (and with LNE the LN affine),
            // loaded with the first chunk: the latency hides under the panel fetch
            float bv_[kTPW];
#pragma unroll
            for (int j = 0; j < kTPW; ++j) {
                acc[j] = f4{0.f, 0.f, 0.f, 0.f};
                int m0, n0;
                const bool ok = tile(j, m0, n0) && n0 + r < BN;
                const float v = bias ? bias[nb + (ok ? n0 + r : 0)] : 0.f;
                bv_[j] = v;
            }
            fetch(0);
            if (mb | nb) __syncthreads();  // the previous block's last panels may still be read
            commit(0);
            __syncthreads();
            int buf = 0;
            for (int kc = 0; kc < K; kc += kKC) {
                const bool more = kc + kKC < K;
                if (more) fetch(kc + kKC);
                const float *As = lds + buf * kPanel, *Bs = As + kBM * kLdS;
#pragma unroll
                for (int j = 0; j < kTPW; ++j) {
                    int m0, n0;
                    if (tile(j, m0, n0)) {  // wave-uniform
                        float av[8], bv[8];
#pragma unroll
                        for (int kk = 0; kk < 8; ++kk) {
                            av[kk] = As[(m0 + r) * kLdS + 4 * kk + q];
                            bv[kk] = Bs[(n0 + r) * kLdS + 4 * kk + q];
                        }
#pragma unroll
                        for (int kk = 0; kk < 8; ++kk)
                            acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[kk], bv[kk], acc[j], 0, 0, 0);
                    }
                }
                // the last chunk needs no barrier: the epilogue touches no panel, and
                // every caller separates two GEMMs by a workgroup barrier
                if (more) {
                    commit(buf ^ 1);
                    __syncthreads();
                }
                buf ^= 1;
            }
            if constexpr (LNE) {
                const float invF = 1.f / (float)N;
                // the LN affine of the lane's four columns, loaded before any store
                float ga_[4], be_[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const int n = (nt < ntn && (nt << 4) + r < BN) ? (nt << 4) + r : 0;
                    const float gv = pr[L.ln == 2 ? L.g + n : 0], bb = pr[L.ln == 2 ? L.be + n : 0];
                    ga_[nt] = L.ln == 2 ? gv : 1.f;
                    be_[nt] = L.ln == 2 ? bb : 0.f;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if (wave + kGW * a >= mtn) break;  // wave-uniform
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = mb + ((wave + kGW * a) << 4) + 4 * q + i;
                        float v[4], s = 0.f;
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            const bool on = nt < ntn && (nt << 4) + r < BN;
                            v[nt] = on ? acc[4 * a + nt][i] + bv_[4 * a + nt] : 0.f;
                            s += v[nt];
                        }
                        float mean = 0.f, rstd = 1.f;
                        if (L.ln) {
                            mean = row_sum(s) * invF;
                            float vs = 0.f;
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) {
                                const float d = v[nt] - mean;
                                vs += (nt < ntn && (nt << 4) + r < BN) ? d * d : 0.f;
                            }
                            rstd = 1.f / sqrtf(row_sum(vs) / (float)N + 1e-5f);
                            if (r == 0 && row < M && L.rs >= 0) base[L.rs + row] = rstd;
                        }
                        if (row < M) {
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) {
                                const int n = (nt << 4) + r;
                                if (nt < ntn && n < BN) {
                                    float y = v[nt];
                                    if (L.ln) {
                                        const float xh = (y - mean) * rstd;
                                        if (L.xh >= 0) base[L.xh + (size_t)row * N + n] = xh;
                                        y = L.ln == 2 ? xh * ga_[nt] + be_[nt] : xh;
                                    }
                                    if (L.relu) y = relu(y);
                                    epi(row, n, y);
                                    if (L.yc >= 0) base[L.yc + (size_t)n * bp + row] = y;
                                }
                            }
                        }
                    }
                }
            } else if constexpr (MODE == 2) {
                const float invF = 1.f / (float)N;
                // every load of the epilogue before its first store: the LN affine of
                // the lane's columns, each row's rstd and the lane's xhat (or y)
                float ga_[4], be_[4];
#pragma unroll
                for (int nt = 0; nt < 4; ++nt) {
                    const int n = (nt < ntn && (nt << 4) + r < BN) ? (nt << 4) + r : 0;
                    const float gv = pr[L.ln == 2 ? L.g + n : 0], bb = pr[L.ln == 2 ? L.be + n : 0];
                    ga_[nt] = L.ln == 2 ? gv : 1.f;
                    be_[nt] = L.ln == 2 ? bb : 0.f;
                }
#pragma unroll
                for (int a = 0; a < 2; ++a) {
                    if (wave + kGW * a >= mtn) break;  // wave-uniform
                    // the m-tile's loads (16 rows of xhat or y, their rstd) ahead of its stores
                    float xv[4][4], rsv[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = mb + ((wave + kGW * a) << 4) + 4 * q + i;
                        const bool rok = row < M;
                        const float rv = base[L.ln && rok ? L.rs + row : 0];
                        rsv[i] = L.ln ? rv : 1.f;
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            const int n = (nt << 4) + r;
                            const bool on = rok && nt < ntn && n < BN;
                            const size_t o = on ? (size_t)row * N + n : 0;
                            const float x = base[L.ln ? L.xh + o : (L.relu ? L.yr + o : 0)];
                            xv[i][nt] = on ? x : 0.f;
                        }
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int row = mb + ((wave + kGW * a) << 4) + 4 * q + i;
                        float dp[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt) {
                            const bool on = nt < ntn && (nt << 4) + r < BN && row < M;
                            const float x = xv[i][nt];
                            const float pre = L.ln == 2 ? x * ga_[nt] + be_[nt] : x;
                            dp[nt] = (on && (!L.relu || pre > 0.f)) ? acc[4 * a + nt][i] : 0.f;
                            const float dx = dp[nt] * ga_[nt];
                            s1 += dx;
                            s2 += dx * x;
                        }
                        float m1 = 0.f, m2 = 0.f;
                        if (L.ln) {
                            m1 = row_sum(s1) * invF;
                            m2 = row_sum(s2) * invF;
                        }
                        if (row < M) {
#pragma unroll
                            for (int nt = 0; nt < 4; ++nt) {
                                const int n = (nt << 4) + r;
                                if (nt < ntn && n < BN) {
                                    const float x = xv[i][nt];
                                    const float dz = L.ln ? rsv[i] * (dp[nt] * ga_[nt] - m1 - x * m2) : dp[nt];
                                    dzr_s[(size_t)row * N + n] = dz;
                                    dzc_s[(size_t)n * bp + row] = dz;
                                    cb[nt] += dz;
                                    cg[nt] += dp[nt] * x;
                                    cbe[nt] += dp[nt];
                                }
                            }
                        }
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < kTPW; ++j) {
                    int m0, n0;
                    if (tile(j, m0, n0)) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int m = m0 + 4 * q + i, n = n0 + r;
                            if (m < BM && n < BN) epi(mb + m, nb + n, acc[j][i] + bv_[j]);
                        }
                    }
                }
            }
        }
    if constexpr (MODE == 2) {
        // the wave's four row groups (lanes l, l ^ 16, l ^ 32, l ^ 48), then per
        // wave into colp_s (the caller sums the waves in order)
#pragma unroll
        for (int nt = 0; nt < 4; ++nt) {
            cb[nt] += __shfl_xor(cb[nt], 16, 64);
            cb[nt] += __shfl_xor(cb[nt], 32, 64);
            cg[nt] += __shfl_xor(cg[nt], 16, 64);
            cg[nt] += __shfl_xor(cg[nt], 32, 64);
            cbe[nt] += __shfl_xor(cbe[nt], 16, 64);
            cbe[nt] += __shfl_xor(cbe[nt], 32, 64);
        }
        if (q == 0) {
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                const int n = (nt << 4) + r;
                if (n < N) {
                    colp_s[wave * N + n] = cb[nt];
                    colp_s[(kGW + wave) * N + n] = cg[nt];
                    colp_s[(2 * kGW + wave) * N + n] = cbe[nt];
                }
            }
        }
    }
}

// LayerNorm(+affine) / ReLU forward of one layer's rows, 16 lanes per row;
// rows r, r + 32, r + 64, r + 96 of a 128-row block are processed together
// with C columns per lane cached in registers (F <= 16 C): all loads of the
// block are issued before the first reduction (one round trip, not three per
// row).  C = 0: any width, three passes over the row per 32 rows.
template <int C>
__device__ __forceinline__ void fwd_rows(const GLay &L, float *base, const float *pr, int bsz, int bp) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    float *yr = base + L.yr;
    const int F = L.fout;
    const float invF = 1.f / (float)F;
    auto out = [&](int row, int j, float y, float mean, float rstd, float ga, float be) {
        if (L.ln) {
            const float xh = (y - mean) * rstd;
            if (L.xh >= 0) base[L.xh + (size_t)row * F + j] = xh;
            y = L.ln == 2 ? xh * ga + be : xh;
        }
        if (L.relu) y = relu(y);
        yr[(size_t)row * F + j] = y;
        if (L.yc >= 0) base[L.yc + (size_t)j * bp + row] = y;
    };
    if constexpr (C > 0) {
        constexpr int R = 4;
        // the LN affine of the lane's columns, loaded before any store
        float ga[C], be[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int j = sub + 16 * i < F ? sub + 16 * i : 0;
            const float a = pr[L.ln == 2 ? L.g + j : 0], b = pr[L.ln == 2 ? L.be + j : 0];
            ga[i] = a;
            be[i] = b;
        }
        for (int r0 = 0; r0 < bsz; r0 += R * 4 * kGW) {
            float z[R][C];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int row = r0 + 4 * wave + rq + 4 * kGW * u;
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const int j = sub + 16 * i;
                    const bool on = row < bsz && j < F;
                    const float v = yr[on ? (size_t)row * F + j : 0];
                    z[u][i] = on ? v : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int row = r0 + 4 * wave + rq + 4 * kGW * u;
                float mean = 0.f, rstd = 1.f;
                if (L.ln) {
                    float s = 0.f;
#pragma unroll
                    for (int i = 0; i < C; ++i) s += z[u][i];
                    mean = row_sum(s) * invF;
                    float vs = 0.f;
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const float d = z[u][i] - mean;
                        vs += (sub + 16 * i < F) ? d * d : 0.f;
                    }
                    rstd = 1.f / sqrtf(row_sum(vs) / (float)F + 1e-5f);
                    if (row < bsz && sub == 0 && L.rs >= 0) base[L.rs + row] = rstd;
                }
                if (row < bsz) {
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const int j = sub + 16 * i;
                        if (j < F) out(row, j, z[u][i], mean, rstd, ga[i], be[i]);
                    }
                }
            }
        }
    } else {
        for (int r0 = 0; r0 < bsz; r0 += 4 * kGW) {
            const int row = r0 + 4 * wave + rq;
            const bool live = row < bsz;
            float s = 0.f;
            if (live)
                for (int j = sub; j < F; j += 16) s += yr[(size_t)row * F + j];
            float mean = 0.f, rstd = 1.f;
            if (L.ln) {
                mean = row_sum(s) * invF;
                float vs = 0.f;
                if (live)
                    for (int j = sub; j < F; j += 16) {
                        const float dz = yr[(size_t)row * F + j] - mean;
                        vs += dz * dz;
                    }
                rstd = 1.f / sqrtf(row_sum(vs) / (float)F + 1e-5f);
                if (live && sub == 0 && L.rs >= 0) base[L.rs + row] = rstd;
            }
            if (!live) continue;
            for (int j = sub; j < F; j += 16)
                out(row, j, yr[(size_t)row * F + j], mean, rstd, L.ln == 2 ? pr[L.g + j] : 1.f,
                    L.ln == 2 ? pr[L.be + j] : 0.f);
        }
    }
}

// Forward of a minibatch (or a block of env rows) through the layer list:
// GEMM + bias -> Ls[l].yr, then LayerNorm(+affine) / ReLU as a row pass,
// keeping xhat / rstd / the feature-major copy where the plan has room for
// them (the learner; the policy step keeps outputs only).  xobs: the
// observation rows (stride = the first layer's fin).
__device__ __forceinline__ void forward_layers(const GLay *Ls, int nl, const float *xobs, int bsz, float *base, const float *pr,
                               int bp, float *lds, int dbg = 0, long long *st = nullptr) {
    for (int l = 0; l < nl; ++l) {
        const GLay &L = Ls[l];
        const float *x = L.src < 0 ? xobs : base + Ls[L.src].yr;
        float *yr = base + L.yr;
        const int F = L.fout;
        const float *bias = pr + L.b;
        const bool lne = F <= kBN && (L.ln || L.relu);  // LayerNorm / ReLU in the GEMM epilogue
        if (!(dbg & 1)) {
            if (lne)
                gemm_nt<1>(x, L.fin, pr + L.w, L.fin, bsz, F, L.fin, lds, bias,
                                   [&](int m, int n, float c) { yr[(size_t)m * F + n] = c; }, L, base, pr, bp);
            else
                gemm_nt<0>(x, L.fin, pr + L.w, L.fin, bsz, F, L.fin, lds, bias,
                                   [&](int m, int n, float c) { yr[(size_t)m * F + n] = c; }, L);
        }
        __syncthreads();
        if (lne || (L.ln == 0 && !L.relu && L.yc < 0) || (dbg & 8)) {
            if (st) st[1 + l] = (long long)__builtin_readcyclecounter();
            continue;
        }
        if (F <= 128) fwd_rows<8>(L, base, pr, bsz, bp);
        else fwd_rows<0>(L, base, pr, bsz, bp);
        __syncthreads();
        if (st) st[1 + l] = (long long)__builtin_readcyclecounter();
    }
}

// ---- the few-row form (ppo_learn_graph_part_kernel<true>) --------------------
// A partner's slice of at most kFR = 16 minibatch rows stays in LDS for the
// whole update: the observation tile, every layer's output Y, xhat and rstd,
// and dY, each a [16][ld] row-major tile (ld = the width rounded up to 16,
// + 4: float4 row reads spread over the banks).  The padding columns are zero
// from the kernel's start and never written, so every contraction runs over
// whole 16-wide chunks with no masks; rows past the slice carry finite values
// and a zero gradient.  One 16-row MFMA m-tile covers the slice, its n-tiles
// go round the four waves; LayerNorm / ReLU (forward and backward) are row
// passes, 16 lanes per row, one row per lane group; bias / LN-affine
// gradients are column sums over the 16 rows, one thread per column, in row
// order.  Weights come from L2 (buffer loads, the agent's partners share
// them): W [out][in] for the forward, the transposed copy for dX.
constexpr int kFR = 16;

__device__ __forceinline__ f4 bload4(__amdgpu_buffer_rsrc_t r, int byte_off) {
    return __builtin_bit_cast(f4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}

// C[16 x N] = X[16 x K] . W^T, W's row n at byte woff + 4 n K of the buffer
// wr: lane (r, q) feeds k = 16c + 4q + j to MFMA j of chunk c (float4 reads
// of X from LDS and of W from L2, four chunks' loads in flight).  epi(row, n,
// v) for the lane's outputs with n < N.  Rows of W past N read other finite
// parameters (or zeros past the buffer) and are never stored.
// TRANSB: W is [K][N] instead (row k at byte woff + 4 k N): MFMA j of chunk c
// takes W[16c + 4q + j][n0 + r], one dword per lane, 16 lanes on one 64-byte
// row segment (the dX of a layer straight from its nn.Linear weight).
template <bool TRANSB = false, class FE>
__device__ __forceinline__ void few_gemm(const float *X, int ldx, __amdgpu_buffer_rsrc_t wr, int woff, int K, int N,
                                         const float *bias, FE epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int nc = (K + 15) >> 4, ntile = (N + 15) >> 4;
    const float *xr = X + r * ldx + 4 * q;
    for (int t = wave; t < ntile; t += kGW) {
        const int n0 = t << 4;
        const int wrow = TRANSB ? woff + (4 * q * N + n0 + r) * 4 : woff + ((n0 + r) * K + 4 * q) * 4;
        const float bv = bias ? bias[n0 + r < N ? n0 + r : 0] : 0.f;  // in flight under the MFMAs
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < nc; c0 += 4) {
            f4 wv[4], xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u < nc ? c0 + u : nc - 1;
                if constexpr (TRANSB) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        wv[u][j] = __builtin_bit_cast(
                            float, __builtin_amdgcn_raw_buffer_load_b32(wr, wrow + ((16 * c + j) * N) * 4, 0, 0));
                } else {
                    wv[u] = bload4(wr, wrow + c * 64);
                }
                xv[u] = *reinterpret_cast<const f4 *>(xr + 16 * c);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u >= nc) break;  // uniform
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u][j], wv[u][j], acc, 0, 0, 0);
            }
        }
        if (n0 + r < N) {
#pragma unroll
            for (int j = 0; j < 4; ++j) epi(4 * q + j, n0 + r, acc[j] + bv);
        }
    }
}

// few_gemm with W [16-rounded N][ldw] and the bias in LDS, zero padded to
// whole 16 x 16 tiles (the evaluation pass's resident weights)
template <class FE>
__device__ __forceinline__ void few_gemm_l(const float *X, int ldx, const float *W, int ldw, int K, int N,
                                           const float *bias, FE epi) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, q = lane >> 4;
    const int nc = (K + 15) >> 4, ntile = (N + 15) >> 4;
    const float *xr = X + r * ldx + 4 * q;
    for (int t = wave; t < ntile; t += kGW) {
        const int n0 = t << 4;
        const float *wr = W + (n0 + r) * ldw + 4 * q;
        const float bv = bias[n0 + r];
        f4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int c0 = 0; c0 < nc; c0 += 4) {  // four chunks' reads in flight, then their MFMAs
            f4 xv[4], wv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int c = c0 + u < nc ? c0 + u : nc - 1;
                xv[u] = *reinterpret_cast<const f4 *>(xr + 16 * c);
                wv[u] = *reinterpret_cast<const f4 *>(wr + 16 * c);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (c0 + u >= nc) break;  // uniform
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(xv[u][j], wv[u][j], acc, 0, 0, 0);
            }
        }
        if (n0 + r < N) {
#pragma unroll
            for (int j = 0; j < 4; ++j) epi(4 * q + j, n0 + r, acc[j] + bv);
        }
    }
}

// LayerNorm(+affine) / ReLU of one row in place (16 lanes per row, sub =
// the lane's column phase), the row's values held in M registers per lane
// (F <= 16 M): every LDS read issued before the first use, the same float
// operations in the same order as the column loops
constexpr int kRowRegs = 8;
// the fields a row pass reads, loaded with the layer's other fields before its
// GEMM (not re-read from the layer table after the barrier)
struct LayRow {
    int ln, relu;
    long long af, rs, xh;
};
template <int M>
__device__ __forceinline__ void few_row_pass(float *y, float *S, const LayRow &L, int F, int ld, int row, int sub) {
    // whole 16-column chunks up to the 16-rounded width (a uniform bound: no
    // per-lane branches); the padding columns read zero and are written zero,
    // columns >= F enter no sum
    const int mp = (F + 15) >> 4;
    float v[M], ga[M], be[M];
    bool ok[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const int j = sub + 16 * i;
        ok[i] = j < F;
        v[i] = ga[i] = be[i] = 0.f;
        if (i < mp) {
            v[i] = y[j];
            if (L.ln == 2) {
                ga[i] = S[L.af + j];
                be[i] = S[L.af + F + j];
            }
        }
    }
    float mean = 0.f, rstd = 1.f;
    if (L.ln) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < M; ++i) s = ok[i] ? s + v[i] : s;
        mean = row_sum(s) * (1.f / (float)F);
        float vs = 0.f;
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const float d = v[i] - mean;
            vs = ok[i] ? vs + d * d : vs;
        }
        rstd = 1.f / sqrtf(row_sum(vs) / (float)F + 1e-5f);
        if (sub == 0 && L.rs >= 0) S[L.rs + row] = rstd;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
        if (i >= mp) break;  // uniform
        const int j = sub + 16 * i;
        float x = v[i];
        if (L.ln) {
            const float xh = (x - mean) * rstd;
            if (L.xh >= 0) S[L.xh + row * ld + j] = ok[i] ? xh : 0.f;
            x = L.ln == 2 ? xh * ga[i] + be[i] : xh;
        }
        if (L.relu) x = relu(x);
        y[j] = ok[i] ? x : 0.f;
    }
}

// Forward of the 16-row LDS tiles through the layer list: the few-row GEMM
// (+ bias) into Y, then LayerNorm(+affine) / ReLU as a row pass in place,
// keeping xhat / rstd where the plan has them (the learner; the policy step
// keeps Y only).  The observation tile is at oc (row stride ld0).
// WLDS: the weights are LDS-resident (layer l's W [16-rounded fout][ldw[l]]
// at S + wl[l], zero padded, its bias after it; the evaluation pass copies
// them once per launch); run: the layers to compute (bit l), the others are
// skipped (the evaluation's forward needs the actor's path only).
template <bool WLDS = false>
__device__ __forceinline__ void few_forward(const GLay *Ls, int nl, float *S, const float *pr,
                                            __amdgpu_buffer_rsrc_t prs, long long oc, int ld0, long long *st,
                                            unsigned run = ~0u, const long long *wl = nullptr,
                                            const int *ldw = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int row = 4 * wave + rq;
    for (int l = 0; l < nl; ++l) {
        if (!((run >> l) & 1u)) continue;  // uniform
        const GLay &L = Ls[l];
        const int F = L.fout, ld = L.ld;
        const LayRow lr{L.ln, L.relu, L.af, L.rs, L.xh};
        const float *X = L.src < 0 ? S + oc : S + Ls[L.src].yr;
        const int ldx = L.src < 0 ? ld0 : Ls[L.src].ld;
        float *Y = S + L.yr;
        // the LN affine for this update's row passes (forward and backward) to
        // LDS, its loads in flight under the GEMM
        float ga[2] = {0.f, 0.f}, be[2] = {0.f, 0.f};
        if (!WLDS && L.ln == 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (tid + h * kGT < F) {
                    ga[h] = pr[L.g + tid + h * kGT];
                    be[h] = pr[L.be + tid + h * kGT];
                }
        }
        if constexpr (WLDS) {
            const float *W = S + wl[l];
            few_gemm_l(X, ldx, W, ldw[l], L.fin, F, W + (long long)((F + 15) & ~15) * ldw[l],
                       [&](int m, int n, float v) { Y[m * ld + n] = v; });
        } else {
            few_gemm(X, ldx, prs, L.w * 4, L.fin, F, pr + L.b, [&](int m, int n, float v) { Y[m * ld + n] = v; });
        }
        if (!WLDS && L.ln == 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h)
                if (tid + h * kGT < F) {
                    S[L.af + tid + h * kGT] = ga[h];
                    S[L.af + F + tid + h * kGT] = be[h];
                }
        }
        __syncthreads();
        if (lr.ln || lr.relu) {
            float *y = Y + row * ld;
            if (F <= 64) {
                few_row_pass<4>(y, S, lr, F, ld, row, sub);
            } else if (F <= 16 * kRowRegs) {
                few_row_pass<kRowRegs>(y, S, lr, F, ld, row, sub);
            } else {
                const float invF = 1.f / (float)F;
                float mean = 0.f, rstd = 1.f;
                if (L.ln) {
                    float s = 0.f;
                    for (int j = sub; j < F; j += 16) s += y[j];
                    mean = row_sum(s) * invF;
                    float vs = 0.f;
                    for (int j = sub; j < F; j += 16) {
                        const float d = y[j] - mean;
                        vs += d * d;
                    }
                    rstd = 1.f / sqrtf(row_sum(vs) / (float)F + 1e-5f);
                    if (sub == 0 && L.rs >= 0) S[L.rs + row] = rstd;
                }
                for (int j = sub; j < F; j += 16) {
                    float v = y[j];
                    if (L.ln) {
                        const float xh = (v - mean) * rstd;
                        if (L.xh >= 0) S[L.xh + row * ld + j] = xh;
                        v = L.ln == 2 ? xh * S[L.af + j] + S[L.af + F + j] : xh;
                    }
                    if (L.relu) v = relu(v);
                    y[j] = v;
                }
            }
            __syncthreads();
        }
        if (st) st[1 + l] = (long long)__builtin_readcyclecounter();
    }

}

// The policy step's plan (act_plan, act_plan_few): what a step of the layer
// list needs besides its ActArgs (rollout.h).
struct GActArgs {
    GLay L[kGL];
    int nl, aout, cout, A, D, n, rows;
    int ld0;                 // few-row form: the observation tile's row stride
    long long oc, lds_floats;  // few-row form: its offset, the LDS tiles' size
    long long ws_block;  // scratch floats per (agent, row block)
    long long obs_off;   // persistent rollout: the step's observation rows [rows][D] in the block scratch
    float *ws;
};

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
long long r4(long long x) { return (x + 3) & ~3ll; }

// validate the layer list; fill the layer table and the per-agent scratch plan.
// extra: floats of the parameter row that no layer owns (the Gaussian head's
// log_std, agx_gauss.h); the layers and they cover the row exactly
int plan_graph(const agx_ppo_graph *net, int64_t batch, GArgs &a, int extra = 0) {
    AGX_REQUIRE(net, "agx_ppo_graph: null graph");
    const int nl = net->n_layers;
    AGX_REQUIRE(nl >= 2 && nl <= kGL, "agx_ppo_graph: %d layers (2..%d)", nl, kGL);
    AGX_REQUIRE(net->obs_dim >= 1 && net->n_params > 0 && net->critic_start > 0 && net->critic_start < net->n_params,
                "agx_ppo_graph: bad sizes");
    AGX_REQUIRE(net->n_actions >= 1 && net->n_actions <= AGX_PPO_GRAPH_MAX_ACTIONS,
                "agx_ppo_graph: %d actions (1..%d)", net->n_actions, AGX_PPO_GRAPH_MAX_ACTIONS);
    AGX_REQUIRE(net->actor_out >= 0 && net->actor_out < nl && net->critic_out >= 0 && net->critic_out < nl &&
                    net->actor_out != net->critic_out,
                "agx_ppo_graph: bad output layers");
    const int64_t bp = (batch + 15) / 16 * 16;
    AGX_REQUIRE(batch >= 1 && bp < (1 << 30), "agx_ppo_graph: bad batch %lld", (long long)batch);
    bool is_src[kGL] = {};
    int consumers[kGL] = {};
    int maxw = 0;
    long long nw = 0;
    for (int l = 0; l < nl; ++l) {
        const agx_ppo_layer &x = net->layers[l];
        AGX_REQUIRE(x.src >= -1 && x.src < l, "agx_ppo_graph: layer %d reads layer %d (not topological)", l, x.src);
        const int fin = x.src < 0 ? net->obs_dim : net->layers[x.src].fout;
        AGX_REQUIRE(x.fin == fin && x.fout >= 1, "agx_ppo_graph: layer %d width mismatch", l);
        AGX_REQUIRE(x.ln >= 0 && x.ln <= 2, "agx_ppo_graph: layer %d ln %d", l, x.ln);
        AGX_REQUIRE((x.ln == 0 && !x.relu) || x.fout <= AGX_PPO_GRAPH_MAX_WIDTH,
                    "agx_ppo_graph: layer %d width %d > %d", l, x.fout, AGX_PPO_GRAPH_MAX_WIDTH);
        auto in = [&](long long off, long long len) { return off >= 0 && off + len <= net->n_params; };
        AGX_REQUIRE(in(x.w, (long long)x.fin * x.fout) && in(x.b, x.fout) &&
                        (x.ln != 2 || (in(x.ln_w, x.fout) && in(x.ln_b, x.fout))),
                    "agx_ppo_graph: layer %d parameters outside the row", l);
        if (x.src >= 0) {
            is_src[x.src] = true;
            AGX_REQUIRE(++consumers[x.src] <= 2, "agx_ppo_graph: layer %d feeds more than two layers", x.src);
        }
        maxw = x.fout > maxw ? x.fout : maxw;
        nw += (long long)x.fin * x.fout + x.fout * (x.ln == 2 ? 3 : 1);
    }
    AGX_REQUIRE(extra >= 0 && nw + extra == net->n_params, "agx_ppo_graph: layers cover %lld of %d parameters", nw,
                net->n_params - (extra > 0 ? extra : 0));
    const agx_ppo_layer &la = net->layers[net->actor_out], &lc = net->layers[net->critic_out];
    AGX_REQUIRE(la.fout == net->n_actions && lc.fout == 1 && la.ln == 0 && lc.ln == 0 && !la.relu && !lc.relu &&
                    !is_src[net->actor_out] && !is_src[net->critic_out],
                "agx_ppo_graph: the output layers must be plain Linear(-> n_actions) / Linear(-> 1)");
    long long off = 0;
    bool seen[kGL] = {};
    for (int l = nl - 1; l >= 0; --l) {  // backward order: the first consumer writes dY, later ones add
        const int s = net->layers[l].src;
        a.L[l].acc = (s >= 0 && seen[s]) ? 1 : 0;
        if (s >= 0) seen[s] = true;
    }
    for (int l = 0; l < nl; ++l) {
        const agx_ppo_layer &x = net->layers[l];
        GLay &L = a.L[l];
        L.fin = x.fin;
        L.fout = x.fout;
        L.w = x.w;
        L.b = x.b;
        L.g = x.ln == 2 ? x.ln_w : -1;
        L.be = x.ln == 2 ? x.ln_b : -1;
        L.ln = x.ln;
        L.relu = x.relu ? 1 : 0;
        L.src = x.src;
        L.yr = off;
        off = r4(off + bp * x.fout);
        L.yc = -1;
        if (is_src[l]) {
            L.yc = off;
            off = r4(off + (long long)x.fout * bp);
        }
        L.xh = L.rs = -1;
        if (x.ln) {
            L.xh = off;
            off = r4(off + bp * x.fout);
            L.rs = off;
            off = r4(off + bp);
        }
        L.dy = off;
        off = r4(off + bp * x.fout);
        L.dy2 = -1;
        if (consumers[l] == 2) {
            L.dy2 = off;
            off = r4(off + bp * x.fout);
        }
        L.wt = -1;  // allocated after the gradient row (below)
        L.dyc = -1;
        if (l == net->actor_out) {  // the value layer's (width 1) row- and feature-major forms coincide
            L.dyc = off;
            off = r4(off + (long long)x.fout * bp);
        } else if (l == net->critic_out) {
            L.dyc = L.dy;
        }
    }
    a.oc = off;
    off = r4(off + (long long)net->obs_dim * bp);
    a.dzr = off;
    off = r4(off + bp * maxw);
    a.dzc = off;
    off = r4(off + bp * maxw);
    a.dzr1 = off;
    off = r4(off + bp * maxw);
    a.dzc1 = off;
    off = r4(off + bp * maxw);
    // backward fusion: a layer whose only consumer is the next layer, at most
    // kBN wide with a LayerNorm / ReLU, gets its dZ from that consumer's dX
    // epilogue (dZ buffers alternate by layer parity, so the consumer's own dZ
    // and its source's never share one)
    for (int l = 0; l < nl; ++l) {
        a.L[l].fuse = a.L[l].fused = 0;
    }
    for (int l = 1; l < nl; ++l) {
        const agx_ppo_layer &x = net->layers[l], &sx = net->layers[l - 1];
        if (x.src == l - 1 && consumers[l - 1] == 1 && sx.fout <= kBN && (sx.ln || sx.relu)) {
            a.L[l].fuse = 1;
            a.L[l - 1].fused = 1;
        }
    }
    a.t1 = off;
    off = r4(off + bp * maxw);
    a.t2 = off;
    off = r4(off + bp * maxw);
    a.gr = off;
    off = r4(off + net->n_params);
    // the transposed weights last: a partner's scratch is everything before the
    // gradient row (its gradient goes to the exchange slab, the transposed
    // weights are shared by the agent's partners)
    a.ws_part = (a.gr + 63) & ~63ll;
    a.wt0 = off;
    for (int l = 0; l < nl; ++l) {
        const agx_ppo_layer &x = net->layers[l];
        if (x.src >= 0) {
            a.L[l].wt = off;
            off = r4(off + (long long)x.fin * x.fout);
        }
    }
    a.wt_agent = ((off - a.wt0) + 63) & ~63ll;
    a.ws_agent = (off + 63) & ~63ll;  // 256-byte aligned agent blocks
    a.nl = nl;
    a.aout = net->actor_out;
    a.cout = net->critic_out;
    a.A = net->n_actions;
    a.D = net->obs_dim;
    a.n = net->n_params;
    a.cstart = net->critic_start;
    a.bp = (int)bp;
    return AGX_OK;
}

constexpr int kActRows = 4 * kGW;  // env rows per policy-step workgroup (one row pass)

// the policy step keeps each layer's output only
long long act_plan(const GArgs &full, GActArgs &a) {
    long long off = 0;
    for (int l = 0; l < full.nl; ++l) {
        a.L[l] = full.L[l];
        GLay &L = a.L[l];
        L.yr = off;
        off = r4(off + (long long)kActRows * L.fout);
        L.yc = L.xh = L.rs = L.dy = L.dy2 = L.wt = L.dyc = -1;
        L.fuse = L.fused = 0;
    }
    a.nl = full.nl;
    a.aout = full.aout;
    a.cout = full.cout;
    a.A = full.A;
    a.D = full.D;
    a.n = full.n;
    a.rows = kActRows;
    a.obs_off = off;
    off = r4(off + (long long)kActRows * full.D);
    a.ws_block = (off + 63) & ~63ll;
    return a.ws_block;
}

// The policy step's few-row form: act_plan's layer table with every output
// a [16][ld] LDS tile (+ the LN affine copy), and the observation tile.  ->
// dynamic LDS bytes, 0 when it does not fit beside the kernel's static LDS
// (or AGX_GRAPH_FEW=0).  The policy-step block is kActRows = 16 rows either way.
template <class KER>
size_t act_plan_few(KER kernel, GActArgs &a) {
    if (const char *e = getenv("AGX_GRAPH_FEW"))
        if (atoi(e) == 0) return 0;
    static_assert(kActRows == kFR, "the few-row policy step covers one row block");
    auto ldof = [](int w) { return (w + 15) / 16 * 16 + 4; };
    long long off = 0;
    for (int l = 0; l < a.nl; ++l) {
        GLay &L = a.L[l];
        L.ld = ldof(L.fout);
        L.yr = off;
        off += (long long)kFR * L.ld;
        L.af = -1;
        if (L.ln == 2) {
            L.af = off;
            off += 2 * ((L.fout + 3) / 4 * 4);
        }
        L.xh = L.rs = -1;
    }
    a.ld0 = ldof(a.D);
    a.oc = off;
    off += (long long)kFR * a.ld0;
    a.lds_floats = (off + 3) & ~3ll;
    hipFuncAttributes fa{};
    const size_t st = hipFuncGetAttributes(&fa, (const void *)kernel) == hipSuccess ? fa.sharedSizeBytes : 8 * 1024;
    const size_t bytes = (size_t)a.lds_floats * 4;
    if (st >= kLdsMax || bytes > kLdsMax - st) return 0;
    (void)hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kLdsMax - st));
    return bytes;
}

}  // namespace
}  // namespace agx
