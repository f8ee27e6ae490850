// Runtime-shape fused PPO learner (include/agx_graph.h): the learner for the
// network shapes architecture mutations produce.
//
// agx_ppo_learn (learner.hip) compiles one plan per network shape: parameters
// in LDS, Adam moments in registers, every offset a constant.  An
// architecture mutation (hpo/mutation.py:829-885) moves an agent to one of
// thousands of shapes — any depth of encoder / head, any width, a latent of
// any size — so this kernel interprets a runtime LAYER LIST instead:
//
//   * one 256-thread workgroup per agent runs every epoch x minibatch update
//     of PPO.learn (ppo.py:836-920) in one launch, like agx_ppo_learn;
//   * a minibatch is processed layer by layer over all its rows: every Linear
//     (forward, dW, dX) is ONE operand form, C = A . B^T with both operands
//     contiguous along the contraction, on f32 MFMA 16x16x4 tiles whose
//     operand panels are staged through LDS from the agent's L2-resident
//     scratch.  The layouts that make that true are written where the data is
//     produced: activations row-major (the next layer's forward) AND
//     feature-major (the next layer's dW contracts over rows), and Adam writes
//     every weight both as nn.Linear [out][in] (forward) and transposed (dX);
//   * LayerNorm / ReLU forward runs in the forward GEMM's epilogue for layers
//     up to 64 wide (each wave owns whole rows), its backward in the
//     consumer's dX epilogue for single-consumer layers; wider / shared layers
//     and the PPO loss are row passes, 16 lanes per row (DPP row reductions);
//     bias and LN-affine gradients are per-wave partials summed in one fixed
//     order (an agent's update does not depend on its population);
//   * two-group gradient-norm clip (ppo.py:910-911) and Adam
//     (optimizer_wrapper.py:444-452) over the flat gradient row.
//
// The layer table, its plans, the GEMM and the forward are graph_net.h's
// (shared with the policy step, graph_rollout.hip); this unit is the backward,
// the learn kernels and their host side.
//
// HEAD (a compile-time parameter of the learn kernels, ppo_learn_graph_kernel
// and the two forms of ppo_learn_graph_part_kernel): kCat, the categorical
// head of a Discrete action space; kGauss, kMulti and kBern below.  The gather
// prologue is ppo_gather.h's kernel over the head's action packer; what else
// the host path knows of a head is HeadTraits.
//
// kGauss: the diagonal-Gaussian
// head of a Box action space (include/agx_gauss.h).  The actor's output is the
// mean, the stored actions are float [A] per row, and the A log_std floats at
// GArgs::lso are parameters no layer owns: the loss row pass computes their
// gradient (a column sum over the rows, as the output-layer bias gradients),
// the clip counts them in the actor group and Adam steps them with the row.
//
// kMulti: the multi-categorical head of a MultiDiscrete action space
// (include/agx_multi.h).  The network is the categorical one at n_actions =
// L = sum nvec, so forward, backward, exchange, clip and Adam are the
// categorical instantiation's; the gather packs a row's K stored actions into
// one target word (bit off_k + a_k per component, gact as the categorical
// index: 4 bytes per row) and the loss row pass walks the K components
// (GArgs::mk / mn, by value in the kernel arguments) with the lanes outside the
// component neutral in row_max / row_sum, as multi_policy.hip's MultiHead::step.
// For K = 1 the pass runs the categorical pass's float operations in its order.
//
// kBern: the Bernoulli head of a MultiBinary action space
// (include/agx_bernoulli.h).  Again the categorical network at n_actions = n;
// the gather packs a row's n stored bits into one target word (bit j = a_j != 0)
// and the loss row pass is elementwise per lane (bern_head.h) with two row sums
// per row: no component walk, no kernel argument of its own.
#include "../../include/agx_bernoulli.h"
#include "../../include/agx_gauss.h"
#include "../../include/agx_multi.h"
#include "bern_head.h"
#include "gauss_head.h"
#include "graph_net.h"
#include "multi_head_check.h"
#include "ppo_gather.h"
#include "ppo_loss_sample.h"

namespace agx {
namespace {

// fixed-order workgroup sum of two per-thread values
__device__ __forceinline__ void block_sum2(float &a, float &b, float *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    a = wave_sum(a);
    b = wave_sum(b);
    __syncthreads();  // red may still be read by the previous call
    if (lane == 0) {
        red[wave] = a;
        red[kGW + wave] = b;
    }
    __syncthreads();
    float ta = 0.f, tb = 0.f;
    for (int i = 0; i < kGW; ++i) {
        ta += red[i];
        tb += red[kGW + i];
    }
    a = ta;
    b = tb;
}

// LayerNorm(+affine) / ReLU backward of one layer's rows: dY -> dZ (row-major
// dzr and feature-major dzc), plus dY' xhat and dY' feature-major (t1c, t2c)
// for the LN-affine gradients.  As fwd_rows: C columns per lane cached for
// 16 / C rows at once (F <= 16 C); C = 0: any width, re-reading the row.
// C > 0 also takes the bias / LN-affine column sums: per lane over its rows,
// across the wave's four row groups, then per wave into colp (LDS, [3][kGW][F]);
// the caller adds the waves in order.  No t1c / t2c round trip through memory.
template <int C>
__device__ __forceinline__ void bwd_rows(const GLay &L, float *base, const float *pr, int bsz, int bp, float *dzr,
                                         float *dzc, float *t1c, float *t2c, float *colp = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int F = L.fout;
    const float invF = 1.f / (float)F;
    const float *dy = base + L.dy;
    auto put = [&](int row, int j, float d, float xh, float dz) {
        if (L.ln == 2) {
            t1c[(size_t)j * bp + row] = d * xh;
            t2c[(size_t)j * bp + row] = d;
        }
        dzr[(size_t)row * F + j] = dz;
        dzc[(size_t)j * bp + row] = dz;
    };
    if constexpr (C > 0) {
        constexpr int R = 16 / C;  // 16 cached columns per lane: three loads each in flight
        // LN affine of the lane's columns (the ReLU mask of an LN layer is
        // recomputed from xhat: the same float ops as the forward, no y load)
        float gam[C], bet[C];
#pragma unroll
        for (int i = 0; i < C; ++i) {
            const int j = sub + 16 * i;
            const float v = pr[L.ln == 2 ? L.g + (j < F ? j : 0) : 0];
            const float b = pr[L.ln == 2 ? L.be + (j < F ? j : 0) : 0];
            gam[i] = L.ln == 2 ? v : 1.f;
            bet[i] = L.ln == 2 ? b : 0.f;
        }
        float cb[C], cg[C], cbe[C];  // the lane's column partial sums (dz, dy' xhat, dy')
#pragma unroll
        for (int i = 0; i < C; ++i) cb[i] = cg[i] = cbe[i] = 0.f;
        for (int r0 = 0; r0 < bsz; r0 += R * 4 * kGW) {
            float dp[R][C], xh[R][C], rs[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int row = r0 + 4 * wave + rq + 4 * kGW * u;
                const int rr = row < bsz ? row : 0;
                const float rv = base[L.ln ? L.rs + rr : 0];
                rs[u] = L.ln ? rv : 1.f;
#pragma unroll
                for (int i = 0; i < C; ++i) {
                    const int j = sub + 16 * i;
                    const bool on = row < bsz && j < F;
                    const size_t o = on ? (size_t)row * F + j : 0;
                    const float d = dy[o], d2 = base[L.dy2 >= 0 ? L.dy2 + o : 0];
                    const float y = base[(L.relu && !L.ln) ? L.yr + o : 0];
                    const float x = base[L.ln ? L.xh + o : 0];
                    const float pre = L.ln == 2 ? x * gam[i] + bet[i] : (L.ln ? x : y);
                    dp[u][i] = (on && (!L.relu || pre > 0.f)) ? (L.dy2 >= 0 ? d + d2 : d) : 0.f;
                    xh[u][i] = (on && L.ln) ? x : 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int row = r0 + 4 * wave + rq + 4 * kGW * u;
                float m1 = 0.f, m2 = 0.f;
                if (L.ln) {
                    float s1 = 0.f, s2 = 0.f;
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const float dx = dp[u][i] * gam[i];
                        s1 += dx;
                        s2 += dx * xh[u][i];
                    }
                    m1 = row_sum(s1) * invF;
                    m2 = row_sum(s2) * invF;
                }
                if (row < bsz) {
#pragma unroll
                    for (int i = 0; i < C; ++i) {
                        const int j = sub + 16 * i;
                        if (j < F) {
                            const float dz = L.ln ? rs[u] * (dp[u][i] * gam[i] - m1 - xh[u][i] * m2) : dp[u][i];
                            dzr[(size_t)row * F + j] = dz;
                            dzc[(size_t)j * bp + row] = dz;
                            cb[i] += dz;
                            cg[i] += dp[u][i] * xh[u][i];
                            cbe[i] += dp[u][i];
                        }
                    }
                }
            }
        }
        // the four row groups of the wave (lanes l, l ^ 16, l ^ 32, l ^ 48), one fixed order
#pragma unroll
        for (int i = 0; i < C; ++i) {
            cb[i] += __shfl_xor(cb[i], 16, 64);
            cb[i] += __shfl_xor(cb[i], 32, 64);
            if (L.ln == 2) {
                cg[i] += __shfl_xor(cg[i], 16, 64);
                cg[i] += __shfl_xor(cg[i], 32, 64);
                cbe[i] += __shfl_xor(cbe[i], 16, 64);
                cbe[i] += __shfl_xor(cbe[i], 32, 64);
            }
        }
        if (rq == 0) {
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const int j = sub + 16 * i;
                if (j < F) {
                    colp[wave * F + j] = cb[i];
                    colp[(kGW + wave) * F + j] = cg[i];
                    colp[(2 * kGW + wave) * F + j] = cbe[i];
                }
            }
        }
    } else {
        for (int r0 = 0; r0 < bsz; r0 += 4 * kGW) {
            const int row = r0 + 4 * wave + rq;
            const bool live = row < bsz;
            // d(pre-activation) of column j: dY masked by the ReLU
            auto dpre = [&](int j) {
                const float d = dy[(size_t)row * F + j] + (L.dy2 >= 0 ? base[L.dy2 + (size_t)row * F + j] : 0.f);
                return (!L.relu || base[L.yr + (size_t)row * F + j] > 0.f) ? d : 0.f;
            };
            float m1 = 0.f, m2 = 0.f, rstd = 1.f;
            if (L.ln) {
                float s1 = 0.f, s2 = 0.f;
                if (live)
                    for (int j = sub; j < F; j += 16) {
                        const float dx = L.ln == 2 ? dpre(j) * pr[L.g + j] : dpre(j);
                        s1 += dx;
                        s2 += dx * base[L.xh + (size_t)row * F + j];
                    }
                m1 = row_sum(s1) * invF;
                m2 = row_sum(s2) * invF;
                rstd = live ? base[L.rs + row] : 0.f;
            }
            if (!live) continue;
            for (int j = sub; j < F; j += 16) {
                const float d = dpre(j);
                float dz = d, xh = 0.f;
                if (L.ln) {
                    xh = base[L.xh + (size_t)row * F + j];
                    const float dx = L.ln == 2 ? d * pr[L.g + j] : d;
                    dz = rstd * (dx - m1 - xh * m2);
                }
                put(row, j, d, xh, dz);
            }
        }
    }
}

// words per wave of the output layers' column partials (colo): 32 logits /
// means and the value; the Gaussian head adds its 32 log_std (and a pad word)
// the head of the three learner kernels and their helpers (a compile-time parameter)
enum Head : int { kCat = 0, kGauss = 1, kMulti = 2, kBern = 3 };
template <Head HEAD>
constexpr int kColo = HEAD == kGauss ? 66 : 33;

// loss_sample's coefficients for a minibatch of 1 / inv_b rows
__device__ __forceinline__ LossCoef loss_coef(const GArgs &g, float inv_b, float entp) {
    LossCoef k;
    k.clip = g.clip;
    k.lo = 1.f - g.clip;
    k.hi = 1.f + g.clip;
    k.inv_b = inv_b;
    k.vf = g.vf;
    k.ent = entp;
    k.vf_half_inv_b = g.vf * 0.5f * inv_b;
    k.g_h = -entp * inv_b;
    return k;
}

// The Gaussian head's loss row pass over `bsz` rows of the general form (the
// geometry of the categorical pass in minibatch_grads: 16 lanes per row,
// dimensions sub and sub + 16 per lane, four rows per lane group in flight):
// mean / value / log_std -> d(mean) in both layouts, d(value), and per wave
// the column partials of the output-layer biases and of log_std in colo
// ([kGW][66]: 32 means, the value, 32 log_std).  The row math is gauss_head.h's
// and loss_sample's, as in agx_ppo_gauss_loss_fwd_bwd.
__device__ __forceinline__ void gauss_loss_rows(const GArgs &g, float *base, const float *pr, const float *act_e,
                                                const float *grow_e, long long s0, int bsz, float inv_b, float entp,
                                                float *colo, float &lsum, float &klsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int bp = g.bp, A = g.A;
    const long long S = g.S;
    const GLay &La = g.L[g.aout];
    const GLay &Lc = g.L[g.cout];
    const float *mup = base + La.yr;
    const float *vp = base + Lc.yr;
    float *dla = base + La.dy;
    float *dlac = base + La.dyc;
    float *dlv = base + Lc.dy;
    const int a0 = sub, a1 = sub + 16;
    const bool on0 = a0 < A, on1 = a1 < A;
    const float l0 = pr[g.lso + (on0 ? a0 : 0)], l1 = pr[g.lso + (on1 ? a1 : 0)];
    const float ls0 = on0 ? l0 : 0.f, ls1 = on1 ? l1 : 0.f;
    const float iv0 = gauss_inv_var(ls0), iv1 = gauss_inv_var(ls1);
    const float H = gauss_entropy(A, row_sum(ls0 + ls1));
    const LossCoef k = loss_coef(g, inv_b, entp);
    float cb0 = 0.f, cb1 = 0.f, cbv = 0.f;  // output-layer bias gradients (column partials)
    float gs0 = 0.f, gs1 = 0.f;             // log_std gradients (column partials)
    constexpr int R = 4;
    for (int rb = 0; rb < bsz; rb += R * 4 * kGW) {
        float pmu0[R], pmu1[R], pa0[R], pa1[R], polp[R], pad[R], pret[R], pov[R], pv[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
            const int row = row0 < bsz ? row0 : 0;
            pmu0[u] = mup[(size_t)row * A + (on0 ? a0 : 0)];
            pmu1[u] = mup[(size_t)row * A + (on1 ? a1 : 0)];
            pa0[u] = act_e[(size_t)(s0 + row) * A + (on0 ? a0 : 0)];
            pa1[u] = act_e[(size_t)(s0 + row) * A + (on1 ? a1 : 0)];
            polp[u] = grow_e[s0 + row];
            pad[u] = grow_e[S + s0 + row];
            pret[u] = grow_e[2 * S + s0 + row];
            pov[u] = grow_e[3 * S + s0 + row];
            pv[u] = vp[row];
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
            const bool live = row0 < bsz;
            const int row = live ? row0 : 0;
            const float mu0 = on0 ? pmu0[u] : 0.f, mu1 = on1 ? pmu1[u] : 0.f;
            const float av0 = on0 ? pa0[u] : 0.f, av1 = on1 ? pa1[u] : 0.f;
            const float lp = row_sum((on0 ? gauss_logp_term(av0, mu0, ls0) : 0.f) +
                                     (on1 ? gauss_logp_term(av1, mu1, ls1) : 0.f));
            float gl, gv;
            Acc one;
            loss_sample(lp, polp[u], pad[u], pret[u], pov[u], pv[u], H, k, gl, gv, one);
            if (live) {
                const float z0 = av0 - mu0, z1 = av1 - mu1;
                if (on0) {
                    const float d0 = gauss_g_mean(gl, z0, iv0);
                    dla[(size_t)row * A + a0] = d0;
                    dlac[(size_t)a0 * bp + row] = d0;
                    cb0 += d0;
                    gs0 += gauss_g_log_std(gl, z0, iv0);
                }
                if (on1) {
                    const float d1 = gauss_g_mean(gl, z1, iv1);
                    dla[(size_t)row * A + a1] = d1;
                    dlac[(size_t)a1 * bp + row] = d1;
                    cb1 += d1;
                    gs1 += gauss_g_log_std(gl, z1, iv1);
                }
                if (sub == 0) {
                    dlv[row] = gv;
                    cbv += gv;
                    lsum += (one.pg + g.vf * 0.5f * one.vl - entp * H) * inv_b;
                    klsum += one.kl * inv_b;  // approx_kl (ppo.py:899-902)
                }
            }
        }
    }
    // the wave's four row groups, then per wave into LDS (the caller sums the waves in order)
    cb0 += __shfl_xor(cb0, 16, 64);
    cb0 += __shfl_xor(cb0, 32, 64);
    cb1 += __shfl_xor(cb1, 16, 64);
    cb1 += __shfl_xor(cb1, 32, 64);
    cbv += __shfl_xor(cbv, 16, 64);
    cbv += __shfl_xor(cbv, 32, 64);
    gs0 += __shfl_xor(gs0, 16, 64);
    gs0 += __shfl_xor(gs0, 32, 64);
    gs1 += __shfl_xor(gs1, 16, 64);
    gs1 += __shfl_xor(gs1, 32, 64);
    if (rq == 0) {
        float *co = colo + wave * kColo<kGauss>;
        co[a0] = cb0;
        co[a1] = cb1;
        if (sub == 0) co[32] = cbv;
        co[33 + a0] = gs0;
        co[33 + a1] = gs1;
    }
}

// ---- the multi-categorical head (include/agx_multi.h) ---------------------
constexpr float kSegOut = -3.0e38f;  // a lane outside the component (or past L) in a maximum

// component k's size n_k (wave-uniform: the head is a kernel argument)
__device__ __forceinline__ int multi_n(const GArgs &g, int k) {
    return (int)((g.mn[k >> 2] >> (8 * (k & 3))) & 0xffu);
}

// What the component walk leaves of a row.  Every lane of the row: its
// log-prob and entropy, summed over the components in ascending k.  Of the
// lane's two logits (each in exactly one component): p, gh = -(log(p + 1e-8) +
// p / (p + 1e-8)) and pg = sum p gh over the logit's own component.
struct MultiRow {
    float lp = 0.f, H = 0.f;
    float p0 = 0.f, p1 = 0.f, gh0 = 0.f, gh1 = 0.f, pg0 = 0.f, pg1 = 0.f;
};

// Component k of a row: in0 / in1, the lane's logits (masked: -1e8) inside the
// component; t0 / t1, the logit is the stored choice.  The categorical pass's
// float operations in its order, with the lanes outside the component neutral
// (multi_policy.hip's seg_lse); the chosen logit comes from a row maximum over
// the one lane holding it (exact) in place of the categorical pass's bpermute.
__device__ __forceinline__ void multi_component(int k, bool in0, bool in1, float lg0, float lg1, bool t0, bool t1,
                                                MultiRow &r) {
    const float mx = row_max(fmaxf(in0 ? lg0 : kSegOut, in1 ? lg1 : kSegOut));
    const float ex0 = in0 ? expf(lg0 - mx) : 0.f, ex1 = in1 ? expf(lg1 - mx) : 0.f;
    const float lse = mx + logf(row_sum(ex0 + ex1));
    const float p0 = in0 ? expf(lg0 - lse) : 0.f, p1 = in1 ? expf(lg1 - lse) : 0.f;
    const float lpe0 = logf(p0 + 1e-8f), lpe1 = logf(p1 + 1e-8f);
    const float Hk = -row_sum((in0 ? p0 * lpe0 : 0.f) + (in1 ? p1 * lpe1 : 0.f));
    const float gh0 = -(lpe0 + p0 / (p0 + 1e-8f)), gh1 = -(lpe1 + p1 / (p1 + 1e-8f));
    const float pg = row_sum((in0 ? p0 * gh0 : 0.f) + (in1 ? p1 * gh1 : 0.f));
    const float lga = row_max(fmaxf((in0 && t0) ? lg0 : kSegOut, (in1 && t1) ? lg1 : kSegOut));
    const float lpk = lga - lse;
    r.lp = k == 0 ? lpk : r.lp + lpk;  // ascending k
    r.H = k == 0 ? Hk : r.H + Hk;
    if (in0) {
        r.p0 = p0;
        r.gh0 = gh0;
        r.pg0 = pg;
    }
    if (in1) {
        r.p1 = p1;
        r.gh1 = gh1;
        r.pg1 = pg;
    }
}

// component k's results c (multi_component from a fresh MultiRow) into the row's
__device__ __forceinline__ void multi_merge(int k, bool in0, bool in1, const MultiRow &c, MultiRow &r) {
    r.lp = k == 0 ? c.lp : r.lp + c.lp;  // ascending k
    r.H = k == 0 ? c.H : r.H + c.H;
    if (in0) {
        r.p0 = c.p0;
        r.gh0 = c.gh0;
        r.pg0 = c.pg0;
    }
    if (in1) {
        r.p1 = c.p1;
        r.gh1 = c.gh1;
        r.pg1 = c.pg1;
    }
}

// The row's clipped surrogate, value loss and approx-KL from its log-prob and
// entropy, and the gradients of the lane's two logits and of the value: the
// categorical pass's operations (tie and closed-interval rules included).
struct MultiOut {
    float dl0, dl1, dvv, loss, kl;
};
__device__ __forceinline__ MultiOut multi_row_loss(const GArgs &g, const MultiRow &r, bool t0, bool t1, float olp,
                                                   float Ad, float Rt, float ov, float v, float inv_b, float entp) {
    const float logp = r.lp, Hs = r.H;
    const float lo = 1.f - g.clip, hi = 1.f + g.clip;
    const float lrt = logp - olp;
    const float ratio = expf(lrt);
    const float rcl = fminf(fmaxf(ratio, lo), hi);
    const float q1 = -Ad * ratio, q2 = -Ad * rcl;
    const float g1 = q1 > q2 ? 1.f : (q1 == q2 ? 0.5f : 0.f);
    const float g2 = q2 > q1 ? 1.f : (q1 == q2 ? 0.5f : 0.f);
    const float inr = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
    const float g_logp = ((g1 * -Ad + g2 * -Ad * inr) * inv_b) * ratio;
    const float dv = v - ov;
    const float vcl = ov + fminf(fmaxf(dv, -g.clip), g.clip);
    const float eu = v - Rt, ec = vcl - Rt;
    const float lu = eu * eu, lc = ec * ec;
    const float gu = lu > lc ? 1.f : (lu == lc ? 0.5f : 0.f);
    const float gc = lc > lu ? 1.f : (lu == lc ? 0.5f : 0.f);
    const float inv = (dv >= -g.clip && dv <= g.clip) ? 1.f : 0.f;
    const float g_H = -entp * inv_b;
    MultiOut o;
    o.dl0 = g_logp * ((t0 ? 1.f : 0.f) - r.p0) + g_H * r.p0 * (r.gh0 - r.pg0);
    o.dl1 = g_logp * ((t1 ? 1.f : 0.f) - r.p1) + g_H * r.p1 * (r.gh1 - r.pg1);
    o.dvv = g.vf * 0.5f * inv_b * (gu * 2.f * eu + gc * 2.f * ec * inv);
    o.loss = (fmaxf(q1, q2) + g.vf * 0.5f * fmaxf(lu, lc) - entp * Hs) * inv_b;
    o.kl = ((ratio - 1.f) - lrt) * inv_b;  // approx_kl (ppo.py:899-902)
    return o;
}

// The multi-categorical head's loss row pass over `bsz` rows of the general
// form: the categorical pass's geometry in minibatch_grads (16 lanes per row,
// flat logits sub and sub + 16 per lane, four rows per lane group in flight)
// and its outputs (d(logits) in both layouts, d(value), the output-layer bias
// column partials in colo, [kGW][33]).  tgt_e: the rows' target words.
__device__ __forceinline__ void multi_loss_rows(const GArgs &g, float *base, const unsigned *tgt_e,
                                                const unsigned *gmask_e, const float *grow_e, long long s0, int bsz,
                                                float inv_b, float entp, float *colo, float &lsum, float &klsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int bp = g.bp, A = g.A, K = g.mk;
    const long long S = g.S;
    const GLay &La = g.L[g.aout];
    const GLay &Lc = g.L[g.cout];
    const float *lgp = base + La.yr;
    const float *vp = base + Lc.yr;
    float *dla = base + La.dy;
    float *dlac = base + La.dyc;
    float *dlv = base + Lc.dy;
    const int a0 = sub, a1 = sub + 16;
    float cb0 = 0.f, cb1 = 0.f, cbv = 0.f;  // output-layer bias gradients (column partials)
    constexpr int R = 4;
    for (int rb = 0; rb < bsz; rb += R * 4 * kGW) {
        unsigned pbits[R], ptgt[R];
        float plg0[R], plg1[R], polp[R], pad[R], pret[R], pov[R], pv[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
            const int row = row0 < bsz ? row0 : 0;
            pbits[u] = gmask_e ? gmask_e[s0 + row] : 0xffffffffu;
            plg0[u] = lgp[(size_t)row * A + (a0 < A ? a0 : 0)];
            plg1[u] = lgp[(size_t)row * A + (a1 < A ? a1 : 0)];
            ptgt[u] = tgt_e[s0 + row];
            polp[u] = grow_e[s0 + row];
            pad[u] = grow_e[S + s0 + row];
            pret[u] = grow_e[2 * S + s0 + row];
            pov[u] = grow_e[3 * S + s0 + row];
            pv[u] = vp[row];
        }
        float lg0[R], lg1[R];
        bool t0[R], t1[R];
        MultiRow mr[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const bool ok0 = (pbits[u] >> a0) & 1u, ok1 = (pbits[u] >> a1) & 1u;
            lg0[u] = a0 < A ? (ok0 ? plg0[u] : -1.0e8f) : kSegOut;
            lg1[u] = a1 < A ? (ok1 ? plg1[u] : -1.0e8f) : kSegOut;
            t0[u] = (ptgt[u] >> a0) & 1u;
            t1[u] = (ptgt[u] >> a1) & 1u;
        }
        int off = 0;
        for (int k = 0; k < K; ++k) {  // wave-uniform: K and the sizes are kernel arguments
            const int n = multi_n(g, k);
            const bool in0 = a0 >= off && a0 < off + n, in1 = a1 >= off && a1 < off + n;
#pragma unroll
            for (int u = 0; u < R; ++u) multi_component(k, in0, in1, lg0[u], lg1[u], t0[u], t1[u], mr[u]);
            off += n;
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
            const bool live = row0 < bsz;
            const int row = live ? row0 : 0;
            const bool ok0 = (pbits[u] >> a0) & 1u, ok1 = (pbits[u] >> a1) & 1u;
            const MultiOut o =
                multi_row_loss(g, mr[u], t0[u], t1[u], polp[u], pad[u], pret[u], pov[u], pv[u], inv_b, entp);
            if (live) {
                const float d0 = ok0 ? o.dl0 : 0.f, d1 = ok1 ? o.dl1 : 0.f;
                if (a0 < A) {
                    dla[(size_t)row * A + a0] = d0;
                    dlac[(size_t)a0 * bp + row] = d0;
                    cb0 += d0;
                }
                if (a1 < A) {
                    dla[(size_t)row * A + a1] = d1;
                    dlac[(size_t)a1 * bp + row] = d1;
                    cb1 += d1;
                }
                if (sub == 0) {
                    dlv[row] = o.dvv;
                    cbv += o.dvv;
                    lsum += o.loss;
                    klsum += o.kl;
                }
            }
        }
    }
    // bias gradients of the output layers: the wave's four row groups, then
    // per wave into LDS (the caller sums the waves in order)
    cb0 += __shfl_xor(cb0, 16, 64);
    cb0 += __shfl_xor(cb0, 32, 64);
    cb1 += __shfl_xor(cb1, 16, 64);
    cb1 += __shfl_xor(cb1, 32, 64);
    cbv += __shfl_xor(cbv, 16, 64);
    cbv += __shfl_xor(cbv, 32, 64);
    if (rq == 0) {
        colo[wave * 33 + a0] = cb0;
        colo[wave * 33 + a1] = cb1;
        if (sub == 0) colo[wave * 33 + 32] = cbv;
    }
}

// ---- the Bernoulli head (include/agx_bernoulli.h) --------------------------
// One row of the Bernoulli pass: the lane's two logits (masked: -1e8; past n:
// off) and target bits -> the gradients of the lane's logits and of the value
// and the row's loss / approx_kl terms (bern_head.h's and loss_sample's math, as
// in agx_ppo_bern_loss_fwd_bwd).  Two row sums, whatever n is.
struct BernRowOut {
    float dl0, dl1, dvv, loss, kl;
};
__device__ __forceinline__ BernRowOut bern_row_loss(const GArgs &g, const LossCoef &k, bool on0, bool on1, float lg0,
                                                    float lg1, bool t0, bool t1, float olp, float Ad, float Rt,
                                                    float ov, float v, float inv_b, float entp) {
    const BernBit b0 = bern_bit(lg0), b1 = bern_bit(lg1);
    const float lp = row_sum((on0 ? (t0 ? b0.lp : b0.lq) : 0.f) + (on1 ? (t1 ? b1.lp : b1.lq) : 0.f));
    const float H = -row_sum((on0 ? bern_neg_entropy(b0) : 0.f) + (on1 ? bern_neg_entropy(b1) : 0.f));
    float gl, gv;
    Acc one;
    loss_sample(lp, olp, Ad, Rt, ov, v, H, k, gl, gv, one);
    BernRowOut o;
    o.dl0 = gl * bern_dlogp(b0, t0) + k.g_h * bern_dH(b0);
    o.dl1 = gl * bern_dlogp(b1, t1) + k.g_h * bern_dH(b1);
    o.dvv = gv;
    o.loss = (one.pg + g.vf * 0.5f * one.vl - entp * H) * inv_b;
    o.kl = one.kl * inv_b;  // approx_kl (ppo.py:899-902)
    return o;
}

// The Bernoulli head's loss row pass over `bsz` rows of the general form: the
// categorical pass's geometry in minibatch_grads (16 lanes per row, bits sub
// and sub + 16 per lane, four rows per lane group in flight) and its outputs
// (d(logits) in both layouts, d(value), the output-layer bias column partials
// in colo, [kGW][33]).  tgt_e: the rows' target words (bit j = a_j != 0).
__device__ __forceinline__ void bern_loss_rows(const GArgs &g, float *base, const unsigned *tgt_e,
                                               const unsigned *gmask_e, const float *grow_e, long long s0, int bsz,
                                               float inv_b, float entp, float *colo, float &lsum, float &klsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int bp = g.bp, A = g.A;
    const long long S = g.S;
    const GLay &La = g.L[g.aout];
    const GLay &Lc = g.L[g.cout];
    const float *lgp = base + La.yr;
    const float *vp = base + Lc.yr;
    float *dla = base + La.dy;
    float *dlac = base + La.dyc;
    float *dlv = base + Lc.dy;
    const int a0 = sub, a1 = sub + 16;
    const bool on0 = a0 < A, on1 = a1 < A;
    const LossCoef k = loss_coef(g, inv_b, entp);
    float cb0 = 0.f, cb1 = 0.f, cbv = 0.f;  // output-layer bias gradients (column partials)
    constexpr int R = 4;
    for (int rb = 0; rb < bsz; rb += R * 4 * kGW) {
        unsigned pbits[R], ptgt[R];
        float plg0[R], plg1[R], polp[R], pad[R], pret[R], pov[R], pv[R];
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
            const int row = row0 < bsz ? row0 : 0;
            pbits[u] = gmask_e ? gmask_e[s0 + row] : 0xffffffffu;
            plg0[u] = lgp[(size_t)row * A + (on0 ? a0 : 0)];
            plg1[u] = lgp[(size_t)row * A + (on1 ? a1 : 0)];
            ptgt[u] = tgt_e[s0 + row];
            polp[u] = grow_e[s0 + row];
            pad[u] = grow_e[S + s0 + row];
            pret[u] = grow_e[2 * S + s0 + row];
            pov[u] = grow_e[3 * S + s0 + row];
            pv[u] = vp[row];
        }
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
            const bool live = row0 < bsz;
            const int row = live ? row0 : 0;
            const bool ok0 = (pbits[u] >> a0) & 1u, ok1 = (pbits[u] >> a1) & 1u;
            const float lg0 = on0 ? (ok0 ? plg0[u] : -1.0e8f) : 0.f;
            const float lg1 = on1 ? (ok1 ? plg1[u] : -1.0e8f) : 0.f;
            const bool t0 = (ptgt[u] >> a0) & 1u, t1 = (ptgt[u] >> a1) & 1u;
            const BernRowOut o =
                bern_row_loss(g, k, on0, on1, lg0, lg1, t0, t1, polp[u], pad[u], pret[u], pov[u], pv[u], inv_b, entp);
            if (live) {
                const float d0 = ok0 ? o.dl0 : 0.f, d1 = ok1 ? o.dl1 : 0.f;
                if (on0) {
                    dla[(size_t)row * A + a0] = d0;
                    dlac[(size_t)a0 * bp + row] = d0;
                    cb0 += d0;
                }
                if (on1) {
                    dla[(size_t)row * A + a1] = d1;
                    dlac[(size_t)a1 * bp + row] = d1;
                    cb1 += d1;
                }
                if (sub == 0) {
                    dlv[row] = o.dvv;
                    cbv += o.dvv;
                    lsum += o.loss;
                    klsum += o.kl;
                }
            }
        }
    }
    // bias gradients of the output layers: the wave's four row groups, then
    // per wave into LDS (the caller sums the waves in order)
    cb0 += __shfl_xor(cb0, 16, 64);
    cb0 += __shfl_xor(cb0, 32, 64);
    cb1 += __shfl_xor(cb1, 16, 64);
    cb1 += __shfl_xor(cb1, 32, 64);
    cbv += __shfl_xor(cbv, 16, 64);
    cbv += __shfl_xor(cbv, 32, 64);
    if (rq == 0) {
        colo[wave * 33 + a0] = cb0;
        colo[wave * 33 + a1] = cb1;
        if (sub == 0) colo[wave * 33 + 32] = cbv;
    }
}

// One minibatch's forward, PPO loss and backward over `bsz` rows (rows
// s0 .. s0 + bsz - 1 of the epoch's minibatch-ordered rollout, observations at
// xobs), accumulating the gradient row G (every entry written: dW by GEMM
// epilogues, bias / LN-affine sums by the column passes) and the loss / approx_kl
// partial sums.  inv_b = 1 / the whole minibatch's size (the loss is a mean over
// it).  base: this workgroup's activation scratch; wb: where the transposed
// weights live (wb + L.wt).  Shared by the one-workgroup-per-agent learner and
// the partnered one (each partner over its slice of the rows).
// kGauss: gact_e holds the rows' float actions [A]; kMulti: the rows' target words
// (multi_loss_rows); kBern: the rows' target words (bern_loss_rows); colo has
// kColo<HEAD> words per wave.
template <Head HEAD>
__device__ __forceinline__ void minibatch_grads(const GArgs &g, float *base, const float *wb, const float *pr, float *G,
                                                const float *xobs, const int *gact_e, const unsigned *gmask_e,
                                                const float *grow_e, long long s0, int bsz, float inv_b, float entp,
                                                float *lds, float *colp, float *colo, float &lsum, float &klsum,
                                                long long *st = nullptr) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int bp = g.bp, A = g.A, D = g.D;
    const long long S = g.S;
    (void)wave;
    // observation, feature-major (the first layer's dW operand)
    for (int i = tid; i < bsz * D; i += kGT) {
        const int b = i / D, d = i - b * D;
        base[g.oc + (size_t)d * bp + b] = xobs[i];
    }

    // ---- forward, layer by layer ------------------------------------
    if (st) st[0] = (long long)__builtin_readcyclecounter();
    forward_layers(g.L, g.nl, xobs, bsz, base, pr, bp, lds, g.dbg, st);

    // ---- loss row pass: logits / value -> d(logits), d(value) (ppo.py:876-908)
    if constexpr (HEAD == kGauss) {
        if (!(g.dbg & 8))
            gauss_loss_rows(g, base, pr, reinterpret_cast<const float *>(gact_e), grow_e, s0, bsz, inv_b, entp, colo,
                            lsum, klsum);
    } else if constexpr (HEAD == kMulti) {
        if (!(g.dbg & 8))
            multi_loss_rows(g, base, reinterpret_cast<const unsigned *>(gact_e), gmask_e, grow_e, s0, bsz, inv_b, entp,
                            colo, lsum, klsum);
    } else if constexpr (HEAD == kBern) {
        if (!(g.dbg & 8))
            bern_loss_rows(g, base, reinterpret_cast<const unsigned *>(gact_e), gmask_e, grow_e, s0, bsz, inv_b, entp,
                           colo, lsum, klsum);
    } else if (!(g.dbg & 8)) {
        const GLay &La = g.L[g.aout];
        const GLay &Lc = g.L[g.cout];
        const float *lgp = base + La.yr;
        const float *vp = base + Lc.yr;
        float *dla = base + La.dy;
        float *dlac = base + La.dyc;
        float *dlv = base + Lc.dy;
        const int a0 = sub, a1 = sub + 16;
        float cb0 = 0.f, cb1 = 0.f, cbv = 0.f;  // output-layer bias gradients (column partials)
        // four rows per 16-lane group at once: every input of the 128-row
        // block is loaded before the first reduction
        constexpr int R = 4;
        for (int rb = 0; rb < bsz; rb += R * 4 * kGW) {
            unsigned pbits[R];
            int pact[R];
            float plg0[R], plg1[R], polp[R], pad[R], pret[R], pov[R], pv[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
                const int row = row0 < bsz ? row0 : 0;
                pbits[u] = gmask_e ? gmask_e[s0 + row] : 0xffffffffu;
                plg0[u] = lgp[(size_t)row * A + (a0 < A ? a0 : 0)];
                plg1[u] = lgp[(size_t)row * A + (a1 < A ? a1 : 0)];
                pact[u] = gact_e[s0 + row];
                polp[u] = grow_e[s0 + row];
                pad[u] = grow_e[S + s0 + row];
                pret[u] = grow_e[2 * S + s0 + row];
                pov[u] = grow_e[3 * S + s0 + row];
                pv[u] = vp[row];
            }
#pragma unroll
            for (int u = 0; u < R; ++u) {
            const int row0 = rb + 4 * wave + rq + 4 * kGW * u;
            const bool live = row0 < bsz;
            const int row = live ? row0 : 0;
            const unsigned bits = pbits[u];
            const bool ok0 = (bits >> a0) & 1u, ok1 = (bits >> a1) & 1u;
            const float lg0 = a0 < A ? (ok0 ? plg0[u] : -1.0e8f) : -3.0e38f;
            const float lg1 = a1 < A ? (ok1 ? plg1[u] : -1.0e8f) : -3.0e38f;
            const float mx = row_max(fmaxf(lg0, lg1));
            const float ex0 = a0 < A ? expf(lg0 - mx) : 0.f, ex1 = a1 < A ? expf(lg1 - mx) : 0.f;
            const float lse = mx + logf(row_sum(ex0 + ex1));
            const float p0 = a0 < A ? expf(lg0 - lse) : 0.f, p1 = a1 < A ? expf(lg1 - lse) : 0.f;
            const float lpe0 = logf(p0 + 1e-8f), lpe1 = logf(p1 + 1e-8f);
            const float Hs = -row_sum((a0 < A ? p0 * lpe0 : 0.f) + (a1 < A ? p1 * lpe1 : 0.f));
            const float gh0 = -(lpe0 + p0 / (p0 + 1e-8f)), gh1 = -(lpe1 + p1 / (p1 + 1e-8f));
            const float pg = row_sum((a0 < A ? p0 * gh0 : 0.f) + (a1 < A ? p1 * gh1 : 0.f));
            const int a_t = pact[u];
            const int srcl = (lane & ~15) + (a_t & 15);
            const float t0 = bperm(srcl, lg0), t1 = bperm(srcl, lg1);
            const float logp = (a_t < 16 ? t0 : t1) - lse;
            const float olp = polp[u], Ad = pad[u], Rt = pret[u], ov = pov[u];
            const float lo = 1.f - g.clip, hi = 1.f + g.clip;
            const float lrt = logp - olp;
            const float ratio = expf(lrt);
            const float rcl = fminf(fmaxf(ratio, lo), hi);
            const float q1 = -Ad * ratio, q2 = -Ad * rcl;
            const float g1 = q1 > q2 ? 1.f : (q1 == q2 ? 0.5f : 0.f);
            const float g2 = q2 > q1 ? 1.f : (q1 == q2 ? 0.5f : 0.f);
            const float inr = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
            const float g_logp = ((g1 * -Ad + g2 * -Ad * inr) * inv_b) * ratio;
            const float v = pv[u];
            const float dv = v - ov;
            const float vcl = ov + fminf(fmaxf(dv, -g.clip), g.clip);
            const float eu = v - Rt, ec = vcl - Rt;
            const float lu = eu * eu, lc = ec * ec;
            const float gu = lu > lc ? 1.f : (lu == lc ? 0.5f : 0.f);
            const float gc = lc > lu ? 1.f : (lu == lc ? 0.5f : 0.f);
            const float inv = (dv >= -g.clip && dv <= g.clip) ? 1.f : 0.f;
            const float g_H = -entp * inv_b;
            const float dl0 = g_logp * ((a0 == a_t ? 1.f : 0.f) - p0) + g_H * p0 * (gh0 - pg);
            const float dl1 = g_logp * ((a1 == a_t ? 1.f : 0.f) - p1) + g_H * p1 * (gh1 - pg);
            if (live) {
                const float d0 = ok0 ? dl0 : 0.f, d1 = ok1 ? dl1 : 0.f;
                if (a0 < A) {
                    dla[(size_t)row * A + a0] = d0;
                    dlac[(size_t)a0 * bp + row] = d0;
                    cb0 += d0;
                }
                if (a1 < A) {
                    dla[(size_t)row * A + a1] = d1;
                    dlac[(size_t)a1 * bp + row] = d1;
                    cb1 += d1;
                }
                if (sub == 0) {
                    const float dvv = g.vf * 0.5f * inv_b * (gu * 2.f * eu + gc * 2.f * ec * inv);
                    dlv[row] = dvv;
                    cbv += dvv;
                    lsum += (fmaxf(q1, q2) + g.vf * 0.5f * fmaxf(lu, lc) - entp * Hs) * inv_b;
                    klsum += ((ratio - 1.f) - lrt) * inv_b;  // approx_kl (ppo.py:899-902)
                }
            }
            }
        }
        // bias gradients of the output layers: the wave's four row groups,
        // then per wave into LDS (summed over the waves in order below)
        cb0 += __shfl_xor(cb0, 16, 64);
        cb0 += __shfl_xor(cb0, 32, 64);
        cb1 += __shfl_xor(cb1, 16, 64);
        cb1 += __shfl_xor(cb1, 32, 64);
        cbv += __shfl_xor(cbv, 16, 64);
        cbv += __shfl_xor(cbv, 32, 64);
        if (rq == 0) {
            colo[wave * 33 + a0] = cb0;
            colo[wave * 33 + a1] = cb1;
            if (sub == 0) colo[wave * 33 + 32] = cbv;
        }
    }
    __syncthreads();
    if (!(g.dbg & 8) && tid <= A) {
        float sb = 0.f;
        for (int w = 0; w < kGW; ++w) sb += colo[w * kColo<HEAD> + (tid < A ? tid : 32)];
        G[tid < A ? g.L[g.aout].b + tid : g.L[g.cout].b] = sb;
    }
    if constexpr (HEAD == kGauss) {
        // d(log_std): the waves' partials in order, and the entropy's -ent_coef / b per row of the slice
        const int d = tid - kWave;
        if (!(g.dbg & 8) && d >= 0 && d < A) {
            float sg = 0.f;
            for (int w = 0; w < kGW; ++w) sg += colo[w * kColo<HEAD> + 33 + d];
            G[g.lso + d] = sg + (-entp * inv_b) * (float)bsz;
        }
    }
    if (st) st[17] = (long long)__builtin_readcyclecounter();

    // ---- backward, layer by layer (reverse) ----------------------------
    float *t1c = base + g.t1, *t2c = base + g.t2;
    for (int l = g.nl - 1; l >= 0; --l) {
        const GLay &L = g.L[l];
        const int F = L.fout;
        float *dzr = base + ((l & 1) ? g.dzr1 : g.dzr), *dzc = base + ((l & 1) ? g.dzc1 : g.dzc);
        float *colp_l = colp + (l & 1) * 3 * kGW * 128;
        // output layers: the loss pass wrote dZ in both layouts and the bias gradient;
        // fused layers: the consumer's dX epilogue wrote dZ and the column partials
        const bool outl = L.dyc >= 0;
        // dY -> dZ through ReLU and LayerNorm(+affine)
        if (!(g.dbg & 8) && !outl && !L.fused) {
            if (F <= 128) bwd_rows<8>(L, base, pr, bsz, bp, dzr, dzc, t1c, t2c, colp_l);
            else bwd_rows<0>(L, base, pr, bsz, bp, dzr, dzc, t1c, t2c);
        }
        if (!outl && !L.fused) __syncthreads();
        if (st) st[18 + 3 * l] = (long long)__builtin_readcyclecounter();
        // bias / LN-affine gradients: column sums over the rows (fixed order);
        // up to 8 feature groups summed before the first store
        if (F <= 128 && !(g.dbg & 24) && !outl) {  // the row pass left per-wave partials in LDS
            for (int o = tid; o < F; o += kGT) {
                float sb = 0.f, sg = 0.f, sbe = 0.f;
                for (int w = 0; w < kGW; ++w) {
                    sb += colp_l[w * F + o];
                    sg += colp_l[(kGW + w) * F + o];
                    sbe += colp_l[(2 * kGW + w) * F + o];
                }
                G[L.b + o] = sb;
                if (L.ln == 2) {
                    G[L.g + o] = sg;
                    G[L.be + o] = sbe;
                }
            }
        }
        for (int ob = 0; ob < ((g.dbg & 16) || F <= 128 || outl ? 0 : F); ob += 8 * 4 * kGW) {
            float rb_[8], rg_[8], rbe_[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int o = ob + 4 * kGW * k + 4 * wave + rq;
                const bool on = o < F;
                float sb = 0.f, sg = 0.f, sbe = 0.f;
                if (ob + 4 * kGW * k < F) {  // wave-uniform
                    for (int b = sub; b < bsz; b += 16) {
                        const size_t x = (size_t)(on ? o : 0) * bp + b;
                        const float v0 = dzc[x];
                        sb += on ? v0 : 0.f;
                        if (L.ln == 2) {
                            const float v1 = t1c[x], v2 = t2c[x];
                            sg += on ? v1 : 0.f;
                            sbe += on ? v2 : 0.f;
                        }
                    }
                }
                rb_[k] = row_sum(sb);
                rg_[k] = L.ln == 2 ? row_sum(sg) : 0.f;
                rbe_[k] = L.ln == 2 ? row_sum(sbe) : 0.f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int o = ob + 4 * kGW * k + 4 * wave + rq;
                if (o < F && sub == 0) {
                    G[L.b + o] = rb_[k];
                    if (L.ln == 2) {
                        G[L.g + o] = rg_[k];
                        G[L.be + o] = rbe_[k];
                    }
                }
            }
        }
        // dW = dZ^T X (contraction over the rows), then dX = dZ W into the
        // source's dY (one GEMM call site for both: instruction-cache footprint)
        const float *xc = L.src < 0 ? base + g.oc : base + g.L[L.src].yc;
        const int fin = L.fin;
        for (int job = 0; job < (L.src >= 0 ? 2 : 1); ++job) {
            if (job) __syncthreads();  // the dW GEMM's last panels are still being read
            if (st && job) st[19 + 3 * l] = (long long)__builtin_readcyclecounter();
            if (g.dbg & (job ? 4 : 2)) continue;
            const float *ga = job ? (outl ? base + L.dy : dzr) : (outl ? base + L.dyc : dzc);
            const float *gb = job ? wb + L.wt : xc;
            const int lda = job ? F : bp, ldb = job ? F : bp;
            const int M = job ? bsz : F, K = job ? F : bsz;
            float *dst = job ? base + (L.acc ? g.L[L.src].dy2 : g.L[L.src].dy) : G + L.w;
            if (job && L.fuse) {  // the source's dZ (other parity) from the epilogue
                const int s_ = L.src;
                gemm_nt<2>(ga, lda, gb, ldb, M, fin, K, lds, nullptr, [](int, int, float) {}, g.L[s_], base, pr,
                           bp, base + ((s_ & 1) ? g.dzr1 : g.dzr), base + ((s_ & 1) ? g.dzc1 : g.dzc),
                           colp + (s_ & 1) * 3 * kGW * 128);
            } else {
                gemm_nt<0>(ga, lda, gb, ldb, M, fin, K, lds, nullptr,
                                   [&](int m, int n, float c) { dst[(size_t)m * fin + n] = c; }, L);
            }
        }
        __syncthreads();
        if (st) st[20 + 3 * l] = (long long)__builtin_readcyclecounter();
    }

}

template <Head HEAD>
__global__ __launch_bounds__(kGT) void ppo_learn_graph_kernel(const GArgs g) {
    __shared__ float red[2 * kGW];
    __shared__ __attribute__((aligned(16))) float lds[kGemmLds];
    __shared__ float colp[2 * 3 * kGW * 128];  // per-wave bias / LN-affine column partials (F <= 128), by layer parity
    __shared__ float colo[kGW * kColo<HEAD>];  // per-wave output-layer partials (32 logits + the value; + log_std)
    if (g.skip && __hip_atomic_load(g.skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    float *const pr = g.params + (size_t)p * g.n;
    float *const gm = g.m + (size_t)p * g.n;
    float *const gv = g.v + (size_t)p * g.n;
    float *const base = g.ws + (size_t)p * g.ws_agent;
    float *const G = base + g.gr;
    const int D = g.D;
    const long long S = g.S;

    // transposed weight copies (the dX operand)
    for (int l = 0; l < g.nl; ++l) {
        const GLay &L = g.L[l];
        if (L.wt < 0) continue;
        float *wt = base + L.wt;
        for (int i = tid; i < L.fout * L.fin; i += kGT) {
            const int o = i / L.fin, c = i - o * L.fin;
            wt[(size_t)c * L.fout + o] = pr[L.w + i];
        }
    }
    __syncthreads();

    int Bp = g.batch_p ? g.batch_p[p] : g.B;
    if (Bp > g.B) Bp = g.B;  // the scratch holds g.B rows (the caller's batch: the population's largest)
    const int Ep = g.epochs_p ? g.epochs_p[p] : g.E;
    const float entp = g.ent_p ? g.ent_p[p] : g.ent;
    const int nmb = (int)((S + Bp - 1) / Bp);
    float loss_total = 0.f;
    double kl_total = 0.0;
    int n_done = 0, epochs_done = 0;
    const long long step0 = g.step[p];
    double pb1 = pow((double)g.b1, (double)step0), pb2 = pow((double)g.b2, (double)step0);
    const float lr_p = g.lr[p];

    for (int e = 0; e < Ep; ++e) {
        const size_t ge = (size_t)e * g.P + p;
        const float *gobs_e = g.gobs + ge * S * D;
        const int *gact_e = g.gact + ge * S * (HEAD == kGauss ? g.A : 1);
        const unsigned *gmask_e = g.gmask ? g.gmask + ge * S : nullptr;
        const float *grow_e = g.grow + ge * 4 * S;
        for (int mb = 0; mb < nmb; ++mb) {
            const long long s0 = (long long)mb * Bp;
            const int bsz = (int)((s0 + Bp <= S) ? Bp : S - s0);
            const float inv_b = 1.f / (float)bsz;
            const float *xobs = gobs_e + s0 * D;

            float lsum = 0.f, klsum = 0.f;
            minibatch_grads<HEAD>(g, base, base, pr, G, xobs, gact_e, gmask_e, grow_e, s0, bsz, inv_b, entp, lds,
                                   colp, colo, lsum, klsum);
            // ---- loss / kl, clip, Adam ------------------------------------------
            block_sum2(lsum, klsum, red);
            if (tid == 0) loss_total += lsum;
            kl_total += (double)klsum;
            ++n_done;
            float q0 = 0.f, q1 = 0.f;
            for (int f = tid; f < g.n; f += kGT) {
                const float x = G[f];
                if (f < g.cstart) q0 += x * x;
                else q1 += x * x;
            }
            block_sum2(q0, q1, red);
            const float c0 = g.max_norm > 0.f ? fminf(g.max_norm / (sqrtf(q0) + 1e-6f), 1.f) : 1.f;
            const float c1 = g.max_norm > 0.f ? fminf(g.max_norm / (sqrtf(q1) + 1e-6f), 1.f) : 1.f;
            pb1 *= (double)g.b1;
            pb2 *= (double)g.b2;
            const float bc1 = (float)(1.0 - pb1);
            const float bc2s = (float)sqrt(1.0 - pb2);
            const float step_size = lr_p / bc1;
            const float ob1 = 1.f - g.b1, ob2 = 1.f - g.b2;
            // Adam over each parameter region, four elements per thread per round:
            // all loads of a round issued before its stores (the stores could
            // alias the loads as far as the compiler knows)
            auto adam_region = [&](int f0, int cnt, long long wt, int fin, int fout) {
                constexpr int U = 16;  // elements per thread per round: all loads, then all stores
                for (int i0 = tid; i0 < cnt; i0 += U * kGT) {
                    float gg[U], mm[U], vv[U], pp[U];
#pragma unroll
                    for (int k = 0; k < U; ++k) {
                        const int i = i0 + k * kGT;
                        const int f = f0 + (i < cnt ? i : 0);
                        gg[k] = G[f];
                        mm[k] = gm[f];
                        vv[k] = gv[f];
                        pp[k] = pr[f];
                    }
#pragma unroll
                    for (int k = 0; k < U; ++k) {
                        const int i = i0 + k * kGT;
                        if (i >= cnt) break;
                        const int f = f0 + i;
                        const float gc = gg[k] * (f < g.cstart ? c0 : c1);
                        const float m = mm[k] + ob1 * (gc - mm[k]);
                        const float v = vv[k] * g.b2 + ob2 * gc * gc;
                        const float np = pp[k] - step_size * (m / (sqrtf(v) / bc2s + g.eps));
                        gm[f] = m;
                        gv[f] = v;
                        pr[f] = np;
                        if (wt >= 0) {
                            const int o = i / fin, c = i - o * fin;
                            base[wt + (size_t)c * fout + o] = np;
                        }
                    }
                }
            };
            // regions: per layer W (with its transposed copy), b, LN weight, LN bias
            for (int rg = 0; rg < ((g.dbg & 32) ? 0 : 4 * g.nl); ++rg) {
                const GLay &L = g.L[rg >> 2];
                const int kind = rg & 3;
                if (kind >= 2 && L.ln != 2) continue;
                const int f0 = kind == 0 ? L.w : kind == 1 ? L.b : kind == 2 ? L.g : L.be;
                adam_region(f0, kind == 0 ? L.fout * L.fin : L.fout, kind == 0 ? L.wt : -1, kind == 0 ? L.fin : 1,
                            kind == 0 ? L.fout : 1);
            }
            if constexpr (HEAD == kGauss) {  // log_std: owned by no layer, no transposed copy
                if (!(g.dbg & 32)) adam_region((int)g.lso, g.A, -1, 1, 1);
            }
            __syncthreads();
        }  // minibatches
        ++epochs_done;
        if (g.target_kl > 0.0 && kl_total / (double)n_done > g.target_kl) break;  // ppo.py:917-918
    }  // epochs
    if (tid == 0) {
        if (g.loss_out) g.loss_out[p] = loss_total / ((float)S * (float)Ep);
        if (g.kl_out) g.kl_out[p] = n_done ? (float)(kl_total / (double)n_done) : 0.f;
        if (g.epochs_out) g.epochs_out[p] = epochs_done;
        g.step[p] = step0 + n_done;
    }
}

// ---------------------------------------------------------------------------
// Partnered runtime-shape learner: an agent's minibatch is split over K
// workgroups ("partners", R rows each) that exchange gradients through L2,
// the compiled learner's scheme (learner.hip) on a runtime layer list:
//   1. each partner runs minibatch_grads over its rows into its own slab of
//      the agent's exchange area (partial gradient row + loss / approx_kl);
//   2. barrier 1, then reduce-scatter: partner kk sums the float4 chunks it
//      owns ([kk cs, (kk + 1) cs)) over the K slabs in partner order, keeps the
//      sums in the agent's sum slab and publishes per-wave partial two-group
//      squared norms;
//   3. barrier 2: every partner sums the K x 4 partial norms in one fixed
//      order (identical clip coefficients everywhere) and runs Adam on its own
//      chunks, writing the parameters, both Adam moments and the transposed
//      weight copy (the dX operand, shared by the agent's partners);
//   4. barrier 3 and an agent-scope acquire: the next update's plain loads of
//      the parameters see every partner's chunks.
// The K partners of an agent are placed on one XCD (block b -> agent b % Q,
// partner b / Q, Q a multiple of 8); that is checked at run time from
// HW_REG_XCC_ID, and a split placement publishes with an agent release (the
// L2 write-back) before every ticket.  Barriers are tickets with bounded spins;
// a timeout sets the caller's error word (AGX_LEARN_ERR_TIMEOUT) and the
// partner exits.  An agent's result depends on K (the row split), never on
// which other agents share the launch.
// ---------------------------------------------------------------------------
constexpr int kMaxGK = 16;
constexpr unsigned kGSpinMax = 1u << 23;

__device__ __forceinline__ bool gpart_sync(unsigned *ctr, unsigned target, bool release, unsigned *tmo,
                                           unsigned *err, int *s_ok) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave's stores have left
    __syncthreads();
    if (threadIdx.x == 0) {
        if (release) {  // partners on other XCDs: write this L2's dirty lines back first
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const unsigned before = __hip_atomic_fetch_add(ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned spins = 0;
        int ok = 1;
        while (before + 1u < target && __hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
            __builtin_amdgcn_s_sleep(1);
            if (++spins > kGSpinMax) {
                __hip_atomic_store(tmo, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (err) __hip_atomic_fetch_or(err, AGX_LEARN_ERR_TIMEOUT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ok = 0;
                break;
            }
        }
        *s_ok = ok;
    }
    __syncthreads();
    return *s_ok != 0;
}

// this CU's L1 no longer holds lines other partners have rewritten (the
// parameters after an Adam step): one agent-scope acquire, waited for by the
// whole workgroup before its next plain loads
__device__ __forceinline__ void gpart_acquire() {
    if (threadIdx.x == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
}

// inner stamps of minibatch_grads: [0] forward start, [1 + l] layer l's forward
// done, [17] loss pass done, [18 + 3l] / [19 + 3l] / [20 + 3l] layer l's row pass,
// dW and dX done
constexpr int kGStampsIn = 18 + 3 * kGL;

__device__ __forceinline__ float ld_sc1(const float *p) {
    return __hip_atomic_load(const_cast<float *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// dW[o][i] = sum over the 16 rows of dZ[row][o] X[row][i] (o < F, i < fin)
// straight into the gradient row Gw ([F][fin]); tiles round the waves
__device__ __forceinline__ void few_dw(const float *dZ, int ldz, const float *X, int ldx, int F, int fin, float *Gw) {
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r = lane & 15, q = lane >> 4;
    const int tm = (F + 15) >> 4, tn = (fin + 15) >> 4, nt = tm * tn;
    auto put = [&](int o0, int i0, const f4 &acc) {
        const int i = i0 + r;
        if (i < fin) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int o = o0 + 4 * q + j;
                if (o < F) Gw[o * fin + i] = acc[j];
            }
        }
    };
    // two tiles per pass (t and t + kGW): both tiles' LDS reads in flight,
    // then two independent MFMA chains; each tile's sum order unchanged
    for (int t = wave; t < nt; t += 2 * kGW) {
        const int t2 = t + kGW;
        const bool two = t2 < nt;  // uniform
        const int o0 = (t % tm) << 4, i0 = (t / tm) << 4;
        const int o1 = two ? (t2 % tm) << 4 : o0, i1 = two ? (t2 / tm) << 4 : i0;
        float a[4], b[4], a2[4], b2[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            a[kk] = dZ[(4 * kk + q) * ldz + o0 + r];
            b[kk] = X[(4 * kk + q) * ldx + i0 + r];
            a2[kk] = dZ[(4 * kk + q) * ldz + o1 + r];
            b2[kk] = X[(4 * kk + q) * ldx + i1 + r];
        }
        f4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[kk], b[kk], acc, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2[kk], b2[kk], acc2, 0, 0, 0);
        }
        put(o0, i0, acc);
        if (two) put(o1, i1, acc2);
    }
}

// The backward of few_row_pass for one row: dY -> dZ in place through the
// ReLU mask and the LayerNorm(+affine) backward, dY' (the affine's input
// gradient) to T for the gamma / beta sums; registers as in few_row_pass, the
// same float operations in the same order as the column loops.
template <int M>
__device__ __forceinline__ void few_row_back(float *dy, const float *xh, float *T, const float *S, const LayRow &L,
                                             int F, int row, int sub) {
    const int mp = (F + 15) >> 4;
    float d[M], x[M], ga[M], be[M];
    bool ok[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const int j = sub + 16 * i;
        ok[i] = j < F;
        d[i] = x[i] = ga[i] = be[i] = 0.f;
        if (i < mp) {
            d[i] = dy[j];
            x[i] = xh[j];
            if (L.ln == 2) {
                ga[i] = S[L.af + j];
                be[i] = S[L.af + F + j];
            }
        }
    }
    const float rs = L.ln ? S[L.rs + row] : 1.f;
    float dp[M];
#pragma unroll
    for (int i = 0; i < M; ++i) {
        const float pre = L.ln == 2 ? x[i] * ga[i] + be[i] : x[i];
        dp[i] = (!L.relu || pre > 0.f) ? d[i] : 0.f;
    }
    float m1 = 0.f, m2 = 0.f;
    if (L.ln) {
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < M; ++i) {
            const float dx = dp[i] * (L.ln == 2 ? ga[i] : 1.f);
            s1 = ok[i] ? s1 + dx : s1;
            s2 = ok[i] ? s2 + dx * x[i] : s2;
        }
        const float invF = 1.f / (float)F;
        m1 = row_sum(s1) * invF;
        m2 = row_sum(s2) * invF;
    }
#pragma unroll
    for (int i = 0; i < M; ++i) {
        if (i >= mp) break;  // uniform
        const int j = sub + 16 * i;
        if (L.ln == 2) T[j] = ok[i] ? dp[i] : 0.f;
        const float v = L.ln ? rs * (dp[i] * (L.ln == 2 ? ga[i] : 1.f) - m1 - x[i] * m2) : dp[i];
        dy[j] = ok[i] ? v : 0.f;
    }
}

// The Gaussian head's loss row pass of the few-row form: the lane group's row
// (4 wave + rq) of the partner's rk <= 16 rows, gauss_loss_rows' math per
// element.  d(mean) / d(value) go to the output layers' dY tiles (zero past the
// slice); the row's d(log_std) terms overwrite its means in the actor output's
// Y tile, which nothing reads after this pass (the caller sums them over the
// 16 rows in row order).
__device__ __forceinline__ void few_gauss_loss_rows(const GArgs &g, float *S, const float *pr, const float *act_e,
                                                    const float *grow_e, long long s0, int rk, float inv_b, float entp,
                                                    float &lsum, float &klsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int row = 4 * wave + rq;
    const int A = g.A;
    const long long S_ = g.S;
    const GLay &La = g.L[g.aout];
    const GLay &Lc = g.L[g.cout];
    float *mup = S + La.yr + row * La.ld;
    float *dla = S + La.dy + row * La.ld;
    const bool live = row < rk;
    const int rr = live ? row : 0;
    const int a0 = sub, a1 = sub + 16;
    const bool on0 = a0 < A, on1 = a1 < A;
    const float l0 = pr[g.lso + (on0 ? a0 : 0)], l1 = pr[g.lso + (on1 ? a1 : 0)];
    const float pa0 = act_e[(size_t)(s0 + rr) * A + (on0 ? a0 : 0)], pa1 = act_e[(size_t)(s0 + rr) * A + (on1 ? a1 : 0)];
    const float pm0 = mup[on0 ? a0 : 0], pm1 = mup[on1 ? a1 : 0];
    const float olp = grow_e[s0 + rr], Ad = grow_e[S_ + s0 + rr];
    const float Rt = grow_e[2 * S_ + s0 + rr], ov = grow_e[3 * S_ + s0 + rr];
    const float v = S[Lc.yr + row * Lc.ld];
    const float ls0 = on0 ? l0 : 0.f, ls1 = on1 ? l1 : 0.f;
    const float iv0 = gauss_inv_var(ls0), iv1 = gauss_inv_var(ls1);
    const float H = gauss_entropy(A, row_sum(ls0 + ls1));
    const LossCoef k = loss_coef(g, inv_b, entp);
    const float mu0 = on0 ? pm0 : 0.f, mu1 = on1 ? pm1 : 0.f;
    const float av0 = on0 ? pa0 : 0.f, av1 = on1 ? pa1 : 0.f;
    const float lp = row_sum((on0 ? gauss_logp_term(av0, mu0, ls0) : 0.f) + (on1 ? gauss_logp_term(av1, mu1, ls1) : 0.f));
    float gl, gv;
    Acc one;
    loss_sample(lp, olp, Ad, Rt, ov, v, H, k, gl, gv, one);
    const float z0 = av0 - mu0, z1 = av1 - mu1;
    // rows past the slice: a zero gradient (their tiles hold the last minibatch's rows)
    if (on0) {
        dla[a0] = live ? gauss_g_mean(gl, z0, iv0) : 0.f;
        mup[a0] = live ? gauss_g_log_std(gl, z0, iv0) : 0.f;
    }
    if (on1) {
        dla[a1] = live ? gauss_g_mean(gl, z1, iv1) : 0.f;
        mup[a1] = live ? gauss_g_log_std(gl, z1, iv1) : 0.f;
    }
    if (sub == 0) {
        S[Lc.dy + row * Lc.ld] = live ? gv : 0.f;
        if (live) {
            lsum += (one.pg + g.vf * 0.5f * one.vl - entp * H) * inv_b;
            klsum += one.kl * inv_b;  // approx_kl (ppo.py:899-902)
        }
    }
}

// The multi-categorical head's loss row pass of the few-row form: the lane
// group's row (4 wave + rq) of the partner's rk <= 16 rows, multi_loss_rows'
// math per element, the categorical few-row pass's outputs (d(logits) /
// d(value) to the output layers' dY tiles, zero past the slice).
__device__ __forceinline__ void few_multi_loss_rows(const GArgs &g, float *S, const unsigned *tgt_e,
                                                    const unsigned *gmask_e, const float *grow_e, long long s0, int rk,
                                                    float inv_b, float entp, float &lsum, float &klsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int row = 4 * wave + rq;
    const int A = g.A, K = g.mk;
    const long long S_ = g.S;
    const GLay &La = g.L[g.aout];
    const GLay &Lc = g.L[g.cout];
    const float *lgp = S + La.yr + row * La.ld;
    float *dla = S + La.dy + row * La.ld;
    const bool live = row < rk;
    const int rr = live ? row : 0;
    const int a0 = sub, a1 = sub + 16;
    const unsigned bits = gmask_e ? gmask_e[s0 + rr] : 0xffffffffu;
    const float plg0 = lgp[a0 < A ? a0 : 0], plg1 = lgp[a1 < A ? a1 : 0];
    const unsigned tgt = tgt_e[s0 + rr];
    const float olp = grow_e[s0 + rr], Ad = grow_e[S_ + s0 + rr];
    const float Rt = grow_e[2 * S_ + s0 + rr], ov = grow_e[3 * S_ + s0 + rr];
    const float v = S[Lc.yr + row * Lc.ld];
    const bool ok0 = (bits >> a0) & 1u, ok1 = (bits >> a1) & 1u;
    const float lg0 = a0 < A ? (ok0 ? plg0 : -1.0e8f) : kSegOut;
    const float lg1 = a1 < A ? (ok1 ? plg1 : -1.0e8f) : kSegOut;
    const bool t0 = (tgt >> a0) & 1u, t1 = (tgt >> a1) & 1u;
    MultiRow mr;
    int off = 0;
    // two components per pass: their reduction chains are independent, so one
    // hides the other's latency; the sums still add in ascending k
    for (int k = 0; k < K; k += 2) {  // wave-uniform: K and the sizes are kernel arguments
        const bool two = k + 1 < K;
        const int n = multi_n(g, k), n2 = two ? multi_n(g, k + 1) : 0;
        const int off2 = off + n;
        MultiRow ra, rb;
        multi_component(0, a0 >= off && a0 < off + n, a1 >= off && a1 < off + n, lg0, lg1, t0, t1, ra);
        multi_component(0, a0 >= off2 && a0 < off2 + n2, a1 >= off2 && a1 < off2 + n2, lg0, lg1, t0, t1, rb);
        multi_merge(k, a0 >= off && a0 < off + n, a1 >= off && a1 < off + n, ra, mr);
        if (two) multi_merge(k + 1, a0 >= off2 && a0 < off2 + n2, a1 >= off2 && a1 < off2 + n2, rb, mr);
        off = off2 + n2;
    }
    const MultiOut o = multi_row_loss(g, mr, t0, t1, olp, Ad, Rt, ov, v, inv_b, entp);
    // rows past the slice: a zero gradient (their tiles hold the last minibatch's rows)
    if (a0 < A) dla[a0] = (live && ok0) ? o.dl0 : 0.f;
    if (a1 < A) dla[a1] = (live && ok1) ? o.dl1 : 0.f;
    if (sub == 0) {
        S[Lc.dy + row * Lc.ld] = live ? o.dvv : 0.f;
        if (live) {
            lsum += o.loss;
            klsum += o.kl;
        }
    }
}

// The Bernoulli head's loss row pass of the few-row form: the lane group's row
// (4 wave + rq) of the partner's rk <= 16 rows, bern_loss_rows' math per
// element, the categorical few-row pass's outputs (d(logits) / d(value) to the
// output layers' dY tiles, zero past the slice).
__device__ __forceinline__ void few_bern_loss_rows(const GArgs &g, float *S, const unsigned *tgt_e,
                                                   const unsigned *gmask_e, const float *grow_e, long long s0, int rk,
                                                   float inv_b, float entp, float &lsum, float &klsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int row = 4 * wave + rq;
    const int A = g.A;
    const long long S_ = g.S;
    const GLay &La = g.L[g.aout];
    const GLay &Lc = g.L[g.cout];
    const float *lgp = S + La.yr + row * La.ld;
    float *dla = S + La.dy + row * La.ld;
    const bool live = row < rk;
    const int rr = live ? row : 0;
    const int a0 = sub, a1 = sub + 16;
    const bool on0 = a0 < A, on1 = a1 < A;
    const unsigned bits = gmask_e ? gmask_e[s0 + rr] : 0xffffffffu;
    const float plg0 = lgp[on0 ? a0 : 0], plg1 = lgp[on1 ? a1 : 0];
    const unsigned tgt = tgt_e[s0 + rr];
    const float olp = grow_e[s0 + rr], Ad = grow_e[S_ + s0 + rr];
    const float Rt = grow_e[2 * S_ + s0 + rr], ov = grow_e[3 * S_ + s0 + rr];
    const float v = S[Lc.yr + row * Lc.ld];
    const bool ok0 = (bits >> a0) & 1u, ok1 = (bits >> a1) & 1u;
    const float lg0 = on0 ? (ok0 ? plg0 : -1.0e8f) : 0.f;
    const float lg1 = on1 ? (ok1 ? plg1 : -1.0e8f) : 0.f;
    const bool t0 = (tgt >> a0) & 1u, t1 = (tgt >> a1) & 1u;
    const BernRowOut o =
        bern_row_loss(g, loss_coef(g, inv_b, entp), on0, on1, lg0, lg1, t0, t1, olp, Ad, Rt, ov, v, inv_b, entp);
    // rows past the slice: a zero gradient (their tiles hold the last minibatch's rows)
    if (on0) dla[a0] = (live && ok0) ? o.dl0 : 0.f;
    if (on1) dla[a1] = (live && ok1) ? o.dl1 : 0.f;
    if (sub == 0) {
        S[Lc.dy + row * Lc.ld] = live ? o.dvv : 0.f;
        if (live) {
            lsum += o.loss;
            klsum += o.kl;
        }
    }
}

// One update's gradient of a partner's rows (rk <= 16 of them, observations
// at xobs, rollout rows s0 ..) into the gradient row G, plus the loss /
// approx_kl partial sums: the few-row counterpart of minibatch_grads, same
// float operations per element.  S: the LDS tiles (plan_few).
// kGauss: gact_e holds the rows' float actions [A] (few_gauss_loss_rows); kMulti:
// the rows' target words (few_multi_loss_rows); kBern: the rows' target words
// (few_bern_loss_rows).
template <Head HEAD>
__device__ __forceinline__ void few_grads(const GArgs &g, float *S, const float *pr, const float *wb, float *G,
                                          const float *xobs, const int *gact_e, const unsigned *gmask_e,
                                          const float *grow_e, long long s0, int rk, float inv_b, float entp,
                                          float &lsum, float &klsum, long long *st) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int row = 4 * wave + rq;  // the lane group's row in the row passes
    const int A = g.A, D = g.D;
    const long long S_ = g.S;
    const auto prs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pr), 0, __builtin_amdgcn_readfirstlane(g.n * 4),
                                                       0x00020000);
    // observation rows (zero past the slice)
    {
        float *x0 = S + g.oc;
        for (int i = tid; i < kFR * D; i += kGT) {
            const int b = i / D, d = i - b * D;
            float v = 0.f;
            if (b < rk) v = xobs[i];
            x0[b * g.ld0 + d] = v;
        }
    }
    __syncthreads();
    if (st) st[0] = (long long)__builtin_readcyclecounter();

    // ---- forward -------------------------------------------------------
    few_forward(g.L, g.nl, S, pr, prs, g.oc, g.ld0, st);

    // ---- PPO loss row pass: logits / value -> d(logits), d(value) (ppo.py:876-908)
    if constexpr (HEAD == kGauss) {
        few_gauss_loss_rows(g, S, pr, reinterpret_cast<const float *>(gact_e), grow_e, s0, rk, inv_b, entp, lsum,
                            klsum);
    } else if constexpr (HEAD == kMulti) {
        few_multi_loss_rows(g, S, reinterpret_cast<const unsigned *>(gact_e), gmask_e, grow_e, s0, rk, inv_b, entp,
                            lsum, klsum);
    } else if constexpr (HEAD == kBern) {
        few_bern_loss_rows(g, S, reinterpret_cast<const unsigned *>(gact_e), gmask_e, grow_e, s0, rk, inv_b, entp,
                           lsum, klsum);
    } else {
        const GLay &La = g.L[g.aout];
        const GLay &Lc = g.L[g.cout];
        const float *lgp = S + La.yr + row * La.ld;
        float *dla = S + La.dy + row * La.ld;
        const bool live = row < rk;
        const int rr = live ? row : 0;
        const int a0 = sub, a1 = sub + 16;
        const unsigned bits = gmask_e ? gmask_e[s0 + rr] : 0xffffffffu;
        const float plg0 = lgp[a0 < A ? a0 : 0], plg1 = lgp[a1 < A ? a1 : 0];
        const int a_t = gact_e[s0 + rr];
        const float olp = grow_e[s0 + rr], Ad = grow_e[S_ + s0 + rr];
        const float Rt = grow_e[2 * S_ + s0 + rr], ov = grow_e[3 * S_ + s0 + rr];
        const float v = S[Lc.yr + row * Lc.ld];
        const bool ok0 = (bits >> a0) & 1u, ok1 = (bits >> a1) & 1u;
        const float lg0 = a0 < A ? (ok0 ? plg0 : -1.0e8f) : -3.0e38f;
        const float lg1 = a1 < A ? (ok1 ? plg1 : -1.0e8f) : -3.0e38f;
        const float mx = row_max(fmaxf(lg0, lg1));
        const float ex0 = a0 < A ? expf(lg0 - mx) : 0.f, ex1 = a1 < A ? expf(lg1 - mx) : 0.f;
        const float lse = mx + logf(row_sum(ex0 + ex1));
        const float p0 = a0 < A ? expf(lg0 - lse) : 0.f, p1 = a1 < A ? expf(lg1 - lse) : 0.f;
        const float lpe0 = logf(p0 + 1e-8f), lpe1 = logf(p1 + 1e-8f);
        const float Hs = -row_sum((a0 < A ? p0 * lpe0 : 0.f) + (a1 < A ? p1 * lpe1 : 0.f));
        const float gh0 = -(lpe0 + p0 / (p0 + 1e-8f)), gh1 = -(lpe1 + p1 / (p1 + 1e-8f));
        const float pg = row_sum((a0 < A ? p0 * gh0 : 0.f) + (a1 < A ? p1 * gh1 : 0.f));
        const int srcl = (lane & ~15) + (a_t & 15);
        const float t0 = bperm(srcl, lg0), t1 = bperm(srcl, lg1);
        const float logp = (a_t < 16 ? t0 : t1) - lse;
        const float lo = 1.f - g.clip, hi = 1.f + g.clip;
        const float lrt = logp - olp;
        const float ratio = expf(lrt);
        const float rcl = fminf(fmaxf(ratio, lo), hi);
        const float q1 = -Ad * ratio, q2 = -Ad * rcl;
        const float g1 = q1 > q2 ? 1.f : (q1 == q2 ? 0.5f : 0.f);
        const float g2 = q2 > q1 ? 1.f : (q1 == q2 ? 0.5f : 0.f);
        const float inr = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
        const float g_logp = ((g1 * -Ad + g2 * -Ad * inr) * inv_b) * ratio;
        const float dv = v - ov;
        const float vcl = ov + fminf(fmaxf(dv, -g.clip), g.clip);
        const float eu = v - Rt, ec = vcl - Rt;
        const float lu = eu * eu, lc = ec * ec;
        const float gu = lu > lc ? 1.f : (lu == lc ? 0.5f : 0.f);
        const float gc = lc > lu ? 1.f : (lu == lc ? 0.5f : 0.f);
        const float inv = (dv >= -g.clip && dv <= g.clip) ? 1.f : 0.f;
        const float g_H = -entp * inv_b;
        const float dl0 = g_logp * ((a0 == a_t ? 1.f : 0.f) - p0) + g_H * p0 * (gh0 - pg);
        const float dl1 = g_logp * ((a1 == a_t ? 1.f : 0.f) - p1) + g_H * p1 * (gh1 - pg);
        // rows past the slice: a zero gradient (their tiles hold the last minibatch's rows)
        if (a0 < A) dla[a0] = (live && ok0) ? dl0 : 0.f;
        if (a1 < A) dla[a1] = (live && ok1) ? dl1 : 0.f;
        if (sub == 0) {
            const float dvv = g.vf * 0.5f * inv_b * (gu * 2.f * eu + gc * 2.f * ec * inv);
            S[Lc.dy + row * Lc.ld] = live ? dvv : 0.f;
            if (live) {
                lsum += (fmaxf(q1, q2) + g.vf * 0.5f * fmaxf(lu, lc) - entp * Hs) * inv_b;
                klsum += ((ratio - 1.f) - lrt) * inv_b;  // approx_kl (ppo.py:899-902)
            }
        }
    }
    __syncthreads();
    if constexpr (HEAD == kGauss) {
        // d(log_std): the 16 rows' terms (left in the mean tile) in row order, and
        // the entropy's -ent_coef / b per row of the slice
        if (wave == kGW - 1 && lane < A) {
            const GLay &La = g.L[g.aout];
            float v[kFR];
#pragma unroll
            for (int b = 0; b < kFR; ++b) v[b] = S[La.yr + b * La.ld + lane];
            float sum = 0.f;
#pragma unroll
            for (int b = 0; b < kFR; ++b) sum += v[b];
            G[g.lso + lane] = sum + (-entp * inv_b) * (float)rk;
        }
    }
    if (st) st[17] = (long long)__builtin_readcyclecounter();

    // ---- backward, layer by layer (reverse) ------------------------------
    float *T = S + g.t1;  // dY' of the current LN-affine layer (its gamma / beta gradients)
    for (int l = g.nl - 1; l >= 0; --l) {
        const GLay &L = g.L[l];
        const int F = L.fout, ld = L.ld;
        float *dZ = S + L.dy;  // dY in, dZ out (in place)
        if (L.ln || L.relu) {
            float *dy = dZ + row * ld;
            const float *xh = S + (L.ln ? L.xh : L.yr) + row * ld;  // xhat, or Y for a plain ReLU
            const LayRow lr{L.ln, L.relu, L.af, L.rs, L.xh};
            if (F <= 64) {
                few_row_back<4>(dy, xh, T + row * ld, S, lr, F, row, sub);
            } else if (F <= 16 * kRowRegs) {
                few_row_back<kRowRegs>(dy, xh, T + row * ld, S, lr, F, row, sub);
            } else {
                const float invF = 1.f / (float)F;
                float m1 = 0.f, m2 = 0.f, rs = 1.f;
                auto dpre = [&](int j, float &x) {
                    const float d = dy[j];
                    x = xh[j];
                    const float pre = L.ln == 2 ? x * S[L.af + j] + S[L.af + F + j] : x;
                    return (!L.relu || pre > 0.f) ? d : 0.f;
                };
                if (L.ln) {
                    float s1 = 0.f, s2 = 0.f;
                    for (int j = sub; j < F; j += 16) {
                        float x;
                        const float dx = dpre(j, x) * (L.ln == 2 ? S[L.af + j] : 1.f);
                        s1 += dx;
                        s2 += dx * x;
                    }
                    m1 = row_sum(s1) * invF;
                    m2 = row_sum(s2) * invF;
                    rs = S[L.rs + row];
                }
                for (int j = sub; j < F; j += 16) {
                    float x;
                    const float dp = dpre(j, x);
                    if (L.ln == 2) T[row * ld + j] = dp;
                    dy[j] = L.ln ? rs * (dp * (L.ln == 2 ? S[L.af + j] : 1.f) - m1 - x * m2) : dp;
                }
            }
            __syncthreads();
        }
        if (st) st[18 + 3 * l] = (long long)__builtin_readcyclecounter();
        // bias / LN-affine gradients: column sums in row order, one sum per
        // wave (0: bias, 1: gamma, 2: beta), the 16 rows' terms loaded first
        if (wave < (L.ln == 2 ? 3 : 1)) {
            const float *src = wave == 0 ? dZ : T;
            const long long go = wave == 0 ? L.b : wave == 1 ? L.g : L.be;
            for (int j = lane; j < F; j += kWave) {
                float v[kFR];
#pragma unroll
                for (int b = 0; b < kFR; ++b) {
                    v[b] = src[b * ld + j];
                    if (wave == 1) v[b] = v[b] * S[L.xh + b * ld + j];
                }
                float sum = 0.f;
#pragma unroll
                for (int b = 0; b < kFR; ++b) sum += v[b];
                G[go + j] = sum;
            }
        }
        const float *X = L.src < 0 ? S + g.oc : S + g.L[L.src].yr;
        const int ldx = L.src < 0 ? g.ld0 : g.L[L.src].ld;
        few_dw(dZ, ld, X, ldx, F, L.fin, G + L.w);
        if (st) st[19 + 3 * l] = (long long)__builtin_readcyclecounter();
        if (L.src >= 0) {  // dX = dZ W into the source's dY (the second consumer adds)
            const GLay &Ls = g.L[L.src];
            float *dys = S + Ls.dy;
            const int lds_ = Ls.ld;
            if (L.acc)
                few_gemm<true>(dZ, ld, prs, L.w * 4, F, L.fin, nullptr,
                               [&](int m, int n, float v) { dys[m * lds_ + n] += v; });
            else
                few_gemm<true>(dZ, ld, prs, L.w * 4, F, L.fin, nullptr,
                               [&](int m, int n, float v) { dys[m * lds_ + n] = v; });
        }
        __syncthreads();
        if (st) st[20 + 3 * l] = (long long)__builtin_readcyclecounter();
    }
}

// FEW: the few-row form (few_grads, activations in dynamic LDS); else the
// general form (minibatch_grads over the partner's global scratch)
template <bool FEW, Head HEAD>
__global__ __launch_bounds__(kGT) void ppo_learn_graph_part_kernel(const GArgs g) {
    __shared__ float red[2 * kGW];
    __shared__ __attribute__((aligned(16))) float lds[kGemmLds];
    __shared__ float colp[2 * 3 * kGW * 128];
    __shared__ float colo[kGW * kColo<HEAD>];
    __shared__ int s_ok;
    __shared__ long long s_st[16 + kGStampsIn];  // phase stamps (agent 0, partner 0, update 1), then per layer
    if (g.skip && __hip_atomic_load(g.skip, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u) return;
    const int b = blockIdx.x;
    const int p = b % g.Q, kk = b / g.Q;
    if (p >= g.P) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = g.K, P = g.P, n = g.n, D = g.D;
    const long long S = g.S;
    float *const pr = g.params + (size_t)p * n;
    float *const gm = g.m + (size_t)p * n;
    float *const gv = g.v + (size_t)p * n;
    // the activation scratch: the few-row form's LDS tiles (zeroed once: their
    // padding columns stay zero), else this partner's block of the global scratch
    extern __shared__ __attribute__((aligned(16))) float gdyn[];
    float *const base = FEW ? gdyn : g.ws + ((size_t)p * K + kk) * g.ws_part;
    if constexpr (FEW) {
        for (int i = tid; i < (int)g.lds_floats; i += kGT) gdyn[i] = 0.f;
    }
    float *const wsh = g.wtb + (size_t)p * g.wt_agent;  // the agent's shared transposed weights
    float *const wb = wsh - g.wt0;                      // wb + L.wt lands in wsh
    unsigned *const c0 = g.cnt + p, *const c1 = g.cnt + P + p, *const c2 = g.cnt + 2 * P + p;
    unsigned *const c3 = g.cnt + 3 * P + p, *const tmo = g.cnt + 4 * P;
    unsigned *const xcc = g.cnt + 4 * P + 1 + (size_t)p * kMaxGK;
    // float4 ownership: chunks [own0, own1) of the n4s = n4 + 1 chunks (the
    // gradient row padded to n4 chunks, then the loss / approx_kl chunk)
    const int n4 = (n + 3) / 4, n4s = n4 + 1, nal = 4 * n4;
    const int cs = (n4s + K - 1) / K;
    const int own0 = kk * cs < n4s ? kk * cs : n4s, own1 = own0 + cs < n4s ? own0 + cs : n4s;
    const int f0 = 4 * own0, f1 = 4 * own1 < n ? 4 * own1 : n;  // owned parameter floats

    // placement id + the transposed copies of the owned weights, one setup barrier
    if (tid == 0) {
        int x;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(x));
        __hip_atomic_store(xcc + kk, (unsigned)(x & 15) + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    for (int l = 0; l < (FEW ? 0 : g.nl); ++l) {
        const GLay &L = g.L[l];
        if (L.wt < 0) continue;
        const int cnt = L.fout * L.fin;
        const int i0 = f0 - L.w > 0 ? f0 - L.w : 0, i1 = f1 - L.w < cnt ? f1 - L.w : cnt;
        float *wt = wb + L.wt;
        for (int i = i0 + tid; i < i1; i += kGT) {
            const int o = i / L.fin, c = i - o * L.fin;
            wt[(size_t)c * L.fout + o] = pr[L.w + i];
        }
    }
    if (!gpart_sync(c0, (unsigned)K, true, tmo, g.err, &s_ok)) return;
    bool local;
    {
        const unsigned v = lane < K ? __hip_atomic_load(xcc + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
        const unsigned v0 = __builtin_amdgcn_readlane(v, 0);
        bool same = v0 != 0u;
        for (int q = 1; q < K; ++q) same = same && __builtin_amdgcn_readlane(v, q) == v0;
        local = same && !g.write_through;
    }
    gpart_acquire();

    int Bp = g.batch_p ? g.batch_p[p] : g.B;
    if (Bp > g.B) Bp = g.B;
    const int Ep = g.epochs_p ? g.epochs_p[p] : g.E;
    const float entp = g.ent_p ? g.ent_p[p] : g.ent;
    const int nmb = (int)((S + Bp - 1) / Bp);
    float loss_total = 0.f;
    double kl_total = 0.0;
    int n_done = 0, epochs_done = 0;
    const long long step0 = g.step[p];
    double pb1 = pow((double)g.b1, (double)step0), pb2 = pow((double)g.b2, (double)step0);
    const float lr_p = g.lr[p];

    for (int e = 0; e < Ep; ++e) {
        const size_t ge = (size_t)e * P + p;
        const float *gobs_e = g.gobs + ge * S * D;
        const int *gact_e = g.gact + ge * S * (HEAD == kGauss ? g.A : 1);
        const unsigned *gmask_e = g.gmask ? g.gmask + ge * S : nullptr;
        const float *grow_e = g.grow + ge * 4 * S;
        for (int mb = 0; mb < nmb; ++mb) {
            const long long s0 = (long long)mb * Bp;
            const int bsz = (int)((s0 + Bp <= S) ? Bp : S - s0);
            const float inv_b = 1.f / (float)bsz;
            const int r0 = kk * g.R, rk = bsz - r0 < 0 ? 0 : (bsz - r0 < g.R ? bsz - r0 : g.R);
            const int upd = e * nmb + mb;
            float *const slab0 = g.slabs + ((size_t)p * 2 + (upd & 1)) * K * g.nslab;  // partner 0's slab
            float *const G = slab0 + (size_t)kk * g.nslab;
            float *const sum = g.sums + ((size_t)p * 2 + (upd & 1)) * g.nslab;

            const bool stamp = g.stamps && b == 0 && upd == 1 && tid == 0;
#define GST(i) \
    if (stamp) s_st[i] = (long long)__builtin_readcyclecounter()
            GST(0);
            // ---- 1. this partner's rows -> its partial gradient row ----------------
            float lsum = 0.f, klsum = 0.f;
            if (rk > 0) {
                if constexpr (FEW)
                    few_grads<HEAD>(g, base, pr, wb, G, gobs_e + (s0 + r0) * D, gact_e, gmask_e, grow_e, s0 + r0, rk,
                                     inv_b, entp, lsum, klsum, stamp ? s_st + 16 : nullptr);
                else
                    minibatch_grads<HEAD>(g, base, wb, pr, G, gobs_e + (s0 + r0) * D, gact_e, gmask_e, grow_e,
                                           s0 + r0, rk, inv_b, entp, lds, colp, colo, lsum, klsum,
                                           stamp ? s_st + 16 : nullptr);
            } else {  // no rows this minibatch (a short last minibatch): publish zeros
                for (int i = tid; i < n; i += kGT) G[i] = 0.f;
            }
            GST(1);
            block_sum2(lsum, klsum, red);
            if (tid == 0) {
                G[nal] = lsum;
                G[nal + 1] = klsum;
            }
            GST(2);
            if (!gpart_sync(c1, (unsigned)(K * (upd + 1)), !local, tmo, g.err, &s_ok)) return;
            GST(3);

            // ---- 2. reduce-scatter of the owned chunks + partial norms ---------------
            // few-row form with at most four owned chunks per thread: the sums stay
            // in registers for Adam and the chunks' moments / parameters are loaded
            // before barrier 2 (they land while it waits)
            const bool regs = FEW && own1 - own0 <= 4 * kGT;
            f4 tg[2][2];
            float mg[2][2][4], vg[2][2][4], pg[2][2][4];
            float q0 = 0.f, q1 = 0.f;
            {
                const auto rs = __builtin_amdgcn_make_buffer_rsrc(slab0, 0, __builtin_amdgcn_readfirstlane(
                                                                                 (int)(K * g.nslab * 4)), 0x00020000);
                // two chunks per thread per round, partner order, up to 16 loads in flight
                int rr = 0;
                for (int cb = own0 + tid; cb < own1; cb += 2 * kGT, ++rr) {
                    f4 t[2] = {f4{0.f, 0.f, 0.f, 0.f}, f4{0.f, 0.f, 0.f, 0.f}};
                    for (int q0_ = 0; q0_ < K; q0_ += 8) {  // uniform
                        f4 x[2][8];
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int c = cb + h * kGT, cl = c < own1 ? c : own0;
#pragma unroll
                            for (int q = 0; q < 8; ++q) {
                                const int qq = q0_ + q, qs = qq < K ? qq : K - 1;
                                const f4 v = __builtin_bit_cast(
                                    f4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)((qs * g.nslab + 4 * cl) * 4), 0, 16));
                                x[h][q] = qq < K ? v : f4{0.f, 0.f, 0.f, 0.f};
                            }
                        }
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            if (q0_ == 0) {
                                t[h] = x[h][0];
#pragma unroll
                                for (int q = 1; q < 8; ++q) t[h] += x[h][q];
                            } else {
#pragma unroll
                                for (int q = 0; q < 8; ++q) t[h] += x[h][q];
                            }
                        }
                    }
                    if (regs) {
                        if (rr == 0) {
                            tg[0][0] = t[0];
                            tg[0][1] = t[1];
                        } else {
                            tg[1][0] = t[0];
                            tg[1][1] = t[1];
                        }
                    }
#pragma unroll
                    for (int h = 0; h < 2; ++h) {
                        const int c = cb + h * kGT;
                        if (c >= own1) break;
                        // (the loss / approx_kl chunk n4 always: every partner reads it after barrier 2)
                        if (!regs || c >= n4) *reinterpret_cast<f4 *>(sum + 4 * c) = t[h];
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            const int f = 4 * c + cc;
                            const float x2 = f < n ? t[h][cc] * t[h][cc] : 0.f;
                            if (f < g.cstart) q0 += x2;
                            else q1 += x2;
                        }
                    }
                }
                q0 = wave_sum(q0);
                q1 = wave_sum(q1);
                if (lane < 2) sum[nal + 4 + (kk * kGW + wave) * 2 + lane] = lane ? q1 : q0;
            }
            if (regs) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            const int f = 4 * (own0 + tid + (2 * r + h) * kGT) + cc;
                            const int fs = f < f1 ? f : f0;
                            mg[r][h][cc] = gm[fs];
                            vg[r][h][cc] = gv[fs];
                            pg[r][h][cc] = pr[fs];
                        }
            }
            GST(4);
            if (!gpart_sync(c2, (unsigned)(K * (upd + 1)), !local, tmo, g.err, &s_ok)) return;
            GST(5);

            // ---- 3. norms (fixed order), loss words, Adam on the owned floats ---------
            float t0, t1, lmb, klmb;
            {
                const int np = 2 * kGW * K;  // <= 128 words: lanes l and l + 64
                float v = 0.f;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const int w = lane + 64 * h;
                    const float x = ld_sc1(sum + nal + 4 + (w < np ? w : 0));
                    v += w < np ? x : 0.f;
                }
                const float lw = ld_sc1(sum + nal), kw = ld_sc1(sum + nal + 1);
                t0 = wave_sum((lane & 1) ? 0.f : v);
                t1 = wave_sum((lane & 1) ? v : 0.f);
                lmb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, lw)));
                klmb = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(unsigned, kw)));
            }
            GST(6);
            if (tid == 0) loss_total += lmb;
            kl_total += (double)klmb;
            ++n_done;
            const float cl0 = g.max_norm > 0.f ? fminf(g.max_norm / (sqrtf(t0) + 1e-6f), 1.f) : 1.f;
            const float cl1 = g.max_norm > 0.f ? fminf(g.max_norm / (sqrtf(t1) + 1e-6f), 1.f) : 1.f;
            pb1 *= (double)g.b1;
            pb2 *= (double)g.b2;
            const float bc1 = (float)(1.0 - pb1);
            const float bc2s = (float)sqrt(1.0 - pb2);
            const float step_size = lr_p / bc1;
            const float ob1 = 1.f - g.b1, ob2 = 1.f - g.b2;
            // the owned float range [f0, f1) in one pass, U elements per thread per
            // round (all loads of a round first); an element inside a layer's W
            // also goes to the transposed copy (the layer found by a short scan of
            // the layer list: contiguous W ranges, at most 16 layers)
            if (regs) {
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int h = 0; h < 2; ++h)
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
                            const int f = 4 * (own0 + tid + (2 * r + h) * kGT) + cc;
                            if (f >= f1) continue;
                            const float gc = tg[r][h][cc] * (f < g.cstart ? cl0 : cl1);
                            const float m = mg[r][h][cc] + ob1 * (gc - mg[r][h][cc]);
                            const float v = vg[r][h][cc] * g.b2 + ob2 * gc * gc;
                            gm[f] = m;
                            gv[f] = v;
                            pr[f] = pg[r][h][cc] - step_size * (m / (sqrtf(v) / bc2s + g.eps));
                        }
            } else {
                constexpr int U = 8;
                for (int i0 = f0 + tid; i0 < f1; i0 += U * kGT) {
                    float gg[U], mm[U], vv[U], pp[U];
#pragma unroll
                    for (int k = 0; k < U; ++k) {
                        const int i = i0 + k * kGT;
                        const int f = i < f1 ? i : f0;
                        gg[k] = sum[f];  // this partner's own reduce-scatter stores
                        mm[k] = gm[f];
                        vv[k] = gv[f];
                        pp[k] = pr[f];
                    }
#pragma unroll
                    for (int k = 0; k < U; ++k) {
                        const int f = i0 + k * kGT;
                        if (f >= f1) break;
                        const float gc = gg[k] * (f < g.cstart ? cl0 : cl1);
                        const float m = mm[k] + ob1 * (gc - mm[k]);
                        const float v = vv[k] * g.b2 + ob2 * gc * gc;
                        const float np_ = pp[k] - step_size * (m / (sqrtf(v) / bc2s + g.eps));
                        gm[f] = m;
                        gv[f] = v;
                        pr[f] = np_;
                        if constexpr (!FEW) {  // the few-row form's dX reads W itself
                            for (int l = 0; l < g.nl; ++l) {
                                const GLay &L = g.L[l];
                                const int i = f - L.w;
                                if (L.wt >= 0 && i >= 0 && i < L.fout * L.fin) {
                                    const int o = i / L.fin, c = i - o * L.fin;
                                    wb[L.wt + (size_t)c * L.fout + o] = np_;
                                    break;
                                }
                            }
                        }
                    }
                }
            }
            GST(7);
            // ---- 4. every partner's chunks visible to this one's next plain loads ---------
            if (!gpart_sync(c3, (unsigned)(K * (upd + 1)), !local, tmo, g.err, &s_ok)) return;
            GST(8);
            gpart_acquire();
            GST(9);
#undef GST
        }  // minibatches
        ++epochs_done;
        if (g.target_kl > 0.0 && kl_total / (double)n_done > g.target_kl) break;  // ppo.py:917-918
    }  // epochs
    if (tid == 0 && kk == 0) {
        if (g.loss_out) g.loss_out[p] = loss_total / ((float)S * (float)Ep);
        if (g.kl_out) g.kl_out[p] = n_done ? (float)(kl_total / (double)n_done) : 0.f;
        if (g.epochs_out) g.epochs_out[p] = epochs_done;
        g.step[p] = step0 + n_done;
    }
    if (g.stamps && b == 0 && tid < 16 + kGStampsIn) g.stamps[tid] = s_st[tid];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// What a head's entry points pass besides the net (validated by their checks)
struct HeadArg {
    long long lso = -1;      // kGauss: log_std's offset in the parameter row
    agx_multi_head multi{};  // kMulti: the components, those past K zeroed
};
// What the host path knows of a head: the parameters no layer owns (plan_graph's
// `extra`), the gather's action packer (ppo_gather.h; its words() sizes gact),
// and what the head writes into GArgs.
struct PlainHead {  // the categorical network as it is
    static int extra(const agx_ppo_graph *) { return 0; }
    static void fill(GArgs &a, const HeadArg &) { a.lso = -1; }
};
template <Head HEAD>
struct HeadTraits;
template <>
struct HeadTraits<kCat> : PlainHead {
    using Pack = CatPack;
    static Pack pack(const HeadArg &) { return {}; }
};
template <>
struct HeadTraits<kBern> : PlainHead {
    using Pack = BernPack;
    static Pack pack(const HeadArg &) { return {}; }
};
template <>
struct HeadTraits<kGauss> {
    static int extra(const agx_ppo_graph *net) { return net->n_actions; }  // log_std
    static void fill(GArgs &a, const HeadArg &h) { a.lso = h.lso; }
    using Pack = GaussPack;
    static Pack pack(const HeadArg &) { return {}; }
};
template <>
struct HeadTraits<kMulti> : PlainHead {
    static void fill(GArgs &a, const HeadArg &h) {
        PlainHead::fill(a, h);
        a.mk = h.multi.K;
        for (int k = 0; k < h.multi.K; ++k) a.mn[k >> 2] |= (unsigned)h.multi.nvec[k] << (8 * (k & 3));
    }
    using Pack = MultiPack;
    static Pack pack(const HeadArg &h) { return {h.multi}; }
};

inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }
// The gather's output in either workspace, from byte `at` (a multiple of 256).
// aw: 4-byte words of a row's gathered action (Pack::words)
struct GatherWs {
    size_t gobs, gact, gmask, grow, end;
};
GatherWs gather_ws(size_t at, const GArgs &a, int64_t P, int64_t S, int64_t epochs, int aw) {
    GatherWs w;
    const size_t per = (size_t)epochs * P * S;
    w.gobs = at;
    w.gact = w.gobs + up256(per * a.D * 4);
    w.gmask = w.gact + up256(per * 4 * aw);
    w.grow = w.gmask + up256(per * 4);
    w.end = w.grow + up256(per * 4 * 4);
    return w;
}
struct GraphWs {
    GatherWs g;
    size_t agents, total;
};
GraphWs graph_ws(const GArgs &a, int64_t P, int64_t S, int64_t epochs, int aw) {
    GraphWs w;
    w.g = gather_ws(0, a, P, S, epochs, aw);
    w.agents = w.g.end;
    w.total = w.agents + (size_t)P * a.ws_agent * 4;
    return w;
}

template <bool FEW, Head HEAD>
int part_occupancy(size_t dyn) {  // co-resident partner workgroups per CU with dyn bytes of dynamic LDS
    static size_t last = (size_t)-1;
    static int n = 1;
    if (dyn != last) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, ppo_learn_graph_part_kernel<FEW, HEAD>, kGT, dyn) != hipSuccess)
            v = 1;
        n = v < 1 ? 1 : v;
        last = dyn;
    }
    return n;
}
// dynamic LDS the few-row form may take: the CU's 160 KB less the kernel's
// static LDS (queried once per head)
template <Head HEAD>
size_t few_lds_budget() {
    static size_t b = 0;
    if (!b) {
        hipFuncAttributes fa{};
        const size_t st = hipFuncGetAttributes(&fa, (const void *)ppo_learn_graph_part_kernel<true, HEAD>) == hipSuccess
                              ? fa.sharedSizeBytes
                              : 8 * 1024;
        b = st < kLdsMax ? kLdsMax - st : 1;
        (void)hipFuncSetAttribute((const void *)ppo_learn_graph_part_kernel<true, HEAD>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)b);
    }
    return b;
}
// the few-row form's plan: the general plan (validation, parameter offsets,
// transposed weights, accumulation order) with every activation tile moved to
// LDS: per layer Y, xhat + rstd (LayerNorm), dY, each [16][ld]; the
// observation tile; one dY' tile for the LN-affine gradients.  -> LDS bytes
// (0: the plan does not fit, or the graph is invalid)
template <Head HEAD>
size_t plan_few(const agx_ppo_graph *net, GArgs &a) {
    if (plan_graph(net, kFR, a, HeadTraits<HEAD>::extra(net)) != AGX_OK) return 0;
    auto ldof = [](int w) { return (w + 15) / 16 * 16 + 4; };
    long long off = 0;
    int ldmax = 0;
    bool affine = false;
    for (int l = 0; l < a.nl; ++l) {
        GLay &L = a.L[l];
        L.ld = ldof(L.fout);
        L.yr = off;
        off += (long long)kFR * L.ld;
        L.xh = L.rs = -1;
        if (L.ln) {
            L.xh = off;
            off += (long long)kFR * L.ld;
            L.rs = off;
            off += kFR;
        }
        L.dy = off;
        off += (long long)kFR * L.ld;
        L.af = -1;
        if (L.ln == 2) {
            L.af = off;
            off += 2 * ((L.fout + 3) / 4 * 4);
        }
        L.yc = L.dy2 = L.dyc = -1;
        L.fuse = L.fused = 0;
        ldmax = L.ld > ldmax ? L.ld : ldmax;
        affine = affine || L.ln == 2;
    }
    a.ld0 = ldof(a.D);
    a.oc = off;
    off += (long long)kFR * a.ld0;
    a.t1 = off;
    if (affine) off += (long long)kFR * ldmax;
    a.lds_floats = (off + 3) & ~3ll;
    a.ws_part = 0;  // no global activation scratch
    const size_t bytes = (size_t)a.lds_floats * 4;
    return bytes <= few_lds_budget<HEAD>() ? bytes : 0;
}
// How a learn() runs, chosen per call (the workspace query makes the same
// choice): the few-row partnered form when a minibatch splits into at most
// kMaxGK slices of at most 16 rows whose tiles fit in LDS (AGX_GRAPH_FEW=0
// turns it off); else the general partnered form, K partners of R rows
// (AGX_GRAPH_ROWS, default 16); K = 1: one workgroup per agent.  The whole
// grid (Q x K workgroups, Q = P rounded up to the 8 XCDs) must be co-resident.
// AGX_GRAPH_SPLIT caps K (tests, diagnostics).
struct Split {
    int K = 1, R = 1, Q = 1;
    bool few = false;
    size_t dyn = 0;  // dynamic LDS bytes (few-row form)
};
template <Head HEAD>
Split graph_split(const agx_ppo_graph *net, int64_t P, int64_t batch) {
    Split sp;
    int rows = 16;
    if (const char *e = getenv("AGX_GRAPH_ROWS")) rows = atoi(e) >= 1 ? atoi(e) : 16;
    int cap = kMaxGK;
    if (const char *e = getenv("AGX_GRAPH_SPLIT")) cap = atoi(e) >= 1 ? atoi(e) : 1;
    bool few_ok = true;
    if (const char *e = getenv("AGX_GRAPH_FEW")) few_ok = atoi(e) != 0;
    sp.Q = (int)((P + 7) / 8 * 8);
    const int64_t cus = cu_count();
    int k = (int)((batch + rows - 1) / rows);
    if (k > cap) k = cap;
    if (few_ok && k > 1 && (batch + k - 1) / k <= kFR) {
        GArgs a{};
        const size_t dyn = plan_few<HEAD>(net, a);
        if (dyn && (int64_t)sp.Q * k <= (int64_t)part_occupancy<true, HEAD>(dyn) * cus) {
            sp.few = true;
            sp.dyn = dyn;
            sp.K = k;
            sp.R = (int)((batch + k - 1) / k);
            return sp;
        }
    }
    while (k > 1 && (int64_t)sp.Q * k > (int64_t)part_occupancy<false, HEAD>(0) * cus) --k;
    if (k > 1 && (int64_t)P * k > (int64_t)part_occupancy<false, HEAD>(0) * cus) k = 1;
    sp.K = k < 1 ? 1 : k;
    sp.R = (int)((batch + sp.K - 1) / sp.K);
    return sp;
}
struct PartWs {
    size_t cnt;  // the counters the gather zeroes: [cnt, g.gobs)
    GatherWs g;
    size_t scratch, wt, slabs, sums, total;
    long long nslab;
};
PartWs part_ws(const GArgs &a, int64_t P, int64_t S, int64_t epochs, int K, int aw) {
    PartWs w;
    w.cnt = 0;
    w.g = gather_ws(up256(((size_t)4 * P + 1 + (size_t)kMaxGK * P) * 4), a, P, S, epochs, aw);
    w.scratch = w.g.end;
    w.wt = w.scratch + up256((size_t)P * K * a.ws_part * 4);
    w.nslab = ((long long)(a.n + 3) / 4 * 4 + 4 + 2 * kGW * K + 63) / 64 * 64;
    w.slabs = w.wt + up256((size_t)P * a.wt_agent * 4);
    w.sums = w.slabs + up256((size_t)P * 2 * K * w.nslab * 4);
    w.total = w.sums + (size_t)P * 2 * w.nslab * 4;
    return w;
}

// A head the multi-categorical learner takes: a layer list agx_ppo_graph_check
// admits and a head that fits it (multi_head_check.h).
// -> h.multi: the head with the components past K zeroed (the kernels never read them)
int multi_check(const char *who, const agx_ppo_graph *net, const agx_multi_head &head, HeadArg &h) {
    GArgs a{};
    AGX_REQUIRE(net, "%s: null graph", who);
    if (int rc = plan_graph(net, 1, a)) return rc;
    const int L = head_width(head, who);
    if (L < 0) return AGX_EINVAL;
    if (int rc = head_fits(net, L, who)) return rc;
    h.multi = head_arg(head);
    return AGX_OK;
}

// The layers and the A log_std floats at lso tile the parameter row exactly,
// and log_std lies in the actor clip group [0, critic_start).
int gauss_check(const agx_ppo_graph *net, int64_t lso) {
    GArgs a{};
    AGX_REQUIRE(net, "agx_ppo_gauss_graph_check: null graph");
    const int rc = plan_graph(net, 1, a, net->n_actions);
    if (rc != AGX_OK) return rc;
    const int A = net->n_actions;
    AGX_REQUIRE(lso >= 0 && lso + A <= net->critic_start,
                "agx_ppo_gauss_graph_check: log_std [%lld, %lld) outside the actor group [0, %d)", (long long)lso,
                (long long)lso + A, net->critic_start);
    // every parameter range by offset: each must start where the previous one ends
    long long beg[4 * kGL + 1], len[4 * kGL + 1];
    int nr = 0;
    auto add = [&](long long b, long long n) {
        int i = nr++;
        for (; i > 0 && beg[i - 1] > b; --i) {
            beg[i] = beg[i - 1];
            len[i] = len[i - 1];
        }
        beg[i] = b;
        len[i] = n;
    };
    for (int l = 0; l < net->n_layers; ++l) {
        const agx_ppo_layer &x = net->layers[l];
        add(x.w, (long long)x.fin * x.fout);
        add(x.b, x.fout);
        if (x.ln == 2) {
            add(x.ln_w, x.fout);
            add(x.ln_b, x.fout);
        }
    }
    add(lso, A);
    long long at = 0;
    for (int i = 0; i < nr; ++i) {
        AGX_REQUIRE(beg[i] == at, "agx_ppo_gauss_graph_check: log_std_off %lld is not the gap the layers leave",
                    (long long)lso);
        at += len[i];
    }
    AGX_REQUIRE(at == net->n_params, "agx_ppo_gauss_graph_check: log_std_off %lld is not the gap the layers leave",
                (long long)lso);
    return AGX_OK;
}

template <Head HEAD>
size_t learn_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t S, int64_t epochs, int64_t batch) {
    GArgs a{};
    if (P <= 0 || S <= 0 || epochs <= 0 || batch <= 0) return 0;
    const int64_t bb = batch < S ? batch : S;
    using T = HeadTraits<HEAD>;
    const int extra = T::extra(net);
    if (plan_graph(net, bb, a, extra) != AGX_OK) return 0;
    const int aw = T::Pack::words(a.A);
    size_t total = graph_ws(a, P, S, epochs, aw).total;
    const Split sp = graph_split<HEAD>(net, P, bb);
    if (sp.K > 1) {  // room for either kernel: the split may change with the call's batch
        GArgs ap{};
        if (sp.few ? !plan_few<HEAD>(net, ap) : plan_graph(net, sp.R, ap, extra) != AGX_OK) return 0;
        const size_t t = part_ws(ap, P, S, epochs, sp.K, aw).total;
        total = t > total ? t : total;
    }
    return total;
}

long long *&g_graph_stamps() {
    static long long *p = nullptr;
    return p;
}

// The learn call of a head's entry point `what` (named in errors); h: validated by the caller
template <Head HEAD>
int learn_graph(const char *what, const agx_ppo_graph *net, const HeadArg &h, const agx_ppo_learn_args *x,
                void *workspace, void *stream) {
    using T = HeadTraits<HEAD>;
    using Pack = typename T::Pack;
    AGX_REQUIRE(x->params && x->exp_avg && x->exp_avg_sq && x->adam_step && x->lr && x->obs && x->actions &&
                    x->old_logp && x->adv && x->ret && x->old_value && x->perms,
                "%s: null pointer", what);
    const int64_t P = x->P, S = x->S, epochs = x->epochs, batch = x->batch;
    AGX_REQUIRE(P > 0 && P <= 65535 && S > 0 && S < (1ll << 31) && epochs > 0 && batch > 0 && epochs * P <= 65535,
                "%s: bad sizes P=%lld S=%lld epochs=%lld batch=%lld", what, (long long)P, (long long)S,
                (long long)epochs, (long long)batch);
    if (int rc = adv_norm_minibatch_check(what, x)) return rc;
    const int64_t bb = batch < S ? batch : S;
    const Split sp = graph_split<HEAD>(net, P, bb);
    const int K = sp.K, R = sp.R, Q = sp.Q;
    GArgs a{};
    const int rc = plan_graph(net, K > 1 ? R : bb, a, T::extra(net));
    if (rc != AGX_OK) return rc;
    if (sp.few) AGX_REQUIRE(plan_few<HEAD>(net, a) == sp.dyn, "%s: few-row plan changed", what);
    T::fill(a, h);
    const int aw = Pack::words(a.A);
    char *ws = static_cast<char *>(workspace);
    hipStream_t s = as_stream(stream);
    unsigned *counters = nullptr;
    int ncounters = 0;
    PartWs pw{};
    GraphWs w{};
    if (K > 1) {
        pw = part_ws(a, P, S, epochs, K, aw);
        counters = reinterpret_cast<unsigned *>(ws + pw.cnt);
        ncounters = (int)(pw.g.gobs / sizeof(unsigned));
    } else {
        w = graph_ws(a, P, S, epochs, aw);
    }
    const GatherWs &gw = K > 1 ? pw.g : w.g;
    float *gobs = reinterpret_cast<float *>(ws + gw.gobs);
    int *gact = reinterpret_cast<int *>(ws + gw.gact);
    unsigned *gmask = x->action_masks ? reinterpret_cast<unsigned *>(ws + gw.gmask) : nullptr;
    float *grow = reinterpret_cast<float *>(ws + gw.grow);
    dim3 ggrid((unsigned)ceil_div(S, 256), (unsigned)(epochs * P));
    ppo_gather_kernel<Pack><<<ggrid, 256, 0, s>>>(
        x->obs, reinterpret_cast<const typename Pack::Elem *>(x->actions), x->old_logp, x->adv, x->ret, x->old_value,
        x->adv_stats, reinterpret_cast<const long long *>(x->perms), x->action_masks, a.A, T::pack(h), S, a.D, (int)P,
        gobs, reinterpret_cast<typename Pack::Word *>(gact), gmask, grow, counters, ncounters, x->epochs_per_agent,
        x->error_word);
    const int rc2 = check_launch(what);
    if (rc2) return rc2;
    if (x->adv_norm_minibatch) {  // IPPO: the gathered advantages, minibatch by minibatch
        ppo_adv_norm_minibatch_kernel<<<dim3((unsigned)ceil_div(S, bb), (unsigned)(epochs * P)), kNormThreads, 0, s>>>(
            grow, S, bb, (int)P, x->epochs_per_agent);
        if (int rc3 = check_launch(what)) return rc3;
    }
    a.ws = reinterpret_cast<float *>(ws + (K > 1 ? pw.scratch : w.agents));
    a.params = x->params;
    a.m = x->exp_avg;
    a.v = x->exp_avg_sq;
    a.lr = x->lr;
    a.b1 = x->beta1;
    a.b2 = x->beta2;
    a.eps = x->eps;
    a.step = reinterpret_cast<long long *>(x->adam_step);
    a.gobs = gobs;
    a.gact = gact;
    a.gmask = gmask;
    a.grow = grow;
    a.S = S;
    a.E = (int)epochs;
    a.B = (int)(batch < S ? batch : S);
    a.P = (int)P;
    a.clip = x->clip_coef;
    a.vf = x->vf_coef;
    a.ent = x->ent_coef;
    a.max_norm = x->max_grad_norm;
    a.target_kl = x->target_kl;
    a.batch_p = x->batch_per_agent;
    a.epochs_p = x->epochs_per_agent;
    a.ent_p = x->ent_coef_per_agent;
    a.loss_out = x->loss_out;
    a.kl_out = x->kl_out;
    a.epochs_out = x->epochs_out;
    a.skip = x->skip_if_set;
    {
        const char *d = getenv("AGX_GRAPH_DEBUG");
        a.dbg = d ? atoi(d) : 0;
    }
    a.err = x->error_word;
    if (K > 1) {
        a.K = K;
        a.R = R;
        a.Q = Q;
        a.nslab = pw.nslab;
        a.wtb = reinterpret_cast<float *>(ws + pw.wt);
        a.slabs = reinterpret_cast<float *>(ws + pw.slabs);
        a.sums = reinterpret_cast<float *>(ws + pw.sums);
        a.cnt = counters;
        a.stamps = g_graph_stamps();
        {
            const char *wt = getenv("AGX_LEARN_WRITETHROUGH");
            a.write_through = wt && atoi(wt) != 0;
        }
        AGX_REQUIRE((int64_t)Q * K <= 65535, "%s: too many workgroups", what);
        if (sp.few)
            ppo_learn_graph_part_kernel<true, HEAD><<<(unsigned)(Q * K), kGT, sp.dyn, s>>>(a);
        else
            ppo_learn_graph_part_kernel<false, HEAD><<<(unsigned)(Q * K), kGT, 0, s>>>(a);
    } else {
        ppo_learn_graph_kernel<HEAD><<<(unsigned)P, kGT, 0, s>>>(a);
    }
    return check_launch(what);
}

// The entry points of a head: its check (check(h): the head's rules, filling h), then the query / the call
template <Head HEAD, class Check>
size_t checked_workspace_bytes(Check check, const agx_ppo_graph *net, int64_t P, int64_t S, int64_t epochs,
                               int64_t batch) {
    HeadArg h;
    if (check(h) != AGX_OK) return 0;
    return learn_graph_workspace_bytes<HEAD>(net, P, S, epochs, batch);
}
template <Head HEAD, class Check>
int checked_learn(const char *what, Check check, const agx_ppo_graph *net, const agx_ppo_learn_args *x,
                  void *workspace, void *stream) {
    AGX_REQUIRE(net && x && workspace, "%s: null net / args / workspace", what);
    HeadArg h;
    if (int rc = check(h)) return rc;
    return learn_graph<HEAD>(what, net, h, x, workspace, stream);
}

}  // namespace
}  // namespace agx

using namespace agx;

extern "C" int agx_debug_graph_stamps(int64_t *buf) {
    g_graph_stamps() = reinterpret_cast<long long *>(buf);
    return AGX_OK;
}

extern "C" int agx_ppo_graph_check(const agx_ppo_graph *net) {
    GArgs a{};
    return plan_graph(net, 1, a);
}

extern "C" size_t agx_ppo_learn_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t S,
                                                      int64_t epochs, int64_t batch) {
    return checked_workspace_bytes<kCat>([](HeadArg &) { return AGX_OK; }, net, P, S, epochs, batch);
}

extern "C" int agx_ppo_learn_graph(const agx_ppo_graph *net, const agx_ppo_learn_args *x, void *workspace,
                                   void *stream) {
    return checked_learn<kCat>("agx_ppo_learn_graph", [](HeadArg &) { return AGX_OK; }, net, x, workspace, stream);
}

extern "C" int agx_ppo_gauss_graph_check(const agx_ppo_graph *net, int64_t log_std_off) {
    return gauss_check(net, log_std_off);
}

extern "C" size_t agx_ppo_learn_gauss_graph_workspace_bytes(const agx_ppo_graph *net, int64_t log_std_off, int64_t P,
                                                            int64_t S, int64_t epochs, int64_t batch) {
    return checked_workspace_bytes<kGauss>([&](HeadArg &) { return gauss_check(net, log_std_off); }, net, P, S, epochs,
                                           batch);
}

extern "C" int agx_ppo_learn_gauss_graph(const agx_ppo_graph *net, int64_t log_std_off, const agx_ppo_learn_args *x,
                                         void *workspace, void *stream) {
    auto check = [&](HeadArg &h) -> int {
        if (int rc = gauss_check(net, log_std_off)) return rc;
        AGX_REQUIRE(!x->action_masks, "agx_ppo_learn_gauss_graph: action masks do not apply to a Gaussian head");
        h.lso = log_std_off;
        return AGX_OK;
    };
    return checked_learn<kGauss>("agx_ppo_learn_gauss_graph", check, net, x, workspace, stream);
}

extern "C" int agx_ppo_multi_graph_check(const agx_ppo_graph *net, agx_multi_head head) {
    HeadArg h;
    return multi_check("agx_ppo_multi_graph_check", net, head, h);
}

extern "C" size_t agx_ppo_learn_multi_graph_workspace_bytes(const agx_ppo_graph *net, agx_multi_head head, int64_t P,
                                                            int64_t S, int64_t epochs, int64_t batch) {
    auto check = [&](HeadArg &h) { return multi_check("agx_ppo_learn_multi_graph_workspace_bytes", net, head, h); };
    return checked_workspace_bytes<kMulti>(check, net, P, S, epochs, batch);
}

extern "C" int agx_ppo_learn_multi_graph(const agx_ppo_graph *net, agx_multi_head head, const agx_ppo_learn_args *x,
                                         void *workspace, void *stream) {
    auto check = [&](HeadArg &h) { return multi_check("agx_ppo_learn_multi_graph", net, head, h); };
    return checked_learn<kMulti>("agx_ppo_learn_multi_graph", check, net, x, workspace, stream);
}

extern "C" int agx_ppo_bern_graph_check(const agx_ppo_graph *net) {
    GArgs a{};
    AGX_REQUIRE(net, "agx_ppo_bern_graph_check: null graph");
    return plan_graph(net, 1, a);
}

extern "C" size_t agx_ppo_learn_bern_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t S,
                                                           int64_t epochs, int64_t batch) {
    return checked_workspace_bytes<kBern>([&](HeadArg &) { return agx_ppo_bern_graph_check(net); }, net, P, S, epochs,
                                          batch);
}

extern "C" int agx_ppo_learn_bern_graph(const agx_ppo_graph *net, const agx_ppo_learn_args *x, void *workspace,
                                        void *stream) {
    return checked_learn<kBern>("agx_ppo_learn_bern_graph", [&](HeadArg &) { return agx_ppo_bern_graph_check(net); },
                                net, x, workspace, stream);
}
