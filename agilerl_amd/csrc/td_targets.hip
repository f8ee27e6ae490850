// Scalar TD targets with an MSE loss: DQN's, MADDPG's critic, DDPG's critic
// and TD3's twin critics, plus TD3 / DDPG target-policy smoothing.
//
// DQN — agilerl/algorithms/dqn.py:296-314 (DQN.update):
//   q_t = max_a Qtgt(s')  |  Qtgt(s')[argmax_a Q(s')] (double)
//         (torch.max / torch.argmax: a NaN is the maximum, the first NaN's
//         index the argmax, ties take the first index)
//   y   = r + (gamma*q_t)*(1-d)        (f32, one rounding per op)
//   loss = MSE(Q(s)[a], y);  dloss/dQ(s)[a] = 2 (Q[a]-y) / B
// Critics — td3.py:503-515, ddpg.py:457-461 (one critic), maddpg.py:764-781:
//   y    = r + ((1 - d) * gamma) * min(Q1'(s', a'), Q2'(s', a'))
//   loss = MSE(Q1, y) + MSE(Q2, y);  dloss/dQk = 2 (Qk - y) / B
// MADDPG first sets NaN rewards to 0 and NaN dones to 1, casts the dones to
// uint8 (truncation) and forms 1 - d in uint8 arithmetic; MATD3
// (matd3.py:861-880) does the same in front of the twin form.
// Smoothing — td3.py:493-501, ddpg.py:448-456:
//   noise = clamp(N(0, policy_noise), -c, c)             (torch.clamp)
//   a'    = max(min(mu'(s') + noise, high), low)         (multi_dim_clamp)
// f32 throughout, one rounding per op (the reference's op order); every mean
// is accumulated in f64 over fixed-order block partials and rounded to f32,
// and TD3's two are added in f32, as the sum of two nn.MSELoss values.
#include "td_rules.h"

#include "../../include/agx_td3.h"

namespace agx {

// the block's squared errors into part1 / part2 [blockIdx], for loss_finalize
template <bool TWO>
__device__ __forceinline__ void block_partials(double s1, double s2, double *__restrict__ part1,
                                               double *__restrict__ part2) {
    if (block_sum<kTdBlock, TWO>(s1, s2)) {
        part1[blockIdx.x] = s1;
        if (TWO) part2[blockIdx.x] = s2;
    }
}

// loss = f32(sum(part1) / B) [+ f32(sum(part2) / B)], one block of 1024
template <bool TWO>
__global__ __launch_bounds__(1024) void loss_finalize(const double *__restrict__ part1,
                                                      const double *__restrict__ part2, int64_t nblk, int64_t B,
                                                      float *__restrict__ loss) {
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += 1024) {
        s1 += part1[i];
        if (TWO) s2 += part2[i];
    }
    if (block_sum<1024, TWO>(s1, s2)) {
        const float l1 = (float)(s1 / (double)B);
        *loss = TWO ? l1 + (float)(s2 / (double)B) : l1;
    }
}

// one row per lane.  A NaN among the next-state values is the row's maximum,
// as for torch.max / torch.argmax (argmax: the first NaN's index)
__global__ __launch_bounds__(kTdBlock) void td_target_kernel(
    const float *__restrict__ qno, const float *__restrict__ qnt, const float *__restrict__ qc,
    const int64_t *__restrict__ act, const float *__restrict__ r, const float *__restrict__ d, int64_t B, int A,
    float g, int dbl, float *__restrict__ y, float *__restrict__ g_q, double *__restrict__ partials) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double sq = 0.0;
    if (i < B) {
        const float qt = row_q_next(dbl ? qno + i * A : nullptr, qnt + i * A, A, dbl);
        const float yi = td_y(r[i], g, qt, d[i]);
        y[i] = yi;
        if (qc) {
            const int64_t ai = act[i];
            const float qa = qc[i * A + ai];
            if (g_q) {
                const float diff = qa - yi;
                const float scale = 2.0f / (float)B;
                for (int a = 0; a < A; ++a) g_q[i * A + a] = (a == ai) ? diff * scale : 0.0f;
            }
            const double dd = (double)qa - (double)yi;
            sq = dd * dd;
        }
    }
    if (partials) block_partials<false>(sq, 0.0, partials, nullptr);
}

// one row per lane.  TWIN: two critics against the smaller target value;
// SANITIZE: MADDPG's NaN and uint8 handling of r and d
template <bool TWIN, bool SANITIZE>
__global__ __launch_bounds__(kTdBlock) void critic_target_kernel(
    const float *__restrict__ q1, const float *__restrict__ q2, const float *__restrict__ qn1,
    const float *__restrict__ qn2, const float *__restrict__ r, const float *__restrict__ d, int64_t B, float g,
    float *__restrict__ y, float *__restrict__ g_q1, float *__restrict__ g_q2, double *__restrict__ part1,
    double *__restrict__ part2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double sq1 = 0.0, sq2 = 0.0;
    if (i < B) {
        float ri = r[i], nd;
        if (SANITIZE) {
            ri = __builtin_isnan(ri) ? 0.0f : ri;
            const float di = __builtin_isnan(d[i]) ? 1.0f : d[i];
            const unsigned char du = (unsigned char)(int)di;  // .to(torch.uint8)
            nd = (float)(unsigned char)(1u - du);              // 1 - uint8 tensor (wraps)
        } else {
            nd = 1.0f - d[i];
        }
        const float qn = TWIN ? nan_min(qn1[i], qn2[i]) : qn1[i];
        const float yi = ri + (nd * g) * qn;
        if (y) y[i] = yi;
        const float scale = 2.0f / (float)B;
        const float a = q1[i];
        if (g_q1) g_q1[i] = (a - yi) * scale;
        const double d1 = (double)a - (double)yi;
        sq1 = d1 * d1;
        if (TWIN) {
            const float b = q2[i];
            if (g_q2) g_q2[i] = (b - yi) * scale;
            const double d2 = (double)b - (double)yi;
            sq2 = d2 * d2;
        }
    }
    block_partials<TWIN>(sq1, sq2, part1, part2);
}

// one element per lane over B*A; out may alias mu (each lane reads its own
// element before it writes it)
__global__ __launch_bounds__(kTdBlock) void td3_smooth_kernel(const float *mu, const float *__restrict__ noise,
                                                              const float *__restrict__ low,
                                                              const float *__restrict__ high, int64_t n, int A,
                                                              float c, float *out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int k = (int)(i % A);
    float e = noise[i];
    e = e < -c ? -c : e;  // clamp(min=-c, max=c) = min(max(e, -c), c); a NaN e stays
    e = e > c ? c : e;
    const float s = mu[i] + e;
    out[i] = nan_max(nan_min(s, high[k]), low[k]);
}

// launch one critic_target_kernel instance and the loss sum over its partials
template <bool TWIN, bool SANITIZE>
static int critic_target(const char *what, const char *what_loss, const float *q1, const float *q2, const float *qn1,
                         const float *qn2, const float *r, const float *d, int64_t B, double gamma, float *y,
                         float *g_q1, float *g_q2, float *loss, void *workspace, void *stream) {
    hipStream_t s = as_stream(stream);
    const int64_t nblk = ceil_div(B, kTdBlock);
    double *part1 = static_cast<double *>(workspace);
    double *part2 = TWIN ? part1 + nblk : nullptr;
    critic_target_kernel<TWIN, SANITIZE><<<(unsigned)nblk, kTdBlock, 0, s>>>(q1, q2, qn1, qn2, r, d, B, (float)gamma,
                                                                            y, g_q1, g_q2, part1, part2);
    int rc = check_launch(what);
    if (rc) return rc;
    loss_finalize<TWIN><<<1, 1024, 0, s>>>(part1, part2, nblk, B, loss);
    return check_launch(what_loss);
}

}  // namespace agx

using namespace agx;

extern "C" size_t agx_td_workspace_bytes(int64_t B) {
    return B > 0 ? (size_t)ceil_div(B, kTdBlock) * sizeof(double) : 0;
}

extern "C" size_t agx_td3_workspace_bytes(int64_t B) { return 2 * agx_td_workspace_bytes(B); }

extern "C" int agx_td_target(const float *q_next_online, const float *q_next_target,
                             const float *q_cur, const int64_t *actions, const float *rewards,
                             const float *dones, int64_t B, int64_t A, double gamma, int double_q,
                             float *y, float *g_q, float *loss, void *workspace, void *stream) {
    AGX_REQUIRE(q_next_target && rewards && dones && y && B >= 0 && A > 0 && A < 65536,
                "agx_td_target: bad arguments");
    AGX_REQUIRE(!double_q || q_next_online, "agx_td_target: double_q needs q_next_online");
    AGX_REQUIRE(!(g_q || loss) || (q_cur && actions), "agx_td_target: loss needs q_cur/actions");
    AGX_REQUIRE(!loss || workspace, "agx_td_target: loss needs the workspace (agx_td_workspace_bytes)");
    if (B == 0) return AGX_OK;
    hipStream_t s = as_stream(stream);
    const int64_t nblk = ceil_div(B, kTdBlock);
    double *part = loss ? static_cast<double *>(workspace) : nullptr;
    td_target_kernel<<<(unsigned)nblk, kTdBlock, 0, s>>>(q_next_online, q_next_target, q_cur, actions, rewards,
                                                         dones, B, (int)A, (float)gamma, double_q, y, g_q, part);
    int rc = check_launch("agx_td_target");
    if (rc || !loss) return rc;
    loss_finalize<false><<<1, 1024, 0, s>>>(part, nullptr, nblk, B, loss);
    return check_launch("agx_td_target loss");
}

extern "C" int agx_maddpg_critic_target(const float *q, const float *q_next, const float *rewards,
                                        const float *dones, int64_t B, double gamma, float *y, float *g_q,
                                        float *loss, void *workspace, void *stream) {
    AGX_REQUIRE(q && q_next && rewards && dones && loss && workspace && B >= 0,
                "agx_maddpg_critic_target: bad arguments");
    if (B == 0) return AGX_OK;
    return critic_target<false, true>("agx_maddpg_critic_target", "agx_maddpg_critic_target loss", q, nullptr, q_next,
                                      nullptr, rewards, dones, B, gamma, y, g_q, nullptr, loss, workspace, stream);
}

extern "C" int agx_td3_smooth_actions(const float *mu, const float *noise, const float *low, const float *high,
                                      int64_t B, int64_t A, double noise_clip, float *out, void *stream) {
    AGX_REQUIRE(mu && noise && low && high && out, "agx_td3_smooth_actions: null pointer");
    AGX_REQUIRE(B >= 0 && A > 0 && A < 65536, "agx_td3_smooth_actions: need B >= 0 and 0 < A < 65536");
    AGX_REQUIRE(B <= (int64_t)0x7fffffff * kTdBlock / A, "agx_td3_smooth_actions: B * A exceeds the grid");
    if (B == 0) return AGX_OK;
    const int64_t n = B * A;
    td3_smooth_kernel<<<(unsigned)ceil_div(n, kTdBlock), kTdBlock, 0, as_stream(stream)>>>(
        mu, noise, low, high, n, (int)A, (float)noise_clip, out);
    return check_launch("agx_td3_smooth_actions");
}

extern "C" int agx_td3_critic_target(const float *q1, const float *q2, const float *q_next1, const float *q_next2,
                                     const float *rewards, const float *dones, int64_t B, double gamma, float *y,
                                     float *g_q1, float *g_q2, float *loss, void *workspace, void *stream) {
    AGX_REQUIRE(q1 && q_next1 && rewards && dones && loss && workspace && B >= 0,
                "agx_td3_critic_target: bad arguments");
    AGX_REQUIRE((q2 != nullptr) == (q_next2 != nullptr),
                "agx_td3_critic_target: q2 and q_next2 go together (both NULL: the single-critic form)");
    AGX_REQUIRE(q2 || !g_q2, "agx_td3_critic_target: g_q2 needs q2");
    AGX_REQUIRE(B <= (int64_t)0x7fffffff * kTdBlock, "agx_td3_critic_target: B exceeds the grid");
    if (B == 0) return AGX_OK;
    auto launch = q2 ? critic_target<true, false> : critic_target<false, false>;
    return launch("agx_td3_critic_target", "agx_td3_critic_target loss", q1, q2, q_next1, q_next2, rewards, dones, B,
                  gamma, y, g_q1, g_q2, loss, workspace, stream);
}

extern "C" int agx_matd3_critic_target(const float *q1, const float *q2, const float *q_next1, const float *q_next2,
                                       const float *rewards, const float *dones, int64_t B, double gamma, float *y,
                                       float *g_q1, float *g_q2, float *loss, void *workspace, void *stream) {
    AGX_REQUIRE(q1 && q2 && q_next1 && q_next2 && rewards && dones && loss && workspace && B >= 0,
                "agx_matd3_critic_target: bad arguments");
    AGX_REQUIRE(B <= (int64_t)0x7fffffff * kTdBlock, "agx_matd3_critic_target: B exceeds the grid");
    if (B == 0) return AGX_OK;
    return critic_target<true, true>("agx_matd3_critic_target", "agx_matd3_critic_target loss", q1, q2, q_next1,
                                     q_next2, rewards, dones, B, gamma, y, g_q1, g_q2, loss, workspace, stream);
}
