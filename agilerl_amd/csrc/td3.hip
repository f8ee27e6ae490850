// TD3 / DDPG target step: target-policy smoothing and the (twin-)critic TD
// target with the MSE loss and its gradients.
//
// Smoothing — agilerl/algorithms/td3.py:493-501, ddpg.py:448-456:
//   noise = clamp(N(0, policy_noise), -c, c)             (torch.clamp)
//   a'    = max(min(mu'(s') + noise, high), low)         (multi_dim_clamp)
// Critic target — td3.py:503-515 (ddpg.py:457-461 with one critic):
//   y    = r + ((1 - d) * gamma) * min(Q1'(s', a'), Q2'(s', a'))
//   loss = MSE(Q1, y) + MSE(Q2, y);  dloss/dQk = 2 (Qk - y) / B
// f32 throughout, one rounding per op (the reference's op order); the two
// means are accumulated in f64 over fixed-order block partials, rounded to
// f32 each and added in f32, as the sum of two nn.MSELoss values.
#include "agx_common.h"

#include "../../include/agx_td3.h"

namespace agx {

constexpr int kTd3Block = 256;

// torch.min / torch.max (and clamp) propagate NaN; fminf / fmaxf do not
__device__ __forceinline__ float nan_min(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return fminf(a, b);
}
__device__ __forceinline__ float nan_max(float a, float b) {
    if (a != a) return a;
    if (b != b) return b;
    return fmaxf(a, b);
}

// one element per lane over B*A; out may alias mu (each lane reads its own
// element before it writes it)
__global__ __launch_bounds__(kTd3Block) void td3_smooth_kernel(const float *mu, const float *__restrict__ noise,
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

// one row per lane; each critic's squared errors are reduced per block (f64,
// fixed order) into part1 / part2 [blockIdx] and summed by td3_loss_finalize
__global__ __launch_bounds__(kTd3Block) void td3_critic_kernel(
    const float *__restrict__ q1, const float *__restrict__ q2, const float *__restrict__ qn1,
    const float *__restrict__ qn2, const float *__restrict__ r, const float *__restrict__ d, int64_t B, float g,
    float *__restrict__ y, float *__restrict__ g_q1, float *__restrict__ g_q2, double *__restrict__ part1,
    double *__restrict__ part2) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    double sq1 = 0.0, sq2 = 0.0;
    if (i < B) {
        const float qn = qn2 ? nan_min(qn1[i], qn2[i]) : qn1[i];
        const float yi = r[i] + ((1.0f - d[i]) * g) * qn;
        if (y) y[i] = yi;
        const float scale = 2.0f / (float)B;
        const float a = q1[i];
        if (g_q1) g_q1[i] = (a - yi) * scale;
        const double d1 = (double)a - (double)yi;
        sq1 = d1 * d1;
        if (q2) {
            const float b = q2[i];
            if (g_q2) g_q2[i] = (b - yi) * scale;
            const double d2 = (double)b - (double)yi;
            sq2 = d2 * d2;
        }
    }
    __shared__ double red[2][kTd3Block / kWave];
    sq1 = wave_sum(sq1);
    sq2 = wave_sum(sq2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x / 64] = sq1;
        red[1][threadIdx.x / 64] = sq2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < kTd3Block / kWave; ++w) {
            t1 += red[0][w];
            t2 += red[1][w];
        }
        part1[blockIdx.x] = t1;
        if (part2) part2[blockIdx.x] = t2;
    }
}

// loss = f32(sum(part1) / B) [+ f32(sum(part2) / B)], one block
__global__ __launch_bounds__(1024) void td3_loss_finalize(const double *__restrict__ part1,
                                                          const double *__restrict__ part2, int64_t nblk, int64_t B,
                                                          float *__restrict__ loss) {
    __shared__ double red[2][1024 / kWave];
    double s1 = 0.0, s2 = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += blockDim.x) {
        s1 += part1[i];
        if (part2) s2 += part2[i];
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x / 64] = s1;
        red[1][threadIdx.x / 64] = s2;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double t1 = 0.0, t2 = 0.0;
        for (int w = 0; w < (int)(blockDim.x / 64); ++w) {
            t1 += red[0][w];
            t2 += red[1][w];
        }
        const float l1 = (float)(t1 / (double)B);
        *loss = part2 ? l1 + (float)(t2 / (double)B) : l1;
    }
}

}  // namespace agx

using namespace agx;

extern "C" int agx_td3_smooth_actions(const float *mu, const float *noise, const float *low, const float *high,
                                      int64_t B, int64_t A, double noise_clip, float *out, void *stream) {
    AGX_REQUIRE(mu && noise && low && high && out, "agx_td3_smooth_actions: null pointer");
    AGX_REQUIRE(B >= 0 && A > 0 && A < 65536, "agx_td3_smooth_actions: need B >= 0 and 0 < A < 65536");
    AGX_REQUIRE(B <= (int64_t)0x7fffffff * kTd3Block / A, "agx_td3_smooth_actions: B * A exceeds the grid");
    if (B == 0) return AGX_OK;
    const int64_t n = B * A;
    td3_smooth_kernel<<<(unsigned)ceil_div(n, kTd3Block), kTd3Block, 0, as_stream(stream)>>>(
        mu, noise, low, high, n, (int)A, (float)noise_clip, out);
    return check_launch("agx_td3_smooth_actions");
}

extern "C" size_t agx_td3_workspace_bytes(int64_t B) {
    return B > 0 ? 2 * (size_t)ceil_div(B, kTd3Block) * sizeof(double) : 0;
}

extern "C" int agx_td3_critic_target(const float *q1, const float *q2, const float *q_next1, const float *q_next2,
                                     const float *rewards, const float *dones, int64_t B, double gamma, float *y,
                                     float *g_q1, float *g_q2, float *loss, void *workspace, void *stream) {
    AGX_REQUIRE(q1 && q_next1 && rewards && dones && loss && workspace && B >= 0,
                "agx_td3_critic_target: bad arguments");
    AGX_REQUIRE((q2 != nullptr) == (q_next2 != nullptr),
                "agx_td3_critic_target: q2 and q_next2 go together (both NULL: the single-critic form)");
    AGX_REQUIRE(q2 || !g_q2, "agx_td3_critic_target: g_q2 needs q2");
    AGX_REQUIRE(B <= (int64_t)0x7fffffff * kTd3Block, "agx_td3_critic_target: B exceeds the grid");
    if (B == 0) return AGX_OK;
    hipStream_t s = as_stream(stream);
    const int64_t nblk = ceil_div(B, kTd3Block);
    double *part1 = static_cast<double *>(workspace);
    double *part2 = q2 ? part1 + nblk : nullptr;
    td3_critic_kernel<<<(unsigned)nblk, kTd3Block, 0, s>>>(q1, q2, q_next1, q_next2, rewards, dones, B, (float)gamma,
                                                           y, g_q1, g_q2, part1, part2);
    int rc = check_launch("agx_td3_critic_target");
    if (rc) return rc;
    td3_loss_finalize<<<1, 1024, 0, s>>>(part1, part2, nblk, B, loss);
    return check_launch("agx_td3_critic_target loss");
}
