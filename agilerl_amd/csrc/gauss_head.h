// The per-row math of the diagonal-Gaussian head (include/agx_gauss.h): one
// dimension's log-prob term, the entropy, the gradients of the mean and of
// log_std, and the step's Philox noise.  Shared by the loss kernel and policy
// step (gauss_policy.hip), the Gaussian head of the runtime-shape learner
// (graph_learner.hip) and the recurrent policy step (recurrent_policy.hip):
// the same float operations in the same order in all of them.
#pragma once

#include "agx_common.h"
#include "rollout.h"

namespace agx {

constexpr float kLog2Pi = 1.8378770664093453f;         // log(2 pi)
constexpr double kGaussEntropy = 1.4189385332046727;   // 0.5 (1 + log(2 pi)) per dimension

// one dimension's log-prob term of action a under N(mu, exp(log_std)^2)
__device__ __forceinline__ float gauss_logp_term(float a, float mu, float ls) {
    const float z = a - mu;
    return -0.5f * (z * z / expf(2.f * ls) + 2.f * ls + kLog2Pi);
}

// 1 / variance of a dimension
__device__ __forceinline__ float gauss_inv_var(float ls) { return 1.f / expf(2.f * ls); }

// entropy of a row from the sum of its A log_std
__device__ __forceinline__ float gauss_entropy(int A, float ls_sum) {
    return (float)(kGaussEntropy * (double)A) + ls_sum;
}

// eps of dimension d (agx_gauss.h): words (x, y) (d even) or (z, w) (d odd) of
// the Philox block of (env, counter ^ (d >> 1) << 56) -> u1, u2 -> Box-Muller.
// u = fl((w >> 8) + 0.5) 2^-24 as gumbel_score's: in (0, 1], so ln u1 is finite.
__device__ __forceinline__ float gauss_noise(int d, unsigned long long env, unsigned long long seed,
                                             unsigned long long counter) {
    const uint4 rnd = philox(make_uint4((unsigned)env, (unsigned)(env >> 32), (unsigned)counter,
                                        (unsigned)(counter >> 32) ^ ((unsigned)(d >> 1) << 24)),
                             make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const unsigned w1 = (d & 1) ? rnd.z : rnd.x, w2 = (d & 1) ? rnd.w : rnd.y;
    const float u1 = ((float)(w1 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(w2 >> 8) + 0.5f) * (1.0f / 16777216.0f);
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// d log_prob / d mu_d = z / var, times the row's d loss / d log_prob
__device__ __forceinline__ float gauss_g_mean(float gl, float z, float iv) { return gl * (z * iv); }

// d log_prob / d log_std_d = z^2 / var - 1, times the row's d loss / d log_prob
// (the entropy's -ent_coef is the caller's: it does not depend on the row)
__device__ __forceinline__ float gauss_g_log_std(float gl, float z, float iv) { return gl * (z * z * iv - 1.f); }

}  // namespace agx
