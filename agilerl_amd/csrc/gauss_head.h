// The per-row math of the diagonal-Gaussian head (include/agx_gauss.h): one
// dimension's log-prob term, the entropy, and the gradients of the mean and of
// log_std.  Shared by the loss kernel (gauss_policy.hip) and the Gaussian head
// of the runtime-shape learner (graph_learner.hip): the same float operations
// in the same order in both.
#pragma once

#include "agx_common.h"

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

// d log_prob / d mu_d = z / var, times the row's d loss / d log_prob
__device__ __forceinline__ float gauss_g_mean(float gl, float z, float iv) { return gl * (z * iv); }

// d log_prob / d log_std_d = z^2 / var - 1, times the row's d loss / d log_prob
// (the entropy's -ent_coef is the caller's: it does not depend on the row)
__device__ __forceinline__ float gauss_g_log_std(float gl, float z, float iv) { return gl * (z * z * iv - 1.f); }

}  // namespace agx
