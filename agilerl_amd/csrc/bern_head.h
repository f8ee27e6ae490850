// The Bernoulli head's per-bit math (include/agx_bernoulli.h), shared by the
// policy step and loss kernels (bern_policy.hip) and the fused learner's row
// passes (graph_learner.hip): every bit is its own distribution, so all of it
// is elementwise per lane; a row needs two row sums (log-prob and entropy).
#pragma once

#include "agx_common.h"

namespace agx {

// sigmoid and log-sigmoid of both signs of one logit, from e = exp(-|l|):
// finite for |l| up to 1e8 (a masked logit: p = 0, q = 1, lq = 0 exactly)
struct BernBit {
    float p, q, lp, lq;
};
__device__ __forceinline__ BernBit bern_bit(float l) {
    const float e = expf(-fabsf(l));
    const float r = 1.f / (1.f + e), er = e * r;
    const float s = log1pf(e);
    BernBit b;
    b.p = l >= 0.f ? r : er;
    b.q = l >= 0.f ? er : r;
    b.lp = fminf(l, 0.f) - s;
    b.lq = fminf(-l, 0.f) - s;
    return b;
}
// the bit's term of -entropy: p log(p + 1e-8) + q log(q + 1e-8)
__device__ __forceinline__ float bern_neg_entropy(const BernBit &b) {
    return b.p * logf(b.p + 1e-8f) + b.q * logf(b.q + 1e-8f);
}
// dH/dl = -p q (t(p) - t(q)), t(x) = log(x + 1e-8) + x / (x + 1e-8)
__device__ __forceinline__ float bern_dH(const BernBit &b) {
    const float tp = logf(b.p + 1e-8f) + b.p / (b.p + 1e-8f);
    const float tq = logf(b.q + 1e-8f) + b.q / (b.q + 1e-8f);
    return -b.p * b.q * (tp - tq);
}
// d log_prob / dl = a - p, without the cancellation near p = 1
__device__ __forceinline__ float bern_dlogp(const BernBit &b, bool a) { return a ? b.q : -b.p; }

}  // namespace agx
