// The per-sample PPO clipped-surrogate loss (ppo.py:868-902) and the
// minibatch reduction shared by agx_ppo_loss_fwd_bwd (ppo_loss.hip: a
// ready-made log-prob and entropy per row) and the head losses with the
// head fused in (gauss_policy.hip, multi_policy.hip, bern_policy.hip).
#pragma once

#include "agx_common.h"

namespace agx {

struct LossCoef {
    float lo, hi, clip, vf_half_inv_b, inv_b, g_h, vf, ent;
};

// the coefficients of a minibatch of `batch` rows (the loss entry points' fill)
inline LossCoef loss_coef(int64_t batch, float clip_coef, float vf_coef, float ent_coef) {
    LossCoef k;
    k.clip = clip_coef;
    k.lo = 1.f - clip_coef;
    k.hi = 1.f + clip_coef;
    k.inv_b = 1.f / (float)batch;
    k.vf = vf_coef;
    k.ent = ent_coef;
    k.vf_half_inv_b = vf_coef * 0.5f * k.inv_b;
    k.g_h = -ent_coef * k.inv_b;
    return k;
}

struct Acc {
    float pg = 0.f, vl = 0.f, h = 0.f, kl = 0.f, cf = 0.f;
    __device__ __forceinline__ void add(const Acc &o) {
        pg += o.pg;
        vl += o.vl;
        h += o.h;
        kl += o.kl;
        cf += o.cf;
    }
};

__device__ __forceinline__ void loss_sample(float lp, float olp, float A, float R, float ov,
                                            float v, float H, const LossCoef &k, float &g_lp,
                                            float &g_v, Acc &acc) {
    const float lr = lp - olp;
    const float ratio = expf(lr);
    const float rc = fminf(fmaxf(ratio, k.lo), k.hi);
    const float p1 = -A * ratio;
    const float p2 = -A * rc;
    const float g1 = p1 > p2 ? 1.f : (p1 == p2 ? 0.5f : 0.f);
    const float g2 = p2 > p1 ? 1.f : (p1 == p2 ? 0.5f : 0.f);
    const float inr = (ratio >= k.lo && ratio <= k.hi) ? 1.f : 0.f;
    g_lp = ((g1 * -A + g2 * -A * inr) * k.inv_b) * ratio;
    const float dv = v - ov;
    const float dvc = fminf(fmaxf(dv, -k.clip), k.clip);
    const float vc = ov + dvc;
    const float eu = v - R;
    const float ec = vc - R;
    const float lu = eu * eu;
    const float lc = ec * ec;
    const float gu = lu > lc ? 1.f : (lu == lc ? 0.5f : 0.f);
    const float gc = lc > lu ? 1.f : (lu == lc ? 0.5f : 0.f);
    const float inv = (dv >= -k.clip && dv <= k.clip) ? 1.f : 0.f;
    g_v = k.vf_half_inv_b * (gu * 2.f * eu + gc * 2.f * ec * inv);
    acc.pg += fmaxf(p1, p2);
    acc.vl += fmaxf(lu, lc);
    acc.h += H;
    acc.kl += (ratio - 1.f) - lr;
    acc.cf += fabsf(ratio - 1.f) > k.clip ? 1.f : 0.f;
}

template <int G>
__device__ __forceinline__ void finish_group(Acc acc, const LossCoef &k, int64_t m, int lane_g,
                                             float *__restrict__ stats) {
    acc.pg = group_sum<G>(acc.pg);
    acc.vl = group_sum<G>(acc.vl);
    acc.h = group_sum<G>(acc.h);
    acc.kl = group_sum<G>(acc.kl);
    acc.cf = group_sum<G>(acc.cf);
    if (lane_g == 0 && stats) {
        const float pg = acc.pg * k.inv_b;
        const float vl = 0.5f * acc.vl * k.inv_b;
        const float el = -acc.h * k.inv_b;
        float *s = stats + m * 8;
        s[0] = pg + k.vf * vl + k.ent * el;
        s[1] = pg;
        s[2] = vl;
        s[3] = el;
        s[4] = acc.kl * k.inv_b;
        s[5] = acc.cf * k.inv_b;
        s[6] = 0.f;
        s[7] = 0.f;
    }
}

}  // namespace agx
