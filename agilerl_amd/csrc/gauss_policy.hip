// PPO for Box action spaces (include/agx_gauss.h): the diagonal-Gaussian
// policy step over a runtime layer list (graph_net.h's forward, then the
// Gaussian step, as graph_rollout.hip's categorical one) and the Gaussian twin
// of agx_ppo_loss_fwd_bwd (log-prob of the stored action, entropy, the clipped
// loss of ppo_loss_sample.h and the gradients of mean / value / log_std in one
// pass).
#include "../../include/agx_gauss.h"
#include "gauss_head.h"
#include "graph_net.h"
#include "head_policy.h"
#include "ppo_loss_sample.h"
#include "rollout.h"

namespace agx {
namespace {

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

// what the Gaussian step writes besides the ActArgs' log_probs / values / entropy
struct GaussHead {
    long long log_std_off;  // the A log_std floats in the parameter row
    float *act_out;         // agent p, env n, dimension d at ((p out_pstride + n) A + d)
    float *act_flat;        // [P N A] host staging, or null
    const float *lo, *hi;   // [A] bounds of the act_flat copy, or null
};

// The Gaussian step of rows [0, nrow) of agent p's row block n0 (means at
// mup [nrow][A] with row stride lda, values at vp with stride ldv): 16 lanes
// per row, dimensions d and d + 16 per lane, as graph_sample.
__device__ __forceinline__ void gauss_step(const ActArgs &g, const GaussHead &h, int A, int lda, int ldv,
                                           const float *mup, const float *vp, const float *log_std, int p, int n0,
                                           int nrow) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int d0 = sub, d1 = sub + 16;
    const bool on0 = d0 < A, on1 = d1 < A;
    const float ls0 = on0 ? log_std[d0] : 0.f, ls1 = on1 ? log_std[d1] : 0.f;
    const float H = gauss_entropy(A, row_sum(ls0 + ls1));
    for (int r0 = 0; r0 < nrow; r0 += 4 * kGW) {
        const int r = r0 + 4 * wave + rq;
        const bool live = r < nrow;
        const int rr = live ? r : 0;
        const float mu0 = on0 ? mup[(size_t)rr * lda + d0] : 0.f;
        const float mu1 = on1 ? mup[(size_t)rr * lda + d1] : 0.f;
        float a0 = mu0, a1 = mu1;
        if (g.sample) {
            const unsigned long long env = stream_env(-1, g.env_base, p, g.N, n0 + rr);
            if (on0) a0 = fmaf(expf(ls0), gauss_noise(d0, env, g.seed, g.counter), mu0);
            if (on1) a1 = fmaf(expf(ls1), gauss_noise(d1, env, g.seed, g.counter), mu1);
        }
        // from the stored (rounded) action, as the learner recomputes it
        const float lp = row_sum((on0 ? gauss_logp_term(a0, mu0, ls0) : 0.f) + (on1 ? gauss_logp_term(a1, mu1, ls1) : 0.f));
        if (!live) continue;
        const size_t row = (size_t)p * g.out_pstride + n0 + r;
        if (h.act_out) {
            if (on0) h.act_out[row * A + d0] = a0;
            if (on1) h.act_out[row * A + d1] = a1;
        }
        if (h.act_flat) {  // host staging: system-scope (write-through) stores, clipped for the env
            float *f = h.act_flat + ((size_t)p * g.N + n0 + r) * A;
            if (on0)
                __hip_atomic_store(f + d0, h.lo ? fminf(fmaxf(a0, h.lo[d0]), h.hi[d0]) : a0, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
            if (on1)
                __hip_atomic_store(f + d1, h.lo ? fminf(fmaxf(a1, h.lo[d1]), h.hi[d1]) : a1, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (sub == 0) {
            if (g.logp_out) g.logp_out[row] = lp;
            if (g.ent_out) g.ent_out[row] = H;
            if (g.value_out) g.value_out[row] = vp[(size_t)r * ldv];
        }
    }
}

// Policy step of workgroup (p, row block): forward through the layer list
// (ppo_act_graph_kernel's two forms), then gauss_step.
template <bool FEW>
__global__ __launch_bounds__(kGT) void ppo_act_gauss_graph_kernel(const GActArgs ga, const ActArgs g,
                                                                  const GaussHead h) {
    __shared__ __attribute__((aligned(16))) float lds[kGemmLds];
    extern __shared__ __attribute__((aligned(16))) float gdyn[];
    const int p = blockIdx.y, n0 = blockIdx.x * ga.rows;
    const int nrow = g.N - n0 < ga.rows ? g.N - n0 : ga.rows;
    const float *pr = g.params + (size_t)p * ga.n;
    const float *obs = g.obs + (size_t)p * g.obs_pstride + (size_t)n0 * ga.D;
    const GLay &La = ga.L[ga.aout], &Lc = ga.L[ga.cout];
    if constexpr (FEW) {
        const int tid = threadIdx.x;
        for (int i = tid; i < (int)ga.lds_floats; i += kGT) gdyn[i] = 0.f;
        __syncthreads();
        for (int i = tid; i < nrow * ga.D; i += kGT) {
            const int b = i / ga.D, d = i - b * ga.D;
            gdyn[ga.oc + b * ga.ld0 + d] = obs[i];
        }
        __syncthreads();
        const auto prs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pr), 0,
                                                           __builtin_amdgcn_readfirstlane(ga.n * 4), 0x00020000);
        few_forward(ga.L, ga.nl, gdyn, pr, prs, ga.oc, ga.ld0, nullptr);
        gauss_step(g, h, ga.A, La.ld, Lc.ld, gdyn + La.yr, gdyn + Lc.yr, pr + h.log_std_off, p, n0, nrow);
    } else {
        float *base = ga.ws + ((size_t)p * gridDim.x + blockIdx.x) * ga.ws_block;
        forward_layers(ga.L, ga.nl, obs, nrow, base, pr, ga.rows, lds);
        gauss_step(g, h, ga.A, ga.A, 1, base + La.yr, base + Lc.yr, pr + h.log_std_off, p, n0, nrow);
    }
}

// gauss_step as the step of head_policy.h's persistent loop: the step's action
// slot / host staging are floats [.., A], the staging copy clipped to lo / hi
struct GaussRolloutHead {
    long long log_std_off;
    const float *lo, *hi;  // [A] device, or null
    __device__ __forceinline__ void step(const ActArgs &g, int A, int lda, int ldv, const float *mup, const float *vp,
                                         const float *pr, int p, int n0, int nrow) const {
        const GaussHead h{log_std_off, reinterpret_cast<float *>(g.act_out), reinterpret_cast<float *>(g.act_flat),
                          lo, hi};
        gauss_step(g, h, A, lda, ldv, mup, vp, pr + log_std_off, p, n0, nrow);
    }
};

// ---------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------
// One wave per minibatch m: 16 lanes per row (dimensions d and d + 16 per
// lane), four rows at a time; every lane of a row holds the row's log-prob
// (row_sum) and so its loss terms, lane 0 of the row counts them.  A lane sums
// its dimensions' log_std gradient over its rows (q, q + 4, ..: a fixed
// order), then the four row quarters add up through xor butterflies.
__global__ __launch_bounds__(256) void ppo_gauss_loss_kernel(
    const float *__restrict__ mean, const float *__restrict__ value, const float *__restrict__ log_std,
    const float *__restrict__ actions, const float *__restrict__ old_logp, const float *__restrict__ adv,
    const float *__restrict__ ret, const float *__restrict__ old_v, const int64_t *__restrict__ index, int64_t b,
    int64_t nmb, int A, LossCoef k, float *__restrict__ g_mean, float *__restrict__ g_value,
    float *__restrict__ g_log_std, float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= nmb) return;  // whole waves exit together
    const int sub = lane & 15, rq = lane >> 4;
    const int d0 = sub, d1 = sub + 16;
    const bool on0 = d0 < A, on1 = d1 < A;
    const float ls0 = on0 ? log_std[m * A + d0] : 0.f, ls1 = on1 ? log_std[m * A + d1] : 0.f;
    const float iv0 = gauss_inv_var(ls0), iv1 = gauss_inv_var(ls1);
    const float H = gauss_entropy(A, row_sum(ls0 + ls1));
    Acc acc;
    float gs0 = 0.f, gs1 = 0.f;
    const int64_t base = m * b;
    for (int64_t j0 = 0; j0 < b; j0 += 4) {  // wave-uniform trip count (row_sum needs whole rows)
        const int64_t j = j0 + rq;
        const bool live = j < b;
        const int64_t o = base + (live ? j : 0);
        const int64_t src = index ? index[o] : o;
        const float mu0 = on0 ? mean[o * A + d0] : 0.f, mu1 = on1 ? mean[o * A + d1] : 0.f;
        const float a0 = on0 ? actions[src * A + d0] : 0.f, a1 = on1 ? actions[src * A + d1] : 0.f;
        const float lp = row_sum((on0 ? gauss_logp_term(a0, mu0, ls0) : 0.f) + (on1 ? gauss_logp_term(a1, mu1, ls1) : 0.f));
        if (!live) continue;
        float gl, gv;
        Acc one;
        loss_sample(lp, old_logp[src], adv[src], ret[src], old_v[src], value[o], H, k, gl, gv, one);
        if (sub == 0) {
            acc.add(one);
            g_value[o] = gv;
        }
        const float z0 = a0 - mu0, z1 = a1 - mu1;
        if (on0) {
            g_mean[o * A + d0] = gauss_g_mean(gl, z0, iv0);
            gs0 += gauss_g_log_std(gl, z0, iv0);
        }
        if (on1) {
            g_mean[o * A + d1] = gauss_g_mean(gl, z1, iv1);
            gs1 += gauss_g_log_std(gl, z1, iv1);
        }
    }
    gs0 += __shfl_xor(gs0, 16, 64);
    gs0 += __shfl_xor(gs0, 32, 64);
    gs1 += __shfl_xor(gs1, 16, 64);
    gs1 += __shfl_xor(gs1, 32, 64);
    if (rq == 0) {  // d(-ent mean(H)) / d log_std_d = -ent
        if (on0) g_log_std[m * A + d0] = gs0 - k.ent;
        if (on1) g_log_std[m * A + d1] = gs1 - k.ent;
    }
    finish_group<64>(acc, k, m, lane, stats);
}

}  // namespace
}  // namespace agx

using namespace agx;

namespace {
// the layer list of a Gaussian actor-critic: its log_std floats are the part
// of the parameter row that no layer owns
int gauss_graph(const agx_ppo_graph *net, GArgs &full) { return plan_graph(net, 1, full, net->n_actions); }

// the rules of every Gaussian entry point for the net and the head -> the plan and the persistent kernel's head
int gauss_plan(const agx_ppo_graph *net, int64_t log_std_off, const float *clip_low, const float *clip_high,
               GArgs &full, GaussRolloutHead &h, const char *who) {
    AGX_REQUIRE(!clip_low == !clip_high, "%s: clip_low and clip_high come together", who);
    if (int rc = gauss_graph(net, full)) return rc;
    AGX_REQUIRE(log_std_off >= 0 && log_std_off + net->n_actions <= net->n_params,
                "%s: log_std outside the parameter row", who);
    h = GaussRolloutHead{(long long)log_std_off, clip_low, clip_high};
    return AGX_OK;
}
}  // namespace

extern "C" size_t agx_ppo_act_gauss_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t N) {
    GArgs full{};
    if (!net || P <= 0 || N <= 0 || gauss_graph(net, full) != AGX_OK) return 0;
    return head_act_workspace_bytes(full, P, N);
}

extern "C" int agx_ppo_act_gauss_graph(const agx_ppo_graph *net, int64_t log_std_off, int64_t P, int64_t N,
                                       const float *params, const float *obs, int64_t obs_agent_stride, int sample,
                                       uint64_t seed, uint64_t counter, float *actions, float *log_probs,
                                       float *values, float *entropy, int64_t out_agent_stride, float *actions_flat,
                                       const float *clip_low, const float *clip_high, const int64_t *agent_env_base,
                                       void *workspace, void *stream) {
    const char *who = "agx_ppo_act_gauss_graph";
    AGX_REQUIRE(net && params && obs && workspace && P > 0 && N > 0 && P <= 65535, "%s: bad arguments", who);
    GArgs full{};
    GaussRolloutHead r{};
    if (int rc = gauss_plan(net, log_std_off, clip_low, clip_high, full, r, who)) return rc;
    const ActArgs g = act_step_args(P, N, params, obs, obs_agent_stride, nullptr, 0, sample, seed, counter, nullptr,
                                    log_probs, values, entropy, out_agent_stride, nullptr, agent_env_base);
    const GaussHead h{r.log_std_off, actions, actions_flat, clip_low, clip_high};
    return launch_head_act(ppo_act_gauss_graph_kernel<true>, ppo_act_gauss_graph_kernel<false>, full, g, P, N,
                           workspace, stream, h, who);
}

// ---------------------------------------------------------------------------
// persistent rollout / evaluation
// ---------------------------------------------------------------------------
extern "C" int64_t agx_ppo_rollout_gauss_graph_max_workgroups(void) {
    return head_rollout_max_workgroups<GaussRolloutHead>();
}

extern "C" int agx_ppo_rollout_gauss_graph_persistent(const agx_ppo_graph *net, int64_t log_std_off, int64_t P,
                                                      int64_t N, const float *params, const agx_rollout_io *ios,
                                                      int64_t nsteps, uint32_t base, uint64_t seed,
                                                      uint64_t counter0, const float *clip_low,
                                                      const float *clip_high, void *args_host, agx_rollout_ctl *ctl,
                                                      double timeout_s, void *workspace, void *stream) {
    auto plan = [&](GArgs &full, GaussRolloutHead &h, const char *who) {
        return gauss_plan(net, log_std_off, clip_low, clip_high, full, h, who);
    };
    return head_rollout_persistent<GaussRolloutHead>(net, plan, P, N, params, ios, nsteps, base, seed, counter0,
                                                     args_host, ctl, timeout_s, workspace, stream,
                                                     "agx_ppo_rollout_gauss_graph_persistent");
}

extern "C" int agx_ppo_eval_gauss_graph_persistent(const agx_ppo_graph *net, int64_t log_std_off, int64_t P,
                                                   int64_t N, const float *params, const float *stage_obs,
                                                   float *actions_flat, const float *clip_low,
                                                   const float *clip_high, const int64_t *agent_env_base,
                                                   int64_t nsteps, uint32_t base, uint64_t seed, uint64_t counter0,
                                                   void *args_host, agx_rollout_ctl *ctl, double timeout_s,
                                                   void *workspace, void *stream) {
    auto plan = [&](GArgs &full, GaussRolloutHead &h, const char *who) {
        return gauss_plan(net, log_std_off, clip_low, clip_high, full, h, who);
    };
    return head_eval_persistent<GaussRolloutHead>(net, plan, P, N, params, stage_obs, actions_flat, agent_env_base,
                                                  nsteps, base, seed, counter0, args_host, ctl, timeout_s, workspace,
                                                  stream,
                                                  "agx_ppo_eval_gauss_graph_persistent");
}

extern "C" int agx_ppo_gauss_loss_fwd_bwd(const float *mean, const float *value, const float *log_std,
                                          const float *actions, const float *old_logp, const float *adv,
                                          const float *ret, const float *old_value, const int64_t *index,
                                          int64_t batch, int64_t num_minibatches, int64_t A, float clip_coef,
                                          float vf_coef, float ent_coef, float *g_mean, float *g_value,
                                          float *g_log_std, float *stats, void *stream) {
    AGX_REQUIRE(batch > 0 && num_minibatches >= 0, "agx_ppo_gauss_loss_fwd_bwd: bad batch %lld x %lld",
                (long long)batch, (long long)num_minibatches);
    AGX_REQUIRE(A >= 1 && A <= AGX_PPO_GRAPH_MAX_ACTIONS, "agx_ppo_gauss_loss_fwd_bwd: %lld action dimensions (1..%d)",
                (long long)A, AGX_PPO_GRAPH_MAX_ACTIONS);
    AGX_REQUIRE(mean && value && log_std && actions && old_logp && adv && ret && old_value && g_mean && g_value &&
                    g_log_std,
                "agx_ppo_gauss_loss_fwd_bwd: null pointer");
    if (num_minibatches == 0) return AGX_OK;
    const LossCoef k = loss_coef(batch, clip_coef, vf_coef, ent_coef);
    const int64_t blocks = ceil_div(num_minibatches, 4);
    AGX_REQUIRE(blocks < ((int64_t)1 << 31), "agx_ppo_gauss_loss_fwd_bwd: too many minibatches");
    ppo_gauss_loss_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(
        mean, value, log_std, actions, old_logp, adv, ret, old_value, index, batch, num_minibatches, (int)A, k, g_mean,
        g_value, g_log_std, stats);
    return check_launch("agx_ppo_gauss_loss_fwd_bwd");
}
