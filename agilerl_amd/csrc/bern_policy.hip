// PPO for MultiBinary action spaces (include/agx_bernoulli.h): the Bernoulli
// policy step over a runtime layer list (graph_net.h's forward, then one
// Bernoulli step per logit) and the Bernoulli twin of agx_ppo_loss_fwd_bwd
// (masked logits, log-prob of the stored bits, entropy, the clipped loss of
// ppo_loss_sample.h and the gradients of logits / value in one pass).
//
// A row's n <= 32 logits sit as in multi_policy.hip: 16 lanes per row, flat
// indices sub and sub + 16 per lane.  Every bit is its own distribution
// (bern_head.h), so there is no component loop: a lane works on its two
// logits alone, and a row takes two row_sum reductions (log-prob, entropy)
// whatever n is.  Lane j holds bit j, so the action stores are coalesced.
#include "../../include/agx_bernoulli.h"
#include "bern_head.h"
#include "graph_net.h"
#include "head_policy.h"
#include "ppo_loss_sample.h"
#include "rollout.h"

namespace agx {
namespace {

// the uniform of flat index j of stream env `env`: the u of gumbel_score
// (rollout.h), word j & 3 of the block of (env, counter ^ (j >> 2) << 56)
__device__ __forceinline__ float bern_uniform(int j, unsigned long long env, unsigned long long seed,
                                              unsigned long long counter) {
    const uint4 rnd = philox(make_uint4((unsigned)env, (unsigned)(env >> 32), (unsigned)counter,
                                        (unsigned)(counter >> 32) ^ ((unsigned)(j >> 2) << 24)),
                             make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const unsigned w = (j & 3) == 0 ? rnd.x : (j & 3) == 1 ? rnd.y : (j & 3) == 2 ? rnd.z : rnd.w;
    return ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f);
}

// what the Bernoulli step writes besides the ActArgs' log_probs / values / entropy
struct BernOut {
    long long *act_out;   // agent p, env r, bit j at ((p out_pstride + r) n + j)
    long long *act_flat;  // [P N n] host staging, or null
};

// The Bernoulli step of rows [0, nrow) of agent p's row block n0 (logits at
// lgp [nrow][n] with row stride lda, values at vp with stride ldv).
__device__ __forceinline__ void bern_step(const ActArgs &g, const BernOut &h, int n, int lda, int ldv,
                                          const float *lgp, const float *vp, int p, int n0, int nrow) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int j0 = sub, j1 = sub + 16;
    const bool on0 = j0 < n, on1 = j1 < n;
    for (int r0 = 0; r0 < nrow; r0 += 4 * kGW) {
        const int r = r0 + 4 * wave + rq;
        const bool live = r < nrow;
        const int rr = live ? r : 0;
        float lg0 = on0 ? lgp[(size_t)rr * lda + j0] : 0.f;
        float lg1 = on1 ? lgp[(size_t)rr * lda + j1] : 0.f;
        if (g.mask && live) {
            const size_t mo = (size_t)p * g.mask_pstride + (size_t)(n0 + r) * n;
            if (on0 && !g.mask[mo + j0]) lg0 = -1.0e8f;
            if (on1 && !g.mask[mo + j1]) lg1 = -1.0e8f;
        }
        const BernBit b0 = bern_bit(lg0), b1 = bern_bit(lg1);
        bool a0 = lg0 > 0.f, a1 = lg1 > 0.f;  // the mode; a logit of exactly 0 gives 0
        if (g.sample) {
            const unsigned long long env = stream_env(-1, g.env_base, p, g.N, n0 + rr);
            if (on0) a0 = bern_uniform(j0, env, g.seed, g.counter) < b0.p;
            if (on1) a1 = bern_uniform(j1, env, g.seed, g.counter) < b1.p;
        }
        const float lp = row_sum((on0 ? (a0 ? b0.lp : b0.lq) : 0.f) + (on1 ? (a1 ? b1.lp : b1.lq) : 0.f));
        const float H = -row_sum((on0 ? bern_neg_entropy(b0) : 0.f) + (on1 ? bern_neg_entropy(b1) : 0.f));
        if (!live) continue;
        const size_t row = (size_t)p * g.out_pstride + n0 + r;
        if (h.act_out) {
            if (on0) h.act_out[row * n + j0] = a0 ? 1 : 0;
            if (on1) h.act_out[row * n + j1] = a1 ? 1 : 0;
        }
        if (h.act_flat) {  // host staging: system-scope (write-through) stores
            long long *f = h.act_flat + ((size_t)p * g.N + n0 + r) * n;
            if (on0) __hip_atomic_store(f + j0, (long long)(a0 ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (on1) __hip_atomic_store(f + j1, (long long)(a1 ? 1 : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (sub == 0) {
            if (g.logp_out) g.logp_out[row] = lp;
            if (g.ent_out) g.ent_out[row] = H;
            if (g.value_out) g.value_out[row] = vp[(size_t)r * ldv];
        }
    }
}

// Policy step of workgroup (p, row block): forward through the layer list
// (ppo_act_graph_kernel's two forms), then bern_step.
template <bool FEW>
__global__ __launch_bounds__(kGT) void ppo_act_bern_graph_kernel(const GActArgs ga, const ActArgs g, const BernOut h) {
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
        bern_step(g, h, ga.A, La.ld, Lc.ld, gdyn + La.yr, gdyn + Lc.yr, p, n0, nrow);
    } else {
        float *base = ga.ws + ((size_t)p * gridDim.x + blockIdx.x) * ga.ws_block;
        forward_layers(ga.L, ga.nl, obs, nrow, base, pr, ga.rows, lds);
        bern_step(g, h, ga.A, ga.A, 1, base + La.yr, base + Lc.yr, p, n0, nrow);
    }
}

// bern_step as the step of head_policy.h's persistent loop: the step's action
// slot / host staging are int64 [.., n]
struct BernRolloutHead {
    __device__ __forceinline__ void step(const ActArgs &g, int n, int lda, int ldv, const float *lgp, const float *vp,
                                         const float *, int p, int n0, int nrow) const {
        const BernOut h{g.act_out, g.act_flat};
        bern_step(g, h, n, lda, ldv, lgp, vp, p, n0, nrow);
    }
};

// ---------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------
// One wave per minibatch m: 16 lanes per row (bits sub and sub + 16 per lane),
// four rows at a time.  The two row sums leave every lane of the row with the
// row's log-prob and entropy, so every lane holds the row's loss terms; lane 0
// of the row counts them.
__global__ __launch_bounds__(256) void ppo_bern_loss_kernel(
    const float *__restrict__ logits, const float *__restrict__ value, int n, const long long *__restrict__ actions,
    const unsigned char *__restrict__ mask, const float *__restrict__ old_logp, const float *__restrict__ adv,
    const float *__restrict__ ret, const float *__restrict__ old_v, const int64_t *__restrict__ index, int64_t b,
    int64_t nmb, LossCoef k, float *__restrict__ g_logits, float *__restrict__ g_value, float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= nmb) return;  // whole waves exit together
    const int sub = lane & 15, rq = lane >> 4;
    const int j0 = sub, j1 = sub + 16;
    const bool on0 = j0 < n, on1 = j1 < n;
    Acc acc;
    const int64_t base = m * b;
    for (int64_t i0 = 0; i0 < b; i0 += 4) {  // wave-uniform trip count (the row reductions need whole rows)
        const int64_t i = i0 + rq;
        const bool live = i < b;
        const int64_t o = base + (live ? i : 0);
        const int64_t src = index ? index[o] : o;
        float lg0 = on0 ? logits[o * n + j0] : 0.f, lg1 = on1 ? logits[o * n + j1] : 0.f;
        bool ok0 = true, ok1 = true;
        if (mask) {
            ok0 = !on0 || mask[src * n + j0];
            ok1 = !on1 || mask[src * n + j1];
            if (!ok0) lg0 = -1.0e8f;
            if (!ok1) lg1 = -1.0e8f;
        }
        const bool a0 = on0 && actions[src * n + j0] != 0, a1 = on1 && actions[src * n + j1] != 0;
        const BernBit b0 = bern_bit(lg0), b1 = bern_bit(lg1);
        const float lp = row_sum((on0 ? (a0 ? b0.lp : b0.lq) : 0.f) + (on1 ? (a1 ? b1.lp : b1.lq) : 0.f));
        const float H = -row_sum((on0 ? bern_neg_entropy(b0) : 0.f) + (on1 ? bern_neg_entropy(b1) : 0.f));
        if (!live) continue;
        float gl, gv;
        Acc one;
        loss_sample(lp, old_logp[src], adv[src], ret[src], old_v[src], value[o], H, k, gl, gv, one);
        if (sub == 0) {
            acc.add(one);
            g_value[o] = gv;
        }
        // a masked logit passes nothing back (the reference's torch.where)
        if (on0) g_logits[o * n + j0] = ok0 ? gl * bern_dlogp(b0, a0) + k.g_h * bern_dH(b0) : 0.f;
        if (on1) g_logits[o * n + j1] = ok1 ? gl * bern_dlogp(b1, a1) + k.g_h * bern_dH(b1) : 0.f;
    }
    finish_group<64>(acc, k, m, lane, stats);
}

}  // namespace
}  // namespace agx

using namespace agx;

namespace {
// the rules of every Bernoulli entry point for the net (the head has no parameters) -> the plan
int bern_plan(const agx_ppo_graph *net, GArgs &full, BernRolloutHead &, const char *) {
    return plan_graph(net, 1, full);
}
}  // namespace

extern "C" size_t agx_ppo_act_bern_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t N) {
    GArgs full{};
    if (!net || P <= 0 || N <= 0 || plan_graph(net, 1, full) != AGX_OK) return 0;
    return head_act_workspace_bytes(full, P, N);
}

extern "C" int agx_ppo_act_bern_graph(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params,
                                      const float *obs, int64_t obs_agent_stride, const uint8_t *action_mask,
                                      int64_t mask_agent_stride, int sample, uint64_t seed, uint64_t counter,
                                      int64_t *actions, float *log_probs, float *values, float *entropy,
                                      int64_t out_agent_stride, int64_t *actions_flat, const int64_t *agent_env_base,
                                      void *workspace, void *stream) {
    const char *who = "agx_ppo_act_bern_graph";
    AGX_REQUIRE(net && params && obs && workspace && P > 0 && N > 0 && P <= 65535, "%s: bad arguments", who);
    GArgs full{};
    BernRolloutHead r{};
    if (int rc = bern_plan(net, full, r, who)) return rc;
    const ActArgs g = act_step_args(P, N, params, obs, obs_agent_stride, action_mask, mask_agent_stride, sample, seed,
                                    counter, nullptr, log_probs, values, entropy, out_agent_stride, nullptr,
                                    agent_env_base);
    const BernOut h{reinterpret_cast<long long *>(actions), reinterpret_cast<long long *>(actions_flat)};
    return launch_head_act(ppo_act_bern_graph_kernel<true>, ppo_act_bern_graph_kernel<false>, full, g, P, N, workspace,
                           stream, h, who);
}

// ---------------------------------------------------------------------------
// persistent rollout / evaluation
// ---------------------------------------------------------------------------
extern "C" int64_t agx_ppo_rollout_bern_graph_max_workgroups(void) {
    return head_rollout_max_workgroups<BernRolloutHead>();
}

extern "C" int agx_ppo_rollout_bern_graph_persistent(const agx_ppo_graph *net, int64_t P, int64_t N,
                                                     const float *params, const agx_rollout_io *ios, int64_t nsteps,
                                                     uint32_t base, uint64_t seed, uint64_t counter0, void *args_host,
                                                     agx_rollout_ctl *ctl, double timeout_s, void *workspace,
                                                     void *stream) {
    auto plan = [&](GArgs &full, BernRolloutHead &h, const char *who) { return bern_plan(net, full, h, who); };
    return head_rollout_persistent<BernRolloutHead>(net, plan, P, N, params, ios, nsteps, base, seed, counter0,
                                                    args_host, ctl, timeout_s, workspace, stream,
                                                    "agx_ppo_rollout_bern_graph_persistent");
}

extern "C" int agx_ppo_eval_bern_graph_persistent(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params,
                                                  const float *stage_obs, int64_t *actions_flat,
                                                  const int64_t *agent_env_base, int64_t nsteps, uint32_t base,
                                                  uint64_t seed, uint64_t counter0, void *args_host,
                                                  agx_rollout_ctl *ctl, double timeout_s, void *workspace,
                                                  void *stream) {
    auto plan = [&](GArgs &full, BernRolloutHead &h, const char *who) { return bern_plan(net, full, h, who); };
    return head_eval_persistent<BernRolloutHead>(net, plan, P, N, params, stage_obs, actions_flat, agent_env_base,
                                                 nsteps, base, seed, counter0, args_host, ctl, timeout_s, workspace,
                                                 stream,
                                                 "agx_ppo_eval_bern_graph_persistent");
}

extern "C" int agx_ppo_bern_loss_fwd_bwd(const float *logits, const float *value, int32_t n, const int64_t *actions,
                                         const uint8_t *mask, const float *old_logp, const float *adv,
                                         const float *ret, const float *old_value, const int64_t *index,
                                         int64_t batch, int64_t num_minibatches, float clip_coef, float vf_coef,
                                         float ent_coef, float *g_logits, float *g_value, float *stats,
                                         void *stream) {
    AGX_REQUIRE(batch > 0 && num_minibatches >= 0, "agx_ppo_bern_loss_fwd_bwd: bad batch %lld x %lld",
                (long long)batch, (long long)num_minibatches);
    AGX_REQUIRE(n >= 1 && n <= AGX_PPO_GRAPH_MAX_ACTIONS, "agx_ppo_bern_loss_fwd_bwd: %d bits (1..%d)", n,
                AGX_PPO_GRAPH_MAX_ACTIONS);
    AGX_REQUIRE(logits && value && actions && old_logp && adv && ret && old_value && g_logits && g_value,
                "agx_ppo_bern_loss_fwd_bwd: null pointer");
    if (num_minibatches == 0) return AGX_OK;
    const LossCoef k = loss_coef(batch, clip_coef, vf_coef, ent_coef);
    const int64_t blocks = ceil_div(num_minibatches, 4);
    AGX_REQUIRE(blocks < ((int64_t)1 << 31), "agx_ppo_bern_loss_fwd_bwd: too many minibatches");
    ppo_bern_loss_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(
        logits, value, n, reinterpret_cast<const long long *>(actions), mask, old_logp, adv, ret, old_value, index,
        batch, num_minibatches, k, g_logits, g_value, stats);
    return check_launch("agx_ppo_bern_loss_fwd_bwd");
}
