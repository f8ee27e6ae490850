// PPO for MultiDiscrete action spaces (include/agx_multi.h): the
// multi-categorical policy step over a runtime layer list (graph_net.h's
// forward, then one categorical step per component, as graph_rollout.hip's
// single one) and the multi-categorical twin of agx_ppo_loss_fwd_bwd (masked
// per-component log-softmax, log-prob of the stored action, entropy, the
// clipped loss of ppo_loss_sample.h and the gradients of logits / value in
// one pass).
//
// The segmented reductions.  A row's L <= 32 logits sit as in graph_sample:
// 16 lanes per row, flat indices sub and sub + 16 per lane, so a component
// [off, off + n) may lie in the lanes' first logits, in their second, or
// across index 16.  Both kernels walk the K components in ascending k (K is a
// kernel argument: a wave-uniform trip count) and run graph_sample's own
// row_max / row_sum DPP reductions with the lanes outside the component
// neutral (-3e38 for a maximum, 0 for a sum); the two in-segment tests cover
// all three placements.  This form was chosen over reading a component's
// logits back from LDS / the workspace per lane because (a) for K = 1 it is
// graph_sample's arithmetic, instruction for instruction, which the
// bit-equality with agx_ppo_act_graph rests on, (b) the reductions are DPP
// moves in registers, with no LDS traffic or barrier after the forward, and
// (c) the per-lane read-back has a lane-dependent trip count n_k.  It costs
// five row reductions per component; the Philox draws and the logit / mask
// loads stay outside the loop, once per lane.
#include "../../include/agx_multi.h"
#include "graph_net.h"
#include "head_policy.h"
#include "multi_head_check.h"
#include "ppo_loss_sample.h"
#include "rollout.h"

namespace agx {
namespace {

constexpr float kOut = -3.0e38f;  // a lane outside the component (or past L) in a maximum

// max-shifted log-sum-exp of the component whose logits are lg0 (in0) / lg1 (in1) of the row's lanes
__device__ __forceinline__ float seg_lse(bool in0, bool in1, float lg0, float lg1) {
    const float mx = row_max(fmaxf(in0 ? lg0 : kOut, in1 ? lg1 : kOut));
    return mx + logf(row_sum((in0 ? expf(lg0 - mx) : 0.f) + (in1 ? expf(lg1 - mx) : 0.f)));
}

// what the multi-categorical step writes besides the ActArgs' log_probs / values / entropy
struct MultiHead {
    agx_multi_head head;
    long long *act_out;   // agent p, env n, component k at ((p out_pstride + n) K + k)
    long long *act_flat;  // [P N K] host staging, or null
};

// The multi-categorical step of rows [0, nrow) of agent p's row block n0
// (logits at lgp [nrow][L] with row stride lda, values at vp with stride ldv).
// head: the kernel's own argument (its nvec[k] reads stay scalar loads of the
// argument block; a copy would be indexed in scratch)
__device__ __forceinline__ void multi_step(const ActArgs &g, const agx_multi_head &head, long long *act_out,
                                           long long *act_flat, int L, int lda, int ldv, const float *lgp,
                                           const float *vp, int p, int n0, int nrow) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int j0 = sub, j1 = sub + 16;
    const int K = head.K;
    for (int r0 = 0; r0 < nrow; r0 += 4 * kGW) {
        const int r = r0 + 4 * wave + rq;
        const bool live = r < nrow;
        const int rr = live ? r : 0;
        float lg0 = j0 < L ? lgp[(size_t)rr * lda + j0] : kOut;
        float lg1 = j1 < L ? lgp[(size_t)rr * lda + j1] : kOut;
        if (g.mask && live) {
            const size_t mo = (size_t)p * g.mask_pstride + (size_t)(n0 + r) * L;
            if (j0 < L && !g.mask[mo + j0]) lg0 = -1.0e8f;
            if (j1 < L && !g.mask[mo + j1]) lg1 = -1.0e8f;
        }
        float sc0 = lg0, sc1 = lg1;
        if (g.sample) {
            const unsigned long long env = stream_env(-1, g.env_base, p, g.N, n0 + rr);
            auto gumbel = [&](int j, float lg) { return j < L ? gumbel_score(lg, j, env, g.seed, g.counter) : kOut; };
            sc0 = gumbel(j0, lg0);
            sc1 = L > 16 ? gumbel(j1, lg1) : kOut;
        }
        float lp = 0.f, H = 0.f;
        int ch0 = 0, ch1 = 0, off = 0;
        for (int k = 0; k < K; ++k) {  // wave-uniform: K and nvec are kernel arguments
            const int n = head.nvec[k];
            const bool in0 = j0 >= off && j0 < off + n, in1 = j1 >= off && j1 < off + n;
            const float lse = seg_lse(in0, in1, lg0, lg1);
            const float p0 = in0 ? expf(lg0 - lse) : 0.f, p1 = in1 ? expf(lg1 - lse) : 0.f;
            const float Hk = -row_sum((in0 ? p0 * logf(p0 + 1e-8f) : 0.f) + (in1 ? p1 * logf(p1 + 1e-8f) : 0.f));
            // first maximum of the component: lane-local (j0 < j1), then the
            // lowest index among the lanes holding the component's maximum
            const float s0 = in0 ? sc0 : kOut, s1 = in1 ? sc1 : kOut;
            const float bl = fmaxf(s0, s1);
            const int il = s0 >= s1 ? j0 : j1;
            const float best = row_max(bl);
            const int choice = (int)(-row_max(bl == best ? -(float)il : -1.0e9f));
            const int srcl = (lane & ~15) + (choice & 15);
            const float c0 = bperm(srcl, lg0), c1 = bperm(srcl, lg1);
            const float lpk = (choice < 16 ? c0 : c1) - lse;
            lp = k == 0 ? lpk : lp + lpk;  // ascending k
            H = k == 0 ? Hk : H + Hk;
            if (sub == (k & 15)) {  // lane k & 15 keeps component k's choice: one coalesced store per row
                if (k < 16)
                    ch0 = choice - off;
                else
                    ch1 = choice - off;
            }
            off += n;
        }
        if (!live) continue;
        const size_t row = (size_t)p * g.out_pstride + n0 + r;
        if (act_out) {
            if (j0 < K) act_out[row * K + j0] = ch0;
            if (j1 < K) act_out[row * K + j1] = ch1;
        }
        if (act_flat) {  // host staging: system-scope (write-through) stores
            long long *f = act_flat + ((size_t)p * g.N + n0 + r) * K;
            if (j0 < K) __hip_atomic_store(f + j0, (long long)ch0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            if (j1 < K) __hip_atomic_store(f + j1, (long long)ch1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        if (sub == 0) {
            if (g.logp_out) g.logp_out[row] = lp;
            if (g.ent_out) g.ent_out[row] = H;
            if (g.value_out) g.value_out[row] = vp[(size_t)r * ldv];
        }
    }
}

// Policy step of workgroup (p, row block): forward through the layer list
// (ppo_act_graph_kernel's two forms), then multi_step.
template <bool FEW>
__global__ __launch_bounds__(kGT) void ppo_act_multi_graph_kernel(const GActArgs ga, const ActArgs g,
                                                                  const MultiHead h) {
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
        multi_step(g, h.head, h.act_out, h.act_flat, ga.A, La.ld, Lc.ld, gdyn + La.yr, gdyn + Lc.yr, p, n0, nrow);
    } else {
        float *base = ga.ws + ((size_t)p * gridDim.x + blockIdx.x) * ga.ws_block;
        forward_layers(ga.L, ga.nl, obs, nrow, base, pr, ga.rows, lds);
        multi_step(g, h.head, h.act_out, h.act_flat, ga.A, ga.A, 1, base + La.yr, base + Lc.yr, p, n0, nrow);
    }
}

// multi_step as the step of head_policy.h's persistent loop: the step's
// action slot / host staging are int64 [.., K]
struct MultiRolloutHead {
    agx_multi_head head;
    __device__ __forceinline__ void step(const ActArgs &g, int L, int lda, int ldv, const float *lgp, const float *vp,
                                         const float *, int p, int n0, int nrow) const {
        multi_step(g, head, g.act_out, g.act_flat, L, lda, ldv, lgp, vp, p, n0, nrow);
    }
};

// ---------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------
// One wave per minibatch m: 16 lanes per row (flat logits sub and sub + 16 per
// lane), four rows at a time.  The component loop leaves each lane with its own
// logits' p, dH/dlg and one-hot (a logit belongs to exactly one component) and
// every lane of the row with the row's log-prob and entropy, so every lane
// holds the row's loss terms; lane 0 of the row counts them.
__global__ __launch_bounds__(256) void ppo_multi_loss_kernel(
    const float *__restrict__ logits, const float *__restrict__ value, const agx_multi_head head, int L,
    const long long *__restrict__ actions, const unsigned char *__restrict__ mask,
    const float *__restrict__ old_logp, const float *__restrict__ adv, const float *__restrict__ ret,
    const float *__restrict__ old_v, const int64_t *__restrict__ index, int64_t b, int64_t nmb, LossCoef k,
    float *__restrict__ g_logits, float *__restrict__ g_value, float *__restrict__ stats) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= nmb) return;  // whole waves exit together
    const int sub = lane & 15, rq = lane >> 4;
    const int j0 = sub, j1 = sub + 16;
    const bool on0 = j0 < L, on1 = j1 < L;
    const int K = head.K;
    Acc acc;
    const int64_t base = m * b;
    for (int64_t i0 = 0; i0 < b; i0 += 4) {  // wave-uniform trip count (the row reductions need whole rows)
        const int64_t i = i0 + rq;
        const bool live = i < b;
        const int64_t o = base + (live ? i : 0);
        const int64_t src = index ? index[o] : o;
        float lg0 = on0 ? logits[o * L + j0] : kOut, lg1 = on1 ? logits[o * L + j1] : kOut;
        bool ok0 = true, ok1 = true;
        if (mask) {
            ok0 = !on0 || mask[src * L + j0];
            ok1 = !on1 || mask[src * L + j1];
            if (!ok0) lg0 = -1.0e8f;
            if (!ok1) lg1 = -1.0e8f;
        }
        float lp = 0.f, H = 0.f;
        float p0 = 0.f, p1 = 0.f, dh0 = 0.f, dh1 = 0.f, oh0 = 0.f, oh1 = 0.f;
        int off = 0;
        for (int c = 0; c < K; ++c) {  // wave-uniform: head is a kernel argument
            const int n = head.nvec[c];
            const bool in0 = j0 >= off && j0 < off + n, in1 = j1 >= off && j1 < off + n;
            long long a = actions[src * K + c];
            a = a < 0 ? 0 : (a >= n ? n - 1 : a);  // never index outside the component
            const int ja = off + (int)a;
            const float lse = seg_lse(in0, in1, lg0, lg1);
            const float q0 = in0 ? expf(lg0 - lse) : 0.f, q1 = in1 ? expf(lg1 - lse) : 0.f;
            const float l0 = logf(q0 + 1e-8f), l1 = logf(q1 + 1e-8f);
            const float Hc = -row_sum((in0 ? q0 * l0 : 0.f) + (in1 ? q1 * l1 : 0.f));
            const float t0 = l0 + q0 / (q0 + 1e-8f), t1 = l1 + q1 / (q1 + 1e-8f);
            const float pt = row_sum((in0 ? q0 * t0 : 0.f) + (in1 ? q1 * t1 : 0.f));
            // the chosen logit: exactly one lane term is non-zero, so the sum is exact
            const float lga = row_sum((in0 && j0 == ja ? lg0 : 0.f) + (in1 && j1 == ja ? lg1 : 0.f));
            const float lpc = lga - lse;
            lp = c == 0 ? lpc : lp + lpc;  // ascending c
            H = c == 0 ? Hc : H + Hc;
            if (in0) {
                p0 = q0;
                dh0 = -q0 * (t0 - pt);
                oh0 = j0 == ja ? 1.f : 0.f;
            }
            if (in1) {
                p1 = q1;
                dh1 = -q1 * (t1 - pt);
                oh1 = j1 == ja ? 1.f : 0.f;
            }
            off += n;
        }
        if (!live) continue;
        float gl, gv;
        Acc one;
        loss_sample(lp, old_logp[src], adv[src], ret[src], old_v[src], value[o], H, k, gl, gv, one);
        if (sub == 0) {
            acc.add(one);
            g_value[o] = gv;
        }
        // a masked logit passes nothing back (the reference's torch.where)
        if (on0) g_logits[o * L + j0] = ok0 ? gl * (oh0 - p0) + k.g_h * dh0 : 0.f;
        if (on1) g_logits[o * L + j1] = ok1 ? gl * (oh1 - p1) + k.g_h * dh1 : 0.f;
    }
    finish_group<64>(acc, k, m, lane, stats);
}

}  // namespace
}  // namespace agx

using namespace agx;

namespace {
// the rules of every multi-categorical entry point for the net and the head -> the plan and the
// persistent kernel's head
int multi_plan(const agx_ppo_graph *net, const agx_multi_head &head, GArgs &full, MultiRolloutHead &h,
               const char *who) {
    const int L = head_width(head, who);
    if (L < 0) return AGX_EINVAL;
    if (int rc = plan_graph(net, 1, full)) return rc;
    if (int rc = head_fits(net, L, who)) return rc;
    h.head = head_arg(head);
    return AGX_OK;
}
}  // namespace

extern "C" size_t agx_ppo_act_multi_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t N) {
    GArgs full{};
    if (!net || P <= 0 || N <= 0 || plan_graph(net, 1, full) != AGX_OK) return 0;
    return head_act_workspace_bytes(full, P, N);
}

extern "C" int agx_ppo_act_multi_graph(const agx_ppo_graph *net, agx_multi_head head, int64_t P, int64_t N,
                                       const float *params, const float *obs, int64_t obs_agent_stride,
                                       const uint8_t *action_mask, int64_t mask_agent_stride, int sample,
                                       uint64_t seed, uint64_t counter, int64_t *actions, float *log_probs,
                                       float *values, float *entropy, int64_t out_agent_stride,
                                       int64_t *actions_flat, const int64_t *agent_env_base, void *workspace,
                                       void *stream) {
    const char *who = "agx_ppo_act_multi_graph";
    AGX_REQUIRE(net && params && obs && workspace && P > 0 && N > 0 && P <= 65535, "%s: bad arguments", who);
    GArgs full{};
    MultiRolloutHead r{};
    if (int rc = multi_plan(net, head, full, r, who)) return rc;
    const ActArgs g = act_step_args(P, N, params, obs, obs_agent_stride, action_mask, mask_agent_stride, sample, seed,
                                    counter, nullptr, log_probs, values, entropy, out_agent_stride, nullptr,
                                    agent_env_base);
    const MultiHead h{r.head, reinterpret_cast<long long *>(actions), reinterpret_cast<long long *>(actions_flat)};
    return launch_head_act(ppo_act_multi_graph_kernel<true>, ppo_act_multi_graph_kernel<false>, full, g, P, N,
                           workspace, stream, h, who);
}

// ---------------------------------------------------------------------------
// persistent rollout / evaluation
// ---------------------------------------------------------------------------
extern "C" int64_t agx_ppo_rollout_multi_graph_max_workgroups(void) {
    return head_rollout_max_workgroups<MultiRolloutHead>();
}

extern "C" int agx_ppo_rollout_multi_graph_persistent(const agx_ppo_graph *net, agx_multi_head head, int64_t P,
                                                      int64_t N, const float *params, const agx_rollout_io *ios,
                                                      int64_t nsteps, uint32_t base, uint64_t seed,
                                                      uint64_t counter0, void *args_host, agx_rollout_ctl *ctl,
                                                      double timeout_s, void *workspace, void *stream) {
    auto plan = [&](GArgs &full, MultiRolloutHead &h, const char *who) { return multi_plan(net, head, full, h, who); };
    return head_rollout_persistent<MultiRolloutHead>(net, plan, P, N, params, ios, nsteps, base, seed, counter0,
                                                     args_host, ctl, timeout_s, workspace, stream,
                                                     "agx_ppo_rollout_multi_graph_persistent");
}

extern "C" int agx_ppo_eval_multi_graph_persistent(const agx_ppo_graph *net, agx_multi_head head, int64_t P,
                                                   int64_t N, const float *params, const float *stage_obs,
                                                   int64_t *actions_flat, const int64_t *agent_env_base,
                                                   int64_t nsteps, uint32_t base, uint64_t seed, uint64_t counter0,
                                                   void *args_host, agx_rollout_ctl *ctl, double timeout_s,
                                                   void *workspace, void *stream) {
    auto plan = [&](GArgs &full, MultiRolloutHead &h, const char *who) { return multi_plan(net, head, full, h, who); };
    return head_eval_persistent<MultiRolloutHead>(net, plan, P, N, params, stage_obs, actions_flat, agent_env_base,
                                                  nsteps, base, seed, counter0, args_host, ctl, timeout_s, workspace,
                                                  stream,
                                                  "agx_ppo_eval_multi_graph_persistent");
}

extern "C" int agx_ppo_multi_loss_fwd_bwd(const float *logits, const float *value, agx_multi_head head,
                                          const int64_t *actions, const uint8_t *mask, const float *old_logp,
                                          const float *adv, const float *ret, const float *old_value,
                                          const int64_t *index, int64_t batch, int64_t num_minibatches,
                                          float clip_coef, float vf_coef, float ent_coef, float *g_logits,
                                          float *g_value, float *stats, void *stream) {
    AGX_REQUIRE(batch > 0 && num_minibatches >= 0, "agx_ppo_multi_loss_fwd_bwd: bad batch %lld x %lld",
                (long long)batch, (long long)num_minibatches);
    const int L = head_width(head, "agx_ppo_multi_loss_fwd_bwd");
    if (L < 0) return AGX_EINVAL;
    AGX_REQUIRE(logits && value && actions && old_logp && adv && ret && old_value && g_logits && g_value,
                "agx_ppo_multi_loss_fwd_bwd: null pointer");
    if (num_minibatches == 0) return AGX_OK;
    const LossCoef k = loss_coef(batch, clip_coef, vf_coef, ent_coef);
    const int64_t blocks = ceil_div(num_minibatches, 4);
    AGX_REQUIRE(blocks < ((int64_t)1 << 31), "agx_ppo_multi_loss_fwd_bwd: too many minibatches");
    ppo_multi_loss_kernel<<<(unsigned)blocks, 256, 0, as_stream(stream)>>>(
        logits, value, head_arg(head), L, reinterpret_cast<const long long *>(actions), mask, old_logp, adv, ret,
        old_value, index, batch, num_minibatches, k, g_logits, g_value, stats);
    return check_launch("agx_ppo_multi_loss_fwd_bwd");
}
