// What the Gaussian, multi-categorical and Bernoulli PPO heads share over a
// runtime layer list: the persistent rollout / evaluation launch (rollout.h's
// host-paced loop, ppo_rollout_graph_persistent_kernel's of graph_rollout.hip,
// written once over the head's step) and the host side that plans and launches
// it and the heads' per-step kernels.  Each head's .hip includes this header
// and instantiates the persistent kernel with its own Head:
//
//   struct Head {  // passed by value to the kernel
//       // the head's step of rows [0, nrow) of agent p's row block n0 over the
//       // step's ActArgs g (g.act_out / g.act_flat are the step's action slot and
//       // host staging, in the head's own element type); pr: the agent's
//       // parameter row
//       __device__ void step(const ActArgs &g, int A, int lda, int ldv, const float *lgp, const float *vp,
//                            const float *pr, int p, int n0, int nrow) const;
//   };
//
// The per-step kernels (ppo_act_{gauss,multi,bern}_graph_kernel) stay in the
// heads' files, each with its own argument struct: written as one template over
// this Head, with the actions routed through ActArgs, the Gaussian and the
// Bernoulli launch measured 1.6 % and 0.5 % slower (profiles/head_policy_ab.md).
// Only their host launcher is shared (launch_head_act).
//
// The persistent steps carry no legal-action mask (ActArgs.mask is null): the
// head steps read a mask with plain loads, which a host staging rewritten
// inside one launch does not allow.
#pragma once

#include "graph_net.h"
#include "rollout.h"

namespace agx {
namespace {

// Persistent rollout / evaluation (agx_ppo_rollout_*_graph_persistent,
// agx_ppo_eval_*_graph_persistent): agx_ppo_rollout_persistent's host-paced loop
// (learner.hip) around the head's step.  Step t: wait for the
// host's release, then the step's ActArgs (host memory): the observation rows
// from the host staging (system-scope loads) into this block's scratch / LDS
// tile and the rollout slot, the previous step's reward / done into slot t-1
// with the episode accounting, and (act) the forward + the head's step, whose
// actions go to the host staging with system-scope stores; then this block's
// done word.
template <bool FEW, class Head>
__global__ __launch_bounds__(kGT) void ppo_rollout_head_persistent_kernel(const GActArgs ga, const ActArgs *steps,
                                                                          int nsteps, agx_rollout_ctl *ctl,
                                                                          unsigned long long timeout_ticks,
                                                                          unsigned base_seq, const Head h) {
    __shared__ __attribute__((aligned(16))) float lds[kGemmLds];
    extern __shared__ __attribute__((aligned(16))) float gdyn[];
    __shared__ ActArgs s_args;
    __shared__ int s_go;
    const int tid = threadIdx.x;
    const int p = blockIdx.y, n0 = blockIdx.x * ga.rows;
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    const int D = ga.D;
    unsigned *rel = rollout_release_word(ctl, gridDim.x * gridDim.y, blk);
    float *base = ga.ws + ((size_t)p * gridDim.x + blockIdx.x) * ga.ws_block;
    float *obs_rows = base + ga.obs_off;  // [rows][D]: this step's observations
    constexpr int kArgWords = (int)(sizeof(ActArgs) / 4);
    static_assert(kArgWords <= kGT, "one thread per word of the step's arguments");
    if (tid == 0)  // this workgroup is resident (agx_rollout_ctl.started counts them)
        __hip_atomic_fetch_add(&ctl->started, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if constexpr (FEW) {  // the LDS tiles' padding (and the rows past the block) stay zero
        for (int i = tid; i < (int)ga.lds_floats; i += kGT) gdyn[i] = 0.f;
    }
    for (int t = 0; t < nsteps; ++t) {
        if (tid < kArgWords)
            reinterpret_cast<unsigned *>(&s_args)[tid] = reinterpret_cast<const unsigned *>(steps + t)[tid];
        if (tid == 0) s_go = wait_release(rel, ctl, base_seq, t, timeout_ticks);
        __syncthreads();
        if (!s_go) return;
        const ActArgs g = s_args;
        const int nrow = g.N - n0 < ga.rows ? g.N - n0 : ga.rows;
        // the host staging of this block's rows (one round trip), then the
        // previous step's reward / done and the episode accounting
        const float *ob = g.obs + (size_t)p * g.obs_pstride + (size_t)n0 * D;
        for (int i = tid; i < nrow * D; i += kGT) {
            const float x = ld_sys(ob + i);
            if constexpr (FEW) {
                const int b = i / D, d = i - b * D;
                gdyn[ga.oc + b * ga.ld0 + d] = x;
            } else {
                obs_rows[i] = x;
            }
            if (g.obs_copy) g.obs_copy[(size_t)p * g.obs_copy_pstride + (size_t)n0 * D + i] = x;
        }
        if (g.st_rew && tid < nrow) {
            const size_t idx = (size_t)p * g.N + n0 + tid;
            store_prev_step(g, p, n0 + tid, idx, load_prev_step(g, idx, true));
        }
        if (g.act) {
            __syncthreads();  // the observation rows are in the scratch
            const float *pr = g.params + (size_t)p * ga.n;
            const GLay &La = ga.L[ga.aout], &Lc = ga.L[ga.cout];
            if constexpr (FEW) {
                const auto prs = __builtin_amdgcn_make_buffer_rsrc(
                    const_cast<float *>(pr), 0, __builtin_amdgcn_readfirstlane(ga.n * 4), 0x00020000);
                few_forward(ga.L, ga.nl, gdyn, pr, prs, ga.oc, ga.ld0, nullptr);
                h.step(g, ga.A, La.ld, Lc.ld, gdyn + La.yr, gdyn + Lc.yr, pr, p, n0, nrow);
            } else {
                forward_layers(ga.L, ga.nl, obs_rows, nrow, base, pr, ga.rows, lds);
                h.step(g, ga.A, ga.A, 1, base + La.yr, base + Lc.yr, pr, p, n0, nrow);
            }
        }
        step_stores_acked();
        publish_done(ctl, blk, base_seq, t);
    }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// scratch of a per-step or persistent launch over the planned layer list `full`
inline size_t head_act_workspace_bytes(const GArgs &full, int64_t P, int64_t N) {
    GActArgs a{};
    return (size_t)P * ceil_div(N, kActRows) * act_plan(full, a) * sizeof(float);
}

// one per-step launch over `full` of a head's kernel pair (few: its few-row form, taken when its tiles
// fit) with the head's argument struct h
template <class Kernel, class Args>
int launch_head_act(Kernel few, Kernel general, const GArgs &full, const ActArgs &g, int64_t P, int64_t N,
                    void *workspace, void *stream, const Args &h, const char *who) {
    GActArgs a{};
    act_plan(full, a);
    a.ws = static_cast<float *>(workspace);
    dim3 grid((unsigned)ceil_div(N, kActRows), (unsigned)P);
    if (const size_t dyn = act_plan_few(few, a))
        few<<<grid, kGT, dyn, as_stream(stream)>>>(a, g, h);
    else
        general<<<grid, kGT, 0, as_stream(stream)>>>(a, g, h);
    return check_launch(who);
}

// co-resident workgroups of Head's persistent kernel (its general form, no dynamic LDS)
template <class Head>
int64_t head_rollout_max_workgroups() {
    static int occ = -1;
    if (occ < 0) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, ppo_rollout_head_persistent_kernel<false, Head>, kGT,
                                                         0) != hipSuccess)
            v = 0;
        occ = v;
    }
    return (int64_t)occ * cu_count();
}

// one persistent launch of Head's kernel over `full`, every workgroup resident
template <class Head>
int launch_head_persistent(const GArgs &full, int64_t P, int64_t N, const ActArgs *steps, int64_t nsteps,
                           uint32_t base, agx_rollout_ctl *ctl, double timeout_s, void *workspace, void *stream,
                           const Head &h, const char *who) {
    const int64_t nwg = P * ceil_div(N, kActRows);
    if (nwg > head_rollout_max_workgroups<Head>()) {
        set_error("%s: %lld workgroups cannot all be resident; use per-step launches", who, (long long)nwg);
        return AGX_EUNSUPPORTED;
    }
    GActArgs a{};
    act_plan(full, a);
    a.ws = static_cast<float *>(workspace);
    const unsigned long long ticks = seconds_to_ticks(timeout_s);
    ctl->nwg = (uint32_t)nwg;
    dim3 grid((unsigned)ceil_div(N, kActRows), (unsigned)P);
    // the few-row form when its tiles fit and the grid stays co-resident with them
    size_t dyn = act_plan_few(ppo_rollout_head_persistent_kernel<true, Head>, a);
    if (dyn) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, ppo_rollout_head_persistent_kernel<true, Head>, kGT,
                                                         dyn) != hipSuccess ||
            (int64_t)v * cu_count() < nwg)
            dyn = 0;
    }
    if (dyn) {
        ppo_rollout_head_persistent_kernel<true, Head><<<grid, kGT, dyn, as_stream(stream)>>>(a, steps, (int)nsteps,
                                                                                              ctl, ticks, base, h);
    } else {
        act_plan(full, a);  // act_plan_few may have laid the outputs out as LDS tiles
        ppo_rollout_head_persistent_kernel<false, Head><<<grid, kGT, 0, as_stream(stream)>>>(a, steps, (int)nsteps,
                                                                                             ctl, ticks, base, h);
    }
    return check_launch(who);
}

// The rollout entry of a head (agx_ppo_rollout_{gauss,multi,bern}_graph_persistent).
// plan(full, h, who): the head's checks of the net
// and the head -> the planned layer list and the kernel's Head.  Step t samples
// with counter0 + 1 + t, the step after the last runs unsampled at counter 0
// and writes values only.
template <class Head, class Plan>
int head_rollout_persistent(const agx_ppo_graph *net, Plan plan, int64_t P, int64_t N, const float *params,
                            const agx_rollout_io *ios, int64_t nsteps, uint32_t base, uint64_t seed,
                            uint64_t counter0, void *args_host, agx_rollout_ctl *ctl, double timeout_s,
                            void *workspace, void *stream, const char *who) {
    if (int rc = check_persistent(net && ios && params && args_host && ctl && workspace, P, N, nsteps, base, timeout_s,
                                  who))
        return rc;
    GArgs full{};
    Head h{};
    if (int rc = plan(full, h, who)) return rc;
    ActArgs *steps = static_cast<ActArgs *>(args_host);
    for (int64_t t = 0; t < nsteps; ++t) {
        const bool last = t + 1 == nsteps;
        if (int rc = check_rollout_io(ios + t, 1, params, who)) return rc;
        AGX_REQUIRE(!ios[t].stage_mask && !ios[t].mask_slot, "%s: step %lld stages a legal-action mask", who,
                    (long long)t);
        fill_rollout_args(steps[t], net->obs_dim, net->n_actions, P, N, params, ios + t, 1, last ? 0 : 1, seed,
                          last ? 0 : counter0 + 1 + (uint64_t)t);
    }
    return launch_head_persistent(full, P, N, steps, nsteps, base, ctl, timeout_s, workspace, stream, h, who);
}

// The evaluation entry of a head: sampled actions to the staging only, counters counter0 + t
template <class Head, class Plan>
int head_eval_persistent(const agx_ppo_graph *net, Plan plan, int64_t P, int64_t N, const float *params,
                         const float *stage_obs, void *actions_flat, const int64_t *agent_env_base, int64_t nsteps,
                         uint32_t base, uint64_t seed, uint64_t counter0, void *args_host, agx_rollout_ctl *ctl,
                         double timeout_s, void *workspace, void *stream, const char *who) {
    if (int rc = check_persistent(net && params && stage_obs && actions_flat && args_host && ctl && workspace, P, N,
                                  nsteps, base, timeout_s, who))
        return rc;
    GArgs full{};
    Head h{};
    if (int rc = plan(full, h, who)) return rc;
    ActArgs *steps = static_cast<ActArgs *>(args_host);
    for (int64_t t = 0; t < nsteps; ++t)
        steps[t] = eval_step_args(net->obs_dim, net->n_actions, P, N, params, stage_obs, nullptr,
                                  static_cast<int64_t *>(actions_flat), agent_env_base, seed, counter0 + (uint64_t)t);
    return launch_head_persistent(full, P, N, steps, nsteps, base, ctl, timeout_s, workspace, stream, h, who);
}

}  // namespace
}  // namespace agx
