// Policy step, persistent rollout and evaluation of runtime-shape networks
// (include/agx_graph.h): graph_net.h's forward of the layer list, then the
// categorical step; the persistent kernels run rollout.h's host-paced step
// around it, as learner.hip's do for the compiled shapes.
#include "graph_net.h"
#include "rollout.h"

namespace agx {
namespace {

// The categorical step of rows [0, nrow) of agent p's row block n0 (logits at
// lgp [nrow][A], values at vp) — masked logits (illegal -> -1e8,
// distributions.py:16-28), Gumbel-max sample from the Philox stream of
// agx_ppo_act, log-prob, entropy, value; 16 lanes per row, actions a and a + 16
// per lane.  HOST_MASK: the mask is host staging (system-scope loads), copied to
// mask_copy when that is set.
struct GSample {
    int A, N, sample;
    int lda, ldv;  // row strides of the logits and the values
    unsigned long long seed, counter;
    const long long *env_base;
    const unsigned char *mask;
    long long mask_pstride;
    unsigned char *mask_copy;
    long long mask_copy_pstride;
    long long *act_out;
    float *logp_out, *value_out, *ent_out;
    long long out_pstride;
    long long *act_flat;
    long long env_off;  // >= 0: the block's agent's first env (else env_base[p], or p N)
};
// the step g over logits of A actions; host_mask: g's mask is host staging (graph_sample<true>)
__device__ __forceinline__ GSample sample_args(const ActArgs &g, int A, int lda, int ldv, bool host_mask,
                                               long long env_off = -1) {
    GSample s;
    s.A = A;
    s.N = g.N;
    s.sample = g.sample;
    s.lda = lda;
    s.ldv = ldv;
    s.seed = g.seed;
    s.counter = g.counter;
    s.env_base = g.env_base;
    s.mask = g.mask;
    s.mask_pstride = g.mask_pstride;
    s.mask_copy = host_mask ? g.mask_copy : nullptr;
    s.mask_copy_pstride = host_mask ? g.mask_copy_pstride : 0;
    s.act_out = g.act_out;
    s.logp_out = g.logp_out;
    s.value_out = g.value_out;
    s.ent_out = g.ent_out;
    s.out_pstride = g.out_pstride;
    s.act_flat = g.act_flat;
    s.env_off = env_off;
    return s;
}
// an evaluation step of the agent whose first env is env_off: sampled actions to act_flat only
__device__ __forceinline__ GSample eval_sample_args(int A, int N, int lda, int ldv, unsigned long long seed,
                                                    unsigned long long counter, long long *act_flat,
                                                    long long env_off) {
    ActArgs g{};
    g.N = N;
    g.sample = 1;
    g.seed = seed;
    g.counter = counter;
    g.act_flat = act_flat;
    return sample_args(g, A, lda, ldv, true, env_off);
}
template <bool HOST_MASK>
__device__ __forceinline__ void graph_sample(const GSample &g, const float *lgp, const float *vp, int p, int n0,
                                             int nrow) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane & 15, rq = lane >> 4;
    const int A = g.A;
    const int a0 = sub, a1 = sub + 16;
    for (int r0 = 0; r0 < nrow; r0 += 4 * kGW) {
        const int r = r0 + 4 * wave + rq;
        const bool live = r < nrow;
        const int rr = live ? r : 0;
        float lg0 = a0 < A ? lgp[(size_t)rr * g.lda + a0] : -3.0e38f;
        float lg1 = a1 < A ? lgp[(size_t)rr * g.lda + a1] : -3.0e38f;
        if (g.mask && live) {
            const size_t mo = (size_t)p * g.mask_pstride + (size_t)(n0 + r) * A;
            unsigned char ok0 = 1, ok1 = 1;
            if (a0 < A) ok0 = HOST_MASK ? ld_sys_u8(g.mask + mo + a0) : g.mask[mo + a0];
            if (a1 < A) ok1 = HOST_MASK ? ld_sys_u8(g.mask + mo + a1) : g.mask[mo + a1];
            if (HOST_MASK && g.mask_copy) {
                const size_t co = (size_t)p * g.mask_copy_pstride + (size_t)(n0 + r) * A;
                if (a0 < A) g.mask_copy[co + a0] = ok0;
                if (a1 < A) g.mask_copy[co + a1] = ok1;
            }
            if (a0 < A && !ok0) lg0 = -1.0e8f;
            if (a1 < A && !ok1) lg1 = -1.0e8f;
        }
        const float mx = row_max(fmaxf(lg0, lg1));
        const float lse = mx + logf(row_sum((a0 < A ? expf(lg0 - mx) : 0.f) + (a1 < A ? expf(lg1 - mx) : 0.f)));
        const float p0 = a0 < A ? expf(lg0 - lse) : 0.f, p1 = a1 < A ? expf(lg1 - lse) : 0.f;
        const float H = -row_sum((a0 < A ? p0 * logf(p0 + 1e-8f) : 0.f) + (a1 < A ? p1 * logf(p1 + 1e-8f) : 0.f));
        float sc0 = lg0, sc1 = lg1;
        if (g.sample) {
            const unsigned long long env = stream_env(g.env_off, g.env_base, p, g.N, n0 + rr);
            auto gumbel = [&](int a, float lg) {
                return a < A ? gumbel_score(lg, a, env, g.seed, g.counter) : -3.0e38f;
            };
            sc0 = gumbel(a0, lg0);
            sc1 = A > 16 ? gumbel(a1, lg1) : -3.0e38f;
        }
        // first maximum over the actions: lane-local (a0 < a1), then the lowest
        // index among the lanes holding the row maximum
        const float bl = fmaxf(sc0, sc1);
        const int il = sc0 >= sc1 ? a0 : a1;
        const float best = row_max(bl);
        const int choice = (int)(-row_max(bl == best ? -(float)il : -1.0e9f));
        const int srcl = (lane & ~15) + (choice & 15);
        const float c0 = bperm(srcl, lg0), c1 = bperm(srcl, lg1);
        if (live && sub == 0) {
            const size_t o = (size_t)p * g.out_pstride + n0 + r;
            if (g.act_out) g.act_out[o] = choice;
            if (g.logp_out) g.logp_out[o] = (choice < 16 ? c0 : c1) - lse;
            if (g.ent_out) g.ent_out[o] = H;
            if (g.value_out) g.value_out[o] = vp[(size_t)r * g.ldv];
            if (g.act_flat)  // host staging: system-scope (write-through) store
                __hip_atomic_store(g.act_flat + (size_t)p * g.N + n0 + r, (long long)choice, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Rollout policy step (PPO.get_action, ppo.py:567-633) of workgroup (p, row
// block): forward through the layer list, then graph_sample.
// FEW: the block's 16 rows through few_forward's LDS tiles (act_plan_few).
template <bool FEW>
__global__ __launch_bounds__(kGT) void ppo_act_graph_kernel(const GActArgs ga, const ActArgs g) {
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
        graph_sample<false>(sample_args(g, ga.A, La.ld, Lc.ld, false), gdyn + La.yr, gdyn + Lc.yr, p, n0, nrow);
    } else {
        float *base = ga.ws + ((size_t)p * gridDim.x + blockIdx.x) * ga.ws_block;
        forward_layers(ga.L, ga.nl, obs, nrow, base, pr, ga.rows, lds);
        graph_sample<false>(sample_args(g, ga.A, ga.A, 1, false), base + La.yr, base + Lc.yr, p, n0, nrow);
    }
}

// Persistent rollout of a runtime-shape population (agx_ppo_rollout_graph_
// persistent / agx_ppo_eval_graph_persistent): agx_ppo_rollout_persistent's
// host-paced loop (learner.hip) around ppo_act_graph_kernel's step.  Step t:
// wait for the host's release, then the step's ActArgs (host memory): the
// observation rows from the host staging (system-scope loads) into this
// block's scratch and the rollout slot, the previous step's reward / done into
// slot t-1 with the episode accounting, and (act) the forward + sample; the
// actions go to the host staging; then this block's done word.
template <bool FEW>
__global__ __launch_bounds__(kGT) void ppo_rollout_graph_persistent_kernel(const GActArgs ga, const ActArgs *steps,
                                                                           int nsteps, agx_rollout_ctl *ctl,
                                                                           unsigned long long timeout_ticks,
                                                                           unsigned base_seq) {
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
                const auto prs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pr), 0,
                                                                   __builtin_amdgcn_readfirstlane(ga.n * 4), 0x00020000);
                few_forward(ga.L, ga.nl, gdyn, pr, prs, ga.oc, ga.ld0, nullptr);
                graph_sample<true>(sample_args(g, ga.A, La.ld, Lc.ld, true), gdyn + La.yr, gdyn + Lc.yr, p, n0, nrow);
            } else {
                forward_layers(ga.L, ga.nl, obs_rows, nrow, base, pr, ga.rows, lds);
                graph_sample<true>(sample_args(g, ga.A, ga.A, 1, true), base + La.yr, base + Lc.yr, p, n0, nrow);
            }
        }
        step_stores_acked();
        publish_done(ctl, blk, base_seq, t);
    }
}

// One evaluation pass of a WHOLE population in one persistent launch
// (agx_ppo_eval_multi_persistent): agent p runs ITS network (its own few-row
// policy-step plan, agents[p]) on its own parameter row over envs
// [p N, (p + 1) N) of the packed host staging, whatever group it trains in;
// the host paces the steps as for ppo_rollout_graph_persistent_kernel.  Step t
// samples with counter agents[p].counter0 + t from the agent's own Philox
// stream (seed, env base).
struct EvalAgent {
    GLay L[kGL];
    int nl, aout, cout, n, ld0;
    long long oc, lds_floats;
    unsigned run;       // the layers on the actor's path (the critic's are not computed)
    int ldw[kGL];       // LDS-resident weights (the WLDS kernel): row stride of layer l's W,
    long long wl[kGL];  // its offset in floats (W, then the bias), -1: layer not run
    long long lds_w;    // floats of LDS with the weights
    const float *params;
    long long env_base;
    unsigned long long seed, counter0;
};

// The episode tally of an evaluation pass on the device (agx_eval_tally):
// at each step the previous env step's reward / done from the host staging
// into the env's running score (f64, as the reference's numpy tally), its
// first finished episode's score, and each workgroup's count of finished envs
// for the host's end-of-pass test.
struct EvalTally {
    const float *rew;
    const unsigned char *done;
    double *scores, *completed;
    unsigned char *finished;
    unsigned *fin_words;
    int prev;  // the staging holds a reward / done when the launch starts
};

constexpr int kEvalStamps = 6 + kGL;  // agx_debug_eval_stamps: per step

template <bool WLDS>
__global__ __launch_bounds__(kGT) void ppo_eval_multi_persistent_kernel(const EvalAgent *__restrict__ agents, int N,
                                                                        int A, int D, const float *stage_obs,
                                                                        long long *act_flat, int nsteps,
                                                                        agx_rollout_ctl *ctl,
                                                                        unsigned long long timeout_ticks,
                                                                        unsigned base_seq, long long *stamps,
                                                                        const EvalTally tally) {
    extern __shared__ __attribute__((aligned(16))) float gdyn[];
    __shared__ int s_go;
    const int tid = threadIdx.x;
    const int p = blockIdx.y, n0 = blockIdx.x * kFR;
    const int blk = blockIdx.y * gridDim.x + blockIdx.x;
    const int nrow = N - n0 < kFR ? N - n0 : kFR;
    const EvalAgent &ag = agents[p];
    unsigned *rel = rollout_release_word(ctl, gridDim.x * gridDim.y, blk);
    const float *pr = ag.params;
    const auto prs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(pr), 0,
                                                       __builtin_amdgcn_readfirstlane(ag.n * 4), 0x00020000);
    for (int i = tid; i < (int)ag.lds_floats; i += kGT) gdyn[i] = 0.f;  // padding and rows past the block
    if constexpr (WLDS) {  // the actor path's weights, once for the whole pass (zero padded)
        __syncthreads();   // the zeroing above before the LN affine copies below
        for (int l = 0; l < ag.nl; ++l) {
            if (!((ag.run >> l) & 1u)) continue;
            const GLay &L = ag.L[l];
            const int K = L.fin, F = L.fout, ldw = ag.ldw[l], Fp = (F + 15) & ~15;
            float *W = gdyn + ag.wl[l];
            for (int i = tid; i < Fp * ldw; i += kGT) {
                const int n = i / ldw, k = i - n * ldw;
                W[i] = (n < F && k < K) ? pr[L.w + n * K + k] : 0.f;
            }
            for (int i = tid; i < Fp; i += kGT) W[Fp * ldw + i] = i < F ? pr[L.b + i] : 0.f;
            if (L.ln == 2)  // the LN affine's LDS copy too (few_forward<true> does not reload it)
                for (int i = tid; i < F; i += kGT) {
                    gdyn[L.af + i] = pr[L.g + i];
                    gdyn[L.af + F + i] = pr[L.be + i];
                }
        }
    }
    const GLay &La = ag.L[ag.aout], &Lc = ag.L[ag.cout];
    for (int t = 0; t < nsteps; ++t) {
        if (tid == 0) s_go = wait_release(rel, ctl, base_seq, t, timeout_ticks);
        __syncthreads();
        if (!s_go) return;
        const bool stamp = stamps && blk == 0 && tid == 0 && t >= 2 && t < 34;
        long long *stp = stamp ? stamps + kEvalStamps * (t - 2) : nullptr;
        if (stamp) stp[0] = (long long)__builtin_amdgcn_s_memrealtime();
        const float *ob = stage_obs + ((size_t)p * N + n0) * D;
        for (int i = tid; i < nrow * D; i += kGT) {
            const int b = i / D, d = i - b * D;
            gdyn[ag.oc + b * ag.ld0 + d] = ld_sys(ob + i);
        }
        if (tally.rew && (t > 0 || tally.prev) && tid < 64) {  // one wave: the block's <= 16 envs
            int fin = 0;
            if (tid < nrow) {
                const size_t idx = (size_t)p * N + n0 + tid;
                const float rw = ld_sys(tally.rew + idx);
                const unsigned char dn = ld_sys_u8(tally.done + idx);
                const double sc = tally.scores[idx] + (double)rw;
                tally.scores[idx] = sc;
                fin = tally.finished[idx];
                if (dn && !fin) {
                    tally.finished[idx] = 1;
                    tally.completed[idx] = sc;
                    fin = 1;
                }
            }
            const unsigned cnt = (unsigned)__builtin_popcountll(__builtin_amdgcn_ballot_w64(fin != 0));
            if (tid == 0) __hip_atomic_store(tally.fin_words + blk, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __syncthreads();
        if (stamp) {
            stp[1] = (long long)__builtin_amdgcn_s_memrealtime();
            stp[4] = (long long)__builtin_readcyclecounter();
        }
        few_forward<WLDS>(ag.L, ag.nl, gdyn, pr, prs, ag.oc, ag.ld0, stp ? stp + 5 : nullptr, ag.run, ag.wl, ag.ldw);
        if (stamp) stp[2] = (long long)__builtin_amdgcn_s_memrealtime();
        graph_sample<true>(eval_sample_args(A, N, La.ld, Lc.ld, ag.seed, ag.counter0 + (unsigned long long)t, act_flat,
                                            ag.env_base),
                           gdyn + La.yr, gdyn + Lc.yr, p, n0, nrow);
        step_stores_acked();
        publish_done(ctl, blk, base_seq, t);
        if (stamp) stp[3] = (long long)__builtin_amdgcn_s_memrealtime();
    }
}

}  // namespace
}  // namespace agx

using namespace agx;

extern "C" size_t agx_ppo_act_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t N) {
    GArgs full{};
    GActArgs a{};
    if (P <= 0 || N <= 0 || plan_graph(net, 1, full) != AGX_OK) return 0;
    return (size_t)P * ceil_div(N, kActRows) * act_plan(full, a) * sizeof(float);
}

extern "C" int agx_ppo_act_graph(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params,
                                 const float *obs, int64_t obs_agent_stride, const uint8_t *action_mask,
                                 int64_t mask_agent_stride, int sample, uint64_t seed, uint64_t counter,
                                 int64_t *actions, float *log_probs, float *values, float *entropy,
                                 int64_t out_agent_stride, int64_t *actions_flat, const int64_t *agent_env_base,
                                 void *workspace, void *stream) {
    AGX_REQUIRE(net && params && obs && workspace && P > 0 && N > 0 && P <= 65535, "agx_ppo_act_graph: bad arguments");
    GArgs full{};
    const int rc = plan_graph(net, 1, full);
    if (rc != AGX_OK) return rc;
    GActArgs a{};
    act_plan(full, a);
    a.ws = static_cast<float *>(workspace);
    const ActArgs g = act_step_args(P, N, params, obs, obs_agent_stride, action_mask, mask_agent_stride, sample, seed,
                                    counter, actions, log_probs, values, entropy, out_agent_stride, actions_flat,
                                    agent_env_base);
    dim3 grid((unsigned)ceil_div(N, kActRows), (unsigned)P);
    if (const size_t dyn = act_plan_few(ppo_act_graph_kernel<true>, a))
        ppo_act_graph_kernel<true><<<grid, kGT, dyn, as_stream(stream)>>>(a, g);
    else
        ppo_act_graph_kernel<false><<<grid, kGT, 0, as_stream(stream)>>>(a, g);
    return check_launch("agx_ppo_act_graph");
}

// ---------------------------------------------------------------------------
// persistent rollout / evaluation of runtime-shape populations
// ---------------------------------------------------------------------------
extern "C" int64_t agx_ppo_rollout_graph_workgroups(int64_t P, int64_t N) { return P * ceil_div(N, kActRows); }

extern "C" int64_t agx_ppo_rollout_graph_max_workgroups(void) {
    static int occ = -1;
    if (occ < 0) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, ppo_rollout_graph_persistent_kernel<false>, kGT, 0) !=
            hipSuccess)
            v = 0;
        occ = v;
    }
    return (int64_t)occ * cu_count();
}

extern "C" size_t agx_ppo_rollout_graph_ctl_bytes(int64_t P, int64_t N) {
    const unsigned nwg = (unsigned)agx_ppo_rollout_graph_workgroups(P, N);
    return (size_t)rollout_release_offset(nwg, nwg) * sizeof(unsigned);
}

namespace {
int launch_graph_persistent(const agx_ppo_graph *net, int64_t P, int64_t N, ActArgs *steps, int64_t nsteps,
                            uint32_t base, agx_rollout_ctl *ctl, double timeout_s, void *workspace, void *stream,
                            const char *who) {
    GArgs full{};
    const int rc = plan_graph(net, 1, full);
    if (rc != AGX_OK) return rc;
    const int64_t nwg = agx_ppo_rollout_graph_workgroups(P, N);
    if (nwg > agx_ppo_rollout_graph_max_workgroups()) {
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
    size_t dyn = act_plan_few(ppo_rollout_graph_persistent_kernel<true>, a);
    if (dyn) {
        int v = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, ppo_rollout_graph_persistent_kernel<true>, kGT, dyn) !=
                hipSuccess ||
            (int64_t)v * cu_count() < nwg)
            dyn = 0;
    }
    if (dyn)
        ppo_rollout_graph_persistent_kernel<true><<<grid, kGT, dyn, as_stream(stream)>>>(a, steps, (int)nsteps, ctl,
                                                                                         ticks, base);
    else
        ppo_rollout_graph_persistent_kernel<false><<<grid, kGT, 0, as_stream(stream)>>>(a, steps, (int)nsteps, ctl,
                                                                                         ticks, base);
    return check_launch(who);
}
}  // namespace

extern "C" int agx_ppo_rollout_graph_persistent(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params,
                                                const agx_rollout_io *ios, int64_t nsteps, uint32_t base,
                                                uint64_t seed, uint64_t counter0, void *args_host,
                                                agx_rollout_ctl *ctl, double timeout_s, void *workspace,
                                                void *stream) {
    if (int rc = check_persistent(net && ios && params && args_host && ctl && workspace, P, N, nsteps, base, timeout_s,
                                  "agx_ppo_rollout_graph_persistent"))
        return rc;
    AGX_REQUIRE(net->obs_dim >= 1, "agx_ppo_rollout_graph_persistent: bad graph");
    ActArgs *steps = static_cast<ActArgs *>(args_host);
    for (int64_t t = 0; t < nsteps; ++t) {
        const bool last = t + 1 == nsteps;
        if (int rc = check_rollout_io(ios + t, 1, params, "agx_ppo_rollout_graph_persistent")) return rc;
        fill_rollout_args(steps[t], net->obs_dim, net->n_actions, P, N, params, ios + t, 1, last ? 0 : 1, seed,
                          last ? 0 : counter0 + 1 + (uint64_t)t);
    }
    return launch_graph_persistent(net, P, N, steps, nsteps, base, ctl, timeout_s, workspace, stream,
                                   "agx_ppo_rollout_graph_persistent");
}

extern "C" int agx_ppo_eval_graph_persistent(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params,
                                             const float *stage_obs, const uint8_t *stage_mask,
                                             int64_t *actions_flat, const int64_t *agent_env_base, int64_t nsteps,
                                             uint32_t base, uint64_t seed, uint64_t counter0, void *args_host,
                                             agx_rollout_ctl *ctl, double timeout_s, void *workspace, void *stream) {
    if (int rc = check_persistent(net && params && stage_obs && actions_flat && args_host && ctl && workspace, P, N,
                                  nsteps, base, timeout_s, "agx_ppo_eval_graph_persistent"))
        return rc;
    ActArgs *steps = static_cast<ActArgs *>(args_host);
    for (int64_t t = 0; t < nsteps; ++t)
        steps[t] = eval_step_args(net->obs_dim, net->n_actions, P, N, params, stage_obs, stage_mask, actions_flat,
                                  agent_env_base, seed, counter0 + (uint64_t)t);
    return launch_graph_persistent(net, P, N, steps, nsteps, base, ctl, timeout_s, workspace, stream,
                                   "agx_ppo_eval_graph_persistent");
}

// ---------------------------------------------------------------------------
// evaluation of a whole population, every agent on its own network
// ---------------------------------------------------------------------------
static long long *&g_eval_stamps() {
    static long long *p = nullptr;
    return p;
}
// diagnostic: block 0's stamps of steps 2..33 of agx_ppo_eval_multi_persistent,
// kEvalStamps per step: release seen, observations staged, forward done, done
// word written (s_memrealtime, 100 MHz), then the shader clock at the forward's
// start and after each layer (0: not run); int64[32 * kEvalStamps], or null
// to stop
extern "C" int agx_debug_eval_stamps(int64_t *buf) {
    g_eval_stamps() = reinterpret_cast<long long *>(buf);
    return AGX_OK;
}

extern "C" size_t agx_ppo_eval_multi_bytes(int64_t P) { return P > 0 ? (size_t)P * sizeof(EvalAgent) : 0; }

namespace {
// agent p's policy-step plan (act_plan + act_plan_few) into x; -> its dynamic
// LDS bytes (0: the plan does not fit).  Only the layers on the actor's path
// run; wlds: their weights get LDS tiles after the activation tiles.
size_t eval_agent_plan(const agx_ppo_graph *net, EvalAgent &x, bool wlds) {
    GArgs full{};
    if (plan_graph(net, 1, full) != AGX_OK) return 0;
    GActArgs a{};
    act_plan(full, a);
    const size_t dyn = wlds ? act_plan_few(ppo_eval_multi_persistent_kernel<true>, a)
                            : act_plan_few(ppo_eval_multi_persistent_kernel<false>, a);
    if (!dyn) return 0;
    for (int l = 0; l < kGL; ++l) x.L[l] = a.L[l];
    x.nl = a.nl;
    x.aout = a.aout;
    x.cout = a.cout;
    x.n = a.n;
    x.ld0 = a.ld0;
    x.oc = a.oc;
    x.lds_floats = a.lds_floats;
    x.run = 0;
    for (int l = a.aout; l >= 0; l = a.L[l].src) x.run |= 1u << l;
    long long off = a.lds_floats;
    for (int l = 0; l < kGL; ++l) {
        x.wl[l] = -1;
        x.ldw[l] = 0;
        if (!wlds || l >= a.nl || !((x.run >> l) & 1u)) continue;
        const long long fp = (a.L[l].fout + 15) / 16 * 16;
        x.ldw[l] = (a.L[l].fin + 15) / 16 * 16 + 4;
        x.wl[l] = off;
        off += fp * x.ldw[l] + fp;
    }
    x.lds_w = (off + 3) & ~3ll;
    if (!wlds) return dyn;
    hipFuncAttributes fa{};
    const size_t st = hipFuncGetAttributes(&fa, (const void *)ppo_eval_multi_persistent_kernel<true>) == hipSuccess
                          ? fa.sharedSizeBytes
                          : 8 * 1024;
    const size_t bytes = (size_t)x.lds_w * 4;
    return bytes <= kLdsMax - st ? bytes : 0;
}

// the population's form: 1 LDS-resident weights, 0 weights from L2, -1 none
// (every workgroup co-resident either way); dyn: the launch's LDS bytes
int eval_form(const agx_ppo_graph *const *nets, int64_t P, int64_t N, size_t *dyn_out) {
    if (!nets || P <= 0 || N <= 0 || P > 65535) return -1;
    if (const char *e = getenv("AGX_GRAPH_FEW"))
        if (atoi(e) == 0) return -1;
    bool wl_ok = true;
    if (const char *e = getenv("AGX_EVAL_WLDS"))
        if (atoi(e) == 0) wl_ok = false;
    for (int w = wl_ok ? 1 : 0; w >= 0; --w) {
        size_t dyn = 0;
        bool ok = true;
        for (int64_t p = 0; p < P && ok; ++p) {
            EvalAgent x{};
            if (!nets[p] || nets[p]->obs_dim != nets[0]->obs_dim || nets[p]->n_actions != nets[0]->n_actions)
                return -1;
            const size_t d = eval_agent_plan(nets[p], x, w == 1);
            ok = d != 0;
            dyn = d > dyn ? d : dyn;
        }
        if (!ok) continue;
        int v = 0;
        const hipError_t e = w ? hipOccupancyMaxActiveBlocksPerMultiprocessor(
                                     &v, ppo_eval_multi_persistent_kernel<true>, kGT, dyn)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(
                                     &v, ppo_eval_multi_persistent_kernel<false>, kGT, dyn);
        if (e != hipSuccess || (int64_t)v * cu_count() < P * ceil_div(N, kFR)) continue;
        if (dyn_out) *dyn_out = dyn;
        return w;
    }
    return -1;
}
}  // namespace

extern "C" int agx_ppo_eval_multi_supported(const agx_ppo_graph *const *nets, int64_t P, int64_t N) {
    return eval_form(nets, P, N, nullptr) >= 0 ? 1 : 0;
}

extern "C" int agx_ppo_eval_multi_persistent(const agx_ppo_graph *const *nets, const float *const *params,
                                             const int64_t *env_base, const uint64_t *seeds,
                                             const uint64_t *counters, int64_t P, int64_t N, const float *stage_obs,
                                             int64_t *actions_flat, int64_t nsteps, uint32_t base, void *agents_host,
                                             void *agents_dev, agx_rollout_ctl *ctl, double timeout_s,
                                             const agx_eval_tally *tally, void *stream) {
    if (int rc = check_persistent(nets && params && env_base && seeds && counters && stage_obs && actions_flat &&
                                      agents_host && agents_dev && ctl,
                                  P, N, nsteps, base, timeout_s, "agx_ppo_eval_multi_persistent"))
        return rc;
    size_t dyn = 0;
    const int form = eval_form(nets, P, N, &dyn);
    AGX_REQUIRE(form >= 0, "agx_ppo_eval_multi_persistent: unsupported population");
    EvalAgent *ag = static_cast<EvalAgent *>(agents_host);
    for (int64_t p = 0; p < P; ++p) {
        AGX_REQUIRE(params[p], "agx_ppo_eval_multi_persistent: agent %lld has no parameters", (long long)p);
        EvalAgent x{};
        eval_agent_plan(nets[p], x, form == 1);
        x.params = params[p];
        x.env_base = env_base[p];
        x.seed = seeds[p];
        x.counter0 = counters[p];
        ag[p] = x;
    }
    hipStream_t s = as_stream(stream);
    if (hipMemcpyAsync(agents_dev, agents_host, (size_t)P * sizeof(EvalAgent), hipMemcpyHostToDevice, s) !=
        hipSuccess) {
        set_error("agx_ppo_eval_multi_persistent: agent table copy failed");
        return AGX_EHIP;
    }
    const int64_t nwg = P * ceil_div(N, kFR);
    const unsigned long long ticks = seconds_to_ticks(timeout_s);
    ctl->nwg = (uint32_t)nwg;
    dim3 grid((unsigned)ceil_div(N, kFR), (unsigned)P);
    EvalTally et{};
    if (tally) {
        AGX_REQUIRE(tally->stage_rew && tally->stage_done && tally->scores && tally->completed && tally->finished &&
                        tally->fin_words,
                    "agx_ppo_eval_multi_persistent: incomplete tally");
        et = EvalTally{tally->stage_rew, tally->stage_done, tally->scores, tally->completed, tally->finished,
                       tally->fin_words, tally->prev ? 1 : 0};
    }
    auto *kern = form == 1 ? ppo_eval_multi_persistent_kernel<true> : ppo_eval_multi_persistent_kernel<false>;
    kern<<<grid, kGT, dyn, s>>>(static_cast<const EvalAgent *>(agents_dev), (int)N, nets[0]->n_actions,
                                nets[0]->obs_dim, stage_obs, reinterpret_cast<long long *>(actions_flat), (int)nsteps,
                                ctl, ticks, base, g_eval_stamps(), et);
    return check_launch("agx_ppo_eval_multi_persistent");
}
