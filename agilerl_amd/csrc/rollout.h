// The rollout policy step shared by the compiled (learner.hip) and the
// runtime-shape (graph_rollout.hip) kernels: the per-step argument block the
// persistent launches read from host memory, the Philox4x32-10 stream and
// the Gumbel-max score of the sample, the host-staging loads, the host-paced
// step of a persistent launch (wait for the release word, the previous
// step's reward / done, the done word), and the host side that fills and
// checks the argument blocks.
#pragma once

#include "agx_common.h"

namespace agx {

__device__ __forceinline__ unsigned mulhilo(unsigned a, unsigned b, unsigned &hi) {
    const unsigned long long prod = (unsigned long long)a * b;
    hi = (unsigned)(prod >> 32);
    return (unsigned)prod;
}
// Philox4x32-10 (Salmon et al., SC'11)
__device__ __forceinline__ uint4 philox(uint4 c, uint2 k) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        unsigned h0, h1;
        const unsigned l0 = mulhilo(0xD2511F53u, c.x, h0);
        const unsigned l1 = mulhilo(0xCD9E8D57u, c.z, h1);
        c = make_uint4(h1 ^ c.y ^ k.x, l1, h0 ^ c.w ^ k.y, l0);
        k.x += 0x9E3779B9u;
        k.y += 0xBB67AE85u;
    }
    return c;
}

struct ActArgs {
    const float *params;
    const float *obs;  // agent p, env n at obs + p*obs_pstride + n*D
    long long obs_pstride;
    int N, P, sample;
    unsigned long long seed, counter;
    long long *act_out;  // agent p, env n at + p*out_pstride + n (each may be null)
    float *logp_out, *value_out, *ent_out;
    long long out_pstride;
    long long *act_flat;  // [P*N] contiguous copy (host staging) or null
    int act;              // 0: scatter only (the step after the last action)
    // rollout bookkeeping fused into the policy step (agx_ppo_rollout_step)
    float *obs_copy;      // obs also written here (rollout slot t), agent stride obs_copy_pstride
    long long obs_copy_pstride;
    const float *st_rew;  // [P*N] reward / done of the previous vector step, or null
    const unsigned char *st_done;
    float *rew_prev;      // rollout slot t-1, agent stride prev_pstride
    unsigned char *done_prev;
    long long prev_pstride;
    float *scores;        // [P*N] running episode score (on_policy.py:147-172), or null
    double *ret_sum;      // [P*N] sum of finished-episode returns
    long long *episodes;  // [P*N] finished-episode count
    // legal-action masks (1 = legal): agent p, env n at mask + p*mask_pstride + n*A, or null;
    // copied to mask_copy (rollout slot t, agent stride mask_copy_pstride) when set
    const unsigned char *mask;
    long long mask_pstride;
    unsigned char *mask_copy;
    long long mask_copy_pstride;
    const long long *env_base;  // [P] global index of each agent's env 0 (Philox stream), or null: p * N
};

// The env staging may be host memory that the host rewrites between the
// steps of one persistent launch: read it with system-scope loads, which
// bypass the vector L1 and the L2 (both may hold the previous step's lines).
__device__ __forceinline__ float ld_sys(const float *p) {
    return __hip_atomic_load(const_cast<float *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ unsigned char ld_sys_u8(const unsigned char *p) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const unsigned w = __hip_atomic_load(reinterpret_cast<unsigned *>(a & ~(uintptr_t)3), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_SYSTEM);
    return (unsigned char)(w >> (8 * (a & 3)));
}

// ---------------------------------------------------------------------------
// The host-paced step of a persistent launch.  The host publishes sequence
// number base + t + 1 in each workgroup's release word once step t's staging
// is written; the workgroup runs the step and publishes the same number in
// its done word (agx_rollout_ctl, agx.h).
// ---------------------------------------------------------------------------
// Thread 0's wait for the release of step t -> go.  No-go: AGX_ROLLOUT_ABORT
// (ctl->timeout = 2), AGX_ROLLOUT_STOP (a clean early end), or timeout_ticks
// of s_memrealtime (100 MHz) without a release (ctl->timeout = 1).
__device__ __forceinline__ bool wait_release(const unsigned *rel, agx_rollout_ctl *ctl, unsigned base, int t,
                                             unsigned long long timeout_ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    for (;;) {
        // relaxed: an acquire at system scope would invalidate the
        // caches on every poll; one invalidate follows the wait
        const unsigned v = __hip_atomic_load(const_cast<unsigned *>(rel), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (v == AGX_ROLLOUT_ABORT) {  // host exception: the rollout is partial
            __hip_atomic_store(&ctl->timeout, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
        if (v == AGX_ROLLOUT_STOP) return false;  // an evaluation whose episodes all finished
        if (v >= base + (unsigned)(t + 1)) return true;
        if (__builtin_amdgcn_s_memrealtime() - t0 > timeout_ticks) {
            __hip_atomic_store(&ctl->timeout, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
        __builtin_amdgcn_s_sleep(2);
    }
}

// End of step t, every thread: the step's host-memory stores (actions) are
// system-scope write-through, so wait for their acknowledgements (no L2
// write-back: a release fence would flush every dirty L2 line per wave) ...
__device__ __forceinline__ void step_stores_acked() {
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
}
// ... then thread 0 publishes this block's done word.
__device__ __forceinline__ void publish_done(agx_rollout_ctl *ctl, int blk, unsigned base, int t) {
    if (threadIdx.x == 0)
        __hip_atomic_store(rollout_done_words(ctl) + blk, base + (unsigned)(t + 1), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// Reward / done of the previous vector step, env idx = p N + n of the host
// staging: the load half (on: this thread has an env and the step a staging) ...
struct PrevStep {
    float rw;
    unsigned char dn;
};
__device__ __forceinline__ PrevStep load_prev_step(const ActArgs &g, size_t idx, bool on) {
    PrevStep s{0.f, 0};
    if (on) {
        s.rw = ld_sys(g.st_rew + idx);
        s.dn = ld_sys_u8(g.st_done + idx);
    }
    return s;
}
// ... and the store half: rollout slot t-1 and the episode accounting.
__device__ __forceinline__ void store_prev_step(const ActArgs &g, int p, int env, size_t idx, PrevStep s) {
    g.rew_prev[(size_t)p * g.prev_pstride + env] = s.rw;
    g.done_prev[(size_t)p * g.prev_pstride + env] = s.dn;
    if (g.scores) {
        float sc = g.scores[idx] + s.rw;
        if (s.dn) {
            g.ret_sum[idx] += (double)sc;
            g.episodes[idx] += 1;
            sc = 0.f;
        }
        g.scores[idx] = sc;
    }
}

// The env index that keys the Philox stream of row `row` of agent p: the
// agent's first env (env_off when >= 0, else env_base[p], else p N) + row.
__device__ __forceinline__ unsigned long long stream_env(long long env_off, const long long *env_base, int p, int N,
                                                         int row) {
    return (env_off >= 0 ? (unsigned long long)env_off
            : env_base   ? (unsigned long long)env_base[p]
                         : (unsigned long long)p * N) +
           row;
}
// Gumbel-max score of action a with logit lg: word a & 3 of the Philox block
// of (env, counter ^ (a >> 2) << 56) -> u in (0, 1) -> lg - log(-log u).
// The callers call it under their own `a < A ? .. : -3e38`: hoisted out of that
// test it costs ppo_rollout_persistent_kernel a wave of occupancy.
// gumbel_noise is the part that does not depend on the logit, log(-log u): a
// persistent step computes it while it waits for the host's release.
__device__ __forceinline__ float gumbel_noise(int a, unsigned long long env, unsigned long long seed,
                                              unsigned long long counter) {
    const uint4 rnd = philox(make_uint4((unsigned)env, (unsigned)(env >> 32), (unsigned)counter,
                                        (unsigned)(counter >> 32) ^ ((unsigned)(a >> 2) << 24)),
                             make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const unsigned w = (a & 3) == 0 ? rnd.x : (a & 3) == 1 ? rnd.y : (a & 3) == 2 ? rnd.z : rnd.w;
    const float u = ((float)(w >> 8) + 0.5f) * (1.0f / 16777216.0f);
    return logf(-logf(u));
}
__device__ __forceinline__ float gumbel_score(float lg, int a, unsigned long long env, unsigned long long seed,
                                              unsigned long long counter) {
    return lg - gumbel_noise(a, env, seed, counter);
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// a per-step launch with no rollout bookkeeping (agx_ppo_act, agx_ppo_act_graph)
inline ActArgs act_step_args(int64_t P, int64_t N, const float *params, const float *obs, int64_t obs_agent_stride,
                             const uint8_t *action_mask, int64_t mask_agent_stride, int sample, uint64_t seed,
                             uint64_t counter, int64_t *actions, float *log_probs, float *values, float *entropy,
                             int64_t out_agent_stride, int64_t *actions_flat, const int64_t *agent_env_base) {
    ActArgs a{};
    a.params = params;
    a.obs = obs;
    a.obs_pstride = obs_agent_stride;
    a.N = (int)N;
    a.P = (int)P;
    a.sample = sample;
    a.seed = seed;
    a.counter = counter;
    a.act_out = reinterpret_cast<long long *>(actions);
    a.logp_out = log_probs;
    a.value_out = values;
    a.ent_out = entropy;
    a.out_pstride = out_agent_stride;
    a.act_flat = reinterpret_cast<long long *>(actions_flat);
    a.act = 1;
    a.mask = action_mask;
    a.mask_pstride = mask_agent_stride;
    a.env_base = reinterpret_cast<const long long *>(agent_env_base);
    return a;
}

// a step of an evaluation pass: sampled actions to the host staging only
inline ActArgs eval_step_args(int D, int A, int64_t P, int64_t N, const float *params, const float *stage_obs,
                              const uint8_t *stage_mask, int64_t *actions_flat, const int64_t *agent_env_base,
                              uint64_t seed, uint64_t counter) {
    return act_step_args(P, N, params, stage_obs, N * (int64_t)D, stage_mask, N * (int64_t)A, 1, seed, counter,
                         nullptr, nullptr, nullptr, nullptr, 0, actions_flat, agent_env_base);
}

// the arguments every persistent launch checks (pointers_ok: the caller's own pointers)
inline int check_persistent(bool pointers_ok, int64_t P, int64_t N, int64_t nsteps, uint32_t base, double timeout_s,
                            const char *who) {
    AGX_REQUIRE(pointers_ok && P > 0 && N > 0 && P <= 65535 && nsteps >= 1, "%s: bad arguments", who);
    AGX_REQUIRE((uint64_t)base + (uint64_t)nsteps < AGX_ROLLOUT_STOP, "%s: base wraps", who);
    AGX_REQUIRE(timeout_s > 0 && timeout_s < 3600, "%s: timeout_s out of range", who);
    return AGX_OK;
}

inline unsigned long long seconds_to_ticks(double s) {  // s_memrealtime: 100 MHz
    return (unsigned long long)(s * 1e8);
}

inline void fill_rollout_args(ActArgs &a, int D, int A, int64_t P, int64_t N, const float *params,
                              const agx_rollout_io *io, int act, int sample, uint64_t seed, uint64_t counter) {
    a.params = params;
    a.obs = io->stage_obs;
    a.obs_pstride = N * (int64_t)D;
    a.N = (int)N;
    a.P = (int)P;
    a.sample = sample;
    a.seed = seed;
    a.counter = counter;
    a.act_out = reinterpret_cast<long long *>(io->actions);
    a.logp_out = io->log_probs;
    a.value_out = io->values;
    a.ent_out = nullptr;
    a.out_pstride = io->slot_agent_stride;
    a.act_flat = reinterpret_cast<long long *>(io->actions_flat);
    a.act = act;
    a.obs_copy = io->obs_slot;
    a.obs_copy_pstride = io->obs_agent_stride;
    a.st_rew = io->stage_rew;
    a.st_done = io->stage_done;
    a.rew_prev = io->rewards_prev;
    a.done_prev = io->dones_prev;
    a.prev_pstride = io->prev_agent_stride;
    a.scores = io->scores;
    a.ret_sum = io->return_sum;
    a.episodes = reinterpret_cast<long long *>(io->episodes);
    a.mask = io->stage_mask;
    a.mask_pstride = N * (int64_t)A;
    a.mask_copy = io->mask_slot;
    a.mask_copy_pstride = io->mask_agent_stride;
    a.env_base = reinterpret_cast<const long long *>(io->agent_env_base);
}

inline int check_rollout_io(const agx_rollout_io *io, int act, const float *params, const char *who) {
    AGX_REQUIRE(io && io->stage_obs, "%s: null io / stage_obs", who);
    AGX_REQUIRE(!act || params, "%s: act needs params", who);
    AGX_REQUIRE(!io->stage_rew || (io->stage_done && io->rewards_prev && io->dones_prev),
                "%s: previous-step scatter needs rewards/dones slots", who);
    AGX_REQUIRE(!io->scores || (io->stage_rew && io->return_sum && io->episodes),
                "%s: episode accounting needs return_sum, episodes and stage rewards", who);
    return AGX_OK;
}


}  // namespace agx
