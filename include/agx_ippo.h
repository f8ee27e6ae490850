/* IPPO (independent PPO for multi-agent environments): the generalised
 * advantage estimate of the reference's experience-tuple learner
 * (agilerl/algorithms/ippo.py:688-725) for every agent group of one learn call
 * in one launch.
 *
 * The reference runs it as float32 torch ops on the CPU: T serial steps of
 * about eight small ops each, with float `dones` and the critic's bootstrap
 * value.  agx_gae (agx.h) is the RolloutBuffer form (numpy's f64 carry, u8
 * dones) and does not give the same bits, so this is a kernel of its own.
 * The other half of IPPO's hot path, the advantages normalised per minibatch
 * (ippo.py:780-783), is agx_ppo_learn_args.adv_norm_minibatch (agx.h).
 * All tensors are f32 on the device, caller-owned; nothing synchronises.
 * Binding: INTEGRATION.md. */
#ifndef AGX_IPPO_H
#define AGX_IPPO_H

#include "agx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_IPPO_MAX_SEGMENTS 8
/* One agent group: M = envs x agents of the group columns, T rows each. */
typedef struct agx_ippo_gae_segment {
    const float *rewards, *dones, *values; /* [T][M] */
    const float *next_value, *next_done;   /* [M]: the critic's value of next_state, the final done flags */
    float *advantages, *returns;           /* [T][M], written in full */
    int64_t M;                             /* 0: the segment is skipped (its pointers are not read) */
} agx_ippo_gae_segment;

/* Replaces agilerl/algorithms/ippo.py:702-725 for up to AGX_IPPO_MAX_SEGMENTS
 * groups (a host table, passed to the kernel by value; T is common to them).
 * Per column, t = T-1 .. 0, with g = (float)gamma and gl = (float)(gamma *
 * gae_lambda) (the double product rounded once), every operation a float32
 * one in exactly this order (no contraction):
 *   nnt     = 1 - d'                 d', v' = next_done, next_value at t = T-1, else dones[t+1], values[t+1]
 *   delta   = (r[t] + (g * v') * nnt) - v[t]
 *   adv[t]  = last = delta + (gl * nnt) * last          (last = 0 before t = T-1)
 *   ret[t]  = adv[t] + v[t]
 * which are the bits the reference's torch loop gives.  A NaN anywhere
 * propagates by IEEE rules down its own column, as there; nothing is special-
 * cased.  One lane per column, rows read coalesced along M.
 * AGX_EINVAL before any HIP call: segments NULL with n_segments > 0,
 * n_segments outside 0..AGX_IPPO_MAX_SEGMENTS, T <= 0, M < 0, or a null
 * pointer in a segment with M > 0. */
int agx_ippo_gae(const agx_ippo_gae_segment *segments, int n_segments, int64_t T, double gamma, double gae_lambda,
                 void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_IPPO_H */
