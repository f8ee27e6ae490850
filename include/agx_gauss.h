/* PPO for Box action spaces: the diagonal-Gaussian policy step and loss.
 *
 * The actor's output layer gives the mean mu [A]; the A log_std floats are
 * parameters of the agent's flat row (the reference's EvolvableDistribution,
 * agilerl/networks/distributions.py:152-183, with action_std_init), owned by no
 * layer of the agx_ppo_graph: n_params counts them, the layers do not cover them.
 *
 *   log_prob(a) = sum_d -0.5 ((a_d - mu_d)^2 / exp(2 log_std_d) + 2 log_std_d + log 2 pi)
 *   entropy     = 0.5 (1 + log 2 pi) A + sum_d log_std_d
 * (agilerl/utils/torch_utils.py:202-257).
 *
 * Noise of the sampled step.  Dimension d of the row whose stream env is `env`
 * (agx_ppo_act: agent_env_base[p] + n, or p N + n) takes the Philox4x32-10 block
 *   counter words (env lo, env hi, counter lo, counter hi ^ ((d >> 1) << 24)),
 *   key words     (seed lo, seed hi)
 * — the block of agx_ppo_act's Gumbel draw with d >> 1 in place of a >> 2 — and
 * from it words (x, y) when d is even, (z, w) when d is odd:
 *   u1 = ((word0 >> 8) + 0.5) 2^-24,  u2 = ((word1 >> 8) + 0.5) 2^-24   (both in (0, 1))
 *   eps = sqrt(-2 ln u1) cos(2 pi u2)                                   (Box-Muller, cospi(2 u2))
 *   a_d = fl(mu_d + exp(log_std_d) eps)
 * The log-prob is computed from the stored (rounded) a_d, as the reference's
 * log_prob(sample()) is and as the learner recomputes it. */
#ifndef AGX_GAUSS_H
#define AGX_GAUSS_H

#include "agx_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The policy step of PPO.get_action (agilerl/algorithms/ppo.py:567-633) for a
 * runtime layer list whose actor output is the Gaussian mean (n_actions = A <=
 * AGX_PPO_GRAPH_MAX_ACTIONS); the A log_std floats sit at params + p n_params +
 * log_std_off.  One workgroup per (agent, 16-row block), forward as
 * agx_ppo_act_graph (same workspace size rule, same AGX_GRAPH_FEW switch).
 * sample 0: the action is the mean.  actions [P][..][A] with agent stride
 * out_agent_stride * A floats (row n of agent p at (p out_agent_stride + n) A);
 * log_probs / values / entropy with agent stride out_agent_stride; each may be
 * NULL.  actions_flat [P N A] (the env staging, system-scope stores) or NULL;
 * clip_low / clip_high [A] (device, both or neither): only the actions_flat
 * copy is clipped to them (ppo.py:604-614: the reference clips for the env at
 * inference only); the stored action and its log-prob are the unclipped
 * sample's. */
size_t agx_ppo_act_gauss_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t N);
int agx_ppo_act_gauss_graph(const agx_ppo_graph *net, int64_t log_std_off, int64_t P, int64_t N, const float *params,
                            const float *obs, int64_t obs_agent_stride, int sample, uint64_t seed, uint64_t counter,
                            float *actions, float *log_probs, float *values, float *entropy, int64_t out_agent_stride,
                            float *actions_flat, const float *clip_low, const float *clip_high,
                            const int64_t *agent_env_base, void *workspace, void *stream);

/* Persistent rollout / evaluation of a Box-action population: the host-paced
 * loops of agx_ppo_rollout_graph_persistent / agx_ppo_eval_graph_persistent
 * (agx_graph.h: same agx_rollout_io steps, control block protocol and bytes,
 * args bytes, workgroup count agx_ppo_rollout_graph_workgroups(P, N), Philox
 * counters counter0 + 1 + t / counter0 + t, AGX_ROLLOUT_ABORT / AGX_ROLLOUT_STOP)
 * around agx_ppo_act_gauss_graph's step, one launch per rollout (replaces
 * rollouts/on_policy.py:23-203's per-step forward).  A step's
 * agx_rollout_io.actions is the float slot [..][A] (row n of agent p at
 * (p slot_agent_stride + n) A) and actions_flat the float staging [P N A];
 * the staging copy is clipped to clip_low / clip_high [A] (device, both or
 * neither; on_policy.py:104-119 clips for the env), the slot holds the
 * unclipped sample.  The step after the last runs unsampled at counter 0 and
 * writes values only.  No step may stage a legal-action mask (AGX_EINVAL).
 * Every workgroup must be co-resident: AGX_EUNSUPPORTED beyond
 * agx_ppo_rollout_gauss_graph_max_workgroups() (this kernel's own occupancy).
 * The net and log_std_off are checked as agx_ppo_act_gauss_graph checks them;
 * `workspace` as there.  The evaluation writes the sampled, clipped actions
 * to actions_flat only. */
int64_t agx_ppo_rollout_gauss_graph_max_workgroups(void);
int agx_ppo_rollout_gauss_graph_persistent(const agx_ppo_graph *net, int64_t log_std_off, int64_t P, int64_t N,
                                           const float *params, const agx_rollout_io *ios, int64_t nsteps,
                                           uint32_t base, uint64_t seed, uint64_t counter0, const float *clip_low,
                                           const float *clip_high, void *args_host, agx_rollout_ctl *ctl,
                                           double timeout_s, void *workspace, void *stream);
int agx_ppo_eval_gauss_graph_persistent(const agx_ppo_graph *net, int64_t log_std_off, int64_t P, int64_t N,
                                        const float *params, const float *stage_obs, float *actions_flat,
                                        const float *clip_low, const float *clip_high, const int64_t *agent_env_base,
                                        int64_t nsteps, uint32_t base, uint64_t seed, uint64_t counter0,
                                        void *args_host, agx_rollout_ctl *ctl, double timeout_s, void *workspace,
                                        void *stream);

/* PPO.learn for a Gaussian head: agx_ppo_learn_graph (agx_graph.h) with the
 * actor output as the mean and the A log_std floats at log_std_off of every
 * agent's row.  log_std belongs to the actor clip group and to no layer: the
 * layers and [log_std_off, log_std_off + A) tile the row exactly, with
 * log_std_off + A <= critic_start.
 *
 * agx_ppo_gauss_graph_check: host-only (no HIP call).  AGX_OK when the learner
 * takes this net; AGX_EINVAL with the reason in agx_last_error otherwise (A
 * outside 1..AGX_PPO_GRAPH_MAX_ACTIONS, log_std_off not the gap the layers
 * leave, the gap outside [0, critic_start), anything agx_ppo_graph_check
 * rejects).
 *
 * agx_ppo_learn_gauss_graph takes agx_ppo_learn_graph's argument block with
 * args->actions float [P][S][A]; args->action_masks must be NULL (AGX_EINVAL).
 * Per-agent batch / epochs / ent_coef, target_kl, skip_if_set, loss_out /
 * kl_out / epochs_out, error_word and adam_step behave as there; so do the
 * forms the call picks between (AGX_GRAPH_FEW, AGX_GRAPH_ROWS,
 * AGX_GRAPH_SPLIT) and the fixed summation order: an agent's update does not
 * depend on which other agents share the launch.  The per-row math is that of
 * agx_ppo_gauss_loss_fwd_bwd below.  The workspace holds the gathered float
 * actions (4 A bytes per row and epoch). */
int agx_ppo_gauss_graph_check(const agx_ppo_graph *net, int64_t log_std_off);
size_t agx_ppo_learn_gauss_graph_workspace_bytes(const agx_ppo_graph *net, int64_t log_std_off, int64_t P, int64_t S,
                                                 int64_t epochs, int64_t batch);
int agx_ppo_learn_gauss_graph(const agx_ppo_graph *net, int64_t log_std_off, const agx_ppo_learn_args *args,
                              void *workspace, void *stream);

/* The Gaussian twin of agx_ppo_loss_fwd_bwd (agx.h; ppo.py:868-902): num_minibatches
 * minibatches of `batch` rows, minibatch m with its own log_std row.
 *   mean [nmb batch][A], value [nmb batch], log_std [nmb][A]     (network outputs / parameters)
 *   actions [rows][A], old_logp / adv / ret / old_value [rows]   (the rollout)
 *   index [nmb batch] int64 rollout row of each sample, or NULL (sample i is row i)
 * -> g_mean [nmb batch][A], g_value [nmb batch], g_log_std [nmb][A], stats [nmb][8]
 * (the layout of agx_ppo_loss_fwd_bwd: loss, pg, value, entropy loss, approx_kl,
 * clip fraction, 0, 0; may be NULL).  The gradients are those of the sum of the
 * minibatches' losses.  g_log_std sums over a minibatch's rows in a fixed order
 * (lane-strided, then in-wave butterflies): no atomics, equal bits every run. */
int agx_ppo_gauss_loss_fwd_bwd(const float *mean, const float *value, const float *log_std, const float *actions,
                               const float *old_logp, const float *adv, const float *ret, const float *old_value,
                               const int64_t *index, int64_t batch, int64_t num_minibatches, int64_t A, float clip_coef,
                               float vf_coef, float ent_coef, float *g_mean, float *g_value, float *g_log_std,
                               float *stats, void *stream);

#ifdef __cplusplus
}
#endif

#endif
