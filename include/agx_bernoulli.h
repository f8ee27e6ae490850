/* PPO for MultiBinary action spaces: the Bernoulli policy step, loss and fused
 * learner.
 *
 * A MultiBinary(n) space has n independent switches: the actor's output layer
 * has width n = net->n_actions (no output activation) and logit j is the
 * log-odds of bit j (the reference's StochasticActor with
 * networks/distributions.py:201-207, 256-263 and utils/torch_utils.py:336-376).
 * Limits: 1 <= n <= AGX_PPO_GRAPH_MAX_ACTIONS.
 *
 * Per row, all in float32, with l_j the logit of bit j:
 *   mask      an optional flat mask [.., n] (uint8, 1 = legal) sets an illegal
 *             logit to -1e8 before anything else (apply_action_mask_discrete
 *             over the single split [n]): a masked bit has p = 0 and is never
 *             sampled as 1
 *   e_j       = exp(-|l_j|),  s_j = log1p(e_j)
 *   p_j       = sigmoid(l_j)  = l_j >= 0 ? 1 / (1 + e_j) : e_j / (1 + e_j)
 *   q_j       = 1 - p_j       = l_j >= 0 ? e_j / (1 + e_j) : 1 / (1 + e_j)
 *   log p_j   = min(l_j, 0) - s_j     (= -softplus(-l_j))
 *   log q_j   = min(-l_j, 0) - s_j    (= -l_j + log p_j)
 *   log_prob  = sum_j (a_j ? log p_j : log q_j)
 *   entropy   = -sum_j [p_j log(p_j + 1e-8) + q_j log(q_j + 1e-8)]
 * Every term is finite for |l_j| up to 1e8, and a masked bit with stored action
 * 0 contributes exactly 0 to both sums.  The sums over j are fixed-order
 * reductions: equal bits on every launch, whatever other agents share it.
 *
 * Sampling: a_j = 1 iff u_j < p_j (torch.bernoulli's rule), u_j the uniform the
 * multi-categorical step draws for flat index j of the row's stream env
 * (agx_multi.h): ((word (j & 3) >> 8) + 0.5) 2^-24 of the Philox4x32-10 block
 * with counter words (env lo, env hi, counter lo, counter hi ^ ((j >> 2) << 24))
 * and key words (seed lo, seed hi).  sample 0: the mode, a_j = 1 iff l_j > 0 (a
 * logit of exactly 0, and a masked one, give 0). */
#ifndef AGX_BERNOULLI_H
#define AGX_BERNOULLI_H

#include "agx_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The policy step of PPO.get_action (agilerl/algorithms/ppo.py:567-633) for a
 * runtime layer list whose actor output is the n = net->n_actions logits of a
 * MultiBinary space.  One workgroup per (agent, 16-row block), forward as
 * agx_ppo_act_graph (same workspace size rule, same AGX_GRAPH_FEW switch).
 * action_mask [P][..][n] (device, uint8) with agent stride mask_agent_stride
 * bytes (row r of agent p at p mask_agent_stride + r n), or NULL.
 * actions int64 [P][..][n] holding 0 / 1, row r of agent p at
 * (p out_agent_stride + r) n.  log_probs / values / entropy with agent stride
 * out_agent_stride; each may be NULL.  actions_flat int64 [P N n] (the env
 * staging, system-scope stores) or NULL. */
size_t agx_ppo_act_bern_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t N);
int agx_ppo_act_bern_graph(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params, const float *obs,
                           int64_t obs_agent_stride, const uint8_t *action_mask, int64_t mask_agent_stride, int sample,
                           uint64_t seed, uint64_t counter, int64_t *actions, float *log_probs, float *values,
                           float *entropy, int64_t out_agent_stride, int64_t *actions_flat,
                           const int64_t *agent_env_base, void *workspace, void *stream);

/* Persistent rollout / evaluation of a MultiBinary population: the host-paced
 * loops of agx_ppo_rollout_graph_persistent / agx_ppo_eval_graph_persistent
 * (agx_graph.h: same agx_rollout_io steps, control block protocol and bytes,
 * args bytes, workgroup count agx_ppo_rollout_graph_workgroups(P, N), Philox
 * counters, AGX_ROLLOUT_ABORT / AGX_ROLLOUT_STOP) around
 * agx_ppo_act_bern_graph's step, one launch per rollout.  A step's
 * agx_rollout_io.actions is the int64 slot [..][n] (row r of agent p at
 * (p slot_agent_stride + r) n) and actions_flat the int64 staging [P N n],
 * both 0 / 1.  No step may stage a legal-action mask (AGX_EINVAL).  Every
 * workgroup must be co-resident: AGX_EUNSUPPORTED beyond
 * agx_ppo_rollout_bern_graph_max_workgroups() (this kernel's own occupancy).
 * The net is checked as agx_ppo_act_bern_graph checks it; `workspace` as
 * there. */
int64_t agx_ppo_rollout_bern_graph_max_workgroups(void);
int agx_ppo_rollout_bern_graph_persistent(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params,
                                          const agx_rollout_io *ios, int64_t nsteps, uint32_t base, uint64_t seed,
                                          uint64_t counter0, void *args_host, agx_rollout_ctl *ctl, double timeout_s,
                                          void *workspace, void *stream);
int agx_ppo_eval_bern_graph_persistent(const agx_ppo_graph *net, int64_t P, int64_t N, const float *params,
                                       const float *stage_obs, int64_t *actions_flat, const int64_t *agent_env_base,
                                       int64_t nsteps, uint32_t base, uint64_t seed, uint64_t counter0,
                                       void *args_host, agx_rollout_ctl *ctl, double timeout_s, void *workspace,
                                       void *stream);

/* The Bernoulli twin of agx_ppo_loss_fwd_bwd (agx.h; ppo.py:868-902):
 * num_minibatches minibatches of `batch` rows over n bits (1 <= n <=
 * AGX_PPO_GRAPH_MAX_ACTIONS, else AGX_EINVAL).
 *   logits [nmb batch][n], value [nmb batch]                    (network outputs, raw)
 *   actions int64 [rows][n], mask uint8 [rows][n] or NULL,
 *   old_logp / adv / ret / old_value [rows]                     (the rollout)
 *   index [nmb batch] int64 rollout row of each sample, or NULL (sample i is row i)
 * -> g_logits [nmb batch][n], g_value [nmb batch], stats [nmb][8] (the layout
 * of agx_ppo_loss_fwd_bwd; may be NULL).  With gl = d loss / d log_prob and
 * g_h = -ent_coef / batch:
 *   g_logit_j = gl (a_j - p_j) + g_h dH/dl_j          (a_j - p_j: q_j or -p_j)
 *   dH/dl_j   = -p_j q_j (t(p_j) - t(q_j)),  t(x) = log(x + 1e-8) + x / (x + 1e-8)
 * and exactly 0 for a masked logit.  A stored action other than 0 counts as 1
 * (a != 0): defined behaviour, no error.  No atomics: equal bits every run. */
int agx_ppo_bern_loss_fwd_bwd(const float *logits, const float *value, int32_t n, const int64_t *actions,
                              const uint8_t *mask, const float *old_logp, const float *adv, const float *ret,
                              const float *old_value, const int64_t *index, int64_t batch, int64_t num_minibatches,
                              float clip_coef, float vf_coef, float ent_coef, float *g_logits, float *g_value,
                              float *stats, void *stream);

/* PPO.learn for a Bernoulli head: agx_ppo_learn_graph (agx_graph.h) over the
 * layer list of the categorical network with n_actions = n, the per-row math
 * that of agx_ppo_bern_loss_fwd_bwd above.
 *
 * agx_ppo_bern_graph_check: host-only (no HIP call).  AGX_OK when the learner
 * takes this net; AGX_EINVAL with the reason in agx_last_error otherwise
 * (exactly what agx_ppo_graph_check rejects: a Bernoulli head adds no
 * condition of its own, n = net->n_actions being the head).  The workspace
 * query returns 0 and the learn call returns AGX_EINVAL without a launch on
 * such a net.
 *
 * agx_ppo_learn_bern_graph takes agx_ppo_learn_graph's argument block with
 * args->actions int64 [P][S][n] and args->action_masks uint8 [P][S][n] or NULL.
 * The gather packs a row's n stored actions into one 32-bit target word (bit j
 * = a_j != 0) and its mask into one (bit j: logit j legal), so the workspace
 * is agx_ppo_learn_graph's.  A stored action other than 0 / 1 learns as 1.
 * Per-agent batch / epochs / ent_coef, target_kl, skip_if_set, loss_out /
 * kl_out / epochs_out, error_word (AGX_LEARN_ERR_PERM included) and adam_step
 * behave as in agx_ppo_learn_graph; so do the forms the call picks between
 * (AGX_GRAPH_FEW, AGX_GRAPH_ROWS, AGX_GRAPH_SPLIT), AGX_GRAPH_DEBUG and the
 * fixed summation order: no atomics in the gradient path, equal bits on every
 * run, and an agent's update does not depend on which other agents share the
 * launch. */
int agx_ppo_bern_graph_check(const agx_ppo_graph *net);
size_t agx_ppo_learn_bern_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t S, int64_t epochs,
                                                int64_t batch);
int agx_ppo_learn_bern_graph(const agx_ppo_graph *net, const agx_ppo_learn_args *args, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif
