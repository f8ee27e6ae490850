/* PPO for MultiDiscrete action spaces: the multi-categorical policy step, loss
 * and fused learner.
 *
 * A MultiDiscrete space with nvec = (n_0 .. n_{K-1}) has L = sum n_k logits:
 * the actor's output layer has width L (no output activation), and component k
 * owns the flat logit indices [off_k, off_k + n_k), off_k = n_0 + .. + n_{k-1}
 * (the reference's StochasticActor, agilerl/networks/actors.py:268, with
 * networks/distributions.py:193-199 and utils/torch_utils.py:260-333).
 * Limits: K >= 1, every n_k >= 1, L <= AGX_PPO_GRAPH_MAX_ACTIONS.
 *
 * Per row:
 *   mask      an optional flat mask [.., L] (uint8, 1 = legal) sets an illegal
 *             logit to -1e8 before anything else (distributions.py:16-28)
 *   lse_k     = m_k + log sum_j exp(lg_j - m_k), m_k the component's maximum
 *   p_j       = exp(lg_j - lse_k)
 *   log_prob  = sum_k (lg[off_k + a_k] - lse_k)
 *   entropy   = sum_k -sum_j p_j log(p_j + 1e-8)
 * Both sums over k run in ascending k in float32; within a component a sum is
 * a fixed-order reduction: equal bits on every launch, whatever other agents
 * share it.
 *
 * Sampling is Gumbel-max per component.  The score of flat logit index j of
 * the row whose stream env is `env` (agx_ppo_act: agent_env_base[p] + n, or
 * p N + n) is agx_ppo_act's score of action j,
 *   lg_j - log(-log u_j),  u_j = ((word (j & 3) >> 8) + 0.5) 2^-24
 * of the Philox4x32-10 block with counter words (env lo, env hi, counter lo,
 * counter hi ^ ((j >> 2) << 24)) and key words (seed lo, seed hi): keyed by
 * the flat index, so K = 1 draws agx_ppo_act_graph's stream and makes its
 * choice.  The choice of a component is its first maximum (lowest index);
 * sample 0: the first arg-max of the (masked) logits. */
#ifndef AGX_MULTI_H
#define AGX_MULTI_H

#include "agx_graph.h"

#ifdef __cplusplus
extern "C" {
#endif

/* nvec by value: the host packs it into the kernel arguments (no device table) */
typedef struct agx_multi_head {
    int32_t K;
    int32_t nvec[AGX_PPO_GRAPH_MAX_ACTIONS];
} agx_multi_head;

/* The policy step of PPO.get_action (agilerl/algorithms/ppo.py:567-633) for a
 * runtime layer list whose actor output is the L logits of `head`
 * (net->n_actions = L).  One workgroup per (agent, 16-row block), forward as
 * agx_ppo_act_graph (same workspace size rule, same AGX_GRAPH_FEW switch).
 * action_mask [P][..][L] (device, uint8) with agent stride mask_agent_stride
 * bytes (row n of agent p at p mask_agent_stride + n L), or NULL.
 * actions int64 [P][..][K], row n of agent p at (p out_agent_stride + n) K:
 * component k's choice in [0, n_k).  log_probs / values / entropy with agent
 * stride out_agent_stride; each may be NULL.  actions_flat int64 [P N K] (the
 * env staging, system-scope stores) or NULL. */
size_t agx_ppo_act_multi_graph_workspace_bytes(const agx_ppo_graph *net, int64_t P, int64_t N);
int agx_ppo_act_multi_graph(const agx_ppo_graph *net, agx_multi_head head, int64_t P, int64_t N, const float *params,
                            const float *obs, int64_t obs_agent_stride, const uint8_t *action_mask,
                            int64_t mask_agent_stride, int sample, uint64_t seed, uint64_t counter, int64_t *actions,
                            float *log_probs, float *values, float *entropy, int64_t out_agent_stride,
                            int64_t *actions_flat, const int64_t *agent_env_base, void *workspace, void *stream);

/* Persistent rollout / evaluation of a MultiDiscrete population: the
 * host-paced loops of agx_ppo_rollout_graph_persistent /
 * agx_ppo_eval_graph_persistent (agx_graph.h: same agx_rollout_io steps,
 * control block protocol and bytes, args bytes, workgroup count
 * agx_ppo_rollout_graph_workgroups(P, N), Philox counters, AGX_ROLLOUT_ABORT /
 * AGX_ROLLOUT_STOP) around agx_ppo_act_multi_graph's step, one launch per
 * rollout.  A step's agx_rollout_io.actions is the int64 slot [..][K] (row n
 * of agent p at (p slot_agent_stride + n) K) and actions_flat the int64
 * staging [P N K].  No step may stage a legal-action mask (AGX_EINVAL).
 * Every workgroup must be co-resident: AGX_EUNSUPPORTED beyond
 * agx_ppo_rollout_multi_graph_max_workgroups() (this kernel's own occupancy).
 * The net and the head are checked as agx_ppo_act_multi_graph checks them;
 * `workspace` as there.  With K = 1 the rollout equals
 * agx_ppo_rollout_graph_persistent's at n_actions = n_0 bit for bit. */
int64_t agx_ppo_rollout_multi_graph_max_workgroups(void);
int agx_ppo_rollout_multi_graph_persistent(const agx_ppo_graph *net, agx_multi_head head, int64_t P, int64_t N,
                                           const float *params, const agx_rollout_io *ios, int64_t nsteps,
                                           uint32_t base, uint64_t seed, uint64_t counter0, void *args_host,
                                           agx_rollout_ctl *ctl, double timeout_s, void *workspace, void *stream);
int agx_ppo_eval_multi_graph_persistent(const agx_ppo_graph *net, agx_multi_head head, int64_t P, int64_t N,
                                        const float *params, const float *stage_obs, int64_t *actions_flat,
                                        const int64_t *agent_env_base, int64_t nsteps, uint32_t base, uint64_t seed,
                                        uint64_t counter0, void *args_host, agx_rollout_ctl *ctl, double timeout_s,
                                        void *workspace, void *stream);

/* The multi-categorical twin of agx_ppo_loss_fwd_bwd (agx.h; ppo.py:868-902):
 * num_minibatches minibatches of `batch` rows.
 *   logits [nmb batch][L], value [nmb batch]                    (network outputs, raw)
 *   actions int64 [rows][K], mask uint8 [rows][L] or NULL,
 *   old_logp / adv / ret / old_value [rows]                     (the rollout)
 *   index [nmb batch] int64 rollout row of each sample, or NULL (sample i is row i)
 * -> g_logits [nmb batch][L], g_value [nmb batch], stats [nmb][8] (the layout
 * of agx_ppo_loss_fwd_bwd; may be NULL).  With gl = d loss / d log_prob and
 * g_h = -ent_coef / batch:
 *   g_logit_j = gl (1[j == off_k + a_k] - p_j) + g_h dH_k/dlg_j
 *   dH_k/dlg_j = -p_j (t_j - sum_i p_i t_i),  t_i = log(p_i + 1e-8) + p_i / (p_i + 1e-8)
 * and exactly 0 for a masked logit.  An action outside [0, n_k) is clamped
 * into it.  No atomics: equal bits every run. */
int agx_ppo_multi_loss_fwd_bwd(const float *logits, const float *value, agx_multi_head head, const int64_t *actions,
                               const uint8_t *mask, const float *old_logp, const float *adv, const float *ret,
                               const float *old_value, const int64_t *index, int64_t batch, int64_t num_minibatches,
                               float clip_coef, float vf_coef, float ent_coef, float *g_logits, float *g_value,
                               float *stats, void *stream);

/* PPO.learn for a multi-categorical head: agx_ppo_learn_graph (agx_graph.h)
 * over the layer list of the categorical network with n_actions = L, the
 * per-row math that of agx_ppo_multi_loss_fwd_bwd above.
 *
 * agx_ppo_multi_graph_check: host-only (no HIP call).  AGX_OK when the learner
 * takes this net and head; AGX_EINVAL with the reason in agx_last_error
 * otherwise (anything agx_ppo_graph_check rejects, K < 1, an n_k < 1, sum n_k
 * != net->n_actions or > AGX_PPO_GRAPH_MAX_ACTIONS).  The workspace query
 * returns 0 and the learn call returns AGX_EINVAL without a launch on such a
 * head.
 *
 * agx_ppo_learn_multi_graph takes agx_ppo_learn_graph's argument block with
 * args->actions int64 [P][S][K] and args->action_masks uint8 [P][S][L] or NULL.
 * The gather packs a row's actions into one 32-bit target word (bit off_k + a_k
 * for every k) and its mask into one (bit j: logit j legal), so the workspace
 * is agx_ppo_learn_graph's.  An action outside [0, n_k) is clamped into its
 * component (defined behaviour, as in the loss kernel above): the learn equals
 * the learn of the clamped rollout bit for bit and sets no error.  Per-agent
 * batch / epochs / ent_coef, target_kl, skip_if_set, loss_out / kl_out /
 * epochs_out, error_word (AGX_LEARN_ERR_PERM included) and adam_step behave as
 * in agx_ppo_learn_graph; so do the forms the call picks between
 * (AGX_GRAPH_FEW, AGX_GRAPH_ROWS, AGX_GRAPH_SPLIT), AGX_GRAPH_DEBUG and the
 * fixed summation order: no atomics in the gradient path, equal bits on every
 * run, and an agent's update does not depend on which other agents share the
 * launch.  With K = 1 the result equals agx_ppo_learn_graph's at n_actions =
 * n_0 bit for bit. */
int agx_ppo_multi_graph_check(const agx_ppo_graph *net, agx_multi_head head);
size_t agx_ppo_learn_multi_graph_workspace_bytes(const agx_ppo_graph *net, agx_multi_head head, int64_t P, int64_t S,
                                                 int64_t epochs, int64_t batch);
int agx_ppo_learn_multi_graph(const agx_ppo_graph *net, agx_multi_head head, const agx_ppo_learn_args *args,
                              void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif
