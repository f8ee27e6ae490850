/* The two device steps of a TD3 / DDPG update that lie between the target
 * networks' forwards: target-policy smoothing and the (twin-)critic TD target
 * with the MSE loss and its gradients.
 *
 * The reference runs them as torch ops (agilerl/algorithms/td3.py:493-515,
 * agilerl/algorithms/ddpg.py:448-461): a clamp of the noise, an add, the
 * min / max of multi_dim_clamp (agilerl/utils/algo_utils.py:268-291), then
 * torch.min of the two target critics, 1 - d, two multiplies, an add, two
 * nn.MSELoss and autograd's backward through them — about a dozen
 * launch-latency-bound kernels at the batch sizes of an update (64-256
 * rows).  Here each step is one launch (plus the fixed-order loss sum).
 * All tensors are f32 on the device, caller-owned; nothing synchronises.
 * Binding: INTEGRATION.md. */
#ifndef AGX_TD3_H
#define AGX_TD3_H

#include "agx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Target-policy smoothing.  Replaces agilerl/algorithms/td3.py:493-501
 * (TD3.learn) and agilerl/algorithms/ddpg.py:448-456 (DDPG.learn):
 *   out = max(min(mu + clamp(noise, -noise_clip, noise_clip), high[k]), low[k])
 * mu, noise, out: [B][A] (mu: the target actor's output; noise: the caller's
 * N(0, policy_noise) draw — no RNG here); low, high: [A], +-inf allowed.
 * One f32 rounding per op; NaNs propagate as in torch.clamp / torch.min /
 * torch.max.  out may alias mu. */
int agx_td3_smooth_actions(const float *mu, const float *noise, const float *low, const float *high, int64_t B,
                           int64_t A, double noise_clip, float *out, void *stream);

/* Bytes of device workspace agx_td3_critic_target needs (the block partials
 * of the two loss sums). */
size_t agx_td3_workspace_bytes(int64_t B);

/* Twin-critic TD target + MSE.  Replaces agilerl/algorithms/td3.py:503-515
 * (TD3.learn); with q2 == q_next2 == NULL the single-critic form,
 * agilerl/algorithms/ddpg.py:457-461 (DDPG.learn):
 *   y    = r + ((1 - d) * (float)gamma) * min(q_next1, q_next2)
 *   loss = f32(mean((q1 - y)^2)) + f32(mean((q2 - y)^2))
 *   g_qk = d loss / d qk = (qk - y) * (2 / B)
 * q1, q2, q_next1, q_next2, rewards, dones, y, g_q1, g_q2: (B) f32 (dones as
 * the replay buffer stores them); y, g_q1, g_q2 may each be NULL; loss: one
 * f32; workspace: agx_td3_workspace_bytes(B). */
int agx_td3_critic_target(const float *q1, const float *q2, const float *q_next1, const float *q_next2,
                          const float *rewards, const float *dones, int64_t B, double gamma, float *y, float *g_q1,
                          float *g_q2, float *loss, void *workspace, void *stream);

/* MATD3's critic step: the twin form above behind MADDPG's input rules.
 * Replaces agilerl/algorithms/matd3.py:861-880 (MATD3.learn_individual):
 * NaN rewards -> 0, NaN dones -> 1, dones cast to uint8 and 1 - d formed in
 * uint8 arithmetic (a done of 2 gives 255), then
 *   y    = r + ((1 - d) * (float)gamma) * min(q_next1, q_next2)   (torch.min: a NaN wins)
 *   loss = f32(mean((q1 - y)^2)) + f32(mean((q2 - y)^2))
 *   g_qk = (qk - y) * (2 / B)
 * Shapes as for agx_td3_critic_target; q2 and q_next2 are required; y, g_q1,
 * g_q2 may each be NULL; workspace: agx_td3_workspace_bytes(B). */
int agx_matd3_critic_target(const float *q1, const float *q2, const float *q_next1, const float *q_next2,
                            const float *rewards, const float *dones, int64_t B, double gamma, float *y, float *g_q1,
                            float *g_q2, float *loss, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_TD3_H */
