/* The loss of a conservative Q-learning (CQL / "CQN") update for Discrete
 * actions: DQN's TD target and MSE plus the row-wise log-sum-exp regulariser,
 * with the dense gradient with respect to Q(s), in one pass.
 *
 * The reference runs it as torch ops (agilerl/algorithms/cqn.py:234-252): a
 * max or an argmax + gather over Q(s'), three elementwise ops for y, a gather
 * of Q(s)[a], logsumexp, two means, nn.MSELoss, an add, and autograd's
 * backward through all of them — about two dozen launch-latency-bound kernels
 * at the batch sizes of an update (64-256 rows).  Here it is one launch plus
 * the fixed-order sum of the block partials.  All tensors are f32 on the
 * device (actions int64), caller-owned; nothing synchronises.
 * Binding: INTEGRATION.md. */
#ifndef AGX_CQN_H
#define AGX_CQN_H

#include "agx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Bytes of device workspace agx_cqn_loss needs (the block partials of the
 * three sums; their number depends on which form of the kernel A selects). */
size_t agx_cqn_workspace_bytes(int64_t B, int64_t A);

/* Replaces agilerl/algorithms/cqn.py:234-252 (CQN.learn) and the backward
 * pass down to Q(s):
 *   q_t   = max_a q_next_target[i]  |  q_next_target[i][argmax_a q_next_online[i]]  (double_q)
 *   y     = r + ((float)gamma * q_t) * (1 - d)           (bit-identical to agx_td_target's y)
 *   lse_i = logsumexp_a q_cur[i]                          (shifted by the row maximum, 0 when it is infinite)
 *   terms = (f32 mean_i lse_i, f32 mean_{i,a} q_cur, f32 mean_i (q_cur[i][a_i] - y_i)^2)
 *   loss  = (terms[0] - terms[1]) + 0.5f * terms[2]      (f32, this order)
 *   g_q[i][a] = exp(q_cur[i][a] - lse_i) / B - 1 / (B A) + [a == a_i] (q_cur[i][a_i] - y_i) / B
 * q_next_online (NULL unless double_q), q_next_target, q_cur, g_q: [B][A];
 * actions int64 [B] with 0 <= actions[i] < A (not checked on the device);
 * rewards, dones, y: [B]; loss: one f32; terms: three f32 or NULL; workspace:
 * agx_cqn_workspace_bytes(B, A).  g_q is written in full.  The q_next rules
 * are agx_td_target's (a NaN is the maximum, the first NaN's index the
 * argmax, ties take the first index); a NaN in a row of q_cur makes that
 * row's lse, its row of g_q and the loss NaN.  The three means are f64 sums
 * over fixed-order block partials: no atomics, the same bits on every call.
 *
 * Two forms, chosen by A: for A <= 32 a block stages its 256 x A tile of
 * q_cur in LDS (coalesced, 16-byte loads when q_cur and g_q are 16-byte
 * aligned), each lane walks one row there and the tile of g_q is stored
 * coalesced; for A > 32 a wave takes a row, its lanes stride over the columns
 * and the row's maxima and sums are wave reductions. */
int agx_cqn_loss(const float *q_next_online, const float *q_next_target, const float *q_cur, const int64_t *actions,
                 const float *rewards, const float *dones, int64_t B, int64_t A, double gamma, int double_q,
                 float *y, float *g_q, float *loss, float *terms, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_CQN_H */
