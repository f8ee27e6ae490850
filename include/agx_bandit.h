/* Arm selection of the neural contextual bandits (NeuralUCB / NeuralTS): the
 * per-arm confidence width, the score, the argmax and the Sherman-Morrison
 * update of the inverse covariance, in one call.
 *
 * The reference runs it as torch ops on every env step
 * (agilerl/algorithms/neural_ucb_bandit.py:237-257, neural_ts_bandit.py:
 * 236-254): two batched matmuls, a sqrt, a host argmax in numpy, and
 * sigma_inv @ v @ v.T @ sigma_inv, which holds a D x D by D x D product.
 * All tensors are on the device, caller-owned; nothing synchronises.
 * Binding: INTEGRATION.md. */
#ifndef AGX_BANDIT_H
#define AGX_BANDIT_H

#include "agx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* D = H + bias_one up to this bound takes the resident form (the D x D matrix
 * in one workgroup's LDS), above it the streaming form up to
 * AGX_BANDIT_MAX_D.  112 x 113 words of matrix, eight staged gradient rows,
 * the u / w vectors and the scores of AGX_BANDIT_MAX_ARMS arms come to 59 KiB:
 * under the 64 KiB a launch takes without opting in to more, so the CU (160
 * KiB) still holds a second workgroup of another agent's stream. */
#define AGX_BANDIT_RESIDENT_MAX_D 112
#define AGX_BANDIT_MAX_D 1025
#define AGX_BANDIT_MAX_ARMS 1024

/* Bytes of device workspace agx_bandit_select needs for A arms and a D x D
 * matrix (the streaming form's column-tile partials and u / w; the resident
 * form needs none and gets the minimum).  0 when (A, D) is out of range. */
size_t agx_bandit_workspace_bytes(int64_t A, int64_t D);

/* Replaces neural_ucb_bandit.py:237-257 / neural_ts_bandit.py:236-254, with
 * D = H + bias_one:
 *   g_k     = fl32(scale * [h_k, 1])  (bias_one = 1)  |  fl32(scale * h_k)  (bias_one = 0)
 *   quad_k  = g_k sigma_inv g_k^T
 *   score_k = mu_k + gamma * sqrt(quad_k)               (mode 0, UCB)
 *           = mu_k + gamma * sqrt(quad_k) * z_k         (mode 1, Thompson)
 *   action  = numpy's argmax of the scores with every arm whose mask byte is not 1 set to -inf
 *             (ties: the first index; a NaN score of a legal arm wins, the first of several; every arm
 *             masked: 0 — what np.argmax(np.ma.array(scores, mask=1 - mask)) gives)
 *   v = g_action, u = sigma_inv v, w = sigma_inv^T v
 *   sigma_inv[i][j] -= u_i w_j / (1 + v . u)            (in place)
 * z_k: words (x, y) of the Philox4x32-10 block with counter (k, 0, *counter lo, *counter hi) and key seed,
 * u1 = ((x >> 8) + 0.5) 2^-24, u2 likewise from y, z = sqrt(-2 ln u1) cospi(2 u2) — agx_gauss.h's draw of
 * dimension 0 of env k.  *counter (may be NULL in mode 0) is advanced by one per mode-1 call; mode 0 leaves it alone.
 * h: [A] rows of H floats, row k at h + k * ldh; mu, scores, quad: [A]; sigma_inv: [D][D] contiguous;
 * mask: [A] bytes or NULL; action, counter: one int64 each.
 * Every sum is accumulated in f64 in a fixed order (no atomics) and rounded to f32 once — the score from
 * the unrounded quadratic form, quad being its rounding: the same bits on every call.  AGX_EINVAL (nothing launched) for A > AGX_BANDIT_MAX_ARMS or D > AGX_BANDIT_MAX_D. */
int agx_bandit_select(const float *h, int64_t ldh, const float *mu, float *sigma_inv, const uint8_t *mask, int64_t A,
                      int64_t H, int bias_one, float scale, float gamma, int mode, uint64_t seed, int64_t *counter,
                      float *scores, float *quad, int64_t *action, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_BANDIT_H */
