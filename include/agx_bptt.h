/* Truncated BPTT for recurrent PPO on a rollout that lives in HBM
 * (agilerl/components/rollout_buffer.py:676-922 prepare_sequence_tensors /
 * get_minibatch_sequences, agilerl/algorithms/ppo.py:923-1111):
 *
 *   agx_bptt_plan             the sequence table of a [T][N] rollout
 *   agx_bptt_gather           one minibatch of sequences, padded and unpadded
 *   agx_ppo_seq_loss_fwd_bwd  the clipped loss over the valid rows of a padded
 *                             minibatch, with its three gradients
 *
 * No floating-point atomics, no workgroup waits on another, every sum is taken
 * in a fixed order: two runs give equal bits.  Binding: agilerl_amd/kernels.py. */
#ifndef AGX_BPTT_H
#define AGX_BPTT_H

#include "agx.h"

#ifdef __cplusplus
extern "C" {
#endif

/* BPTTSequenceType (agilerl/typing.py:160-174) */
#define AGX_BPTT_CHUNKED 0
#define AGX_BPTT_MAXIMUM 1
#define AGX_BPTT_FIFTY_PERCENT_OVERLAP 2

#define AGX_BPTT_MAX_HIDDEN_KEYS 4 /* actor / critic encoder x (h, c) */

/* Rows of `seq` (and of `row_offset`, plus one) that agx_bptt_plan may write:
 * sequences of one env start at distinct steps under every type, so T * N
 * bounds their number. */
int64_t agx_bptt_capacity(int64_t T, int64_t N);

/* Bytes of agx_bptt_plan's workspace (per env: three counts, two offsets). */
size_t agx_bptt_plan_workspace_bytes(int64_t N);

/* dones uint8 [T][N] (anything but 0 ends an episode; T: the filled length).
 * An episode also ends at T - 1.  An episode of e steps gives, with
 * m = max_seq_len (0: none): one sequence of e steps when m == 0 or e < m, else
 *   CHUNKED                 e / m sequences of m steps from 0, m, 2m ... (the
 *                           tail e % m is dropped)
 *   MAXIMUM                 e - m + 1 sequences from 0, 1, 2 ...
 *   FIFTY_PERCENT_OVERLAP   sequences from 0, m / 2, ... up to e - m (m >= 2)
 * in env-major order, the episodes of an env in time order.
 *   seq        int32 [capacity][3]  (env, first step, length)
 *   row_offset int32 [capacity + 1] exclusive prefix of the lengths; entry S
 *                                   is their sum
 *   meta       int32 [4]            S, L = the longest sequence, the sum, 0
 * Needs T * N * max(m, 1) < 2^31.  Three launches. */
int agx_bptt_plan(const uint8_t *dones, int64_t T, int64_t N, int64_t max_seq_len, int type, int32_t *seq,
                  int32_t *row_offset, int32_t *meta, void *workspace, void *stream);

/* One minibatch: sequences ids[0 .. Bs) of the table, padded to L steps.
 * local_off[b]: the sum of the lengths of ids[0 .. b) (the place of sequence
 * b's first step among the minibatch's valid rows); n_valid: their total.
 * Sources are the rollout's [T][N][...] arrays; hidden[k] is
 * [T][N][layers[k]][H[k]].  Outputs:
 *   obs_out [Bs][L][D], act_out [Bs][L][A], mask_out uint8 [Bs][L][M] (when
 *   mask != NULL), all zero on pad rows; pad_mask uint8 [Bs][L];
 *   hidden_out[k] [layers[k]][Bs][H[k]]: the state stored at each sequence's
 *   first step;
 *   old_logp / adv / ret / old_value [n_valid] and valid_row int64 [n_valid]
 *   (the padded row b * L + t of each valid row), sequence-major then time.
 * Every output element is written, so nothing needs clearing first.  An id
 * outside [0, S) gives an all-pad sequence.  One launch. */
typedef struct agx_bptt_gather_args {
    const int32_t *seq;
    const int64_t *ids;
    const int32_t *local_off;
    int64_t S, Bs, L, T, N, D, A, M, n_valid;
    const float *obs, *actions;
    const uint8_t *mask;
    const float *log_probs, *advantages, *returns, *values;
    const float *hidden[AGX_BPTT_MAX_HIDDEN_KEYS];
    int32_t layers[AGX_BPTT_MAX_HIDDEN_KEYS], H[AGX_BPTT_MAX_HIDDEN_KEYS];
    int32_t n_hidden, pad_;
    float *obs_out, *act_out;
    uint8_t *mask_out, *pad_mask;
    float *hidden_out[AGX_BPTT_MAX_HIDDEN_KEYS];
    float *old_logp, *adv, *ret, *old_value;
    int64_t *valid_row;
} agx_bptt_gather_args;

int agx_bptt_gather(const agx_bptt_gather_args *args, void *stream);

/* Bytes of agx_ppo_seq_loss_fwd_bwd's workspace for `rows` padded rows. */
size_t agx_ppo_seq_loss_workspace_bytes(int64_t rows);

/* The masked twin of agx_ppo_loss_fwd_bwd.  logp / value / entropy [rows] are
 * the network's outputs over every padded row; valid_row [n_valid], strictly
 * ascending, names the rows that count, and old_logp / adv / ret / old_value
 * [n_valid] belong to them in that order.  Means are over n_valid.  The value
 * loss is mean(max((v - R)^2, (v_clip - R)^2)), without the flat loop's 1/2
 * (ppo.py:1035 against ppo.py:889).  g_logp / g_value / g_entropy [rows]: the
 * gradients of the loss, 0 on pad rows.
 * stats float [8]: loss, policy, value, entropy loss, approx_kl, clip fraction,
 * 0, 0; summed in double in a fixed order.  Two launches. */
int agx_ppo_seq_loss_fwd_bwd(const float *logp, const float *value, const float *entropy, int64_t rows,
                             const int64_t *valid_row, int64_t n_valid, const float *old_logp, const float *adv,
                             const float *ret, const float *old_value, float clip_coef, float vf_coef,
                             float ent_coef, float *g_logp, float *g_value, float *g_entropy, float *stats,
                             void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_BPTT_H */
