/* The heads of recurrent PPO's BPTT learner: everything after the LSTM of both
 * networks of an agent, over the R = Bs * L padded rows of a minibatch, with
 * its backward.
 *
 *   per network:  latent = act(W_out h_top + b_out)
 *                 head   = Linear [LayerNorm] ReLU ... Linear
 *   actor:        masked logits -> log_prob of the given action, entropy
 *                 (Discrete: log-softmax, H = -sum p log(p + 1e-8);
 *                  Box: the diagonal Gaussian of gauss_head.h with log_std;
 *                  multi-categorical: the K categoricals of agx_multi.h over
 *                  slices of the A = sum nvec logits, summed over k;
 *                  Bernoulli: the A independent bits of agx_bernoulli.h)
 *   critic:       value
 *
 * A network is an agx_recurrent_net (agx_recurrent.h) with the limits of
 * agx_ppo_act_recurrent; its lstm, state and store fields are not read, the
 * LSTM's width comes with h_top.  Every pointer is a live module parameter.
 *
 * Forward: one launch, grid (ceil(R / 16), 2): a workgroup takes a 16-row tile
 * of one network's h_top through every layer in LDS.  With `saved` it also
 * writes what the backward reads.  Backward: two launches.  `rows` (the same
 * grid) turns g_log_prob / g_entropy / g_value into the gradient of every
 * layer's pre-activation, stores those in the workspace and ends in dh_top;
 * `params` gives one wave one 16 x 16 tile of some layer's [dW | db], summed
 * over all R rows in ascending order, and the LayerNorm affines and log_std as
 * column sums.  fp32 on v_mfma_f32_16x16x4_f32, 8-wave workgroups, no atomics,
 * no workgroup waits on another, every sum in a fixed order: two runs give
 * equal bits.  The kernels are row-wise: a padded row is a row like any other,
 * and one whose three upstream gradients are zero adds zero everywhere.
 *
 * Binding: agilerl_amd/kernels.py recurrent_heads_forward / _backward. */
#ifndef AGX_RECURRENT_HEADS_H
#define AGX_RECURRENT_HEADS_H

#include <stddef.h>

#include "agx_recurrent.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradients of one Linear of a network; ln_w / ln_b where the layer has a LayerNorm. */
typedef struct agx_recurrent_linear_grad {
    float *w, *b, *ln_w, *ln_b;
} agx_recurrent_linear_grad;

/* The inputs of both directions.  Index 0 is the actor, 1 the critic. */
typedef struct agx_recurrent_heads {
    agx_recurrent_net net[2]; /* net[0].head ends in A outputs, net[1].head in 1 */
    const float *h_top[2];   /* [R][H[k]]: the top LSTM layer's output at every padded row */
    int32_t H[2];            /* a multiple of 16 in [16, AGX_LSTM_MAX_HIDDEN] */
    const float *actions;    /* Discrete [R] (the index as a float), Box [R][A], multi [R][K] (component k's index
                                as a float; one outside [0, n_k) is clamped into it), Bernoulli [R][A] (anything
                                but 0 counts as 1) */
    const float *log_std;    /* [A], Box only */
    const uint8_t *mask;     /* [R][A] or NULL, not with Box: 1 = legal; illegal logits become -1e8 and get a
                                gradient of exactly 0 */
    int64_t R;               /* 1 .. 2^24 */
    int32_t A;               /* 1 .. AGX_PPO_GRAPH_MAX_ACTIONS: actions, dimensions, sum nvec or bits */
    int32_t box;             /* AGX_RECURRENT_HEAD_* (agx_recurrent.h) */
    agx_multi_head multi;    /* AGX_RECURRENT_HEAD_MULTI only, as in agx_recurrent_step */
} agx_recurrent_heads;

/* The backward's upstream gradients and outputs.  Every output is overwritten. */
typedef struct agx_recurrent_heads_grads {
    const float *g_log_prob, *g_entropy, *g_value; /* [R] */
    float *dh_top[2];        /* [R][H[k]] */
    float *out_w[2], *out_b[2];
    agx_recurrent_linear_grad head[2][AGX_RECURRENT_MAX_HEAD];
    float *log_std;          /* [A], Box only */
} agx_recurrent_heads_grads;

/* Bytes of the forward's `saved` (layer inputs, pre-LayerNorm outputs, the masked logits or means) and of the
 * backward's workspace (every layer's dZ; dY and x-hat of the LayerNorm layers).  0 for shapes outside the limits. */
size_t agx_recurrent_heads_saved_bytes(const agx_recurrent_heads *heads);
size_t agx_recurrent_heads_workspace_bytes(const agx_recurrent_heads *heads);

/* log_prob, entropy, value [R].  saved: NULL (nothing kept) or agx_recurrent_heads_saved_bytes bytes.  One launch on
 * `stream`; nothing is synchronised.  AGX_EINVAL (agx_last_error says why) for shapes outside the limits. */
int agx_recurrent_heads_forward(const agx_recurrent_heads *heads, float *log_prob, float *entropy, float *value,
                                void *saved, void *stream);

/* `heads` and `saved` as the forward had them.  Two launches on `stream`. */
int agx_recurrent_heads_backward(const agx_recurrent_heads *heads, const void *saved,
                                 const agx_recurrent_heads_grads *grads, void *workspace, void *stream);

/* The same four entry points for an agent whose networks share one encoder (`share_encoders`), on the same
 * structs: h_top[0], H[0] and net[0].out_* are the shared ones, of net[1] only the head is read (its first
 * layer's `in` must be net[0].latent); h_top[1], H[1], dh_top[1], out_w[1] and out_b[1] are ignored.
 *
 * Forward, grid (ceil(R / 16), 1): one latent per row tile, saved once, then both heads in that workgroup as one
 * tile list per depth; log_prob, entropy and value have the bits of agx_recurrent_heads_forward for a critic whose
 * output Linear is a copy of the actor's on the same h_top.  Backward rows, the same grid: one workgroup walks both
 * heads back to the latent, forms dLatent = dX_actor + dX_critic in LDS in that order, applies the output
 * activation's backward once and writes one dZ_out and one dh_top[0] = dZ_out W_out.  Backward params: the same
 * one-wave jobs over one output Linear ([dW_out | db_out] from the summed dZ_out) and the two heads. */
size_t agx_recurrent_heads_saved_bytes_shared(const agx_recurrent_heads *heads);
size_t agx_recurrent_heads_workspace_bytes_shared(const agx_recurrent_heads *heads);
int agx_recurrent_heads_forward_shared(const agx_recurrent_heads *heads, float *log_prob, float *entropy,
                                       float *value, void *saved, void *stream);
int agx_recurrent_heads_backward_shared(const agx_recurrent_heads *heads, const void *saved,
                                        const agx_recurrent_heads_grads *grads, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_RECURRENT_HEADS_H */
