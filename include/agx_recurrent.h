/* The fused policy step of recurrent PPO (agilerl/algorithms/ppo.py with
 * `recurrent`, separate encoders): one launch takes a block of envs through
 * both networks of the agent, the StochasticActor and the ValueNetwork, each
 * an EvolvableLSTM encoder (nn.LSTM, output Linear, output activation) and an
 * EvolvableMLP head, and through the distribution of the action space:
 *
 *   per network:  (h', c') = LSTM(obs, (h, c))  at T = 1, every layer
 *                 latent   = act(W_out h'_top + b_out)
 *                 head     = Linear [LayerNorm] ReLU ... Linear
 *   Discrete:     masked logits, log-softmax, entropy, Gumbel-max sample
 *   Box:          mean + exp(log_std) * eps, Gaussian log-prob and entropy
 *   MultiDiscrete: K categoricals over slices of the A = sum nvec masked logits
 *                 (agx_multi.h): per-component log-softmax, entropy and
 *                 Gumbel-max sample; log-prob and entropy summed over k
 *   MultiBinary:  A independent Bernoullis over the masked logits
 *                 (agx_bernoulli.h)
 *
 * Grid (ceil(N / 16), 2): a workgroup owns a 16-env row tile of one network
 * (y = 0 the actor, y = 1 the critic).  The tiles of every layer stay in LDS,
 * the cell update in registers; only the step's outputs reach global memory.
 * The new states have the bits of agx_lstm_forward at T = 1 (the same gate
 * chains, csrc/lstm_gates.h), so sequences the learner re-runs from stored
 * states meet the states the rollout carried.  fp32 on
 * v_mfma_f32_16x16x4_f32; no atomics; no workgroup waits on another.
 *
 * The samples are the Philox streams of agx_ppo_act (Discrete: Gumbel-max,
 * word a & 3 of the block of (env, counter ^ (a >> 2) << 56)) and of
 * agx_ppo_act_gauss_graph (Box: Box-Muller per dimension), keyed by the env's
 * row index, `seed` and `counter`.  MultiDiscrete scores flat logit j as
 * Discrete scores action j and takes each component's first maximum, so
 * nvec = (A) makes Discrete's choices; MultiBinary's bit j is u_j < sigmoid(lg_j)
 * with the u_j of that score (agx_ppo_act_bern_graph's rule).
 *
 * Binding: agilerl_amd/kernels.py ppo_act_recurrent. */
#ifndef AGX_RECURRENT_H
#define AGX_RECURRENT_H

#include "agx_graph.h"
#include "agx_lstm.h"
#include "agx_multi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_RECURRENT_MAX_HEAD 4 /* head Linear layers: up to 3 hidden and the output */

/* the actor's distribution: the values of `box` */
#define AGX_RECURRENT_HEAD_DISCRETE 0
#define AGX_RECURRENT_HEAD_BOX 1
#define AGX_RECURRENT_HEAD_MULTI 2     /* multi-categorical (MultiDiscrete) */
#define AGX_RECURRENT_HEAD_BERNOULLI 3 /* MultiBinary */

#define AGX_RECURRENT_ACT_NONE 0
#define AGX_RECURRENT_ACT_RELU 1
#define AGX_RECURRENT_ACT_TANH 2

/* y = x W^T + b, W [out][in]; ln_w / ln_b: the affine of a LayerNorm over
 * `out` after it (eps 1e-5), or both NULL; relu: ReLU last. */
typedef struct agx_recurrent_linear {
    const float *w, *b, *ln_w, *ln_b;
    int32_t in, out, relu, pad_;
} agx_recurrent_linear;

/* One network.  The pointers are the live module parameters.  Limits: the
 * LSTM's (agx_lstm.h); latent and every hidden head width in [1,
 * AGX_PPO_GRAPH_MAX_WIDTH]; 2 <= n_head <= AGX_RECURRENT_MAX_HEAD, the last
 * head layer plain (no LayerNorm, no ReLU). */
typedef struct agx_recurrent_net {
    agx_lstm_desc lstm;      /* g_* unused */
    const float *out_w, *out_b; /* the encoder's output Linear [latent][H], [latent] */
    int32_t latent, out_act; /* AGX_RECURRENT_ACT_* after it */
    agx_recurrent_linear head[AGX_RECURRENT_MAX_HEAD];
    int32_t n_head, pad_;
    const float *h, *c;      /* [L][N][H]: the states the step starts from */
    float *h_next, *c_next;  /* [L][N][H]: the states after it (may be h, c themselves) */
    float *h_store, *c_store; /* [N][L][H] or NULL: the states the step was taken from, rollout-buffer order */
} agx_recurrent_net;

/* One policy step of N envs.  Every output pointer may be NULL. */
typedef struct agx_recurrent_step {
    agx_recurrent_net actor, critic; /* actor.head ends in A outputs, critic.head in 1 */
    const float *obs;        /* [N][in] */
    const float *log_std;    /* [A], Box only */
    const uint8_t *reset;    /* [N] or NULL: 1 = the row starts from the zero state (and stores it) */
    const uint8_t *mask;     /* [N][A] or NULL, not with Box: 1 = legal; illegal logits become -1e8 */
    int64_t N;
    int32_t A;               /* Discrete: actions; Box: dimensions; multi: sum nvec; Bernoulli: bits;
                                1 .. AGX_PPO_GRAPH_MAX_ACTIONS */
    int32_t box;             /* AGX_RECURRENT_HEAD_* */
    int32_t sample;          /* 0: no draw, `actions` and `log_probs` are not written */
    int32_t pad_;
    uint64_t seed, counter;
    float *actions;          /* Discrete [N] (the index as a float), Box [N][A], multi [N][K] (component k's
                                index in [0, n_k) as a float), Bernoulli [N][A] (0 / 1) */
    float *log_probs, *entropy, *values; /* [N] */
    float *obs_store;        /* [N][in] or NULL: a copy of obs (the rollout slot) */
    agx_multi_head multi;    /* AGX_RECURRENT_HEAD_MULTI only: K >= 1 components, every n_k >= 1, sum n_k == A.
                                The host reduces it to one word for the kernel (bit j: logit j starts a component) */
} agx_recurrent_step;

/* One launch on `stream`; nothing is synchronised.  AGX_EINVAL (agx_last_error
 * says why) for shapes outside the limits. */
int agx_ppo_act_recurrent(const agx_recurrent_step *step, void *stream);

/* The same step for an agent whose networks share one encoder (`share_encoders`): step->actor is the shared
 * encoder with the actor's head; of step->critic only `head` and `n_head` are read, and its first layer's `in`
 * must be actor.latent.  The critic's lstm, out_*, latent, states and stores are ignored.  Grid (ceil(N / 16), 1):
 * a workgroup runs the LSTM and the output Linear once per row tile and then both heads off the one latent tile in
 * LDS, depth by depth as one tile list over its 8 waves.  Every output tile is the same single-wave chain as in
 * agx_ppo_act_recurrent, so actions, log-probs, entropy and next states have the bits that entry gives on the same
 * actor, and the values the bits it gives for a critic whose encoder is a copy of the actor's. */
int agx_ppo_act_recurrent_shared(const agx_recurrent_step *step, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_RECURRENT_H */
