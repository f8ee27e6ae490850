/* Stacked LSTM sequences (torch.nn.LSTM, batch_first, unidirectional, no
 * projection; agilerl/modules/lstm.py EvolvableLSTM's `{name}_lstm`):
 *
 *   (i, f, g, o) = (sigm, sigm, tanh, sigm)(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh)
 *   c_t = f * c_{t-1} + i * g,   h_t = o * tanh(c_t)
 *
 * fp32 on v_mfma_f32_16x16x4_f32.  One workgroup carries a 16-row tile of the
 * batch through every layer and every step: c_t stays in registers, h_t in a
 * double-buffered LDS tile, W_hh in registers for H <= AGX_LSTM_RESIDENT_H.
 * A row's result does not depend on B, on T or on the row's place in its
 * tile, so a sequence run in chunks (the state carried through h_n / c_n)
 * has the bits of the sequence run whole.  The backward is a reverse scan per
 * layer on the same tiles, then everything without a serial dependency over
 * all B * T rows at once; no floating-point atomics, every sum in a fixed
 * order.
 *
 * Replaces nn.LSTM's forward and autograd's backward through it; binding:
 * agilerl_amd/modules/lstm.py. */
#ifndef AGX_LSTM_H
#define AGX_LSTM_H

#include "agx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_LSTM_MAX_LAYERS 4
#define AGX_LSTM_MAX_HIDDEN 512    /* H: a multiple of 16 in [16, 512] */
#define AGX_LSTM_MAX_INPUT 512     /* layer 0's input size, any value in [1, 512] */
#define AGX_LSTM_RESIDENT_H 64     /* W_hh operands live in registers up to here */

/* One layer, nn.LSTM layouts, gate order i, f, g, o along 4H: w_ih [4H][in_k]
 * (in_0 = in, in_k = H above), w_hh [4H][H], b_ih / b_hh [4H]; g_*: the
 * backward's outputs of the same shapes (forward: unused). */
typedef struct agx_lstm_layer {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float *g_w_ih, *g_w_hh, *g_b_ih, *g_b_hh;
} agx_lstm_layer;

typedef struct agx_lstm_desc {
    agx_lstm_layer layer[AGX_LSTM_MAX_LAYERS];
    int32_t in, H, L;
} agx_lstm_desc;

/* Bytes of `saved` for B sequences of T steps, N = B * T: per layer the
 * post-activation gates [N][4H] and c_t [N][H], and below the top layer its
 * output h_t [N][H]: 4 * N * H * (6 L - 1).  0 for a descriptor outside the
 * limits (agx_last_error says why). */
size_t agx_lstm_saved_bytes(const agx_lstm_desc *desc, int64_t B, int64_t T);

/* x [B][T][in], h0 / c0 [L][B][H] -> y [B][T][H] (the top layer's h_t), h_n /
 * c_n [L][B][H].  One launch for the whole stack.  saved == NULL: the no-grad
 * form, which writes y, h_n and c_n only (the layers below the top pass their
 * outputs through y in place). */
int agx_lstm_forward(const agx_lstm_desc *desc, const float *x, const float *h0, const float *c0, int64_t B, int64_t T,
                     float *y, float *h_n, float *c_n, void *saved, void *stream);

/* Bytes of the backward's workspace: the gate gradients [N][4H] of the layer
 * at hand and, with L > 1, the gradient [N][H] handed to the layer below. */
size_t agx_lstm_workspace_bytes(const agx_lstm_desc *desc, int64_t B, int64_t T);

/* gy [B][T][H]; gh_n / gc_n [L][B][H] (NULL: zero); gx [B][T][in], gh0 / gc0
 * [L][B][H] (NULL: not needed).  `saved` and y are the forward's.  Writes
 * every g_* of the descriptor, each element once (g_b_ih and g_b_hh get the
 * same sums).  Three launches per layer. */
int agx_lstm_backward(const agx_lstm_desc *desc, const float *x, const float *h0, const float *c0, int64_t B, int64_t T,
                      const float *y, const void *saved, const float *gy, const float *gh_n, const float *gc_n,
                      float *gx, float *gh0, float *gc0, void *workspace, void *stream);

/* ---- The split form (csrc/lstm_split.hip) ---------------------------------
 * A layer split by hidden unit across the device, one launch per time step
 * (wave-tasks of 16 units x 16 rows, grouped by unit tile so that a slice of
 * W_hh is staged through LDS once per workgroup and step), the input half of
 * the gates hoisted into one device-wide projection per layer.  Nothing waits
 * on another workgroup, no atomics, no sum is split, and every element takes
 * the whole kernels' chain: the results have agx_lstm_forward's and
 * agx_lstm_backward's bits.  It serves every descriptor they serve; `saved`
 * has the same layout, so a split forward may be followed by either backward
 * and the other way round.  T + 1 launches per layer forward, at most T + 3
 * backward; no host synchronisation, no allocation, capturable. */

/* Which form is faster for (desc, B, T): *split = 1 from the width at which
 * tools/lstm_time.py measured the split form clear of the whole one in every
 * sequence cell, 0 below it (always 0 for H <= 128).  Host only, no HIP call. */
int agx_lstm_choose_plan(const agx_lstm_desc *desc, int64_t B, int64_t T, int32_t *split);

/* Bytes of the split form's workspace, N = B * T.  Forward (backward == 0):
 * the projection [N][4H] of the layer at hand, 16 N H (used when saved ==
 * NULL; with `saved` the projection lies in its gate region).  Backward: the
 * whole backward's workspace and the cell gradient [B][H]:
 * 4 (N H (L > 1 ? 5 : 4) + B H), which is no less than the forward's, so one
 * buffer of that size serves both.  0 for a descriptor outside the limits. */
size_t agx_lstm_split_workspace_bytes(const agx_lstm_desc *desc, int64_t B, int64_t T, int backward);

/* agx_lstm_forward's arguments and the workspace (never NULL). */
int agx_lstm_forward_split(const agx_lstm_desc *desc, const float *x, const float *h0, const float *c0, int64_t B,
                           int64_t T, float *y, float *h_n, float *c_n, void *saved, void *workspace, void *stream);

/* agx_lstm_backward's arguments; the workspace has the split form's size. */
int agx_lstm_backward_split(const agx_lstm_desc *desc, const float *x, const float *h0, const float *c0, int64_t B,
                            int64_t T, const float *y, const void *saved, const float *gy, const float *gh_n,
                            const float *gc_n, float *gx, float *gh0, float *gc0, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_LSTM_H */
