/* SimBa encoders (agilerl/modules/simba.py, create_simba in
 * agilerl/utils/evolvable_networks.py:647-710, SimbaResidualBlock in
 * agilerl/modules/custom_components.py:224-261):
 *
 *   h0 = Linear(in -> H)(x)
 *   h_i = h_{i-1} + Linear(scale*H -> H)(relu(Linear(H -> scale*H)(LayerNorm(h_{i-1}))))
 *   out = act(Linear(H -> out)(LayerNorm(h_blocks)))
 *
 * forward and backward in blocks + 2 launches each, fp32 on
 * v_mfma_f32_16x16x4_f32.  A residual block is one launch: the [B][scale*H]
 * activation lives in LDS a chunk at a time and never reaches memory; the
 * backward recomputes it from the block's saved input and per-row LayerNorm
 * statistics.  No floating-point atomics: every sum has a fixed order.
 *
 * Replaces EvolvableSimBa.forward's self.model(x) and autograd's backward
 * through it; binding: agilerl_amd/modules/simba.py. */
#ifndef AGX_SIMBA_H
#define AGX_SIMBA_H

#include "agx.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AGX_SIMBA_MAX_BLOCKS 8
#define AGX_SIMBA_MAX_ROWS 1024
#define AGX_SIMBA_MAX_WIDTH 512   /* in, H and out */
#define AGX_SIMBA_MAX_INNER 2048  /* scale * H */

#define AGX_SIMBA_ACT_NONE 0
#define AGX_SIMBA_ACT_RELU 1

/* One residual block, nn.Linear / nn.LayerNorm layouts: ln_* [H],
 * w1 [scale*H][H], b1 [scale*H], w2 [H][scale*H], b2 [H]; g_*: the
 * backward's outputs of the same shapes (forward: unused). */
typedef struct agx_simba_block {
    const float *ln_g, *ln_b, *w1, *b1, *w2, *b2;
    float *g_ln_g, *g_ln_b, *g_w1, *g_b1, *g_w2, *g_b2;
} agx_simba_block;

/* The encoder.  w_in [H][in], b_in [H]; ln_g / ln_b [H]: the output
 * LayerNorm; w_out [out][H], b_out [out].  acts [blocks + 1][B][H]: h_0 ..
 * h_blocks, and stats [blocks + 1][B][2]: (mean, rstd) of each row under
 * block i's LayerNorm (i < blocks) and under the output LayerNorm (i ==
 * blocks); out [B][out].  The forward writes acts, stats and out; the
 * backward reads them. */
typedef struct agx_simba_desc {
    const float *w_in, *b_in, *ln_g, *ln_b, *w_out, *b_out;
    float *g_w_in, *g_b_in, *g_ln_g, *g_ln_b, *g_w_out, *g_b_out;
    agx_simba_block blk[AGX_SIMBA_MAX_BLOCKS];
    float *acts, *stats, *out;
    int32_t in, H, scale, blocks, out_dim, act;
    float eps;
} agx_simba_desc;

/* x [B][in], 1 <= B <= 1024. */
int agx_simba_forward(const agx_simba_desc *desc, const float *x, int64_t B, void *stream);

/* Bytes of device workspace agx_simba_backward needs (two [B][H] gradient
 * buffers and the per-row-tile LayerNorm affine partial sums). */
size_t agx_simba_workspace_bytes(const agx_simba_desc *desc, int64_t B);

/* grad_out [B][out]; grad_x [B][in] (NULL: not needed).  Writes every g_*
 * of the descriptor, each element once. */
int agx_simba_backward(const agx_simba_desc *desc, const float *x, int64_t B, const float *grad_out, float *grad_x,
                       void *workspace, void *stream);

/* ---- split plans: wide encoders and large batches --------------------------
 * The kernels above split a block's work by 16-row tiles only.  A plan
 * (slices S, row_tiles R, w_parts Q) splits it further; (1, 1, 1) is exactly
 * the kernels above and their bits.
 *   S, 1..16 and at most ceil(scale*H / 16): the 16-unit tiles of the inner
 *      dimension are dealt to S slices in order, the extra tiles to the
 *      first slices.  The block forward and the backward's dx role run on a
 *      (row groups x S) grid, each workgroup walking its slice only.
 *   R, 1, 2 or 4: row tiles a workgroup stages; every weight operand it loads
 *      feeds R MFMA accumulators.  Bounded by LDS (160 KB): the forward
 *      stages [16R][H+4] + [16R][132] floats, the backward two [16R][H+4].
 *   Q, 1..4 and at most ceil(B / 16): the row tiles are dealt to Q workgroups
 *      per 32 inner units in the backward's dW role.
 * Partial tiles go to the workspace; the workgroup of a row group (of a unit
 * range) that arrives last, by a ticket from an integer counter, sums them
 * in slice (range) order and finishes the output, so the bits do not depend
 * on the arrival order.  No workgroup waits for another and there are no
 * floating-point atomics.  The counters are the first
 * AGX_SIMBA_COUNTER_BYTES of the workspace: zero on entry, zero on return. */
#define AGX_SIMBA_MAX_SLICES 16
#define AGX_SIMBA_MAX_W_PARTS 4
#define AGX_SIMBA_COUNTER_BYTES 1024

typedef struct agx_simba_plan {
    int32_t slices, row_tiles, w_parts;
} agx_simba_plan;

/* Host only: the plan the library would run at this shape (from the sweep of
 * tools/simba_time.py; (1, 1, 1) for B <= 256 and scale*H*H <= 4*224*224).
 * Reads desc->H and desc->scale only. */
int agx_simba_choose_plan(const agx_simba_desc *desc, int64_t B, agx_simba_plan *plan);

/* Bytes of workspace of the split entry points, I = scale*H, or 0 for a plan
 * outside the limits (agx_last_error says why):
 *   AGX_SIMBA_COUNTER_BYTES + 4 * ((S > 1 ? S*B*H : 0)
 *     + (backward ? 2*B*H + 4*ceil(B/16)*H + (Q > 1 ? Q*(2*I*H + I) : 0) : 0))
 * Reads desc->H and desc->scale only. */
size_t agx_simba_split_workspace_bytes(const agx_simba_desc *desc, int64_t B, const agx_simba_plan *plan,
                                       int backward);

/* agx_simba_forward / agx_simba_backward under a plan.  The plan is checked
 * before anything else and before any HIP call. */
int agx_simba_forward_split(const agx_simba_desc *desc, const float *x, int64_t B, const agx_simba_plan *plan,
                            void *workspace, void *stream);
int agx_simba_backward_split(const agx_simba_desc *desc, const float *x, int64_t B, const float *grad_out,
                             float *grad_x, const agx_simba_plan *plan, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* AGX_SIMBA_H */
