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

#ifdef __cplusplus
}
#endif

#endif /* AGX_SIMBA_H */
