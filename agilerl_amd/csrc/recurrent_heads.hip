// The heads of recurrent PPO's BPTT learner (include/agx_recurrent_heads.h):
// the output Linear, the MLP head and the action distribution of both networks
// over the padded rows of a minibatch, forward (optionally saving) and
// backward.  8 waves per workgroup, fp32 MFMA, no atomics, fixed-order sums.
//
// Forward, grid (ceil(R / 16), 2): workgroup (x, y) takes rows 16 x .. 16 x +
// 15 of h_top of the actor (y = 0) or the critic (y = 1).  LDS: three slots of
// 16 rows, each as wide as the launch's widest tile (row stride: 16-rounded
// width + 4).  Slot 2 takes the h_top tile; slots 0 / 1 carry the latent and
// the head activations in turn through recurrent_dense.h's `dense` (bias, then
// k ascending) and `row_pass`, the forward of the fused policy step.  The
// saving form copies each tile a later layer's gradient needs to `saved` when
// it is whole: the latent, every hidden layer's output, the pre-LayerNorm
// output of LayerNorm layers, and the actor's masked logits (or means).  The
// epilogue is 16 lanes per row, entries a and a + 16 per lane; the
// multi-categorical and Bernoulli heads take 32 lanes per row over all 8 waves,
// one logit per lane, with per-component segmented scans (seg_scan.h), in the
// forward and in the backward's logit gradient alike.
//
// Backward rows, the same grid, two LDS slots.  The gradient of the last
// layer's output is formed in registers from the saved logits (softmax and the
// entropy's derivative) or means and written as a 16-row tile G.  Per layer,
// last to first: the row pass turns dA into dZ in place (the ReLU mask from the
// saved output, the LayerNorm backward with the row statistics recomputed from
// the saved pre-norm output in the forward's order; dY and x-hat go to the
// workspace for the affine's column sums), dZ goes to the workspace, and
// dX = dZ W is one 16 x 16 tile per wave and pass with W read down its columns
// in its stored [out][in] layout (64 contiguous bytes per k across a tile's 16
// lanes, four 16-deep steps' operands ahead of their MFMAs), into the other
// slot.  The walk ends with the output activation's backward on the latent and
// dh_top = dZ_out W_out, written to global memory.
//
// Backward params, grid ceil(jobs / 8): one wave per job.  A job is a 16 x 16
// tile of [dW_l | db_l] of one layer of either network, summed over all R rows
// in ascending 64-row batches by MFMA (A: dZ_l transposed, B: the layer's
// saved input, or 1 for the bias tile), or 64 columns of a LayerNorm's affine
// gradients, or log_std's gradient: column sums over rows ascending.  No sum
// is split across waves.
//
// The shared-encoder forms (agx_recurrent_heads_*_shared) run the forward and the backward rows on a grid of
// (ceil(R / 16), 1): one workgroup takes both heads off one latent tile and back to it (the kernels' own comments),
// and the parameter pass has one output Linear in its job list.
#include "../../include/agx_recurrent_heads.h"

#include "agx_common.h"
#include "bern_head.h"
#include "gauss_head.h"
#include "lstm_gates.h"
#include "multi_head_check.h"
#include "recurrent_dense.h"
#include "seg_scan.h"

namespace agx {
namespace {

constexpr int kLdsCap = 160 * 1024;
constexpr int kMaxLayers = 2 * (AGX_RECURRENT_MAX_HEAD + 1);  // the dense layers of a launch
constexpr int kMaxLn = 2 * (AGX_RECURRENT_MAX_HEAD - 1);      // its LayerNorms

// One network as the kernels read it: the descriptor's dense part and where its tensors lie in `saved` and
// in the workspace (float offsets; -1: not kept).
struct Net {
    const float *h_top, *out_w, *out_b;
    agx_recurrent_linear head[AGX_RECURRENT_MAX_HEAD];
    int H, latent, out_act, n_head;
    int64_t sv_lat;                               // [R][latent], after the activation
    int64_t sv_act[AGX_RECURRENT_MAX_HEAD - 1];   // [R][out]: hidden layer j's output
    int64_t sv_pre[AGX_RECURRENT_MAX_HEAD - 1];   // [R][out]: its pre-LayerNorm output
    int64_t sv_out;                               // [R][A]: the actor's masked logits or means
    int64_t ws_dzo;                               // [R][latent]: dZ of the output Linear
    int64_t ws_dz[AGX_RECURRENT_MAX_HEAD];        // [R][out]: dZ of head layer j
    int64_t ws_dy[AGX_RECURRENT_MAX_HEAD - 1];    // [R][out]: the gradient of a LayerNorm's output
    int64_t ws_xh[AGX_RECURRENT_MAX_HEAD - 1];    // [R][out]: its normalised input
};

struct RowArgs {
    Net net[2];
    const float *actions, *log_std;
    const uint8_t *mask;
    int R, A, box, slot;
    unsigned starts;                              // the multi head (seg_scan.h)
    float *log_prob, *entropy, *value;            // forward
    float *saved;                                 // forward: written (or null); backward: read
    float *ws;                                    // backward
    const float *g_lp, *g_ent, *g_val;
    float *dh_top[2];
};

__device__ __forceinline__ int r16(int v) { return (v + 15) & ~15; }

// rows b0 .. b0 + 15 (below R) and the first F columns of the tile Y [16][ld] -> dst [R][F]
__device__ __forceinline__ void store_rows(const float *Y, int ld, int F, float *dst, int R, int b0) {
    const int rr = threadIdx.x >> 5, cc = threadIdx.x & 31;
    if (b0 + rr >= R) return;
    float *d = dst + (int64_t)(b0 + rr) * F;
    for (int k = cc; k < F; k += 32) d[k] = Y[rr * ld + k];
}

// acc[row][col] += sum_k arow[k] * wcol[k * ldw], k < K ascending: lstm.hip's chain_col for any K.  arow: this
// lane's row of an LDS tile that is finite up to the 16-rounded K; wcol: this lane's column of W [K][ldw].
__device__ __forceinline__ f32x4 chain_colk(int K, int q, f32x4 acc, const float *arow, const float *wcol, int ldw) {
    const int K16 = r16(K);
#pragma unroll 1
    for (int kc = 0; kc < K; kc += 64) {
        f32x4 a[4];
        float w[16];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int k = kc + 16 * s + 4 * q;
            a[s] = *reinterpret_cast<const f32x4 *>(arow + min(k, K16 - 4));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = wcol[(int64_t)min(k + j, K - 1) * ldw];
                w[4 * s + j] = k + j < K ? v : 0.f;
            }
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (kc + 16 * s < K) {
#pragma unroll
                for (int j = 0; j < 4; ++j) acc = MFMA(a[s][j], w[4 * s + j], acc);
            }
    }
    return acc;
}

// one 16 x 16 tile of Y = G W, this wave's
__device__ __forceinline__ void dense_t_tile(int tile, const float *G, int ldg, int F, const float *W, int K, float *Y,
                                             int ldy) {
    const int lane = threadIdx.x & 63, r = lane & 15, q = lane >> 4;
    const int col = tile * 16 + r;
    const f32x4 acc = chain_colk(F, q, f32x4{0.f, 0.f, 0.f, 0.f}, G + r * ldg, W + min(col, K - 1), K);
#pragma unroll
    for (int i = 0; i < 4; ++i) Y[(4 * q + i) * ldy + col] = col < K ? acc[i] : 0.f;
}

// Y [16][ldy] = G [16][ldg] W over the 16-rounded width of K, W [F][K]; zeros in the columns past K
__device__ __forceinline__ void dense_t(const float *G, int ldg, int F, const float *W, int K, float *Y, int ldy) {
    const int wave = threadIdx.x >> 6;
    for (int tile = wave; tile < ((K + 15) >> 4); tile += kRW) dense_t_tile(tile, G, ldg, F, W, K, Y, ldy);
}

// One head's place in the shared-encoder kernels' walk: the tile at hand and its row stride
struct Walk {
    float *G;
    int ld;
};

// ---------------------------------------------------------------------------
// forward

// log-softmax, entropy and the log-prob of the given action over the 16 rows of logits Y [16][ld]
__device__ __forceinline__ void categorical_rows(const RowArgs &a, const float *Y, int ld, int b0, float *keep) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave >= 4) return;
    const int sub = lane & 15, rl = 4 * wave + (lane >> 4);
    const int A = a.A, row = b0 + rl;
    const bool live = row < a.R;
    const int a0 = sub, a1 = sub + 16;
    float lg0 = a0 < A ? Y[rl * ld + a0] : -3.0e38f;
    float lg1 = a1 < A ? Y[rl * ld + a1] : -3.0e38f;
    if (a.mask && live) {
        const uint8_t *m = a.mask + (size_t)row * A;
        if (a0 < A && !m[a0]) lg0 = -1.0e8f;
        if (a1 < A && !m[a1]) lg1 = -1.0e8f;
    }
    if (keep && live) {
        if (a0 < A) keep[(int64_t)row * A + a0] = lg0;
        if (a1 < A) keep[(int64_t)row * A + a1] = lg1;
    }
    const float mx = row_max(fmaxf(lg0, lg1));
    const float lse = mx + logf(row_sum((a0 < A ? expf(lg0 - mx) : 0.f) + (a1 < A ? expf(lg1 - mx) : 0.f)));
    const float p0 = a0 < A ? expf(lg0 - lse) : 0.f, p1 = a1 < A ? expf(lg1 - lse) : 0.f;
    const float H = -row_sum((a0 < A ? p0 * logf(p0 + 1e-8f) : 0.f) + (a1 < A ? p1 * logf(p1 + 1e-8f) : 0.f));
    const int act = live ? min(max((int)a.actions[row], 0), A - 1) : 0;
    const int srcl = (lane & ~15) + (act & 15);
    const float c0 = bperm(srcl, lg0), c1 = bperm(srcl, lg1);
    if (live && sub == 0) {
        a.entropy[row] = H;
        a.log_prob[row] = (act < 16 ? c0 : c1) - lse;
    }
}

// the Gaussian log-prob of the given action and the entropy over the 16 rows of means Y [16][ld]
__device__ __forceinline__ void gauss_rows(const RowArgs &a, const float *Y, int ld, int b0, float *keep) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave >= 4) return;
    const int sub = lane & 15, rl = 4 * wave + (lane >> 4);
    const int A = a.A, row = b0 + rl;
    const bool live = row < a.R;
    const int d0 = sub, d1 = sub + 16;
    const bool on0 = d0 < A, on1 = d1 < A;
    const float ls0 = on0 ? a.log_std[d0] : 0.f, ls1 = on1 ? a.log_std[d1] : 0.f;
    const float H = gauss_entropy(A, row_sum(ls0 + ls1));
    const float mu0 = on0 ? Y[rl * ld + d0] : 0.f, mu1 = on1 ? Y[rl * ld + d1] : 0.f;
    const float x0 = (on0 && live) ? a.actions[(int64_t)row * A + d0] : mu0;
    const float x1 = (on1 && live) ? a.actions[(int64_t)row * A + d1] : mu1;
    const float lp = row_sum((on0 ? gauss_logp_term(x0, mu0, ls0) : 0.f) + (on1 ? gauss_logp_term(x1, mu1, ls1) : 0.f));
    if (!live) return;
    if (keep) {
        if (on0) keep[(int64_t)row * A + d0] = mu0;
        if (on1) keep[(int64_t)row * A + d1] = mu1;
    }
    if (sub == 0) {
        a.entropy[row] = H;
        a.log_prob[row] = lp;
    }
}

// One lane's share of the K categoricals over the (masked) logit lg of lane g: the log-sum-exp of its component
// and its own probability
struct MultiLane {
    float lse, p;
};
__device__ __forceinline__ MultiLane multi_lane(const SegLane &g, float lg) {
    const float mx = seg_total(g, seg_scan_max(g, lg));
    MultiLane m;
    m.lse = mx + logf(seg_total(g, seg_scan_sum(g, g.on ? expf(lg - mx) : 0.f)));
    m.p = g.on ? expf(lg - m.lse) : 0.f;
    return m;
}
// component k's action of a live row, clamped into [0, n_k), as a flat logit index
__device__ __forceinline__ int multi_action(const RowArgs &a, const SegLane &g, int row) {
    const int act = (int)a.actions[(int64_t)row * __popc(a.starts) + g.k];
    return g.first + min(max(act, 0), g.last - g.first);
}

// the multi-categorical log-prob of the given actions and the entropy over the 16 rows of logits Y [16][ld]
__device__ __forceinline__ void multi_rows(const RowArgs &a, const float *Y, int ld, int b0, float *keep) {
    const SegLane g = seg_lane(a.starts, a.A);
    const int A = a.A, row = b0 + g.rl;
    const bool live = row < a.R;
    float lg = g.on ? Y[g.rl * ld + g.j] : -3.0e38f;
    if (a.mask && live && g.on && !a.mask[(size_t)row * A + g.j]) lg = -1.0e8f;
    if (keep && live && g.on) keep[(int64_t)row * A + g.j] = lg;
    const MultiLane m = multi_lane(g, lg);
    const float nh = seg_scan_sum(g, g.on ? m.p * logf(m.p + 1e-8f) : 0.f);
    const float H = -row32_sum(g.on && g.j == g.last ? nh : 0.f);
    const bool taken = live && g.on && g.j == multi_action(a, g, row);
    const float lp = row32_sum(taken ? lg - m.lse : 0.f);
    if (live && g.j == 0) {
        a.entropy[row] = H;
        a.log_prob[row] = lp;
    }
}

// the Bernoulli log-prob of the given bits and the entropy over the 16 rows of logits Y [16][ld]
__device__ __forceinline__ void bern_rows(const RowArgs &a, const float *Y, int ld, int b0, float *keep) {
    const SegLane g = bit_lane(a.A);
    const int A = a.A, row = b0 + g.rl;
    const bool live = row < a.R;
    float lg = g.on ? Y[g.rl * ld + g.j] : 0.f;
    if (a.mask && live && g.on && !a.mask[(size_t)row * A + g.j]) lg = -1.0e8f;
    if (keep && live && g.on) keep[(int64_t)row * A + g.j] = lg;
    const BernBit b = bern_bit(lg);
    const bool one = live && g.on && a.actions[(int64_t)row * A + g.j] != 0.f;
    const float H = -row32_sum(g.on ? bern_neg_entropy(b) : 0.f);
    const float lp = row32_sum(g.on ? (one ? b.lp : b.lq) : 0.f);
    if (live && g.j == 0) {
        a.entropy[row] = H;
        a.log_prob[row] = lp;
    }
}

// the actor's distribution over the 16 rows of its head's output Y [16][ld]
__device__ __forceinline__ void actor_rows(const RowArgs &a, const float *Y, int ld, int b0, float *keep) {
    if (a.box == AGX_RECURRENT_HEAD_BOX)
        gauss_rows(a, Y, ld, b0, keep);
    else if (a.box == AGX_RECURRENT_HEAD_MULTI)
        multi_rows(a, Y, ld, b0, keep);
    else if (a.box == AGX_RECURRENT_HEAD_BERNOULLI)
        bern_rows(a, Y, ld, b0, keep);
    else
        categorical_rows(a, Y, ld, b0, keep);
}

__device__ __forceinline__ void value_rows(const RowArgs &a, const float *Y, int ld, int b0) {
    const int row = b0 + threadIdx.x;
    if (threadIdx.x < 16 && row < a.R) a.value[row] = Y[threadIdx.x * ld];
}

template <bool SAVE>
__global__ __launch_bounds__(kRT) void heads_fwd_kernel(const RowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const bool critic = blockIdx.y != 0;
    const Net &n = a.net[critic ? 1 : 0];
    const int R = a.R, H = n.H, ldh = H + 4;
    const int b0 = blockIdx.x * 16;
    float *xs = lds + 2 * a.slot;

    lstm::stage_step(xs, ldh, n.h_top, R, 1, 0, H, H, b0);
    __syncthreads();
    int F = n.latent, side = 0;
    float *Y = lds;
    int ldY = r16(F) + 4;
    dense(xs, ldh, H, n.out_w, n.out_b, F, Y, ldY);
    __syncthreads();
    row_pass(Y, ldY, F, nullptr, nullptr, n.out_act);
    __syncthreads();
    if (SAVE) store_rows(Y, ldY, F, a.saved + n.sv_lat, R, b0);
    for (int j = 0; j < n.n_head; ++j) {
        const agx_recurrent_linear &hl = n.head[j];
        const float *X = Y;
        const int ldX = ldY;
        side ^= 1;
        Y = lds + side * a.slot;
        F = hl.out;
        ldY = r16(F) + 4;
        dense(X, ldX, hl.in, hl.w, hl.b, F, Y, ldY);
        __syncthreads();
        if (SAVE && hl.ln_w) {
            store_rows(Y, ldY, F, a.saved + n.sv_pre[j], R, b0);
            __syncthreads();  // the row pass works in place
        }
        row_pass(Y, ldY, F, hl.ln_w, hl.ln_b, hl.relu ? AGX_RECURRENT_ACT_RELU : AGX_RECURRENT_ACT_NONE);
        __syncthreads();
        if (SAVE && j < n.n_head - 1) store_rows(Y, ldY, F, a.saved + n.sv_act[j], R, b0);
    }
    if (critic)
        value_rows(a, Y, ldY, b0);
    else
        actor_rows(a, Y, ldY, b0, SAVE ? a.saved + n.sv_out : nullptr);
}

// The shared-encoder forward (agx_recurrent_heads_forward_shared), grid (ceil(R / 16), 1): net[0]'s output Linear
// once per row tile, then both heads off the one latent tile.  Four LDS slots: the h_top tile in slot 2, the latent
// in slot 0, the actor's head on between slots 1 and 0 as above, the critic's between slots 2 and 3 (h_top is dead
// once the latent is whole).  Depth j of both heads is one tile list over the 8 waves (dense_pair) and one row
// pass (actor: waves 0 .. 3, critic: 4 .. 7); the actor's depth 1 overwrites the latent after the barrier that ends
// depth 0, where the critic has read it and the saving form has stored it.
template <bool SAVE>
__global__ __launch_bounds__(kRT) void heads_fwd_shared_kernel(const RowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Net &na = a.net[0], &nc = a.net[1];
    const int R = a.R, H = na.H, ldh = H + 4;
    const int b0 = blockIdx.x * 16;
    float *xs = lds + 2 * a.slot;

    lstm::stage_step(xs, ldh, na.h_top, R, 1, 0, H, H, b0);
    __syncthreads();
    const int ldl = r16(na.latent) + 4;
    dense(xs, ldh, H, na.out_w, na.out_b, na.latent, lds, ldl);
    __syncthreads();
    row_pass(lds, ldl, na.latent, nullptr, nullptr, na.out_act);
    __syncthreads();
    if (SAVE) store_rows(lds, ldl, na.latent, a.saved + na.sv_lat, R, b0);
    DenseSide sa{nullptr, lds, 0, ldl, true}, sc{nullptr, lds, 0, ldl, true};
    for (int j = 0; j < (na.n_head > nc.n_head ? na.n_head : nc.n_head); ++j) {
        const agx_recurrent_linear &la = na.head[min(j, na.n_head - 1)], &lc = nc.head[min(j, nc.n_head - 1)];
        sa.on = j < na.n_head;
        sc.on = j < nc.n_head;
        if (sa.on) sa.advance(lds + ((j + 1) & 1) * a.slot, la.out);
        if (sc.on) sc.advance(lds + (2 + (j & 1)) * a.slot, lc.out);
        dense_pair(la, sa, lc, sc);
        __syncthreads();
        const bool pa = SAVE && sa.on && la.ln_w, pc = SAVE && sc.on && lc.ln_w;
        if (pa) store_rows(sa.Y, sa.ldy, la.out, a.saved + na.sv_pre[j], R, b0);
        if (pc) store_rows(sc.Y, sc.ldy, lc.out, a.saved + nc.sv_pre[j], R, b0);
        if (pa || pc) __syncthreads();  // the row pass works in place
        row_pass_pair(la, sa, lc, sc);
        __syncthreads();
        if (SAVE && j < na.n_head - 1) store_rows(sa.Y, sa.ldy, la.out, a.saved + na.sv_act[j], R, b0);
        if (SAVE && j < nc.n_head - 1) store_rows(sc.Y, sc.ldy, lc.out, a.saved + nc.sv_act[j], R, b0);
    }
    value_rows(a, sc.Y, sc.ldy, b0);
    actor_rows(a, sa.Y, sa.ldy, b0, SAVE ? a.saved + na.sv_out : nullptr);
}

// ---------------------------------------------------------------------------
// backward, rows

// G [16][ld] = the gradient of the actor's logits (or means) and of the critic's value, zeros past the width
__device__ __forceinline__ void head_grad_rows(const RowArgs &a, const Net &n, bool critic, float *G, int ld, int b0) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave >= 4) return;
    const int sub = lane & 15, rl = 4 * wave + (lane >> 4);
    const int A = a.A, row = b0 + rl;
    const bool live = row < a.R;
    float *g = G + rl * ld;
    if (critic) {
        g[sub] = (live && sub == 0) ? a.g_val[row] : 0.f;
        return;
    }
    const int a0 = sub, a1 = sub + 16;
    const bool on0 = live && a0 < A, on1 = live && a1 < A;
    const float gl = live ? a.g_lp[row] : 0.f, ge = live ? a.g_ent[row] : 0.f;
    const float *kept = a.saved + n.sv_out + (int64_t)(live ? row : 0) * A;
    float v0 = 0.f, v1 = 0.f;
    if (a.box) {
        const float *x = a.actions + (int64_t)(live ? row : 0) * A;
        if (on0) v0 = gauss_g_mean(gl, x[a0] - kept[a0], gauss_inv_var(a.log_std[a0]));
        if (on1) v1 = gauss_g_mean(gl, x[a1] - kept[a1], gauss_inv_var(a.log_std[a1]));
    } else {
        // log_prob = lg[act] - lse: d / d lg_j = [j == act] - p_j.  H = -sum p log(p + eps): with t_k = dH / dp_k =
        // -(log(p_k + eps) + p_k / (p_k + eps)), dH / d lg_j = p_j (t_j - sum_k p_k t_k).  Masked entries get none.
        const float lg0 = on0 ? kept[a0] : (a0 < A ? 0.f : -3.0e38f), lg1 = on1 ? kept[a1] : (a1 < A ? 0.f : -3.0e38f);
        const float mx = row_max(fmaxf(lg0, lg1));
        const float lse = mx + logf(row_sum((a0 < A ? expf(lg0 - mx) : 0.f) + (a1 < A ? expf(lg1 - mx) : 0.f)));
        const float p0 = a0 < A ? expf(lg0 - lse) : 0.f, p1 = a1 < A ? expf(lg1 - lse) : 0.f;
        const float t0 = -(logf(p0 + 1e-8f) + p0 / (p0 + 1e-8f)), t1 = -(logf(p1 + 1e-8f) + p1 / (p1 + 1e-8f));
        const float pt = row_sum((a0 < A ? p0 * t0 : 0.f) + (a1 < A ? p1 * t1 : 0.f));
        const int act = live ? min(max((int)a.actions[row], 0), A - 1) : 0;
        v0 = gl * ((a0 == act ? 1.f : 0.f) - p0) + ge * (p0 * (t0 - pt));
        v1 = gl * ((a1 == act ? 1.f : 0.f) - p1) + ge * (p1 * (t1 - pt));
        if (a.mask && live) {
            const uint8_t *m = a.mask + (size_t)row * A;
            if (a0 < A && !m[a0]) v0 = 0.f;
            if (a1 < A && !m[a1]) v1 = 0.f;
        }
    }
    g[a0] = on0 ? v0 : 0.f;
    if (A > 16) g[a1] = on1 ? v1 : 0.f;
}

// head_grad_rows for the actor's multi-categorical and Bernoulli heads, 32 lanes per row.  With gl / ge the row's
// upstream gradients of log_prob / entropy: multi gl ([j == off_k + a_k] - p_j) + ge p_j (t_j - sum_{i in k} p_i t_i),
// t = -(log(p + eps) + p / (p + eps)), the inner sum one more segmented scan; Bernoulli gl (a_j - p_j) + ge dH / dl_j
// (bern_head.h).  A masked logit gets exactly 0.
__device__ __forceinline__ void head_grad_rows32(const RowArgs &a, const Net &n, float *G, int ld, int b0) {
    const bool multi = a.box == AGX_RECURRENT_HEAD_MULTI;
    const SegLane g = multi ? seg_lane(a.starts, a.A) : bit_lane(a.A);
    const int A = a.A, row = b0 + g.rl;
    const bool live = row < a.R, on = live && g.on;
    const float gl = live ? a.g_lp[row] : 0.f, ge = live ? a.g_ent[row] : 0.f;
    const float lg = on ? a.saved[n.sv_out + (int64_t)row * A + g.j] : (g.on ? 0.f : -3.0e38f);
    float v;
    if (multi) {
        const MultiLane m = multi_lane(g, lg);
        const float t = -(logf(m.p + 1e-8f) + m.p / (m.p + 1e-8f));
        const float pt = seg_total(g, seg_scan_sum(g, g.on ? m.p * t : 0.f));
        const bool taken = on && g.j == multi_action(a, g, row);
        v = gl * ((taken ? 1.f : 0.f) - m.p) + ge * (m.p * (t - pt));
    } else {
        const BernBit b = bern_bit(g.on ? lg : 0.f);
        v = gl * bern_dlogp(b, on && a.actions[(int64_t)row * A + g.j] != 0.f) + ge * bern_dH(b);
    }
    if (a.mask && on && !a.mask[(size_t)row * A + g.j]) v = 0.f;
    if (g.j < r16(A)) G[g.rl * ld + g.j] = on ? v : 0.f;
}

// dA -> dZ of hidden head layer j over the rows of G [16][ld] in place: the ReLU mask from the layer's saved output,
// then the LayerNorm backward (16 lanes per row; the row statistics as row_pass takes them), on waves w0 .. w0 + 3
__device__ __forceinline__ void hidden_grad_rows(const RowArgs &a, const Net &n, int j, float *G, int ld, int b0,
                                                 int w0 = 0) {
    const int wave = (int)(threadIdx.x >> 6) - w0, lane = threadIdx.x & 63;
    if (wave < 0 || wave >= 4) return;
    const agx_recurrent_linear &hl = n.head[j];
    const int sub = lane & 15, rl = 4 * wave + (lane >> 4);
    const int F = hl.out, F16 = r16(F), row = b0 + rl;
    const bool live = row < a.R;
    const int64_t o = (int64_t)(live ? row : 0) * F;
    const float *out = a.saved + n.sv_act[j] + o;
    float *g = G + rl * ld;
    if (!hl.ln_w) {
        if (hl.relu)
            for (int k = sub; k < F; k += 16) g[k] = (live && out[k] > 0.f) ? g[k] : 0.f;
        return;
    }
    const float *pre = a.saved + n.sv_pre[j] + o;
    float *dy_out = a.ws + n.ws_dy[j] + o, *xh_out = a.ws + n.ws_xh[j] + o;
    const float inv = 1.f / (float)F;
    float s = 0.f;
    for (int k = sub; k < F16; k += 16) s = (k < F && live) ? s + pre[k] : s;
    const float mean = row_sum(s) * inv;
    float vs = 0.f;
    for (int k = sub; k < F16; k += 16) {
        const float d = ((k < F && live) ? pre[k] : 0.f) - mean;
        vs = k < F ? vs + d * d : vs;
    }
    const float rstd = 1.f / sqrtf(row_sum(vs) / (float)F + 1e-5f);
    float s1 = 0.f, s2 = 0.f;
    for (int k = sub; k < F16; k += 16) {
        if (k < F && live) {
            const float xh = (pre[k] - mean) * rstd;
            const float dy = (!hl.relu || out[k] > 0.f) ? g[k] : 0.f;
            const float dxh = dy * hl.ln_w[k];
            dy_out[k] = dy;
            xh_out[k] = xh;
            s1 += dxh;
            s2 += dxh * xh;
        }
    }
    s1 = row_sum(s1) * inv;
    s2 = row_sum(s2) * inv;
    for (int k = sub; k < F; k += 16) {
        float dz = 0.f;
        if (live) {
            const float xh = (pre[k] - mean) * rstd;
            const float dy = (!hl.relu || out[k] > 0.f) ? g[k] : 0.f;
            dz = rstd * (dy * hl.ln_w[k] - s1 - xh * s2);
        }
        g[k] = dz;
    }
}

__global__ __launch_bounds__(kRT) void heads_bwd_rows_kernel(const RowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const bool critic = blockIdx.y != 0;
    const Net &n = a.net[critic ? 1 : 0];
    const int R = a.R, H = n.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * 16;
    int side = 0;
    float *G = lds;
    int F = n.head[n.n_head - 1].out, ldG = r16(F) + 4;
    if (!critic && a.box >= AGX_RECURRENT_HEAD_MULTI)
        head_grad_rows32(a, n, G, ldG, b0);
    else
        head_grad_rows(a, n, critic, G, ldG, b0);
    __syncthreads();
    for (int j = n.n_head - 1; j >= 0; --j) {
        const agx_recurrent_linear &hl = n.head[j];
        if (j < n.n_head - 1) {
            hidden_grad_rows(a, n, j, G, ldG, b0);
            __syncthreads();
        }
        store_rows(G, ldG, F, a.ws + n.ws_dz[j], R, b0);
        side ^= 1;
        float *X = lds + side * a.slot;
        const int ldX = r16(hl.in) + 4;
        dense_t(G, ldG, F, hl.w, hl.in, X, ldX);
        __syncthreads();
        G = X;
        ldG = ldX;
        F = hl.in;
    }
    // the latent's activation, then the output Linear
    if (wave < 4 && n.out_act != AGX_RECURRENT_ACT_NONE) {
        const int rl = 4 * wave + q, row = b0 + rl;
        const float *lat = a.saved + n.sv_lat + (int64_t)(row < R ? row : 0) * F;
        for (int k = r; k < F; k += 16) {
            const float y = row < R ? lat[k] : 0.f, g = G[rl * ldG + k];
            G[rl * ldG + k] = n.out_act == AGX_RECURRENT_ACT_RELU ? (y > 0.f ? g : 0.f) : g * (1.f - y * y);
        }
    }
    __syncthreads();
    store_rows(G, ldG, F, a.ws + n.ws_dzo, R, b0);
    float *dh = a.dh_top[critic ? 1 : 0];
    for (int tile = wave; tile < (H >> 4); tile += kRW) {
        const int col = tile * 16 + r;
        const f32x4 acc = chain_colk(F, q, f32x4{0.f, 0.f, 0.f, 0.f}, G + r * ldG, n.out_w + col, H);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = b0 + 4 * q + i;
            if (row < R) dh[(int64_t)row * H + col] = acc[i];
        }
    }
}

// The shared-encoder backward rows (agx_recurrent_heads_backward_shared), grid (ceil(R / 16), 1): one workgroup
// walks both heads back to the latent, the actor between slots 0 and 1, the critic between slots 2 and 3.  Step t
// takes the actor's layer n_a - 1 - t and the critic's n_c - 1 - t: the two row passes side by side (waves 0 .. 3
// and 4 .. 7) and the two dX = dZ W as one tile list over the 8 waves.  A head that has reached the latent keeps
// its dX where it is.  Then dLatent = dX_actor + dX_critic, in that order, the output activation's backward once,
// one dZ_out to the workspace and one dh_top = dZ_out W_out.
__global__ __launch_bounds__(kRT) void heads_bwd_rows_shared_kernel(const RowArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const Net &na = a.net[0], &nc = a.net[1];
    const int R = a.R, H = na.H;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int b0 = blockIdx.x * 16;
    Walk wa{lds, r16(a.A) + 4}, wc{lds + 2 * a.slot, 16 + 4};
    if (a.box >= AGX_RECURRENT_HEAD_MULTI)
        head_grad_rows32(a, na, wa.G, wa.ld, b0);
    else
        head_grad_rows(a, na, false, wa.G, wa.ld, b0);
    head_grad_rows(a, nc, true, wc.G, wc.ld, b0);
    __syncthreads();
    for (int t = 0; t < (na.n_head > nc.n_head ? na.n_head : nc.n_head); ++t) {
        const int ja = na.n_head - 1 - t, jc = nc.n_head - 1 - t;
        const bool ra = ja >= 0 && t > 0, rc = jc >= 0 && t > 0;  // hidden layers: dA -> dZ first
        if (ra) hidden_grad_rows(a, na, ja, wa.G, wa.ld, b0);
        if (rc) hidden_grad_rows(a, nc, jc, wc.G, wc.ld, b0, 4);
        if (ra || rc) __syncthreads();
        const bool oa = ja >= 0, oc = jc >= 0;
        const agx_recurrent_linear &la = na.head[max(ja, 0)], &lc = nc.head[max(jc, 0)];
        if (oa) store_rows(wa.G, wa.ld, la.out, a.ws + na.ws_dz[ja], R, b0);
        if (oc) store_rows(wc.G, wc.ld, lc.out, a.ws + nc.ws_dz[jc], R, b0);
        float *Xa = lds + ((t + 1) & 1) * a.slot, *Xc = lds + (2 + ((t + 1) & 1)) * a.slot;
        const int ta = oa ? (la.in + 15) >> 4 : 0, tc = oc ? (lc.in + 15) >> 4 : 0;
        for (int tile = wave; tile < ta + tc; tile += kRW) {
            if (tile < ta)
                dense_t_tile(tile, wa.G, wa.ld, la.out, la.w, la.in, Xa, r16(la.in) + 4);
            else
                dense_t_tile(tile - ta, wc.G, wc.ld, lc.out, lc.w, lc.in, Xc, r16(lc.in) + 4);
        }
        __syncthreads();
        if (oa) wa = Walk{Xa, r16(la.in) + 4};
        if (oc) wc = Walk{Xc, r16(lc.in) + 4};
    }
    // dLatent, the latent's activation, then the output Linear
    const int F = na.latent;
    float *G = wa.G;
    const int ldG = wa.ld;
    if (wave < 4) {
        const int rl = 4 * wave + q, row = b0 + rl;
        const float *lat = a.saved + na.sv_lat + (int64_t)(row < R ? row : 0) * F;
        for (int k = r; k < F; k += 16) {
            const float g = G[rl * ldG + k] + wc.G[rl * wc.ld + k];
            float dz = g;
            if (na.out_act != AGX_RECURRENT_ACT_NONE) {
                const float y = row < R ? lat[k] : 0.f;
                dz = na.out_act == AGX_RECURRENT_ACT_RELU ? (y > 0.f ? g : 0.f) : g * (1.f - y * y);
            }
            G[rl * ldG + k] = dz;
        }
    }
    __syncthreads();
    store_rows(G, ldG, F, a.ws + na.ws_dzo, R, b0);
    for (int tile = wave; tile < (H >> 4); tile += kRW) {
        const int col = tile * 16 + r;
        const f32x4 acc = chain_colk(F, q, f32x4{0.f, 0.f, 0.f, 0.f}, G + r * ldG, na.out_w + col, H);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int row = b0 + 4 * q + i;
            if (row < R) a.dh_top[0][(int64_t)row * H + col] = acc[i];
        }
    }
}

// ---------------------------------------------------------------------------
// backward, parameters

struct ParamLayer {
    const float *dZ, *X;  // [R][out], the layer's input [R][in]
    float *gw, *gb;       // [out][in], [out]
    int in, out, job0, ct;  // its first job; ct = ceil(in / 16) + 1 column tiles, the last one the bias
};

struct ColJob {
    const float *dy, *xh;  // [R][F]
    float *gw, *gb;        // [F]
    int F, job0;
};

struct ParamArgs {
    ParamLayer layer[kMaxLayers];
    ColJob ln[kMaxLn];
    int n_layers, n_ln, n_jobs, ls_job;  // ls_job: log_std's job, or -1
    int R, A;
    const float *means, *actions, *log_std, *g_lp, *g_ent;
    float *g_log_std;
};

__global__ __launch_bounds__(kRT) void heads_bwd_params_kernel(const ParamArgs a) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int job = blockIdx.x * kRW + wave;
    const int R = a.R;
    if (job >= a.n_jobs) return;
    if (job == a.ls_job) {  // d log_std: lane d sums its column over the rows
        if (lane < a.A) {
            const float iv = gauss_inv_var(a.log_std[lane]);
            float s = 0.f;
            for (int n = 0; n < R; ++n) {
                const int64_t o = (int64_t)n * a.A + lane;
                s += gauss_g_log_std(a.g_lp[n], a.actions[o] - a.means[o], iv) + a.g_ent[n];
            }
            a.g_log_std[lane] = s;
        }
        return;
    }
    if (a.n_ln > 0 && job >= a.ln[0].job0) {  // a LayerNorm's affine: lane = column
        int c = 0;
        while (c + 1 < a.n_ln && job >= a.ln[c + 1].job0) ++c;
        const ColJob &cj = a.ln[c];
        const int col = (job - cj.job0) * 64 + lane;
        if (col < cj.F) {
            float sw = 0.f, sb = 0.f;
            for (int n = 0; n < R; ++n) {
                const float dy = cj.dy[(int64_t)n * cj.F + col];
                sw += dy * cj.xh[(int64_t)n * cj.F + col];
                sb += dy;
            }
            cj.gw[col] = sw;
            cj.gb[col] = sb;
        }
        return;
    }
    int li = 0;
    while (li + 1 < a.n_layers && job >= a.layer[li + 1].job0) ++li;
    const ParamLayer &p = a.layer[li];
    const int t = job - p.job0, jt = t / p.ct, ctile = t - jt * p.ct;
    const bool bias = ctile == p.ct - 1;
    const int j0 = jt * 16, col = ctile * 16 + r;
    const float *gcol = p.dZ + min(j0 + r, p.out - 1);
    const float *xcol = p.X + min(col, p.in - 1);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int n0 = 0; n0 < R; n0 += 64) {
        float g[16], w[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int n = n0 + 16 * (u >> 2) + 4 * q + (u & 3);
            const bool ok = n < R;
            const int64_t nn = ok ? n : R - 1;
            const float gv = gcol[nn * p.out];
            g[u] = ok ? gv : 0.f;
            w[u] = bias ? 1.f : xcol[nn * p.in];
        }
#pragma unroll
        for (int u = 0; u < 16; ++u)
            if (n0 + 16 * (u >> 2) < R) acc = MFMA(g[u], w[u], acc);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = j0 + 4 * q + i;
        if (j >= p.out) continue;
        if (bias) {
            if (r == 0) p.gb[j] = acc[i];
        } else if (col < p.in) {
            p.gw[(int64_t)j * p.in + col] = acc[i];
        }
    }
}

// ---------------------------------------------------------------------------
// host

// the head of n over a latent of `width` floats
int check_head(const agx_recurrent_net &n, int width, int out, const char *name, const char *who) {
    AGX_REQUIRE(n.n_head >= 2 && n.n_head <= AGX_RECURRENT_MAX_HEAD, "%s: %s: %d head layers outside [2, %d]", who,
                name, n.n_head, AGX_RECURRENT_MAX_HEAD);
    for (int j = 0; j < n.n_head; ++j) {
        const agx_recurrent_linear &h = n.head[j];
        const bool last = j == n.n_head - 1;
        AGX_REQUIRE(h.w && h.b && !h.ln_w == !h.ln_b, "%s: %s: head layer %d: NULL parameter", who, name, j);
        AGX_REQUIRE(h.in == width && h.out >= 1 && h.out <= AGX_PPO_GRAPH_MAX_WIDTH,
                    "%s: %s: head layer %d: %d -> %d after width %d", who, name, j, h.in, h.out, width);
        AGX_REQUIRE(!last || (h.out == out && !h.ln_w && !h.relu), "%s: %s: the head must end in a plain Linear to %d",
                    who, name, out);
        width = h.out;
    }
    return AGX_OK;
}

int check_net(const agx_recurrent_net &n, int H, const float *h_top, int out, const char *name, const char *who) {
    AGX_REQUIRE(H >= 16 && H <= AGX_LSTM_MAX_HIDDEN && H % 16 == 0,
                "%s: %s: hidden size %d is not a multiple of 16 in [16, %d]", who, name, H, AGX_LSTM_MAX_HIDDEN);
    AGX_REQUIRE(h_top && n.out_w && n.out_b, "%s: %s: h_top or the output Linear is NULL", who, name);
    AGX_REQUIRE(n.latent >= 1 && n.latent <= AGX_PPO_GRAPH_MAX_WIDTH, "%s: %s: latent %d outside [1, %d]", who, name,
                n.latent, AGX_PPO_GRAPH_MAX_WIDTH);
    AGX_REQUIRE(n.out_act >= AGX_RECURRENT_ACT_NONE && n.out_act <= AGX_RECURRENT_ACT_TANH,
                "%s: %s: output activation %d", who, name, n.out_act);
    return check_head(n, n.latent, out, name, who);
}

// shared: net[1] gives its head only, over net[0]'s latent
int check_heads(const agx_recurrent_heads *heads, const char *who, bool shared) {
    AGX_REQUIRE(heads, "%s: heads is NULL", who);
    const agx_recurrent_heads &s = *heads;
    AGX_REQUIRE(s.R >= 1 && s.R <= (1 << 24), "%s: R %lld outside [1, 2^24]", who, (long long)s.R);
    AGX_REQUIRE(s.A >= 1 && s.A <= AGX_PPO_GRAPH_MAX_ACTIONS, "%s: %d actions (1..%d)", who, s.A,
                AGX_PPO_GRAPH_MAX_ACTIONS);
    AGX_REQUIRE(s.actions, "%s: actions is NULL", who);
    AGX_REQUIRE(s.box >= AGX_RECURRENT_HEAD_DISCRETE && s.box <= AGX_RECURRENT_HEAD_BERNOULLI, "%s: head kind %d", who,
                s.box);
    AGX_REQUIRE(s.box == AGX_RECURRENT_HEAD_BOX ? (s.log_std && !s.mask) : !s.log_std,
                "%s: log_std goes with Box, a mask with the other heads", who);
    if (s.box == AGX_RECURRENT_HEAD_MULTI) {
        const int L = head_width(s.multi, who);
        if (L < 0) return AGX_EINVAL;
        AGX_REQUIRE(L == s.A, "%s: nvec sums to %d, the head has %d logits", who, L, s.A);
    }
    if (int rc = check_net(s.net[0], s.H[0], s.h_top[0], s.A, "actor", who)) return rc;
    if (shared) return check_head(s.net[1], s.net[0].latent, 1, "critic", who);
    return check_net(s.net[1], s.H[1], s.h_top[1], 1, "critic", who);
}

// The networks as the kernels read them and the sizes of `saved` and of the workspace, in floats.  shared: the
// critic's Net is its head over the actor's output Linear, latent and dZ_out, which are kept once.
void plan(const agx_recurrent_heads &s, Net (&net)[2], int64_t &saved, int64_t &ws, bool shared) {
    saved = ws = 0;
    const int64_t R = s.R;
    for (int k = 0; k < 2; ++k) {
        const bool own = k == 0 || !shared;  // the network has an output Linear of its own
        const agx_recurrent_net &d = s.net[k], &e = s.net[own ? k : 0];
        Net &n = net[k];
        n.h_top = s.h_top[own ? k : 0];
        n.out_w = e.out_w;
        n.out_b = e.out_b;
        n.H = s.H[own ? k : 0];
        n.latent = e.latent;
        n.out_act = e.out_act;
        n.n_head = d.n_head;
        n.sv_lat = own ? saved : net[0].sv_lat;
        n.ws_dzo = own ? ws : net[0].ws_dzo;
        if (own) {
            saved += R * d.latent;
            ws += R * d.latent;
        }
        for (int j = 0; j < AGX_RECURRENT_MAX_HEAD; ++j) {
            const bool on = j < d.n_head;
            n.head[j] = on ? d.head[j] : agx_recurrent_linear{};
            n.ws_dz[j] = on ? ws : -1;
            if (on) ws += R * d.head[j].out;
            if (j == AGX_RECURRENT_MAX_HEAD - 1) break;
            const bool hidden = j < d.n_head - 1, ln = hidden && d.head[j].ln_w;
            n.sv_act[j] = hidden ? saved : -1;
            if (hidden) saved += R * d.head[j].out;
            n.sv_pre[j] = n.ws_dy[j] = n.ws_xh[j] = -1;
            if (ln) {
                n.sv_pre[j] = saved;
                saved += R * d.head[j].out;
                n.ws_dy[j] = ws;
                n.ws_xh[j] = ws + R * d.head[j].out;
                ws += 2 * R * d.head[j].out;
            }
        }
        n.sv_out = k == 0 ? saved : -1;
        if (k == 0) saved += R * s.A;
    }
}

int widest(const Net &n) {
    int w = n.H > n.latent ? n.H : n.latent;
    for (int j = 0; j < n.n_head; ++j) w = n.head[j].out > w ? n.head[j].out : w;
    return w;
}

RowArgs row_args(const agx_recurrent_heads &s, int64_t &saved, int64_t &ws, bool shared) {
    RowArgs a{};
    plan(s, a.net, saved, ws, shared);
    a.actions = s.actions;
    a.log_std = s.log_std;
    a.mask = s.mask;
    a.R = (int)s.R;
    a.A = s.A;
    a.box = s.box;
    a.starts = s.box == AGX_RECURRENT_HEAD_MULTI ? multi_starts(s.multi) : 0;
    const int wa = widest(a.net[0]), wc = widest(a.net[1]);
    a.slot = 16 * ((((wa > wc ? wa : wc) + 15) & ~15) + 4);
    return a;
}

void allow_lds() {
    static const bool once = [] {
        (void)hipFuncSetAttribute((const void *)heads_fwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kLdsCap);
        (void)hipFuncSetAttribute((const void *)heads_fwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kLdsCap);
        (void)hipFuncSetAttribute((const void *)heads_bwd_rows_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kLdsCap);
        (void)hipFuncSetAttribute((const void *)heads_fwd_shared_kernel<false>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap);
        (void)hipFuncSetAttribute((const void *)heads_fwd_shared_kernel<true>,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap);
        (void)hipFuncSetAttribute((const void *)heads_bwd_rows_shared_kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap);
        return true;
    }();
    (void)once;
}

size_t plan_bytes(const agx_recurrent_heads *heads, bool shared, bool workspace, const char *who) {
    if (check_heads(heads, who, shared)) return 0;
    int64_t saved, ws;
    (void)row_args(*heads, saved, ws, shared);
    return (size_t)(workspace ? ws : saved) * sizeof(float);
}

int heads_forward(const agx_recurrent_heads *heads, float *log_prob, float *entropy, float *value, void *saved,
                  void *stream, bool shared, const char *who) {
    if (int rc = check_heads(heads, who, shared)) return rc;
    AGX_REQUIRE(log_prob && entropy && value, "%s: an output is NULL", who);
    int64_t nsaved, nws;
    RowArgs a = row_args(*heads, nsaved, nws, shared);
    a.log_prob = log_prob;
    a.entropy = entropy;
    a.value = value;
    a.saved = static_cast<float *>(saved);
    allow_lds();
    const dim3 grid((unsigned)ceil_div(heads->R, 16), shared ? 1 : 2);
    // 3 slots, at most 3 * 16 * 516 * 4 = 97 KB; shared: 4 slots, at most 129 KB
    const size_t bytes = (size_t)(shared ? 4 : 3) * a.slot * sizeof(float);
    if (shared && saved)
        hipLaunchKernelGGL(heads_fwd_shared_kernel<true>, grid, dim3(kRT), bytes, as_stream(stream), a);
    else if (shared)
        hipLaunchKernelGGL(heads_fwd_shared_kernel<false>, grid, dim3(kRT), bytes, as_stream(stream), a);
    else if (saved)
        hipLaunchKernelGGL(heads_fwd_kernel<true>, grid, dim3(kRT), bytes, as_stream(stream), a);
    else
        hipLaunchKernelGGL(heads_fwd_kernel<false>, grid, dim3(kRT), bytes, as_stream(stream), a);
    return check_launch(who);
}

int heads_backward(const agx_recurrent_heads *heads, const void *saved, const agx_recurrent_heads_grads *grads,
                   void *workspace, void *stream, bool shared, const char *who) {
    if (int rc = check_heads(heads, who, shared)) return rc;
    AGX_REQUIRE(saved && grads && workspace, "%s: saved, grads or the workspace is NULL", who);
    const agx_recurrent_heads &s = *heads;
    const agx_recurrent_heads_grads &g = *grads;
    AGX_REQUIRE(g.g_log_prob && g.g_entropy && g.g_value, "%s: an upstream gradient is NULL", who);
    AGX_REQUIRE((s.box == AGX_RECURRENT_HEAD_BOX) == (g.log_std != nullptr), "%s: log_std's gradient goes with Box",
                who);
    for (int k = 0; k < 2; ++k) {
        AGX_REQUIRE((shared && k == 1) || (g.dh_top[k] && g.out_w[k] && g.out_b[k]),
                    "%s: network %d: a gradient output is NULL", who, k);
        for (int j = 0; j < s.net[k].n_head; ++j) {
            const agx_recurrent_linear_grad &o = g.head[k][j];
            AGX_REQUIRE(o.w && o.b && (!s.net[k].head[j].ln_w || (o.ln_w && o.ln_b)),
                        "%s: network %d: head layer %d: a gradient output is NULL", who, k, j);
        }
    }
    int64_t nsaved, nws;
    RowArgs a = row_args(s, nsaved, nws, shared);
    float *sv = const_cast<float *>(static_cast<const float *>(saved)), *ws = static_cast<float *>(workspace);
    a.saved = sv;
    a.ws = ws;
    a.g_lp = g.g_log_prob;
    a.g_ent = g.g_entropy;
    a.g_val = g.g_value;
    a.dh_top[0] = g.dh_top[0];
    a.dh_top[1] = shared ? nullptr : g.dh_top[1];
    allow_lds();
    const dim3 grid((unsigned)ceil_div(s.R, 16), shared ? 1 : 2);
    if (shared)
        hipLaunchKernelGGL(heads_bwd_rows_shared_kernel, grid, dim3(kRT), (size_t)4 * a.slot * sizeof(float),
                           as_stream(stream), a);
    else
        hipLaunchKernelGGL(heads_bwd_rows_kernel, grid, dim3(kRT), (size_t)2 * a.slot * sizeof(float),
                           as_stream(stream), a);
    if (int rc = check_launch(who)) return rc;

    ParamArgs p{};
    int jobs = 0;
    for (int k = 0; k < 2; ++k) {
        const Net &n = a.net[k];
        if (k == 0 || !shared) {  // shared: one output Linear, its dZ the sum of both heads' shares
            ParamLayer &o = p.layer[p.n_layers++];
            o = ParamLayer{ws + n.ws_dzo, n.h_top, g.out_w[k], g.out_b[k], n.H, n.latent, jobs, (n.H + 15) / 16 + 1};
            jobs += ((n.latent + 15) / 16) * o.ct;
        }
        for (int j = 0; j < n.n_head; ++j) {
            const agx_recurrent_linear &hl = n.head[j];
            ParamLayer &l = p.layer[p.n_layers++];
            l = ParamLayer{ws + n.ws_dz[j], sv + (j ? n.sv_act[j - 1] : n.sv_lat), g.head[k][j].w, g.head[k][j].b,
                           hl.in, hl.out, jobs, (hl.in + 15) / 16 + 1};
            jobs += ((hl.out + 15) / 16) * l.ct;
        }
    }
    for (int k = 0; k < 2; ++k) {
        const Net &n = a.net[k];
        for (int j = 0; j < n.n_head - 1; ++j)
            if (n.head[j].ln_w) {
                p.ln[p.n_ln++] = ColJob{ws + n.ws_dy[j], ws + n.ws_xh[j], g.head[k][j].ln_w, g.head[k][j].ln_b,
                                        n.head[j].out, jobs};
                jobs += (n.head[j].out + 63) / 64;
            }
    }
    p.ls_job = s.box == AGX_RECURRENT_HEAD_BOX ? jobs++ : -1;
    p.n_jobs = jobs;
    p.R = (int)s.R;
    p.A = s.A;
    p.means = sv + a.net[0].sv_out;
    p.actions = s.actions;
    p.log_std = s.log_std;
    p.g_lp = g.g_log_prob;
    p.g_ent = g.g_entropy;
    p.g_log_std = g.log_std;
    hipLaunchKernelGGL(heads_bwd_params_kernel, dim3((unsigned)ceil_div(jobs, kRW)), dim3(kRT), 0, as_stream(stream), p);
    return check_launch(who);
}

}  // namespace
}  // namespace agx

using namespace agx;

extern "C" size_t agx_recurrent_heads_saved_bytes(const agx_recurrent_heads *heads) {
    return plan_bytes(heads, false, false, "agx_recurrent_heads_saved_bytes");
}

extern "C" size_t agx_recurrent_heads_workspace_bytes(const agx_recurrent_heads *heads) {
    return plan_bytes(heads, false, true, "agx_recurrent_heads_workspace_bytes");
}

extern "C" int agx_recurrent_heads_forward(const agx_recurrent_heads *heads, float *log_prob, float *entropy,
                                           float *value, void *saved, void *stream) {
    return heads_forward(heads, log_prob, entropy, value, saved, stream, false, "agx_recurrent_heads_forward");
}

extern "C" int agx_recurrent_heads_backward(const agx_recurrent_heads *heads, const void *saved,
                                            const agx_recurrent_heads_grads *grads, void *workspace, void *stream) {
    return heads_backward(heads, saved, grads, workspace, stream, false, "agx_recurrent_heads_backward");
}

extern "C" size_t agx_recurrent_heads_saved_bytes_shared(const agx_recurrent_heads *heads) {
    return plan_bytes(heads, true, false, "agx_recurrent_heads_saved_bytes_shared");
}

extern "C" size_t agx_recurrent_heads_workspace_bytes_shared(const agx_recurrent_heads *heads) {
    return plan_bytes(heads, true, true, "agx_recurrent_heads_workspace_bytes_shared");
}

extern "C" int agx_recurrent_heads_forward_shared(const agx_recurrent_heads *heads, float *log_prob, float *entropy,
                                                  float *value, void *saved, void *stream) {
    return heads_forward(heads, log_prob, entropy, value, saved, stream, true, "agx_recurrent_heads_forward_shared");
}

extern "C" int agx_recurrent_heads_backward_shared(const agx_recurrent_heads *heads, const void *saved,
                                                   const agx_recurrent_heads_grads *grads, void *workspace,
                                                   void *stream) {
    return heads_backward(heads, saved, grads, workspace, stream, true, "agx_recurrent_heads_backward_shared");
}
