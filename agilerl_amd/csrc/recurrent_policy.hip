// The fused policy step of recurrent PPO (include/agx_recurrent.h): LSTM
// encoder at T = 1, output Linear, MLP head and the action distribution of
// both networks of an agent in one launch.
//
// Grid (ceil(N / 16), 2), 8 waves: workgroup (x, y) takes env rows 16 x ..
// 16 x + 15 through the actor (y = 0) or the critic (y = 1), so the two
// encoders run side by side and neither waits on the other: the actor
// workgroup writes action / log-prob / entropy, the critic workgroup the value.
//
// LDS: four slots of 16 rows, each wide enough for the widest tile of the
// launch (row stride: the tile's 16-rounded width + 4, which spreads the
// 16-byte A-operand reads of the 16 rows over the banks).
//   slot 0  the observation tile, zero-padded to 16 columns
//   slot 1  h_prev of the layer at hand (zeros for rows flagged in `reset`)
//   slot 2/3  h' of layer l in slot 2 + (l & 1): the A operand of layer l + 1
//             and, for the top layer, of the output Linear
// After the LSTM slots 0 and 1 are free and carry the latent and the head
// activations, ping-pong.
//
// LSTM layer: waves split by 16-unit tile as lstm.hip's fwd_kernel (wave w
// owns tiles w, w + 8, ..).  A tile's four gate accumulators start at b_ih +
// b_hh, take the input chain and then the h chain through lstm_gates.h with
// the same A operand, so lane (r, q) ends with all four pre-activations of
// rows 4q .. 4q + 3, unit 16 tile + r; c_prev comes from global memory into
// that lane, c' = f c + i g and h' = o tanh(c') stay in registers, h' goes to
// the LDS tile and both to the next-state outputs.  The accumulation order is
// fwd_kernel's, so the states have agx_lstm_forward's bits at T = 1 (W_hh
// register residency is a sequence optimisation: one step reads it once).
//
// Dense layers (recurrent_dense.h): one 16 x 16 output tile per wave and pass, one accumulator
// from the bias over k ascending, four 16-deep steps' operands requested ahead
// of their MFMAs; columns past the width are written as zeros, which is the
// padding the next layer's A operand needs.  LayerNorm / activation are row
// passes over the LDS tile, 16 lanes per row (waves 0 .. 3 hold the 16 rows).
//
// Epilogue, 16 lanes per row, entries a and a + 16 per lane, with the
// operation order of the categorical step of graph_rollout.hip and of
// gauss_policy.hip's gauss_step, on rollout.h's and gauss_head.h's streams.
// The multi-categorical and Bernoulli epilogues take all 8 waves, 32 lanes per
// row and one logit per lane (seg_scan.h): a component is a run of lanes, and
// its max, sum exp, entropy and Gumbel arg-max are segmented scans whose cost
// does not depend on the number of components.
//
// The shared-encoder form (agx_ppo_act_recurrent_shared, recurrent_step_shared_kernel below) runs a grid of
// (ceil(N / 16), 1): the same LSTM and output Linear once per row tile, then both heads in that workgroup.
#include "../../include/agx_recurrent.h"

#include <cstddef>
#include <cstring>

#include "agx_common.h"
#include "bern_head.h"
#include "gauss_head.h"
#include "lstm_gates.h"
#include "multi_head_check.h"
#include "recurrent_dense.h"
#include "rollout.h"
#include "seg_scan.h"

namespace agx {
namespace {

constexpr int kLdsCap = 160 * 1024;

// What the kernel takes by value: agx_recurrent_step up to `multi`, field for field, with the multi head reduced
// to `starts` (seg_scan.h) in the place of the pad word.  1200 bytes as before the multi head, 1204 with the slot
// width: under the 4 KB of kernel arguments (the 132-byte agx_multi_head stays on the host).
struct StepArgs {
    agx_recurrent_net actor, critic;
    const float *obs, *log_std;
    const uint8_t *reset, *mask;
    int64_t N;
    int32_t A, box, sample;
    uint32_t starts;
    uint64_t seed, counter;
    float *actions, *log_probs, *entropy, *values, *obs_store;
};
static_assert(sizeof(StepArgs) == offsetof(agx_recurrent_step, multi), "StepArgs mirrors agx_recurrent_step");
static_assert(sizeof(StepArgs) + sizeof(int) <= 4096, "the kernel arguments pass 4 KB");

// The categorical step of the 16 rows of logits Y [16][ld]: graph_rollout.hip's graph_sample, the action as a float
__device__ __forceinline__ void categorical_step(const StepArgs &s, const float *Y, int ld, int b0) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave >= 4) return;
    const int sub = lane & 15, rl = 4 * wave + (lane >> 4);
    const int A = s.A, N = (int)s.N, row = b0 + rl;
    const bool live = row < N;
    const int a0 = sub, a1 = sub + 16;
    float lg0 = a0 < A ? Y[rl * ld + a0] : -3.0e38f;
    float lg1 = a1 < A ? Y[rl * ld + a1] : -3.0e38f;
    if (s.mask && live) {
        const uint8_t *m = s.mask + (size_t)row * A;
        if (a0 < A && !m[a0]) lg0 = -1.0e8f;
        if (a1 < A && !m[a1]) lg1 = -1.0e8f;
    }
    const float mx = row_max(fmaxf(lg0, lg1));
    const float lse = mx + logf(row_sum((a0 < A ? expf(lg0 - mx) : 0.f) + (a1 < A ? expf(lg1 - mx) : 0.f)));
    const float p0 = a0 < A ? expf(lg0 - lse) : 0.f, p1 = a1 < A ? expf(lg1 - lse) : 0.f;
    const float H = -row_sum((a0 < A ? p0 * logf(p0 + 1e-8f) : 0.f) + (a1 < A ? p1 * logf(p1 + 1e-8f) : 0.f));
    if (live && sub == 0 && s.entropy) s.entropy[row] = H;
    if (!s.sample) return;  // uniform
    const unsigned long long env = stream_env(-1, nullptr, 0, N, live ? row : 0);
    const float sc0 = a0 < A ? gumbel_score(lg0, a0, env, s.seed, s.counter) : -3.0e38f;
    const float sc1 = a1 < A ? gumbel_score(lg1, a1, env, s.seed, s.counter) : -3.0e38f;
    // first maximum over the actions: lane-local (a0 < a1), then the lowest index among the row's maxima
    const float bl = fmaxf(sc0, sc1);
    const int il = sc0 >= sc1 ? a0 : a1;
    const float best = row_max(bl);
    const int choice = (int)(-row_max(bl == best ? -(float)il : -1.0e9f));
    const int srcl = (lane & ~15) + (choice & 15);
    const float c0 = bperm(srcl, lg0), c1 = bperm(srcl, lg1);
    if (live && sub == 0) {
        if (s.actions) s.actions[row] = (float)choice;
        if (s.log_probs) s.log_probs[row] = (choice < 16 ? c0 : c1) - lse;
    }
}

// The Gaussian step of the 16 rows of means Y [16][ld]: gauss_policy.hip's gauss_step
__device__ __forceinline__ void gauss_step(const StepArgs &s, const float *Y, int ld, int b0) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave >= 4) return;
    const int sub = lane & 15, rl = 4 * wave + (lane >> 4);
    const int A = s.A, N = (int)s.N, row = b0 + rl;
    const bool live = row < N;
    const int d0 = sub, d1 = sub + 16;
    const bool on0 = d0 < A, on1 = d1 < A;
    const float ls0 = on0 ? s.log_std[d0] : 0.f, ls1 = on1 ? s.log_std[d1] : 0.f;
    const float H = gauss_entropy(A, row_sum(ls0 + ls1));
    if (live && sub == 0 && s.entropy) s.entropy[row] = H;
    if (!s.sample) return;  // uniform
    const float mu0 = on0 ? Y[rl * ld + d0] : 0.f, mu1 = on1 ? Y[rl * ld + d1] : 0.f;
    const unsigned long long env = stream_env(-1, nullptr, 0, N, live ? row : 0);
    float a0 = mu0, a1 = mu1;
    if (on0) a0 = fmaf(expf(ls0), gauss_noise(d0, env, s.seed, s.counter), mu0);
    if (on1) a1 = fmaf(expf(ls1), gauss_noise(d1, env, s.seed, s.counter), mu1);
    const float lp = row_sum((on0 ? gauss_logp_term(a0, mu0, ls0) : 0.f) + (on1 ? gauss_logp_term(a1, mu1, ls1) : 0.f));
    if (!live) return;
    if (s.actions) {
        if (on0) s.actions[(size_t)row * A + d0] = a0;
        if (on1) s.actions[(size_t)row * A + d1] = a1;
    }
    if (sub == 0 && s.log_probs) s.log_probs[row] = lp;
}

// The multi-categorical step of the 16 rows of logits Y [16][ld]: the K categoricals of agx_multi.h, lane j of a
// row on flat logit j.  Scores are keyed by the flat index, so one component of A choices makes categorical_step's
// choices.
__device__ __forceinline__ void multi_step(const StepArgs &s, const float *Y, int ld, int b0) {
    const SegLane g = seg_lane(s.starts, s.A);
    const int A = s.A, N = (int)s.N, row = b0 + g.rl;
    const bool live = row < N;
    float lg = g.on ? Y[g.rl * ld + g.j] : -3.0e38f;
    if (s.mask && live && g.on && !s.mask[(size_t)row * A + g.j]) lg = -1.0e8f;
    const float mx = seg_total(g, seg_scan_max(g, lg));
    const float lse = mx + logf(seg_total(g, seg_scan_sum(g, g.on ? expf(lg - mx) : 0.f)));
    const float p = g.on ? expf(lg - lse) : 0.f;
    const bool tail = g.on && g.j == g.last;  // the lane that ends with its component's totals
    const float nh = seg_scan_sum(g, g.on ? p * logf(p + 1e-8f) : 0.f);
    const float H = -row32_sum(tail ? nh : 0.f);
    if (live && g.j == 0 && s.entropy) s.entropy[row] = H;
    if (!s.sample) return;  // uniform
    const unsigned long long env = stream_env(-1, nullptr, 0, N, live ? row : 0);
    float sc = g.on ? gumbel_score(lg, g.j, env, s.seed, s.counter) : -3.0e38f;
    int ix = g.j;
    seg_scan_argmax(g, sc, ix);
    const float chosen = bperm(g.half + (tail ? ix : g.j), lg);
    const float lp = row32_sum(tail ? chosen - lse : 0.f);
    if (!live) return;
    if (tail && s.actions) s.actions[(size_t)row * __popc(s.starts) + g.k] = (float)(ix - g.first);
    if (g.j == 0 && s.log_probs) s.log_probs[row] = lp;
}

// The Bernoulli step of the 16 rows of logits Y [16][ld]: bern_policy.hip's bern_step, lane j of a row on bit j
__device__ __forceinline__ void bern_step(const StepArgs &s, const float *Y, int ld, int b0) {
    const SegLane g = bit_lane(s.A);
    const int A = s.A, N = (int)s.N, row = b0 + g.rl;
    const bool live = row < N;
    float lg = g.on ? Y[g.rl * ld + g.j] : 0.f;
    if (s.mask && live && g.on && !s.mask[(size_t)row * A + g.j]) lg = -1.0e8f;
    const BernBit b = bern_bit(lg);
    const float H = -row32_sum(g.on ? bern_neg_entropy(b) : 0.f);
    if (live && g.j == 0 && s.entropy) s.entropy[row] = H;
    if (!s.sample) return;  // uniform
    const unsigned long long env = stream_env(-1, nullptr, 0, N, live ? row : 0);
    const bool a = g.on && bern_uniform(g.j, env, s.seed, s.counter) < b.p;
    const float lp = row32_sum(g.on ? (a ? b.lp : b.lq) : 0.f);
    if (!live) return;
    if (g.on && s.actions) s.actions[(size_t)row * A + g.j] = a ? 1.f : 0.f;
    if (g.j == 0 && s.log_probs) s.log_probs[row] = lp;
}

// The LSTM of network n at T = 1 over env rows b0 .. b0 + 15: h' of the top layer ends in slot 2 + ((L - 1) & 1),
// whole, and slots 0 and 1 are free.  `keep_obs`: this workgroup also writes the rollout slot's copy of obs.
__device__ __forceinline__ void lstm_step(const StepArgs &s, const agx_recurrent_net &n, float *lds, int slot, int b0,
                                          bool keep_obs) {
    const int N = (int)s.N, H = n.lstm.H, L = n.lstm.L, in = n.lstm.in;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, q = lane >> 4;
    const int sr = threadIdx.x >> 5, sc = threadIdx.x & 31;  // staging: 32 threads per row
    const int in16 = (in + 15) & ~15, ldx = in16 + 4, ldh = H + 4;
    float *xs = lds, *hs = lds + slot;
    const int srow = b0 + sr;
    const bool slive = srow < N;
    const bool skeep = slive && !(s.reset && s.reset[srow]);  // the row carries its state into the step

    lstm::stage_step(xs, ldx, s.obs, N, 1, 0, in, in16, b0);
    if (keep_obs && s.obs_store && slive)
        for (int k = sc; k < in; k += 32) s.obs_store[(int64_t)srow * in + k] = s.obs[(int64_t)srow * in + k];

    for (int l = 0; l < L; ++l) {
        const agx_lstm_layer &p = n.lstm.layer[l];
        const int K = l ? H : in;
        const float *xin = l ? lds + (2 + ((l - 1) & 1)) * slot : xs;
        const int ldin = l ? ldh : ldx;
        float *hout = lds + (2 + (l & 1)) * slot;
        {  // h_prev of this layer into LDS; the state the step is taken from into the rollout slot
            const int64_t o = ((int64_t)l * N + min(srow, N - 1)) * H;
            const int64_t so = ((int64_t)min(srow, N - 1) * L + l) * H;
            for (int k = sc; k < H; k += 32) {
                const float hv = skeep ? n.h[o + k] : 0.f;
                hs[sr * ldh + k] = hv;
                if (slive && n.h_store) n.h_store[so + k] = hv;
                if (slive && n.c_store) n.c_store[so + k] = skeep ? n.c[o + k] : 0.f;
            }
        }
        __syncthreads();
        const float *xrow = xin + r * ldin, *hrow = hs + r * ldh;
        const bool vec_ih = (K & 3) == 0 && lstm::aligned16(p.w_ih);
        const bool vec_hh = lstm::aligned16(p.w_hh);
        for (int tile = wave; tile < (H >> 4); tile += kRW) {
            const int unit = tile * 16 + r;
            f32x4 acc[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float b = p.b_ih[g * H + unit] + p.b_hh[g * H + unit];
                acc[g] = f32x4{b, b, b, b};
            }
            const float *wi = p.w_ih + (int64_t)unit * K;
            if (vec_ih)
                lstm::gates_vec<2>(K, q, acc, xrow, wi, (int64_t)H * K);
            else
                lstm::gates_any(K, q, acc, xrow, wi, (int64_t)H * K);
            const float *wh = p.w_hh + (int64_t)unit * H;
            if (vec_hh)
                lstm::gates_vec<2>(H, q, acc, hrow, wh, (int64_t)H * H);
            else
                lstm::gates_any(H, q, acc, hrow, wh, (int64_t)H * H);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = b0 + 4 * q + i;
                const bool live = row < N;
                const int64_t o = ((int64_t)l * N + min(row, N - 1)) * H + unit;
                const float cp = (live && !(s.reset && s.reset[row])) ? n.c[o] : 0.f;
                const float ig = lstm::sigm(acc[0][i]), fg = lstm::sigm(acc[1][i]), gg = tanhf(acc[2][i]),
                            og = lstm::sigm(acc[3][i]);
                const float cv = fg * cp + ig * gg;
                const float hv = og * tanhf(cv);
                hout[(4 * q + i) * ldh + unit] = hv;
                if (live) {
                    if (n.h_next) n.h_next[o] = hv;
                    if (n.c_next) n.c_next[o] = cv;
                }
            }
        }
        __syncthreads();  // h' is whole, and hs is free for the next layer's h_prev
    }
}

// the actor's distribution over the 16 rows of its head's output Y [16][ld]
__device__ __forceinline__ void actor_step(const StepArgs &s, const float *Y, int ld, int b0) {
    if (s.box == AGX_RECURRENT_HEAD_BOX)
        gauss_step(s, Y, ld, b0);
    else if (s.box == AGX_RECURRENT_HEAD_MULTI)
        multi_step(s, Y, ld, b0);
    else if (s.box == AGX_RECURRENT_HEAD_BERNOULLI)
        bern_step(s, Y, ld, b0);
    else
        categorical_step(s, Y, ld, b0);
}

__device__ __forceinline__ void value_store(const StepArgs &s, const float *Y, int ld, int b0) {
    const int row = b0 + threadIdx.x;
    if (threadIdx.x < 16 && row < (int)s.N && s.values) s.values[row] = Y[threadIdx.x * ld];
}

__global__ __launch_bounds__(kRT) void recurrent_step_kernel(const StepArgs s, const int slot) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const bool critic = blockIdx.y != 0;
    const agx_recurrent_net &n = critic ? s.critic : s.actor;
    const int H = n.lstm.H, L = n.lstm.L, ldh = H + 4;
    const int b0 = blockIdx.x * 16;
    lstm_step(s, n, lds, slot, b0, !critic);

    // the encoder's output Linear and activation, then the head: slots 0 and 1 in turn
    const float *X = lds + (2 + ((L - 1) & 1)) * slot;
    int ldX = ldh, F = n.latent, side = 0;
    float *Y = lds;
    int ldY = ((F + 15) & ~15) + 4;
    dense(X, ldX, H, n.out_w, n.out_b, F, Y, ldY);
    __syncthreads();
    row_pass(Y, ldY, F, nullptr, nullptr, n.out_act);
    __syncthreads();
    for (int j = 0; j < n.n_head; ++j) {
        const agx_recurrent_linear &hl = n.head[j];
        X = Y;
        ldX = ldY;
        side ^= 1;
        Y = lds + side * slot;
        F = hl.out;
        ldY = ((F + 15) & ~15) + 4;
        dense(X, ldX, hl.in, hl.w, hl.b, F, Y, ldY);
        __syncthreads();
        row_pass(Y, ldY, F, hl.ln_w, hl.ln_b, hl.relu ? AGX_RECURRENT_ACT_RELU : AGX_RECURRENT_ACT_NONE);
        __syncthreads();
    }
    if (critic)
        value_store(s, Y, ldY, b0);
    else
        actor_step(s, Y, ldY, b0);
}

// The shared-encoder step (agx_ppo_act_recurrent_shared), grid (ceil(N / 16), 1): the LSTM and the output Linear
// of s.actor once per row tile, then both heads in this workgroup off the one latent tile.  The latent lands in
// slot 0; by then the LSTM's slots 2 and 3 are dead, so the actor's head goes on between slots 1 and 0 as in the
// kernel above while the critic's takes slots 2 and 3, and no fifth slot is needed at any shape.  Depth j of both
// heads is one tile list over the 8 waves (dense_pair) and one row pass (actor: waves 0 .. 3, critic: 4 .. 7)
// between one pair of barriers; the actor's depth 1 overwrites the latent only after the barrier that ends
// depth 0, where the critic has read it.  A head that has run out of layers keeps its output where it is.
__global__ __launch_bounds__(kRT) void recurrent_step_shared_kernel(const StepArgs s, const int slot) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const agx_recurrent_net &n = s.actor;
    const int H = n.lstm.H, L = n.lstm.L;
    const int b0 = blockIdx.x * 16;
    lstm_step(s, n, lds, slot, b0, true);

    const int ldl = ((n.latent + 15) & ~15) + 4;
    dense(lds + (2 + ((L - 1) & 1)) * slot, H + 4, H, n.out_w, n.out_b, n.latent, lds, ldl);
    __syncthreads();
    row_pass(lds, ldl, n.latent, nullptr, nullptr, n.out_act);
    __syncthreads();
    DenseSide a{nullptr, lds, 0, ldl, true}, c{nullptr, lds, 0, ldl, true};
    const int na = n.n_head, nc = s.critic.n_head;
    for (int j = 0; j < (na > nc ? na : nc); ++j) {
        const agx_recurrent_linear &la = n.head[min(j, na - 1)], &lc = s.critic.head[min(j, nc - 1)];
        a.on = j < na;
        c.on = j < nc;
        if (a.on) a.advance(lds + ((j + 1) & 1) * slot, la.out);
        if (c.on) c.advance(lds + (2 + (j & 1)) * slot, lc.out);
        dense_pair(la, a, lc, c);
        __syncthreads();
        row_pass_pair(la, a, lc, c);
        __syncthreads();
    }
    value_store(s, c.Y, c.ldy, b0);
    actor_step(s, a.Y, a.ldy, b0);
}

int check_head(const agx_recurrent_net &n, int width, int out, const char *name, const char *who);

int check_net(const agx_recurrent_net &n, int out, const char *name, const char *who) {
    const agx_lstm_desc &d = n.lstm;
    AGX_REQUIRE(d.L >= 1 && d.L <= AGX_LSTM_MAX_LAYERS, "%s: %s: %d layers outside [1, %d]", who, name, d.L,
                AGX_LSTM_MAX_LAYERS);
    AGX_REQUIRE(d.H >= 16 && d.H <= AGX_LSTM_MAX_HIDDEN && d.H % 16 == 0,
                "%s: %s: hidden size %d is not a multiple of 16 in [16, %d]", who, name, d.H, AGX_LSTM_MAX_HIDDEN);
    AGX_REQUIRE(d.in >= 1 && d.in <= AGX_LSTM_MAX_INPUT, "%s: %s: input size %d outside [1, %d]", who, name, d.in,
                AGX_LSTM_MAX_INPUT);
    for (int l = 0; l < d.L; ++l) {
        const agx_lstm_layer &p = d.layer[l];
        AGX_REQUIRE(p.w_ih && p.w_hh && p.b_ih && p.b_hh, "%s: %s: LSTM layer %d: a parameter is NULL", who, name, l);
    }
    AGX_REQUIRE(n.out_w && n.out_b && n.h && n.c, "%s: %s: the output Linear or a state is NULL", who, name);
    AGX_REQUIRE(n.latent >= 1 && n.latent <= AGX_PPO_GRAPH_MAX_WIDTH, "%s: %s: latent %d outside [1, %d]", who, name,
                n.latent, AGX_PPO_GRAPH_MAX_WIDTH);
    AGX_REQUIRE(n.out_act >= AGX_RECURRENT_ACT_NONE && n.out_act <= AGX_RECURRENT_ACT_TANH,
                "%s: %s: output activation %d", who, name, n.out_act);
    return check_head(n, n.latent, out, name, who);
}

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

int widest(const agx_recurrent_net &n) {
    int w = n.lstm.in > n.lstm.H ? n.lstm.in : n.lstm.H;
    w = n.latent > w ? n.latent : w;
    for (int j = 0; j < n.n_head; ++j) w = n.head[j].out > w ? n.head[j].out : w;
    return w;
}

}  // namespace
}  // namespace agx

using namespace agx;

// Both entry points: `shared` takes the encoder of s.actor for both heads and reads the critic's head only
static int act_recurrent(const agx_recurrent_step *step, void *stream, bool shared, const char *who) {
    AGX_REQUIRE(step, "%s: step is NULL", who);
    const agx_recurrent_step &s = *step;
    AGX_REQUIRE(s.N >= 1 && s.N <= (1 << 24), "%s: N %lld outside [1, 2^24]", who, (long long)s.N);
    AGX_REQUIRE(s.A >= 1 && s.A <= AGX_PPO_GRAPH_MAX_ACTIONS, "%s: %d actions (1..%d)", who, s.A,
                AGX_PPO_GRAPH_MAX_ACTIONS);
    AGX_REQUIRE(s.obs, "%s: obs is NULL", who);
    AGX_REQUIRE(s.box >= AGX_RECURRENT_HEAD_DISCRETE && s.box <= AGX_RECURRENT_HEAD_BERNOULLI, "%s: head kind %d", who,
                s.box);
    AGX_REQUIRE(s.box == AGX_RECURRENT_HEAD_BOX ? (s.log_std && !s.mask) : !s.log_std,
                "%s: log_std goes with Box, a mask with the other heads", who);
    StepArgs k;
    std::memcpy(&k, step, sizeof k);
    k.starts = 0;
    if (s.box == AGX_RECURRENT_HEAD_MULTI) {
        const int L = head_width(s.multi, who);
        if (L < 0) return AGX_EINVAL;
        AGX_REQUIRE(L == s.A, "%s: nvec sums to %d, the head has %d logits", who, L, s.A);
        k.starts = multi_starts(s.multi);
    }
    if (int rc = check_net(s.actor, s.A, "actor", who)) return rc;
    int wc = 0;
    if (shared) {
        if (int rc = check_head(s.critic, s.actor.latent, 1, "critic", who)) return rc;
        for (int j = 0; j < s.critic.n_head; ++j) wc = s.critic.head[j].out > wc ? s.critic.head[j].out : wc;
    } else {
        if (int rc = check_net(s.critic, 1, "critic", who)) return rc;
        AGX_REQUIRE(s.actor.lstm.in == s.critic.lstm.in, "%s: the networks read observations of %d and %d floats",
                    who, s.actor.lstm.in, s.critic.lstm.in);
        wc = widest(s.critic);
    }
    const int wa = widest(s.actor);
    const int slot = 16 * ((((wa > wc ? wa : wc) + 15) & ~15) + 4);
    const size_t bytes = (size_t)4 * slot * sizeof(float);  // at most 4 * 16 * 516 * 4 = 129 KB
    static const bool once = [] {
        (void)hipFuncSetAttribute((const void *)recurrent_step_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  kLdsCap);
        (void)hipFuncSetAttribute((const void *)recurrent_step_shared_kernel,
                                  hipFuncAttributeMaxDynamicSharedMemorySize, kLdsCap);
        return true;
    }();
    (void)once;
    const dim3 grid((unsigned)ceil_div(s.N, 16), shared ? 1 : 2);
    if (shared)
        hipLaunchKernelGGL(recurrent_step_shared_kernel, grid, dim3(kRT), bytes, as_stream(stream), k, slot);
    else
        hipLaunchKernelGGL(recurrent_step_kernel, grid, dim3(kRT), bytes, as_stream(stream), k, slot);
    return check_launch(who);
}

extern "C" int agx_ppo_act_recurrent(const agx_recurrent_step *step, void *stream) {
    return act_recurrent(step, stream, false, "agx_ppo_act_recurrent");
}

extern "C" int agx_ppo_act_recurrent_shared(const agx_recurrent_step *step, void *stream) {
    return act_recurrent(step, stream, true, "agx_ppo_act_recurrent_shared");
}
