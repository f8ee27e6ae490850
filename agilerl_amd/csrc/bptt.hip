// Truncated BPTT for recurrent PPO (include/agx_bptt.h): the sequence table, the
// padded minibatch gather and the masked clipped loss, all on a rollout that
// stays in HBM.
//
// Reference: agilerl/components/rollout_buffer.py:676-922 (a Python loop per env,
// per episode and per buffer key over a CPU copy of the buffer, then Python index
// lists per minibatch) and agilerl/algorithms/ppo.py:1007-1050 (three masked index
// ops and the loss block).
//
// Plan.  One wave per env.  Its lanes take 64 steps at a time; the done flags
// become one 64-bit ballot word (the bit of step T - 1 forced on: the buffer's end
// closes an episode), and the wave walks the word's set bits with bit scans, the
// start of the running episode carried from word to word.  An episode's sequences
// all have one length and a fixed stride, so their number, their rows and their
// table entries are closed forms of the episode's length.  Pass 1 counts
// sequences, rows and the longest length per env; one workgroup scans the N
// counts in env order; pass 2 repeats the walk and writes the table at the
// scanned offsets, 64 sequences of an episode per step.  Integers only.
//
// Gather.  One wave per (sequence, group of 16 steps).  Rows are moved as float4
// when the row length is a multiple of 4 floats and the arrays are 16-byte
// aligned, as dwords otherwise; the wave that owns a step writes its zeros when
// the step is padding, so no output is cleared beforehand.  The group-0 wave of a
// sequence also moves the hidden state of the sequence's first step into the
// (layers, batch, hidden) order the LSTM kernel takes.
//
// Loss.  The BPTT loop's loss (ppo.py:1015-1050): as the flat loop's, but the value
// loss is mean(max(..)) without the flat loop's factor 1/2.  One lane per padded
// row.  valid_row is ascending, so a lane finds its row's place among the valid
// rows (or that it is padding) by bisection; it
// evaluates ppo_loss_sample.h's sample with 1 / n_valid, writes the three
// gradients (zeros on padding) and hands its five loss terms, as doubles, to a
// butterfly sum per wave, an in-order sum per workgroup and an in-order sum of
// the workgroups' partials in a second launch.
#include "../../include/agx_bptt.h"
#include "ppo_loss_sample.h"

namespace agx {

// ---- plan -------------------------------------------------------------------
constexpr int kPlanBlock = 256;
constexpr int kPlanWaves = kPlanBlock / kWave;

// the sequences of an episode of e steps: k of them, `len` steps each, `stride` apart
__device__ __forceinline__ void episode_shape(int e, int m, int type, int &k, int &len, int &stride) {
    if (m == 0 || e < m) {
        k = 1;
        len = e;
        stride = 0;
        return;
    }
    len = m;
    if (type == AGX_BPTT_CHUNKED) {
        k = e / m;
        stride = m;
    } else if (type == AGX_BPTT_MAXIMUM) {
        k = e - m + 1;
        stride = 1;
    } else {
        stride = m / 2;
        k = (e - m) / stride + 1;
    }
}

// counts [N][3]: sequences, rows, longest length; env_off [N][2]: first table entry, first row
template <bool kWrite>
__global__ __launch_bounds__(kPlanBlock) void bptt_walk(const uint8_t *__restrict__ dones, int T, int N, int m,
                                                        int type, int32_t *__restrict__ counts,
                                                        const int32_t *__restrict__ env_off,
                                                        int32_t *__restrict__ seq, int32_t *__restrict__ row_offset) {
    const int lane = threadIdx.x & (kWave - 1);
    const int env = blockIdx.x * kPlanWaves + threadIdx.x / kWave;
    if (env >= N) return;  // whole waves leave together
    int ep_start = 0, nseq = 0, nrows = 0, longest = 0, so = 0, ro = 0;
    if (kWrite) {
        so = env_off[2 * env];
        ro = env_off[2 * env + 1];
    }
    for (int base = 0; base < T; base += kWave) {
        const int t = base + lane;
        const bool end = t < T && (t == T - 1 || dones[(size_t)t * N + env] != 0);
        unsigned long long word = __ballot(end);
        while (word) {  // wave-uniform
            const int last = base + __builtin_ctzll(word);
            word &= word - 1;
            int k, len, stride;
            episode_shape(last - ep_start + 1, m, type, k, len, stride);
            if (kWrite) {
                for (int j = lane; j < k; j += kWave) {
                    int32_t *s = seq + 3 * (size_t)(so + j);
                    s[0] = env;
                    s[1] = ep_start + j * stride;
                    s[2] = len;
                    row_offset[so + j] = ro + j * len;
                }
                so += k;
                ro += k * len;
            } else {
                nseq += k;
                nrows += k * len;
                longest = longest > len ? longest : len;
            }
            ep_start = last + 1;
        }
    }
    if (!kWrite && lane == 0) {
        counts[3 * env] = nseq;
        counts[3 * env + 1] = nrows;
        counts[3 * env + 2] = longest;
    }
}

// exclusive scan of the env counts in env order, one workgroup; meta = S, L, rows, 0
__global__ __launch_bounds__(kPlanBlock) void bptt_scan(const int32_t *__restrict__ counts, int N,
                                                        int32_t *__restrict__ env_off, int32_t *__restrict__ meta,
                                                        int32_t *__restrict__ row_offset) {
    __shared__ int wsum[3][kPlanWaves];
    const int lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    int carry_s = 0, carry_r = 0, longest = 0;
    for (int base = 0; base < N; base += kPlanBlock) {
        const int i = base + threadIdx.x;
        const int cs = i < N ? counts[3 * i] : 0, cr = i < N ? counts[3 * i + 1] : 0;
        if (i < N) longest = longest > counts[3 * i + 2] ? longest : counts[3 * i + 2];
        int is = cs, ir = cr;  // inclusive within the wave
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const int a = __shfl_up(is, o, kWave), b = __shfl_up(ir, o, kWave);
            if (lane >= o) {
                is += a;
                ir += b;
            }
        }
        if (lane == kWave - 1) {
            wsum[0][w] = is;
            wsum[1][w] = ir;
        }
        __syncthreads();
        int ps = 0, pr = 0, ts = 0, tr = 0;
        for (int j = 0; j < kPlanWaves; ++j) {
            if (j < w) {
                ps += wsum[0][j];
                pr += wsum[1][j];
            }
            ts += wsum[0][j];
            tr += wsum[1][j];
        }
        if (i < N) {
            env_off[2 * i] = carry_s + ps + is - cs;
            env_off[2 * i + 1] = carry_r + pr + ir - cr;
        }
        carry_s += ts;
        carry_r += tr;
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(longest, o, kWave);
        longest = longest > other ? longest : other;
    }
    if (lane == 0) wsum[2][w] = longest;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int j = 1; j < kPlanWaves; ++j) longest = longest > wsum[2][j] ? longest : wsum[2][j];
        meta[0] = carry_s;
        meta[1] = longest;
        meta[2] = carry_r;
        meta[3] = 0;
        row_offset[carry_s] = carry_r;
    }
}

// ---- gather -----------------------------------------------------------------
constexpr int kGatherBlock = 256;
constexpr int kGatherSteps = 16;  // steps of one sequence per wave

// steps [t0, t0 + nt) of one sequence: rows of `width` floats from src[(start + t) * N + env] to
// dst[b * L + t], zeros from step `len` on
template <bool kVec>
__device__ __forceinline__ void move_rows(const float *__restrict__ src, float *__restrict__ dst, int width, int t0,
                                          int nt, int len, int64_t start, int64_t N, int64_t env, int64_t dst_row0,
                                          int lane) {
    if (kVec) {
        const int wv = width >> 2;
        const float4 *s4 = reinterpret_cast<const float4 *>(src);
        float4 *d4 = reinterpret_cast<float4 *>(dst);
        for (int i = lane; i < nt * wv; i += kWave) {
            const int t = t0 + i / wv, c = i % wv;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (t < len) v = s4[((start + t) * N + env) * wv + c];
            d4[(dst_row0 + t) * wv + c] = v;
        }
    } else {
        for (int i = lane; i < nt * width; i += kWave) {
            const int t = t0 + i / width, c = i % width;
            float v = 0.f;
            if (t < len) v = src[((start + t) * N + env) * width + c];
            dst[(dst_row0 + t) * width + c] = v;
        }
    }
}

__global__ __launch_bounds__(kGatherBlock) void bptt_gather(const agx_bptt_gather_args a, int groups, bool vec_obs,
                                                            bool vec_act) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t wave = (int64_t)blockIdx.x * (kGatherBlock / kWave) + threadIdx.x / kWave;
    if (wave >= a.Bs * groups) return;  // whole waves leave together
    const int64_t b = wave / groups;
    const int g = (int)(wave % groups);
    const int64_t id = a.ids[b];
    int64_t env = 0, start = 0;
    int len = 0;
    if (id >= 0 && id < a.S) {
        env = a.seq[3 * id];
        start = a.seq[3 * id + 1];
        len = a.seq[3 * id + 2];
        // a table entry that leaves the rollout or the padded length counts as padding past that point
        if (env < 0 || env >= a.N || start < 0 || start >= a.T) len = 0;
        if (len > a.T - start) len = (int)(a.T - start);
        if (len > a.L) len = (int)a.L;
        if (len < 0) len = 0;
    }
    const int L = (int)a.L;
    const int t0 = g * kGatherSteps;
    const int nt = L - t0 < kGatherSteps ? L - t0 : kGatherSteps;
    const int64_t row0 = b * a.L;

    if (vec_obs) move_rows<true>(a.obs, a.obs_out, (int)a.D, t0, nt, len, start, a.N, env, row0, lane);
    else move_rows<false>(a.obs, a.obs_out, (int)a.D, t0, nt, len, start, a.N, env, row0, lane);
    if (vec_act) move_rows<true>(a.actions, a.act_out, (int)a.A, t0, nt, len, start, a.N, env, row0, lane);
    else move_rows<false>(a.actions, a.act_out, (int)a.A, t0, nt, len, start, a.N, env, row0, lane);
    if (a.mask) {
        const int M = (int)a.M;
        for (int i = lane; i < nt * M; i += kWave) {
            const int t = t0 + i / M, c = i % M;
            a.mask_out[(row0 + t) * M + c] = t < len ? a.mask[((start + t) * a.N + env) * M + c] : (uint8_t)0;
        }
    }
    // one lane per step: the pad mask and the step's place among the minibatch's valid rows
    if (lane < nt) {
        const int t = t0 + lane;
        const bool valid = t < len;
        a.pad_mask[row0 + t] = valid ? 1 : 0;
        const int64_t k = (int64_t)a.local_off[b] + t;
        if (valid && k >= 0 && k < a.n_valid) {
            const int64_t src = (start + t) * a.N + env;
            a.old_logp[k] = a.log_probs[src];
            a.adv[k] = a.advantages[src];
            a.ret[k] = a.returns[src];
            a.old_value[k] = a.values[src];
            a.valid_row[k] = row0 + t;
        }
    }
    if (g == 0) {  // [T][N][layers][H] at the first step -> [layers][Bs][H]
        for (int q = 0; q < a.n_hidden; ++q) {
            const int H = a.H[q], nl = a.layers[q];
            const float *src = a.hidden[q] + ((start * a.N + env) * nl) * H;
            for (int i = lane; i < nl * H; i += kWave) {
                const int l = i / H, h = i % H;
                a.hidden_out[q][((int64_t)l * a.Bs + b) * H + h] = len > 0 ? src[i] : 0.f;
            }
        }
    }
}

// ---- masked loss --------------------------------------------------------------
constexpr int kLossBlock = 256;
constexpr int kLossTerms = 5;  // policy, value, entropy, kl, clip fraction

__device__ __forceinline__ void block_sums(double (&v)[kLossTerms], double *__restrict__ out) {
    __shared__ double red[kLossTerms][kLossBlock / kWave];
#pragma unroll
    for (int q = 0; q < kLossTerms; ++q) v[q] = wave_sum(v[q]);
    if ((threadIdx.x & (kWave - 1)) == 0) {
#pragma unroll
        for (int q = 0; q < kLossTerms; ++q) red[q][threadIdx.x / kWave] = v[q];
    }
    __syncthreads();
    if (threadIdx.x < kLossTerms) {
        double s = 0.0;
        for (int j = 0; j < kLossBlock / kWave; ++j) s += red[threadIdx.x][j];
        out[threadIdx.x] = s;
    }
}

__global__ __launch_bounds__(kLossBlock) void seq_loss_rows(
    const float *__restrict__ logp, const float *__restrict__ value, const float *__restrict__ entropy, int64_t rows,
    const int64_t *__restrict__ valid_row, int64_t n_valid, const float *__restrict__ old_logp,
    const float *__restrict__ adv, const float *__restrict__ ret, const float *__restrict__ old_value, LossCoef k,
    float *__restrict__ g_logp, float *__restrict__ g_value, float *__restrict__ g_entropy,
    double *__restrict__ partials) {
    const int64_t p = (int64_t)blockIdx.x * kLossBlock + threadIdx.x;
    double term[kLossTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (p < rows) {
        int64_t lo = 0, hi = n_valid;  // the first valid row >= p
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (valid_row[mid] < p) lo = mid + 1;
            else hi = mid;
        }
        float gl = 0.f, gv = 0.f, gh = 0.f;
        if (lo < n_valid && valid_row[lo] == p) {
            Acc acc;
            loss_sample(logp[p], old_logp[lo], adv[lo], ret[lo], old_value[lo], value[p], entropy[p], k, gl, gv, acc);
            gh = k.g_h;
            term[0] = (double)acc.pg;
            term[1] = (double)acc.vl;
            term[2] = (double)acc.h;
            term[3] = (double)acc.kl;
            term[4] = (double)acc.cf;
        }
        g_logp[p] = gl;
        g_value[p] = gv;
        g_entropy[p] = gh;
    }
    block_sums(term, partials + (size_t)blockIdx.x * kLossTerms);
}

__global__ __launch_bounds__(kLossBlock) void seq_loss_finalize(const double *__restrict__ partials, int64_t nblk,
                                                                int64_t n_valid, LossCoef k,
                                                                float *__restrict__ stats) {
    __shared__ double total[kLossTerms];
    double term[kLossTerms] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = threadIdx.x; i < nblk; i += kLossBlock) {
#pragma unroll
        for (int q = 0; q < kLossTerms; ++q) term[q] += partials[i * kLossTerms + q];
    }
    block_sums(term, total);
    __syncthreads();
    if (threadIdx.x == 0) {
        const double n = (double)n_valid;
        const double pg = total[0] / n, vl = total[1] / n, el = -total[2] / n;  // no 1/2: ppo.py:1035
        stats[0] = (float)(pg + (double)k.vf * vl + (double)k.ent * el);
        stats[1] = (float)pg;
        stats[2] = (float)vl;
        stats[3] = (float)el;
        stats[4] = (float)(total[3] / n);
        stats[5] = (float)(total[4] / n);
        stats[6] = 0.f;
        stats[7] = 0.f;
    }
}

}  // namespace agx

using namespace agx;

static inline bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

extern "C" int64_t agx_bptt_capacity(int64_t T, int64_t N) { return T > 0 && N > 0 ? T * N : 0; }

extern "C" size_t agx_bptt_plan_workspace_bytes(int64_t N) { return N > 0 ? (size_t)N * 5 * sizeof(int32_t) : 0; }

extern "C" int agx_bptt_plan(const uint8_t *dones, int64_t T, int64_t N, int64_t max_seq_len, int type, int32_t *seq,
                             int32_t *row_offset, int32_t *meta, void *workspace, void *stream) {
    AGX_REQUIRE(T > 0 && N > 0, "agx_bptt_plan: empty rollout T=%lld N=%lld", (long long)T, (long long)N);
    AGX_REQUIRE(dones && seq && row_offset && meta && workspace, "agx_bptt_plan: null pointer");
    AGX_REQUIRE(max_seq_len >= 0, "agx_bptt_plan: max_seq_len %lld < 0", (long long)max_seq_len);
    AGX_REQUIRE(type == AGX_BPTT_CHUNKED || type == AGX_BPTT_MAXIMUM || type == AGX_BPTT_FIFTY_PERCENT_OVERLAP,
                "agx_bptt_plan: unknown sequence type %d", type);
    AGX_REQUIRE(type != AGX_BPTT_FIFTY_PERCENT_OVERLAP || max_seq_len != 1,
                "agx_bptt_plan: FIFTY_PERCENT_OVERLAP needs max_seq_len >= 2 (the stride is max_seq_len / 2)");
    const int64_t m1 = max_seq_len > 1 ? max_seq_len : 1;
    AGX_REQUIRE(T < ((int64_t)1 << 31) && N < ((int64_t)1 << 31) && m1 < ((int64_t)1 << 31) &&
                    T * N < ((int64_t)1 << 31) / m1,
                "agx_bptt_plan: T * N * max(max_seq_len, 1) must be < 2^31");
    hipStream_t s = as_stream(stream);
    int32_t *counts = static_cast<int32_t *>(workspace);
    int32_t *env_off = counts + 3 * N;
    const unsigned blocks = (unsigned)ceil_div(N, kPlanWaves);
    bptt_walk<false><<<blocks, kPlanBlock, 0, s>>>(dones, (int)T, (int)N, (int)max_seq_len, type, counts, nullptr,
                                                   nullptr, nullptr);
    int rc = check_launch("agx_bptt_plan count");
    if (rc) return rc;
    bptt_scan<<<1, kPlanBlock, 0, s>>>(counts, (int)N, env_off, meta, row_offset);
    rc = check_launch("agx_bptt_plan scan");
    if (rc) return rc;
    bptt_walk<true><<<blocks, kPlanBlock, 0, s>>>(dones, (int)T, (int)N, (int)max_seq_len, type, nullptr, env_off, seq,
                                                  row_offset);
    return check_launch("agx_bptt_plan write");
}

extern "C" int agx_bptt_gather(const agx_bptt_gather_args *args, void *stream) {
    AGX_REQUIRE(args, "agx_bptt_gather: null arguments");
    const agx_bptt_gather_args &a = *args;
    AGX_REQUIRE(a.S > 0 && a.Bs > 0 && a.L > 0 && a.T > 0 && a.N > 0 && a.D > 0 && a.A > 0 && a.n_valid >= 0,
                "agx_bptt_gather: bad shape S=%lld Bs=%lld L=%lld T=%lld N=%lld D=%lld A=%lld", (long long)a.S,
                (long long)a.Bs, (long long)a.L, (long long)a.T, (long long)a.N, (long long)a.D, (long long)a.A);
    AGX_REQUIRE(a.L <= a.T && a.n_valid <= a.Bs * a.L, "agx_bptt_gather: L %lld > T or n_valid %lld > Bs * L",
                (long long)a.L, (long long)a.n_valid);
    AGX_REQUIRE(a.D < (1 << 20) && a.A < (1 << 20) && a.M < (1 << 20) && a.L < (1 << 24) &&
                    a.T * a.N < ((int64_t)1 << 31),
                "agx_bptt_gather: shape too large");
    AGX_REQUIRE(a.seq && a.ids && a.local_off && a.obs && a.actions && a.log_probs && a.advantages && a.returns &&
                    a.values && a.obs_out && a.act_out && a.pad_mask && a.old_logp && a.adv && a.ret && a.old_value &&
                    a.valid_row,
                "agx_bptt_gather: null pointer");
    AGX_REQUIRE(!a.mask || (a.mask_out && a.M > 0), "agx_bptt_gather: a mask needs mask_out and M > 0");
    AGX_REQUIRE(a.n_hidden >= 0 && a.n_hidden <= AGX_BPTT_MAX_HIDDEN_KEYS, "agx_bptt_gather: %d hidden keys (0..%d)",
                a.n_hidden, AGX_BPTT_MAX_HIDDEN_KEYS);
    for (int q = 0; q < a.n_hidden; ++q)
        AGX_REQUIRE(a.hidden[q] && a.hidden_out[q] && a.layers[q] > 0 && a.H[q] > 0 && a.layers[q] * a.H[q] < (1 << 24),
                    "agx_bptt_gather: hidden key %d: null pointer or bad shape", q);
    const int groups = (int)ceil_div(a.L, kGatherSteps);
    const int64_t waves = a.Bs * groups;
    const int64_t blocks = ceil_div(waves, kGatherBlock / kWave);
    AGX_REQUIRE(blocks < ((int64_t)1 << 31), "agx_bptt_gather: too many sequences");
    const bool vec_obs = a.D % 4 == 0 && aligned16(a.obs) && aligned16(a.obs_out);
    const bool vec_act = a.A % 4 == 0 && aligned16(a.actions) && aligned16(a.act_out);
    bptt_gather<<<(unsigned)blocks, kGatherBlock, 0, as_stream(stream)>>>(a, groups, vec_obs, vec_act);
    return check_launch("agx_bptt_gather");
}

extern "C" size_t agx_ppo_seq_loss_workspace_bytes(int64_t rows) {
    return rows > 0 ? (size_t)ceil_div(rows, kLossBlock) * kLossTerms * sizeof(double) : 0;
}

extern "C" int agx_ppo_seq_loss_fwd_bwd(const float *logp, const float *value, const float *entropy, int64_t rows,
                                        const int64_t *valid_row, int64_t n_valid, const float *old_logp,
                                        const float *adv, const float *ret, const float *old_value, float clip_coef,
                                        float vf_coef, float ent_coef, float *g_logp, float *g_value,
                                        float *g_entropy, float *stats, void *workspace, void *stream) {
    AGX_REQUIRE(rows > 0 && n_valid > 0 && n_valid <= rows, "agx_ppo_seq_loss_fwd_bwd: %lld valid of %lld rows",
                (long long)n_valid, (long long)rows);
    AGX_REQUIRE(logp && value && entropy && valid_row && old_logp && adv && ret && old_value && g_logp && g_value &&
                    g_entropy && stats && workspace,
                "agx_ppo_seq_loss_fwd_bwd: null pointer");
    const int64_t blocks = ceil_div(rows, kLossBlock);
    AGX_REQUIRE(blocks < ((int64_t)1 << 31), "agx_ppo_seq_loss_fwd_bwd: too many rows");
    LossCoef k = loss_coef(n_valid, clip_coef, vf_coef, ent_coef);
    // the BPTT loop's value loss is mean(max(..)) (ppo.py:1035), not the flat loop's 0.5 * mean (ppo.py:889)
    k.vf_half_inv_b = vf_coef * k.inv_b;
    hipStream_t s = as_stream(stream);
    double *partials = static_cast<double *>(workspace);
    seq_loss_rows<<<(unsigned)blocks, kLossBlock, 0, s>>>(logp, value, entropy, rows, valid_row, n_valid, old_logp,
                                                          adv, ret, old_value, k, g_logp, g_value, g_entropy,
                                                          partials);
    int rc = check_launch("agx_ppo_seq_loss_fwd_bwd rows");
    if (rc) return rc;
    seq_loss_finalize<<<1, kLossBlock, 0, s>>>(partials, blocks, n_valid, k, stats);
    return check_launch("agx_ppo_seq_loss_fwd_bwd finalize");
}
