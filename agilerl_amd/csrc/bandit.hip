// Arm selection of the neural contextual bandits — agilerl/algorithms/
// neural_ucb_bandit.py:237-257 and neural_ts_bandit.py:236-254 (get_action
// after the gradients are known):
//   quad_k  = g_k Sigma^-1 g_k^T                      (g_k = scale [h_k, 1]: the closed-form gradient of the
//                                                      output Linear(H, 1), or an explicit row when bias_one = 0)
//   score_k = mu_k + gamma sqrt(quad_k) [* z_k]       (UCB | Thompson, z_k a Philox Box-Muller normal)
//   action  = np.argmax over the legal arms           (masked arms count as -inf, as np.ma fills them)
//   Sigma^-1 -= u w^T / (1 + v.u),  v = g_action, u = Sigma^-1 v, w = Sigma^-T v
// The last line is the reference's Sigma^-1 v v^T Sigma^-1 / (1 + v^T Sigma^-1 v)
// without its D x D by D x D product: two matrix-vector products and one pass.
//
// The step is a chain of tiny dependent operations on a D x D matrix that the
// next env step needs again, so its time is latency, not throughput.  Every
// sum is accumulated in f64 (full rate on CDNA, and the operand counts here are
// thousands) in a fixed order and rounded to f32 once.
//
// Two forms, chosen by D (AGX_BANDIT_RESIDENT_MAX_D, agx_bandit.h):
//   * resident: one workgroup of 8 waves holds the matrix in LDS (row stride
//     D | 1 words: lanes walking a column sit on distinct banks, lanes walking a
//     row are consecutive anyway).  A wave takes an arm: its lanes stride over
//     the columns j, each forms t_j = sum_i g_i S[i][j] and the wave sums
//     t_j g_j.  Wave 0 takes the argmax; D lanes form u, D others w; the
//     updated matrix goes from LDS to memory.  One launch, the matrix read once
//     and written once.
//   * streaming: the matrix stays in memory / L2 and the step is four launches
//     in stream order — (row tile, column tile) partials of quad for eight arms per
//     workgroup (each matrix element read once per eight arms), the selection,
//     u and w, the rank-1 pass.  A single launch would need a grid-wide
//     hand-off between those phases (a spin on a flag by co-resident
//     workgroups); replayed from a captured graph the launch boundaries cost
//     about as much and cannot hang.
#include "rollout.h"

#include "../../include/agx_bandit.h"

namespace agx {

constexpr int kBanditWaves = 8;                       // resident form: one workgroup of 8 waves
constexpr int kBanditThreads = kBanditWaves * kWave;  // 512
constexpr int kArmTile = 8;                           // streaming form: arms per workgroup of the quad kernel
constexpr int kColTile = 256;                         // ... and its columns (one per thread)
constexpr int kRowTile = 128;                         // ... and the rows a thread walks
constexpr int kRowWaves = 4;                          // waves of the u / w and update kernels

struct BanditArgs {
    const float *h;
    long long ldh;
    const float *mu;
    float *sigma;
    const unsigned char *mask;
    int A, H, D;
    float scale, gamma;
    int mode;
    unsigned long long seed;
    long long *counter;
    float *scores, *quad;
    long long *action;
};

// element i of arm k's gradient row
__device__ __forceinline__ float bandit_g(const BanditArgs &a, int k, int i) {
    return i < a.H ? a.scale * a.h[(size_t)k * a.ldh + i] : a.scale;
}

// gauss_policy.hip's draw of dimension 0 of env k
__device__ __forceinline__ float bandit_normal(int k, unsigned long long seed, unsigned long long counter) {
    const uint4 rnd = philox(make_uint4((unsigned)k, 0u, (unsigned)counter, (unsigned)(counter >> 32)),
                             make_uint2((unsigned)seed, (unsigned)(seed >> 32)));
    const float u1 = ((float)(rnd.x >> 8) + 0.5f) * (1.0f / 16777216.0f);
    const float u2 = ((float)(rnd.y >> 8) + 0.5f) * (1.0f / 16777216.0f);
    return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// The score as selection sees it: -inf for an arm whose mask byte is not 1.
// mu and the width often cancel (a low mean under a wide bound), so the sum is
// formed in f64 from the unrounded quadratic form and rounded once: its error
// is half an ulp of the score, not of the larger operand.
__device__ __forceinline__ float bandit_score(const BanditArgs &a, int k, double quad, unsigned long long counter) {
    double width = (double)a.gamma * sqrt(quad);
    if (a.mode) width *= (double)bandit_normal(k, a.seed, counter);
    const float s = (float)((double)a.mu[k] + width);
    a.quad[k] = (float)quad;
    a.scores[k] = s;
    return !a.mask || a.mask[k] == 1 ? s : -INFINITY;
}

// np.argmax's order: a NaN beats every number, the first of equals wins
__device__ __forceinline__ bool bandit_better(float s, int i, float t, int j) {
    const bool ns = s != s, nt = t != t;
    if (ns != nt) return ns;
    if (ns) return i < j;
    return s > t || (s == t && i < j);
}

// one wave: argmax of sc[0 .. A) in every lane
__device__ __forceinline__ int bandit_argmax(const float *sc, int A, int lane) {
    float best = -INFINITY;
    int idx = 0x7fffffff;
    for (int k = lane; k < A; k += kWave)
        if (bandit_better(sc[k], k, best, idx)) {
            best = sc[k];
            idx = k;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(best, o, 64);
        const int j = __shfl_xor(idx, o, 64);
        if (bandit_better(t, j, best, idx)) {
            best = t;
            idx = j;
        }
    }
    return idx;
}

__device__ __forceinline__ void bandit_publish(const BanditArgs &a, int action, unsigned long long counter) {
    *a.action = action;
    if (a.counter && a.mode) *a.counter = (long long)(counter + 1);  // a Thompson call used one block of the stream
}

// ---- resident form ---------------------------------------------------------------------
__global__ __launch_bounds__(kBanditThreads) void bandit_resident_kernel(BanditArgs a) {
    extern __shared__ double bandit_lds[];
    const int D = a.D, A = a.A, S = D | 1;
    double *ud = bandit_lds, *wd = ud + D;
    float *sm = reinterpret_cast<float *>(wd + D);  // [D][S]
    float *gb = sm + D * S;                          // [kBanditWaves][D]
    float *sc = gb + kBanditWaves * D;               // [A]
    __shared__ int s_act;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned long long counter = a.counter ? (unsigned long long)*a.counter : 0ull;

    for (int i = wave; i < D; i += kBanditWaves)
        for (int j = lane; j < D; j += kWave) sm[i * S + j] = a.sigma[(size_t)i * D + j];

    float *g = gb + wave * D;
    for (int k0 = 0; k0 < A; k0 += kBanditWaves) {  // uniform over the workgroup: the barriers are inside
        const int k = k0 + wave;
        if (k < A)
            for (int i = lane; i < D; i += kWave) g[i] = bandit_g(a, k, i);
        __syncthreads();
        if (k < A) {
            double p = 0.0;
            for (int j = lane; j < D; j += kWave) {
                double t = 0.0;
                for (int i = 0; i < D; ++i) t += (double)g[i] * (double)sm[i * S + j];
                p += t * (double)g[j];
            }
            p = wave_sum(p);
            if (lane == 0) sc[k] = bandit_score(a, k, p, counter);
        }
        __syncthreads();
    }
    if (wave == 0) {
        const int best = bandit_argmax(sc, A, lane);
        if (lane == 0) {
            s_act = best;
            bandit_publish(a, best, counter);
        }
    }
    __syncthreads();
    const int act = s_act;
    float *v = gb;
    if (tid < D) v[tid] = bandit_g(a, act, tid);
    __syncthreads();
    if (tid < D) {  // u_i: lane i walks row i (stride S, odd: distinct banks)
        double s = 0.0;
        for (int j = 0; j < D; ++j) s += (double)sm[tid * S + j] * (double)v[j];
        ud[tid] = s;
    } else if (tid >= kBanditThreads / 2 && tid - kBanditThreads / 2 < D) {  // w_j: lane j walks column j
        const int j = tid - kBanditThreads / 2;
        double s = 0.0;
        for (int i = 0; i < D; ++i) s += (double)sm[i * S + j] * (double)v[i];
        wd[j] = s;
    }
    __syncthreads();
    double vu = 0.0;  // every wave forms v.u for itself, in the same order
    for (int i = lane; i < D; i += kWave) vu += (double)v[i] * ud[i];
    const double r = 1.0 / (1.0 + wave_sum(vu));
    for (int i = wave; i < D; i += kBanditWaves) {
        const double ui = ud[i] * r;
        for (int j = lane; j < D; j += kWave) a.sigma[(size_t)i * D + j] = (float)((double)sm[i * S + j] - ui * wd[j]);
    }
}

static size_t bandit_resident_lds(int64_t A, int64_t D) {
    return (size_t)(2 * D) * sizeof(double) + (size_t)(D * (D | 1) + kBanditWaves * D + A) * sizeof(float);
}

// ---- streaming form ----------------------------------------------------------------------
// part[t][k], t = row tile * column tiles + column tile: the part of quad_k
// = sum_ij g_i S[i][j] g_j over rows [r kRowTile, (r + 1) kRowTile) and columns
// [c kColTile, (c + 1) kColTile).  The rows are tiled over workgroups because a
// thread's walk down its column is a chain of dependent-latency loads: at D =
// 501 and 7 arms two column tiles alone would leave the matrix to two CUs.
__global__ __launch_bounds__(kColTile) void bandit_quad_kernel(BanditArgs a, double *__restrict__ part) {
    extern __shared__ float bandit_gt[];  // [kArmTile][D]
    __shared__ double red[kColTile / kWave][kArmTile];
    const int D = a.D, A = a.A, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int k0 = blockIdx.x * kArmTile;
    const int na = A - k0 < kArmTile ? A - k0 : kArmTile;
    for (int r = 0; r < kArmTile; ++r)
        for (int i = tid; i < D; i += kColTile) bandit_gt[r * D + i] = r < na ? bandit_g(a, k0 + r, i) : 0.f;
    __syncthreads();
    const int j = blockIdx.y * kColTile + tid;
    double p[kArmTile];
#pragma unroll
    for (int r = 0; r < kArmTile; ++r) p[r] = 0.0;
    const int i0 = blockIdx.z * kRowTile, i1 = i0 + kRowTile < D ? i0 + kRowTile : D;
    if (j < D) {
        for (int i = i0; i < i1; ++i) {
            const double s = (double)a.sigma[(size_t)i * D + j];
#pragma unroll
            for (int r = 0; r < kArmTile; ++r) p[r] += (double)bandit_gt[r * D + i] * s;
        }
#pragma unroll
        for (int r = 0; r < kArmTile; ++r) p[r] *= (double)bandit_gt[r * D + j];
    }
#pragma unroll
    for (int r = 0; r < kArmTile; ++r) {
        const double s = wave_sum(p[r]);
        if (lane == 0) red[wave][r] = s;
    }
    __syncthreads();
    if (tid < na)
        part[((size_t)blockIdx.z * gridDim.y + blockIdx.y) * A + k0 + tid] =
            ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

__global__ __launch_bounds__(AGX_BANDIT_MAX_ARMS) void bandit_select_kernel(BanditArgs a,
                                                                            const double *__restrict__ part, int nct) {
    __shared__ float sc[AGX_BANDIT_MAX_ARMS];
    const int A = a.A, k = threadIdx.x;
    const unsigned long long counter = a.counter ? (unsigned long long)*a.counter : 0ull;
    if (k < A) {
        double q = 0.0;
        for (int c = 0; c < nct; ++c) q += part[(size_t)c * A + k];
        sc[k] = bandit_score(a, k, q, counter);
    }
    __syncthreads();
    if (k < kWave) {
        const int best = bandit_argmax(sc, A, k);
        if (k == 0) bandit_publish(a, best, counter);
    }
}

__device__ __forceinline__ int bandit_taken(const BanditArgs &a) {
    const long long act = *a.action;
    return act < 0 ? 0 : act >= a.A ? a.A - 1 : (int)act;
}

// workgroups [0, ceil(D / 4)): u, a wave per row; the rest: w, a lane per column of a 64-wide tile
__global__ __launch_bounds__(kRowWaves *kWave) void bandit_uw_kernel(BanditArgs a, double *__restrict__ u,
                                                                     double *__restrict__ w) {
    __shared__ double red[kRowWaves][kWave];
    const int D = a.D, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int act = bandit_taken(a);
    const int nu = (D + kRowWaves - 1) / kRowWaves;
    if ((int)blockIdx.x < nu) {
        const int i = blockIdx.x * kRowWaves + wave;
        if (i < D) {
            double s = 0.0;
            for (int j = lane; j < D; j += kWave) s += (double)a.sigma[(size_t)i * D + j] * (double)bandit_g(a, act, j);
            s = wave_sum(s);
            if (lane == 0) u[i] = s;
        }
    } else {
        const int j = ((int)blockIdx.x - nu) * kWave + lane;
        double s = 0.0;
        if (j < D)
            for (int i = wave; i < D; i += kRowWaves)
                s += (double)a.sigma[(size_t)i * D + j] * (double)bandit_g(a, act, i);
        red[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && j < D) w[j] = ((red[0][lane] + red[1][lane]) + red[2][lane]) + red[3][lane];
    }
}

// a wave per row; every wave forms v.u for itself, in the same order
__global__ __launch_bounds__(kRowWaves *kWave) void bandit_update_kernel(BanditArgs a, const double *__restrict__ u,
                                                                         const double *__restrict__ w) {
    const int D = a.D, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int act = bandit_taken(a);
    double vu = 0.0;
    for (int i = lane; i < D; i += kWave) vu += (double)bandit_g(a, act, i) * u[i];
    const double r = 1.0 / (1.0 + wave_sum(vu));
    const int i = blockIdx.x * kRowWaves + wave;
    if (i < D) {
        const double ui = u[i] * r;
        for (int j = lane; j < D; j += kWave) {
            float *p = a.sigma + (size_t)i * D + j;
            *p = (float)((double)*p - ui * w[j]);
        }
    }
}

static int64_t bandit_col_tiles(int64_t D) { return ceil_div(D, kColTile); }
static int64_t bandit_row_tiles(int64_t D) { return ceil_div(D, kRowTile); }

}  // namespace agx

using namespace agx;

extern "C" size_t agx_bandit_workspace_bytes(int64_t A, int64_t D) {
    if (A < 1 || A > AGX_BANDIT_MAX_ARMS || D < 1 || D > AGX_BANDIT_MAX_D) return 0;
    if (D <= AGX_BANDIT_RESIDENT_MAX_D) return 16;
    return (size_t)(2 * D + bandit_col_tiles(D) * bandit_row_tiles(D) * A) * sizeof(double);
}

extern "C" int agx_bandit_select(const float *h, int64_t ldh, const float *mu, float *sigma_inv, const uint8_t *mask,
                                 int64_t A, int64_t H, int bias_one, float scale, float gamma, int mode, uint64_t seed,
                                 int64_t *counter, float *scores, float *quad, int64_t *action, void *workspace,
                                 void *stream) {
    AGX_REQUIRE(mu && sigma_inv && scores && quad && action && workspace, "agx_bandit_select: null pointer");
    AGX_REQUIRE(H >= 0 && (bias_one == 0 || bias_one == 1) && H + bias_one >= 1, "agx_bandit_select: need D >= 1");
    AGX_REQUIRE(h || H == 0, "agx_bandit_select: null h");
    AGX_REQUIRE(ldh >= H, "agx_bandit_select: ldh < H");
    AGX_REQUIRE(mode == 0 || (mode == 1 && counter), "agx_bandit_select: mode is 0 (UCB) or 1 (Thompson, needs counter)");
    const int64_t D = H + bias_one;
    AGX_REQUIRE(A >= 1 && A <= AGX_BANDIT_MAX_ARMS, "agx_bandit_select: need 1 <= A <= %d", AGX_BANDIT_MAX_ARMS);
    AGX_REQUIRE(D <= AGX_BANDIT_MAX_D, "agx_bandit_select: D = %lld exceeds %d", (long long)D, AGX_BANDIT_MAX_D);
    hipStream_t s = as_stream(stream);
    BanditArgs a{h,     ldh,   mu,   sigma_inv, mask, (int)A, (int)H, (int)D,
                 scale, gamma, mode, seed,      reinterpret_cast<long long *>(counter),
                 scores, quad, reinterpret_cast<long long *>(action)};
    if (D <= AGX_BANDIT_RESIDENT_MAX_D) {
        bandit_resident_kernel<<<1, kBanditThreads, bandit_resident_lds(A, D), s>>>(a);
        return check_launch("agx_bandit_select");
    }
    const int64_t nct = bandit_col_tiles(D), nrt = bandit_row_tiles(D);
    double *u = static_cast<double *>(workspace), *w = u + D, *part = w + D;
    bandit_quad_kernel<<<dim3((unsigned)ceil_div(A, kArmTile), (unsigned)nct, (unsigned)nrt), kColTile,
                         (size_t)kArmTile * D * sizeof(float), s>>>(a, part);
    int rc = check_launch("agx_bandit_select quad");
    if (rc) return rc;
    bandit_select_kernel<<<1, AGX_BANDIT_MAX_ARMS, 0, s>>>(a, part, (int)(nct * nrt));
    if ((rc = check_launch("agx_bandit_select selection"))) return rc;
    const unsigned nrow = (unsigned)ceil_div(D, kRowWaves);
    bandit_uw_kernel<<<nrow + (unsigned)ceil_div(D, kWave), kRowWaves * kWave, 0, s>>>(a, u, w);
    if ((rc = check_launch("agx_bandit_select u, w"))) return rc;
    bandit_update_kernel<<<nrow, kRowWaves * kWave, 0, s>>>(a, u, w);
    return check_launch("agx_bandit_select update");
}
