// The conservative Q-learning loss for Discrete actions — agilerl/algorithms/
// cqn.py:234-252 (CQN.learn) and its backward pass down to Q(s):
//   q_t   = max_a Qtgt(s')  |  Qtgt(s')[argmax_a Q(s')] (double)      (td_rules.h: agx_td_target's rules)
//   y     = r + (gamma*q_t)*(1-d)                                      (f32, one rounding per op)
//   lse_i = logsumexp_a Q(s_i) = log(sum_a exp(Q - shift)) + shift     (torch.logsumexp: shift = the row
//           maximum, 0 when that is infinite)
//   loss  = (mean_i lse_i - mean_{i,a} Q(s)) + 0.5 * mean_i (Q(s_i)[a_i] - y_i)^2
//   dloss/dQ[i,a] = exp(Q[i,a] - lse_i) / B - 1/(B*A) + [a == a_i] (Q[i,a_i] - y_i) / B
//           (exp(Q - lse): the softmax as torch's backward of logsumexp forms it)
// A NaN in a row of Q(s) is skipped by the maximum and carried by the exp-sum,
// so the row's lse, its gradient row and the loss are NaN.  The three means
// are f64 sums over fixed-order block partials, rounded to f32 and combined in
// f32 in the reference's order by cqn_finalize.
//
// Two forms.  Every element of Q(s) is read and every element of the gradient
// written, so a lane walking its own row in global memory (td_target_kernel's
// pattern, fine for one gathered element per row) would touch A cache lines
// per load instruction:
//   * A <= kLaneRowMaxA (32): row per lane.  The block's 256 x A tile of Q(s)
//     is contiguous; it is staged in LDS with coalesced loads (16 bytes per lane
//     when the tensors are 16-byte aligned), the row stride padded to an odd
//     number of words so the 32 lanes of a half-wave sit on 32 banks.  Each
//     lane walks its row there and leaves the gradient in place; the tile is
//     stored coalesced.  At most 256 x 33 words = 33 KiB of LDS, under the 64 KiB
//     a block may take, and every lane still has a row to itself.
//   * A > 32: row per wave.  The lanes stride over the columns (coalesced as
//     they are), the row's maximum, exp-sum and next-state argmax are wave
//     reductions.  Above 32 columns a lane's serial walk is longer than the
//     wave's strided one and the LDS tile would no longer fit 256 rows.
#include "td_rules.h"

#include "../../include/agx_cqn.h"

namespace agx {

constexpr int kLaneRowMaxA = 32;
constexpr int kWaveRows = kTdBlock / kWave;  // rows a block of the row-per-wave form holds at a time
constexpr int64_t kWaveMaxBlocks = 4096;     // its grid; the blocks stride over the rows

// torch.logsumexp's shift: the row maximum, 0 when it is infinite
__device__ __forceinline__ float lse_shift(float m) { return __builtin_isinf(m) ? 0.0f : m; }

// dloss/dQ of one element
__device__ __forceinline__ float cqn_grad(float q, float lse, float inv_b, float inv_ba, bool taken, float td) {
    const float gq = expf(q - lse) * inv_b - inv_ba;
    return taken ? gq + td * inv_b : gq;
}

// the block's three sums into part[0 / 1 / 2][blockIdx], for cqn_finalize
__device__ __forceinline__ void cqn_partials(double s_lse, double s_q, double s_sq, double *__restrict__ part) {
    if (block_sum3<kTdBlock>(s_lse, s_q, s_sq)) {
        part[blockIdx.x] = s_lse;
        part[gridDim.x + blockIdx.x] = s_q;
        part[2 * (int64_t)gridDim.x + blockIdx.x] = s_sq;
    }
}

// A lane's walk over the elements of a rows x A tile in steps of a fixed
// stride, as (row, column) and the word of the padded LDS image (row stride
// S): one division when it starts, none per element.
struct TileCursor {
    int row, col, step_rows, step_cols, A, S;
    __device__ __forceinline__ TileCursor(int first, int stride, int A_, int S_) : A(A_), S(S_) {
        row = first / A;
        col = first - row * A;
        step_rows = stride / A;
        step_cols = stride - step_rows * A;
    }
    __device__ __forceinline__ int word() const { return row * S + col; }
    __device__ __forceinline__ void next() {  // one element on
        if (++col == A) {
            col = 0;
            ++row;
        }
    }
    __device__ __forceinline__ void stride() {  // one stride on
        row += step_rows;
        col += step_cols;
        if (col >= A) {
            col -= A;
            ++row;
        }
    }
};

// Row per lane, A <= kLaneRowMaxA.  LDS: kTdBlock * (A | 1) floats (dynamic).
template <bool VEC>
__global__ __launch_bounds__(kTdBlock) void cqn_lane_rows_kernel(
    const float *__restrict__ qno, const float *__restrict__ qnt, const float *__restrict__ qc,
    const int64_t *__restrict__ act, const float *__restrict__ r, const float *__restrict__ d, int64_t B, int A,
    float g, int dbl, float *__restrict__ y, float *__restrict__ g_q, double *__restrict__ part) {
    extern __shared__ float tile[];
    const int S = A | 1;
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTdBlock;
    const int rows = (int)(B - row0 < kTdBlock ? B - row0 : kTdBlock);
    const int n = rows * A;
    const float *src = qc + row0 * A;
    float *dst = g_q + row0 * A;
    const int n4 = VEC ? n >> 2 : 0;  // row0 * A is a multiple of 256 words: the tile is as aligned as the tensor

    // element 4 k of lane tid's k-th vector; the scalar tail starts at 4 n4 + tid
    TileCursor vec(4 * tid, 4 * kTdBlock, A, S);
    for (int k = tid; k < n4; k += kTdBlock, vec.stride()) {
        const f4 v = reinterpret_cast<const f4 *>(src)[k];
        TileCursor c = vec;
#pragma unroll
        for (int j = 0; j < 4; ++j, c.next()) tile[c.word()] = v[j];
    }
    TileCursor tail(4 * n4 + tid, kTdBlock, A, S);
    for (int e = 4 * n4 + tid; e < n; e += kTdBlock, tail.stride()) tile[tail.word()] = src[e];
    __syncthreads();

    double s_lse = 0.0, s_q = 0.0, s_sq = 0.0;
    if (tid < rows) {
        const int64_t i = row0 + tid;
        float *q = tile + tid * S;
        const float qt = row_q_next(dbl ? qno + i * A : nullptr, qnt + i * A, A, dbl);
        const float yi = td_y(r[i], g, qt, d[i]);
        y[i] = yi;
        float m = q[0];
        for (int a = 1; a < A; ++a) m = fmaxf(m, q[a]);
        const float shift = lse_shift(m);
        float sum = 0.0f;
        for (int a = 0; a < A; ++a) {
            const float v = q[a];
            sum += expf(v - shift);
            s_q += (double)v;
        }
        const float lse = logf(sum) + shift;
        const int ai = (int)act[i];
        const float qa = q[ai];
        const float td = qa - yi;
        const float inv_b = 1.0f / (float)B, inv_ba = 1.0f / ((float)B * (float)A);
        for (int a = 0; a < A; ++a) q[a] = cqn_grad(q[a], lse, inv_b, inv_ba, a == ai, td);
        const double dd = (double)qa - (double)yi;
        s_lse = (double)lse;
        s_sq = dd * dd;
    }
    __syncthreads();

    vec = TileCursor(4 * tid, 4 * kTdBlock, A, S);
    for (int k = tid; k < n4; k += kTdBlock, vec.stride()) {
        f4 v;
        TileCursor c = vec;
#pragma unroll
        for (int j = 0; j < 4; ++j, c.next()) v[j] = tile[c.word()];
        reinterpret_cast<f4 *>(dst)[k] = v;
    }
    tail = TileCursor(4 * n4 + tid, kTdBlock, A, S);
    for (int e = 4 * n4 + tid; e < n; e += kTdBlock, tail.stride()) dst[e] = tile[tail.word()];
    cqn_partials(s_lse, s_q, s_sq, part);
}

// torch.argmax over a row split among lanes: does (ov, oi) come before (bv, bi)?
// A NaN is the largest value; equal values (and two NaNs) go to the lower
// index; an index of INT32_MAX marks a lane that saw no column.
__device__ __forceinline__ bool argmax_before(float ov, int oi, float bv, int bi) {
    if (oi == 0x7fffffff) return false;
    if (bi == 0x7fffffff) return true;
    if (argmax_takes(ov, bv)) return true;
    return oi < bi && (ov == bv || (ov != ov && bv != bv));
}

// Row per wave, A > kLaneRowMaxA: the block's waves stride over the rows.
__global__ __launch_bounds__(kTdBlock) void cqn_wave_rows_kernel(
    const float *__restrict__ qno, const float *__restrict__ qnt, const float *__restrict__ qc,
    const int64_t *__restrict__ act, const float *__restrict__ r, const float *__restrict__ d, int64_t B, int A,
    float g, int dbl, float *__restrict__ y, float *__restrict__ g_q, double *__restrict__ part) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    const float inv_b = 1.0f / (float)B, inv_ba = 1.0f / ((float)B * (float)A);
    double s_lse = 0.0, s_q = 0.0, s_sq = 0.0;  // summed over the wave's rows in lane 0
    for (int64_t i = (int64_t)blockIdx.x * kWaveRows + wave; i < B; i += (int64_t)gridDim.x * kWaveRows) {
        const float *q = qc + i * A;
        const float *tn = qnt + i * A;
        float qt;
        if (dbl) {
            const float *on = qno + i * A;
            float bv = 0.0f;
            int bi = 0x7fffffff;
            for (int c = lane; c < A; c += kWave) {
                const float v = on[c];
                if (bi == 0x7fffffff || argmax_takes(v, bv)) {
                    bv = v;
                    bi = c;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (argmax_before(ov, oi, bv, bi)) {
                    bv = ov;
                    bi = oi;
                }
            }
            qt = tn[bi];  // A > 0: some lane saw a column, so 0 <= bi < A in every lane
        } else {
            qt = -__builtin_inff();
            for (int c = lane; c < A; c += kWave) qt = nan_max(qt, tn[c]);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) qt = nan_max(qt, __shfl_xor(qt, o, 64));
        }
        const float yi = td_y(r[i], g, qt, d[i]);

        float m = -__builtin_inff();
        for (int c = lane; c < A; c += kWave) m = fmaxf(m, q[c]);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
        const float shift = lse_shift(m);
        float sum = 0.0f;
        double sq = 0.0;
        for (int c = lane; c < A; c += kWave) {
            const float v = q[c];
            sum += expf(v - shift);
            sq += (double)v;
        }
        sum = wave_sum(sum);
        sq = wave_sum(sq);
        const float lse = logf(sum) + shift;
        const int ai = (int)act[i];
        const float qa = q[ai];
        const float td = qa - yi;
        float *gr = g_q + i * A;
        for (int c = lane; c < A; c += kWave) gr[c] = cqn_grad(q[c], lse, inv_b, inv_ba, c == ai, td);
        if (lane == 0) {
            y[i] = yi;
            const double dd = (double)qa - (double)yi;
            s_lse += (double)lse;
            s_q += sq;
            s_sq += dd * dd;
        }
    }
    cqn_partials(s_lse, s_q, s_sq, part);
}

// terms = f32 of the three means, loss = (terms[0] - terms[1]) + 0.5f * terms[2]; one block of 1024
__global__ __launch_bounds__(1024) void cqn_finalize(const double *__restrict__ part, int64_t nblk, int64_t B, int A,
                                                     float *__restrict__ loss, float *__restrict__ terms) {
    double s_lse = 0.0, s_q = 0.0, s_sq = 0.0;
    for (int64_t i = threadIdx.x; i < nblk; i += 1024) {
        s_lse += part[i];
        s_q += part[nblk + i];
        s_sq += part[2 * nblk + i];
    }
    if (block_sum3<1024>(s_lse, s_q, s_sq)) {
        const float mean_lse = (float)(s_lse / (double)B);
        const float mean_q = (float)(s_q / ((double)B * (double)A));
        const float mse = (float)(s_sq / (double)B);
        const float cql1 = mean_lse - mean_q;
        *loss = cql1 + 0.5f * mse;
        if (terms) {
            terms[0] = mean_lse;
            terms[1] = mean_q;
            terms[2] = mse;
        }
    }
}

static int64_t cqn_blocks(int64_t B, int64_t A) {
    if (A <= kLaneRowMaxA) return ceil_div(B, kTdBlock);
    const int64_t n = ceil_div(B, kWaveRows);
    return n < kWaveMaxBlocks ? n : kWaveMaxBlocks;
}

}  // namespace agx

using namespace agx;

extern "C" size_t agx_cqn_workspace_bytes(int64_t B, int64_t A) {
    return B > 0 && A > 0 ? (size_t)cqn_blocks(B, A) * 3 * sizeof(double) : 0;
}

extern "C" int agx_cqn_loss(const float *q_next_online, const float *q_next_target, const float *q_cur,
                            const int64_t *actions, const float *rewards, const float *dones, int64_t B, int64_t A,
                            double gamma, int double_q, float *y, float *g_q, float *loss, float *terms,
                            void *workspace, void *stream) {
    AGX_REQUIRE(q_next_target && q_cur && actions && rewards && dones && y && g_q && loss && workspace,
                "agx_cqn_loss: null pointer");
    AGX_REQUIRE(B >= 0 && A > 0 && A < 65536, "agx_cqn_loss: need B >= 0 and 0 < A < 65536");
    AGX_REQUIRE(!double_q || q_next_online, "agx_cqn_loss: double_q needs q_next_online");
    AGX_REQUIRE(B <= (int64_t)0x7fffffff * kTdBlock, "agx_cqn_loss: B exceeds the grid");
    if (B == 0) return AGX_OK;
    hipStream_t s = as_stream(stream);
    const int64_t nblk = cqn_blocks(B, A);
    double *part = static_cast<double *>(workspace);
    if (A <= kLaneRowMaxA) {
        const size_t lds = (size_t)kTdBlock * ((size_t)A | 1) * sizeof(float);
        const bool vec = (((uintptr_t)q_cur | (uintptr_t)g_q) & 15) == 0;
        auto kernel = vec ? cqn_lane_rows_kernel<true> : cqn_lane_rows_kernel<false>;
        kernel<<<(unsigned)nblk, kTdBlock, lds, s>>>(q_next_online, q_next_target, q_cur, actions, rewards, dones, B,
                                                     (int)A, (float)gamma, double_q, y, g_q, part);
    } else {
        cqn_wave_rows_kernel<<<(unsigned)nblk, kTdBlock, 0, s>>>(q_next_online, q_next_target, q_cur, actions,
                                                                 rewards, dones, B, (int)A, (float)gamma, double_q,
                                                                 y, g_q, part);
    }
    int rc = check_launch("agx_cqn_loss");
    if (rc) return rc;
    cqn_finalize<<<1, 1024, 0, s>>>(part, nblk, B, (int)A, loss, terms);
    return check_launch("agx_cqn_loss sums");
}
