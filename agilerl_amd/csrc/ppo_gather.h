// The gather prologue of every fused PPO learner (learner.hip, graph_learner.hip):
// the rollout SoA permuted into minibatch order, the advantages normalised, the
// learner's counters zeroed.  One kernel over a per-head action packer:
//
//   struct Pack {  // passed by value to the kernel
//       using Elem = ...;  // element type of the rollout's stored actions
//       using Word = ...;  // 4-byte type of the gathered action words (gact)
//       // 4-byte words of a gathered row, for an actor of A outputs
//       static constexpr int words(int A);
//       // gathered row dst's words from rollout row sp's stored action
//       __device__ void operator()(const Elem *act, size_t sp, int A, Word *gact, size_t dst) const;
//   };
#pragma once

#include "../../include/agx_multi.h"
#include "agx_common.h"

namespace agx {
namespace {

// categorical: the int64 action index [P][S] as one int
struct CatPack {
    using Elem = long long;
    using Word = int;
    static constexpr int words(int) { return 1; }
    __device__ __forceinline__ void operator()(const Elem *act, size_t sp, int, Word *gact, size_t dst) const {
        gact[dst] = (int)act[sp];
    }
};

// Gaussian: the float actions [P][S][A], copied
struct GaussPack {
    using Elem = float;
    using Word = float;
    static constexpr int words(int A) { return A; }
    __device__ __forceinline__ void operator()(const Elem *act, size_t sp, int A, Word *gact, size_t dst) const {
        for (int d = 0; d < A; ++d) gact[dst * A + d] = act[sp * A + d];
    }
};

// multi-categorical: the int64 actions [P][S][K] packed into one target word
// (bit off_k + a_k set for every component, a_k clamped into [0, n_k): never a
// bit outside the component)
struct MultiPack {
    using Elem = long long;
    using Word = unsigned;
    agx_multi_head head;
    static constexpr int words(int) { return 1; }
    __device__ __forceinline__ void operator()(const Elem *act, size_t sp, int, Word *gact, size_t dst) const {
        const int K = head.K;
        unsigned tgt = 0;
        int off = 0;
        for (int k = 0; k < K; ++k) {
            const int n = head.nvec[k];
            long long a = act[sp * K + k];
            a = a < 0 ? 0 : (a >= n ? n - 1 : a);
            tgt |= 1u << (off + (int)a);
            off += n;
        }
        gact[dst] = tgt;
    }
};

// Bernoulli: the int64 actions [P][S][n] packed into one target word (bit j = a_j != 0)
struct BernPack {
    using Elem = long long;
    using Word = unsigned;
    static constexpr int words(int) { return 1; }
    __device__ __forceinline__ void operator()(const Elem *act, size_t sp, int n, Word *gact, size_t dst) const {
        unsigned tgt = 0;
        for (int a = 0; a < n; ++a) tgt |= (act[sp * n + a] != 0 ? 1u : 0u) << a;
        gact[dst] = tgt;
    }
};

// Block (x, e * P + p), thread j: row j of agent p's epoch-e order.  masks (or
// null; a Gaussian head has none): the flat legal-action masks [P][S][A].
template <class Pack>
__global__ void ppo_gather_kernel(const float *__restrict__ obs, const typename Pack::Elem *__restrict__ act,
                                  const float *__restrict__ old_logp, const float *__restrict__ adv,
                                  const float *__restrict__ ret, const float *__restrict__ old_v,
                                  const double *__restrict__ adv_stats, const long long *__restrict__ perms,
                                  const unsigned char *__restrict__ masks, int A, const Pack pack, long long S, int D,
                                  int P, float *__restrict__ gobs, typename Pack::Word *__restrict__ gact,
                                  unsigned *__restrict__ gmask, float *__restrict__ grow,
                                  unsigned *__restrict__ counters, int ncounters, const int *__restrict__ epochs_p,
                                  unsigned *__restrict__ err) {
    const int ep = blockIdx.y;  // e * P + p
    const int p = ep % P;
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    // the learner's arrival counters + timeout word (stream-ordered before it;
    // replaces a separate memset launch) and its tagged hand-off words, spread
    // over the blocks of the first (epoch, agent) row
    if (blockIdx.y == 0)
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ncounters; i += gridDim.x * blockDim.x)
            counters[i] = 0u;
    if (j >= S) return;
    // epochs beyond an agent's own update_epochs: the learner never reads
    // them, and their perms rows are not part of the contract (agx.h)
    if (epochs_p && ep / P >= epochs_p[p]) return;
    long long src = perms[(size_t)ep * S + j];
    if (src < 0 || src >= S) {
        // a host-side slip must not become a device fault: flag it in the
        // caller's sticky error word (bit 2; PPOPopulation.check_errors raises
        // AgxError) and gather row 0 in its place
        if (err) __hip_atomic_fetch_or(err, AGX_LEARN_ERR_PERM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        src = 0;
    }
    const size_t sp = (size_t)p * S + src, dst = (size_t)ep * S + j;
    for (int d = 0; d < D; ++d) gobs[dst * D + d] = obs[sp * D + d];
    pack(act, sp, A, gact, dst);
    if (masks) {  // [P][S][A] u8 -> one bit per logit
        unsigned bits = 0;
        for (int a = 0; a < A; ++a) bits |= (masks[sp * A + a] != 0 ? 1u : 0u) << a;
        gmask[dst] = bits;
    }
    float *gr = grow + (size_t)ep * 4 * S;
    double a = adv[sp];
    if (adv_stats) a = (a - adv_stats[2 * p]) * (1.0 / (adv_stats[2 * p + 1] + 1e-8));  // == adv_normalize_kernel
    gr[j] = old_logp[sp];
    gr[S + j] = (float)a;
    gr[2 * S + j] = ret[sp];
    gr[3 * S + j] = old_v[sp];
}

// agx_ppo_learn_args.adv_norm_minibatch: the gathered advantages normalised
// minibatch by minibatch (ippo.py:780-783), in place, after ppo_gather_kernel.
// Block (m, e * P + p): rows [m B, min((m + 1) B, S)) of agent p's epoch-e
// order, the rows the learner's minibatch m reads.  Two passes, mean then
// unbiased standard deviation, each an f64 sum in a fixed order (a thread's
// rows ascending, the xor butterfly of its wave, the waves ascending), then
// (a - mean) / (std + 1e-8) in f64, rounded to f32 once as ppo_gather_kernel's
// adv_stats form is.  A minibatch of fewer than two rows has no unbiased std
// (the host rejects the sizes that produce one) and is left as gathered.
constexpr int kNormThreads = 256;
__device__ __forceinline__ double norm_block_sum(double v, double *part) {
    v = wave_sum(v);
    __syncthreads();  // the previous sum's readers are done with part
    if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = v;
    __syncthreads();
    double s = part[0];
    for (int w = 1; w < kNormThreads / kWave; ++w) s += part[w];
    return s;
}

__global__ __launch_bounds__(kNormThreads) void ppo_adv_norm_minibatch_kernel(float *__restrict__ grow, long long S,
                                                                              long long B, int P,
                                                                              const int *__restrict__ epochs_p) {
    __shared__ double part[kNormThreads / kWave];
    const int ep = blockIdx.y;  // e * P + p
    if (epochs_p && ep / P >= epochs_p[ep % P]) return;  // rows the learner never reads (uniform over the block)
    const long long lo = (long long)blockIdx.x * B;
    const long long hi = lo + B < S ? lo + B : S;
    const long long n = hi - lo;
    if (n < 2) return;
    float *a = grow + (size_t)ep * 4 * S + S + lo;
    double s = 0.0;
    for (long long i = threadIdx.x; i < n; i += kNormThreads) s += (double)a[i];
    const double mean = norm_block_sum(s, part) / (double)n;
    double q = 0.0;
    for (long long i = threadIdx.x; i < n; i += kNormThreads) {
        const double c = (double)a[i] - mean;
        q += c * c;
    }
    const double denom = sqrt(norm_block_sum(q, part) / (double)(n - 1)) + 1e-8;
    for (long long i = threadIdx.x; i < n; i += kNormThreads) a[i] = (float)(((double)a[i] - mean) / denom);
}

// The host-side rules of the flag, before any launch (`what`: the entry point).
inline int adv_norm_minibatch_check(const char *what, const agx_ppo_learn_args *x) {
    if (!x->adv_norm_minibatch) return AGX_OK;
    AGX_REQUIRE(!x->adv_stats, "%s: adv_norm_minibatch normalises the advantages itself: adv_stats must be NULL",
                what);
    if (x->batch_per_agent) {
        set_error("%s: adv_norm_minibatch with batch_per_agent is not supported", what);
        return AGX_EUNSUPPORTED;
    }
    const long long bb = x->batch < x->S ? x->batch : x->S;
    AGX_REQUIRE(bb > 1 && x->S % bb != 1,
                "%s: adv_norm_minibatch: S=%lld, batch=%lld leave a one-row minibatch, which has no unbiased std",
                what, (long long)x->S, (long long)x->batch);
    return AGX_OK;
}

}  // namespace
}  // namespace agx
