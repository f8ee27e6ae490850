// IPPO's generalised advantage estimate (include/agx_ippo.h): the float32 op
// sequence of agilerl/algorithms/ippo.py:702-725 for every agent group of a
// learn call in one launch.
#include "../../include/agx_ippo.h"
#include "agx_common.h"

namespace agx {
namespace {

constexpr int kMaxIppo = AGX_IPPO_MAX_SEGMENTS;
struct IppoGaeSet {
    agx_ippo_gae_segment s[kMaxIppo];
};

// blockIdx.y = segment, one lane per column m, T serial steps from the last
// row up; a row's loads and stores are coalesced along M.  Every expression
// is one float32 operation per torch op (the build has -ffp-contract=off).
__global__ __launch_bounds__(256) void ippo_gae_kernel(IppoGaeSet set, long long T, float g, float gl) {
    const agx_ippo_gae_segment &S = set.s[blockIdx.y];
    const long long M = S.M;
    const long long m = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= M) return;
    const float *__restrict__ r = S.rewards;
    const float *__restrict__ d = S.dones;
    const float *__restrict__ v = S.values;
    float *__restrict__ adv = S.advantages;
    float *__restrict__ ret = S.returns;
    float nd = S.next_done[m], nv = S.next_value[m];
    float last = 0.0f;
    for (long long t = T - 1; t >= 0; --t) {
        const size_t i = (size_t)t * (size_t)M + (size_t)m;
        const float vt = v[i];
        const float nnt = 1.0f - nd;
        const float delta = (r[i] + (g * nv) * nnt) - vt;
        last = delta + (gl * nnt) * last;
        adv[i] = last;
        ret[i] = last + vt;
        nd = d[i];
        nv = vt;
    }
}

}  // namespace
}  // namespace agx

using namespace agx;

extern "C" int agx_ippo_gae(const agx_ippo_gae_segment *segments, int n_segments, int64_t T, double gamma,
                            double gae_lambda, void *stream) {
    AGX_REQUIRE(n_segments >= 0 && n_segments <= kMaxIppo && (segments || n_segments == 0),
                "agx_ippo_gae: bad segment list (n=%d, max %d)", n_segments, kMaxIppo);
    AGX_REQUIRE(T > 0, "agx_ippo_gae: T=%lld must be positive", (long long)T);
    IppoGaeSet set = {};
    int64_t most = 0;
    for (int k = 0; k < n_segments; ++k) {
        const agx_ippo_gae_segment &S = segments[k];
        AGX_REQUIRE(S.M >= 0, "agx_ippo_gae: segment %d: M=%lld is negative", k, (long long)S.M);
        if (S.M == 0) continue;  // skipped: set.s[k].M stays 0
        AGX_REQUIRE(S.rewards && S.dones && S.values && S.next_value && S.next_done && S.advantages && S.returns,
                    "agx_ippo_gae: segment %d: null pointer", k);
        AGX_REQUIRE(S.M < (1ll << 31) * 256, "agx_ippo_gae: segment %d: M=%lld too large", k, (long long)S.M);
        set.s[k] = S;
        most = S.M > most ? S.M : most;
    }
    if (most == 0) return AGX_OK;  // nothing to compute
    ippo_gae_kernel<<<dim3((unsigned)ceil_div(most, 256), (unsigned)n_segments), 256, 0, as_stream(stream)>>>(
        set, (long long)T, (float)gamma, (float)(gamma * gae_lambda));
    return check_launch("agx_ippo_gae");
}
