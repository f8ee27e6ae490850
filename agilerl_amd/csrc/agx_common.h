// Internal helpers shared by the libagx.so translation units (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/agx.h"

namespace agx {

// persistent-rollout control block (agx.h agx_rollout_ctl): header, nwg done
// words, then one 64-byte release line per workgroup
__host__ __device__ inline unsigned *rollout_done_words(void *ctl) { return static_cast<unsigned *>(ctl) + 4; }
__host__ __device__ inline unsigned rollout_release_offset(unsigned nwg, unsigned w) {  // in words
    return ((4 + nwg + 15) / 16 + w) * 16;
}
__host__ __device__ inline unsigned *rollout_release_word(void *ctl, unsigned nwg, unsigned w) {
    return static_cast<unsigned *>(ctl) + rollout_release_offset(nwg, w);
}

// thread-local last error (agx_last_error)
void set_error(const char *fmt, ...);

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Check the launch that was just queued; never synchronises.
inline int check_launch(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        set_error("%s: %s", what, hipGetErrorString(e));
        return AGX_EHIP;
    }
    return AGX_OK;
}

#define AGX_REQUIRE(cond, ...)          \
    do {                                \
        if (!(cond)) {                  \
            ::agx::set_error(__VA_ARGS__); \
            return AGX_EINVAL;          \
        }                               \
    } while (0)

constexpr int kWave = 64;

// ---- wave-level reductions (64 lanes, xor butterflies) ------------------
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// reduce within aligned groups of G lanes (G power of two <= 64)
template <int G, typename T>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- lane helpers ------------------------------------------------------------
typedef float f4 __attribute__((ext_vector_type(4)));

template <int C>
__device__ __forceinline__ float dpp(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), C, 0xf, 0xf, true));
}
// sum / max over the 16 lanes of a DPP row; result in every lane of the row
__device__ __forceinline__ float row_sum(float v) {
    v += dpp<0xb1>(v);   // quad_perm [1,0,3,2]
    v += dpp<0x4e>(v);   // quad_perm [2,3,0,1]
    v += dpp<0x141>(v);  // row_half_mirror
    v += dpp<0x140>(v);  // row_mirror
    return v;
}
__device__ __forceinline__ float row_max(float v) {
    v = fmaxf(v, dpp<0xb1>(v));
    v = fmaxf(v, dpp<0x4e>(v));
    v = fmaxf(v, dpp<0x141>(v));
    v = fmaxf(v, dpp<0x140>(v));
    return v;
}
// v of lane `lane`
__device__ __forceinline__ float bperm(int lane, float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(lane << 2, __builtin_bit_cast(int, v)));
}
__device__ __forceinline__ float relu(float x) { return x > 0.f ? x : 0.f; }

inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the device's CU count, queried once (runtime.hip)
int cu_count();

}  // namespace agx
