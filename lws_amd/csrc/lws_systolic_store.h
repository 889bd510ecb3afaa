// lws_systolic_store.h -- the storage formats of the systolic engine's skewed HBM layout, shared by the update kernel
// (lws_systolic.hip, every build) and the layout passes (lws_systolic_layout.h); MAX_ITERS comes with lws_systolic_geom.h.
// H16 = false: float2 state, float magnitudes (20 B per active bin and sweep).  H16 = true (LWS_STORAGE_FP16): half2 state
// and half magnitudes (10 B), both multiplied by store_scale(largest magnitude of the spectrogram), a power of two that
// brings the data to [0, 2): exact, and the whole kernel then works in that scaled domain (its thresholds are scaled the
// same way; the weighted sums are only ever normalised, so nothing else changes).  Arithmetic and the LDS rings are fp32
// in both formats; the rounding to half happens once per pass over HBM (NSLOTS sweeps).
#pragma once
#include <hip/hip_runtime.h>

#include "lws_systolic_geom.h"

namespace lws {

typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
__host__ __device__ __forceinline__ float store_scale(float amax) {
    unsigned b;
    __builtin_memcpy(&b, &amax, 4);
    const unsigned e = (b >> 23) & 0xffu;
    const unsigned sb = (e == 0u || e == 0xffu) ? 0x3f800000u : ((e >= 254u ? 1u : 254u - e) << 23);
    float sc;
    __builtin_memcpy(&sc, &sb, 4);
    return sc;
}
__device__ __forceinline__ float2 unpack_h2(unsigned u) {
    const h2_t h = __builtin_bit_cast(h2_t, u);
    return make_float2((float)h.x, (float)h.y);
}
__device__ __forceinline__ unsigned pack_h2(float2 v) {   // round to nearest even
    const h2_t h = {(_Float16)v.x, (_Float16)v.y};
    return __builtin_bit_cast(unsigned, h);
}
__device__ __forceinline__ float unpack_h(unsigned short u) { return (float)__builtin_bit_cast(_Float16, u); }
__device__ __forceinline__ unsigned short pack_h(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }
template <bool H16> struct Store {
    using cplx = float2; using real = float;
    static constexpr int CB = 8, RB = 4;
};
template <> struct Store<true> {
    using cplx = unsigned; using real = unsigned short;
    static constexpr int CB = 4, RB = 2;
};

}  // namespace lws
