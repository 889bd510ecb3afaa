// lws_bin.h -- device vocabulary of the order-exact engines: the statements of the reference's tap loop and the write-back of a bin,
// written once.  lws_generic.hip is the engine whose bits the others promise -- the serial online kernels (lws_online.hip), the one-lane
// no-future kernel (lws_nofuture.hip), the fp64 online kernels (lws_online64.hip), the team engine with one lane per bin and its ordered
// kernel (lws_team.hip) -- and that promise holds because they all inline this text, under -ffp-contract=off (Makefile).
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

namespace lws {

// a += w*b + conj(w)*c in the grouped form of lwslib.cpp:310-311: cancels exactly when c == conj(b)
// (Hermitian images / real input), which keeps ill-conditioned bins in step with the CPU arithmetic.
template <typename C> __device__ __forceinline__ void pair(C &a, const C w, const C b, const C c) {
    a.x += w.x * (b.x + c.x) - w.y * (b.y - c.y);
    a.y += w.x * (b.y + c.y) + w.y * (b.x - c.x);
}
template <typename C> __device__ __forceinline__ void mac(C &a, const C w, const C s) {   // a += w * s
    a.x += w.x * s.x - w.y * s.y;
    a.y += w.x * s.y + w.y * s.x;
}
template <typename C> __device__ __forceinline__ void macc(C &a, const C w, const C s) {  // a += conj(w) * s
    a.x += w.x * s.x + w.y * s.y;
    a.y += w.x * s.y - w.y * s.x;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>), in that order
template <int... Is, typename F_>
__device__ __forceinline__ void static_for_impl(std::integer_sequence<int, Is...>, F_ &&f) {
    (f(std::integral_constant<int, Is>{}), ...);
}
template <int N_, typename F_> __device__ __forceinline__ void static_for(F_ &&f) {
    static_for_impl(std::make_integer_sequence<int, N_>{}, static_cast<F_ &&>(f));
}

// c ? a : b per component (a select, where `c ? p[i] : zero` would make the compiler branch around the load)
template <typename C> __device__ __forceinline__ C sel(bool c, C a, C b) { C r; r.x = c ? a.x : b.x; r.y = c ? a.y : b.y; return r; }

// sum over the Q adjacent lanes of a group (Q = 2, 4, 8, 16; groups are aligned), in data-parallel-primitive moves
template <int Q> __device__ __forceinline__ float group_sum(float v) {
    auto dpp = [](float x, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), decltype(ctrl)::value, 0xf, 0xf, true));
    };
    v += dpp(v, std::integral_constant<int, 0xB1>());                    // quad_perm [1,0,3,2]
    if constexpr (Q >= 4) v += dpp(v, std::integral_constant<int, 0x4E>());   // quad_perm [2,3,0,1]
    if constexpr (Q >= 8) v += dpp(v, std::integral_constant<int, 0x141>());  // row_half_mirror: the other quad of the 8
    if constexpr (Q >= 16) v += dpp(v, std::integral_constant<int, 0x140>()); // row_mirror: the other half of the 16
    return v;
}

// |a| of a weighted sum about to be re-projected on its target magnitude (lwslib.cpp:356-360: a -> target a / |a|).  In fp32 a sum of
// data near 1e-20 squares to a denormal or to zero -- the bin is then left alone as if its neighbourhood were silent -- and one near
// 1e+20 to infinity -- the bin is then written as zero.  Such a sum is first multiplied by the power of two that brings its larger
// component to [1, 2) (exact; the quotient a / |a| does not see it), so that "|a| > 0" keeps its meaning and the result stays finite
// for any normal fp32 data.  A sum whose square is between 1e-30 and 1e+30 -- any sum of data at ordinary scales -- goes through
// unchanged: the same operations on the same values as before, no bit moves.  fp64 sums have the range as they are.
template <typename real, typename C> __device__ __forceinline__ real rescued_norm(C &a) {
    real m2 = a.x * a.x + a.y * a.y;
    if constexpr (sizeof(real) == 4) {
        if (!(m2 >= 1e-30f && m2 <= 1e30f)) {
            const float big = fmaxf(fabsf(a.x), fabsf(a.y));
            const unsigned e = (__float_as_uint(big) >> 23) & 0xffu;
            // (a zero or denormal component pair stays as it is: m2 is 0 again and the bin is left alone; infinities and NaN too)
            const float s = (e == 0u || e == 0xffu) ? 1.0f : __uint_as_float((e >= 254u ? 1u : 254u - e) << 23);
            a.x *= s; a.y *= s;
            m2 = a.x * a.x + a.y * a.y;
        }
    }
    return sqrt(m2);
}

// The exact write-back of a bin whose weighted sum is `acc` (lwslib.cpp:356-367): |acc|, nothing if that is not above zero, else
// v = acc target / |acc| into the bin and conj(v) into its Hermitian image in the low or the high pad column.  The bin is column n of
// its extended frame (F + 2L columns; nyq = F + L - 1) and element `at` of `base`, in global memory or in an LDS ring, a column
// further on `stride` elements further on (1; a whole row in the time-skewed copy of the batch engine).  `at` is an index into
// whatever the caller has a pointer to, not the column: (S, m_ext * Np + n, n, ...) for a spectrogram in memory or a whole ring,
// (cur, n, n, ...) where `cur` is the bin's own frame -- there the two coincide -- and (SW + lane, row, n, ..., NL) in the skewed
// copy, whose element (row, lane) is SW[row * NL + lane].  Base and index rather than a pointer to the bin: that is how the engines
// addressed these stores before they shared this text, and the compiler's registers follow the form.  The threshold test and
// the load of `target` are the caller's: engines order them differently against the sum.  RESCUE = false: the plain square root
// (fp64: the same code either way).
template <typename real, bool RESCUE = true, typename C, typename I>
__device__ __forceinline__ void finish_bin(C *base, I at, int n, int F, int L, C acc, real target, int stride = 1) {
    real mag;
    if constexpr (RESCUE) mag = rescued_norm<real>(acc);
    else mag = sqrt(acc.x * acc.x + acc.y * acc.y);
    if (!(mag > 0)) return;
    C v;
    v.x = acc.x * target / mag;
    v.y = acc.y * target / mag;
    base[at * stride] = v;
    const int nyq = F + L - 1;
    C vc;
    vc.x = v.x; vc.y = -v.y;
    if (n >= L + 1 && n < 2 * L + 1) base[(at + 2 * (L - n)) * stride] = vc;
    else if (n >= F - 1 && n < nyq) base[(at + 2 * (nyq - n)) * stride] = vc;
}

}  // namespace lws
