// lws_misi_la_kernels.h -- the one-shot kernel of online MISI (k_misi_la), part of the one translation unit lws_gla.hip (whose header
// comment is the map of these files).
#pragma once

#include "lws_rtisi_kernels.h"   // RtisiArgs, rtisi_sample, rtisi_project, rtisi_put_pair

namespace {

// ---- Online MISI: the K sources of a mixture under a look-ahead, MISI as k_rtisi is Griffin-Lim.  One workgroup per MIXTURE marches
// over the frames; inside each stage its sources are taken one after another.  The state is K copies of k_rtisi's (ring_k, fcur_k,
// fnxt_k), and over the active window of R samples, sample hop m + d at index d:
//   target : keep g_last y, once per commit step.  g_last = num / den (1 where den == 0) is the share of a sample's overlap-add weight
//            w = awin swin that has entered: den sums w over every frame that covers the sample, ascending, num is that sum as it stood
//            behind frame `last` -- from the two device windows, no table;
//   xs     : [K][R], x_k = y_k + delta with delta = (target - sum_k y_k) / K (k ascending), every y_k gathered by rtisi_sample once per
//            inner iteration, before any fnxt is written; the forward load of frame j is xs_k[hop (j - m) + n] awin[n].
// A thread owns the indices d = threadIdx.x + i blockDim.x of target and of all K rows of xs in every loop that writes them, so
// target needs no barrier of its own and y_k becomes x_k in place.  Loops that enclose a barrier run over m, it, k, j and the
// direction: kernel arguments and counters derived from them alone.
struct MisiLaArgs {
    RtisiArgs r;         // r.state_floats: the state of ONE source, R + 2 (LA + 1) N; r.len: samples of the mixture and of each signal
    int K;
    size_t all_floats;   // K r.state_floats + (K + 1) R: the scratch slice of a workgroup
};

// The bins k = threadIdx.x + i blockDim.x of one frame that a thread holds in registers: F <= blockDim.x up to N = 1024, and
// blockDim.x = RTISI_MAX_THREADS above (la_placement)
constexpr int RTISI_BINS = (MAXN / 2 + 1 + RTISI_MAX_THREADS - 1) / RTISI_MAX_THREADS;

// the unit phasor rtisi_project scales: (1, 0) where X == 0
__device__ __forceinline__ float2 rtisi_phasor(float2 X) {
    const float mag = sqrtf(X.x * X.x + X.y * X.y);
    return mag > 0.f ? make_float2(X.x / mag, X.y / mag) : make_float2(1.f, 0.f);
}

// START (lws_hip.h's LWS_START_*) is how a frame enters in pass 0.  GIVEN: f_kj = inv(S_kj), two frames per transform, source by
// source.  MIXTURE: c_kj = A_kj X / |X| with X = fwd(keep y under frame j), ONE forward transform per entering frame for all K
// sources -- its phasors X / |X| wait in registers (RTISI_BINS bins per thread) while the K inverse transforms take the transform
// buffers -- then f_kj = inv(c_kj), one frame per transform.  S is not read; without iterations c_kj goes where S_kj was.  A template
// parameter with a block of its own, so that the GIVEN instances are the code they were.
template <bool IN_LDS, int START>
__global__ void __launch_bounds__(RTISI_MAX_THREADS) k_misi_la(float2 *C, const float *A, const float *Y, float *xout, const float *awin,
                                                               const float *swin, float *scratch, MisiLaArgs q) {
    extern __shared__ float2 lds[];
    const RtisiArgs a = q.r;
    const int b = blockIdx.x, K = q.K, N = a.N, F = N / 2 + 1, hop = a.hop, M = a.M, W = a.LA + 1, R = N + a.LA * hop;
    const int t_end = hop * (M - 1) + N - a.zero_hi;
    float2 *bufA = lds, *bufB = lds + N, *bufC = lds + 2 * N;   // as in k_rtisi
    float *state = IN_LDS ? reinterpret_cast<float *>(lds + (a.odd > 1 ? 3 : 2) * N) : scratch + (size_t)b * q.all_floats;
    float *target = state + (size_t)K * a.state_floats, *xs = target + R;
    size_t cur = R, nxt = R + (size_t)W * N;   // fcur and fnxt within the state of a source; its ring is at 0
    float2 *Cb = C + (size_t)b * K * M * F;
    const float *Ab = A ? A + (size_t)b * K * M * F : nullptr;   // null without iterations, and not read then
    const float *yb = Y + (size_t)b * a.len;
    float *xb = xout ? xout + (size_t)b * K * a.len : nullptr;
    for (int k = 0; k < K; ++k)
        for (int i = threadIdx.x; i < R; i += blockDim.x) state[(size_t)k * a.state_floats + i] = 0.f;
    __syncthreads();
    int base = 0, slot_m = 0;   // slot_m: the slot of frame m
    for (int m = 0; m < M; ++m) {
        const int last = m + a.LA < M - 1 ? m + a.LA : M - 1;
        for (int d = threadIdx.x; d < R; d += blockDim.x) {
            const int t = hop * m + d;
            float v = 0.f;
            if (t >= a.zero_lo && t < t_end) {
                int s_hi = t / hop;
                if (s_hi > M - 1) s_hi = M - 1;
                const int s_lo = (t - N + 1 <= 0) ? 0 : (t - N + hop) / hop;
                float num = 0.f, den = 0.f;
                for (int s = s_lo, n = t - s_lo * hop; s <= s_hi; ++s, n -= hop) {
                    den += awin[n] * swin[n];
                    if (s <= last) num = den;
                }
                const int i = t - a.zero_lo;
                v = (den != 0.f ? num / den : 1.0f) * (i < a.len ? yb[i] : 0.f);
            }
            target[d] = v;
        }
        if (START == LWS_START_MIXTURE) {   // pass 0, in front of the passes
            int slot = m == 0 ? slot_m : slot_m == 0 ? a.LA : slot_m - 1;
            for (int j = m == 0 ? 0 : m + a.LA; j <= last; ++j) {
                float2 P[RTISI_BINS];   // X / |X| of frame j
                float2 *r = bufB;
                // one transform call: ph 0 forward, the mixture under frame j; ph 1 + k inverse, source k
#pragma nounroll
                for (int ph = 0; ph <= K; ++ph) {
                    float2 *x = bufA, *y = bufB;
                    if (ph == 0) {
                        for (int n = threadIdx.x; n < N; n += blockDim.x) {
                            const int t = j * hop + n, i = t - a.zero_lo;
                            const float v = t >= a.zero_lo && t < t_end && i < a.len ? yb[i] : 0.f;
                            x[n] = make_float2(v * awin[n], 0.f);
                        }
                    } else {
                        if (ph == 1) {   // the forward result is read here and not again: the later inverses take bufA, bufB
                            x = r == bufB ? bufA : (a.odd > 1 ? bufC : bufB);   // the buffers: as in k_rtisi
                            y = r;
#pragma unroll
                            for (int c = 0; c < RTISI_BINS; ++c) {
                                const int i = threadIdx.x + c * blockDim.x;
                                if (i < F) {
                                    const float2 zk = r[i], zn = r[i == 0 ? 0 : N - i];
                                    P[c] = rtisi_phasor(make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)));
                                }
                            }
                        }
                        const float *Ak = Ab + ((size_t)(ph - 1) * M + j) * F;
                        float2 *Ck = Cb + ((size_t)(ph - 1) * M + j) * F;
#pragma unroll
                        for (int c = 0; c < RTISI_BINS; ++c) {
                            const int i = threadIdx.x + c * blockDim.x;
                            if (i < F) {
                                const float mag = Ak[i];
                                const float2 u = make_float2(mag * P[c].x, mag * P[c].y);
                                if (a.iters == 0) Ck[i] = u;   // an entry row is the result only where nothing iterates on it
                                rtisi_put_pair(x, i, N, u, make_float2(0.f, 0.f));
                            }
                        }
                    }
                    __syncthreads();
                    int n_ = N, odd_ = a.odd, log2e_ = a.log2e;   // derived at the call: see k_rtisi.  An instance of its own, as in the passes
                    asm volatile("" : "+s"(n_), "+s"(odd_), "+s"(log2e_));
                    r = fft_lds<FFT_USER_MISI_LA_ENTRY>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
                    if (ph > 0) {
                        const float inv = 1.0f / (float)N;
                        float *o0 = state + (size_t)(ph - 1) * a.state_floats + cur + (size_t)slot * N;
                        for (int n = threadIdx.x; n < N; n += blockDim.x) o0[n] = r[n].x * (inv * swin[n]);
                        __syncthreads();   // r is the next load's buffer
                    }
                }
                if (++slot > a.LA) slot = 0;
            }
        }
        // pass 0: the frames that have not entered, f_kj = inv(S_kj), into fcur_k; passes 1 .. iters: the active frames of every source,
        // from xs into fnxt_k
        for (int it = START == LWS_START_MIXTURE ? 1 : 0; it <= a.iters; ++it) {
            if (it > 0) {
                for (int d = threadIdx.x; d < R; d += blockDim.x) {
                    const int t = hop * m + d;
                    float acc = 0.f;
                    for (int k = 0; k < K; ++k) {
                        const float *sk = state + (size_t)k * a.state_floats;
                        const float y = rtisi_sample(sk, sk + cur, t, m, last, slot_m, base, R, t_end, a);
                        xs[(size_t)k * R + d] = y;
                        acc = k ? acc + y : y;
                    }
                    const float delta = (target[d] - acc) / (float)K;
                    for (int k = 0; k < K; ++k) xs[(size_t)k * R + d] += delta;
                }
                __syncthreads();
            }
            const int j0 = it > 0 ? m : m == 0 ? 0 : m + a.LA;   // as in k_rtisi
            for (int k = 0; k < K; ++k) {
                float *dst = state + (size_t)k * a.state_floats + (it == 0 ? cur : nxt);
                float2 *Ck = Cb + (size_t)k * M * F;
                int slot = it > 0 || m == 0 ? slot_m : slot_m == 0 ? a.LA : slot_m - 1;
                for (int j = j0; j <= last; j += 2) {
                    const bool two = j + 1 <= last;
                    float2 *r = bufB;
#pragma nounroll
                    for (int ph = it == 0 ? 1 : 0; ph < 2; ++ph) {
                        float2 *x = bufA, *y = bufB;
                        if (ph == 0) {
                            const float *xk = xs + (size_t)k * R + (j - m) * hop;
                            for (int n = threadIdx.x; n < N; n += blockDim.x) {
                                const float w = awin[n];
                                x[n] = make_float2(xk[n] * w, two ? xk[hop + n] * w : 0.f);
                            }
                        } else if (it == 0) {
                            const float2 *r0 = Ck + (size_t)j * F, *r1 = r0 + F;
                            for (int i = threadIdx.x; i < F; i += blockDim.x)
                                rtisi_put_pair(x, i, N, r0[i], two ? r1[i] : make_float2(0.f, 0.f));
                        } else {
                            x = r == bufB ? bufA : (a.odd > 1 ? bufC : bufB);   // the buffers: as in k_rtisi
                            y = r;
                            const bool commit = it == a.iters && j == m;
                            const float *A0 = Ab + ((size_t)k * M + j) * F, *A1 = A0 + F;
                            for (int i = threadIdx.x; i < F; i += blockDim.x) {
                                const float2 zk = r[i], zn = r[i == 0 ? 0 : N - i];
                                const float2 u = rtisi_project(make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)), A0[i]);
                                float2 v = make_float2(0.f, 0.f);
                                if (two) v = rtisi_project(make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)), A1[i]);
                                if (commit) Ck[(size_t)m * F + i] = u;
                                rtisi_put_pair(x, i, N, u, v);
                            }
                        }
                        __syncthreads();
                        // one call site for both directions and every source, its uniforms derived here: see k_rtisi.  An instance of
                        // its own, so that k_rtisi's stays what it was.
                        int n_ = N, odd_ = a.odd, log2e_ = a.log2e;
                        asm volatile("" : "+s"(n_), "+s"(odd_), "+s"(log2e_));
                        r = fft_lds<FFT_USER_MISI_LA>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
                    }
                    const float inv = 1.0f / (float)N;
                    float *o0 = dst + (size_t)slot * N, *o1 = dst + (size_t)(slot < a.LA ? slot + 1 : 0) * N;
                    for (int n = threadIdx.x; n < N; n += blockDim.x) {
                        const float w = inv * swin[n];
                        o0[n] = r[n].x * w;
                        if (two) o1[n] = r[n].y * w;
                    }
                    __syncthreads();   // r is the next load's buffer, dst the next reader's
                    slot += 2;
                    if (slot > a.LA) slot -= W;
                    if (slot > a.LA) slot -= W;   // W == 1
                }
            }
            if (it > 0) { const size_t t = cur; cur = nxt; nxt = t; }
        }
        // done_k += f_km; what no later frame reaches is final (hop samples, or all N behind the last frame) and g = 1 there: the signals
        // are v_k + (y - sum_k v_k) / K, k ascending, with the final samples of all K rings at hand
        const int nfinal = m == M - 1 ? N : hop;
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            int pos = base + n;
            if (pos >= R) pos -= R;
            const int t = hop * m + n, i = t - a.zero_lo;
            const bool out = xb && n < nfinal && t >= a.zero_lo && t < t_end && i < a.len;
            float share = 0.f;
            if (out) {
                float acc = 0.f;
                for (int k = 0; k < K; ++k) {
                    const float *sk = state + (size_t)k * a.state_floats;
                    const float v = sk[pos] + sk[cur + (size_t)slot_m * N + n];
                    acc = k ? acc + v : v;
                }
                share = (yb[i] - acc) / (float)K;
            }
            for (int k = 0; k < K; ++k) {
                float *sk = state + (size_t)k * a.state_floats;
                const float v = sk[pos] + sk[cur + (size_t)slot_m * N + n];
                if (out) xb[(size_t)k * a.len + i] = v + share;
                sk[pos] = n < nfinal ? 0.f : v;
            }
        }
        base += hop;
        if (base >= R) base -= R;
        if (++slot_m > a.LA) slot_m = 0;
        __syncthreads();
    }
}

}  // namespace
