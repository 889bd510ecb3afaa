// lws_misi_kernels.h -- the kernels of MISI and of its backward pass, part of the one translation unit lws_gla.hip (whose header
// comment is the map of these files).  MISI iterates with k_gla_inverse and projects with gla_bin: it builds on lws_gla_kernels.h.
#pragma once

#include "lws_gla_kernels.h"   // k_gla_inverse's frames, gla_sample, gla_bin; rtisi_put_pair through it

namespace {

// ---- MISI: K sources coupled through their mixture y.  Per iteration: k_gla_inverse over the B K spectrograms, k_misi_residual,
// k_misi_forward.  The timeline is the uncut one of gla_sample (length Tfull = hop (M - 1) + N); y[b][j] sits at t = zero_lo + j.

// delta[b][t] = (y - sum_k OLA_k(t)) / K, k ascending (each OLA_k gathered in ascending frame order: a fixed order, no atomics),
// zero in the perfectrec cuts.  sig: [B][K][Tfull], the K overlap-added signals, which the forward load and k_misi_signals read
// back instead of gathering them again.  TRACE: part[b][blockIdx.x] = fp64 (sum y^2, sum e^2) of this block's samples, for k_gla_sum_rows.
template <bool TRACE>
__global__ void __launch_bounds__(256) k_misi_residual(const float *frames, const float *y, float *delta, float *sig, double *part,
                                                       int K, int M, int N, int hop, int zero_lo, int zero_hi) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const int Tfull = hop * (M - 1) + N, t_end = Tfull - zero_hi;
    double y2 = 0, e2 = 0;
    if (t < Tfull) {
        float d = 0.f;
        const bool kept = t >= zero_lo && t < t_end;
        float acc = 0.f;
        for (int k = 0; k < K; ++k) {
            const size_t bk = (size_t)b * K + k;
            const float x = gla_sample(frames + bk * M * N, t, M, N, hop, zero_lo, t_end);
            sig[bk * Tfull + t] = x;
            acc = k ? acc + x : x;
        }
        if (kept) {
            const float yv = y[(size_t)b * (t_end - zero_lo) + (t - zero_lo)], e = yv - acc;
            d = e / (float)K;
            if (TRACE) { y2 = (double)yv * yv; e2 = (double)e * e; }
        }
        delta[(size_t)b * Tfull + t] = d;
    }
    if constexpr (TRACE) {
        __shared__ double red[2][256];
        const int tid = threadIdx.x;
        red[0][tid] = y2; red[1][tid] = e2;
        __syncthreads();
        for (int s2 = blockDim.x / 2; s2 > 0; s2 >>= 1) {
            if (tid < s2) { red[0][tid] += red[0][tid + s2]; red[1][tid] += red[1][tid + s2]; }
            __syncthreads();
        }
        if (tid < 2) part[((size_t)b * gridDim.x + blockIdx.x) * 2 + tid] = red[tid][0];
    }
}

// k_gla_forward for source blockIdx.y % K of mixture blockIdx.y / K with the shared mixture error in its load,
// (OLA_k(t) + delta[t]) awin[n], OLA_k as k_misi_residual stored it; the epilogue is the magnitude projection alone (gla_bin without
// momentum or sums).  TAPE: X as it stands before the projection also goes to tape[B K][M][F], for the backward pass.
template <bool TAPE>
__global__ void __launch_bounds__(FFT_THREADS) k_misi_forward(const float *sig, const float *delta, const float *awin, float2 *C,
                                                               const float *A, int K, int M, int N, int odd, int log2e, int hop,
                                                               float2 *tape) {
    extern __shared__ float2 lds[];
    const int m0 = 2 * blockIdx.x, bk = blockIdx.y, F = N / 2 + 1;
    const bool two = m0 + 1 < M;
    const int Tfull = hop * (M - 1) + N;
    const float *sg = sig + (size_t)bk * Tfull, *dl = delta + (size_t)(bk / K) * Tfull;
    float2 *xa = lds, *ya = lds + N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float w = awin[n];
        const int t0 = m0 * hop + n, t1 = t0 + hop;
        const float re = (sg[t0] + dl[t0]) * w;
        const float im = two ? (sg[t1] + dl[t1]) * w : 0.f;
        xa[n] = make_float2(re, im);
    }
    __syncthreads();
    const float2 *r = fft_lds(xa, ya, N, odd, log2e, -1.0f);
    const size_t base = ((size_t)bk * M + m0) * F;
    const GlaStep st{0.f, 0};
    double p = 0, e = 0;
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
        if constexpr (TAPE) {
            tape[base + k] = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
            if (two) tape[base + F + k] = make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x));
        }
        gla_bin<false>(make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)), C, A, nullptr, base + k, st, p, e);
        if (two) gla_bin<false>(make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)), C, A, nullptr, base + F + k, st, p, e);
    }
}

// s_k = OLA_k + delta on the kept samples: x[b][k][len], len = Tfull - zero_lo - zero_hi
__global__ void __launch_bounds__(256) k_misi_signals(const float *sig, const float *delta, float *x, int K, int Tfull, int zero_lo,
                                                      int len) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x, bk = blockIdx.y;
    if (j >= len) return;
    const int t = zero_lo + j;
    x[(size_t)bk * len + j] = sig[(size_t)bk * Tfull + t] + delta[(size_t)(bk / K) * Tfull + t];
}

// ---- MISI, backward: the gradient of a loss on the final C and on the signals with respect to A, the start and the mixture, from
// the tape of k_misi_forward<true>.  Complex gradients are g = dL/dRe + j dL/dIm.  An iteration runs its three launches the other
// way: k_misi_bwd_project (the projection's derivative per bin, then the adjoint of the forward transform: a raw inverse transform
// times awin), k_misi_bwd_share (the adjoint of sharing the mixture error out), k_misi_bwd_frames (the adjoint of the inverse
// transform: a forward transform of the frames times swin, weighted).  No atomics: every sum has one owner and a fixed order.

// Step 3 for one bin: gc the gradient on c = A X / |X|, X from the tape.  gA gets Re(conj(u) gc), u = X / |X| (u = 1 where |X| == 0,
// as the forward gives A + 0j there), written on the first visit and added after that; returns what the inverse transform takes in
// this bin, gX / 2 (Re gX at the bins 0 and N/2, which have no mirror image) with gX = j u (A / |X|) Im(conj(u) gc).
__device__ __forceinline__ float2 misi_bwd_bin(const float2 *gc, const float2 *tape, const float *A, float *gA, size_t i, bool edge,
                                               int first) {
    const float2 g = gc[i], X = tape[i];
    const float mag = sqrtf(X.x * X.x + X.y * X.y);
    float ga = g.x;
    float2 gX = make_float2(0.f, 0.f);
    if (mag > 0.f) {
        const float ux = X.x / mag, uy = X.y / mag;
        ga = ux * g.x + uy * g.y;
        const float s = (A[i] / mag) * (ux * g.y - uy * g.x);
        gX = make_float2(-uy * s, ux * s);
    }
    gA[i] = first ? ga : gA[i] + ga;
    return edge ? make_float2(gX.x, 0.f) : make_float2(0.5f * gX.x, 0.5f * gX.y);
}

// Steps 3 and 4 for the frames m0 = 2 blockIdx.x and m0 + 1 of source blockIdx.y: Z = G_m + j G_{m+1} on the Hermitian-completed
// bins as k_gla_inverse builds it, one raw inverse transform (the N of the adjoint and the 1/N of the inverse cancel), times awin,
// into the frame buffer; k_misi_bwd_share overlap-adds it.
__global__ void __launch_bounds__(FFT_THREADS) k_misi_bwd_project(const float2 *gc, const float2 *tape, const float *A, float *gA,
                                                                   float *frames, const float *awin, int M, int N, int odd, int log2e,
                                                                   int first) {
    extern __shared__ float2 lds[];
    const int m0 = 2 * blockIdx.x, bk = blockIdx.y, F = N / 2 + 1;
    const bool two = m0 + 1 < M;
    const size_t base = ((size_t)bk * M + m0) * F;
    float2 *x = lds, *y = lds + N;
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        const bool edge = k == 0 || k == N / 2;
        const float2 u = misi_bwd_bin(gc, tape, A, gA, base + k, edge, first);
        const float2 v = two ? misi_bwd_bin(gc, tape, A, gA, base + F + k, edge, first) : make_float2(0.f, 0.f);
        rtisi_put_pair(x, k, N, u, v);
    }
    __syncthreads();
    const float2 *r = fft_lds<FFT_USER_MISI_BWD>(x, y, N, odd, log2e, 1.0f);
    float *o0 = frames + ((size_t)bk * M + m0) * N, *o1 = o0 + N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float w = awin[n];
        o0[n] = r[n].x * w;
        if (two) o1[n] = r[n].y * w;
    }
}

// Step 1 per sample t of the uncut timeline: gv_k(t) is the overlap-add of the frames k_misi_bwd_project left (gla_sample: ascending
// frames, zero in the perfectrec cuts) or, ENTRY, the cotangent gs of the signals itself ([B][K][len], null: zeros); m = mean_k gv_k
// (k ascending), gsig[b][k][t] = gv_k - m, and gy[b][t - zero_lo] = m (first) or += m.  gy may be null.
template <bool ENTRY>
__global__ void __launch_bounds__(256) k_misi_bwd_share(const float *src, float *gsig, float *gy, int K, int M, int N, int hop,
                                                        int zero_lo, int zero_hi, int first) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, b = blockIdx.y;
    const int Tfull = hop * (M - 1) + N, t_end = Tfull - zero_hi, len = t_end - zero_lo;
    if (t >= Tfull) return;
    const bool kept = t >= zero_lo && t < t_end;
    float acc = 0.f;
    for (int k = 0; k < K; ++k) {
        const size_t bk = (size_t)b * K + k;
        float g;
        if (ENTRY) g = (kept && src) ? src[bk * len + (t - zero_lo)] : 0.f;
        else g = gla_sample(src + bk * M * N, t, M, N, hop, zero_lo, t_end);
        gsig[bk * Tfull + t] = g;
        acc = k ? acc + g : g;
    }
    const float m = acc / (float)K;
    for (int k = 0; k < K; ++k) gsig[((size_t)b * K + k) * Tfull + t] -= m;
    if (kept && gy) {
        float *o = gy + (size_t)b * len + (t - zero_lo);
        *o = first ? m : *o + m;
    }
}

// Step 2 for the frames m0, m0 + 1 of source blockIdx.y: z = (gsig at hop m0 + j gsig at hop (m0 + 1)) swin, one forward transform,
// the pair separated as k_gla_forward separates it, times 2/N (1/N at the bins 0 and N/2, whose imaginary parts the forward never
// reads: zero), plus the cotangent gC of the final C where one is given (the entry pass).
__global__ void __launch_bounds__(FFT_THREADS) k_misi_bwd_frames(const float *gsig, const float *swin, const float2 *gC, float2 *gc,
                                                                  int M, int N, int odd, int log2e, int hop) {
    extern __shared__ float2 lds[];
    const int m0 = 2 * blockIdx.x, bk = blockIdx.y, F = N / 2 + 1;
    const bool two = m0 + 1 < M;
    const int Tfull = hop * (M - 1) + N;
    const float *sg = gsig + (size_t)bk * Tfull;
    float2 *xa = lds, *ya = lds + N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float w = swin[n];
        const int t0 = m0 * hop + n, t1 = t0 + hop;
        xa[n] = make_float2(sg[t0] * w, two ? sg[t1] * w : 0.f);
    }
    __syncthreads();
    const float2 *r = fft_lds<FFT_USER_MISI_BWD>(xa, ya, N, odd, log2e, -1.0f);
    const size_t base = ((size_t)bk * M + m0) * F;
    const float inv = 1.0f / (float)N;
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
        const bool edge = k == 0 || k == N / 2;
        const float w = edge ? 0.5f * inv : inv;             // (1/2 of the separation) (2/N, or 1/N)
        float2 g0 = make_float2(w * (zk.x + zn.x), edge ? 0.f : w * (zk.y - zn.y));
        float2 g1 = make_float2(w * (zk.y + zn.y), edge ? 0.f : w * (zn.x - zk.x));
        if (gC) {
            const float2 c0 = gC[base + k];
            g0 = make_float2(g0.x + c0.x, g0.y + c0.y);
            if (two) {
                const float2 c1 = gC[base + F + k];
                g1 = make_float2(g1.x + c1.x, g1.y + c1.y);
            }
        }
        gc[base + k] = g0;
        if (two) gc[base + F + k] = g1;
    }
}

}  // namespace
