// lws_gla_kernels.h -- the kernels of (Fast) Griffin-Lim and of its backward pass, part of the one translation unit lws_gla.hip (whose
// header comment is the map of these files).  One iteration projects the iterate onto the consistent spectrograms,
// X = stft(istft(c)) -- the round trip lws_consistency_dev makes -- and rescales X to the target magnitudes, t = A X / |X|, with the
// momentum of Fast Griffin-Lim, c = t + alpha (t - t_prev).
//
// Two launches per iteration, both one workgroup per PAIR of frames of one spectrogram (the transform of lws_fft.h, in LDS):
//   k_gla_inverse : frames m, m+1 go through ONE N-point inverse transform as Z = X_m + j X_{m+1} on the Hermitian-completed
//                   bins (real part: frame m, imaginary part: frame m+1), times the synthesis window, into the frame buffer;
//   k_gla_forward : loads z = x_m + j x_{m+1} where each sample is the overlap-add of the windowed inverse frames that cover
//                   it, gathered in ascending frame order (no signal buffer, no atomics), transforms once, separates
//                   X_m[k] = (Z[k] + conj Z[N-k]) / 2, X_{m+1}[k] = (Z[k] - conj Z[N-k]) / 2j, and in its epilogue reads
//                   c, A, t_prev and writes t, c and the per-frame fp64 sums (|c|^2, |X - c|^2) of the consistency pair.
// An odd last frame pairs with zeros.  The iterate lives in the caller's buffer; the last iteration leaves t_n there.
#pragma once

#include "lws_fft.h"
#include "lws_rtisi_kernels.h"   // rtisi_put_pair, which the backward pass packs its pair with

namespace {

__global__ void k_gla_abs(const float2 *C, float *A, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) A[i] = sqrtf(C[i].x * C[i].x + C[i].y * C[i].y);
}

// lws.pyx:118-128 for frames m0 = 2 blockIdx.x and m0 + 1.  np.real(ifft(Hermitian completion)) never sees the imaginary
// parts of the bins 0 and N/2 (they transform to an imaginary signal), so they must not leak into the partner frame.
__global__ void __launch_bounds__(FFT_THREADS) k_gla_inverse(const float2 *C, float *frames, const float *swin, int M, int N,
                                                              int odd, int log2e) {
    extern __shared__ float2 lds[];
    const int m0 = 2 * blockIdx.x, b = blockIdx.y, F = N / 2 + 1;
    const bool two = m0 + 1 < M;
    const float2 *r0 = C + ((size_t)b * M + m0) * F, *r1 = r0 + F;
    float2 *x = lds, *y = lds + N;
    for (int k = threadIdx.x; k < N; k += blockDim.x) {
        const int kk = k < F ? k : N - k;
        float2 u = r0[kk], v = two ? r1[kk] : make_float2(0.f, 0.f);
        if (k >= F) { u.y = -u.y; v.y = -v.y; }
        if (kk == 0 || kk == N / 2) u.y = v.y = 0.f;
        x[k] = make_float2(u.x - v.y, u.y + v.x);            // u + j v
    }
    __syncthreads();
    const float2 *r = fft_lds(x, y, N, odd, log2e, 1.0f);
    const float inv = 1.0f / (float)N;
    float *o0 = frames + ((size_t)b * M + m0) * N, *o1 = o0 + N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float w = inv * swin[n];
        o0[n] = r[n].x * w;
        if (two) o1[n] = r[n].y * w;
    }
}

// signal[t] of k_overlap_add, gathered: the frames s with 0 <= t - s hop < N, ascending; zero in the perfectrec cuts
__device__ __forceinline__ float gla_sample(const float *f, int t, int M, int N, int hop, int zero_lo, int t_end) {
    if (t < zero_lo || t >= t_end) return 0.f;
    int s_hi = t / hop;
    if (s_hi > M - 1) s_hi = M - 1;
    const int s_lo = (t - N + 1 <= 0) ? 0 : (t - N + hop) / hop;
    float acc = 0.f;
    for (int s = s_lo; s <= s_hi; ++s) acc += f[(size_t)s * N + (t - s * hop)];
    return acc;
}

struct GlaStep {
    float alpha;      // momentum of this step (0: c = t)
    int keep_t;       // write t to the t buffer (a later step has momentum)
};

// One bin of the epilogue: X the projection, c the iterate that entered the step.
template <bool SUMS>
__device__ __forceinline__ void gla_bin(float2 X, float2 *c, const float *A, float2 *T, size_t i, GlaStep st, double &p, double &e) {
    const float2 s = c[i];
    if (SUMS) {
        const double dx = (double)X.x - s.x, dy = (double)X.y - s.y;
        e += dx * dx + dy * dy;
        p += (double)s.x * s.x + (double)s.y * s.y;
    }
    const float a = A[i], mag = sqrtf(X.x * X.x + X.y * X.y);
    float2 t = make_float2(a, 0.f);
    if (mag > 0.f) t = make_float2(a * (X.x / mag), a * (X.y / mag));
    float2 cn = t;
    if (st.alpha != 0.f) {
        const float2 tp = T[i];
        cn = make_float2(t.x + st.alpha * (t.x - tp.x), t.y + st.alpha * (t.y - tp.y));
    }
    if (st.keep_t) T[i] = t;
    c[i] = cn;
}

// lws.pyx:82-88 for the frames m0, m0 + 1 of the overlap-added signal (length Tfull = hop (M - 1) + N, never stored), then the
// magnitude projection.  rows (SUMS): [B][M][2] doubles, (sum |c|^2, sum |X - c|^2) of each frame, as k_stft_frames writes them.
// TAPE: X as it stands before the projection also goes to tape[B][M][F], for the backward pass (its transform is an instance of its
// own, see lws_fft.h, so that the untaped kernels stay what they were).
template <bool SUMS, bool TAPE>
__global__ void __launch_bounds__(FFT_THREADS) k_gla_forward(const float *frames, const float *awin, float2 *C, const float *A,
                                                              float2 *T, double *rows, int M, int N, int odd, int log2e, int hop,
                                                              int zero_lo, int zero_hi, GlaStep st, float2 *tape) {
    extern __shared__ float2 lds[];
    __shared__ double red[SUMS ? 4 : 1][FFT_THREADS];
    const int m0 = 2 * blockIdx.x, b = blockIdx.y, F = N / 2 + 1;
    const bool two = m0 + 1 < M;
    const int t_end = hop * (M - 1) + N - zero_hi;
    const float *f = frames + (size_t)b * M * N;
    float2 *xa = lds, *ya = lds + N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float w = awin[n];
        const float re = gla_sample(f, m0 * hop + n, M, N, hop, zero_lo, t_end) * w;
        const float im = two ? gla_sample(f, (m0 + 1) * hop + n, M, N, hop, zero_lo, t_end) * w : 0.f;
        xa[n] = make_float2(re, im);
    }
    __syncthreads();
    const float2 *r = fft_lds<TAPE ? FFT_USER_GLA_TAPE : FFT_USER_SHARED>(xa, ya, N, odd, log2e, -1.0f);
    const size_t base = ((size_t)b * M + m0) * F;
    double p0 = 0, e0 = 0, p1 = 0, e1 = 0;
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
        if constexpr (TAPE) {
            tape[base + k] = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
            if (two) tape[base + F + k] = make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x));
        }
        gla_bin<SUMS>(make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)), C, A, T, base + k, st, p0, e0);
        if (two) gla_bin<SUMS>(make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)), C, A, T, base + F + k, st, p1, e1);
    }
    if (SUMS) {
        const int tid = threadIdx.x;
        red[0][tid] = p0; red[1][tid] = e0; red[2][tid] = p1; red[3][tid] = e1;
        __syncthreads();
        for (int s2 = blockDim.x / 2; s2 > 0; s2 >>= 1) {
            if (tid < s2)
                for (int q = 0; q < 4; ++q) red[q][tid] += red[q][tid + s2];
            __syncthreads();
        }
        if (tid < (two ? 4 : 2)) rows[((size_t)b * M + m0) * 2 + tid] = red[tid][0];
    }
}

__global__ void k_gla_sum_rows(const double *rows, double *out, int M, int B) {   // one thread per spectrogram, fixed order
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double p = 0, e = 0;
    for (int m = 0; m < M; ++m) { p += rows[((size_t)b * M + m) * 2]; e += rows[((size_t)b * M + m) * 2 + 1]; }
    out[2 * b] = p;
    out[2 * b + 1] = e;
}

// ---- Griffin-Lim, backward: the gradient of a loss on t_n with respect to A and the start, from the tape of
// k_gla_forward<false, true>.  c_i = (1 + alpha_i) t_i - alpha_i t_{i-1} is linear in the t's, so no t is kept: the gradient on t_i
// is gt_i = (1 + alpha_i) gc_i - alpha_{i+1} gc_{i+1} (gOut for i = n), a two-term recurrence over two gradient buffers.  An
// iteration runs the forward's two launches the other way: k_gla_bwd_project (gt, the projection's derivative per bin, a raw inverse
// transform times awin), k_gla_bwd_frames (the overlap-add gathered in its load, a forward transform times swin, weighted).  No
// atomics: every sum has one owner and a fixed order.

// gt for one bin and misi_bwd_bin's step 3 on it: ga (null: zeros) the gradient on c_i or gOut, gb that on c_{i+1}, read only where
// its coefficient cb is not zero.  Step 3 is written out again, not shared with misi_bwd_bin: with one function taking gt by value
// the compiler swaps the operands of two multiplies in k_misi_bwd_project, whose instruction stream is to stay the parent's.
__device__ __forceinline__ float2 gla_bwd_bin(const float2 *ga, const float2 *gb, float ca, float cb, const float2 *tape,
                                              const float *A, float *gA, size_t i, bool edge, int first) {
    float2 g = make_float2(0.f, 0.f);
    if (ga) {
        const float2 a = ga[i];
        g = make_float2(ca * a.x, ca * a.y);
    }
    if (cb != 0.f) {
        const float2 b = gb[i];
        g = make_float2(g.x - cb * b.x, g.y - cb * b.y);
    }
    const float2 X = tape[i];
    const float mag = sqrtf(X.x * X.x + X.y * X.y);
    float da = g.x;
    float2 gX = make_float2(0.f, 0.f);
    if (mag > 0.f) {
        const float ux = X.x / mag, uy = X.y / mag;
        da = ux * g.x + uy * g.y;
        const float s = (A[i] / mag) * (ux * g.y - uy * g.x);
        gX = make_float2(-uy * s, ux * s);
    }
    gA[i] = first ? da : gA[i] + da;
    return edge ? make_float2(gX.x, 0.f) : make_float2(0.5f * gX.x, 0.5f * gX.y);
}

// Steps 0, 3 and 4 for the frames m0 = 2 blockIdx.x and m0 + 1 of spectrogram blockIdx.y: k_misi_bwd_project with gt formed in its
// load.  The frame buffer it fills is the one k_gla_bwd_frames gathers from.
__global__ void __launch_bounds__(FFT_THREADS) k_gla_bwd_project(const float2 *ga, const float2 *gb, float ca, float cb,
                                                                  const float2 *tape, const float *A, float *gA, float *frames,
                                                                  const float *awin, int M, int N, int odd, int log2e, int first) {
    extern __shared__ float2 lds[];
    const int m0 = 2 * blockIdx.x, b = blockIdx.y, F = N / 2 + 1;
    const bool two = m0 + 1 < M;
    const size_t base = ((size_t)b * M + m0) * F;
    float2 *x = lds, *y = lds + N;
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        const bool edge = k == 0 || k == N / 2;
        const float2 u = gla_bwd_bin(ga, gb, ca, cb, tape, A, gA, base + k, edge, first);
        const float2 v = two ? gla_bwd_bin(ga, gb, ca, cb, tape, A, gA, base + F + k, edge, first) : make_float2(0.f, 0.f);
        rtisi_put_pair(x, k, N, u, v);
    }
    __syncthreads();
    const float2 *r = fft_lds<FFT_USER_GLA_BWD>(x, y, N, odd, log2e, 1.0f);
    float *o0 = frames + ((size_t)b * M + m0) * N, *o1 = o0 + N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float w = awin[n];
        o0[n] = r[n].x * w;
        if (two) o1[n] = r[n].y * w;
    }
}

// Step 2 for the frames m0, m0 + 1 of spectrogram blockIdx.y: each sample of gv gathered from the frames that cover it as
// k_gla_forward gathers its signal (gla_sample: ascending frames, zero in the perfectrec cuts, no signal buffer), times swin, one
// forward transform, then the separation and weights of k_misi_bwd_frames.  gc: where the gradient on c_{i-1} goes.
__global__ void __launch_bounds__(FFT_THREADS) k_gla_bwd_frames(const float *frames, const float *swin, float2 *gc, int M, int N,
                                                                 int odd, int log2e, int hop, int zero_lo, int zero_hi) {
    extern __shared__ float2 lds[];
    const int m0 = 2 * blockIdx.x, b = blockIdx.y, F = N / 2 + 1;
    const bool two = m0 + 1 < M;
    const int t_end = hop * (M - 1) + N - zero_hi;
    const float *f = frames + (size_t)b * M * N;
    float2 *xa = lds, *ya = lds + N;
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
        const float w = swin[n];
        const float re = gla_sample(f, m0 * hop + n, M, N, hop, zero_lo, t_end) * w;
        const float im = two ? gla_sample(f, (m0 + 1) * hop + n, M, N, hop, zero_lo, t_end) * w : 0.f;
        xa[n] = make_float2(re, im);
    }
    __syncthreads();
    const float2 *r = fft_lds<FFT_USER_GLA_BWD>(xa, ya, N, odd, log2e, -1.0f);
    const size_t base = ((size_t)b * M + m0) * F;
    const float inv = 1.0f / (float)N;
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
        const bool edge = k == 0 || k == N / 2;
        const float w = edge ? 0.5f * inv : inv;             // (1/2 of the separation) (2/N, or 1/N)
        gc[base + k] = make_float2(w * (zk.x + zn.x), edge ? 0.f : w * (zk.y - zn.y));
        if (two) gc[base + F + k] = make_float2(w * (zk.y + zn.y), edge ? 0.f : w * (zn.x - zk.x));
    }
}

}  // namespace
