// lws_gla.hip -- (Fast) Griffin-Lim refinement on the device, fused with its transforms.  One iteration projects the iterate
// onto the consistent spectrograms, X = stft(istft(c)) -- the round trip lws_consistency_dev makes -- and rescales X to the
// target magnitudes, t = A X / |X|, with the momentum of Fast Griffin-Lim, c = t + alpha (t - t_prev).
//
// Two launches per iteration, both one workgroup per PAIR of frames of one spectrogram (the transform of lws_fft.h, in LDS):
//   k_gla_inverse : frames m, m+1 go through ONE N-point inverse transform as Z = X_m + j X_{m+1} on the Hermitian-completed
//                   bins (real part: frame m, imaginary part: frame m+1), times the synthesis window, into the frame buffer;
//   k_gla_forward : loads z = x_m + j x_{m+1} where each sample is the overlap-add of the windowed inverse frames that cover
//                   it, gathered in ascending frame order (no signal buffer, no atomics), transforms once, separates
//                   X_m[k] = (Z[k] + conj Z[N-k]) / 2, X_{m+1}[k] = (Z[k] - conj Z[N-k]) / 2j, and in its epilogue reads
//                   c, A, t_prev and writes t, c and the per-frame fp64 sums (|c|^2, |X - c|^2) of the consistency pair.
// An odd last frame pairs with zeros.  The iterate lives in the caller's buffer; the last iteration leaves t_n there.
//
// The file: the kernels first -- Griffin-Lim, MISI, RTISI-LA (k_rtisi) and its backward pass (k_rtisi_bwd), online MISI (k_misi_la), their
// streaming forms and the backward passes of MISI and of Griffin-Lim, each with its own comment -- then the host half.  The one-shot calls check their arguments and open
// the same way (GlaCall); the two stream handles are one struct whose every decision is made by the step clock of lws_la_stream.h,
// plain C++ that the CPU tests drive without a device.
#include "../../include/lws_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "lws_common.h"
#include "lws_fft.h"

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
    const float2 *r = fft_lds<TAPE ? 10 : 0>(xa, ya, N, odd, log2e, -1.0f);
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

// ---- RTISI-LA (Zhu, Beauregard & Wyse 2007): Griffin-Lim under a look-ahead of LA frames.  One workgroup per spectrogram marches
// over the frames m = 0 .. M-1; committing frame m runs `iters` Jacobi iterations over the active frames m .. min(m + LA, M-1)
// against the committed overlap-add sum, then adds frame m to that sum for good.  The timeline is the uncut one of gla_sample.
//   ring : the committed sum `done` over [hop m, hop (m + LA) + N), a ring of R = N + LA hop floats (sample t of the window sits at
//          (base + t - hop m) mod R); the hop samples frame m leaves behind are final, go to the signal and are zeroed for re-use;
//   fcur : the windowed inverse frames f_j of the active frames, frame j in slot j mod (LA + 1);
//   fnxt : the f_j of the iteration under way (Jacobi: every pair reads fcur), swapped with fcur after the last pair.
// The three live in dynamic LDS behind the transform buffers (IN_LDS) or in a slice of device scratch of this workgroup alone,
// ordered by the same barriers.  Every loop that encloses a barrier runs over m, last, it, j or the direction: kernel arguments and
// counters derived from them alone, the same in every thread.
constexpr int RTISI_MAX_THREADS = 1024;
struct RtisiArgs {
    int M, N, odd, log2e, hop, LA, iters, zero_lo, zero_hi, len;
    size_t state_floats;   // R + 2 (LA + 1) N
};

// Z = c_j + i c_{j+1} on the Hermitian-completed bins, as k_gla_inverse builds it
__device__ __forceinline__ void rtisi_put_pair(float2 *Z, int k, int N, float2 u, float2 v) {
    if (k == 0 || k == N / 2) {
        Z[k] = make_float2(u.x, v.x);
    } else {
        Z[k] = make_float2(u.x - v.y, u.y + v.x);
        Z[N - k] = make_float2(u.x + v.y, v.x - u.y);
    }
}

// sample t of keep (done + sum of the active frames m .. last that cover t, ascending); slot: that of frame m
__device__ __forceinline__ float rtisi_sample(const float *ring, const float *f, int t, int m, int last, int slot, int base, int R,
                                              int t_end, RtisiArgs a) {
    if (t < a.zero_lo || t >= t_end) return 0.f;
    int d = t - a.hop * m;                                   // in [0, R): the ring's window starts at frame m
    int pos = base + d;
    if (pos >= R) pos -= R;
    float acc = ring[pos];
    for (int s = m; s <= last; ++s, d -= a.hop) {
        if ((unsigned)d < (unsigned)a.N) acc += f[(size_t)slot * a.N + d];
        if (++slot > a.LA) slot = 0;
    }
    return acc;
}

__device__ __forceinline__ float2 rtisi_project(float2 X, float a) {
    const float mag = sqrtf(X.x * X.x + X.y * X.y);
    return mag > 0.f ? make_float2(a * (X.x / mag), a * (X.y / mag)) : make_float2(a, 0.f);
}

// START (lws_hip.h's LWS_START_*) is how a frame enters in pass 0.  GIVEN: f_j = inv(S_j), two frames per transform.  OVERLAP (RTISI's
// own initial estimate): c_j = A_j X / |X| with X = fwd of the partial sum keep (done + f_m + .. + f_{j-1}) under frame j, then
// f_j = inv(c_j) -- the forward load, projection and inverse of a later pass with last = j - 1, one frame per transform (imaginary
// half zero), since the load of frame j + 1 reads f_j.  S is not read; without iterations c_j goes where S_j was.  A template
// parameter, so that the GIVEN instances are the code they were: both kernels sit at the SGPR limit (see the transform call).
// The kernel's text is lws_rtisi_march.h, compiled twice: as k_rtisi, and with the flag RTISI_TAPE as k_rtisi_tape<IN_LDS, START> (run
// under GIVEN only), which also writes every projection argument X to tape[b][m][it-1][j-m][k] for the backward pass.
#define RTISI_KERNEL k_rtisi
#define RTISI_TAPE 0
#define RTISI_TAPE_ARG
#include "lws_rtisi_march.h"
#undef RTISI_KERNEL
#undef RTISI_TAPE
#undef RTISI_TAPE_ARG
#define RTISI_KERNEL k_rtisi_tape
#define RTISI_TAPE 1
#define RTISI_TAPE_ARG , float2 *tape
#include "lws_rtisi_march.h"
#undef RTISI_KERNEL
#undef RTISI_TAPE
#undef RTISI_TAPE_ARG

// ---- RTISI-LA, backward: the gradient of a loss on the committed C and on the signal with respect to A and the start, from the tape
// of k_rtisi_tape (lws.py's rtisi_la_grad is the definition).  One workgroup per spectrogram marches m = M-1 .. 0 and runs the inner
// iterations of each commit step the other way.  Every active frame was projected from ONE sum, so the gradients on all f_j are
// windows of one timeline vector and the state is three vectors over the active window [hop m, hop m + R), R = N + LA hop, sample t
// at index t mod R (base = hop m mod R, counted, not divided):
//   gdone : the gradient on the committed sum `done`; as the window moves down, the hop samples it gains take the cotangent of the
//           signal (zero in the perfectrec cuts), and those it loses are no longer read;
//   G     : the gradient on the f_j of the active frames but m, left by the iteration (or commit step) that read them;
//   Gn    : the gradient on the sum the iteration under way projected from, swapped with G once it is complete.
// They live behind the transform buffers in LDS (IN_LDS) or in a slice of device scratch of this workgroup alone.  Per pass `it` =
// iters .. 1 and pair of active frames (j, j + 1) -- an odd last frame pairs with zeros: load (gf_j + i gf_{j+1}) swin, gf_j =
// gdone under frame m in pass `iters` and G otherwise; one forward transform; separate and weight into gc_j, gc_{j+1} (the adjoint
// of the inverse transform), plus the cotangent of C for frame m in pass `iters`; the projection's derivative per bin from the
// tape, gA accumulated by the one thread that owns the bin; the Hermitian pair gX / 2; one raw inverse transform; times awin,
// overlap-added into Gn, each sample by its owner, j ascending.  Then Gn *= keep, gdone += Gn, G <-> Gn.  Pass 0 takes the forward
// half alone for the frames that entered in step m, into gS.  Without iterations pass 0 is all there is: gS_m = gC_m + the adjoint
// of istft on the signal's cotangent under frame m.  No atomics: one fixed summation order, so a gradient repeats bit for bit.
// Every loop that encloses a barrier runs over m, it, j or the direction: kernel arguments and counters derived from them alone.
__device__ __forceinline__ float2 rtisi_bwd_bin(float2 g, float2 X, float a, float *gA, bool edge) {
    const float mag = sqrtf(X.x * X.x + X.y * X.y);
    float da = g.x;
    float2 gX = make_float2(0.f, 0.f);
    if (mag > 0.f) {
        const float ux = X.x / mag, uy = X.y / mag;
        da = ux * g.x + uy * g.y;
        const float s = (a / mag) * (ux * g.y - uy * g.x);
        gX = make_float2(-uy * s, ux * s);
    }
    *gA += da;
    return edge ? make_float2(gX.x, 0.f) : make_float2(0.5f * gX.x, 0.5f * gX.y);
}

// a: RtisiArgs with state_floats = 3 R.  gC, gx, gS may be null (zeros; not wanted).  gA arrives zeroed.
template <bool IN_LDS>
__global__ void __launch_bounds__(RTISI_MAX_THREADS) k_rtisi_bwd(const float2 *gC, const float *gx, const float *A, const float2 *tape,
                                                                 float *gA, float2 *gS, const float *awin, const float *swin,
                                                                 float *scratch, RtisiArgs a) {
    extern __shared__ float2 lds[];
    const int b = blockIdx.x, N = a.N, F = N / 2 + 1, hop = a.hop, M = a.M, W = a.LA + 1, R = N + a.LA * hop;
    const int t_end = hop * (M - 1) + N - a.zero_hi;
    float2 *bufA = lds, *bufB = lds + N, *bufC = lds + 2 * N;   // as in k_rtisi
    float *state = IN_LDS ? reinterpret_cast<float *>(lds + (a.odd > 1 ? 3 : 2) * N) : scratch + (size_t)b * a.state_floats;
    float *gdone = state, *G = state + R, *Gn = G + R;
    const float2 *gCb = gC ? gC + (size_t)b * M * F : nullptr;
    const float *gxb = gx ? gx + (size_t)b * a.len : nullptr;
    const float *Ab = A + (size_t)b * M * F;
    const float2 *tb = tape + (size_t)b * M * a.iters * W * F;   // not read without iterations
    float *gAb = gA + (size_t)b * M * F;
    float2 *gSb = gS ? gS + (size_t)b * M * F : nullptr;
    int base = (hop * (M - 1)) % R;
    for (int d = threadIdx.x; d < R; d += blockDim.x) {          // the window of the last frame
        const int t = hop * (M - 1) + d, i = t - a.zero_lo;
        int pos = base + d;
        if (pos >= R) pos -= R;
        gdone[pos] = gxb && t >= a.zero_lo && t < t_end && i < a.len ? gxb[i] : 0.f;
        G[pos] = 0.f;
    }
    __syncthreads();
    for (int m = M - 1; m >= 0; --m) {
        const int last = m + a.LA < M - 1 ? m + a.LA : M - 1;
        if (m < M - 1) {   // the window moves down by one hop; G's new samples are not read before Gn has replaced it
            base -= hop;
            if (base < 0) base += R;
            for (int d = threadIdx.x; d < hop; d += blockDim.x) {
                const int t = hop * m + d, i = t - a.zero_lo;
                int pos = base + d;
                if (pos >= R) pos -= R;
                gdone[pos] = gxb && t >= a.zero_lo && t < t_end && i < a.len ? gxb[i] : 0.f;
            }
            __syncthreads();
        }
        for (int it = a.iters; it >= 0; --it) {
            const bool entry = it == 0;   // the forward half alone, into gS
            if (entry && !gSb) continue;
            // pass 0 takes the frames that entered in step m: 0 .. last in the first step, m + LA (if there is one) after that;
            // without iterations frame m itself, from gdone
            const int j0 = !entry || a.iters == 0 ? m : m == 0 ? 0 : m + a.LA;
            const int j1 = entry && a.iters == 0 ? m : last;
            if (!entry)
                for (int d = threadIdx.x; d < R; d += blockDim.x) Gn[d] = 0.f;   // its last readers are behind a barrier
            for (int j = j0; j <= j1; j += 2) {
                const bool two = j + 1 <= j1;
                const bool head = it == a.iters && j == m;   // undoing done += f_m
                const float *g0 = head ? gdone : G;
                float2 *r = bufB;
#pragma nounroll
                for (int ph = 0; ph < (entry ? 1 : 2); ++ph) {
                    float2 *x = bufA, *y = bufB;
                    if (ph == 0) {
                        for (int n = threadIdx.x; n < N; n += blockDim.x) {
                            const float w = swin[n];
                            int p0 = base + (j - m) * hop + n;   // below 2 R
                            if (p0 >= R) p0 -= R;
                            int p1 = p0 + hop;
                            if (p1 >= R) p1 -= R;
                            x[n] = make_float2(g0[p0] * w, two ? G[p1] * w : 0.f);
                        }
                    } else {
                        x = r == bufB ? bufA : (a.odd > 1 ? bufC : bufB);   // the buffers: as in k_rtisi
                        y = r;
                        const float inv = 1.0f / (float)N;
                        const float2 *T0 = tb + (((size_t)m * a.iters + (it - 1)) * W + (j - m)) * F;
                        const float *A0 = Ab + (size_t)j * F;
                        float *gA0 = gAb + (size_t)j * F;
                        for (int k = threadIdx.x; k < F; k += blockDim.x) {
                            const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
                            const bool edge = k == 0 || k == N / 2;
                            const float w = edge ? 0.5f * inv : inv;             // (1/2 of the separation) (2/N, or 1/N)
                            float2 c0 = make_float2(w * (zk.x + zn.x), edge ? 0.f : w * (zk.y - zn.y));
                            if (head && gCb) {
                                const float2 c = gCb[(size_t)m * F + k];
                                c0 = make_float2(c0.x + c.x, c0.y + c.y);
                            }
                            const float2 u = rtisi_bwd_bin(c0, T0[k], A0[k], gA0 + k, edge);
                            float2 v = make_float2(0.f, 0.f);
                            if (two) {
                                const float2 c1 = make_float2(w * (zk.y + zn.y), edge ? 0.f : w * (zn.x - zk.x));
                                v = rtisi_bwd_bin(c1, T0[F + k], A0[F + k], gA0 + F + k, edge);
                            }
                            rtisi_put_pair(x, k, N, u, v);
                        }
                    }
                    __syncthreads();
                    int n_ = N, odd_ = a.odd, log2e_ = a.log2e;   // derived at the call: see k_rtisi.  An instance of its own
                    asm volatile("" : "+s"(n_), "+s"(odd_), "+s"(log2e_));
                    r = fft_lds<13>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
                }
                if (entry) {
                    const float inv = 1.0f / (float)N;
                    float2 *o0 = gSb + (size_t)j * F;
                    for (int k = threadIdx.x; k < F; k += blockDim.x) {
                        const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
                        const bool edge = k == 0 || k == N / 2;
                        const float w = edge ? 0.5f * inv : inv;
                        float2 c0 = make_float2(w * (zk.x + zn.x), edge ? 0.f : w * (zk.y - zn.y));
                        if (head && gCb) {
                            const float2 c = gCb[(size_t)m * F + k];
                            c0 = make_float2(c0.x + c.x, c0.y + c.y);
                        }
                        o0[k] = c0;
                        if (two) o0[F + k] = make_float2(w * (zk.y + zn.y), edge ? 0.f : w * (zn.x - zk.x));
                    }
                } else {
                    // Gn += the pair times awin over the samples the two frames cover, each by the thread that owns it
                    const int span = two ? N + hop : N;
                    for (int d = threadIdx.x; d < span; d += blockDim.x) {
                        int pos = base + (j - m) * hop + d;   // below 2 R
                        if (pos >= R) pos -= R;
                        float acc = Gn[pos];
                        if (d < N) acc += r[d].x * awin[d];
                        if (two && d >= hop) acc += r[d - hop].y * awin[d - hop];
                        Gn[pos] = acc;
                    }
                }
                __syncthreads();   // r is the next load's buffer, Gn the next pair's
            }
            if (!entry) {
                for (int d = threadIdx.x; d < R; d += blockDim.x) {
                    const int t = hop * m + d;
                    int pos = base + d;
                    if (pos >= R) pos -= R;
                    const float v = t >= a.zero_lo && t < t_end ? Gn[pos] : 0.f;
                    Gn[pos] = v;
                    gdone[pos] += v;
                }
                __syncthreads();
                float *sw = G; G = Gn; Gn = sw;
            }
        }
    }
}

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
                    r = fft_lds<7>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
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
                        r = fft_lds<2>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
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

// ---- Streaming RTISI-LA: the commit steps of k_rtisi, a few per launch, with the state kept in device memory between launches.  One
// workgroup per stream runs q.nsteps steps.  Everything is counted from the launch's first step: frame 0 is the frame that step
// commits, sample 0 its first sample, so no index grows with the length of a stream.  The frames 0 .. nheld-1 entered in earlier
// calls: their rows (A, and S where it is still read) are in the handle's `held` buffers, the rows of the later frames in the caller's
// chunk.  While the stream is open every step looks at LA frames ahead (Mrel = nsteps + LA); the closing launch knows the end
// (Mrel = what is left) and cuts the emitted samples there, never the iteration: the stream computes rtisi_la(..., open_end=True).
// State per stream in device memory: ring | fcur | (scratch placement only) the other frame buffer.  IN_LDS copies ring and fcur in on
// entry and out on exit and has fnxt in LDS alone; otherwise the kernel works in place and q.cur says which buffer is fcur.  Pairing,
// buffers, arithmetic and barriers are k_rtisi's, step for step; the loops that enclose a barrier run over kernel arguments and
// counters derived from them alone.
struct RtisiHeld {
    const float2 *S;     // [B][rows][F]: start rows of the held frames (read by pass 0 of the first launch, and without iterations)
    const float *A;      // [B][rows][F]: magnitudes of the held frames
    float2 *S_next;      // where the rows of the frames still active after this launch go (null: not kept)
    float *A_next;
};   // the launch's other arguments: RtisiStreamArgs of lws_la_stream.h

template <class T> __device__ __forceinline__ const T *rtisi_row(const T *held, const T *chunk, int j, int nheld, int F) {
    return j < nheld ? held + (size_t)j * F : chunk + (size_t)(j - nheld) * F;
}

// START: as in k_rtisi.  Under OVERLAP the handle holds no start rows; without iterations the entry row of frame j is the row the
// stream returns, so it goes to Cout where this launch commits frame j (j < nsteps) and into the next held rows (S_next) otherwise,
// and so do, before the first step, the rows held from earlier launches.
template <bool IN_LDS, int START>
__global__ void __launch_bounds__(RTISI_MAX_THREADS) k_rtisi_stream(const float2 *S, const float *A, float2 *Cout, float *xout,
                                                                    const float *awin, const float *swin, float *state, RtisiHeld h,
                                                                    RtisiStreamArgs q) {
    extern __shared__ float2 lds[];
    const int b = blockIdx.x, N = q.N, F = N / 2 + 1, hop = q.hop, W = q.LA + 1, R = N + q.LA * hop;
    const RtisiArgs a{q.Mrel, N, q.odd, q.log2e, hop, q.LA, q.iters, q.zero_lo, 0, 0, 0};   // what rtisi_sample reads
    constexpr int no_end = 0x7fffffff;   // the iteration sees no tail cut
    float2 *bufA = lds, *bufB = lds + N, *bufC = lds + 2 * N;   // as in k_rtisi
    float *gs = state + (size_t)b * q.state_floats;
    float *ls = IN_LDS ? reinterpret_cast<float *>(lds + (q.odd > 1 ? 3 : 2) * N) : gs;
    float *ring = ls;
    int cur = R, nxt = R + W * N;   // fcur and fnxt within ls
    if (IN_LDS) {
        for (int i = threadIdx.x; i < R + W * N; i += blockDim.x) ls[i] = gs[i];
    } else if (q.cur) {
        cur = nxt;
        nxt = R;
    }
    // where the rows of this stream start (offsets and, for the frame buffers, indices: pointers held across the loops cost SGPR pairs)
    const size_t held_at = (size_t)b * q.held_rows * F, chunk_at = (size_t)b * q.chunk_rows * F;
    if (START != LWS_START_GIVEN && q.iters == 0 && !q.origin) {
        // the entry rows of the frames that entered in earlier launches go where those of this launch go at entry, here at the start
        // so that nothing of it is carried over the loops
        for (int j = 0; j < q.nheld; ++j) {
            const float2 *src = h.S + held_at + (size_t)j * F;
            float2 *to = j < q.nsteps ? Cout + ((size_t)b * q.out_rows + j) * F : h.S_next + held_at + (size_t)(j - q.nsteps) * F;
            for (int k = threadIdx.x; k < F; k += blockDim.x) to[k] = src[k];
        }
    }
    __syncthreads();
    int base = q.base, slot_m = q.slot_m;   // slot_m: the slot of frame m
    for (int m = 0; m < q.nsteps; ++m) {
        const int last = m + q.LA < q.Mrel - 1 ? m + q.LA : q.Mrel - 1;
        const bool origin = q.origin && m == 0;   // k_rtisi's m == 0: the LA + 1 first frames enter together
        for (int it = 0; it <= q.iters; ++it) {
            const float *fcur = ls + cur;
            float *dst = ls + (it == 0 ? cur : nxt);
            const bool entry = START == LWS_START_OVERLAP && it == 0;   // as in k_rtisi
            const int j0 = it > 0 ? m : origin ? 0 : m + q.LA;
            int slot = it > 0 || origin ? slot_m : slot_m == 0 ? q.LA : slot_m - 1;
            for (int j = j0; j <= last; j += entry ? 1 : 2) {
                const bool two = !entry && j + 1 <= last;
                const int upto = entry ? j - 1 : last;
                float2 *r = bufB;
#pragma nounroll
                for (int ph = it == 0 && !entry ? 1 : 0; ph < 2; ++ph) {
                    float2 *x = bufA, *y = bufB;
                    if (ph == 0) {
                        for (int n = threadIdx.x; n < N; n += blockDim.x) {
                            const float w = awin[n];
                            const float re = rtisi_sample(ring, fcur, j * hop + n, m, upto, slot_m, base, R, no_end, a) * w;
                            const float im = two ? rtisi_sample(ring, fcur, (j + 1) * hop + n, m, upto, slot_m, base, R, no_end, a) * w : 0.f;
                            x[n] = make_float2(re, im);
                        }
                    } else if (it == 0 && !entry) {
                        const float2 *Sh = h.S + held_at, *Sc = S + chunk_at;
                        const float2 *r0 = rtisi_row(Sh, Sc, j, q.nheld, F), *r1 = two ? rtisi_row(Sh, Sc, j + 1, q.nheld, F) : r0;
                        for (int k = threadIdx.x; k < F; k += blockDim.x)
                            rtisi_put_pair(x, k, N, r0[k], two ? r1[k] : make_float2(0.f, 0.f));
                    } else {
                        x = r == bufB ? bufA : (q.odd > 1 ? bufC : bufB);   // the buffers: as in k_rtisi
                        y = r;
                        const bool commit = entry ? q.iters == 0 : it == q.iters && j == m;
                        const float *Ah = h.A + held_at, *Ac = A + chunk_at;
                        float2 *Co = Cout + (size_t)b * q.out_rows * F;
                        if (entry) {   // row m of Co, written below, is the place of frame j (derived here: see the transform's uniforms)
                            int row = j - q.nsteps;
                            asm volatile("" : "+s"(row));
                            Co = row < 0 ? Co + (size_t)(j - m) * F : h.S_next + held_at + (ptrdiff_t)(row - m) * F;
                        }
                        const float *A0 = rtisi_row(Ah, Ac, j, q.nheld, F), *A1 = two ? rtisi_row(Ah, Ac, j + 1, q.nheld, F) : A0;
                        for (int k = threadIdx.x; k < F; k += blockDim.x) {
                            const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
                            const float2 u = rtisi_project(make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)), A0[k]);
                            float2 v = make_float2(0.f, 0.f);
                            if (two) v = rtisi_project(make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)), A1[k]);
                            if (commit) Co[(size_t)m * F + k] = u;
                            rtisi_put_pair(x, k, N, u, v);
                        }
                    }
                    __syncthreads();
                    // one call site for both directions, its uniforms derived here: see k_rtisi.  An instance of its own, so that
                    // k_rtisi's and k_misi_la's stay what they were.
                    int n_ = N, odd_ = q.odd, log2e_ = q.log2e;
                    asm volatile("" : "+s"(n_), "+s"(odd_), "+s"(log2e_));
                    r = fft_lds<START == LWS_START_GIVEN ? 3 : 6>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
                }
                const float inv = 1.0f / (float)N;
                float *o0 = dst + (size_t)slot * N, *o1 = dst + (size_t)(slot < q.LA ? slot + 1 : 0) * N;
                for (int n = threadIdx.x; n < N; n += blockDim.x) {
                    const float w = inv * swin[n];
                    o0[n] = r[n].x * w;
                    if (two) o1[n] = r[n].y * w;
                }
                __syncthreads();   // r is the next load's buffer, dst the next reader's
                slot += entry ? 1 : 2;
                if (slot > q.LA) slot -= W;
                if (slot > q.LA) slot -= W;   // W == 1
            }
            if (it > 0) { const int t = cur; cur = nxt; nxt = t; }
        }
        if (START == LWS_START_GIVEN && q.iters == 0) {   // nothing was projected: the committed row is the start row
            const float2 *r0 = rtisi_row(h.S + held_at, S + chunk_at, m, q.nheld, F);
            float2 *Co = Cout + (size_t)b * q.out_rows * F;
            for (int k = threadIdx.x; k < F; k += blockDim.x) Co[(size_t)m * F + k] = r0[k];
        }
        // done += f_m; what no later frame reaches is final: hop samples (what lies behind the last frame of the stream: below)
        const float *fm = ls + cur + (size_t)slot_m * N;
        float *xb = xout ? xout + (size_t)b * q.out_samples : nullptr;
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            int pos = base + n;
            if (pos >= R) pos -= R;
            const float v = ring[pos] + fm[n];
            const int t = hop * m + n;
            if (n < hop) {
                if (xb && t >= q.zero_lo && t < q.emit_end) xb[t - q.zero_lo] = v;
                ring[pos] = 0.f;
            } else {
                ring[pos] = v;
            }
        }
        base += hop;
        if (base >= R) base -= R;
        if (++slot_m > q.LA) slot_m = 0;
        __syncthreads();
    }
    if (q.closing && xout) {   // the N - hop samples behind the last commit: final now, also when this launch has no step (LA == 0)
        float *xb = xout + (size_t)b * q.out_samples;
        for (int d = threadIdx.x; d < N - hop; d += blockDim.x) {
            int pos = base + d;
            if (pos >= R) pos -= R;
            const int t = hop * q.nsteps + d;
            if (t >= q.zero_lo && t < q.emit_end) xb[t - q.zero_lo] = ring[pos];
        }
    }
    if (IN_LDS) {
        for (int i = threadIdx.x; i < R; i += blockDim.x) gs[i] = ring[i];
        for (int i = threadIdx.x; i < W * N; i += blockDim.x) gs[R + i] = ls[cur + i];
    }
    const float2 *Sh = h.S + held_at, *Sc = S + chunk_at;
    const float *Ah = h.A + held_at, *Ac = A + chunk_at;
    // the rows of the frames nsteps .. nsteps + LA - 1, active in the next launch, into the other held buffer
    for (int i = 0; i < q.LA; ++i) {
        if (h.A_next) {
            const float *src = rtisi_row(Ah, Ac, q.nsteps + i, q.nheld, F);
            float *to = h.A_next + held_at + (size_t)i * F;
            for (int k = threadIdx.x; k < F; k += blockDim.x) to[k] = src[k];
        }
        if (START == LWS_START_GIVEN && h.S_next) {
            const float2 *src = rtisi_row(Sh, Sc, q.nsteps + i, q.nheld, F);
            float2 *to = h.S_next + held_at + (size_t)i * F;
            for (int k = threadIdx.x; k < F; k += blockDim.x) to[k] = src[k];
        }
    }
}

// ---- Streaming online MISI: the commit steps of k_misi_la, a few per launch, as k_rtisi_stream runs those of k_rtisi.  One workgroup
// per mixture; everything is counted from the launch's first step (frame 0 is the frame that step commits, sample 0 its first
// sample).  Rows (S, and A per source) and mixture samples that entered in earlier calls come from the handle's `held` buffers, later
// ones from the caller's chunk: mixture sample t is held.y[t] for t < ny_held and Y[t - ny_held] behind that, nothing beyond the
// ny_chunk samples passed.  The denominator of the entered share g sums w over the frames from the stream's first (frame0, relative,
// <= 0) to every frame that covers the sample while the stream is open, to Mrel - 1 in the closing launch, which knows the end: the
// one arithmetic difference from k_misi_la; the stream computes misi_la(..., open_end=True).  State per stream in device memory,
// K x (ring | fcur | (scratch placement only) the other frame buffer); target and xs are temporaries of a step, in LDS or, with the
// scratch placement, in (K + 1) R floats behind the stream's state that carry nothing from launch to launch.  IN_LDS copies rings and
// fcur_k in on entry and out on exit.  What the next launch still needs -- the rows of the frames nsteps .. nsteps + LA - 1 and the
// R - hop mixture samples from hop nsteps on -- the launch copies into the other held buffers (two of each, as in k_rtisi_stream: a
// launch never writes what it reads), and it does so before its first step: carried over the loops to an epilogue, those pointers and
// counts cost the lanes that keep the SGPRs parked and 36 bytes of reserved scratch per lane.  Pairing, buffers, arithmetic and
// barriers are k_misi_la's, step for step; the loops that enclose a barrier run over kernel arguments and counters derived from them
// alone.  The loops over the sources stay rolled (K is an argument: unrolled on a guess they only add to the SGPRs parked).
struct MisiStreamHeld {
    const float2 *S;     // [B][K][rows][F]: as RtisiHeld, per source
    const float *A;
    const float *y;      // [B][y_rows]: the mixture samples in front of the chunk's
    float2 *S_next;
    float *A_next;
    float *y_next;       // where the samples still under the active frames after this launch go (null: not kept)
};   // the launch's other arguments: MisiStreamArgs of lws_la_stream.h

__device__ __forceinline__ float misi_stream_y(const float *held, const float *chunk, int t, int ny_held, int ny_chunk) {
    if (t < ny_held) return held[t];
    const int i = t - ny_held;
    return i < ny_chunk ? chunk[i] : 0.f;
}

// START: as in k_misi_la, the mixture under frame j read as the target reads it.  Under MIXTURE the handle holds no start rows;
// without iterations the entry rows of frame j are the rows the stream returns, so they go to Cout where this launch commits frame j
// (j < nsteps) and into the next held rows (S_next) otherwise, and so do, before the first step, the rows held from earlier launches.
template <bool IN_LDS, int START>
__global__ void __launch_bounds__(RTISI_MAX_THREADS) k_misi_la_stream(const float2 *S, const float *A, const float *Y, float2 *Cout,
                                                                      float *xout, const float *awin, const float *swin, float *state,
                                                                      MisiStreamHeld h, MisiStreamArgs p) {
    extern __shared__ float2 lds[];
    const RtisiStreamArgs q = p.r;
    const int b = blockIdx.x, K = p.K, N = q.N, F = N / 2 + 1, hop = q.hop, W = q.LA + 1, R = N + q.LA * hop;
    const RtisiArgs a{q.Mrel, N, q.odd, q.log2e, hop, q.LA, q.iters, q.zero_lo, 0, 0, 0};   // what rtisi_sample reads
    constexpr int no_end = 0x7fffffff;   // the iteration sees no tail cut
    float2 *bufA = lds, *bufB = lds + N, *bufC = lds + 2 * N;   // as in k_rtisi
    float *gs = state + (size_t)b * p.stream_floats;
    float *ls = IN_LDS ? reinterpret_cast<float *>(lds + (q.odd > 1 ? 3 : 2) * N) : gs;
    const int sstride = IN_LDS ? R + 2 * W * N : (int)q.state_floats;   // of a source in ls
    const int target_at = K * sstride, xs_at = target_at + R;   // target and xs within ls: indices, not pointers held across the loops
    int cur = R, nxt = R + W * N;   // fcur and fnxt within the state of a source; its ring is at 0
    if (IN_LDS) {
#pragma nounroll
        for (int k = 0; k < K; ++k)
            for (int i = threadIdx.x; i < R + W * N; i += blockDim.x) ls[(size_t)k * sstride + i] = gs[(size_t)k * q.state_floats + i];
    } else if (q.cur) {
        cur = nxt;
        nxt = R;
    }
    const size_t hy_at = (size_t)b * p.y_rows, cy_at = (size_t)b * p.ny_chunk;   // where the mixture samples of this stream start
    // what the next launch still needs goes into the other held buffers, here at the start, so that nothing of it is carried over the
    // loops: the rows of the frames nsteps .. nsteps + LA - 1, active then ...
#pragma nounroll
    for (int k = 0; k < K; ++k) {
        const size_t held_at = ((size_t)b * K + k) * q.held_rows * F, chunk_at = ((size_t)b * K + k) * q.chunk_rows * F;
        for (int i = 0; i < q.LA; ++i) {
            if (h.A_next) {
                const float *src = rtisi_row(h.A + held_at, A + chunk_at, q.nsteps + i, q.nheld, F);
                float *to = h.A_next + held_at + (size_t)i * F;
                for (int j = threadIdx.x; j < F; j += blockDim.x) to[j] = src[j];
            }
            if (START == LWS_START_GIVEN && h.S_next) {
                const float2 *src = rtisi_row(h.S + held_at, S + chunk_at, q.nsteps + i, q.nheld, F);
                float2 *to = h.S_next + held_at + (size_t)i * F;
                for (int j = threadIdx.x; j < F; j += blockDim.x) to[j] = src[j];
            }
        }
    }
    // ... the entry rows of the frames that entered in earlier launches, to where those of this launch go at entry ...
    if (START != LWS_START_GIVEN && q.iters == 0 && !q.origin) {
#pragma nounroll
        for (int k = 0; k < K; ++k) {
            const size_t held_at = ((size_t)b * K + k) * q.held_rows * F;
            for (int j = 0; j < q.nheld; ++j) {
                const float2 *src = h.S + held_at + (size_t)j * F;
                float2 *to = j < q.nsteps ? Cout + (((size_t)b * K + k) * q.out_rows + j) * F : h.S_next + held_at + (size_t)(j - q.nsteps) * F;
                for (int i = threadIdx.x; i < F; i += blockDim.x) to[i] = src[i];
            }
        }
    }
    // ... and the mixture samples under them
    if (h.y_next) {
        float *to = h.y_next + (size_t)b * p.y_rows;
        for (int i = threadIdx.x; i < p.y_keep; i += blockDim.x)
            to[i] = misi_stream_y(h.y + hy_at, Y + cy_at, hop * q.nsteps + i, p.ny_held, p.ny_chunk);
    }
    __syncthreads();
    int base = q.base, slot_m = q.slot_m;   // slot_m: the slot of frame m
    for (int m = 0; m < q.nsteps; ++m) {
        const int last = m + q.LA < q.Mrel - 1 ? m + q.LA : q.Mrel - 1;
        const bool origin = q.origin && m == 0;   // k_misi_la's m == 0: the LA + 1 first frames enter together
        for (int d = threadIdx.x; d < R; d += blockDim.x) {
            const int t = hop * m + d;
            float v = 0.f;
            if (t >= q.zero_lo) {
                int s = p.frame0, n = t - s * hop;            // the first frame of the stream, or the first that covers t
                if (n > N - 1) {
                    const int skip = (n - N + hop) / hop;
                    s += skip;
                    n -= skip * hop;
                }
                int s_hi = t / hop;
                if (q.closing && s_hi > q.Mrel - 1) s_hi = q.Mrel - 1;
                float num = 0.f, den = 0.f;
                for (; s <= s_hi; ++s, n -= hop) {
                    den += awin[n] * swin[n];
                    if (s <= last) num = den;
                }
                v = (den != 0.f ? num / den : 1.0f) * misi_stream_y(h.y + hy_at, Y + cy_at, t, p.ny_held, p.ny_chunk);
            }
            ls[target_at + d] = v;
        }
        if (START == LWS_START_MIXTURE) {   // pass 0 in front of the passes: k_misi_la's block, on the stream's rows and samples
            int slot = origin ? slot_m : slot_m == 0 ? q.LA : slot_m - 1;
            for (int j = origin ? 0 : m + q.LA; j <= last; ++j) {
                float2 P[RTISI_BINS];
                float2 *r = bufB;
#pragma nounroll
                for (int ph = 0; ph <= K; ++ph) {
                    float2 *x = bufA, *y = bufB;
                    if (ph == 0) {
                        for (int n = threadIdx.x; n < N; n += blockDim.x) {
                            const int t = j * hop + n;
                            const float v = t >= q.zero_lo ? misi_stream_y(h.y + hy_at, Y + cy_at, t, p.ny_held, p.ny_chunk) : 0.f;
                            x[n] = make_float2(v * awin[n], 0.f);
                        }
                    } else {
                        if (ph == 1) {
                            x = r == bufB ? bufA : (q.odd > 1 ? bufC : bufB);
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
                        int bk = b * K + ph - 1;   // where the rows of this source start, derived here: see the transform's uniforms
                        asm volatile("" : "+s"(bk));
                        const float *Ak = rtisi_row(h.A + (size_t)bk * q.held_rows * F, A + (size_t)bk * q.chunk_rows * F, j, q.nheld, F);
                        int row = j - q.nsteps;
                        asm volatile("" : "+s"(row));
                        float2 *Co = row < 0 ? Cout + ((size_t)bk * q.out_rows + j) * F : h.S_next + ((size_t)bk * q.held_rows + row) * F;
#pragma unroll
                        for (int c = 0; c < RTISI_BINS; ++c) {
                            const int i = threadIdx.x + c * blockDim.x;
                            if (i < F) {
                                const float mag = Ak[i];
                                const float2 u = make_float2(mag * P[c].x, mag * P[c].y);
                                if (q.iters == 0) Co[i] = u;
                                rtisi_put_pair(x, i, N, u, make_float2(0.f, 0.f));
                            }
                        }
                    }
                    __syncthreads();
                    int n_ = N, odd_ = q.odd, log2e_ = q.log2e;   // derived at the call: see k_rtisi.  An instance of its own, as in the passes
                    asm volatile("" : "+s"(n_), "+s"(odd_), "+s"(log2e_));
                    r = fft_lds<8>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
                    if (ph > 0) {
                        const float inv = 1.0f / (float)N;
                        float *o0 = ls + (size_t)(ph - 1) * sstride + cur + slot * N;
                        for (int n = threadIdx.x; n < N; n += blockDim.x) o0[n] = r[n].x * (inv * swin[n]);
                        __syncthreads();   // r is the next load's buffer
                    }
                }
                if (++slot > q.LA) slot = 0;
            }
        }
        for (int it = START == LWS_START_MIXTURE ? 1 : 0; it <= q.iters; ++it) {
            if (it > 0) {
                for (int d = threadIdx.x; d < R; d += blockDim.x) {
                    const int t = hop * m + d;
                    float acc = 0.f;
#pragma nounroll
                    for (int k = 0; k < K; ++k) {
                        const float *sk = ls + (size_t)k * sstride;
                        const float y = rtisi_sample(sk, sk + cur, t, m, last, slot_m, base, R, no_end, a);
                        ls[xs_at + k * R + d] = y;
                        acc = k ? acc + y : y;
                    }
                    const float delta = (ls[target_at + d] - acc) / (float)K;
#pragma nounroll
                    for (int k = 0; k < K; ++k) ls[xs_at + k * R + d] += delta;
                }
                __syncthreads();
            }
            const int j0 = it > 0 ? m : origin ? 0 : m + q.LA;   // as in k_rtisi_stream
#pragma nounroll
            for (int k = 0; k < K; ++k) {
                float *dst = ls + (size_t)k * sstride + (it == 0 ? cur : nxt);
                int slot = it > 0 || origin ? slot_m : slot_m == 0 ? q.LA : slot_m - 1;
                for (int j = j0; j <= last; j += 2) {
                    const bool two = j + 1 <= last;
                    float2 *r = bufB;
#pragma nounroll
                    for (int ph = it == 0 ? 1 : 0; ph < 2; ++ph) {
                        float2 *x = bufA, *y = bufB;
                        if (ph == 0) {
                            const float *xk = ls + xs_at + k * R + (j - m) * hop;
                            for (int n = threadIdx.x; n < N; n += blockDim.x) {
                                const float w = awin[n];
                                x[n] = make_float2(xk[n] * w, two ? xk[hop + n] * w : 0.f);
                            }
                        } else if (it == 0) {
                            int bk = b * K + k;   // where the rows of this source start, derived here: see the transform's uniforms
                            asm volatile("" : "+s"(bk));
                            const float2 *Sh = h.S + (size_t)bk * q.held_rows * F, *Sc = S + (size_t)bk * q.chunk_rows * F;
                            const float2 *r0 = rtisi_row(Sh, Sc, j, q.nheld, F), *r1 = two ? rtisi_row(Sh, Sc, j + 1, q.nheld, F) : r0;
                            for (int i = threadIdx.x; i < F; i += blockDim.x)
                                rtisi_put_pair(x, i, N, r0[i], two ? r1[i] : make_float2(0.f, 0.f));
                        } else {
                            x = r == bufB ? bufA : (q.odd > 1 ? bufC : bufB);   // the buffers: as in k_rtisi
                            y = r;
                            const bool commit = it == q.iters && j == m;
                            int bk = b * K + k;   // as above
                            asm volatile("" : "+s"(bk));
                            const float *Ah = h.A + (size_t)bk * q.held_rows * F, *Ac = A + (size_t)bk * q.chunk_rows * F;
                            float2 *Co = Cout + (size_t)bk * q.out_rows * F;
                            const float *A0 = rtisi_row(Ah, Ac, j, q.nheld, F), *A1 = two ? rtisi_row(Ah, Ac, j + 1, q.nheld, F) : A0;
                            for (int i = threadIdx.x; i < F; i += blockDim.x) {
                                const float2 zk = r[i], zn = r[i == 0 ? 0 : N - i];
                                const float2 u = rtisi_project(make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)), A0[i]);
                                float2 v = make_float2(0.f, 0.f);
                                if (two) v = rtisi_project(make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)), A1[i]);
                                if (commit) Co[(size_t)m * F + i] = u;
                                rtisi_put_pair(x, i, N, u, v);
                            }
                        }
                        __syncthreads();
                        // one call site for both directions and every source, its uniforms derived here: see k_rtisi.  An instance of
                        // its own, so that those of the three kernels above stay what they were.
                        int n_ = N, odd_ = q.odd, log2e_ = q.log2e;
                        asm volatile("" : "+s"(n_), "+s"(odd_), "+s"(log2e_));
                        r = fft_lds<4>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
                    }
                    const float inv = 1.0f / (float)N;
                    float *o0 = dst + (size_t)slot * N, *o1 = dst + (size_t)(slot < q.LA ? slot + 1 : 0) * N;
                    for (int n = threadIdx.x; n < N; n += blockDim.x) {
                        const float w = inv * swin[n];
                        o0[n] = r[n].x * w;
                        if (two) o1[n] = r[n].y * w;
                    }
                    __syncthreads();   // r is the next load's buffer, dst the next reader's
                    slot += 2;
                    if (slot > q.LA) slot -= W;
                    if (slot > q.LA) slot -= W;   // W == 1
                }
            }
            if (it > 0) { const int t = cur; cur = nxt; nxt = t; }
        }
        if (START == LWS_START_GIVEN && q.iters == 0) {   // nothing was projected: the committed rows are the start rows
#pragma nounroll
            for (int k = 0; k < K; ++k) {
                const float2 *r0 = rtisi_row(h.S + ((size_t)b * K + k) * q.held_rows * F, S + ((size_t)b * K + k) * q.chunk_rows * F, m,
                                             q.nheld, F);
                float2 *Co = Cout + ((size_t)b * K + k) * q.out_rows * F;
                for (int i = threadIdx.x; i < F; i += blockDim.x) Co[(size_t)m * F + i] = r0[i];
            }
        }
        // done_k += f_km; the hop samples no later frame reaches are final and g = 1 there: the signals are v_k + (y - sum_k v_k) / K,
        // k ascending (what lies behind the last frame of the stream: below)
        float *xb = xout ? xout + (size_t)b * K * q.out_samples : nullptr;
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            int pos = base + n;
            if (pos >= R) pos -= R;
            const int t = hop * m + n;
            const bool out = xb && n < hop && t >= q.zero_lo && t < q.emit_end;
            float share = 0.f;
            if (out) {
                float acc = 0.f;
#pragma nounroll
                for (int k = 0; k < K; ++k) {
                    const float *sk = ls + (size_t)k * sstride;
                    const float v = sk[pos] + sk[cur + slot_m * N + n];
                    acc = k ? acc + v : v;
                }
                share = (misi_stream_y(h.y + hy_at, Y + cy_at, t, p.ny_held, p.ny_chunk) - acc) / (float)K;
            }
#pragma nounroll
            for (int k = 0; k < K; ++k) {
                float *sk = ls + (size_t)k * sstride;
                const float v = sk[pos] + sk[cur + slot_m * N + n];
                if (out) xb[(size_t)k * q.out_samples + (t - q.zero_lo)] = v + share;
                sk[pos] = n < hop ? 0.f : v;
            }
        }
        base += hop;
        if (base >= R) base -= R;
        if (++slot_m > q.LA) slot_m = 0;
        __syncthreads();
    }
    if (q.closing && xout) {   // the N - hop samples behind the last commit: final now, also when this launch has no step (LA == 0)
        float *xb = xout + (size_t)b * K * q.out_samples;
        for (int d = threadIdx.x; d < N - hop; d += blockDim.x) {
            int pos = base + d;
            if (pos >= R) pos -= R;
            const int t = hop * q.nsteps + d;
            if (t >= q.zero_lo && t < q.emit_end) {
                float acc = 0.f;
#pragma nounroll
                for (int k = 0; k < K; ++k) {
                    const float v = ls[(size_t)k * sstride + pos];
                    acc = k ? acc + v : v;
                }
                const float share = (misi_stream_y(h.y + hy_at, Y + cy_at, t, p.ny_held, p.ny_chunk) - acc) / (float)K;
#pragma nounroll
                for (int k = 0; k < K; ++k) xb[(size_t)k * q.out_samples + (t - q.zero_lo)] = ls[(size_t)k * sstride + pos] + share;
            }
        }
    }
    if (IN_LDS) {
#pragma nounroll
        for (int k = 0; k < K; ++k) {
            float *gk = gs + (size_t)k * q.state_floats;
            const float *lk = ls + (size_t)k * sstride;
            for (int i = threadIdx.x; i < R; i += blockDim.x) gk[i] = lk[i];
            for (int i = threadIdx.x; i < W * N; i += blockDim.x) gk[R + i] = lk[cur + i];
        }
    }
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
    const float2 *r = fft_lds<9>(x, y, N, odd, log2e, 1.0f);
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
    const float2 *r = fft_lds<9>(xa, ya, N, odd, log2e, -1.0f);
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
    const float2 *r = fft_lds<11>(x, y, N, odd, log2e, 1.0f);
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
    const float2 *r = fft_lds<11>(xa, ya, N, odd, log2e, -1.0f);
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

// ---- The host half.  Windows and scratch of the iteration, one set per device, serialised on the device by the event scheme of
// lws_stft.hip.  The windows stay on the device between calls: a call with the windows of the previous one uploads nothing.
struct GlaCtx {
    Scratch frames, t, a, rows, trace, win_a, win_s;
    Scratch delta, sig;                   // MISI: the shared mixture error, and the K overlap-added signals
    Scratch gc;                           // MISI backward: the gradient on the iterate, between the iterations
    Scratch gc2;                          // Griffin-Lim backward: with gc, the gradients on c_i and c_{i+1}
    Scratch state;                        // RTISI-LA: ring and frames of the workgroups whose state does not fit in LDS
    std::vector<double> host_a, host_s;   // what win_a / win_s hold
    hipEvent_t last = nullptr;
    bool busy = false;
};
std::mutex g_mu;
GlaCtx g_ctx[MAX_DEVICES];

int ctx_enter(GlaCtx &c, hipStream_t s) {
    if (!c.last) STFT_TRY(hipEventCreateWithFlags(&c.last, hipEventDisableTiming));
    if (c.busy) STFT_TRY(hipStreamWaitEvent(s, c.last, 0));
    return LWS_OK;
}
int ctx_leave(GlaCtx &c, hipStream_t s) {
    STFT_TRY(hipEventRecord(c.last, s));
    c.busy = true;
    return LWS_OK;
}

int upload_window(Scratch &dst, std::vector<double> &held, const double *w, int N, hipStream_t s) {
    if ((int)held.size() == N && dst.p && !memcmp(held.data(), w, (size_t)N * sizeof(double))) return LWS_OK;
    held.clear();
    std::vector<float> f(N);
    for (int i = 0; i < N; ++i) f[i] = (float)w[i];
    int rc = dst.ensure((size_t)N * sizeof(float));
    if (rc) return rc;
    STFT_TRY(hipMemcpyAsync(dst.p, f.data(), (size_t)N * sizeof(float), hipMemcpyHostToDevice, s));
    STFT_TRY(hipStreamSynchronize(s));   // f goes out of scope
    held.assign(w, w + N);
    return LWS_OK;
}

// Every kernel of this file that takes dynamic LDS, and how much it may ask for: the transform buffers, or (a look-ahead kernel with
// its state in LDS) all a workgroup can have.
constexpr size_t RTISI_LDS_CAP = 160 * 1024;
struct LdsOptIn {
    hipError_t (*allow)(int);
    int bytes;
};
#define LA_OPT_IN(kernel, start)                                                \
    {&lws::allow_dynamic_lds<&kernel<true, start>>, (int)RTISI_LDS_CAP},        \
    {&lws::allow_dynamic_lds<&kernel<false, start>>, 3 * MAXN * (int)sizeof(float2)}
#define FFT_OPT_IN(...) {&lws::allow_dynamic_lds<&__VA_ARGS__>, 3 * MAXN * (int)sizeof(float2)}
const LdsOptIn LDS_OPT_INS[] = {
    FFT_OPT_IN(k_gla_inverse), FFT_OPT_IN(k_gla_forward<true, false>), FFT_OPT_IN(k_gla_forward<false, false>),
    FFT_OPT_IN(k_gla_forward<false, true>), FFT_OPT_IN(k_gla_bwd_project), FFT_OPT_IN(k_gla_bwd_frames),
    FFT_OPT_IN(k_misi_forward<false>), FFT_OPT_IN(k_misi_forward<true>), FFT_OPT_IN(k_misi_bwd_project), FFT_OPT_IN(k_misi_bwd_frames),
    LA_OPT_IN(k_rtisi, LWS_START_GIVEN), LA_OPT_IN(k_rtisi, LWS_START_OVERLAP),
    {&lws::allow_dynamic_lds<&k_rtisi_tape<true, LWS_START_GIVEN>>, (int)RTISI_LDS_CAP}, FFT_OPT_IN(k_rtisi_tape<false, LWS_START_GIVEN>),
    {&lws::allow_dynamic_lds<&k_rtisi_bwd<true>>, (int)RTISI_LDS_CAP}, FFT_OPT_IN(k_rtisi_bwd<false>),
    LA_OPT_IN(k_misi_la, LWS_START_GIVEN), LA_OPT_IN(k_misi_la, LWS_START_MIXTURE),
    LA_OPT_IN(k_rtisi_stream, LWS_START_GIVEN), LA_OPT_IN(k_rtisi_stream, LWS_START_OVERLAP),
    LA_OPT_IN(k_misi_la_stream, LWS_START_GIVEN), LA_OPT_IN(k_misi_la_stream, LWS_START_MIXTURE),
};
#undef LA_OPT_IN
#undef FFT_OPT_IN
int allow_lds_all() {
    for (const LdsOptIn &k : LDS_OPT_INS) STFT_TRY(k.allow(k.bytes));
    return LWS_OK;
}

// The magnitudes of a call: those given, or those of the rows, by k_gla_abs into `scratch`.
int magnitudes(const float *&A, const float2 *rows, size_t bins, Scratch &scratch, hipStream_t s) {
    if (A) return LWS_OK;
    int rc = scratch.ensure(bins * sizeof(float));
    if (rc) return rc;
    hipLaunchKernelGGL(k_gla_abs, dim3((unsigned)((bins + 255) / 256)), dim3(256), 0, s, rows, static_cast<float *>(scratch.p), bins);
    A = static_cast<const float *>(scratch.p);
    return LWS_OK;
}

// What the one-shot calls share once their arguments are checked: the device's context under g_mu, the LDS opt-in, both windows on
// the device, the factors of N and the cuts of perfectrec.  open() after the checks, close() after the last launch.
struct GlaCall {
    std::lock_guard<std::mutex> lk{g_mu};
    GlaCtx &c;
    hipStream_t s;
    const float *wa = nullptr, *ws = nullptr;
    Factors fc{};
    size_t lds = 0;                 // of a launch that only transforms
    int zero_lo = 0, zero_hi = 0;   // with perfectrec the reference cuts the first prepad and the last N - hop samples and the forward
                                    // transform pads zeros back in their place (same frame count), as in lws_consistency_dev
    GlaCall(int device, void *stream) : c(g_ctx[device]), s(static_cast<hipStream_t>(stream)) {}
    int open(int device, int N, int hop, const double *awin, const double *swin, int perfectrec) {
        STFT_TRY(hipSetDevice(device));
        int rc = ctx_enter(c, s);
        if (!rc) rc = allow_lds_all();
        if (!rc) rc = upload_window(c.win_a, c.host_a, awin, N, s);
        if (!rc) rc = upload_window(c.win_s, c.host_s, swin, N, s);
        wa = static_cast<const float *>(c.win_a.p);
        ws = static_cast<const float *>(c.win_s.p);
        fc = factor(N);
        lds = fft_lds_bytes(N);
        zero_lo = perfectrec ? prepad(N, hop) : 0;
        zero_hi = perfectrec ? N - hop : 0;
        return rc;
    }
    int close() {
        STFT_TRY(hipGetLastError());
        return ctx_leave(c, s);
    }
};

}  // namespace

namespace {

// lws_griffin_lim_dev, and with a tape (taped) lws_griffin_lim_tape_dev: the same launches, the forward one writing X as well
int gla_run(int device, void *C_dev, const float *A_dev, int B, int M, int N, int fshift, const double *awin, const double *swin,
            int perfectrec, int iters, double alpha, double *trace, float2 *tape, bool taped, void *stream) {
    int rc = check_shape(device, B, M, N, fshift);
    if (rc) return rc;
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (!(alpha >= 0.0 && alpha < 1.0)) return lws::set_error(LWS_ERR_INVALID, "momentum %g outside [0, 1)", alpha);
    if (!C_dev || !awin || !swin) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    if (taped && (!A_dev || (iters > 0 && !tape))) return lws::set_error(LWS_ERR_INVALID, "null magnitudes or tape");
    if (iters > 0 && (rc = check_round_trip(M, N, fshift, perfectrec))) return rc;
    if (B == 0 || iters == 0) return LWS_OK;
    GlaCall g(device, stream);
    if ((rc = g.open(device, N, fshift, awin, swin, perfectrec))) return rc;
    GlaCtx &c = g.c;
    hipStream_t s = g.s;
    const int F = N / 2 + 1;
    const size_t bins = (size_t)B * M * F;
    const bool momentum = alpha > 0.0 && iters > 2;   // the first step has none and the last leaves t_n, not c_n
    if ((rc = c.frames.ensure((size_t)B * M * N * sizeof(float)))) return rc;
    if (momentum && (rc = c.t.ensure(bins * sizeof(float2)))) return rc;
    if (trace && (rc = c.rows.ensure((size_t)B * M * 2 * sizeof(double)))) return rc;
    if (trace && (rc = c.trace.ensure((size_t)iters * B * 2 * sizeof(double)))) return rc;
    float2 *C = static_cast<float2 *>(C_dev), *T = static_cast<float2 *>(c.t.p);
    float *frames = static_cast<float *>(c.frames.p);
    if ((rc = magnitudes(A_dev, C, bins, c.a, s))) return rc;
    const dim3 grid((M + 1) / 2, B);
    for (int i = 1; i <= iters; ++i) {
        const GlaStep st{(momentum && i >= 2 && i < iters) ? (float)alpha : 0.f, (momentum && i + 1 < iters) ? 1 : 0};
        hipLaunchKernelGGL(k_gla_inverse, grid, dim3(FFT_THREADS), g.lds, s, C, frames, g.ws, M, N, g.fc.odd, g.fc.log2e);
        if (taped) {
            hipLaunchKernelGGL((k_gla_forward<false, true>), grid, dim3(FFT_THREADS), g.lds, s, frames, g.wa, C, A_dev, T,
                               static_cast<double *>(nullptr), M, N, g.fc.odd, g.fc.log2e, fshift, g.zero_lo, g.zero_hi, st,
                               tape + (size_t)(i - 1) * bins);
        } else if (trace) {
            double *rows = static_cast<double *>(c.rows.p);
            hipLaunchKernelGGL((k_gla_forward<true, false>), grid, dim3(FFT_THREADS), g.lds, s, frames, g.wa, C, A_dev, T, rows, M, N,
                               g.fc.odd, g.fc.log2e, fshift, g.zero_lo, g.zero_hi, st, static_cast<float2 *>(nullptr));
            hipLaunchKernelGGL(k_gla_sum_rows, dim3((B + 63) / 64), dim3(64), 0, s, rows,
                               static_cast<double *>(c.trace.p) + (size_t)(i - 1) * B * 2, M, B);
        } else {
            hipLaunchKernelGGL((k_gla_forward<false, false>), grid, dim3(FFT_THREADS), g.lds, s, frames, g.wa, C, A_dev, T,
                               static_cast<double *>(nullptr), M, N, g.fc.odd, g.fc.log2e, fshift, g.zero_lo, g.zero_hi, st,
                               static_cast<float2 *>(nullptr));
        }
    }
    STFT_TRY(hipGetLastError());
    if (trace) {
        STFT_TRY(hipMemcpyAsync(trace, c.trace.p, (size_t)iters * B * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        STFT_TRY(hipStreamSynchronize(s));
    }
    return g.close();
}

}  // namespace

extern "C" int lws_griffin_lim_dev(int device, void *C_dev, const float *A_dev, int B, int M, int N, int fshift,
                                   const double *awin, const double *swin, int perfectrec, int iters, double alpha,
                                   double *trace, void *stream) {
    return gla_run(device, C_dev, A_dev, B, M, N, fshift, awin, swin, perfectrec, iters, alpha, trace, nullptr, false, stream);
}

extern "C" int lws_griffin_lim_tape_dev(int device, void *C_dev, const float *A_dev, int B, int M, int N, int fshift,
                                        const double *awin, const double *swin, int perfectrec, int iters, double alpha,
                                        void *tape_dev, void *stream) {
    return gla_run(device, C_dev, A_dev, B, M, N, fshift, awin, swin, perfectrec, iters, alpha, nullptr,
                   static_cast<float2 *>(tape_dev), true, stream);
}

extern "C" int lws_griffin_lim_backward_dev(int device, const void *gC_dev, const float *A_dev, const void *tape_dev, int B, int M,
                                            int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters,
                                            double alpha, float *gA_out, void *gS_out, void *stream) {
    int rc = check_shape(device, B, M, N, fshift);
    if (rc) return rc;
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (!(alpha >= 0.0 && alpha < 1.0)) return lws::set_error(LWS_ERR_INVALID, "momentum %g outside [0, 1)", alpha);
    if (!A_dev || !gA_out || !awin || !swin || (iters > 0 && !tape_dev)) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    if (iters > 0 && (rc = check_round_trip(M, N, fshift, perfectrec))) return rc;
    if (B == 0) return LWS_OK;
    GlaCall g(device, stream);
    if ((rc = g.open(device, N, fshift, awin, swin, perfectrec))) return rc;
    GlaCtx &c = g.c;
    hipStream_t s = g.s;
    const int F = N / 2 + 1;
    const size_t bins = (size_t)B * M * F;
    const float2 *gC = static_cast<const float2 *>(gC_dev), *tape = static_cast<const float2 *>(tape_dev);
    float2 *gS = static_cast<float2 *>(gS_out);
    if (iters == 0) {   // t_0 is the start itself
        STFT_TRY(hipMemsetAsync(gA_out, 0, bins * sizeof(float), s));
        if (gS && gC) STFT_TRY(hipMemcpyAsync(gS, gC, bins * sizeof(float2), hipMemcpyDeviceToDevice, s));
        if (gS && !gC) STFT_TRY(hipMemsetAsync(gS, 0, bins * sizeof(float2), s));
        return g.close();
    }
    if ((rc = c.frames.ensure((size_t)B * M * N * sizeof(float)))) return rc;
    if (iters > 1 && (rc = c.gc.ensure(bins * sizeof(float2)))) return rc;
    if (iters > 2 && (rc = c.gc2.ensure(bins * sizeof(float2)))) return rc;
    float *frames = static_cast<float *>(c.frames.p);
    // ga holds the gradient on c_i and gb that on c_{i+1} when step i starts; step i leaves the gradient on c_{i-1} in gb, whose
    // last reader was this step's first launch, and the two change places.  The first step run (i = iters) reads the caller's
    // cotangent instead, and the gradient on c_n, which nothing reads, is zero: no second term at i = iters - 1.
    float2 *ga = static_cast<float2 *>(c.gc2.p), *gb = static_cast<float2 *>(c.gc.p);
    const dim3 grid((M + 1) / 2, B);
    for (int i = iters; i >= 1; --i) {
        const bool entry = i == iters;
        const float ca = entry ? 1.f : 1.f + (i >= 2 ? (float)alpha : 0.f);
        const float cb = (entry || i + 1 == iters) ? 0.f : (float)alpha;
        hipLaunchKernelGGL(k_gla_bwd_project, grid, dim3(FFT_THREADS), g.lds, s, entry ? gC : static_cast<const float2 *>(ga),
                           static_cast<const float2 *>(gb), ca, cb, tape + (size_t)(i - 1) * bins, A_dev, gA_out, frames, g.wa, M, N,
                           g.fc.odd, g.fc.log2e, entry ? 1 : 0);
        if (i == 1 && !gS) break;
        hipLaunchKernelGGL(k_gla_bwd_frames, grid, dim3(FFT_THREADS), g.lds, s, frames, g.ws, i == 1 ? gS : gb, M, N, g.fc.odd,
                           g.fc.log2e, fshift, g.zero_lo, g.zero_hi);
        float2 *sw = ga; ga = gb; gb = sw;
    }
    return g.close();
}

namespace {

// lws_misi_dev, and with a tape (taped) lws_misi_tape_dev: the same launches, the forward one writing X as well
int misi_run(int device, void *C_dev, const float *A_dev, const float *y_dev, int B, int K, int M, int N, int fshift,
             const double *awin, const double *swin, int perfectrec, int iters, float *x_dev, double *trace, float2 *tape, bool taped,
             void *stream) {
    int rc = check_shape(device, B, M, N, fshift);
    if (rc) return rc;
    if (K < 1) return lws::set_error(LWS_ERR_INVALID, "%d sources", K);
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (!C_dev || !y_dev || !awin || !swin) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    if (taped && (!A_dev || (iters > 0 && !tape))) return lws::set_error(LWS_ERR_INVALID, "null magnitudes or tape");
    if ((long long)B * K > 65535) return lws::set_error(LWS_ERR_UNSUPPORTED, "%d x %d spectrograms in one call (at most 65535)", B, K);
    const int len = lws_istft_length(M, N, fshift, perfectrec);
    if (len < 1) return lws::set_error(LWS_ERR_INVALID, "%d frames leave no samples", M);
    if (iters > 0 && (rc = check_round_trip(M, N, fshift, perfectrec))) return rc;
    if (B == 0 || (iters == 0 && !x_dev)) return LWS_OK;
    GlaCall g(device, stream);
    if ((rc = g.open(device, N, fshift, awin, swin, perfectrec))) return rc;
    GlaCtx &c = g.c;
    hipStream_t s = g.s;
    const int F = N / 2 + 1, BK = B * K, Tfull = fshift * (M - 1) + N, nblk = (Tfull + 255) / 256;
    const size_t bins = (size_t)BK * M * F;
    const bool want_trace = trace && iters > 0;
    if ((rc = c.frames.ensure((size_t)BK * M * N * sizeof(float)))) return rc;
    if ((rc = c.delta.ensure((size_t)B * Tfull * sizeof(float)))) return rc;
    if ((rc = c.sig.ensure((size_t)BK * Tfull * sizeof(float)))) return rc;
    if (want_trace && (rc = c.rows.ensure((size_t)B * nblk * 2 * sizeof(double)))) return rc;
    if (want_trace && (rc = c.trace.ensure((size_t)iters * B * 2 * sizeof(double)))) return rc;
    float2 *C = static_cast<float2 *>(C_dev);
    float *frames = static_cast<float *>(c.frames.p), *delta = static_cast<float *>(c.delta.p);
    float *sig = static_cast<float *>(c.sig.p);
    double *rows = static_cast<double *>(c.rows.p);
    if (iters > 0 && (rc = magnitudes(A_dev, C, bins, c.a, s))) return rc;
    const dim3 grid((M + 1) / 2, BK), rgrid(nblk, B);
    const int zero_lo = g.zero_lo, zero_hi = g.zero_hi;
    for (int i = 1; i <= iters; ++i) {
        hipLaunchKernelGGL(k_gla_inverse, grid, dim3(FFT_THREADS), g.lds, s, C, frames, g.ws, M, N, g.fc.odd, g.fc.log2e);
        if (want_trace) {
            hipLaunchKernelGGL(k_misi_residual<true>, rgrid, dim3(256), 0, s, frames, y_dev, delta, sig, rows, K, M, N, fshift, zero_lo, zero_hi);
            hipLaunchKernelGGL(k_gla_sum_rows, dim3((B + 63) / 64), dim3(64), 0, s, rows,
                               static_cast<double *>(c.trace.p) + (size_t)(i - 1) * B * 2, nblk, B);
        } else {
            hipLaunchKernelGGL(k_misi_residual<false>, rgrid, dim3(256), 0, s, frames, y_dev, delta, sig, static_cast<double *>(nullptr), K,
                               M, N, fshift, zero_lo, zero_hi);
        }
        if (taped)
            hipLaunchKernelGGL(k_misi_forward<true>, grid, dim3(FFT_THREADS), g.lds, s, sig, delta, g.wa, C, A_dev, K, M, N, g.fc.odd,
                               g.fc.log2e, fshift, tape + (size_t)(i - 1) * bins);
        else
            hipLaunchKernelGGL(k_misi_forward<false>, grid, dim3(FFT_THREADS), g.lds, s, sig, delta, g.wa, C, A_dev, K, M, N, g.fc.odd,
                               g.fc.log2e, fshift, static_cast<float2 *>(nullptr));
    }
    if (x_dev) {   // the signals of the final iterate, with their own residual shared out
        hipLaunchKernelGGL(k_gla_inverse, grid, dim3(FFT_THREADS), g.lds, s, C, frames, g.ws, M, N, g.fc.odd, g.fc.log2e);
        hipLaunchKernelGGL(k_misi_residual<false>, rgrid, dim3(256), 0, s, frames, y_dev, delta, sig, static_cast<double *>(nullptr), K,
                           M, N, fshift, zero_lo, zero_hi);
        hipLaunchKernelGGL(k_misi_signals, dim3((len + 255) / 256, BK), dim3(256), 0, s, sig, delta, x_dev, K, Tfull, zero_lo, len);
    }
    STFT_TRY(hipGetLastError());
    if (want_trace) {
        STFT_TRY(hipMemcpyAsync(trace, c.trace.p, (size_t)iters * B * 2 * sizeof(double), hipMemcpyDeviceToHost, s));
        STFT_TRY(hipStreamSynchronize(s));
    }
    return g.close();
}

}  // namespace

extern "C" int lws_misi_dev(int device, void *C_dev, const float *A_dev, const float *y_dev, int B, int K, int M, int N, int fshift,
                            const double *awin, const double *swin, int perfectrec, int iters, float *x_dev, double *trace,
                            void *stream) {
    return misi_run(device, C_dev, A_dev, y_dev, B, K, M, N, fshift, awin, swin, perfectrec, iters, x_dev, trace, nullptr, false, stream);
}

extern "C" int lws_misi_tape_dev(int device, void *C_dev, const float *A_dev, const float *y_dev, int B, int K, int M, int N, int fshift,
                                 const double *awin, const double *swin, int perfectrec, int iters, float *x_dev, void *tape_dev,
                                 void *stream) {
    return misi_run(device, C_dev, A_dev, y_dev, B, K, M, N, fshift, awin, swin, perfectrec, iters, x_dev, nullptr,
                    static_cast<float2 *>(tape_dev), true, stream);
}

extern "C" int lws_misi_backward_dev(int device, const void *gC_dev, const float *gx_dev, const float *A_dev, const void *tape_dev, int B,
                                     int K, int M, int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters,
                                     float *gA_out, void *gS_out, float *gy_out, void *stream) {
    int rc = check_shape(device, B, M, N, fshift);
    if (rc) return rc;
    if (K < 1) return lws::set_error(LWS_ERR_INVALID, "%d sources", K);
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (!A_dev || !gA_out || !awin || !swin || (iters > 0 && !tape_dev)) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    if ((long long)B * K > 65535) return lws::set_error(LWS_ERR_UNSUPPORTED, "%d x %d spectrograms in one call (at most 65535)", B, K);
    const int len = lws_istft_length(M, N, fshift, perfectrec);
    if (len < 1) return lws::set_error(LWS_ERR_INVALID, "%d frames leave no samples", M);
    if (iters > 0 && (rc = check_round_trip(M, N, fshift, perfectrec))) return rc;
    if (B == 0) return LWS_OK;
    GlaCall g(device, stream);
    if ((rc = g.open(device, N, fshift, awin, swin, perfectrec))) return rc;
    GlaCtx &c = g.c;
    hipStream_t s = g.s;
    const int F = N / 2 + 1, BK = B * K, Tfull = fshift * (M - 1) + N, nblk = (Tfull + 255) / 256;
    const size_t bins = (size_t)BK * M * F;
    if (iters > 0 && (rc = c.frames.ensure((size_t)BK * M * N * sizeof(float)))) return rc;
    if ((rc = c.sig.ensure((size_t)BK * Tfull * sizeof(float)))) return rc;
    if (iters > 0 && (rc = c.gc.ensure(bins * sizeof(float2)))) return rc;
    float *frames = static_cast<float *>(c.frames.p), *gsig = static_cast<float *>(c.sig.p);
    float2 *gc = static_cast<float2 *>(c.gc.p), *gS = static_cast<float2 *>(gS_out);
    const float2 *gC = static_cast<const float2 *>(gC_dev), *tape = static_cast<const float2 *>(tape_dev);
    const dim3 grid((M + 1) / 2, BK), rgrid(nblk, B);
    if (iters == 0) STFT_TRY(hipMemsetAsync(gA_out, 0, bins * sizeof(float), s));
    // the gradient on c_i, i = iters .. 0: from the cotangents on entry, through one iteration each after that; the one on c_0 is
    // the result for the start and goes to the caller (or nowhere)
    for (int i = iters; i >= 0; --i) {
        const bool entry = i == iters;
        if (!entry)
            hipLaunchKernelGGL(k_misi_bwd_project, grid, dim3(FFT_THREADS), g.lds, s, gc, tape + (size_t)i * bins, A_dev, gA_out, frames,
                               g.wa, M, N, g.fc.odd, g.fc.log2e, i + 1 == iters ? 1 : 0);
        if (i == 0 && !gS && !gy_out) break;
        if (entry)
            hipLaunchKernelGGL(k_misi_bwd_share<true>, rgrid, dim3(256), 0, s, gx_dev, gsig, gy_out, K, M, N, fshift, g.zero_lo, g.zero_hi, 1);
        else
            hipLaunchKernelGGL(k_misi_bwd_share<false>, rgrid, dim3(256), 0, s, frames, gsig, gy_out, K, M, N, fshift, g.zero_lo, g.zero_hi, 0);
        if (i == 0 && !gS) break;
        hipLaunchKernelGGL(k_misi_bwd_frames, grid, dim3(FFT_THREADS), g.lds, s, gsig, g.ws, entry ? gC : static_cast<const float2 *>(nullptr),
                           i == 0 ? gS : gc, M, N, g.fc.odd, g.fc.log2e, fshift);
    }
    return g.close();
}

namespace {

// Where the state of a look-ahead kernel lives: behind the transform buffers in LDS if all of it fits there, in device scratch
// otherwise.  K == 0: the one spectrogram of k_rtisi.  K sources (k_misi_la): K such states and the (K + 1) R floats of the coupling.
struct LaPlacement {
    size_t source_floats, all_floats, lds_bytes;   // state of one spectrogram (R + 2 (LA + 1) N), of a workgroup; the launch's LDS
    bool in_lds;
    int threads;   // one workgroup per CU and every step behind a barrier: a thread per sample, up to 16 waves, hides the LDS latency
};
LaPlacement la_placement(int N, int hop, int LA, int K) {
    LaPlacement p;
    p.source_floats = la_state_floats(N, hop, LA);
    p.all_floats = K == 0 ? p.source_floats : (size_t)K * p.source_floats + ((size_t)K + 1) * ((size_t)N + (size_t)LA * hop);
    const size_t all = fft_lds_bytes(N) + p.all_floats * sizeof(float);
    p.in_lds = all <= RTISI_LDS_CAP;
    p.lds_bytes = p.in_lds ? all : fft_lds_bytes(N);
    p.threads = N <= FFT_THREADS ? FFT_THREADS : N >= RTISI_MAX_THREADS ? RTISI_MAX_THREADS : (N + FFT_THREADS - 1) / FFT_THREADS * FFT_THREADS;
    return p;
}

}  // namespace

extern "C" int lws_rtisi_la_placement(int N, int fshift, int look_ahead, int K, int *in_lds, int *threads, size_t *lds_bytes) {
    if (N < 1 || fshift < 1 || look_ahead < 0 || K < 0)
        return lws::set_error(LWS_ERR_INVALID, "placement of N = %d, hop %d, look-ahead %d, %d sources", N, fshift, look_ahead, K);
    const LaPlacement p = la_placement(N, fshift, look_ahead, K);
    if (in_lds) *in_lds = p.in_lds ? 1 : 0;
    if (threads) *threads = p.threads;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return LWS_OK;
}

extern "C" int lws_rtisi_la_dev(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift,
                                const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, void *stream) {
    return lws_rtisi_la_dev_ex(device, C_dev, A_dev, x_dev, B, M, N, fshift, awin, swin, perfectrec, iters, look_ahead, LWS_START_GIVEN,
                               stream);
}

namespace {

// The state of k_rtisi_bwd: gdone, G and Gn over the active window, 3 R floats (never more than the forward's R + 2 (LA + 1) N),
// behind the transform buffers in LDS if that fits, in device scratch otherwise.  The workgroup is the forward's.
LaPlacement la_bwd_placement(int N, int hop, int LA) {
    LaPlacement p;
    p.source_floats = p.all_floats = 3 * ((size_t)N + (size_t)LA * hop);
    const size_t all = fft_lds_bytes(N) + p.all_floats * sizeof(float);
    p.in_lds = all <= RTISI_LDS_CAP;
    p.lds_bytes = p.in_lds ? all : fft_lds_bytes(N);
    p.threads = la_placement(N, hop, LA, 0).threads;
    return p;
}

// lws_rtisi_la_dev_ex, and with a tape (taped, under LWS_START_GIVEN) lws_rtisi_la_tape_dev: the same launch, the projection writing
// its argument as well
int rtisi_run(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift, const double *awin,
              const double *swin, int perfectrec, int iters, int look_ahead, int start, float2 *tape, bool taped, void *stream);

}  // namespace

extern "C" int lws_rtisi_la_bwd_placement(int N, int fshift, int look_ahead, int *in_lds, int *threads, size_t *lds_bytes) {
    if (N < 1 || fshift < 1 || look_ahead < 0)
        return lws::set_error(LWS_ERR_INVALID, "placement of N = %d, hop %d, look-ahead %d", N, fshift, look_ahead);
    const LaPlacement p = la_bwd_placement(N, fshift, look_ahead);
    if (in_lds) *in_lds = p.in_lds ? 1 : 0;
    if (threads) *threads = p.threads;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return LWS_OK;
}

extern "C" int lws_rtisi_la_dev_ex(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift,
                                   const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, int start,
                                   void *stream) {
    return rtisi_run(device, C_dev, A_dev, x_dev, B, M, N, fshift, awin, swin, perfectrec, iters, look_ahead, start, nullptr, false,
                     stream);
}

extern "C" int lws_rtisi_la_tape_dev(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift,
                                     const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, void *tape_dev,
                                     void *stream) {
    return rtisi_run(device, C_dev, A_dev, x_dev, B, M, N, fshift, awin, swin, perfectrec, iters, look_ahead, LWS_START_GIVEN,
                     static_cast<float2 *>(tape_dev), true, stream);
}

extern "C" int lws_rtisi_la_backward_dev(int device, const void *gC_dev, const float *gx_dev, const float *A_dev, const void *tape_dev,
                                         int B, int M, int N, int fshift, const double *awin, const double *swin, int perfectrec,
                                         int iters, int look_ahead, float *gA_out, void *gS_out, void *stream) {
    int rc = check_shape(device, B, M, N, fshift);
    if (rc) return rc;
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (look_ahead < 0) return lws::set_error(LWS_ERR_INVALID, "look-ahead of %d frames", look_ahead);
    if (!A_dev || !gA_out || !awin || !swin || (iters > 0 && !tape_dev)) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    if (iters > 0 && (rc = check_round_trip(M, N, fshift, perfectrec))) return rc;
    if (B == 0) return LWS_OK;
    GlaCall g(device, stream);
    if ((rc = g.open(device, N, fshift, awin, swin, perfectrec))) return rc;
    const int F = N / 2 + 1, LA = look_ahead < M - 1 ? look_ahead : M - 1, len = lws_istft_length(M, N, fshift, perfectrec);
    STFT_TRY(hipMemsetAsync(gA_out, 0, (size_t)B * M * F * sizeof(float), g.s));   // the kernel adds to it
    if (iters == 0 && !gS_out) return g.close();
    const LaPlacement p = la_bwd_placement(N, fshift, LA);
    if (!p.in_lds && (rc = g.c.state.ensure((size_t)B * p.all_floats * sizeof(float)))) return rc;
    const RtisiArgs a{M, N, g.fc.odd, g.fc.log2e, fshift, LA, iters, g.zero_lo, g.zero_hi, len < 0 ? 0 : len, p.all_floats};
    float *scratch = p.in_lds ? nullptr : static_cast<float *>(g.c.state.p);
    auto *kernel = p.in_lds ? k_rtisi_bwd<true> : k_rtisi_bwd<false>;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(p.threads), p.lds_bytes, g.s, static_cast<const float2 *>(gC_dev), len < 1 ? nullptr : gx_dev,
                       A_dev, static_cast<const float2 *>(tape_dev), gA_out, static_cast<float2 *>(gS_out), g.wa, g.ws, scratch, a);
    return g.close();
}

namespace {

int rtisi_run(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift, const double *awin,
              const double *swin, int perfectrec, int iters, int look_ahead, int start, float2 *tape, bool taped, void *stream) {
    int rc = check_shape(device, B, M, N, fshift);
    if (rc) return rc;
    if (start != LWS_START_GIVEN && start != LWS_START_OVERLAP) return lws::set_error(LWS_ERR_INVALID, "start %d for RTISI-LA", start);
    const bool given = start == LWS_START_GIVEN;
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (look_ahead < 0) return lws::set_error(LWS_ERR_INVALID, "look-ahead of %d frames", look_ahead);
    if (!C_dev || !awin || !swin) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    if (taped && (!A_dev || (iters > 0 && !tape))) return lws::set_error(LWS_ERR_INVALID, "null magnitudes or tape");
    if (iters > 0 && (rc = check_round_trip(M, N, fshift, perfectrec))) return rc;
    const int len = lws_istft_length(M, N, fshift, perfectrec);
    if (B == 0 || (given && iters == 0 && (!x_dev || len < 1))) return LWS_OK;   // an entry estimate is a result without iterations too
    GlaCall g(device, stream);
    if ((rc = g.open(device, N, fshift, awin, swin, perfectrec))) return rc;
    const int F = N / 2 + 1, LA = look_ahead < M - 1 ? look_ahead : M - 1;   // no frame beyond M - 1 to look at
    const LaPlacement p = la_placement(N, fshift, LA, 0);
    if (!p.in_lds && (rc = g.c.state.ensure((size_t)B * p.all_floats * sizeof(float)))) return rc;
    float2 *C = static_cast<float2 *>(C_dev);
    if ((iters > 0 || !given) && (rc = magnitudes(A_dev, C, (size_t)B * M * F, g.c.a, g.s))) return rc;   // the entry projection reads A
    const RtisiArgs a{M, N, g.fc.odd, g.fc.log2e, fshift, LA, iters, g.zero_lo, g.zero_hi, len, p.source_floats};
    float *x = len < 1 ? nullptr : x_dev, *scratch = p.in_lds ? nullptr : static_cast<float *>(g.c.state.p);
    if (taped && iters > 0) {   // without iterations nothing is projected: the untaped kernel
        auto *kernel = p.in_lds ? k_rtisi_tape<true, LWS_START_GIVEN> : k_rtisi_tape<false, LWS_START_GIVEN>;
        hipLaunchKernelGGL(kernel, dim3(B), dim3(p.threads), p.lds_bytes, g.s, C, A_dev, x, g.wa, g.ws, scratch, a, tape);
        return g.close();
    }
    auto *kernel = p.in_lds ? (given ? k_rtisi<true, LWS_START_GIVEN> : k_rtisi<true, LWS_START_OVERLAP>)
                            : (given ? k_rtisi<false, LWS_START_GIVEN> : k_rtisi<false, LWS_START_OVERLAP>);
    hipLaunchKernelGGL(kernel, dim3(B), dim3(p.threads), p.lds_bytes, g.s, C, A_dev, x, g.wa, g.ws, scratch, a);
    return g.close();
}

}  // namespace

extern "C" int lws_misi_la_dev(int device, void *C_dev, const float *A_dev, const float *y_dev, float *x_dev, int B, int K, int M, int N,
                               int fshift, const double *awin, const double *swin, int perfectrec, int iters, int look_ahead,
                               void *stream) {
    return lws_misi_la_dev_ex(device, C_dev, A_dev, y_dev, x_dev, B, K, M, N, fshift, awin, swin, perfectrec, iters, look_ahead,
                              LWS_START_GIVEN, stream);
}

extern "C" int lws_misi_la_dev_ex(int device, void *C_dev, const float *A_dev, const float *y_dev, float *x_dev, int B, int K, int M,
                                  int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters, int look_ahead,
                                  int start, void *stream) {
    int rc = check_shape(device, B, M, N, fshift);
    if (rc) return rc;
    if (start != LWS_START_GIVEN && start != LWS_START_MIXTURE) return lws::set_error(LWS_ERR_INVALID, "start %d for online MISI", start);
    const bool given = start == LWS_START_GIVEN;
    if (K < 1) return lws::set_error(LWS_ERR_INVALID, "%d sources", K);
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (look_ahead < 0) return lws::set_error(LWS_ERR_INVALID, "look-ahead of %d frames", look_ahead);
    if (!C_dev || !y_dev || !awin || !swin) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    const int len = lws_istft_length(M, N, fshift, perfectrec);
    if (len < 1) return lws::set_error(LWS_ERR_INVALID, "%d frames leave no samples", M);
    if (iters > 0 && (rc = check_round_trip(M, N, fshift, perfectrec))) return rc;
    if (B == 0 || (given && iters == 0 && !x_dev)) return LWS_OK;   // an entry estimate is a result without iterations too
    GlaCall g(device, stream);
    if ((rc = g.open(device, N, fshift, awin, swin, perfectrec))) return rc;
    const int F = N / 2 + 1, LA = look_ahead < M - 1 ? look_ahead : M - 1;   // no frame beyond M - 1 to look at
    const LaPlacement p = la_placement(N, fshift, LA, K);
    if (!p.in_lds && (rc = g.c.state.ensure((size_t)B * p.all_floats * sizeof(float)))) return rc;
    float2 *C = static_cast<float2 *>(C_dev);
    if ((iters > 0 || !given) && (rc = magnitudes(A_dev, C, (size_t)B * K * M * F, g.c.a, g.s))) return rc;   // the entry projection reads A
    const MisiLaArgs q{{M, N, g.fc.odd, g.fc.log2e, fshift, LA, iters, g.zero_lo, g.zero_hi, len, p.source_floats}, K, p.all_floats};
    float *scratch = p.in_lds ? nullptr : static_cast<float *>(g.c.state.p);
    auto *kernel = p.in_lds ? (given ? k_misi_la<true, LWS_START_GIVEN> : k_misi_la<true, LWS_START_MIXTURE>)
                            : (given ? k_misi_la<false, LWS_START_GIVEN> : k_misi_la<false, LWS_START_MIXTURE>);
    hipLaunchKernelGGL(kernel, dim3(B), dim3(p.threads), p.lds_bytes, g.s, C, A_dev, y_dev, x_dev, g.wa, g.ws, scratch, q);
    return g.close();
}

// ---- The look-ahead streams: one handle for lws_rtisi_stream (K == 0) and lws_misi_stream (K sources of each of B mixtures).  What a
// stream carries between calls is its own -- state, held rows, (K > 0) held mixture samples and, with the scratch placement, the room
// for target and xs, windows, the magnitudes of a chunk given without them -- so streams share nothing with each other or with the
// calls on GlaCtx.  What a call does is decided by the clock (lws_la_stream.h); only la_launch knows which kernel runs.
struct lws_la_stream {
    int device = 0, B = 0;
    LaClock clock;
    Scratch state, held_s[2], held_a[2], held_y[2], abuf, win_a, win_s;
    hipEvent_t last = nullptr;            // the event scheme of GlaCtx, for a caller that changes streams between calls
    hipStream_t last_stream = nullptr;
    bool busy = false;
    std::mutex mu;
};
struct lws_rtisi_stream : lws_la_stream {};
struct lws_misi_stream : lws_la_stream {};

namespace {

int la_enter(lws_la_stream &h, hipStream_t s) {
    if (h.busy && s != h.last_stream) STFT_TRY(hipStreamWaitEvent(s, h.last, 0));
    return LWS_OK;
}
int la_leave(lws_la_stream &h, hipStream_t s) {
    STFT_TRY(hipEventRecord(h.last, s));
    h.busy = true;
    h.last_stream = s;
    return LWS_OK;
}

// a chunk's rows, and the samples under them, into the held buffers the next launch reads: what arrives before the first commit can run
int la_stash(lws_la_stream &h, const LaPlan &p, const float2 *S, const float *A, const float *y, int frames, int samples, hipStream_t s) {
    const LaClock &c = h.clock;
    const size_t F = (size_t)c.N / 2 + 1, at = (size_t)p.stash_row, specs = (size_t)h.B * (c.K ? c.K : 1);
    if (c.given)   // no other start reads the rows
        STFT_TRY(hipMemcpy2DAsync(static_cast<float2 *>(h.held_s[p.write].p) + at * F, (size_t)c.LA * F * sizeof(float2), S,
                                  (size_t)frames * F * sizeof(float2), (size_t)frames * F * sizeof(float2), specs,
                                  hipMemcpyDeviceToDevice, s));
    if (A)
        STFT_TRY(hipMemcpy2DAsync(static_cast<float *>(h.held_a[p.write].p) + at * F, (size_t)c.LA * F * sizeof(float), A,
                                  (size_t)frames * F * sizeof(float), (size_t)frames * F * sizeof(float), specs, hipMemcpyDeviceToDevice,
                                  s));
    if (c.K)
        STFT_TRY(hipMemcpy2DAsync(static_cast<float *>(h.held_y[p.write].p) + p.stash_y, (size_t)c.y_rows * sizeof(float), y,
                                  (size_t)samples * sizeof(float), (size_t)samples * sizeof(float), h.B, hipMemcpyDeviceToDevice, s));
    return LWS_OK;
}

int la_launch(lws_la_stream &h, const LaPlan &p, const float2 *S, const float *A, const float *y, float2 *C_out, float *x_out,
              hipStream_t s) {
    const LaClock &c = h.clock;
    const LaPlacement pl = la_placement(c.N, c.hop, p.a.r.LA, c.K);
    const float2 *hs = static_cast<const float2 *>(h.held_s[p.read].p);
    const float *ha = static_cast<const float *>(h.held_a[p.read].p), *hy = static_cast<const float *>(h.held_y[p.read].p);
    float2 *s_next = p.keep_s ? static_cast<float2 *>(h.held_s[p.write].p) : nullptr;
    float *a_next = p.keep_a ? static_cast<float *>(h.held_a[p.write].p) : nullptr;
    float *y_next = p.keep_y ? static_cast<float *>(h.held_y[p.write].p) : nullptr;
    const float *wa = static_cast<const float *>(h.win_a.p), *ws = static_cast<const float *>(h.win_s.p);
    float *st = static_cast<float *>(h.state.p);
    const dim3 grid(h.B), block(pl.threads);
    if (c.K == 0) {
        auto *kernel = pl.in_lds ? (c.given ? k_rtisi_stream<true, LWS_START_GIVEN> : k_rtisi_stream<true, LWS_START_OVERLAP>)
                                 : (c.given ? k_rtisi_stream<false, LWS_START_GIVEN> : k_rtisi_stream<false, LWS_START_OVERLAP>);
        hipLaunchKernelGGL(kernel, grid, block, pl.lds_bytes, s, S, A, C_out, x_out, wa, ws, st, RtisiHeld{hs, ha, s_next, a_next}, p.a.r);
    } else {
        auto *kernel = pl.in_lds ? (c.given ? k_misi_la_stream<true, LWS_START_GIVEN> : k_misi_la_stream<true, LWS_START_MIXTURE>)
                                 : (c.given ? k_misi_la_stream<false, LWS_START_GIVEN> : k_misi_la_stream<false, LWS_START_MIXTURE>);
        hipLaunchKernelGGL(kernel, grid, block, pl.lds_bytes, s, S, A, y, C_out, x_out, wa, ws, st,
                           MisiStreamHeld{hs, ha, hy, s_next, a_next, y_next}, p.a);
    }
    STFT_TRY(hipGetLastError());
    return LWS_OK;
}

void la_destroy(lws_la_stream *h) {
    (void)hipSetDevice(h->device);
    for (Scratch *b : {&h->state, &h->held_s[0], &h->held_s[1], &h->held_a[0], &h->held_a[1], &h->held_y[0], &h->held_y[1], &h->abuf,
                       &h->win_a, &h->win_s})
        if (b->p) (void)hipFree(b->p);
    if (h->last) (void)hipEventDestroy(h->last);
}

// mixture: a lws_misi_stream of K >= 1 sources (other start: LWS_START_MIXTURE); else a lws_rtisi_stream, K == 0 (LWS_START_OVERLAP)
template <class Handle>
int la_create(int device, int B, int K, int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters,
              int look_ahead, int start, bool mixture, Handle **out) {
    if (!out) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    *out = nullptr;
    int rc = check_shape(device, B, 1, N, fshift);
    if (rc) return rc;
    if (start != LWS_START_GIVEN && start != (mixture ? LWS_START_MIXTURE : LWS_START_OVERLAP))
        return lws::set_error(LWS_ERR_INVALID, "start %d for %s", start, mixture ? "online MISI" : "RTISI-LA");
    const bool given = start == LWS_START_GIVEN;
    if (B < 1) return lws::set_error(LWS_ERR_INVALID, "%d streams", B);
    if (mixture && K < 1) return lws::set_error(LWS_ERR_INVALID, "%d sources", K);
    if (iters < 0) return lws::set_error(LWS_ERR_INVALID, "%d iterations", iters);
    if (look_ahead < 0) return lws::set_error(LWS_ERR_INVALID, "look-ahead of %d frames", look_ahead);
    if (!awin || !swin) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    if (!la_look_ahead_fits(N, fshift, look_ahead, K)) return lws::set_error(LWS_ERR_UNSUPPORTED, "look-ahead of %d frames", look_ahead);
    STFT_TRY(hipSetDevice(device));
    if ((rc = allow_lds_all())) return rc;
    Handle *h = new Handle;
    h->device = device; h->B = B;
    LaClock &c = h->clock;
    la_clock_init(c, N, fshift, look_ahead, iters, K, perfectrec != 0, given, la_placement(N, fshift, look_ahead, K).in_lds);
    const size_t F = (size_t)N / 2 + 1, rows = (size_t)B * (K ? K : 1) * look_ahead * F;
    const size_t state_bytes = (size_t)B * (K ? c.stream_floats : c.state_floats) * sizeof(float);
    const size_t y_bytes = (size_t)B * c.y_rows * sizeof(float);
    std::vector<float> wa(N), ws(N);
    for (int i = 0; i < N; ++i) { wa[i] = (float)awin[i]; ws[i] = (float)swin[i]; }
    rc = h->state.ensure(state_bytes);
    if (!rc) rc = h->win_a.ensure((size_t)N * sizeof(float));
    if (!rc) rc = h->win_s.ensure((size_t)N * sizeof(float));
    if (!rc && K) rc = h->held_y[0].ensure(y_bytes);
    if (!rc && K) rc = h->held_y[1].ensure(y_bytes);
    if (!rc && (given || iters == 0)) rc = h->held_s[0].ensure(rows * sizeof(float2));   // start rows, or entry rows to return
    if (!rc && iters == 0) rc = h->held_s[1].ensure(rows * sizeof(float2));
    if (!rc && (iters > 0 || !given)) rc = h->held_a[0].ensure(rows * sizeof(float));
    if (!rc && (iters > 0 || !given)) rc = h->held_a[1].ensure(rows * sizeof(float));
    hipError_t e = hipSuccess;
    if (!rc) e = hipEventCreateWithFlags(&h->last, hipEventDisableTiming);
    if (!rc && e == hipSuccess) e = hipMemset(h->state.p, 0, state_bytes);
    if (!rc && e == hipSuccess && K) e = hipMemset(h->held_y[0].p, 0, y_bytes);
    if (!rc && e == hipSuccess && K) e = hipMemset(h->held_y[1].p, 0, y_bytes);
    if (!rc && e == hipSuccess) e = hipMemcpy(h->win_a.p, wa.data(), (size_t)N * sizeof(float), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) e = hipMemcpy(h->win_s.p, ws.data(), (size_t)N * sizeof(float), hipMemcpyHostToDevice);
    if (!rc && e == hipSuccess) e = hipDeviceSynchronize();   // the state is zero before any stream of the caller's touches it
    if (!rc && e != hipSuccess) rc = lws::set_error(LWS_ERR_HIP, "creating a stream's state failed: %s", hipGetErrorString(e));
    if (rc) {
        la_destroy(h);
        delete h;
        return rc;
    }
    *out = h;
    return LWS_OK;
}

int la_push(lws_la_stream *h, const void *S_dev, const float *A_dev, const float *y_dev, int frames, int samples, void *C_out_dev,
            float *x_out_dev, int *frames_out, int *samples_out, void *stream) {
    if (frames_out) *frames_out = 0;
    if (samples_out) *samples_out = 0;
    if (!h) return lws::set_error(LWS_ERR_INVALID, "null stream handle");
    std::lock_guard<std::mutex> lk(h->mu);
    LaClock &c = h->clock;
    long long want = 0;
    switch (la_check_push(c, frames, samples, &want)) {
    case LA_NEGATIVE: return lws::set_error(LWS_ERR_INVALID, "%d frames", frames);
    case LA_FINISHED: return lws::set_error(LWS_ERR_INVALID, "push after finish");
    case LA_TOO_LONG: return lws::set_error(LWS_ERR_UNSUPPORTED, "%d frames in one push", frames);
    case LA_SAMPLES:
        return lws::set_error(LWS_ERR_INVALID, "%d mixture samples for %d frames after %lld: expected %lld", samples, frames, c.entered,
                              want);
    case LA_GO: break;
    }
    if (frames == 0) return LWS_OK;
    const bool given = c.given;
    if ((!S_dev && (given || !A_dev)) || (c.K && !y_dev))   // magnitudes alone serve any other start
        return lws::set_error(LWS_ERR_INVALID, "null pointer");
    const LaPlan p = la_plan_push(c, frames, samples);
    if (p.launch && !C_out_dev) return lws::set_error(LWS_ERR_INVALID, "null pointer");
    STFT_TRY(hipSetDevice(h->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = la_enter(*h, s);
    if (rc) return rc;
    const float2 *S = static_cast<const float2 *>(S_dev);
    const size_t bins = (size_t)h->B * (c.K ? c.K : 1) * frames * (c.N / 2 + 1);
    if ((c.iters > 0 || !given) && (rc = magnitudes(A_dev, S, bins, h->abuf, s))) return rc;   // |S| by the kernel the one-shot calls use
    if (given && c.iters == 0) A_dev = nullptr;
    rc = p.launch ? la_launch(*h, p, S, A_dev, y_dev, static_cast<float2 *>(C_out_dev), x_out_dev, s)
                  : la_stash(*h, p, S, A_dev, y_dev, frames, samples, s);
    if (rc) return rc;
    c = p.after;
    if (frames_out) *frames_out = p.frames_out;
    if (samples_out) *samples_out = p.samples_out;
    return la_leave(*h, s);
}

int la_finish(lws_la_stream *h, void *C_out_dev, float *x_out_dev, int *frames_out, int *samples_out, void *stream) {
    if (frames_out) *frames_out = 0;
    if (samples_out) *samples_out = 0;
    if (!h) return lws::set_error(LWS_ERR_INVALID, "null stream handle");
    std::lock_guard<std::mutex> lk(h->mu);
    LaClock &c = h->clock;
    if (la_check_finish(c) != LA_GO) return lws::set_error(LWS_ERR_INVALID, "finish after finish");
    const LaPlan p = la_plan_finish(c, x_out_dev != nullptr);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (p.launch) {
        if (p.a.r.nsteps > 0 && !C_out_dev) return lws::set_error(LWS_ERR_INVALID, "null pointer");
        STFT_TRY(hipSetDevice(h->device));
        int rc = la_enter(*h, s);
        if (!rc) rc = la_launch(*h, p, nullptr, nullptr, nullptr, static_cast<float2 *>(C_out_dev), x_out_dev, s);
        if (rc) return rc;
    }
    c = p.after;
    if (frames_out) *frames_out = p.frames_out;
    if (samples_out) *samples_out = p.samples_out;
    return p.launch ? la_leave(*h, s) : LWS_OK;
}

}  // namespace

extern "C" int lws_rtisi_stream_create(int device, int B, int N, int fshift, const double *awin, const double *swin, int perfectrec,
                                       int iters, int look_ahead, lws_rtisi_stream **out) {
    return lws_rtisi_stream_create_ex(device, B, N, fshift, awin, swin, perfectrec, iters, look_ahead, LWS_START_GIVEN, out);
}
extern "C" int lws_rtisi_stream_create_ex(int device, int B, int N, int fshift, const double *awin, const double *swin, int perfectrec,
                                          int iters, int look_ahead, int start, lws_rtisi_stream **out) {
    return la_create(device, B, 0, N, fshift, awin, swin, perfectrec, iters, look_ahead, start, false, out);
}
extern "C" int lws_rtisi_stream_push(lws_rtisi_stream *h, const void *S_dev, const float *A_dev, int frames, void *C_out_dev,
                                     float *x_out_dev, int *frames_out, int *samples_out, void *stream) {
    return la_push(h, S_dev, A_dev, nullptr, frames, 0, C_out_dev, x_out_dev, frames_out, samples_out, stream);
}
extern "C" int lws_rtisi_stream_finish(lws_rtisi_stream *h, void *C_out_dev, float *x_out_dev, int *frames_out, int *samples_out,
                                       void *stream) {
    return la_finish(h, C_out_dev, x_out_dev, frames_out, samples_out, stream);
}
extern "C" void lws_rtisi_stream_destroy(lws_rtisi_stream *h) {
    if (!h) return;
    la_destroy(h);
    delete h;
}

extern "C" int lws_misi_stream_create(int device, int B, int K, int N, int fshift, const double *awin, const double *swin,
                                      int perfectrec, int iters, int look_ahead, lws_misi_stream **out) {
    return lws_misi_stream_create_ex(device, B, K, N, fshift, awin, swin, perfectrec, iters, look_ahead, LWS_START_GIVEN, out);
}
extern "C" int lws_misi_stream_create_ex(int device, int B, int K, int N, int fshift, const double *awin, const double *swin,
                                         int perfectrec, int iters, int look_ahead, int start, lws_misi_stream **out) {
    return la_create(device, B, K, N, fshift, awin, swin, perfectrec, iters, look_ahead, start, true, out);
}
extern "C" int lws_misi_stream_push(lws_misi_stream *h, const void *S_dev, const float *A_dev, const float *y_dev, int frames,
                                    int samples, void *C_out_dev, float *x_out_dev, int *frames_out, int *samples_out, void *stream) {
    return la_push(h, S_dev, A_dev, y_dev, frames, samples, C_out_dev, x_out_dev, frames_out, samples_out, stream);
}
extern "C" int lws_misi_stream_finish(lws_misi_stream *h, void *C_out_dev, float *x_out_dev, int *frames_out, int *samples_out,
                                      void *stream) {
    return la_finish(h, C_out_dev, x_out_dev, frames_out, samples_out, stream);
}
extern "C" void lws_misi_stream_destroy(lws_misi_stream *h) {
    if (!h) return;
    la_destroy(h);
    delete h;
}
