// lws_rtisi_kernels.h -- the one-shot kernels of RTISI-LA (k_rtisi, k_rtisi_tape: the text of lws_rtisi_march.h, compiled twice) and
// its backward pass (k_rtisi_bwd), part of the one translation unit lws_gla.hip (whose header comment is the map of these files).
// RtisiArgs and the rtisi_* helpers serve the other look-ahead kernels too; rtisi_put_pair every backward pass.
#pragma once

#include "lws_fft.h"

namespace {

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
                    r = fft_lds<FFT_USER_RTISI_BWD>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
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

}  // namespace
