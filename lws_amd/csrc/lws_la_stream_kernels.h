// lws_la_stream_kernels.h -- the two stream kernels, k_rtisi_stream and k_misi_la_stream, with the rows and samples a stream's handle
// holds for them (RtisiHeld, MisiStreamHeld); part of the one translation unit lws_gla.hip (whose header comment is the map of these
// files).  Their other arguments are the plain C++ of lws_la_stream.h, which the step clock fills.
#pragma once

#include "lws_la_stream.h"          // RtisiStreamArgs, MisiStreamArgs
#include "lws_misi_la_kernels.h"    // rtisi_phasor, RTISI_BINS; the rtisi_* helpers through it

namespace {

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
                    r = fft_lds<START == LWS_START_GIVEN ? FFT_USER_RTISI_STREAM : FFT_USER_RTISI_STREAM_OVERLAP>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
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
                    r = fft_lds<FFT_USER_MISI_LA_STREAM_ENTRY>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
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
                        r = fft_lds<FFT_USER_MISI_LA_STREAM>(x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
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

}  // namespace
