// lws_fft.h -- the LDS-resident transform and the host helpers around it, shared by the translation units that transform
// frames on the device (lws_stft.hip, lws_gla.hip).  Everything here has internal linkage: each unit gets its own copy.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/lws_hip.h"
#include "lws_common.h"
#include "lws_la_stream.h"   // Factors, factor, prepad: plain C++, shared with the CPU tests

namespace {

constexpr int MAXN = 4096, MINN = 32, FFT_THREADS = 256;   // two N-point complex buffers (three if N is not a power of two): <= 96 KB of LDS

#define STFT_TRY(expr)                                                                                              \
    do {                                                                                                            \
        hipError_t e_ = (expr);                                                                                     \
        if (e_ != hipSuccess)                                                                                       \
            return lws::set_error(LWS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// Complex DFT of n = m 2^a points held in LDS (x: data, y: scratch of the same size, followed -- if m > 1 -- by n entries for
// the twiddle table), by all threads of the block; natural order in and out.  sign = -1 forward, +1 inverse (unnormalised).
// Returns the buffer that holds the result.  USER: a caller that passes other buffers than the start of the dynamic LDS (k_rtisi)
// takes an instance of its own, so that what the compiler derives from the other callers' arguments (all alike) stays derived; with
// one shared instance a scalar shift moves by two slots in each of them.  Nothing computed depends on that: it only keeps their
// instruction streams what they were.  tools/compare_kernel_isa.py checks it, kernel by kernel, against another build's assembly.
// The instances and their owners (plain ints, not an enum: the value is all a mangled name may see of them).  A kernel added to
// lws_gla.hip that passes other arguments than a present owner does takes the next number.
constexpr int FFT_USER_SHARED = 0;                  // lws_stft.hip; k_gla_inverse, k_gla_forward without a tape, k_misi_forward
constexpr int FFT_USER_RTISI = 1;                   // k_rtisi under LWS_START_GIVEN
constexpr int FFT_USER_MISI_LA = 2;                 // k_misi_la, the passes
constexpr int FFT_USER_RTISI_STREAM = 3;            // k_rtisi_stream under LWS_START_GIVEN
constexpr int FFT_USER_MISI_LA_STREAM = 4;          // k_misi_la_stream, the passes
constexpr int FFT_USER_RTISI_OVERLAP = 5;           // k_rtisi under LWS_START_OVERLAP
constexpr int FFT_USER_RTISI_STREAM_OVERLAP = 6;    // k_rtisi_stream under LWS_START_OVERLAP
constexpr int FFT_USER_MISI_LA_ENTRY = 7;           // k_misi_la, the entry block of LWS_START_MIXTURE
constexpr int FFT_USER_MISI_LA_STREAM_ENTRY = 8;    // k_misi_la_stream, the same block
constexpr int FFT_USER_MISI_BWD = 9;                // k_misi_bwd_project, k_misi_bwd_frames
constexpr int FFT_USER_GLA_TAPE = 10;               // k_gla_forward with a tape
constexpr int FFT_USER_GLA_BWD = 11;                // k_gla_bwd_project, k_gla_bwd_frames
constexpr int FFT_USER_RTISI_TAPE = 12;             // k_rtisi_tape
constexpr int FFT_USER_RTISI_BWD = 13;              // k_rtisi_bwd
template <int USER = FFT_USER_SHARED> __device__ float2 *fft_lds(float2 *x, float2 *y, int n, int m, int a, float sign) {
    const int tid = threadIdx.x, nthr = blockDim.x;
    const int n2 = n / m;                                // 2^a
    float2 *tw = y + n;
    if (m > 1) {
        // exp(sign 2 pi j i / n), and the m interleaved subsequences side by side: y[r n2 + j] = x[m j + r].  The angle is reduced in
        // integers to the nearest quarter turn, 4 i = q n + rem with |rem| <= n / 2, so that the rounded quotient is at most 1/4:
        // 2 i / n rounded as it stands is off by up to 2^-24 of a half turn near i = n, six times the rounding of the twiddle itself,
        // and the m terms of an output bin see those errors coherently (an impulse's flat spectrum most of all)
        for (int i = tid; i < n; i += nthr) {
            const int q = (4 * i + (n >> 1)) / n, rem = 4 * i - q * n;
            float sn, cs;
            sincospif((float)rem / (float)(2 * n), &sn, &cs);
            const float c = (q & 1) ? ((q & 2) ? sn : -sn) : ((q & 2) ? -cs : cs);
            const float s = (q & 1) ? ((q & 2) ? -cs : cs) : ((q & 2) ? -sn : sn);
            tw[i] = make_float2(c, sign * s);
            const int j = i / m, r = i - j * m;
            y[r * n2 + j] = x[i];
        }
        __syncthreads();
        float2 *t = x; x = y; y = t;
    }
    // radix-2 Stockham (auto-sort, decimation in frequency) of the m blocks of n2 points, all blocks in every stage
    int ncur = n2, s = 1;
    for (int st = 0; st < a; ++st) {
        const int h = ncur >> 1;
        for (int i0 = tid; i0 < n / 2; i0 += nthr) {
            const int blk = i0 / (n2 / 2), i = i0 - blk * (n2 / 2);
            const int p = i / s, q = i - p * s;          // s is a power of two: shifts
            float sn, cs;
            sincospif(sign * 2.0f * (float)p / (float)ncur, &sn, &cs);
            const float2 *xb = x + blk * n2;
            float2 *yb = y + blk * n2;
            const float2 u = xb[q + s * p], v = xb[q + s * (p + h)];
            const float2 d = make_float2(u.x - v.x, u.y - v.y);
            yb[q + s * (2 * p)] = make_float2(u.x + v.x, u.y + v.y);
            yb[q + s * (2 * p + 1)] = make_float2(d.x * cs - d.y * sn, d.x * sn + d.y * cs);
        }
        __syncthreads();
        float2 *t = x; x = y; y = t;
        ncur = h;
        s <<= 1;
    }
    if (m == 1) return x;
    // X[k + n2 q] = sum_r exp(sign 2 pi j r (k + n2 q) / n) Y_r[k]
    for (int o = tid; o < n; o += nthr) {
        const int k = o % n2;
        float ar = 0.f, ai = 0.f;
        int idx = 0;                                     // (r o) mod n
        for (int r = 0; r < m; ++r) {
            const float2 v = x[r * n2 + k], w = tw[idx];
            ar += v.x * w.x - v.y * w.y;
            ai += v.x * w.y + v.y * w.x;
            idx += o;
            if (idx >= n) idx -= n;
        }
        y[o] = make_float2(ar, ai);
    }
    __syncthreads();
    return y;
}

struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
    int ensure(size_t bytes) {
        if (bytes <= cap) return LWS_OK;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return lws::set_error(LWS_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
        cap = bytes;
        return LWS_OK;
    }
};

size_t fft_lds_bytes(int N) { return (size_t)(factor(N).odd > 1 ? 3 : 2) * N * sizeof(float2); }

constexpr int MAX_DEVICES = 64;
int check_shape(int device, int B, int M, int N, int hop, int min_frames = 1) {
    if (device < 0 || device >= MAX_DEVICES) return lws::set_error(LWS_ERR_INVALID, "device index %d out of range", device);
    if (B < 0 || M < min_frames) return lws::set_error(LWS_ERR_INVALID, "empty batch or no frames");
    if (N < MINN || N > MAXN || (N & 1)) return lws::set_error(LWS_ERR_UNSUPPORTED, "frame size %d: the device transform serves even sizes in [%d, %d]", N, MINN, MAXN);
    if (hop < 1 || hop > N) return lws::set_error(LWS_ERR_INVALID, "frame shift %d", hop);
    return LWS_OK;
}

// stft(istft(.)) of M frames must give M frames again for the round trip to be a projection: with perfectrec the cuts of
// lws.pyx:130-137 leave too little of fewer than about N / hop frames (and nothing at all of hop == N)
int check_round_trip(int M, int N, int hop, int perfectrec) {
    if (perfectrec && lws_stft_frames(lws_istft_length(M, N, hop, perfectrec), N, hop, perfectrec) != M)
        return lws::set_error(LWS_ERR_INVALID, "the round trip does not keep %d frames (too few frames for perfectrec)", M);
    return LWS_OK;
}

}  // namespace
