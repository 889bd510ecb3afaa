// lws_gla.hip -- the iterative phase reconstructions on the device, fused with their transforms: ONE translation unit (what the compiler
// derives for a kernel depends on what else the unit holds, see lws_fft.h), its kernels in headers by family, each with its own comment:
//   lws_gla_kernels.h        (Fast) Griffin-Lim and its backward pass: k_gla_*
//   lws_misi_kernels.h       MISI and its backward pass: k_misi_residual, k_misi_forward, k_misi_signals, k_misi_bwd_*
//   lws_rtisi_kernels.h      RTISI-LA in one shot, k_rtisi and k_rtisi_tape (the text of lws_rtisi_march.h, twice), and k_rtisi_bwd
//   lws_misi_la_kernels.h    online MISI in one shot: k_misi_la
//   lws_la_stream_kernels.h  the streaming forms: k_rtisi_stream, k_misi_la_stream
//   lws_fft.h                the transform they share, and the names of its instances (FFT_USER_*), one per kernel that needs its own
// This file is the host half: the context and what the one-shot calls share once their arguments are checked (GlaCall), the LDS opt-in
// table, the entry points, and the stream handle -- one struct for both kinds of stream, whose every decision is made by the step clock
// of lws_la_stream.h, plain C++ that the CPU tests drive without a device.
#include "../../include/lws_hip.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <mutex>
#include <vector>

#include "lws_common.h"
#include "lws_fft.h"
#include "lws_gla_kernels.h"
#include "lws_misi_kernels.h"
#include "lws_rtisi_kernels.h"
#include "lws_misi_la_kernels.h"
#include "lws_la_stream_kernels.h"

namespace {

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

// Every kernel of this unit that takes dynamic LDS, and how much it may ask for: the transform buffers, or (a look-ahead kernel with
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

// what the two placement queries hand back, each part where the caller asks for it
int report_placement(const LaPlacement &p, int *in_lds, int *threads, size_t *lds_bytes) {
    if (in_lds) *in_lds = p.in_lds ? 1 : 0;
    if (threads) *threads = p.threads;
    if (lds_bytes) *lds_bytes = p.lds_bytes;
    return LWS_OK;
}

}  // namespace

extern "C" int lws_rtisi_la_placement(int N, int fshift, int look_ahead, int K, int *in_lds, int *threads, size_t *lds_bytes) {
    if (N < 1 || fshift < 1 || look_ahead < 0 || K < 0)
        return lws::set_error(LWS_ERR_INVALID, "placement of N = %d, hop %d, look-ahead %d, %d sources", N, fshift, look_ahead, K);
    return report_placement(la_placement(N, fshift, look_ahead, K), in_lds, threads, lds_bytes);
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
    return report_placement(la_bwd_placement(N, fshift, look_ahead), in_lds, threads, lds_bytes);
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
