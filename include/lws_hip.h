/*
 * lws_hip.h -- C ABI of the MI355X-native LWS engine (liblws_hip.so).
 *
 * This is the drop-in boundary for the hot path of Jonathan-LeRoux/lws: everything the
 * reference's Python binding (python/lws.pyx) or its mex gateways (matlab/{batch,online,
 * nofuture}_lws.cpp) do between "I have a complex T x F spectrogram, weights and a threshold
 * schedule" and "here is the updated spectrogram".  Plain pointers and sizes only; no C++,
 * torch or HIP types appear in a signature (a stream is passed as void*).
 *
 * Each entry point names the reference interface it replaces.
 *
 * Conventions
 *   - spectrograms: B independent T x F complex matrices, row-major, bin fastest, frame next
 *     (numpy C order of a (B,T,F) array; identical memory to MATLAB's F x T column-major).
 *     F must be odd (non-negative frequencies of an even FFT) -- lws.pyx:223-224.
 *   - host entry points take/return complex128 (interleaved re,im doubles), exactly the dtype
 *     the reference returns (lws.pyx:212-213,256); device entry points work in place on
 *     complex64 (fp32 plans) or complex128 (fp64 plans) device memory.
 *   - weights: complex128 interleaved, C order [Qp][Q][L+1] as produced by create_weights
 *     (lws.pyx:160-181): Qp == Q ("summarised") or Qp == 2(F-1) ("general", the reference's
 *     fractionalQ kernels).  A weight participates iff |w| > 1e-12 (lws.pyx:231-232).
 *   - thresholds: `iters` doubles, NOT yet scaled; every spectrogram scales them by its own
 *     mean(|S|) as lws.pyx:240,245 / batch_lws.cpp:119-129 do.
 *   - every function returns LWS_OK (0) or an error code; lws_last_error() gives the text of the
 *     calling thread's most recent failure.  Nothing aborts, nothing throws.
 *   - a plan may be used from one thread at a time; distinct plans are independent.
 */
#ifndef LWS_HIP_H_
#define LWS_HIP_H_

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct lws_plan lws_plan; /* opaque */

enum {
    LWS_OK = 0,
    LWS_ERR_INVALID = 1,     /* bad shape / argument (the ValueErrors of lws.pyx) */
    LWS_ERR_HIP = 2,         /* a HIP runtime call failed */
    LWS_ERR_NOMEM = 3,
    LWS_ERR_UNSUPPORTED = 4  /* valid request this build cannot serve */
};

/* plan flags */
enum {
    LWS_PRECISION_FP32 = 0,        /* default: fp32 state, weights and accumulation */
    LWS_PRECISION_FP64 = 1,        /* fp64 everywhere (reference arithmetic): batch sweeps of Q = 2 / 4 plans (frames up to ~2090 bins) on the fp64 systolic engine (lws_sys64.hip), no-future and online sweeps of Q = 2 / 3 / 4 / 8 plans on LDS engines that are bit-identical to the order-exact generic engine (lws_nofuture.hip, lws_online64.hip), batch sweeps of the other plans with summarised tensors -- Q from 2 to 16, L up to 10, in practice the Q and shapes the fp64 systolic engine does not take -- on the band engine (lws_band.hip, round 6), online sweeps of the other plans (and of Q = 8 plans) on the team engine's order-exact kernel (lws_team.hip: the generic engine's bits, ~10x faster), the rest on that engine */
    LWS_NOFUTURE_Q4_COMPAT = 2,    /* reproduce NoFuture_LWSQ4's addressing (lwslib.cpp:559-594) when Q == Qp == 4 */
    LWS_FORCE_GENERIC = 4,         /* never use the specialised systolic batch kernel */
    LWS_NO_DIRECT_IO = 8,          /* always go through the extended buffers (prep / extract passes), even for a call
                                      that is one batch stage on device complex64 data -- for comparison */
    LWS_GENERIC_PLAIN_LAYOUT = 32, /* generic engine: batch sweeps in the reference's layout instead of the time-skewed copy
                                      (same results bit for bit; for comparison) */
    LWS_STORAGE_FP16 = 16          /* fp16-complex storage (BASELINE config 5): between passes over HBM the batch kernel keeps
                                      the spectrogram as half2 and the target magnitudes as half (10 B instead of 20 B per
                                      active bin and sweep), scaled per spectrogram by the power of two that brings its
                                      largest magnitude to [1, 2); arithmetic stays fp32.  The reference has no such mode
                                      (every pointer of lwslib.h:6-26 is double*): tolerance in DESIGN.md section 6.
                                      Applies to batch sweeps the systolic kernel serves; I/O stays complex64 / complex128 */
};

/* which of the plan's weight tensors a call uses (class lws passes W_ai to nofuture_lws, lws.pyx:475) */
enum { LWS_W = 0, LWS_W_AI = 1, LWS_W_AF = 2 };

int lws_hip_version(void);                 /* 10000*major + 100*minor + patch */
const char *lws_last_error(void);
int lws_device_count(void);                /* GPUs visible to this process, 0 if none */

/* Replaces the per-call weight preparation of lws.pyx:227-232, 280-285, 341-352 and
 * batch_lws.cpp:78-105: uploads the three weight tensors once.  W_ai / W_af may be NULL if the
 * online path is not used.  `device` is a HIP device ordinal. */
int lws_plan_create(lws_plan **plan, int device, int F, int L, int Q, int Qp,
                    const double *W, const double *W_ai, const double *W_af, unsigned flags);
void lws_plan_destroy(lws_plan *plan);

/* lws.batch_lws(S, W, thresholds)            (lws.pyx:209-258; mex batch_lws.cpp:20-154)
 * S_out may alias S_in.  iters == 0 copies the input (lws.pyx:219-220). */
int lws_batch_lws(lws_plan *plan, int wsel, const double *S_in, double *S_out, int B, int T,
                  const double *thresholds, int iters);

/* lws.nofuture_lws(S, W, thresholds)         (lws.pyx:261-311; mex nofuture_lws.cpp:20-157) */
int lws_nofuture_lws(lws_plan *plan, int wsel, const double *S_in, double *S_out, int B, int T,
                     const double *thresholds, int iters);

/* lws.online_lws(S, W, W_ai, W_af, thresholds, LA, fshift)
 *                                            (lws.pyx:314-375; mex online_lws.cpp:21-181;
 *                                             driver TF_RTISI_LA lwslib.cpp:1424-1492)
 * qdiv is the reference's Qfloat = N / fshift (only read when update == 1, which no shipped caller
 * uses; kept for interface fidelity). */
int lws_online_lws(lws_plan *plan, const double *S_in, double *S_out, int B, int T,
                   const double *thresholds, int iters, int LA, double qdiv);

/* lws.lws.run_lws(S) = nofuture -> online -> batch (lws.pyx:495-499) without leaving the device.
 * Between stages the edge-pad frames are refreshed from the current first/last frame exactly as
 * three separate calls would (each call re-runs extspec, lws.pyx:155-156,235). A stage with
 * zero iterations is skipped.  Thresholds are per stage. */
int lws_run_lws(lws_plan *plan, const double *S_in, double *S_out, int B, int T,
                const double *thr_nofuture, int it_nofuture,
                const double *thr_online, int it_online, int LA, double qdiv,
                const double *thr_batch, int it_batch);

/* Device-resident variants: `S_dev` is a device pointer to B*T*F complex64 (fp32 plan) or
 * complex128 (fp64 plan) values, updated in place; `stream` is a hipStream_t (or NULL).
 * Work is enqueued on `stream`; the call returns without synchronising unless noted. */
int lws_batch_lws_dev(lws_plan *plan, int wsel, void *S_dev, int B, int T,
                      const double *thresholds, int iters, void *stream);
int lws_nofuture_lws_dev(lws_plan *plan, int wsel, void *S_dev, int B, int T,
                         const double *thresholds, int iters, void *stream);
int lws_online_lws_dev(lws_plan *plan, void *S_dev, int B, int T,
                       const double *thresholds, int iters, int LA, double qdiv, void *stream);

/* lws.lws.run_lws on device-resident spectrograms (in place), the three stages enqueued back to back on `stream`. */
int lws_run_lws_dev(lws_plan *plan, void *S_dev, int B, int T,
                    const double *thr_nofuture, int it_nofuture,
                    const double *thr_online, int it_online, int LA, double qdiv,
                    const double *thr_batch, int it_batch, void *stream);

/* Host-only query (no device needed): does the weight tensor W[Qp][Q][L+1] (complex128 interleaved, as create_weights returns it,
 * lws.pyx:160-181) have the structure the fast kernels rely on -- W[p][r][k] == W[0][r][k] exp(2 pi j p r step / period) for every row
 * p?  Returns 1 and sets *period, *step (period 0: the tensor has no neighbour-frame weights and fits any twiddle), else 0.  For
 * create_weights' tensors period / step = frame / hop in lowest terms; plans whose tensors have it run on the systolic / LDS engines
 * when their shape is served, the others on the generic engine. */
int lws_weights_structure(const double *W, int Q, int Qp, int L, int *period, int *step);

/* Pre-size every scratch buffer of the plan for calls of up to B spectrograms of T frames and `max_iters` thresholds
 * per stage.  The *_dev entry points only enqueue work and return -- unless a scratch buffer has to grow, which is a
 * (synchronising) hipMalloc: reserve once and they never allocate.  The reference allocates per call (lws.pyx:227-240;
 * the mex gateways malloc and never free, batch_lws.cpp:81-118). */
int lws_plan_reserve(lws_plan *plan, int B, int T, int max_iters);

/* Consistency-residual proxy: for each spectrogram b
 *   out[2b]   = sum over bins of |acc + w00*S|^2   (acc = the LWS weighted sum of the bin without its centre tap,
 *                                                   w00 = W[bin % Qp][0][0], which holds create_weights' -1)
 *   out[2b+1] = sum over bins of |S|^2
 * in fp64, on the device buffer `S_dev` (complex64 for fp32 and fp16-storage plans, complex128 for fp64 plans; left unchanged).
 * out is a HOST array of 2*B doubles (synchronises).  Every plan computes it with W (never W_ai / W_af) on the generic accumulate.
 * Edge frames enter with the replicated neighbours of extspec (lws.pyx:146-157), as in a batch sweep.  On interior frames
 * 10 log10(out[2b+1] / out[2b]) agrees with the true inconsistency sum |stft(istft(S)) - S|^2 to about 0.2 dB, but the L-bin
 * truncation floors it near 40 dB at L = 5 (a consistent STFT reads ~40 dB, not ~300): it is not get_consistency. */
int lws_residual_dev(lws_plan *plan, const void *S_dev, int B, int T, double *out, void *stream);
/* The same for HOST spectrograms S[B][T][F] complex128. */
int lws_residual(lws_plan *plan, const double *S, int B, int T, double *out);

/* The JOB's residual pair for a caller that runs ONE PROCESS PER GPU (the layout bench.py uses; BASELINE.json north_star: "RCCL
 * over xGMI used only for the optional final consistency-residual reduction"): this rank's spectrograms are summed on the device
 *   local[0] = sum_b sum over bins |acc + w00*S|^2,   local[1] = sum_b sum over bins |S|^2      (fp64, fixed order)
 * and the pair is all-reduced (ncclSum over 2 doubles, in place on the device, on `stream`) over the ranks of `rccl_comm` -- an
 * ncclComm_t the caller created (ncclCommInitRank) for its ranks; NULL: no collective, out = this rank's sums.  out: 2 HOST doubles,
 * the same on every rank (synchronises).  RCCL is loaded at the first call (dlopen librccl.so.1): the library does not link
 * against it, and callers that never pass a communicator never need it (LWS_ERR_UNSUPPORTED if it cannot be loaded).  The reference
 * has no counterpart (single process, no residual); the single-process multi-GPU form is lws_multi_residual below. */
int lws_residual_allreduce_dev(lws_plan *plan, const void *S_dev, int B, int T, void *rccl_comm, double *out, void *stream);

/* Timing of the most recent *_dev / host call on this plan, measured with HIP events on the
 * stream the kernels ran on: total milliseconds spent in the update kernels and the number of
 * update-kernel launches (prep / extract kernels are not counted). */
int lws_last_kernel_time(lws_plan *plan, float *ms, int *launches);

/* Device-to-device stream copy of `bytes` (a multiple of 16) with the library's own kernel: the measured HBM copy
 * rate the roofline fraction is quoted beside (spec peak and measured copy peak). */
int lws_stream_copy(void *dst_dev, const void *src_dev, size_t bytes, void *stream);

/* Name of the update kernel the last call dispatched ("generic_fp32", "systolic_q4", ...). */
const char *lws_last_kernel_name(lws_plan *plan);

/* Which stage of this plan's calls ("batch", "no-future", "online") last ran on the order-exact generic engine -- 20-40x slower than
 * the kernels built for the common shapes -- or "" if none ever has.  (lws_last_kernel_name only names the LAST stage of a
 * run_lws pipeline.) */
const char *lws_generic_stage(lws_plan *plan);

/* ---- the steps either side of the path, on the device (lws.pyx:43-144; float32, any even frame size N in [32, 4096]
 *      -- an odd factor times a power of two: radix-2 stages and one stage of odd-point DFTs; fftsize == fsize unless said otherwise).  Windows are host arrays of N doubles, already normalised the way the caller
 *      wants them (class lws: awin and synthwin(awin, fshift)).  perfectrec as in lws.pyx:55-67,130-137. ---- */

/* Frames stft() produces for a signal of `len` samples (lws.pyx:55-76): never negative; 0 without perfectrec for a signal that is
 * shorter than one frame even when padded to the frame-shift grid (the host returns an empty spectrogram); -1 for len < 0,
 * N < 1 or fshift < 1. */
int lws_stft_frames(int len, int N, int fshift, int perfectrec);
/* Samples istft() returns for M frames (lws.pyx:121,130-137): never negative.  With perfectrec it is what the slice
 * signal[prepad : fshift - N] keeps of fshift (M - 1) + N samples -- nothing of fewer than about N / fshift frames, and nothing
 * of any number of frames with fshift == N (an end index of 0 is the start of the array). */
int lws_istft_length(int M, int N, int fshift, int perfectrec);
/* stft (lws.pyx:43-90) of B signals x_dev[B][len] (float32) into S_dev[B][M][N/2+1] (complex64), M = lws_stft_frames().
 * M == 0: LWS_OK, nothing is enqueued and neither pointer is used.  (The same holds for lws_stft_zp_dev.) */
int lws_stft_dev(int device, const float *x_dev, int B, int len, int N, int fshift, const double *awin,
                 int perfectrec, void *S_dev, void *stream);
/* istft (lws.pyx:93-137) of S_dev[B][M][N/2+1] (complex64) into x_dev[B][lws_istft_length()] (float32).  M < 1: LWS_ERR_INVALID;
 * lws_istft_length() == 0 (perfectrec cuts away all that so few frames cover): LWS_OK, nothing is enqueued and neither pointer
 * is used. */
int lws_istft_dev(int device, const void *S_dev, int B, int M, int N, int fshift, const double *swin,
                  int perfectrec, float *x_dev, void *stream);
/* stft with a transform longer than the frame (lws.pyx:49-50,85: np.fft.fft(frame, n = fftsize) of the fsize windowed samples,
 * zeros behind them): fsize even, fsize <= fftsize, fftsize an even size in [32, 4096]; frame count and padding follow fsize
 * (M = lws_stft_frames(len, fsize, ...)); awin has fsize entries; S_dev[B][M][fftsize/2+1].  (There is no inverse counterpart: the
 * reference's istft raises for every fftsize != 2 (bins - 1), lws.pyx:107-126; class lws pads its windows instead, 396-411.) */
int lws_stft_zp_dev(int device, const float *x_dev, int B, int len, int fsize, int fftsize, int fshift, const double *awin,
                    int perfectrec, void *S_dev, void *stream);
/* get_consistency (lws.pyx:140-144) per spectrogram: out[2b] = sum |S|^2, out[2b+1] = sum |stft(istft(S)) - S|^2
 * (fp64 sums of the fp32 transform); consistency in dB = 10 log10(out[2b] / out[2b+1]).  out: HOST, 2*B doubles
 * (synchronises).  Sums of several spectrograms / ranks add up to the batch consistency.  With perfectrec, an M the round trip
 * stft(istft(.)) does not keep -- lws_stft_frames(lws_istft_length(M, ...), ...) != M: too few frames -- is LWS_ERR_INVALID, before
 * anything is enqueued (the host's get_consistency fails to subtract spectrograms of two shapes there). */
int lws_consistency_dev(int device, const void *S_dev, int B, int M, int N, int fshift, const double *awin,
                        const double *swin, int perfectrec, double *out, void *stream);

/* (Fast) Griffin-Lim refinement, device resident (lws_gla.hip; the reference has no counterpart).  With the projection
 * P(c) = stft(istft(c)) -- the round trip of lws_consistency_dev, perfectrec included -- iteration i = 1..iters computes
 * X = P(c), t_i = A X / |X| (A + 0j where |X| == 0), and c = t_i for i = 1, c = t_i + alpha (t_i - t_{i-1}) after that; alpha = 0 is
 * plain Griffin-Lim.  C_dev[B][M][N/2+1] (complex64) holds c_0 on entry and t_iters -- whose magnitudes are A -- on return;
 * iters == 0 leaves it unchanged.  A_dev[B][M][N/2+1] (float32) are the target magnitudes, NULL: |c_0|.  trace: NULL (the call
 * only enqueues work on `stream`), or HOST, iters*B*2 doubles (synchronises): trace[(i-1)*B*2 + 2b] = sum |c_{i-1}|^2 and
 * [.. + 1] = sum |P(c_{i-1}) - c_{i-1}|^2, the pair of lws_consistency_dev for the iterate entering step i.  float32 transforms,
 * two frames per complex transform.  iters < 0, alpha outside [0, 1), or, with iters > 0 and perfectrec, an M the round trip does
 * not keep (too few frames for perfectrec, as lws_consistency_dev): LWS_ERR_INVALID, before anything is enqueued. */
int lws_griffin_lim_dev(int device, void *C_dev, const float *A_dev, int B, int M, int N, int fshift, const double *awin,
                        const double *swin, int perfectrec, int iters, double alpha, double *trace, void *stream);

/* Training through Griffin-Lim (a few unrolled Fast Griffin-Lim steps under a waveform or spectral loss, "deep Griffin-Lim"):
 * lws_griffin_lim_dev with a tape, and its backward pass.  lws_griffin_lim_tape_dev takes the arguments of lws_griffin_lim_dev
 * without the trace and with A_dev required, runs the same launches -- C_dev comes back with the bits of lws_griffin_lim_dev -- and
 * also writes the X of every step, before its projection, to tape_dev[iters][B][M][N/2+1] (complex64; required if iters > 0).
 * lws_griffin_lim_backward_dev: from the cotangent gC_dev[B][M][N/2+1] (complex64; NULL: zeros) of the returned C = t_iters, the
 * gradients of the loss with respect to the magnitudes, gA_out[B][M][N/2+1] (float32, required), and the start, gS_out[B][M][N/2+1]
 * (complex64; NULL: not stored, and the last launch is left out).  Complex gradients are g = dL/dRe + j dL/dIm (dL = Re sum
 * conj(g) dz).  A_dev, tape_dev and alpha are those of the forward call; alpha is a number, not a variable: it gets no gradient.
 * The update c_i = t_i + alpha_i (t_i - t_{i-1}) (alpha_1 = 0, alpha_i = alpha after that) is linear in the t's, so the momentum needs
 * no tape of its own: with gc_i the gradient on c_i and gc_iters = 0 (c_iters is never used), backward from i = iters to 1,
 * gt = gC for i = iters and (1 + alpha_i) gc_i - alpha_{i+1} gc_{i+1} otherwise; with u = X_i / |X_i| of the tape: gA += Re(conj(u) gt),
 * gX = j u (A / |X_i|) Im(conj(u) gt) (u = 1 and gX = 0 where |X_i| == 0); gv = N istft(gX / 2, Re gX at the bins 0 and N/2; window
 * awin); gc_{i-1} = (2/N) stft(gv; window swin) (1/N and no imaginary part at the bins 0 and N/2; the perfectrec cuts carry no
 * gradient); gS = gc_0.  iters == 0: gA = 0, gS = gC.  Two launches per iteration, as the forward; no atomics, every sum in a fixed
 * order: results repeat bit for bit.  The calls only enqueue work on `stream`.  Argument errors and status codes as
 * lws_griffin_lim_dev (alpha outside [0, 1) included); a null A_dev, gA_out or (iters > 0) tape_dev: LWS_ERR_INVALID, before anything
 * is enqueued. */
int lws_griffin_lim_tape_dev(int device, void *C_dev, const float *A_dev, int B, int M, int N, int fshift, const double *awin,
                             const double *swin, int perfectrec, int iters, double alpha, void *tape_dev, void *stream);
int lws_griffin_lim_backward_dev(int device, const void *gC_dev, const float *A_dev, const void *tape_dev, int B, int M, int N,
                                 int fshift, const double *awin, const double *swin, int perfectrec, int iters, double alpha,
                                 float *gA_out, void *gS_out, void *stream);

/* MISI (Multiple Input Spectrogram Inversion, Gunawan & Sen 2010), device resident (lws_gla.hip; the reference has no counterpart):
 * Griffin-Lim on the K sources of each of B mixtures, coupled through the known mixture y.  Iteration i = 1..iters computes
 * x_k = istft(c_k), e = y - sum_k x_k (k ascending), X_k = stft(x_k + e / K), c_k = A X_k / |X_k| (A + 0j where |X_k| == 0); no
 * momentum.  C_dev[B][K][M][N/2+1] (complex64) holds c_0 on entry and c_iters -- whose magnitudes are A -- on return; iters == 0
 * leaves it unchanged.  A_dev[B][K][M][N/2+1] (float32) are the target magnitudes, NULL: |c_0|.  y_dev[B][len] (float32), len =
 * lws_istft_length(M, ...), are the mixtures.  x_dev: NULL, or [B][K][len] (float32) for the signals of the returned spectrograms
 * with their own residual shared out, s_k = istft(c_k) + (y - sum_j istft(c_j)) / K, which sum to y (also with iters == 0).
 * trace: NULL (the call only enqueues work on `stream`), or HOST, iters*B*2 doubles (synchronises): trace[(i-1)*B*2 + 2b] =
 * sum y^2 and [.. + 1] = sum e^2 of the iterate entering step i (fp64 sums; 10 log10 of their ratio is the mixture consistency
 * in dB).  K < 1, iters < 0, a null C_dev / y_dev / window, or an M the round trip stft(istft(.)) does not keep (too few frames
 * for perfectrec): LWS_ERR_INVALID; frame sizes outside the device transform: as lws_griffin_lim_dev. */
int lws_misi_dev(int device, void *C_dev, const float *A_dev, const float *y_dev, int B, int K, int M, int N, int fshift,
                 const double *awin, const double *swin, int perfectrec, int iters, float *x_dev, double *trace, void *stream);

/* Training through MISI (unfolded MISI under a waveform loss, Wang, Le Roux & Hershey 2018): lws_misi_dev with a tape, and its
 * backward pass.  lws_misi_tape_dev takes the arguments of lws_misi_dev without the trace and with A_dev required, runs the same
 * launches -- C_dev and x_dev come back with the bits of lws_misi_dev -- and also writes the X_k of every step, before their
 * projection, to tape_dev[iters][B][K][M][N/2+1] (complex64; required if iters > 0).
 * lws_misi_backward_dev: from the cotangents gC_dev[B][K][M][N/2+1] (complex64) of the returned C and gx_dev[B][K][len] (float32) of
 * the signals -- either may be NULL: zeros -- the gradients of the loss with respect to the magnitudes, gA_out[B][K][M][N/2+1]
 * (float32, required), the start, gS_out[B][K][M][N/2+1] (complex64), and the mixtures, gy_out[B][len] (float32); gS_out and gy_out
 * may be NULL: not stored.  Complex gradients are g = dL/dRe + j dL/dIm (dL = Re sum conj(g) dz).  A_dev and tape_dev are those of the
 * forward call.  Backward from i = iters to 1, with u = X / |X| of the tape: gA += Re(conj(u) gc), gX = j u (A / |X|) Im(conj(u) gc)
 * (u = 1 and gX = 0 where |X| == 0); gv_k = N istft(gX / 2, Re gX at the bins 0 and N/2; window awin); m = mean_k gv_k (k ascending),
 * gy += m; gc_k = (2/N) stft(gv_k - m; window swin) (1/N and no imaginary part at the bins 0 and N/2); on entry
 * gc = gC + that of gx, and the gc left over is gS.  iters == 0: gA = 0, gS and gy from the entry alone.  Three launches per
 * iteration, no atomics, every sum in a fixed order: results repeat bit for bit.  The calls only enqueue work on `stream`.  Argument
 * errors and status codes as lws_misi_dev; a null A_dev, gA_out or (iters > 0) tape_dev: LWS_ERR_INVALID. */
int lws_misi_tape_dev(int device, void *C_dev, const float *A_dev, const float *y_dev, int B, int K, int M, int N, int fshift,
                      const double *awin, const double *swin, int perfectrec, int iters, float *x_dev, void *tape_dev, void *stream);
int lws_misi_backward_dev(int device, const void *gC_dev, const float *gx_dev, const float *A_dev, const void *tape_dev, int B, int K,
                          int M, int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters, float *gA_out,
                          void *gS_out, float *gy_out, void *stream);

/* RTISI-LA (Real-Time Iterative Spectrogram Inversion with Look-Ahead, Zhu, Beauregard & Wyse 2007), device resident (lws_gla.hip;
 * what the reference's online sweeps approximate): Griffin-Lim under a look-ahead, frame m of the result depending on no input
 * frame later than m + look_ahead.  With inv(c) = swin irfft(c) and fwd(y) = rfft(awin y) on the uncut timeline of hop (M - 1) + N
 * samples (with perfectrec the samples istft cuts read as zero), the frames m = 0 .. M-1 are committed in order: the frames up to
 * last = min(m + look_ahead, M - 1) enter as f_j = inv(c_j); `iters` times, y = done + sum_{j = m..last} f_j (j ascending),
 * c_j = A_j X_j / |X_j| with X_j = fwd(y at hop j) (A_j + 0j where |X_j| == 0) and f_j = inv(c_j) for all j = m..last from the same
 * y; then done += f_m.  C_dev[B][M][N/2+1] (complex64) holds the start on entry and the committed c_m -- whose magnitudes are A --
 * on return; iters == 0 leaves it unchanged.  A_dev[B][M][N/2+1] (float32): target magnitudes, NULL: |C| on entry.  x_dev: NULL,
 * or [B][lws_istft_length(M, N, fshift, perfectrec)] (float32) for the committed sum cut as istft cuts it, which is istft of the
 * result (also with iters == 0).  One workgroup per spectrogram and one launch; the call only enqueues work on `stream`.
 * iters < 0, look_ahead < 0, a null C_dev / window, or, with iters > 0 and perfectrec, an M the round trip does not keep:
 * LWS_ERR_INVALID, before anything is enqueued; frame sizes outside the device transform: as lws_griffin_lim_dev. */
int lws_rtisi_la_dev(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift,
                     const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, void *stream);

/* How a frame enters the look-ahead iterations (the *_ex entry points below; the ones without _ex pass LWS_START_GIVEN).
 *   LWS_START_GIVEN   : from the caller's start row, f_j = inv(c_j): C_dev / S_dev carry a phase.
 *   LWS_START_OVERLAP : RTISI-LA only -- RTISI's own initial estimate.  Frames enter one at a time, j ascending; frame j, entering in
 *                       commit step m, takes c_j = A_j X / |X| with X = fwd(keep (done + sum_{i = m..j-1} f_i) at hop j), the
 *                       transform of the partial overlap-add sum under it (A_j + 0j where |X| == 0: frame 0, a silent sum, and
 *                       every frame at fshift == N), then f_j = inv(c_j).
 *   LWS_START_MIXTURE : online MISI only -- the mixture phase.  Frame j of every source k takes c_kj = A_kj X / |X| with
 *                       X = fwd(keep y at hop j), one transform of the mixture under the frame for all K sources.
 * Under the last two only magnitudes are read: A_dev, or |C| / |S| where it is NULL, and the phases of the start are ignored; the
 * entry rows are a result of their own, so iters == 0 returns them (and their signals) instead of the start.  Nothing else
 * changes: the iterations, the commits, the open end of the streams, the placement lws_rtisi_la_placement reports.  A start the
 * function does not take: LWS_ERR_INVALID, nothing enqueued. */
enum {
    LWS_START_GIVEN = 0,
    LWS_START_OVERLAP = 1,
    LWS_START_MIXTURE = 2
};

/* lws_rtisi_la_dev with a start: LWS_START_GIVEN or LWS_START_OVERLAP.  Under LWS_START_OVERLAP C_dev is read for |C| only, and
 * only where A_dev is NULL; every row is written, also with iters == 0. */
int lws_rtisi_la_dev_ex(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift,
                        const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, int start, void *stream);

/* Training through RTISI-LA (a model that will run under the causal iteration at inference is trained through it): lws_rtisi_la_dev
 * with a tape, and its backward pass; LWS_START_GIVEN only.  lws_rtisi_la_tape_dev takes the arguments of lws_rtisi_la_dev with A_dev
 * required, runs the same iteration -- C_dev and x_dev come back with the bits of lws_rtisi_la_dev -- and also writes the argument X of
 * every projection to tape_dev[B][M][iters][LA + 1][N/2+1] (complex64; required if iters > 0), LA = min(look_ahead, M - 1): row
 * [b][m][it - 1][j - m] is frame j in inner iteration `it` of commit step m; rows of frames beyond last = min(m + LA, M - 1) are
 * neither written nor read.
 * lws_rtisi_la_backward_dev: from the cotangents gC_dev[B][M][N/2+1] (complex64) of the returned C and gx_dev[B][len] (float32, len =
 * lws_istft_length(M, ...)) of the signal -- either may be NULL: zeros -- the gradients of the loss with respect to the magnitudes,
 * gA_out[B][M][N/2+1] (float32, required), and the start, gS_out[B][M][N/2+1] (complex64; NULL: not stored).  Complex gradients are
 * g = dL/dRe + j dL/dIm.  A_dev, tape_dev, iters and look_ahead are those of the forward call.  With inv_adj(g) = (2/N) rfft(swin g)
 * (1/N and no imaginary part at the bins 0 and N/2), fwd_adj(gX) = N awin irfft(gX / 2, Re gX at the bins 0 and N/2), v[j] the samples
 * hop j .. hop j + N of a timeline vector v: gdone = keep gx placed on the uncut timeline, G = 0; for m = M-1 .. 0, for it = iters .. 1:
 * Gn = 0; for j = m .. last: gf = gdone[m] if (it == iters and j == m) else G[j], gc = inv_adj(gf) (+ gC_m for that same pair), u = X /
 * |X| of the tape, gA_j += Re(conj(u) gc), gX = j u (A_j / |X|) Im(conj(u) gc) (u = 1, gX = 0 where |X| == 0), Gn[j] += fwd_adj(gX);
 * then Gn *= keep, gdone += Gn, G = Gn; after the iterations gS_j = inv_adj(G[j]) for the frames that entered in step m.  iters == 0:
 * gA = 0, gS_m = gC_m + inv_adj(gdone[m]).  One launch, one workgroup per spectrogram; no atomics, every sum in a fixed order: results
 * repeat bit for bit.  The calls only enqueue work on `stream`.  Argument errors and status codes as lws_rtisi_la_dev; a null A_dev,
 * gA_out or (iters > 0) tape_dev: LWS_ERR_INVALID, before anything is enqueued.
 * lws_rtisi_la_bwd_placement: where the backward kernel keeps its state (3 (N + look_ahead fshift) floats) for a look-ahead already
 * clamped to M - 1, as lws_rtisi_la_placement reports it for the forward kernels. */
int lws_rtisi_la_tape_dev(int device, void *C_dev, const float *A_dev, float *x_dev, int B, int M, int N, int fshift,
                          const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, void *tape_dev,
                          void *stream);
int lws_rtisi_la_backward_dev(int device, const void *gC_dev, const float *gx_dev, const float *A_dev, const void *tape_dev, int B, int M,
                              int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters, int look_ahead,
                              float *gA_out, void *gS_out, void *stream);
int lws_rtisi_la_bwd_placement(int N, int fshift, int look_ahead, int *in_lds, int *threads, size_t *lds_bytes);

/* Streaming RTISI-LA (lws_gla.hip): lws_rtisi_la_dev for frames that arrive over time, B streams side by side, the state of the
 * iteration (the overlap-add ring, the windowed inverse frames and the magnitudes of the look_ahead frames still active; per stream)
 * in device memory owned by the handle.  The rows all calls return, one after another, are what one call with every pushed row
 * would return under an open end: as lws_rtisi_la_dev, except that with perfectrec the samples behind fshift M read as zero only
 * in the returned signal, not inside the iteration -- lws_amd.rtisi_la(..., open_end=True) is the fp64 definition.  A stream has
 * no length limit.
 *   create : windows as lws_rtisi_la_dev takes them (the handle keeps its own device copy); synchronises once.
 *   push   : S_dev[B][frames][N/2+1] (complex64) the next `frames` rows of every stream, A_dev[B][frames][N/2+1] (float32) their
 *            target magnitudes or NULL (|S|).  Commits every frame m with m + look_ahead pushed: *frames_out = max(0, pushed -
 *            look_ahead) - committed rows, written to C_out_dev[B][frames][N/2+1] (rows beyond *frames_out of each stream are left
 *            alone), and -- x_out_dev not NULL -- the fshift samples each commit finalises, less what perfectrec cuts at the start, to
 *            x_out_dev[B][frames fshift], *samples_out of each stream.  Both counts come from the host's counters; the call only
 *            enqueues work on `stream` and keeps no reference to the caller's buffers.  frames == 0 does nothing.
 *   finish : commits the rest, C_out_dev[B][look_ahead][N/2+1] and x_out_dev[B][N + look_ahead fshift]; with fewer than look_ahead + 1
 *            rows pushed, as one call on them would (look_ahead clamped); with none, 0 and 0.  The stream takes no rows after it.
 * Calls on one handle are ordered by `stream`, or by an event of the handle's if `stream` changes between calls.  A null handle,
 * frames < 0, a null S_dev with frames > 0, a null C_out_dev with rows to return, a push or finish after finish: LWS_ERR_INVALID,
 * nothing enqueued.  create: B < 1, iters < 0, look_ahead < 0, null window: LWS_ERR_INVALID; frame sizes: as lws_griffin_lim_dev. */
typedef struct lws_rtisi_stream lws_rtisi_stream;
int lws_rtisi_stream_create(int device, int B, int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters,
                            int look_ahead, lws_rtisi_stream **out);
/* ... with a start, LWS_START_GIVEN or LWS_START_OVERLAP, for the life of the stream: the stream then computes
 * lws_amd.rtisi_la(..., start='overlap', open_end=True).  Under LWS_START_OVERLAP push takes magnitudes alone: S_dev may be NULL
 * where A_dev is given (and is read for |S| only where it is not); with iters == 0 the rows returned are the entry estimates.  push,
 * finish and destroy are the same functions. */
int lws_rtisi_stream_create_ex(int device, int B, int N, int fshift, const double *awin, const double *swin, int perfectrec, int iters,
                               int look_ahead, int start, lws_rtisi_stream **out);
int lws_rtisi_stream_push(lws_rtisi_stream *h, const void *S_dev, const float *A_dev, int frames, void *C_out_dev, float *x_out_dev,
                          int *frames_out, int *samples_out, void *stream);
int lws_rtisi_stream_finish(lws_rtisi_stream *h, void *C_out_dev, float *x_out_dev, int *frames_out, int *samples_out, void *stream);
void lws_rtisi_stream_destroy(lws_rtisi_stream *h);

/* Online MISI, device resident (lws_gla.hip): MISI under a look-ahead, for the K sources of each of B mixtures -- lws_misi_dev as
 * lws_rtisi_la_dev is lws_griffin_lim_dev.  Frame m of every source depends on no input frame later than m + look_ahead and on no
 * mixture sample behind the end of that frame.  On the timeline and with inv, fwd and the cuts of lws_rtisi_la_dev, the mixture y
 * sitting where istft would put it, w = awin swin, and g_l = (sum_{j <= l} w) / (sum_j w) over the frames j that cover a sample
 * (ascending; 1 where the denominator is 0), the frames m = 0 .. M-1 are committed in order: the frames up to
 * last = min(m + look_ahead, M - 1) enter as f_kj = inv(c_kj); `iters` times, y_k = done_k + sum_{j = m..last} f_kj (j ascending),
 * e = g_last y - sum_k y_k (k ascending), c_kj = A_kj X / |X| with X = fwd(y_k + e / K at hop j) (A_kj + 0j where |X| == 0) and
 * f_kj = inv(c_kj) for all k and all j = m..last from the same iterate; then done_k += f_km.  C_dev[B][K][M][N/2+1] (complex64) holds
 * the starts on entry and the committed c_km -- whose magnitudes are A -- on return; iters == 0 leaves it unchanged.
 * A_dev[B][K][M][N/2+1] (float32): target magnitudes, NULL: |C| on entry.  y_dev[B][len] (float32), len = lws_istft_length(M, ...):
 * the mixtures.  x_dev: NULL, or [B][K][len] (float32) for s_k = done_k + (y - sum_j done_j) / K cut as istft cuts it, which sum
 * to y (also with iters == 0).  look_ahead is clamped to M - 1.  One workgroup per mixture and one launch; the call only enqueues
 * work on `stream`.  K < 1, iters < 0, look_ahead < 0, a null C_dev / y_dev / window, frames that leave no samples, or, with
 * iters > 0 and perfectrec, an M the round trip does not keep: LWS_ERR_INVALID, before anything is enqueued; frame sizes outside
 * the device transform: as lws_griffin_lim_dev. */
int lws_misi_la_dev(int device, void *C_dev, const float *A_dev, const float *y_dev, float *x_dev, int B, int K, int M, int N,
                    int fshift, const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, void *stream);
/* ... with a start: LWS_START_GIVEN or LWS_START_MIXTURE (above).  Under LWS_START_MIXTURE C_dev is read for |C| only, and only where
 * A_dev is NULL; every row is written, also with iters == 0. */
int lws_misi_la_dev_ex(int device, void *C_dev, const float *A_dev, const float *y_dev, float *x_dev, int B, int K, int M, int N,
                       int fshift, const double *awin, const double *swin, int perfectrec, int iters, int look_ahead, int start,
                       void *stream);

/* Streaming online MISI (lws_gla.hip): lws_misi_la_dev for frames and mixture that arrive over time, B mixtures of K sources side by
 * side, the state of the iteration (per source the overlap-add ring, the windowed inverse frames and the magnitudes of the look_ahead
 * frames still active; per mixture the samples under those frames) in device memory owned by the handle.  The rows all calls return,
 * one after another, are what one call with everything pushed would return under an open end -- lws_amd.misi_la(..., open_end=True)
 * is the fp64 definition: as lws_misi_la_dev, except that with perfectrec the samples behind fshift M read as zero only in the
 * returned signals, not inside the iteration, and that in the steps push runs the denominator of g sums w over every frame j >= 0
 * that would cover a sample, as if the stream never ended (finish, which knows M, sums over 0 .. M-1: g = 1 there).  A stream has no
 * length limit.
 *   count  : after M frames the stream holds need(M) = fshift (M - 1) + N - lo mixture samples (need(0) = 0), every sample under
 *            those frames; lo is the lead-in perfectrec cuts (N - fshift, or N - N % fshift if that is not 0), else 0.  A push of
 *            `frames` rows must bring exactly samples = need(M + frames) - need(M): the first N - fshift more than frames fshift, and
 *            with perfectrec the stream ends N - fshift samples behind what istft returns -- the zeros stft pads with, or the real
 *            continuation.  Any other count: LWS_ERR_INVALID, the handle left as it was.
 *   create : windows as lws_misi_la_dev takes them (the handle keeps its own device copy); synchronises once.
 *   push   : S_dev[B][K][frames][N/2+1] (complex64) the next rows of every source, A_dev (float32, same layout) their target
 *            magnitudes or NULL (|S|), y_dev[B][samples] (float32) the next mixture samples.  Commits every frame m with
 *            m + look_ahead pushed: *frames_out = max(0, pushed - look_ahead) - committed rows of every source, written to
 *            C_out_dev[B][K][frames][N/2+1] -- the row stride is the chunk's `frames`, the first *frames_out rows of each source are
 *            valid, the rest left alone -- and, x_out_dev not NULL, the fshift samples each commit finalises, less what perfectrec
 *            cuts at the start, s_k = done_k + (y - sum_j done_j) / K, to x_out_dev[B][K][frames fshift], *samples_out of each
 *            source.  Both counts come from the host's counters; the call only enqueues work on `stream` and keeps no reference to
 *            the caller's buffers.  frames == 0 (with samples == 0) does nothing.  At most (2^31 - N) / fshift - look_ahead - 2
 *            frames per push (LWS_ERR_UNSUPPORTED beyond).
 *   finish : commits the rest with last = min(m + look_ahead, M - 1), C_out_dev[B][K][look_ahead][N/2+1] and
 *            x_out_dev[B][K][N + look_ahead fshift]; with fewer than look_ahead + 1 rows pushed, with look_ahead clamped to M - 1 as
 *            one call on them would; with none, 0 and 0.  The stream takes no rows after it.
 * Placement and workgroup are what lws_rtisi_la_placement(N, fshift, look_ahead, K >= 1, ...) says, for the stream's look_ahead.
 * Calls on one handle are ordered by `stream`, or by an event of the handle's if `stream` changes between calls.  A null handle,
 * frames < 0, a null S_dev / y_dev with frames > 0, a null C_out_dev with rows to return, a push or finish after finish:
 * LWS_ERR_INVALID, nothing enqueued.  create: B < 1, K < 1, iters < 0, look_ahead < 0, null window: LWS_ERR_INVALID; frame sizes: as
 * lws_griffin_lim_dev. */
typedef struct lws_misi_stream lws_misi_stream;
int lws_misi_stream_create(int device, int B, int K, int N, int fshift, const double *awin, const double *swin, int perfectrec,
                           int iters, int look_ahead, lws_misi_stream **out);
/* ... with a start, LWS_START_GIVEN or LWS_START_MIXTURE, for the life of the stream: the stream then computes
 * lws_amd.misi_la(..., start='mixture', open_end=True); it holds every mixture sample under a pushed frame, so nothing more is
 * passed.  Under LWS_START_MIXTURE push takes magnitudes alone: S_dev may be NULL where A_dev is given (and is read for |S| only
 * where it is not); with iters == 0 the rows returned are the entry estimates.  push, finish and destroy are the same functions. */
int lws_misi_stream_create_ex(int device, int B, int K, int N, int fshift, const double *awin, const double *swin, int perfectrec,
                              int iters, int look_ahead, int start, lws_misi_stream **out);
int lws_misi_stream_push(lws_misi_stream *h, const void *S_dev, const float *A_dev, const float *y_dev, int frames, int samples,
                         void *C_out_dev, float *x_out_dev, int *frames_out, int *samples_out, void *stream);
int lws_misi_stream_finish(lws_misi_stream *h, void *C_out_dev, float *x_out_dev, int *frames_out, int *samples_out, void *stream);
void lws_misi_stream_destroy(lws_misi_stream *h);

/* Where the look-ahead kernels keep their state, and with how many threads they run: what lws_rtisi_la_dev and its stream (K == 0) or
 * lws_misi_la_dev and its stream (K >= 1 sources) decide for frames of N samples at hop fshift under a look-ahead of look_ahead frames (the clamped
 * one: min(look_ahead, M - 1) of a call).  *in_lds: 1 if ring and frame buffers sit in LDS behind the transform buffers, 0 if in
 * device scratch; *threads: the workgroup; *lds_bytes: the dynamic LDS the launch asks for.  Any of the three may be NULL.  Host
 * only: no device call, no check of N against the device transform.  N < 1, fshift < 1, look_ahead < 0 or K < 0: LWS_ERR_INVALID. */
int lws_rtisi_la_placement(int N, int fshift, int look_ahead, int K, int *in_lds, int *threads, size_t *lds_bytes);

/* ---- host-side construction of windows, weights and schedules (lws.pyx:10-40,160-206), fp64, no device work: what a
 *      caller without numpy needs to build a plan.  Complex outputs are interleaved (re, im) doubles. ---- */

/* hann (lws.pyx:10-19): out[n]. */
int lws_hann(int n, int symmetric, int use_offset, double *out);
/* synthwin (lws.pyx:22-40): synthesis window normalised for perfect reconstruction; swin may be NULL (= awin). */
int lws_synthwin(const double *awin, int fsize, int fshift, const double *swin, double *out);
/* shape of create_weights' result: Q = ceil(fsize/fshift), Qprime = Q (summarised, shift divides the window) or fsize. */
int lws_weights_shape(int fsize, int fshift, int use_summarized_weights, int *Qprime, int *Q);
/* create_weights (lws.pyx:160-181): W[Qprime][Q][L+1] complex128. */
int lws_create_weights(const double *awin, const double *swin, int fsize, int fshift, int L, int use_summarized_weights,
                       double *W);
/* build_asymmetric_windows (lws.pyx:184-200) from the product awin*swin: win_ai[fsize], win_af[fsize]. */
int lws_build_asymmetric_windows(const double *awin_swin, int fsize, int fshift, double *win_ai, double *win_af);
/* get_thresholds (lws.pyx:203-206): out[i] = alpha * exp(-beta * i^gamma). */
int lws_get_thresholds(int iterations, double alpha, double beta, double gamma, double *out);
/* What `lws.lws(awin_or_fsize, fshift, L=..., swin=...)` sets up (lws.pyx:384-431): awin == NULL means the default
 * sqrt-Hann window of `fsize` samples; swin may be NULL; the three weight tensors W, W_ai, W_af are built and the plan
 * created.  awin_out / swin_out (may be NULL) receive the windows actually used, fsize doubles each. */
int lws_plan_create_from_windows(lws_plan **plan, int device, const double *awin, const double *swin, int fsize,
                                 int fshift, int L, int symmetric_win, unsigned flags, double *awin_out, double *swin_out);

/* ---- one node, several GPUs, no torch: independent spectrograms are dealt in contiguous blocks to one plan per device,
 *      each driven by its own host thread and stream; no exchange between devices during the sweeps.
 *      `devices`: ndev HIP ordinals, or NULL for devices 0..ndev-1; ndev <= 0 means every visible device.  A device may
 *      be listed more than once (several shards on one GPU).  What a mex gateway or a C++ caller uses where the Python
 *      layer uses one process per GPU (bench.py). ---- */
typedef struct lws_multi_plan lws_multi_plan; /* opaque */
int lws_multi_plan_create(lws_multi_plan **mp, int ndev, const int *devices, int F, int L, int Q, int Qp,
                          const double *W, const double *W_ai, const double *W_af, unsigned flags);
void lws_multi_plan_destroy(lws_multi_plan *mp);
int lws_multi_plan_shards(const lws_multi_plan *mp);
/* lws_batch_lws / lws_run_lws over all shards; S_out may alias S_in; same results as one plan on one device. */
int lws_multi_batch_lws(lws_multi_plan *mp, int wsel, const double *S_in, double *S_out, int B, int T,
                        const double *thresholds, int iters);
int lws_multi_run_lws(lws_multi_plan *mp, const double *S_in, double *S_out, int B, int T,
                      const double *thr_nofuture, int it_nofuture,
                      const double *thr_online, int it_online, int LA, double qdiv,
                      const double *thr_batch, int it_batch);
/* The job's consistency-residual pair (see lws_residual_dev) of HOST spectrograms S[B][T][F] complex128, summed over all
 * shards on the host: out[0] = sum |acc + w00 S|^2, out[1] = sum |S|^2. */
int lws_multi_residual(lws_multi_plan *mp, const double *S, int B, int T, double *out);

#ifdef __cplusplus
}
#endif
#endif
