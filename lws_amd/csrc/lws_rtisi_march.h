// lws_rtisi_march.h -- the text of k_rtisi (lws_rtisi_kernels.h, where its comment is), included there once per value of the compile-time flag
// RTISI_TAPE: 0 gives k_rtisi, the kernel and arguments it always was; 1 gives k_rtisi_tape, which also stores the argument X of every
// projection to tape[b][m][it-1][j-m][k], of extent (B, M, iters, LA + 1, F), for the backward pass (rows beyond `last` are never
// written; used under LWS_START_GIVEN only).  A flag of the preprocessor and not of the template: any template parameter or argument
// more renames the untaped kernels, and a shared device function inlined into both changes their register allocation -- they are to
// keep the instruction streams they had (tools/compare_kernel_isa.py); for the same reason each has a transform instance of its own
// (the FFT_USER_* of lws_fft.h).  No include guard: RTISI_KERNEL, RTISI_TAPE and RTISI_TAPE_ARG are set by the includer.
template <bool IN_LDS, int START>
__global__ void __launch_bounds__(RTISI_MAX_THREADS) RTISI_KERNEL(float2 *C, const float *A, float *xout, const float *awin, const float *swin,
                                                        float *scratch, RtisiArgs a RTISI_TAPE_ARG) {
    extern __shared__ float2 lds[];
    const int b = blockIdx.x, N = a.N, F = N / 2 + 1, hop = a.hop, M = a.M, W = a.LA + 1, R = N + a.LA * hop;
    const int t_end = hop * (M - 1) + N - a.zero_hi;
    float2 *bufA = lds, *bufB = lds + N, *bufC = lds + 2 * N;   // bufC: the twiddle table's place, N not a power of two only
    float *state = IN_LDS ? reinterpret_cast<float *>(lds + (a.odd > 1 ? 3 : 2) * N) : scratch + (size_t)b * a.state_floats;
    float *ring = state, *fcur = state + R, *fnxt = fcur + (size_t)W * N;
    float2 *Cb = C + (size_t)b * M * F;
    const float *Ab = A ? A + (size_t)b * M * F : nullptr;   // null without iterations under GIVEN, and not read then
    float *xb = xout ? xout + (size_t)b * a.len : nullptr;
    for (int i = threadIdx.x; i < R; i += blockDim.x) ring[i] = 0.f;
    __syncthreads();
    int base = 0, slot_m = 0;   // slot_m: the slot of frame m
    for (int m = 0; m < M; ++m) {
        const int last = m + a.LA < M - 1 ? m + a.LA : M - 1;
        // pass 0: the frames that have not entered, f_j = inv(S_j) or inv of the entry estimate (LA + 1 frames at m = 0, one per step
        // after that), into fcur; passes 1 .. iters: the active frames, from fcur into fnxt
        for (int it = 0; it <= a.iters; ++it) {
            float *dst = it == 0 ? fcur : fnxt;
            const bool entry = START == LWS_START_OVERLAP && it == 0;   // frames enter one by one, through the projection
            // pass 0 starts at frame 0 (slot 0) in the first step and at frame m + LA after that: the slot before slot_m, cyclically
            const int j0 = it > 0 ? m : m == 0 ? 0 : m + a.LA;
            int slot = it > 0 || m == 0 ? slot_m : slot_m == 0 ? a.LA : slot_m - 1;   // of frame j: j mod (LA + 1), counted, not divided
            for (int j = j0; j <= last; j += entry ? 1 : 2) {
                const bool two = !entry && j + 1 <= last;
                const int upto = entry ? j - 1 : last;   // the frames in the sum the forward load gathers
                // one transform call for both directions (ph 0: forward, not in pass 0; ph 1: inverse): its uniform state once
                float2 *r = bufB;
#pragma nounroll
                for (int ph = it == 0 && !entry ? 1 : 0; ph < 2; ++ph) {
                    float2 *x = bufA, *y = bufB;
                    if (ph == 0) {
                        for (int n = threadIdx.x; n < N; n += blockDim.x) {
                            const float w = awin[n];
                            const float re = rtisi_sample(ring, fcur, j * hop + n, m, upto, slot_m, base, R, t_end, a) * w;
                            const float im = two ? rtisi_sample(ring, fcur, (j + 1) * hop + n, m, upto, slot_m, base, R, t_end, a) * w : 0.f;
                            x[n] = make_float2(re, im);
                        }
                    } else if (it == 0 && !entry) {
                        const float2 *r0 = Cb + (size_t)j * F, *r1 = r0 + F;
                        for (int k = threadIdx.x; k < F; k += blockDim.x)
                            rtisi_put_pair(x, k, N, r0[k], two ? r1[k] : make_float2(0.f, 0.f));
                    } else {
                        // the projected pair goes where the forward result is not, and where the inverse transform finds room for
                        // its table behind its second buffer: result in bufB -> (bufA, bufB, table bufC); in bufA -> (bufC, bufA,
                        // table bufB)
                        x = r == bufB ? bufA : (a.odd > 1 ? bufC : bufB);
                        y = r;
                        // an entry row is the result only where nothing iterates on it
                        const bool commit = entry ? a.iters == 0 : it == a.iters && j == m;
                        const float *A0 = Ab + (size_t)j * F, *A1 = A0 + F;
#if RTISI_TAPE
                        float2 *T0 = tape + ((((size_t)b * M + m) * a.iters + (it - 1)) * W + (j - m)) * F;
#endif
                        for (int k = threadIdx.x; k < F; k += blockDim.x) {
                            const float2 zk = r[k], zn = r[k == 0 ? 0 : N - k];
#if RTISI_TAPE
                            T0[k] = make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y));
                            if (two) T0[F + k] = make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x));
#endif
                            const float2 u = rtisi_project(make_float2(0.5f * (zk.x + zn.x), 0.5f * (zk.y - zn.y)), A0[k]);
                            float2 v = make_float2(0.f, 0.f);
                            if (two) v = rtisi_project(make_float2(0.5f * (zk.y + zn.y), 0.5f * (zn.x - zk.x)), A1[k]);
                            if (commit) Cb[(size_t)(entry ? j : m) * F + k] = u;
                            rtisi_put_pair(x, k, N, u, v);
                        }
                    }
                    __syncthreads();
                    // the transform's own uniforms (its strides, quotients and stage masks) are derived here, at the call, from
                    // values the compiler cannot see through: hoisted over all five loops they cost more SGPRs than a wave has
                    int n_ = N, odd_ = a.odd, log2e_ = a.log2e;
                    asm volatile("" : "+s"(n_), "+s"(odd_), "+s"(log2e_));
                    r = fft_lds<RTISI_TAPE ? FFT_USER_RTISI_TAPE : START == LWS_START_GIVEN ? FFT_USER_RTISI : FFT_USER_RTISI_OVERLAP>(
                        x, y, n_, odd_, log2e_, ph == 0 ? -1.0f : 1.0f);
                }
                // times the synthesis window, into the slots of frames j and j + 1
                const float inv = 1.0f / (float)N;
                float *o0 = dst + (size_t)slot * N, *o1 = dst + (size_t)(slot < a.LA ? slot + 1 : 0) * N;
                for (int n = threadIdx.x; n < N; n += blockDim.x) {
                    const float w = inv * swin[n];
                    o0[n] = r[n].x * w;
                    if (two) o1[n] = r[n].y * w;
                }
                __syncthreads();   // r is the next load's buffer, dst the next reader's
                slot += entry ? 1 : 2;
                if (slot > a.LA) slot -= W;
                if (slot > a.LA) slot -= W;   // W == 1
            }
            if (it > 0) { fnxt = fcur; fcur = dst; }
        }
        // done += f_m; what no later frame reaches is final: hop samples, or all N behind the last frame
        const float *fm = fcur + (size_t)slot_m * N;
        const int nfinal = m == M - 1 ? N : hop;
        for (int n = threadIdx.x; n < N; n += blockDim.x) {
            int pos = base + n;
            if (pos >= R) pos -= R;
            const float v = ring[pos] + fm[n];
            const int t = hop * m + n;
            if (n < nfinal) {
                if (xb && t >= a.zero_lo && t < t_end) xb[t - a.zero_lo] = v;
                ring[pos] = 0.f;
            } else {
                ring[pos] = v;
            }
        }
        base += hop;
        if (base >= R) base -= R;
        if (++slot_m > a.LA) slot_m = 0;
        __syncthreads();
    }
}
