// lws_systolic_driver.hip -- what every build of the systolic engine shares, compiled once: the layout passes
// (lws_systolic_layout.h) and the host side of a call -- scratch, the conversion to the skewed layout, the launches of the
// build's update kernel (SystolicBuild::launch_update, lws_systolic.hip) with their workgroup counts, schedules longer than
// one launch and the re-run after a failed hand-over, and the conversion back.
#include "lws_common.h"
#include "lws_systolic.h"
#include "lws_systolic_layout.h"

#include <cstdio>
#include <type_traits>

namespace lws {

void systolic_release(SystolicPlan &sp) {
    for (int i = 0; i < 3; ++i) {
        if (sp.tables[i] && static_cast<SystolicTables *>(sp.tables[i])->tw_dev) (void)hipFree(static_cast<SystolicTables *>(sp.tables[i])->tw_dev);
        delete static_cast<SystolicTables *>(sp.tables[i]);
        sp.tables[i] = nullptr;
        sp.ok[i] = false;
    }
    if (sp.sk_state) (void)hipFree(sp.sk_state);
    if (sp.sk_amp) (void)hipFree(sp.sk_amp);
    if (sp.thr_chunk) (void)hipFree(sp.thr_chunk);
    sp.sk_state = sp.sk_amp = sp.thr_chunk = nullptr;
    sp.sk_state_cap = sp.sk_amp_cap = sp.thr_chunk_cap = 0;
}

bool systolic_supports(const SystolicPlan &sp, int wsel, int T) {
    return wsel >= 0 && wsel < 3 && sp.ok[wsel] && T >= 1;  // (any number of sweeps: more than MAX_ITERS run as several launches)
}

const char *systolic_name(const SystolicPlan &sp) { return sp.name; }

namespace {

static_assert(Store<true>::CB == 4 && Store<true>::RB == 2 && Store<false>::CB == 8 && Store<false>::RB == 4, "SystolicGeom::cb, rb");

hipError_t grow(void *&buf, size_t &cap, size_t need) {
    if (need <= cap) return hipSuccess;
    if (buf) (void)hipFree(buf);
    buf = nullptr; cap = 0;
    const hipError_t e = hipMalloc(&buf, need);
    if (e == hipSuccess) cap = need;
    return e;
}

// dense threshold table of one launch of a schedule longer than MAX_ITERS sweeps (a synchronising hipMalloc when it grows)
hipError_t ensure_thr_chunk(SystolicPlan &sp, int B, int iters) {
    return iters <= MAX_ITERS ? hipSuccess : grow(sp.thr_chunk, sp.thr_chunk_cap, (size_t)B * MAX_ITERS * sizeof(float));
}

// (grows the plan's scratch if needed -- a synchronising hipMalloc; systolic_reserve() does that ahead of time)
hipError_t prepare(const SystolicBuild &b, SystolicPlan &sp, int B, int T, int iters, SystolicCall &g) {
    hipError_t e;
    int n_cu = 0, dev = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    static_cast<SystolicGeom &>(g) = systolic_geometry(b.dims, sp.F, sp.Q, B, T, iters, n_cu, sp.sw->systolic_nwg, sp.h16);
    if ((e = grow(sp.sk_state, sp.sk_state_cap, g.need_s)) != hipSuccess) return e;
    if ((e = grow(sp.sk_amp, sp.sk_amp_cap, g.need_a)) != hipSuccess) return e;
    g.state_w = static_cast<char *>(sp.sk_state);
    g.state_nyq = g.state_w + g.off_state_nyq;
    g.amp_w = static_cast<char *>(sp.sk_amp);
    g.amp_nyq = g.amp_w + g.off_amp_nyq;
    g.amax_bits = reinterpret_cast<unsigned *>(g.amp_w + g.off_amax);
    g.thr_min = reinterpret_cast<float *>(g.amp_w + g.off_thr_min);
    g.progress = reinterpret_cast<unsigned *>(g.amp_w + g.off_progress);
    g.err = reinterpret_cast<int *>(g.amp_w + g.off_err);
    return hipSuccess;
}

hipError_t clear_flags(const SystolicCall &g, hipStream_t stream) {   // amax | thr_min | progress counters | error flag
    return hipMemsetAsync(g.amax_bits, 0, g.need_a - g.off_amax, stream);
}

Skew skew_of(const SystolicBuild &b, const SystolicPlan &sp, const SystolicCall &g, int T) {
    return Skew{T, sp.Q, sp.F - 1, g.G, g.TpPad, g.NT, b.dims.rowl_shift, b.dims.skew};
}

// f(std::bool_constant<H16>) for the plan's storage format: every launch of a layout pass is written once
template <typename F> void for_format(bool h16, F f) {
    if (h16) f(std::true_type{});
    else f(std::false_type{});
}

// caller's data -> skewed layout (gate: see k_to_skew; H16: the largest magnitude is taken once, before the first conversion)
template <typename Source>
hipError_t load(const SystolicBuild &b, SystolicPlan &sp, const SystolicCall &g, Source src, double *partial, int B, int T,
                hipStream_t stream, const int *gate) {
    for_format(sp.h16, [&](auto h16) {
        hipLaunchKernelGGL((k_to_skew<decltype(h16)::value, Source>), dim3(g.Kt * g.NT, B), dim3(256), 0, stream, src, (void *)g.state_w, (void *)g.amp_w,
                           (void *)g.state_nyq, (void *)g.amp_nyq, g.amax_bits, partial, skew_of(b, sp, g, T), gate);
    });
    return hipGetLastError();
}
hipError_t load_extended(const SystolicBuild &b, SystolicPlan &sp, const SystolicCall &g, float2 *state, const float *amp, int B, int T,
                         hipStream_t stream, const int *gate) {
    const int Np = sp.F + 2 * sp.L;
    if (sp.h16 && !gate)   // (real frames only; the pad columns repeat real bins)
        hipLaunchKernelGGL(k_amax<float>, dim3(64, B), dim3(256), 0, stream, amp + (size_t)(sp.Q - 1) * Np,
                           (size_t)(T + 2 * (sp.Q - 1)) * Np, (size_t)T * Np, g.amax_bits);
    return load(b, sp, g, Extended{state, amp, Np, sp.L}, nullptr, B, T, stream, gate);
}
hipError_t load_callers(const SystolicBuild &b, SystolicPlan &sp, const SystolicCall &g, const float2 *in, int B, int T, double *partial,
                        hipStream_t stream, const int *gate) {
    if (sp.h16 && !gate)
        hipLaunchKernelGGL(k_amax<float2>, dim3(64, B), dim3(256), 0, stream, in, (size_t)T * sp.F, (size_t)T * sp.F, g.amax_bits);
    return load(b, sp, g, Callers{in, nullptr, sp.F}, partial, B, T, stream, gate);
}
// skewed layout -> caller's data
template <typename Sink>
hipError_t unload(const SystolicBuild &b, SystolicPlan &sp, const SystolicCall &g, Sink dst, int B, int T, hipStream_t stream) {
    for_format(sp.h16, [&](auto h16) {
        hipLaunchKernelGGL((k_from_skew<decltype(h16)::value, Sink>), dim3(g.Kt * g.NT, B), dim3(256), 0, stream, dst, (void *)g.state_w,
                           (void *)g.state_nyq, reinterpret_cast<const float *>(g.amax_bits), (const float *)g.thr_min, skew_of(b, sp, g, T));
    });
    return hipGetLastError();
}

// All sweeps of a call, state in the skewed layout.  `reload(gate)` re-creates that layout from the caller's (still
// untouched) data, as a launch that only runs if *gate != 0.
template <typename Reload>
hipError_t run_kernel(const SystolicBuild &b, SystolicPlan &sp, const SystolicCall &g, int wsel, const float *thr, int B, int T, int iters,
                      hipStream_t stream, int *launches, Reload reload) {
    const int WPS = b.dims.wps;
    hipError_t e = hipSuccess;
    if (sp.h16) {
        hipLaunchKernelGGL(k_thr_min, dim3(B), dim3(64), 0, stream, thr, reinterpret_cast<const float *>(g.amax_bits), iters, g.thr_min);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if ((e = ensure_thr_chunk(sp, B, iters)) != hipSuccess) return e;
    int n_launch = 0;
    bool multi = false, refused0 = false, refused1 = false;
    // one launch of the build's kernel; the kernel's name as lws_last_kernel_name reports it
    auto update = [&](const float *thr_c, int n_it, int b0, int nb, int nwg, unsigned *progress, const int *gate) {
        const char *kind = nullptr;
        const hipError_t eu = b.launch_update(sp, g, wsel, thr_c, n_it, b0, nb, nwg, progress, gate, T, stream, &kind);
        if (kind) {
            snprintf(sp.name_buf, sizeof sp.name_buf, "systolic%s_q%d_l%d_%s%s", b.tag, sp.Q, sp.Lk, kind, sp.h16 ? "_f16" : "");
            sp.name = sp.name_buf;
        }
        return eu;
    };
    // every sweep of the call, either with the workgroup counts of `g` or (single) with one workgroup per spectrogram
    auto sweep_all = [&](bool single, const int *gate) -> hipError_t {
        // more sweeps than one launch's threshold table holds: several launches over the same (resident) skewed state.
        // Same results: a launch boundary is just a longer lag between two sweeps.
        for (int it0 = 0; it0 < iters; it0 += MAX_ITERS) {
            const int n_it = iters - it0 < MAX_ITERS ? iters - it0 : MAX_ITERS;
            const float *thr_c = thr;
            if (iters > MAX_ITERS) {   // the kernel reads a dense [B][n_iters] table: this launch's columns, copied in stream order
                if ((e = hipMemcpy2DAsync(sp.thr_chunk, (size_t)n_it * sizeof(float), thr + it0, (size_t)iters * sizeof(float),
                                          (size_t)n_it * sizeof(float), B, hipMemcpyDeviceToDevice, stream)) != hipSuccess) return e;
                thr_c = static_cast<const float *>(sp.thr_chunk);
            }
            for (int chunk = 0; chunk < (single ? 1 : 2); ++chunk) {
                // chunk 0: the first n_full spectrograms (all of them unless the batch leaves a partial last round on the
                // chip); chunk 1: the rest, with several workgroups per spectrogram
                const int b0 = (single || chunk == 0) ? 0 : g.n_full;
                const int nb = single ? B : (chunk == 0 ? g.n_full : B - g.n_full);
                const int nwg = single ? 1 : (chunk == 0 ? g.nwg : g.nwg_rest);
                if (nb <= 0) continue;
                unsigned *progress = g.progress + (chunk == 0 ? 0 : (size_t)B * g.nwg * WPS);
                if (nwg > 1 && n_launch > 0) {   // multi-workgroup launches re-use the counters: start them from zero again
                    if ((e = hipMemsetAsync(progress, 0, (size_t)nb * nwg * WPS * sizeof(unsigned), stream)) != hipSuccess) return e;
                }
                e = update(thr_c, n_it, b0, nb, nwg, progress, gate);
                if (e == hipErrorLaunchOutOfResources && nwg > 1 && it0 == 0) {
                    // the occupancy guard refused a grid of several workgroups per spectrogram (launch_km): nothing was launched for
                    // these spectrograms -- serve them with one workgroup each (same results), here and in the launches that follow
                    (void)hipGetLastError();
                    if (chunk == 0) refused0 = true; else refused1 = true;
                }
                if ((chunk == 0 ? refused0 : refused1) && nwg > 1)
                    e = update(thr_c, n_it, b0, nb, 1, progress, gate);
                else multi |= nwg > 1;
                if (e != hipSuccess) return e;
                if (!gate) ++n_launch;
            }
        }
        return hipSuccess;
    };
    if ((e = sweep_all(false, nullptr)) != hipSuccess) return e;
    if (multi) {
        // Several workgroups per spectrogram hand rows over through HBM and need each other resident.  If one of them
        // timed out (flag set), everything is done again with one workgroup per spectrogram, from the caller's data: the
        // launches below are enqueued unconditionally and return at once unless the flag is set, so the call stays
        // asynchronous and never returns the results of a failed hand-over.
        if ((e = reload(g.err)) != hipSuccess) return e;
        if ((e = sweep_all(true, g.err)) != hipSuccess) return e;
    }
    sp.err_dev = g.err; sp.last_nwg = multi ? (g.nwg > g.nwg_rest ? g.nwg : g.nwg_rest) : 1;
    if (launches) *launches = n_launch;
    return e;
}

}  // namespace

hipError_t systolic_reserve(const SystolicBuild &b, SystolicPlan &sp, int B, int T, int iters) {
    SystolicCall g;
    hipError_t e = prepare(b, sp, B, T, iters, g);
    if (e != hipSuccess) return e;
    return ensure_thr_chunk(sp, B, iters);   // (schedules longer than one launch's table: sized here, not in the first call)
}

hipError_t launch_systolic(const SystolicBuild &b, SystolicPlan &sp, int wsel, float2 *state, const float *amp, const float *thr, int B,
                           int T, int iters, hipStream_t stream, int *launches, hipEvent_t ev0, hipEvent_t ev1) {
    SystolicCall g;
    hipError_t e;
    if ((e = prepare(b, sp, B, T, iters, g)) != hipSuccess) return e;
    if ((e = clear_flags(g, stream)) != hipSuccess) return e;
    auto reload = [&](const int *gate) { return load_extended(b, sp, g, state, amp, B, T, stream, gate); };
    if ((e = reload(nullptr)) != hipSuccess) return e;
    if (ev0) (void)hipEventRecord(ev0, stream);
    if ((e = run_kernel(b, sp, g, wsel, thr, B, T, iters, stream, launches, reload)) != hipSuccess) return e;
    if (ev1) (void)hipEventRecord(ev1, stream);
    return unload(b, sp, g, Extended{state, amp, sp.F + 2 * sp.L, sp.L}, B, T, stream);
}

// ---- a call that is one batch stage on the caller's unpadded complex64 spectrograms: no extended buffers at all
size_t systolic_io_partials(const SystolicBuild &b, const SystolicPlan &sp, int T) {            // one partial sum per tile of k_to_skew
    return (size_t)systolic_Kt(T + 2 * (sp.Q - 1)) * systolic_NT(b.dims.skew, sp.F);
}

hipError_t systolic_io_load(const SystolicBuild &b, SystolicPlan &sp, const float2 *in, int B, int T, int iters, double *partial,
                            double *mean_amp, hipStream_t stream) {
    SystolicCall g;
    hipError_t e;
    if ((e = prepare(b, sp, B, T, iters, g)) != hipSuccess) return e;
    if ((e = clear_flags(g, stream)) != hipSuccess) return e;
    if ((e = load_callers(b, sp, g, in, B, T, partial, stream, nullptr)) != hipSuccess) return e;
    hipLaunchKernelGGL(k_mean_partials, dim3(B), dim3(256), 0, stream, partial, mean_amp, g.Kt * g.NT, (double)T * (double)sp.F);
    return hipGetLastError();
}

hipError_t systolic_io_run(const SystolicBuild &b, SystolicPlan &sp, int wsel, const float *thr, const float2 *in, float2 *out,
                           double *partial, int B, int T, int iters, hipStream_t stream, int *launches, hipEvent_t ev0, hipEvent_t ev1) {
    SystolicCall g;
    hipError_t e;
    if ((e = prepare(b, sp, B, T, iters, g)) != hipSuccess) return e;   // same shapes: no reallocation, same pointers
    if (ev0) (void)hipEventRecord(ev0, stream);
    auto reload = [&](const int *gate) { return load_callers(b, sp, g, in, B, T, partial, stream, gate); };
    if ((e = run_kernel(b, sp, g, wsel, thr, B, T, iters, stream, launches, reload)) != hipSuccess) return e;
    if (ev1) (void)hipEventRecord(ev1, stream);
    return unload(b, sp, g, Callers{in, out, sp.F}, B, T, stream);
}

}  // namespace lws
