// lws_systolic.h -- interface of the systolic batch-LWS engine: the builds of its update kernel (lws_systolic.hip, one
// compilation per row of lws_systolic_builds.h) and the driver they all share (lws_systolic_driver.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "lws_switches.h"
#include "lws_systolic_geom.h"
#include "lws_systolic_builds.h"
#include "lws_weights.h"

namespace lws {

struct SystolicPlan {
    bool ok[3] = {false, false, false};  // per weight tensor: kernel applicable
    int F = 0, L = 0, Q = 0;
    int Lk = 0;               // stencil half-width of the kernel build that serves the plan: L, or L + 1 for an even L (the
                              // windows are fetched as pairs of bins; the extra tap has weight zero and is never fetched)
    void *tables[3] = {nullptr, nullptr, nullptr};  // device weight tables
    void *sk_state = nullptr, *sk_amp = nullptr;    // skewed-layout scratch
    size_t sk_state_cap = 0, sk_amp_cap = 0;
    const char *name = "systolic";
    char name_buf[64] = {0};
    int *err_dev = nullptr;   // device flag of the last launch: a workgroup gave up waiting for its producer (the call was
                              // then re-run with one workgroup per spectrogram, on the device, before it completed)
    int last_nwg = 1;         // workgroups per spectrogram of the last launch
    bool h16 = false;         // fp16-complex storage of the skewed layout (LWS_STORAGE_FP16)
    void *thr_chunk = nullptr;   // dense threshold table of one launch of a schedule longer than one launch holds (MAX_ITERS)
    size_t thr_chunk_cap = 0;
    const Switches *sw = nullptr;   // the owner's snapshot (lws_capi.hip refreshes it in every public call): LWS_SYSTOLIC_NWG, _SPIN_LIMIT, _STRESS, _ROLEMAP
};

// The weights of one tensor as the update kernel takes them (made by a build's `build`, read by its `launch_update`).
constexpr int SYSTOLIC_NW_MAX = 144;   // the most weights a build carries (SysArgs::w of the Q = 8 builds)
struct SystolicTables {
    int Q, L;
    uint64_t mask;
    bool k0real, r13;  // structure the kernels can exploit (FLAG_K0REAL / FLAG_R13)
    // W[p][r][k] = W[0][r][k] exp(2 pi j p r tw_s / tw_P); LWS_TW: the table of the kernel on the device
    int tw_P = 0, tw_s = 0;
    float *tw_dev = nullptr;
    float tw_nyq[16] = {0};  // tau_r(F-1), r = 0..7
    float w[2 * SYSTOLIC_NW_MAX];   // (re, im) in the order of SysArgs::w
};

// Shapes (lws_systolic_geom.h) and scratch pointers of one call.
struct SystolicCall : SystolicGeom {
    char *state_w, *state_nyq;
    char *amp_w, *amp_nyq;
    unsigned *amax_bits, *progress;
    float *thr_min;
    int *err;
};

// What a build of lws_systolic.hip is, from its switches (plan creation skips some kinds on request: LWS_SYSTOLIC_NO_SHORT,
// LWS_SYSTOLIC_NO_TW, LWS_SYSTOLIC_NO_R16 -- comparison runs)
enum SystolicKind : unsigned {
    SYSTOLIC_SHORT = 1,   // short frames: two / four sweep slots per wave (LWS_SPW = 2 / 4)
    SYSTOLIC_TW = 2,      // twiddles from a table (LWS_TW)
    SYSTOLIC_TWQ = 4,     // ... on the ring of exactly 5 / 6 frames per stencil row (LWS_TWQ)
    SYSTOLIC_R16 = 8,     // Q = 2 on a 16-step ring (LWS_R16)
};

// One compilation of lws_systolic.hip (a row of lws_systolic_builds.h): its constants and the two things only it can do.
// Everything else is the shared driver below (lws_systolic_driver.hip), which takes the plan's build.
struct SystolicBuild {
    SystolicDims dims;
    unsigned kind;        // SystolicKind bits
    const char *tag;      // in the kernel's name: systolic<tag>_q<Q>_l<L>_<kind>
    // Upload tables for the (host, complex128 interleaved) weight tensors W, of the structure ws (lws_weights.h), that the
    // kernel can serve.  Never fails for "not applicable"; only for HIP errors.
    hipError_t (*build)(SystolicPlan &sp, int F, int L, int Q, int Qp, const double *const W[3], const WeightStructure ws[3], bool fp16_storage);
    // One launch of the update kernel over spectrograms [b0, b0 + nb) with `nwg` workgroups each: n_it sweeps.  *kind: which
    // instantiation ran ("hann", "allmask", ...).
    hipError_t (*launch_update)(SystolicPlan &sp, const SystolicCall &g, int wsel, const float *thr, int n_it, int b0, int nb, int nwg,
                                unsigned *progress, const int *gate, int T, hipStream_t stream, const char **kind);
};

void systolic_release(SystolicPlan &sp);
bool systolic_supports(const SystolicPlan &sp, int wsel, int T);
// Allocates the skewed-layout scratch for calls of up to B spectrograms x T frames (so that later calls do not).
hipError_t systolic_reserve(const SystolicBuild &b, SystolicPlan &sp, int B, int T, int iters);
const char *systolic_name(const SystolicPlan &sp);
// Runs `iters` batch sweeps on the extended buffers (reference layout), in place.
// ev0/ev1 (may be null) are recorded around the update kernel(s) only.
hipError_t launch_systolic(const SystolicBuild &b, SystolicPlan &sp, int wsel, float2 *state, const float *amp,
                           const float *thr, int B, int T, int iters, hipStream_t stream,
                           int *launches, hipEvent_t ev0, hipEvent_t ev1);
// A call that consists of one batch stage on device complex64 spectrograms [B][T][F] skips the extended buffers:
// systolic_io_load converts `in` straight to the kernel's layout and computes mean|S| (partial: scratch of
// B * systolic_io_partials() doubles), the caller scales the thresholds, systolic_io_run runs the sweeps and writes `out`.
size_t systolic_io_partials(const SystolicBuild &b, const SystolicPlan &sp, int T);
hipError_t systolic_io_load(const SystolicBuild &b, SystolicPlan &sp, const float2 *in, int B, int T, int iters, double *partial,
                            double *mean_amp, hipStream_t stream);
// (`in` and `partial` as given to systolic_io_load: a failed multi-workgroup hand-over re-converts from them; `in` may be `out`)
hipError_t systolic_io_run(const SystolicBuild &b, SystolicPlan &sp, int wsel, const float *thr, const float2 *in, float2 *out,
                           double *partial, int B, int T, int iters, hipStream_t stream, int *launches, hipEvent_t ev0, hipEvent_t ev1);

}  // namespace lws

// every build's entry, in its namespace ...
#define LWS_DECLARE_ENTRY(name) namespace LWS_ROW_FIELD(NS, name) { const lws::SystolicBuild &systolic_entry(); }
LWS_SYSTOLIC_BUILDS(LWS_DECLARE_ENTRY)
#undef LWS_DECLARE_ENTRY

namespace lws {
// ... and all of them in the order plan creation tries them (internal linkage: the library exports no symbol for it)
static inline const SystolicBuild *const *systolic_builds(int *n) {
#define LWS_ENTRY_PTR(name) &LWS_ROW_FIELD(NS, name)::systolic_entry(),
    static const SystolicBuild *const builds[] = {LWS_SYSTOLIC_BUILDS(LWS_ENTRY_PTR)};
#undef LWS_ENTRY_PTR
    *n = (int)(sizeof builds / sizeof builds[0]);
    return builds;
}
}  // namespace lws
