// lws_systolic_geom.h -- the shapes of one call of the systolic engine: plain integer arithmetic on the constants of a build
// (a row of lws_systolic_builds.h), the plan's (F, Q), the call's (B, T, sweeps), the number of CUs and LWS_SYSTOLIC_NWG.
// No HIP here: lws_systolic_driver.hip allocates and carves the scratch by these figures, tests/systolic_geometry_main.cpp
// prints them (compiled with g++).
#pragma once
#include <cstddef>

namespace lws {

constexpr int SYS_LANES = 64;        // lanes of a wave
constexpr int SYS_TILE = 64;         // the layout passes move tiles of 64 frames x 64 production times
constexpr int MAX_ITERS = 440;   // sweeps of one launch (their thresholds live in LDS); longer schedules run as several launches

// What the shared driver needs to know of a build of lws_systolic.hip.
struct SystolicDims {
    int rowl_shift;   // a ring row, hence a row of the skewed layout, holds ROWL = 1 << rowl_shift frames (a round)
    int skew;         // frame m trails frame m-1 by SKEW steps
    int lag;          // sweep j+1 trails sweep j by LAG steps
    int nslots;       // sweeps in flight per pass over HBM
    int wps;          // waves per sweep slot
    constexpr int rowl() const { return 1 << rowl_shift; }
    constexpr int rowp() const { return skew << rowl_shift; }   // steps of a round: the frame period of a lane
};

// Layout tiles (also the grid of the layout passes and the number of partial sums of mean|S|): Kt groups of 64 frames, each
// with NT time tiles -- a group's production times span SKEW*63 + C steps.  (constexpr: host and device)
constexpr int systolic_NT(int skew, int F) { return (skew * (SYS_LANES - 1) + (F - 1) + SYS_TILE - 1) / SYS_TILE; }
constexpr int systolic_Kt(int Tp) { return (Tp + SYS_LANES - 1) / SYS_LANES; }

struct SystolicGeom {
    int Tp, Kr, Kt, G, TpPad, NT, nwg;   // Kr: rounds of ROWL frames (the kernel's clock); Kt: groups of 64 frames (layout tiles)
    int n_full, nwg_rest;   // batches larger than the chip: n_full spectrograms with one workgroup each, then the rest
                            // (B - n_full, fewer than there are CUs) with nwg_rest workgroups each
    int cb, rb;             // bytes per stored complex value / magnitude (fp32: 8 / 4, fp16 storage: 4 / 2)
    int ring_max;           // most workgroups per spectrogram whose lags fit into one pass
    // the two scratch blocks, in bytes.  State block: state_w [B][G][ROWL] | state_nyq [B][TpPad].  Magnitude block: amp_w,
    // amp_nyq (the same shapes), then from a 16-byte boundary amax [B] | smallest threshold [B] | progress counters | error flag
    // (the last of the n_prog words)
    size_t n_w, n_n, n_prog;
    size_t off_state_nyq, need_s;
    size_t off_amp_nyq, off_amax, off_thr_min, off_progress, off_err, need_a;
};

inline SystolicGeom systolic_geometry(const SystolicDims &d, int F, int Q, int B, int T, int iters, int n_cu, int forced, bool h16) {
    SystolicGeom g;
    const int ROWL = d.rowl(), ROWP = d.rowp();
    g.cb = h16 ? 4 : 8;
    g.rb = h16 ? 2 : 4;
    g.Tp = T + 2 * (Q - 1);
    // rounds of ROWL frames per pass; at least so many that a pass (G rows) is longer than the lag of the last sweep slot behind
    // the loader plus what the loader reads ahead: pass g+1 follows pass g on the same clock and reads the rows pass g's last
    // slot has written (only the short-frame builds, with their 14 / 24 slots and short rounds, ever need the padding)
    const int KR_MIN = (d.nslots * d.lag + 96 + ROWP - 1) / ROWP;
    const int kr = (g.Tp + ROWL - 1) / ROWL;
    g.Kr = kr > KR_MIN ? kr : KR_MIN;
    g.Kt = systolic_Kt(g.Tp);
    g.G = ROWP * g.Kr;
    g.TpPad = (g.Tp + 63) & ~63;
    g.NT = systolic_NT(d.skew, F);
    // workgroups per spectrogram: as many as there are CUs to keep busy and passes to share out; every workgroup must
    // be resident (they wait for each other), which one workgroup per CU (the rings fill the LDS) and a grid no larger
    // than the CU count guarantee on a device this process has to itself; if they are not (a shared or partitioned
    // device), the hand-over times out and the call is re-run with one workgroup per spectrogram (run_kernel)
    const int n_pass_max = ((iters < MAX_ITERS ? iters : MAX_ITERS) + d.nslots - 1) / d.nslots;
    // each workgroup trails its producer by NSLOTS*LAG + 56 rows, and the first one starts its next pass G rows after
    // its previous one: the lags around the ring must fit into one pass
    g.ring_max = g.G / (d.nslots * d.lag + 96);
    auto pick = [&](int nb) {
        int n = nb > 0 ? n_cu / nb : 1;
        if (n > n_pass_max) n = n_pass_max;
        if (forced >= 1 && (long)forced * nb <= n_cu) n = forced;
        if (n > g.ring_max) n = g.ring_max;
        return n < 1 ? 1 : n;
    };
    g.nwg = pick(B);
    // a batch that does not fill the last round of workgroups: the spectrograms of that round share the idle CUs
    g.n_full = B; g.nwg_rest = 1;
    if (g.nwg == 1 && B > n_cu && B % n_cu != 0 && pick(B % n_cu) > 1) { g.n_full = B - B % n_cu; g.nwg_rest = pick(B % n_cu); }
    // sized for the largest number of workgroups any iteration count can give this batch, so that the scratch of a shape
    // does not grow with the schedule
    g.n_prog = ((size_t)B * (size_t)(n_cu / (B > 0 ? B : 1) + 1) + (size_t)n_cu) * d.wps + 8;
    g.n_w = (size_t)B * g.G * ROWL;
    g.n_n = (size_t)B * g.TpPad;
    g.off_state_nyq = g.n_w * g.cb;
    g.need_s = (g.n_w + g.n_n) * g.cb;
    g.off_amp_nyq = g.n_w * g.rb;
    g.off_amax = ((g.n_w + g.n_n) * g.rb + 15) & ~(size_t)15;
    g.off_thr_min = g.off_amax + (size_t)B * sizeof(unsigned);
    g.off_progress = g.off_thr_min + (size_t)B * sizeof(float);
    g.off_err = g.off_progress + (g.n_prog - 1) * sizeof(unsigned);
    g.need_a = g.off_progress + g.n_prog * sizeof(unsigned);
    return g;
}

}  // namespace lws
