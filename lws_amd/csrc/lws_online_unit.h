// lws_online_unit.h -- the decode of an online sweep: TF_RTISI_LA's loop nest (lwslib.cpp:1432-1491) turned inside out, written once for
// every engine that runs the online driver (lws_generic.hip, lws_team.hip, lws_online.hip, lws_online64.hip).
//
// The reference, for each new frame m: one first estimate of frame m from the past (W_ai, threshold 0, no centre frame, nothing to
// its right); then, for each of the n_thr iterations, frames max(0, m - LA) .. m in order, the look-ahead frames with W, frame m with
// W_af, each with as many frames to its right as exist yet (up to Q - 1).  Every one of those calls is a SWEEP, numbered in call
// order per frame position: sweep s = m per + q, per = n_thr + 1, and an engine works on the j-th frame of a sweep, j = 0 .. LA.
//
// The same text compiles for the GPU (hipcc) and for the host (g++: tests/online_unit_main.cpp prints the units and
// tests/test_online_unit.py holds them to a restatement of the loop nest), like lws_band_core.h.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LWS_UNIT_FN __host__ __device__ __forceinline__
#else
#define LWS_UNIT_FN inline
#endif

namespace lws {

struct OnlineUnit {
    int m, q;       // newest frame of the sweep; 0: its first estimate, else iteration q - 1 (threshold index q - 1)
    int rho;        // the frame this unit updates
    int wset;       // weight tensor: 0 W, 1 W_ai, 2 W_af
    int ts;         // frames usable on the right, plus one (the reference's rframe, lwslib.cpp:1143-1151)
    bool valid;     // the sweep has a j-th frame
    bool centre;    // the frame's own bins take part (cframe)
};

// Sweep: the caller's type of a sweep number (int where T (n_thr + 1) is known to fit, as in the LDS engines: a 32-bit division)
template <typename Sweep> LWS_UNIT_FN OnlineUnit online_unit(Sweep s, int j, int per, int LA, int Q) {
    OnlineUnit u;
    u.m = (int)(s / per);
    u.q = (int)(s - (Sweep)u.m * per);
    const int first = u.m - LA > 0 ? u.m - LA : 0;
    if (u.q == 0) { u.valid = (j == 0); u.rho = u.m; u.wset = 1; u.centre = false; u.ts = 1; }
    else {
        u.rho = first + j; u.valid = u.rho <= u.m; u.wset = (u.rho == u.m) ? 2 : 0; u.centre = true;
        u.ts = u.m - u.rho + 1; if (u.ts > Q) u.ts = Q;
    }
    return u;
}

}  // namespace lws
