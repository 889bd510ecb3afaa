// systolic_geometry_main.cpp -- lws_amd/csrc/lws_systolic_geom.h on its own (tests/test_systolic_geometry.py feeds it cases).
// stdin: one case per line,  rowl_shift skew lag nslots wps  F Q B T iters n_cu forced h16
// stdout: the geometry of each, one line of name=value fields.
#include <cstdio>

#include "../lws_amd/csrc/lws_systolic_geom.h"

int main() {
    lws::SystolicDims d;
    int F, Q, B, T, iters, n_cu, forced, h16;
    while (scanf("%d %d %d %d %d %d %d %d %d %d %d %d %d", &d.rowl_shift, &d.skew, &d.lag, &d.nslots, &d.wps, &F, &Q, &B, &T, &iters, &n_cu,
                 &forced, &h16) == 13) {
        const lws::SystolicGeom g = lws::systolic_geometry(d, F, Q, B, T, iters, n_cu, forced, h16 != 0);
        printf("Tp=%d Kr=%d Kt=%d G=%d TpPad=%d NT=%d nwg=%d n_full=%d nwg_rest=%d cb=%d rb=%d ring_max=%d", g.Tp, g.Kr, g.Kt, g.G, g.TpPad,
               g.NT, g.nwg, g.n_full, g.nwg_rest, g.cb, g.rb, g.ring_max);
        printf(" n_w=%zu n_n=%zu n_prog=%zu off_state_nyq=%zu need_s=%zu off_amp_nyq=%zu off_amax=%zu off_thr_min=%zu off_progress=%zu"
               " off_err=%zu need_a=%zu", g.n_w, g.n_n, g.n_prog, g.off_state_nyq, g.need_s, g.off_amp_nyq, g.off_amax, g.off_thr_min,
               g.off_progress, g.off_err, g.need_a);
        printf(" io_partials=%d\n", lws::systolic_Kt(T + 2 * (Q - 1)) * lws::systolic_NT(d.skew, F));
    }
    return 0;
}
