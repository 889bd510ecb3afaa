// online_unit_main.cpp -- lws_amd/csrc/lws_online_unit.h on its own (tests/test_online_unit.py compares this with the reference's loop nest).
//   online_unit_main T LA n_thr Q   one line per (s, j), s = 0 .. T (n_thr + 1) - 1, j = 0 .. LA, in that order:
//                                   s j valid m q rho wset centre ts
#include <cstdio>
#include <cstdlib>

#include "../lws_amd/csrc/lws_online_unit.h"

int main(int argc, char **argv) {
    if (argc != 5) { fprintf(stderr, "usage: online_unit_main T LA n_thr Q\n"); return 2; }
    const int T = atoi(argv[1]), LA = atoi(argv[2]), n_thr = atoi(argv[3]), Q = atoi(argv[4]);
    const int per = n_thr + 1;
    for (long s = 0; s < (long)T * per; ++s)
        for (int j = 0; j <= LA; ++j) {
            const lws::OnlineUnit u = lws::online_unit(s, j, per, LA, Q);
            const lws::OnlineUnit v = lws::online_unit((int)s, j, per, LA, Q);   // the LDS engines count sweeps in an int
            if (u.m != v.m || u.q != v.q || u.rho != v.rho || u.wset != v.wset || u.ts != v.ts || u.valid != v.valid || u.centre != v.centre) {
                fprintf(stderr, "int and long sweep numbers disagree at s = %ld, j = %d\n", s, j);
                return 1;
            }
            printf("%ld %d %d %d %d %d %d %d %d\n", s, j, (int)u.valid, u.m, u.q, u.rho, u.wset, (int)u.centre, u.ts);
        }
    return 0;
}
