// lws_weights.h -- what the engines ask about a weight tensor, answered once (lws_weights.cpp; plan creation fills one record per
// tensor).  Host only, no HIP: tests/test_weight_analysis.py compiles it with g++.
#pragma once

#include <utility>
#include <vector>

namespace lws {

// Structure of a weight tensor W[Qp][Q][L+1] (host, complex128 interleaved).  create_weights (lws.pyx:160-181) builds
// W[p][r][k] == W[0][r][k] exp(2 pi j p r s / P) for every row p, s / P = hop / frame in lowest terms -- P = Q, s = 1 when the hop
// divides the frame -- for summarised (Qp = Q) and general (Qp = N) tensors alike.
struct WeightStructure {
    double scale = 0;       // largest |w|
    // Smallest P <= 256 dividing Qp such that the rows repeat with period P, to 1e-9 of the largest weight -- Q for a summarised
    // tensor (trivially), frame / gcd(frame, hop) for create_weights' general ones -- or 0.  The no-future LDS kernels then index
    // row (bin mod P) where the reference indexes row bin (LWSfractionalQ, lwslib.cpp:393,408: mod = bin, modneg = N - bin).
    int row_period = 0;
    // The twiddles (P, s), P <= 4096, the rows follow to 1e-9 of the largest weight: the turn per bin is read from row 1 against
    // row 0 at the first frame offset r that has a weight, which gives r candidates; the ones every row agrees with, in that order.
    // (1, 0): a tensor of one row.  (0, 0): no neighbour-frame weight at all and every row repeats row 0 -- fits any twiddle (W_ai
    // of hop = frame / 2).
    std::vector<std::pair<int, int>> fits;
    // ... and for the first of them ((0, 0) read as (1, 0)), with exact twiddles on the axes: every row the image of row 0 to
    // 1e-13 / to 1e-9, and the rows agree about which weights the reference skips (|w| <= 1e-12, lws.pyx:232)?  The band engine's
    // guard: an fp64 plan promises the reference's values to rounding, fp32 arithmetic needs no more than 1e-9.
    bool band_rows_fp64 = false, band_rows_fp32 = false;
    // Q in {2, 4}, Qp a multiple of Q: every row an exact quarter-turn image of row 0, to 1e-13, with the same agreement (sys64)
    bool quarter_turns = false;

    // The first twiddle of period <= pmax the tensor has (false: none)
    bool twiddle(int pmax, int *P, int *s) const {
        for (const auto &f : fits)
            if (f.first <= pmax) { *P = f.first; *s = f.second; return true; }
        return false;
    }
};

// W may be null (a tensor the plan does not have): no structure.
WeightStructure analyse_weights(const double *W, int Q, int Qp, int L);

}  // namespace lws
