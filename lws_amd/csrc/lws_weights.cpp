// lws_weights.cpp -- the analysis of a weight tensor (lws_weights.h): everything the engine guards want to know about W, which never
// changes after plan creation, from one place.
#include "lws_weights.h"

#include <cmath>
#include <cstddef>

#include "lws_band_host.h"

namespace lws {
namespace {

// how the unit twiddle exp(2 pi j p r s / P) of a row is formed and applied
enum class Turn {
    CosSin,    // std::cos / std::sin of the reduced angle
    OnAxes,    // band::unit: exact on the axes (the band engine's tables are made of these)
    Quarters,  // P in {2, 4}: a swap of the components, no product (the fp64 systolic kernel compiles these in)
};

struct Tensor {
    const double *W;
    int Q, Qp, K1;
    double scale;
    double at(int p, int r, int k, int c) const { return W[2 * (((size_t)p * Q + r) * K1 + k) + c]; }

    // Every row the image of row 0 under exp(2 pi j p r s / P), to `tol` of the largest weight?  skips: ... and the rows agree
    // about which weights the reference skips by their own magnitude (lws.pyx:232) -- rows that do not cannot share row 0.
    bool rows_follow(int P, int s, double tol, bool skips, Turn turn) const {
        for (int p = 0; p < Qp; ++p)
            for (int r = 0; r < Q; ++r) {
                const long long num = ((long long)p * r * s) % P;
                double cr = 1, ci = 0;
                if (turn == Turn::OnAxes) {
                    band::unit(num, P, &cr, &ci);
                } else if (turn == Turn::CosSin) {
                    const double ang = 2.0 * M_PI * (double)num / P;
                    cr = std::cos(ang); ci = std::sin(ang);
                }
                const int n = turn == Turn::Quarters ? (int)(4 * num / P) : 0;
                for (int k = 0; k < K1; ++k) {
                    if (r == 0 && k == 0) continue;   // never read by the kernels (update == 2)
                    const double br = at(0, r, k, 0), bi = at(0, r, k, 1);
                    double er, ei;
                    if (turn == Turn::Quarters) {
                        er = n == 0 ? br : (n == 1 ? -bi : (n == 2 ? -br : bi));
                        ei = n == 0 ? bi : (n == 1 ? br : (n == 2 ? -bi : -br));
                    } else {
                        er = br * cr - bi * ci;
                        ei = br * ci + bi * cr;
                    }
                    if (std::hypot(at(p, r, k, 0) - er, at(p, r, k, 1) - ei) > tol * scale) return false;
                    if (skips && (std::hypot(at(p, r, k, 0), at(p, r, k, 1)) > 1e-12) != (std::hypot(br, bi) > 1e-12)) return false;
                }
            }
        return true;
    }

    int row_period(int pmax) const {
        const size_t RQ = (size_t)Q * K1;
        for (int P = 1; P <= pmax && P <= Qp; ++P) {
            if (Qp % P != 0) continue;
            bool ok = true;
            for (int p = P; p < Qp && ok; ++p)
                for (size_t x = 0; x < RQ; ++x) {
                    const size_t i = (size_t)p * RQ + x, j = (size_t)(p % P) * RQ + x;
                    if (std::hypot(W[2 * i] - W[2 * j], W[2 * i + 1] - W[2 * j + 1]) > 1e-9 * scale) { ok = false; break; }
                }
            if (ok) return P;
        }
        return 0;
    }

    void twiddle_fits(int pmax, std::vector<std::pair<int, int>> &fits) const {
        auto verify = [&](int P, int sg) {
            // the rows a kernel reads besides p = bin: p = Qp - bin (modneg, lwslib.cpp:300,408)
            return ((long long)Qp * sg) % P == 0 && rows_follow(P, sg, 1e-9, false, Turn::CosSin);
        };
        if (Qp == 1) { fits.emplace_back(1, 0); return; }
        // the turn per bin, theta = s / P, from row 1 against row 0 on the largest weight of the first frame offset r that has one:
        // that gives r theta mod 1, i.e. r candidates for theta
        int rb = 0, kb = 0;
        for (int r = 1; r < Q && rb == 0; ++r)
            for (int k = 0; k < K1; ++k)
                if (std::hypot(at(0, r, k, 0), at(0, r, k, 1)) > std::fmax(1e-6 * scale, rb ? std::hypot(at(0, rb, kb, 0), at(0, rb, kb, 1)) : 0.0)) { rb = r; kb = k; }
        if (rb == 0) {   // nothing but the centre frame: the rows must simply repeat row 0
            if (verify(1, 0)) fits.emplace_back(0, 0);
            return;
        }
        const double br = at(0, rb, kb, 0), bi = at(0, rb, kb, 1), wr = at(1, rb, kb, 0), wi = at(1, rb, kb, 1);
        double tr = std::atan2(wi * br - wr * bi, wr * br + wi * bi) / (2.0 * M_PI);   // arg(w / b) in turns = rb theta mod 1
        tr -= std::floor(tr);
        for (int j = 0; j < rb; ++j) {
            const double theta = (tr + j) / rb;
            for (int P = 1; P <= pmax; ++P) {
                const double sp = theta * P, sr = std::round(sp);
                if (std::fabs(sp - sr) > 1e-7) continue;
                const int sg = (int)sr % P;
                if (verify(P, sg)) fits.emplace_back(P, sg);
                break;                                        // (the smallest P of this candidate: if it fails, multiples of it fail too)
            }
        }
    }
};

}  // namespace

WeightStructure analyse_weights(const double *W, int Q, int Qp, int L) {
    WeightStructure ws;
    if (!W || Q < 1 || Qp < 1 || L < 0) return ws;
    Tensor t{W, Q, Qp, L + 1, 0.0};
    for (size_t x = 0; x < (size_t)Qp * Q * t.K1; ++x) t.scale = std::fmax(t.scale, std::hypot(W[2 * x], W[2 * x + 1]));
    ws.scale = t.scale;
    ws.row_period = Qp == Q ? Q : t.row_period(256);
    if (Q < 2 || !(t.scale > 0)) return ws;
    t.twiddle_fits(4096, ws.fits);
    int P = 0, s = 0;
    if (ws.twiddle(4096, &P, &s)) {
        if (P < 1) { P = 1; s = 0; }
        ws.band_rows_fp64 = t.rows_follow(P, s, 1e-13, true, Turn::OnAxes);
        ws.band_rows_fp32 = t.rows_follow(P, s, 1e-9, true, Turn::OnAxes);
    }
    if ((Q == 2 || Q == 4) && Qp % Q == 0) ws.quarter_turns = t.rows_follow(Q, 1, 1e-13, true, Turn::Quarters);
    return ws;
}

}  // namespace lws
