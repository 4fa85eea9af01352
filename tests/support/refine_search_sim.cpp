// Host driver of csrc/refine_search.h for tests/test_sets_refine_host.py: one search on an analytic function, every
// number printed as a hexadecimal float so that the test compares bits.
//
// stdin:  d max_rounds nan_round
//         lo[d]  hi[d]  x0[d]
//         kind   ("quad": c[d], f = -1/2 sum (x - c)^2;  "gauss": m, C[m][d], W[m], f = sum_i W_i exp(-|x - C_i|^2 / 2);
//                 "nan": f = NaN everywhere)
// nan_round >= 1: the value of that round's trial point is reported as NaN (an Armijo failure); 0: never;
// nan_round = -r: every trial from round r on is NaN.
// stdout: one line "P x[d] value accepted" per evaluated point (the start first, then each round's trial; accepted = 1
//         when the point became the search's accepted point: the start, and every trial that passed the Armijo test), then
//         "E status rounds value x[d] g[d]" with the accepted point, its value and gradient (of the maximised function).
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "refine_search.h"

using namespace cbo;

int main()
{
    int d, max_rounds, nan_round;
    if (!(std::cin >> d >> max_rounds >> nan_round) || d < 1 || d > CBO_MAX_DIM) return 2;
    auto read_hex = [](double &v) {
        std::string t;
        if (!(std::cin >> t)) return false;
        v = std::strtod(t.c_str(), nullptr);
        return true;
    };
    double lo[CBO_MAX_DIM] = {0}, hi[CBO_MAX_DIM] = {0}, x0[CBO_MAX_DIM] = {0};
    for (int k = 0; k < d; ++k) if (!read_hex(lo[k])) return 2;
    for (int k = 0; k < d; ++k) if (!read_hex(hi[k])) return 2;
    for (int k = 0; k < d; ++k) if (!read_hex(x0[k])) return 2;
    std::string kind;
    std::cin >> kind;
    std::vector<double> C, W;
    int m = 0;
    if (kind == "quad") {
        C.resize(d);
        for (int k = 0; k < d; ++k) if (!read_hex(C[k])) return 2;
    } else if (kind == "gauss") {
        std::cin >> m;
        C.resize((size_t)m * d);
        W.resize(m);
        for (double &v : C) if (!read_hex(v)) return 2;
        for (double &v : W) if (!read_hex(v)) return 2;
    } else if (kind != "nan") {
        return 2;
    }
    auto eval = [&](const double *x, double &f, double *g) {
        if (kind == "quad") {
            double s = 0.0;
            for (int k = 0; k < d; ++k) { s += (x[k] - C[k]) * (x[k] - C[k]); g[k] = -(x[k] - C[k]); }
            f = -0.5 * s;
        } else if (kind == "gauss") {
            f = 0.0;
            for (int k = 0; k < d; ++k) g[k] = 0.0;
            for (int i = 0; i < m; ++i) {
                double s = 0.0;
                for (int k = 0; k < d; ++k) s += (x[k] - C[(size_t)i * d + k]) * (x[k] - C[(size_t)i * d + k]);
                const double e = W[i] * std::exp(-0.5 * s);
                f += e;
                for (int k = 0; k < d; ++k) g[k] -= e * (x[k] - C[(size_t)i * d + k]);
            }
        } else {
            f = NAN;
            for (int k = 0; k < d; ++k) g[k] = 0.0;
        }
    };
    std::vector<double> S((size_t)kRefineHistory * d), Y((size_t)kRefineHistory * d);
    RefineState st;
    refine_begin(st, d, x0, lo, hi, S.data(), Y.data());
    for (int evals = 0; !refine_done(st); ++evals) {
        if (evals > max_rounds + 1) return 3;                  // the state machine must end by itself
        const double *x = refine_point(st);
        double f, g[CBO_MAX_DIM];
        eval(x, f, g);
        if ((nan_round >= 1 && evals == nan_round) || (nan_round < 0 && evals >= -nan_round)) f = NAN;
        std::printf("P");
        for (int k = 0; k < d; ++k) std::printf(" %a", x[k]);
        double point[CBO_MAX_DIM];
        for (int k = 0; k < d; ++k) point[k] = x[k];
        refine_feed(st, lo, hi, f, g, max_rounds);
        // accepted: the point is now the search's accepted point with this value (a trial that failed the Armijo test
        // leaves the accepted point where it was)
        bool accepted = std::isfinite(f) && st.f == -f;
        for (int k = 0; k < d; ++k) accepted = accepted && st.x[k] == point[k];
        std::printf(" %a %d\n", f, accepted ? 1 : 0);
    }
    std::printf("E %d %d %a", st.status, st.rounds, -st.f);
    for (int k = 0; k < d; ++k) std::printf(" %a", st.x[k]);
    for (int k = 0; k < d; ++k) std::printf(" %a", -st.g[k]);
    std::printf("\n");
    return 0;
}
