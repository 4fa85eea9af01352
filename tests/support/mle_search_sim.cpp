// Host simulator of csrc/mle_search.h for tests/test_mle_sets_host.py: one search of the state machine, driven with a
// closed-form "likelihood" of theta this program evaluates itself, with u_k = log(theta_k):
//   quad:  lml = -sum_k (w_k (u_k - c_k)) (u_k - c_k) / 2            d lml / d theta_k = -(w_k (u_k - c_k)) / theta_k
//   rosen: lml = -sum_{k < P-1} (b (u_{k+1} - u_k^2)^2 + (1 - u_k)^2) - (1 - u_{P-1})^2 / 2     (the valley u = (1, .., 1))
// every sum from 0 in index order -- or NaN at evaluation number nan_at (counted from 0, the start; -1: never).  Every
// number is exchanged as a hexadecimal float.
// stdin:  P max_rounds nan_at start_is_x extra_feeds / start (P) / kind / parameters (quad: w (P), c (P); rosen: b).
//         start: theta0 (start_is_x = 0: the search transforms it itself) or the position x0 (1).  extra_feeds: feeds of a
//         made-up pair after the search has ended (they must change nothing).
// stdout: "P <x_0> .. <x_{P-1}> <lml> <accepted>"  every evaluated position in order, and whether the search moved there
//         "E <status> <rounds> <lml> <theta ..> <dlml ..> <x ..>"   the end
// Build: g++ -O2 -std=c++17 -ffp-contract=off -Iinclude -Icbo_with_oop_amd/csrc tests/support/mle_search_sim.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mle_search.h"

static bool read_hex(double &v)
{
    char buf[128];
    if (std::scanf("%127s", buf) != 1) return false;
    v = std::strtod(buf, nullptr);
    return true;
}

static bool read_hexes(std::vector<double> &v, size_t n)
{
    v.resize(n);
    for (size_t i = 0; i < n; ++i)
        if (!read_hex(v[i])) return false;
    return true;
}

int main()
{
    int P = 0, max_rounds = 0, nan_at = -1, start_is_x = 0, extra_feeds = 0;
    if (std::scanf("%d %d %d %d %d", &P, &max_rounds, &nan_at, &start_is_x, &extra_feeds) != 5) return 2;
    if (P < 1 || P > cbo::kMleMaxParams || max_rounds < 0 || max_rounds > 100000 || extra_feeds < 0) return 2;
    std::vector<double> start, w, c;
    double b = 0.0;
    char kind[16];
    if (!read_hexes(start, (size_t)P) || std::scanf("%15s", kind) != 1) return 2;
    const bool quad = std::strcmp(kind, "quad") == 0;
    if (quad) {
        if (!read_hexes(w, (size_t)P) || !read_hexes(c, (size_t)P)) return 2;
    } else if (std::strcmp(kind, "rosen") == 0) {
        if (!read_hex(b)) return 2;
    } else {
        return 2;
    }

    std::vector<double> S((size_t)cbo::kRefineHistory * (size_t)P, 0.0), Y((size_t)cbo::kRefineHistory * (size_t)P, 0.0);
    cbo::MleSearch s;
    if (start_is_x) cbo::mle_begin_at(s, P, start.data(), S.data(), Y.data());
    else cbo::mle_begin(s, P, start.data(), S.data(), Y.data());

    auto evaluate = [&](const double *th, double &lml, double *dl) {
        double u[cbo::kMleMaxParams] = {0.0};
        for (int k = 0; k < P; ++k) u[k] = std::log(th[k]);
        double sum = 0.0;
        if (quad) {
            for (int k = 0; k < P; ++k) {
                const double r = u[k] - c[(size_t)k];
                sum = sum + (w[(size_t)k] * r) * r / 2.0;
                dl[k] = -(w[(size_t)k] * r) / th[k];
            }
        } else {
            double du[cbo::kMleMaxParams];
            for (int k = 0; k < P; ++k) du[k] = 0.0;
            for (int k = 0; k + 1 < P; ++k) {
                const double v = u[k + 1] - u[k] * u[k], o = 1.0 - u[k];
                sum = sum + (b * v * v + o * o);
                du[k] = du[k] + (-4.0 * b * v * u[k] - 2.0 * o);
                du[k + 1] = du[k + 1] + 2.0 * b * v;
            }
            const double o = 1.0 - u[P - 1];
            sum = sum + o * o / 2.0;
            du[P - 1] = du[P - 1] - o;
            for (int k = 0; k < P; ++k) dl[k] = -du[k] / th[k];
        }
        lml = -sum;
    };

    for (int e = 0; e <= max_rounds && !cbo::mle_done(s); ++e) {
        double xt[cbo::kMleMaxParams], lml = 0.0, dl[cbo::kMleMaxParams];
        for (int k = 0; k < P; ++k) xt[k] = cbo::mle_point(s)[k];
        evaluate(cbo::mle_theta(s), lml, dl);
        if (e == nan_at) lml = NAN;
        cbo::mle_feed(s, lml, dl, max_rounds);
        bool moved = -s.f == lml;
        for (int k = 0; k < P; ++k) moved = moved && s.x[k] == xt[k];
        for (int k = 0; k < P; ++k) std::printf(k ? " %a" : "P %a", xt[k]);
        std::printf(" %a %d\n", lml, moved ? 1 : 0);
    }
    if (!cbo::mle_done(s)) return 3;                              // more evaluations than 1 + max_rounds
    for (int e = 0; e < extra_feeds; ++e) {
        double dl[cbo::kMleMaxParams];
        for (int k = 0; k < cbo::kMleMaxParams; ++k) dl[k] = 1.0 + e;
        cbo::mle_feed(s, 1e300, dl, max_rounds);
    }
    std::printf("E %d %d %a", s.status, s.rounds, -s.f);
    for (int k = 0; k < P; ++k) std::printf(" %a", s.th[k]);
    for (int k = 0; k < P; ++k) std::printf(" %a", s.dl[k]);
    for (int k = 0; k < P; ++k) std::printf(" %a", s.x[k]);
    std::printf("\n");
    return 0;
}
