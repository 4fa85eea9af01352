// Host simulator of csrc/hmc_chain.h for tests/test_hmc_sets_host.py: one HMC chain of the state machine, driven with a
// closed-form likelihood this program evaluates itself -- a quadratic in theta,
//   lml(theta) = -sum_k ((a_k theta_k) theta_k / 2 + b_k theta_k)   (summed from 0 in index order),
//   d lml / d theta_k = -(a_k theta_k + b_k),
// or NaN at evaluation number nan_at (counted from 0; -1: never).  Every number is exchanged as a hexadecimal float.
// stdin:  P num_samples hmc_iters nan_at start_is_x / stepsize / start (P) / a (P) / b (P) / momenta (num_samples x P) /
//         uniforms.  start: theta0 (start_is_x = 0: the chain transforms it itself) or the position x0 (1).
// stdout: "X <e> <x_0> .. <x_{P-1}>"     the position of evaluation e, in the order of the evaluations
//         "S <i> <accept> <row_0> ..."   sample i's flag and row, once the chain is done
//         "F <evals> <theta ...> <lml> <dlml ...>"   the chain's last state
// Build: g++ -O1 -std=c++17 -ffp-contract=off -Iinclude -Icbo_with_oop_amd/csrc tests/support/hmc_chain_sim.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "hmc_chain.h"

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
    int P = 0, num_samples = 0, hmc_iters = 0, nan_at = -1, start_is_x = 0;
    if (std::scanf("%d %d %d %d %d", &P, &num_samples, &hmc_iters, &nan_at, &start_is_x) != 5) return 2;
    if (P < 1 || P > cbo::kHmcMaxParams || num_samples < 1 || hmc_iters < 0) return 2;
    double stepsize = 0.0;
    std::vector<double> theta0, a, b, momenta, uniforms;
    if (!read_hex(stepsize) || !read_hexes(theta0, (size_t)P) || !read_hexes(a, (size_t)P) || !read_hexes(b, (size_t)P) ||
        !read_hexes(momenta, (size_t)num_samples * (size_t)P) || !read_hexes(uniforms, (size_t)num_samples))
        return 2;
    std::vector<double> rows((size_t)num_samples * (size_t)P, 0.0);
    std::vector<int> accepts((size_t)num_samples, -1);

    cbo::HmcChain c;
    if (start_is_x) cbo::hmc_begin_at(c, P, theta0.data(), num_samples, hmc_iters, stepsize);
    else cbo::hmc_begin(c, P, theta0.data(), num_samples, hmc_iters, stepsize);
    const long long positions = 1 + (long long)num_samples * hmc_iters;
    long long e = 0;
    for (; e < positions && !cbo::hmc_done(c); ++e) {
        const double *th = cbo::hmc_theta(c);
        std::printf("X %lld", e);
        for (int k = 0; k < P; ++k) std::printf(" %a", c.x[k]);
        std::printf("\n");
        double lml = 0.0, dl[cbo::kHmcMaxParams];
        for (int k = 0; k < P; ++k) {
            lml = lml + ((a[(size_t)k] * th[k]) * th[k] / 2.0 + b[(size_t)k] * th[k]);
            dl[k] = -(a[(size_t)k] * th[k] + b[(size_t)k]);
        }
        lml = -lml;
        if (e == nan_at) lml = NAN;
        cbo::hmc_feed(c, lml, dl, momenta.data(), uniforms.data(), rows.data(), accepts.data());
    }
    if (!cbo::hmc_done(c)) return 3;                              // more positions than 1 + num_samples * hmc_iters
    for (int i = 0; i < num_samples; ++i) {
        std::printf("S %d %d", i, accepts[(size_t)i]);
        for (int k = 0; k < P; ++k) std::printf(" %a", rows[(size_t)i * (size_t)P + (size_t)k]);
        std::printf("\n");
    }
    std::printf("F %d", c.evals);
    for (int k = 0; k < P; ++k) std::printf(" %a", c.th[k]);
    std::printf(" %a", -c.f);
    for (int k = 0; k < P; ++k) std::printf(" %a", c.dl[k]);
    std::printf("\n");
    return 0;
}
