/*! @file sx_cooling.cpp
 * @brief the host side of the radiative cooling (sx_cooling_*): the table of power-law segments with its exponents and
 *        Townsend's temporal evolution function, and the host evaluators of the arithmetic in sx_cool.hpp.  No kernels.
 */
#include "sx_cool.hpp"

#include <algorithm>

using namespace sx::cool;

namespace
{

Table tableOf(const sx_cooling* c)
{
    return Table{c->T.data(), c->lambda.data(), c->alpha.data(), c->Y.data(), (uint32_t)c->T.size()};
}

} // namespace

extern "C"
{

    int sx_cooling_create(sx_cooling** out, const double* T, const double* lambda, uint32_t n)
    {
        if (!out || !T || !lambda || n < 2 || n > kMaxNodes) return SX_ERR_ARG;
        for (uint32_t k = 0; k < n; ++k)
        {
            if (!std::isfinite(T[k]) || !std::isfinite(lambda[k]) || !(T[k] > 0.0) || !(lambda[k] > 0.0)) return SX_ERR_ARG;
            if (k && !(T[k] > T[k - 1])) return SX_ERR_ARG;
        }
        auto* c = new sx_cooling;
        c->T.assign(T, T + n);
        c->lambda.assign(lambda, lambda + n);
        c->alpha.resize(n);
        c->Y.resize(n);
        for (uint32_t k = 0; k + 1 < n; ++k)
            c->alpha[k] = std::log(lambda[k + 1] / lambda[k]) / std::log(T[k + 1] / T[k]);
        c->alpha[n - 1] = c->alpha[n - 2];
        const double norm = lambda[n - 1] / T[n - 1];
        c->Y[n - 1]       = 0.0;
        bool ok           = true;
        for (uint32_t k = n - 1; k-- > 0;)
        {
            const double ck = norm * (T[k] / lambda[k]);
            c->Y[k]         = c->Y[k + 1] + ck * segIntegral(c->alpha[k], std::log(T[k + 1] / T[k]));
            // a table whose Y does not resolve its nodes (an exponent or a ratio beyond double) cannot be searched
            ok = ok && std::isfinite(c->alpha[k]) && std::isfinite(c->Y[k]) && c->Y[k] > c->Y[k + 1];
        }
        if (!ok)
        {
            delete c;
            return SX_ERR_ARG;
        }
        *out = c;
        return SX_OK;
    }

    void sx_cooling_destroy(sx_cooling* c) { delete c; }

    uint32_t sx_cooling_num_nodes(const sx_cooling* c) { return c ? (uint32_t)c->T.size() : 0u; }

    int sx_cooling_get_table(const sx_cooling* c, double* T, double* lambda, double* alpha, double* Y)
    {
        if (!c) return SX_ERR_ARG;
        if (T) std::copy(c->T.begin(), c->T.end(), T);
        if (lambda) std::copy(c->lambda.begin(), c->lambda.end(), lambda);
        if (alpha) std::copy(c->alpha.begin(), c->alpha.end(), alpha);
        if (Y) std::copy(c->Y.begin(), c->Y.end(), Y);
        return SX_OK;
    }

    double sx_cooling_rate_host(const sx_cooling* c, double T) { return c ? rate(tableOf(c), T) : NAN; }

    double sx_cooling_integrate_host(const sx_cooling* c, double T0, double s)
    {
        return c ? integrate(tableOf(c), T0, s) : NAN;
    }

} // extern "C"
