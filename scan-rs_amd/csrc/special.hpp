// Special functions of the sSeq differential-expression tests (diff-exp/src/dist.rs), written once for host and device:
// the same source runs in the kernels of sseq.hip and behind the scanrs_host_* entry points the CPU test-suite checks.
//
//   lgamma_pos      ln Γ(z), z > 0: Stirling's series (8 terms) at z >= 15, the recurrence Γ(z+1) = z Γ(z) below
//   log_beta_pf     ln[x^a y^b / B(a, b)], y = 1 - x, without the cancellation of three large ln Γ values: for a, b >= 15
//                   the Stirling form a ln(x/x0) + b ln(y/y0) + ½ ln(ab/(2π(a+b))) - (δ(a)+δ(b)-δ(a+b)), x0 = a/(a+b);
//                   for one large and one small parameter the large pair's ln Γ difference from the same series
//   betainc         regularised incomplete beta I_x(a, b): continued fraction (modified Lentz) on the side of the mean
//                   where it converges, the symmetry I_x(a,b) = 1 - I_{1-x}(b,a) on the other
//   betaincinv      x with I_x(a, b) = p: Newton steps on the density, kept inside a shrinking bracket (bisection when a
//                   step would leave it; geometric halving while the lower end is still 0)
//   nb_term         ln of one term of the exact test's conditional distribution (dist.rs:259-310, written per term)
//   nb_asymptotic   the beta approximation of the exact test (dist.rs:226-257)
//
// α = sf_a μ/(1+φμ) reaches 10^5 - 10^6 on the rest side of a one-vs-rest test, so large parameters are the normal case.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCANRS_HD __host__ __device__
#else
#define SCANRS_HD
#endif

namespace scanrs {
namespace special {

constexpr double LN_SQRT_2PI = 0.91893853320467274178; // ½ ln 2π
constexpr double STIRLING_MIN = 15.0;

// δ(z) = ln Γ(z) - [(z - ½) ln z - z + ½ ln 2π], z >= 15 (the series' next term is below 1e-20 there)
SCANRS_HD inline double stirling_tail(double z) {
    const double t = 1.0 / (z * z);
    double s = -3617.0 / 122400.0;
    s = s * t + 1.0 / 156.0;
    s = s * t - 691.0 / 360360.0;
    s = s * t + 1.0 / 1188.0;
    s = s * t - 1.0 / 1680.0;
    s = s * t + 1.0 / 1260.0;
    s = s * t - 1.0 / 360.0;
    s = s * t + 1.0 / 12.0;
    return s / z;
}

SCANRS_HD inline double lgamma_pos(double z) {
    if (!(z > 0.0)) return z == 0.0 ? INFINITY : NAN;
    if (z >= STIRLING_MIN) return (z - 0.5) * log(z) - z + LN_SQRT_2PI + stirling_tail(z);
    // raise the argument to >= 15: ln Γ(z) = ln Γ(z + m) - ln[z (z+1) ... (z+m-1)]
    double prod = 1.0, w = z;
    while (w < STIRLING_MIN) {
        prod *= w;
        w += 1.0;
    }
    return (w - 0.5) * log(w) - w + LN_SQRT_2PI + stirling_tail(w) - log(prod);
}

// ln Γ(y) - ln Γ(y + s) for y >= 15, s > 0
SCANRS_HD inline double lgamma_diff_large(double y, double s) {
    return -(y - 0.5) * log1p(s / y) - s * log(y + s) + s + stirling_tail(y) - stirling_tail(y + s);
}

SCANRS_HD inline double log_beta(double a, double b) {
    const double lo = a < b ? a : b, hi = a < b ? b : a;
    if (hi < STIRLING_MIN) return lgamma_pos(a) + lgamma_pos(b) - lgamma_pos(a + b);
    if (lo < STIRLING_MIN) return lgamma_pos(lo) + lgamma_diff_large(hi, lo);
    const double ab = a + b;
    return -a * log1p(b / a) - b * log1p(a / b) + 0.5 * log(ab / (a * b)) + LN_SQRT_2PI + stirling_tail(a) + stirling_tail(b) -
           stirling_tail(ab);
}

// ln[x^a y^b / B(a, b)] with y = 1 - x given separately (no rounding of 1 - x near 1)
SCANRS_HD inline double log_beta_pf(double a, double b, double x, double y) {
    if (a >= STIRLING_MIN && b >= STIRLING_MIN) {
        const double ab = a + b;
        // a ln(x/x0) + b ln(y/y0): (x - x0)/x0 = (x (a+b) - a)/a
        const double u = fma(x, ab, -a) / a, v = fma(y, ab, -b) / b;
        return a * log1p(u) + b * log1p(v) + 0.5 * log(a * b / ab) - LN_SQRT_2PI - (stirling_tail(a) + stirling_tail(b) - stirling_tail(ab));
    }
    return a * log(x) + b * log(y) - log_beta(a, b);
}

// continued fraction of I_x(a, b) (modified Lentz)
SCANRS_HD inline double betacf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 1e-16;
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 200000; m++) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d;
        if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) < eps) break;
    }
    return h;
}

SCANRS_HD inline double betainc(double a, double b, double x) {
    if (!(x > 0.0)) return 0.0;
    if (!(x < 1.0)) return 1.0;
    const double y = 1.0 - x;
    if (x * (a + b + 2.0) < a + 1.0) return exp(log_beta_pf(a, b, x, y)) * betacf(a, b, x) / a;
    return 1.0 - exp(log_beta_pf(a, b, x, y)) * betacf(b, a, y) / b;
}

SCANRS_HD inline double betaincinv(double a, double b, double p) {
    if (!(p > 0.0)) return 0.0;
    if (!(p < 1.0)) return 1.0;
    double lo = 0.0, hi = 1.0;
    double x = (a >= 1.0 && b >= 1.0) ? (a - 1.0 / 3.0) / (a + b - 2.0 / 3.0) : a / (a + b);
    if (!(x > 0.0 && x < 1.0)) x = 0.5;
    for (int it = 0; it < 400; it++) {
        const double f = betainc(a, b, x) - p;
        if (f == 0.0) return x;
        if (f < 0.0)
            lo = x;
        else
            hi = x;
        // density x^(a-1) (1-x)^(b-1) / B(a, b)
        const double dens = exp(log_beta_pf(a, b, x, 1.0 - x)) / (x * (1.0 - x));
        double xn = x - f / dens;
        if (!(xn > lo && xn < hi)) xn = lo > 0.0 ? 0.5 * (lo + hi) : hi * 0.0625;
        if (fabs(xn - x) <= 1e-15 * x) return xn;
        if (hi - lo <= 1e-16 * hi) return xn;
        x = xn;
    }
    return x;
}

// ln of term k of the exact test's distribution of x_a given x_a + x_b = n (dist.rs:259-310 per term: the reference's running
// recurrence written directly, so that every term - the observed one included - is the same function of its own k)
SCANRS_HD inline double nb_term(uint64_t k, uint64_t n, double sar, double sbr, double add_total) {
    const double kk = (double)k, jj = (double)(n - k);
    return lgamma_pos(sar + kk) + lgamma_pos(sbr + jj) - lgamma_pos(kk + 1.0) - lgamma_pos(jj + 1.0) + add_total;
}
// the constant of log_prob_all (dist.rs:264), literal: (sa + sb) ln(r/(r+μ)) as the reference writes it
SCANRS_HD inline double nb_add_total(uint64_t n, double sa, double sb, double mu, double r) {
    return (double)n * log(mu / (r + mu)) + (sa + sb) * log(r / (r + mu)) - lgamma_pos(sa * r) - lgamma_pos(sb * r);
}

// dist.rs:226-257
SCANRS_HD inline double nb_asymptotic(uint64_t count_a, uint64_t count_b, double sf_a, double sf_b, double mu, double phi) {
    const double alpha = sf_a * mu / (1.0 + phi * mu);
    const double beta = (sf_b / sf_a) * alpha;
    const double xa = (double)count_a, xb = (double)count_b;
    const double median = betaincinv(alpha, beta, 0.5);
    const double qa = (xa + 0.5) / (xa + xb);
    if (qa < median) return 2.0 * (qa < 0.0 ? 0.0 : qa > 1.0 ? 1.0 : betainc(alpha, beta, qa));
    const double qb = (xb + 0.5) / (xa + xb);
    return 2.0 * (qb < 0.0 ? 0.0 : qb > 1.0 ? 1.0 : betainc(beta, alpha, qb));
}

} // namespace special
} // namespace scanrs
