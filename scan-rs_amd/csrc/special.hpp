// Special functions of the sSeq differential-expression tests (diff-exp/src/dist.rs), written once for host and device:
// the same source runs in the kernels of sseq.hip and behind the scanrs_host_* entry points the CPU test-suite checks.
//
//   lgamma_pos      ln Γ(z), z > 0: Stirling's series (8 terms) at z >= 15, the recurrence Γ(z+1) = z Γ(z) below
//   log_beta_pf     ln[x^a y^b / B(a, b)], y = 1 - x, without the cancellation of three large ln Γ values: for a, b >= 15
//                   the Stirling form a ln(x/x0) + b ln(y/y0) + ½ ln(ab/(2π(a+b))) - (δ(a)+δ(b)-δ(a+b)), x0 = a/(a+b), its two
//                   logarithms taken as log1p(u) - u of one shared numerator; for one large and one small parameter the large
//                   pair's ln Γ difference from the same series
//   betainc         regularised incomplete beta I_x(a, b): continued fraction (DiDonato & Morris, modified Lentz) on the side of
//                   the mean where it converges, the symmetry I_x(a,b) = 1 - I_{1-x}(b,a) on the other
//   betaincinv      x with I_x(a, b) = p: Newton steps on the density, kept inside a shrinking bracket (bisection when a
//                   step would leave it; geometric halving while the lower end is still 0)
//   lgamma_rise     ln Γ(y + k) - ln Γ(y) as one quantity, without the cancellation of two large ln Γ values
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

// log1p(z) - z, z > -1, without the cancellation at small z: with w = z/(2+z), log1p(z) = 2 atanh(w) and 2w - z = -z w, so
// log1p(z) - z = w (2 w^2 (1/3 + w^2/5 + w^4/7 + ...) - z); |w| <= 1/3 where the series is used
SCANRS_HD inline double log1pmx(double z) {
    if (fabs(z) > 0.5) return log1p(z) - z;
    const double w = z / (2.0 + z), w2 = w * w;
    double s = 0.0, p = 1.0;
    for (int k = 3; k < 45; k += 2) {
        const double t = p / k;
        s += t;
        if (t < 1e-17 * s) break;
        p *= w2;
    }
    return w * (2.0 * w2 * s - z);
}

// n = x (a+b) - a = -[y (a+b) - b], y = 1 - x: the distance of x from x0 = a/(a+b) in units of 1/(a+b), the one number through which
// the prefactor and the continued fraction see x near x0. It takes a + b as the exact pair ab + ab_lo and one rounding in the fma;
// formed from a rounded 1 - x or a rounded a + b it is off by (a+b) ulp, and ln of the prefactor with it.
SCANRS_HD inline double beta_excess(double a, double b, double x) {
    const double ab = a + b, t = ab - a, ab_lo = (a - (ab - t)) + (b - t);
    return fma(x, ab, -a) + x * ab_lo;
}

// ln[x^a y^b / B(a, b)], y = 1 - x, from x and n = beta_excess(a, b, x): every caller's x is the given number, its 1 - x the rounded one
SCANRS_HD inline double log_beta_pf(double a, double b, double x, double n) {
    if (a >= STIRLING_MIN && b >= STIRLING_MIN) {
        // a ln(x/x0) + b ln(y/y0): (x - x0)/x0 = n/a = u and (y - y0)/y0 = -n/b = v, so the first-order terms a u + b v cancel exactly
        // and a [log1p(u) - u] + b [log1p(v) - v] is left, two terms of one sign
        const double ab = a + b;
        const double u = n / a, v = -n / b;
        // far below x0 (or y0) the logarithm is taken of x/x0 (or y/y0; y is exact there, x > 1/2) itself: u rounds to -1 once x/x0 < 1e-16
        const double su = u > -0.5 ? log1pmx(u) : log(x * ab / a) - u;
        const double sv = v > -0.5 ? log1pmx(v) : log((1.0 - x) * ab / b) - v;
        return a * su + b * sv + 0.5 * log(a * b / ab) - LN_SQRT_2PI - (stirling_tail(a) + stirling_tail(b) - stirling_tail(ab));
    }
    // 1 - x is exact for x >= 1/2; below, log1p(-x) spares its rounding, which b multiplies
    return a * log(x) + b * (x < 0.5 ? log1p(-x) : log(1.0 - x)) - log_beta(a, b);
}

// I_x(a, b) = x^a y^b / B(a, b) / betacf: the continued fraction b_0 + a_1/(b_1 + a_2/(b_2 + ...)) of DiDonato & Morris (ACM TOMS 18, 1992),
// the even part of the classical fraction, by modified Lentz; n = beta_excess(a, b, x). The classical fraction's partial
// denominators 1 - (a+m)(a+b+m) x / ((a+2m)(a+2m+1)) each cancel to ~1/a next to x0, and its value (up to ~a for b << a) multiplies what
// they lose; here that difference is written out, a y - b x = -n, and no term cancels.
SCANRS_HD inline double betacf(double a, double b, double x, double n) {
    const double tiny = 1e-300, eps = 1e-16;
    double f = a * (1.0 - n) / (a + 1.0);
    if (fabs(f) < tiny) f = tiny;
    double c = f, d = 0.0;
    for (int m = 1; m <= 200000; m++) {
        const double den = a + 2.0 * m - 1.0;
        const double am = (a + m - 1.0) * (a + b + m - 1.0) * m * (b - m) * x * x / (den * den);
        const double bm = m + m * (b - m) * x / den + (a + m) * (1.0 - n + m * (2.0 - x)) / (den + 2.0);
        d = bm + am * d;
        if (fabs(d) < tiny) d = tiny;
        c = bm + am / c;
        if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = c * d;
        f *= del;
        if (fabs(del - 1.0) < eps) break;
    }
    return f;
}

SCANRS_HD inline double betainc(double a, double b, double x) {
    if (!(x > 0.0)) return 0.0;
    if (!(x < 1.0)) return 1.0;
    const double y = 1.0 - x, n = beta_excess(a, b, x);
    if (x * (a + b + 2.0) < a + 1.0) return exp(log_beta_pf(a, b, x, n)) / betacf(a, b, x, n);
    return 1.0 - exp(log_beta_pf(a, b, x, n)) / betacf(b, a, y, -n);
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
        const double dens = exp(log_beta_pf(a, b, x, beta_excess(a, b, x))) / (x * (1.0 - x));
        double xn = x - f / dens;
        // settled: before the bracket is asked, since a step that rounds to nothing leaves xn = x, which IS the bracket's end now and
        // not inside it; halving from there creeps back towards x and stops some ulp short of it
        if (fabs(xn - x) <= 1e-15 * x) return xn;
        if (!(xn > lo && xn < hi)) xn = lo > 0.0 ? 0.5 * (lo + hi) : hi * 0.0625;
        if (hi - lo <= 1e-16 * hi) return xn;
        x = xn;
    }
    return x;
}

// ln Γ(y + k) - ln Γ(y), y > 0, k = 0, 1, 2, ..., as one quantity: exactly 0 at k = 0. Below 15 the argument is raised, ln Γ(y + k) - ln Γ(y) =
// ln[y (y+1) ... (y+m-1)] + ln Γ(y + k) - ln Γ(y + m), and the product alone serves k <= m; from 15 on Stirling's series gives the difference
// (lgamma_diff_large). Two rounded ln Γ values of size y ln y would leave an ulp of THAT in a difference of size k ln y: at y = sf / φ = 2e8
// (the rest side of a one-vs-rest test) 4.8e-7 in the logarithm of every term, independently per term.
SCANRS_HD inline double lgamma_rise(double y, double k) {
    if (y >= STIRLING_MIN) return -lgamma_diff_large(y, k);
    double prod = 1.0;
    while (y < STIRLING_MIN && k > 0.0) {
        prod *= y;
        y += 1.0;
        k -= 1.0;
    }
    const double head = log(prod); // log(1.0) = 0 where nothing was raised
    return k > 0.0 ? head - lgamma_diff_large(y, k) : head;
}

// ln of term k of the exact test's distribution of x_a given x_a + x_b = n (dist.rs:259-310 per term: the reference's running
// recurrence written directly, so that every term - the observed one included - is the same function of its own k):
//   [ln Γ(sar + k) - ln Γ(sar) - ln k!] + [ln Γ(sbr + n-k) - ln Γ(sbr) - ln (n-k)!] + add_total
// Each side is one number of its own count; with sar == sbr the mirror term n - k adds the same two numbers in the other order and has the
// same bits, so `<=` against the observed term includes it. Nothing here is contracted: a fused multiply-add across the two sides would
// round one of them and not the other.
SCANRS_HD inline double nb_side(double sr, double count) { return lgamma_rise(sr, count) - lgamma_pos(count + 1.0); }
SCANRS_HD inline double nb_term(uint64_t k, uint64_t n, double sar, double sbr, double add_total) {
#pragma clang fp contract(off)
    const double a = nb_side(sar, (double)k), b = nb_side(sbr, (double)(n - k));
    return (a + b) + add_total;
}
// the constant of log_prob_all (dist.rs:264) without its two ln Γ(s r), which nb_term's differences hold: n ln(μ/(r+μ)) + (sa + sb) ln(r/(r+μ)),
// literal as the reference writes it
SCANRS_HD inline double nb_add_total(uint64_t n, double sa, double sb, double mu, double r) {
    return (double)n * log(mu / (r + mu)) + (sa + sb) * log(r / (r + mu));
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
