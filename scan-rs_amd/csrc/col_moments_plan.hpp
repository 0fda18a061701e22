// The plan of col_moments_kernel (normalize_ops.hip) as plain host arithmetic: from the numbers the device hands back (the largest
// count, per ScaleAxis link its smallest positive and its largest factor) to "take the fixed-point route or not" and the two
// binary exponents of its quanta. normalize_ops.hip calls it with what max_u32_kernel / minmax_nonneg_kernel found;
// scanrs_host_col_moments_plan exposes it to the CPU test-suite, which holds it to an exact emulation of the accumulation.
//
// The kernel adds rint(v 2^e1) (and rint(v^2 2^e2)) as 64-bit integers per inner position, so every term is off by at most
// q/2, q = 2^-e: an ABSOLUTE error per term. A slice's sum is at least (its number of terms) x (the smallest term any slice
// can hold), so its relative error is at most q / (2 v_min) — and nothing better can be said from global numbers: a slice
// made of the smallest terms only is as far from the largest value as the map allows. The plan therefore takes
//   x     = the chain applied to the largest count under every link's largest factor   (no term is larger)
//   v_min = the chain applied to count 1 under every link's smallest POSITIVE factor   (no term other than an exact 0 is smaller;
//           a zero factor in front of the logarithm gives terms that are exactly 0 and are added exactly)
// chooses e1 / e2 as large as the accumulators allow for x, and accepts when
//   v_min 2^e1 >= 2^40      (sum of f:   relative error of every slice <= 2^-41 = 4.6e-13)
//   v_min^2 2^e2 >= 2^33    (sum of f^2: relative error of every slice <= 2^-34 = 5.9e-11; mode 2 only)
// Together with the f64 evaluation of the terms and the addition of at most 256 workgroup sums in double (< 3e-14) this keeps
// sum and mean within 1e-12 relative and the variance within 1e-10 S2/m of the exact values, for every slice: the contract of
// tests/test_gpu_moments.py. Everything else goes to the ordinary pass.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>

namespace scanrs {
namespace col_moments {

// kinds as in common.hpp (OP_SCALE_AXIS, OP_LN_1P, OP_LOG2_1P, OP_LOG10_1P); repeated here so that the header stands alone
enum { LINK_SCALE = 1, LINK_LN_1P = 2, LINK_LOG2_1P = 3, LINK_LOG10_1P = 4 };
constexpr double SLACK = 1.0001;  // covers the roundings of the bound's own arithmetic and of the device's logarithm (2 ulp)
constexpr int TERM_BITS = 50;     // x 2^e <= 2^50: the kernel's conversion (t + 2^52) needs t < 2^51
constexpr int SUM_BITS = 62;      // a workgroup's sum stays below 2^62
constexpr int KEEP1 = 40, KEEP2 = 33;

struct Link {
    int kind;
    int on_summed_axis; // ScaleAxis: the factors belong to the positions that are summed over (the copy's outer vectors)
    double fmin_pos;    // ScaleAxis: smallest factor > 0 (anything else when there is none: then fmax is 0)
    double fmax;        // ScaleAxis: largest factor; negative or not finite = the link holds such a factor
};
struct Plan {
    bool ok;
    int e1, e2;
};

// ceil(log2(y)) for finite y > 0, from the exponent (no rounding of a logarithm near a power of two)
inline int ceil_log2(double y) {
    int e;
    const double m = std::frexp(y, &e); // y = m 2^e, m in [0.5, 1)
    return m == 0.5 ? e - 1 : e;
}
// log(1 + x) as the map evaluates it (x + 1.0 is rounded first) and as it is mathematically: the larger / smaller of the two
// bounds what any evaluation gives
inline void log1p_both(int kind, double x, double &lo, double &hi) {
    double a, b;
    if (kind == LINK_LN_1P) {
        a = std::log(1.0 + x), b = std::log1p(x);
    } else if (kind == LINK_LOG2_1P) {
        a = std::log2(1.0 + x), b = std::log1p(x) * 1.4426950408889634074;
    } else {
        a = std::log10(1.0 + x), b = std::log1p(x) * 0.43429448190325182765;
    }
    lo = std::fmin(a, b);
    hi = std::fmax(a, b);
}

inline Plan plan(uint32_t max_count, const Link *links, int n_links, uint64_t n_outer, uint64_t n_inner, uint32_t n_wg, int mode) {
    Plan p = {false, 0, 0};
    if ((mode != 1 && mode != 2) || n_outer == 0 || n_inner == 0 || n_wg == 0 || n_links < 0 || (n_links && !links)) return p;
    if (n_outer >= (1ull << 40)) return p;
    bool has_log = false;
    double x = (double)(max_count ? max_count : 1u), v = 1.0;
    for (int i = 0; i < n_links; i++) {
        const Link &l = links[i];
        if (l.kind == LINK_SCALE) {
            if (!l.on_summed_axis) return p;
            if (!(l.fmax >= 0.0) || !std::isfinite(l.fmax)) return p; // a negative or non-finite factor
            if (l.fmax == 0.0) return p;                               // every term is 0: nothing to scale a quantum by
            if (!(l.fmin_pos > 0.0) || !(l.fmin_pos <= l.fmax)) return p;
            x *= l.fmax;
            v *= l.fmin_pos;
        } else if (l.kind == LINK_LN_1P || l.kind == LINK_LOG2_1P || l.kind == LINK_LOG10_1P) {
            has_log = true;
            double lo, hi;
            log1p_both(l.kind, x, lo, hi);
            x = hi;
            log1p_both(l.kind, v, lo, hi);
            v = lo;
        } else {
            return p;
        }
        if (!std::isfinite(x) || !(x > 0.0) || !(v > 0.0) || x < 1e-300 || v < 1e-300) return p;
    }
    if (!has_log) return p;
    const double cells = (double)((n_outer + n_wg - 1) / n_wg);
    const double xs = x * SLACK, xs2 = x * x * SLACK, vs = v / SLACK;
    if (!std::isfinite(xs2) || xs2 < 1e-300) return p;
    // a workgroup adds at most `cells` values of at most x (x^2): sums below 2^62, and every term at most 2^50
    const int e1 = std::min(SUM_BITS - ceil_log2(xs * cells), TERM_BITS - ceil_log2(xs));
    const int e2 = std::min(SUM_BITS - ceil_log2(xs2 * cells), TERM_BITS - ceil_log2(xs2));
    if (e1 > 1000 || e2 > 1000 || e1 < -1000 || e2 < -1000) return p;
    // the smallest term keeps 40 bits above the quantum (33 for the squares): see the head of this file
    if (!(std::ldexp(vs, e1) >= std::ldexp(1.0, KEEP1))) return p;
    if (mode == 2 && !(std::ldexp(vs * vs, e2) >= std::ldexp(1.0, KEEP2))) return p;
    p.ok = true;
    p.e1 = e1;
    p.e2 = e2;
    return p;
}

} // namespace col_moments
} // namespace scanrs
