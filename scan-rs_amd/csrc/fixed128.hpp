// 128-bit fixed-point sums of doubles, written once for host and device (sseq.hip, cluster.hip, sseq_host.cpp, cluster_host.cpp).
//
// A term t is rounded once to a quantum of 2^-E (scale = 2^E, chosen per sum from a bound of the sums so that every sum stays
// below 2^124) and held as two u64 words. Integer sums are exact and associative: the result depends neither on the order in
// which the terms arrive nor on how they were grouped, and sums of two groups can be added later without any rounding.
// The quantum is absolute: a sum far below the bound it was chosen from keeps few bits of its own. Who shares one quantum among
// many sums has to know how small a term of theirs can be (fixed_single_quantum_keeps), or give every sum its own (fixed_term_class).
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SCANRS_FX_HD __host__ __device__
#else
#define SCANRS_FX_HD
#endif

namespace scanrs {

struct U128 {
    unsigned long long lo, hi;
};
SCANRS_FX_HD inline U128 to_fixed(double t, double scale) {
    const double y = t * scale; // scale is a power of two: exact
    const double hd = floor(y * 5.421010862427522e-20); // 2^-64
    const double ld = rint(y - hd * 18446744073709551616.0); // exact difference; < 2^64, rounded only below 2^53
    return U128{(unsigned long long)ld, (unsigned long long)hd};
}
SCANRS_FX_HD inline void add128(U128 &a, U128 b) {
    a.lo += b.lo;
    a.hi += b.hi + (a.lo < b.lo ? 1ull : 0ull);
}
// a power of two with bound * scale < 2^124 (sums of up to 2^124 fit the 128-bit accumulators with room for the rounding)
inline double fixed_scale(double bound) {
    if (!(bound > 0.0) || !std::isfinite(bound)) return 1.0;
    return std::ldexp(1.0, 124 - std::ilogb(bound) - 1);
}
SCANRS_FX_HD inline double from_fixed(const unsigned long long *w, double scale) {
    return ((double)w[1] * 18446744073709551616.0 + (double)w[0]) / scale;
}

// ---- how much of a term one quantum keeps (the moments of compute_sseq_params: sseq_host.cpp, sseq.hip) -------------------------
// Rounding a term t to the quantum 1/scale loses at most half a quantum, so a sum of terms that are all >= tmin comes back within
// 1 / (2 tmin scale) of its own size. The single-quantum pass is taken when the smallest term any sum can hold keeps FX_KEEP_BITS_1
// bits in Σ t (2^-41 = 4.5e-13 of every sum, under the 1e-12 asked of means) and FX_KEEP_BITS_2 bits in Σ t² (2^-34 = 5.8e-11 of every
// sum, under the 1e-10 asked of E[X²]); these are col_moments_plan.hpp's two numbers. Otherwise every sum gets a quantum of its own.
constexpr int FX_KEEP_BITS_1 = 40, FX_KEEP_BITS_2 = 33;
SCANRS_FX_HD inline bool fixed_single_quantum_keeps(double tmin, double scale1, double scale2) {
    return tmin * scale1 >= 1099511627776.0 /* 2^FX_KEEP_BITS_1 */ && tmin * tmin * scale2 >= 8589934592.0 /* 2^FX_KEEP_BITS_2 */;
}
// the grouped sums of sseq_de_pairs and merge_clusters: terms x / u_c <= 1 and their squares under one scale, the smallest possible term
// a count of 1 in the cell of the largest total
SCANRS_FX_HD inline bool fixed_totals_quantum_keeps(unsigned long long largest_total, double scale) {
    return largest_total == 0ull || fixed_single_quantum_keeps(1.0 / (double)largest_total, scale, scale);
}
// The per-sum quantum: the CLASS of a sum is 1 + FX_CLASS_CLAMP + the binary exponent of its largest term, clamped to +-FX_CLASS_CLAMP
// (0: the sum has no positive term). It is a maximum of integers: it depends neither on the order of the terms nor on how they were
// split over copies or shards. With at most 2^log2m terms below 2^(e + 1) the sum stays below 2^123 under the scale 2^(122 - log2m - e),
// and as the sum is at least its largest term, 2^e, rounding m terms moves it by less than 2^(2 log2m - 123) of itself; the squares'
// largest is below 2^(2e + 2) and at least 2^(2e). (Terms beyond 2^+-FX_CLASS_CLAMP are outside what the moments promise.)
constexpr int FX_CLASS_CLAMP = 440;
SCANRS_FX_HD inline unsigned fixed_term_class(double t) {
    if (!(t > 0.0)) return 0u;
    unsigned long long b;
    __builtin_memcpy(&b, &t, 8);
    int e = (int)((b >> 52) & 0x7FFull) - 1023; // a subnormal reads as -1023 and is clamped
    e = e < -FX_CLASS_CLAMP ? -FX_CLASS_CLAMP : e > FX_CLASS_CLAMP ? FX_CLASS_CLAMP : e;
    return (unsigned)(e + FX_CLASS_CLAMP + 1);
}
SCANRS_FX_HD inline double fixed_class_scale1(unsigned cls, int log2m) {
    return cls ? ldexp(1.0, 122 - log2m - ((int)cls - FX_CLASS_CLAMP - 1)) : 1.0;
}
SCANRS_FX_HD inline double fixed_class_scale2(unsigned cls, int log2m) {
    return cls ? ldexp(1.0, 121 - log2m - 2 * ((int)cls - FX_CLASS_CLAMP - 1)) : 1.0;
}
// the smallest L with m <= 2^L
inline int fixed_log2_ceil(unsigned long long m) {
    int l = 0;
    while (l < 64 && (1ull << l) < m) l++;
    return l;
}
// The signed form (subset.hip: the mapped values of the residual maps and of negative scale factors): the magnitude is rounded as
// to_fixed rounds it (rint is symmetric about zero) and a negative term is held as its two's complement, so that sums of mixed signs
// stay plain 128-bit additions (add128, shfl_down128, the limbs of an all-reduce). A sum below 2^127 in magnitude comes back with
// its sign.
SCANRS_FX_HD inline U128 to_fixed_signed(double t, double scale) {
    U128 v = to_fixed(fabs(t), scale);
    if (t < 0.0) {
        v.lo = ~v.lo + 1ull;
        v.hi = ~v.hi + (v.lo == 0ull ? 1ull : 0ull);
    }
    return v;
}
SCANRS_FX_HD inline double from_fixed_signed(const unsigned long long *w, double scale) {
    if (!(w[1] >> 63)) return from_fixed(w, scale);
    const unsigned long long n[2] = {~w[0] + 1ull, ~w[1] + (w[0] == 0ull ? 1ull : 0ull)};
    return -from_fixed(n, scale);
}

#if defined(__HIPCC__) || defined(__CUDACC__)
// p[0] = lo, p[1] = hi, in global memory or LDS; the carry of each addition is added by the lane that made it
__device__ __forceinline__ void atomic_add128(unsigned long long *p, U128 b) {
    const unsigned long long old = atomicAdd(p, b.lo);
    const unsigned long long carry = old + b.lo < old ? 1ull : 0ull;
    if (b.hi + carry) atomicAdd(p + 1, b.hi + carry);
}
__device__ __forceinline__ U128 shfl_down128(U128 v, int off) {
    return U128{(unsigned long long)__shfl_down((long long)v.lo, off), (unsigned long long)__shfl_down((long long)v.hi, off)};
}
#endif

} // namespace scanrs
