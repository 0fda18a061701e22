// 128-bit fixed-point sums of doubles, written once for host and device (sseq.hip, cluster.hip, sseq_host.cpp, cluster_host.cpp).
//
// A term t is rounded once to a quantum of 2^-E (scale = 2^E, chosen per sum from a bound of the sums so that every sum stays
// below 2^124) and held as two u64 words. Integer sums are exact and associative: the result depends neither on the order in
// which the terms arrive nor on how they were grouped, and sums of two groups can be added later without any rounding.
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
