// The arithmetic of hclust that the device chain (hclust.hip) and its host twin (hclust_host.cpp) must share operation for operation:
// the squared Euclidean distance of two observations (hclust/src/lib.rs:19-23), the Lance-Williams update of the five reducible
// methods, and the order in which a row scan prefers its candidates. One header, compiled for both sides with contraction off, so
// that the two give the same bits.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define SCANRS_HD __host__ __device__
#else
#define SCANRS_HD
#endif

// no fused multiply-add anywhere below (Rust does not fuse; a fused sum would move heights off the reference's distance set)
#pragma clang fp contract(off)

namespace scanrs {

// kodama::Method's order (scanrs_amd.h: SCANRS_LINKAGE_*)
enum : int { HC_SINGLE = 0, HC_COMPLETE = 1, HC_AVERAGE = 2, HC_WEIGHTED = 3, HC_WARD = 4, HC_CENTROID = 5, HC_MEDIAN = 6 };

// Σ_k (b_k - a_k)², k in order, multiply and add rounded separately
SCANRS_HD inline double hclust_sqdist(const double *a, const double *b, uint32_t d) {
    double s = 0.0;
    for (uint32_t k = 0; k < d; k++) {
        const double t = b[k] - a[k];
        const double q = t * t;
        s = s + q;
    }
    return s;
}

// Clusters a and b (sizes na, nb, dissimilarity dab) become one; dka, dkb are cluster k's (size nk) dissimilarities to them.
// Ward's values are SQUARED distances (its stored matrix is the squared one; the square root is taken of the finished heights).
SCANRS_HD inline double hclust_lw(int method, double dka, double dkb, double dab, double na, double nb, double nk) {
    switch (method) {
    case HC_SINGLE:
        return dkb < dka ? dkb : dka;
    case HC_COMPLETE:
        return dkb > dka ? dkb : dka;
    case HC_AVERAGE: {
        const double p = na * dka, q = nb * dkb;
        return (p + q) / (na + nb);
    }
    case HC_WEIGHTED: {
        const double p = 0.5 * dka, q = 0.5 * dkb;
        return p + q;
    }
    default: { // HC_WARD
        const double p = (na + nk) * dka, q = (nb + nk) * dkb, r = nk * dab;
        return ((p + q) - r) / ((na + nb) + nk);
    }
    }
}

// the order of a row scan's candidates: the smaller dissimilarity, then the smaller index (the chain's previous element is
// preferred over both by the caller when it attains the minimum)
SCANRS_HD inline bool hclust_better(double v, uint32_t c, double best, uint32_t best_c) { return v < best || (v == best && c < best_c); }

} // namespace scanrs
