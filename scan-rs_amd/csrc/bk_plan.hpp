// bk_plan.hpp — which columns of svd_bk's projection take the dense route T' = (op(A) K) C and which are recomputed by a sparse
// product: host arithmetic only, no launch, no device call. The driver (solver.cpp, BkRun::make_plan) hands over max |C| per column
// of Q and acts on the answer; scanrs_host_bk_plan exposes the same function to the CPU test-suite, which holds it to its Python
// twin (tests/bk_reuse_ref.py, plan_rule) and to a table of literal cases (tests/test_bk_plan_cpu.py). DESIGN.md section 4c.
//
// T' = (op(A) K) C amplifies the rounding of op(A) K by |C|. Columns of Q whose coefficient column stays below the bound L
// ("reuse_cmax", 1e5) take the cheap dense route; the others — directions in which the Krylov blocks are numerically dependent —
// are recomputed directly as a (narrow) sparse product op(A) Q[:, direct]. What is held (tests/test_gpu_bk_reuse.py): every returned
// triplet has max |op(A) x_i - s_i y_i| <= sqrt(q) L 2^-53 s_1, L the bound finally used (1.1e-11 sqrt(q) s_1 at 1e5).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <vector>

#include "spmm_route.hpp"

namespace scanrs {

constexpr uint32_t BK_PASS_MAX = TL_LMAX; // widest repair pass: up to here it runs through the hybrid LDS-tile product, a wider one through the gather kernels at about twice the time
constexpr double BK_RAISE_MAX = 100.0;    // the bound is raised by at most two decades
constexpr uint32_t BK_COST_PASS = 128;    // columns of one sparse pass in the cost model of the last block

inline uint32_t bk_block_width(uint32_t k, double k_multiplier, uint64_t Mg, uint64_t Ng) {
    const uint32_t b = (uint32_t)std::ceil((double)k * k_multiplier); // bk_svd.rs:49
    return (uint32_t)std::min<uint64_t>(std::min(Mg, Ng), b);         // bk_svd.rs:81
}
// T' = H C needs the half-products in T beside the projected blocks: a second panel, for even block widths only
inline bool bk_reuse(uint32_t b) { return (b % 2u) == 0u; }
// blocks 1 .. n_iter-2: their coefficients are known before the end, so they are projected beside the sparse passes
inline uint32_t bk_early_blocks(uint32_t b, uint32_t n_iter) { return (bk_reuse(b) && n_iter >= 3) ? n_iter - 2 : 0; }

struct BkPlan {
    bool reuse = false;
    uint32_t flagged_older = 0; // the older blocks' columns at or above reuse_cmax, before any raise
    // 0 = no older column flagged, 1 = the flagged ones fit the repair pass, 2 = bound raised to the largest flagged, 3 = raised to
    // `need`, 4 = bound unchanged and a pass wider than BK_PASS_MAX columns
    int limit_branch = 0;
    double limit = 0.0;           // the bound finally used
    std::vector<uint32_t> direct; // recomputed by the sparse product, in the order the repair pass carries them: the older flagged columns ascending, then the whole last block when last_direct
    bool last_direct = false;     // the last block has no half-product: all of it rides in the repair pass
    bool full_direct = false;     // no dense route at all: one q-wide product op(A) Q
    uint32_t n_early = 0;
    double cmax_dense = 0.0;      // the largest max|C| among the columns that take the dense route (0 when full_direct)
};

// colmax[q]: max |C| per column of Q, q = b n_iter (read only when the bookkeeping is used: even b and coef_valid).
// coef_valid = no panel was completed with random directions, which would void Q = K C: then everything is computed directly.
inline BkPlan bk_plan(const double *colmax, uint32_t b, uint32_t n_iter, double reuse_cmax, bool coef_valid) {
    BkPlan p;
    const uint32_t q = b * n_iter, last_lo = (n_iter - 1) * b;
    p.reuse = bk_reuse(b);
    p.n_early = bk_early_blocks(b, n_iter);
    p.limit = reuse_cmax;
    if (p.reuse && !coef_valid)
        for (uint32_t j = 0; j < q; j++) p.direct.push_back(j); // one q-wide product: full_direct below
    if (p.reuse && coef_valid) {
        // The repair pass carries the last block (b columns) plus the flagged columns of the older blocks. When a few flagged columns
        // too many stand in the way of a pass of BK_PASS_MAX columns (22 on the 1 M-cell benchmark), the bound is raised — by at most
        // two decades: the same residual bound with the raised L, at most 1.1e-9 sqrt(q) s_1 — until the pass fits.
        // The rule looks at b and the coefficients only — not at whether this handle (or this shard) happens to run the hybrid product:
        // the flagged set, and with it the rounding of the result, is the same on every rank of a sharded run and under any memory
        // pressure.
        std::vector<double> flagged;
        for (uint32_t j = 0; j < last_lo; j++)
            if (!(colmax[j] < p.limit)) flagged.push_back(colmax[j]);
        p.flagged_older = (uint32_t)flagged.size();
        p.limit_branch = flagged.empty() ? 0 : 4; // 4 unless the flagged columns fit or one of the two raises applies
        if (n_iter >= 2 && b <= BK_PASS_MAX) {
            const uint32_t room = BK_PASS_MAX - b;
            if (flagged.size() > room) {
                std::sort(flagged.begin(), flagged.end(), std::greater<double>());
                const double need = flagged[room]; // the largest coefficient that has to take the dense route
                if (flagged[0] < BK_RAISE_MAX * p.limit) { // all of them within the two decades: the pass carries the last block alone (100 columns run 9 % faster than 104)
                    p.limit = std::nextafter(flagged[0], INFINITY);
                    p.limit_branch = 2;
                } else if (need < BK_RAISE_MAX * p.limit && (room == 0 || flagged[room - 1] > need)) {
                    p.limit = std::nextafter(need, INFINITY);
                    p.limit_branch = 3;
                }
            } else if (!flagged.empty()) {
                p.limit_branch = 1;
            }
        }
        for (uint32_t j = 0; j < last_lo; j++)
            if (!(colmax[j] < p.limit)) p.direct.push_back(j);
        // The last Krylov block: its half-product op(A) K_{n-1} exists only to feed T'_{n-1}. Computing ALL of it directly, in the
        // same sparse pass as the older flagged columns, never costs more passes of BK_COST_PASS columns than the half-product plus
        // the repair pass: with c(x) = ceil(x / BK_COST_PASS), `older` flagged columns and `all` flagged ones (all >= older),
        // c(b + older) <= c(b) + c(older) <= c(b) + c(all), because c is subadditive. So the comparison of the two costs always
        // comes out in favour of the direct block, and only n_iter == 1 (no older block: K_0 has no half-product yet) keeps it.
        p.last_direct = n_iter >= 2;
        for (uint32_t j = last_lo; j < q; j++)
            if (p.last_direct || !(colmax[j] < p.limit)) p.direct.push_back(j);
    }
    p.full_direct = !(p.reuse && (p.direct.size() * 2 < q || p.last_direct));
    if (!p.full_direct) {
        std::vector<char> is_direct(q, 0);
        for (uint32_t j : p.direct) is_direct[j] = 1;
        for (uint32_t j = 0; j < q; j++)
            if (!is_direct[j]) p.cmax_dense = std::max(p.cmax_dense, colmax[j]);
    }
    return p;
}

// the decisions of a run as the counters "bk_*" give them (q, b and early_projections are the driver's own)
inline void bk_record(Storage::BkDecisions &d, const BkPlan &p, bool coef_valid) {
    d.coef_valid = coef_valid;
    d.flagged_older = p.flagged_older;
    d.limit_branch = (uint64_t)p.limit_branch;
    d.limit = p.limit;
    d.direct_columns = p.direct.size();
    d.last_direct = p.last_direct;
    d.full_direct = p.full_direct;
    d.cmax_dense = p.cmax_dense;
}

// SCANRS_TRACE=1, when the bookkeeping is used: the flagged columns per block and per decade, and the route of the last block
inline void bk_plan_trace(const double *colmax, uint32_t b, uint32_t n_iter, const BkPlan &p) {
    const uint32_t q = b * n_iter;
    size_t flagged = 0; // at the bound finally used, the last block counted by its own columns
    for (uint32_t j = 0; j < q; j++) flagged += !(colmax[j] < p.limit);
    fprintf(stderr, "[scanrs trace] bk: %zu of %u projection columns recomputed directly\n", flagged, q);
    for (uint32_t blk = 0; blk < n_iter; blk++) {
        int cnt = 0;
        for (uint32_t j = blk * b; j < (blk + 1) * b; j++) cnt += !(colmax[j] < p.limit);
        fprintf(stderr, "[scanrs trace] bk:   block %u: %d\n", blk, cnt);
    }
    for (double thr : {1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e9, 1e10}) {
        int cnt = 0;
        for (uint32_t j = 0; j < q; j++) cnt += !(colmax[j] < thr);
        fprintf(stderr, "[scanrs trace] bk:   columns with max|C| >= %.0e: %d\n", thr, cnt);
    }
    fprintf(stderr, "[scanrs trace] bk: last block %s\n", p.last_direct ? "computed directly with the repair pass" : "through its half-product");
}

} // namespace scanrs
