// Host logic of sSeq differential expression (diff-exp/src/diff_exp.rs, dist.rs, stat.rs): size factors, the parameters from
// the moments, the split of the tests between the exact and the asymptotic branch, BH, log2 fold change and normalized means.
// The passes over the nonzeros and the tests themselves run on the device (sseq.hip).
#include "common.hpp"
#include "fixed128.hpp"
#include "shard_exchange.hpp"
#include "special.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// the reference's host arithmetic is not contracted: fused multiply-adds here would move the parameters off its bits
#pragma clang fp contract(off)

namespace scanrs {

// ---- sharded handles ---------------------------------------------------------------------------------------------
// The cells are the sharded dimension: the copy holds the cells [begin, begin + n_local) of `global`, and every per-cell argument
// spans the whole matrix (cell_range). All sums that cross the shards are integers and go through the exchange steps of
// shard_exchange.hpp, counted in "de_shard_allreduces": they come out bit for bit as the sums of the unsharded handle, whatever the
// number of shards and whichever transport carries them.
static ShardExchange de_exchange(Storage &st) { return ShardExchange{st, st.de_shard_allreduces}; }
// the largest count of the whole matrix
static uint32_t sseq_max_count_global(Storage &st, const SparseCopy &cp) {
    const unsigned long long mine = sseq_max_count(st, cp);
    const std::vector<unsigned long long> all = de_exchange(st).gather_host(&mine, 1);
    return (uint32_t)*std::max_element(all.begin(), all.end());
}

// ---- stat.rs ----------------------------------------------------------------------------------------------------------------
// percentile_of_sorted (stat.rs:140-162): linear interpolation between the neighbouring ranks
static double percentile_of_sorted(const std::vector<double> &s, double pct) {
    if (s.empty()) fail(SCANRS_ERR_ARGUMENT, "percentile of an empty list");
    if (s.size() == 1) return s[0];
    if (pct == 100.0) return s.back();
    const double length = (double)(s.size() - 1);
    const double rank = (pct / 100.0) * length;
    const double l_rank = std::floor(rank);
    const double d = rank - l_rank;
    const size_t n = (size_t)l_rank;
    return s[n] + (s[n + 1] - s[n]) * d;
}
static double percentile(std::vector<double> v, double pct) {
    std::stable_sort(v.begin(), v.end(), [](double a, double b) { return a < b; });
    return percentile_of_sorted(v, pct);
}
// Statistics::sum (stat.rs:49-80): the partials of Shewchuk's exact summation, added up in order at the end
static double exact_sum(const std::vector<double> &v) {
    std::vector<double> partials;
    for (double x0 : v) {
        double x = x0;
        size_t j = 0;
        for (size_t i = 0; i < partials.size(); i++) {
            double y = partials[i];
            if (std::fabs(x) < std::fabs(y)) std::swap(x, y);
            const double hi = x + y;
            const double lo = y - (hi - x);
            if (lo != 0.0) partials[j++] = lo;
            x = hi;
        }
        if (j >= partials.size()) {
            partials.push_back(x);
        } else {
            partials[j] = x;
            partials.resize(j + 1);
        }
    }
    double s = 0.0;
    for (double p : partials) s += p;
    return s;
}

// ---- dist.rs (host forms; the device runs the same special.hpp) ----------------------------------------------------------------
double sseq_host_exact_test(uint64_t xa, uint64_t xb, double sf_a, double sf_b, double mu, double phi) {
    if (xa + xb == 0) return 1.0;
    if (phi == 0.0) return 1.0;
    if (sf_a == 0.0 || sf_b == 0.0) return 1.0;
    const uint64_t n = xa + xb;
    const double r = 1.0 / phi, sar = sf_a * r, sbr = sf_b * r;
    const double add = special::nb_add_total(n, sf_a, sf_b, mu, r);
    const double obs = special::nb_term(xa, n, sar, sbr, add);
    std::vector<double> t(n + 1);
    double max_all = -INFINITY, max_ext = -INFINITY;
    for (uint64_t k = 0; k <= n; k++) {
        t[k] = special::nb_term(k, n, sar, sbr, add);
        if (t[k] <= obs) max_ext = std::max(max_ext, t[k]);
        max_all = std::max(max_all, t[k]);
    }
    double sum_all = 0.0, sum_ext = 0.0;
    for (double x : t) {
        if (x <= obs) sum_ext += std::exp(x - max_ext);
        sum_all += std::exp(x - max_all);
    }
    return std::exp((std::log(sum_ext) + max_ext) - (std::log(sum_all) + max_all));
}

// nb_exact_ratio_step (dist.rs:124-126)
static inline double ratio_step(double k, double n, double sa_r, double sb_r) { return (sa_r + k) * (n - k) / ((k + 1.0) * (sb_r + n - k - 1.0)); }

// nb_exact_test_ratio (dist.rs:155-215), line for line
double sseq_host_exact_test_ratio(uint64_t xa, uint64_t xb, double sf_a, double sf_b, double mu, double phi) {
    if (xa + xb == 0) return 1.0;
    if (phi == 0.0) return 1.0;
    if (sf_a == 0.0 || sf_b == 0.0) return 1.0;
    const uint64_t n = xa + xb;
    const double nn = (double)n;
    const double r = 1.0 / phi;
    const double sa_r = sf_a * r, sb_r = sf_b * r;
    uint64_t mode = n;
    for (uint64_t k = 0; k < n; k++)
        if (ratio_step((double)k, nn, sa_r, sb_r) < 1.0) {
            mode = k;
            break;
        }
    std::vector<double> u(n + 1, 0.0);
    u[mode] = 1.0;
    for (uint64_t k = mode; k < n; k++) u[k + 1] = u[k] * ratio_step((double)k, nn, sa_r, sb_r);
    for (uint64_t k = mode; k-- > 0;) u[k] = u[k + 1] / ratio_step((double)k, nn, sa_r, sb_r);
    const double u_obs = u[xa];
    if (u_obs == 0.0 || !std::isfinite(u_obs)) return sseq_host_exact_test(xa, xb, sf_a, sf_b, mu, phi);
    // sa_r == sb_r: the terms k and n - k are equal in exact arithmetic, and the two sweeps round them apart. The mirror of the observed term
    // belongs to the extreme set whichever way that went (the reference leaves it to `<=` and drops it in some cases)
    const uint64_t mirror = sa_r == sb_r ? n - xa : xa;
    double sum_all = 0.0, sum_ext = 0.0;
    for (uint64_t k = 0; k <= n; k++) {
        sum_all += u[k];
        if (u[k] <= u_obs || k == mirror) sum_ext += u[k];
    }
    return sum_ext / sum_all;
}

// log_prob_all (dist.rs:259-310): the terms the exact test sums, from the same rounded sf r it passes to them
static void sseq_host_log_prob_all(uint64_t n, double sf_a, double sf_b, double mu, double r, double *out) {
    const double sar = sf_a * r, sbr = sf_b * r;
    const double add = special::nb_add_total(n, sf_a, sf_b, mu, r);
    for (uint64_t k = 0; k <= n; k++) out[k] = special::nb_term(k, n, sar, sbr, add);
}

// The anchor of nb_exact_test_ratio (dist.rs:178-184: the first k in 0 .. n-1 with step(k) < 1, else n) without the scan.
// step(k) < 1  <=>  (sa_r + k)(n - k) < (k + 1)(sb_r + n - k - 1)  <=>  n (sa_r - 1) - (sb_r - 1) < k (sa_r + sb_r - 2): the k^2 and
// k n terms cancel. With B = sa_r + sb_r - 2 > 0 the steps cross 1 once, downwards, behind k = A / B; with B <= 0 they are below
// 1 on a prefix of the range only, so the answer is 0 or n and the f64 predicate at k = 0 decides. For B > 0 the f64 predicate at
// the neighbours moves the closed form onto the reference's rounding. The anchor fixes the range of the terms, not the result.
uint64_t sseq_ratio_anchor(uint64_t n, double sa_r, double sb_r) {
    const double nn = (double)n;
    auto below = [&](uint64_t k) { return ratio_step((double)k, nn, sa_r, sb_r) < 1.0; };
    const double a = nn * (sa_r - 1.0) - (sb_r - 1.0), b = sa_r + sb_r - 2.0;
    if (!(b > 0.0)) return below(0) ? 0 : n;
    const double q = a / b;
    uint64_t k = !(q >= 0.0) ? 0 : q >= nn ? n : std::min<uint64_t>(n, (uint64_t)std::floor(q) + 1);
    for (int i = 0; i < 64 && k > 0 && below(k - 1); i++) k--;
    for (int i = 0; i < 64 && k < n && !below(k); i++) k++;
    return k;
}

// adjusted_pvalue_bh (dist.rs:22-50): descending, NaNs in front (stable), q = min(1, running min of p n/(n - rank))
void sseq_host_bh(const double *p, uint64_t n, double *out) {
    std::vector<uint64_t> ord(n);
    for (uint64_t i = 0; i < n; i++) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint64_t ia, uint64_t ib) {
        const double a = p[ia], b = p[ib];
        if (std::isnan(a) || std::isnan(b)) return std::isnan(a) && !std::isnan(b);
        return a > b;
    });
    const double len = (double)n;
    double mn = std::numeric_limits<double>::max();
    for (uint64_t idx = 0; idx < n; idx++) {
        double v = p[ord[idx]] * (len / (len - (double)idx));
        if (v < mn) mn = v;
        out[ord[idx]] = std::min(mn, 1.0);
    }
}

// ---- diff_exp.rs:377-456 ------------------------------------------------------------------------------------------------------
void sseq_params_from_moments(const double *mean_g, const double *var_g, uint64_t n, double sum_size_factors, double n_cells, double n_genes,
                              double zeta_quintile, uint8_t *use_genes, double *gene_moment_phi, double *zeta_hat, double *delta,
                              double *gene_phi) {
    std::vector<double> used;
    for (uint64_t i = 0; i < n; i++) {
        use_genes[i] = var_g[i] > 0.0;
        double res = 0.0;
        if (use_genes[i]) {
            res = std::max(0.0, (n_cells * var_g[i] - mean_g[i] * sum_size_factors) / (mean_g[i] * mean_g[i] * sum_size_factors));
            used.push_back(res);
        }
        gene_moment_phi[i] = res;
    }
    double zh = 0.0, dl = 0.0;
    if (!used.empty()) {
        zh = percentile(used, 100.0 * zeta_quintile);
        const double mean_phi = exact_sum(used) / (double)used.size();
        double a = 0.0, b = 0.0;
        for (double x : used) a += (x - mean_phi) * (x - mean_phi);
        for (double x : used) b += (x - zh) * (x - zh);
        dl = (a / (n_genes - 1.0)) / (b / (n_genes - 2.0));
    }
    bool cond = false;
    for (double x : used) cond = cond || x > 0.0;
    for (uint64_t i = 0; i < n; i++) gene_phi[i] = (cond && var_g[i] > 0.0) ? (1.0 - dl) * gene_moment_phi[i] + dl * zh : 0.0;
    *zeta_hat = zh;
    *delta = dl;
}

// ---- the group pass -------------------------------------------------------------------------------------------------------------
static void check_labels(const int16_t *labels, uint64_t cells, uint32_t n_groups) {
    if (n_groups == 0 || n_groups > SSEQ_MAX_GROUPS) fail(SCANRS_ERR_ARGUMENT, "n_groups must be in 1 .. %u", SSEQ_MAX_GROUPS);
    for (uint64_t c = 0; c < cells; c++)
        if (labels[c] < -1 || labels[c] >= (int)n_groups) fail(SCANRS_ERR_ARGUMENT, "label %d of cell %llu is outside -1 .. n_groups - 1", (int)labels[c], (unsigned long long)c);
}

void sseq_group_sums(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const int16_t *labels,
                     uint32_t n_groups, uint64_t *sums, uint64_t *cells_per_group) {
    const CellRange cr = cell_range(st, cells); // labels: one per cell of the whole matrix; the device gets this rank's slice
    check_labels(labels, cr.global, n_groups);
    int16_t *d_lab = st.scratch.get<int16_t>("sseq_labels", std::max<uint64_t>(1, cr.n_local));
    unsigned long long *d_sums = st.scratch.get<unsigned long long>("sseq_sums", std::max<uint64_t>(1, genes * n_groups));
    h2d(d_lab, labels + cr.begin, cr.n_local, st.stream);
    launch_sseq_group_pass(st, cp, gene_major, genes, d_lab, n_groups, d_sums, nullptr, 1.0, 1.0, nullptr, nullptr);
    if (genes) { // (the genes are not sharded: none on one rank is none on every rank, and then no step)
        de_exchange(st).sum(d_sums, genes * n_groups);
        SCANRS_D2H(sums, d_sums, genes * n_groups * 8, st.stream);
    }
    SCANRS_SYNC(st.stream);
    if (cells_per_group) {
        std::fill(cells_per_group, cells_per_group + n_groups, 0);
        for (uint64_t c = 0; c < cr.global; c++)
            if (labels[c] >= 0) cells_per_group[labels[c]]++;
    }
}

// ---- compute_sseq_params (diff_exp.rs:458-500) ----------------------------------------------------------------------------------
void sseq_params(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, double zeta_quintile,
                 const uint64_t *cell_indices, uint64_t n_sel, const double *umi_counts, double *size_factors, double *gene_means,
                 double *gene_variances, uint8_t *use_genes, double *gene_moment_phi, double *zeta_hat, double *delta, double *gene_phi) {
    // sharded: `cells` from here on is the whole matrix (cell_indices, umi_counts and size_factors span it); the host folds below run
    // replicated over the global arrays in cell order, the device gets the slice [cr.begin, cr.begin + cr.n_local)
    const CellRange cr = cell_range(st, cells);
    cells = cr.global;
    if (cell_indices)
        for (uint64_t i = 0; i < n_sel; i++)
            if (cell_indices[i] >= cells) fail(SCANRS_ERR_ARGUMENT, "cell index %llu out of range", (unsigned long long)cell_indices[i]);
    const uint64_t m = cell_indices ? n_sel : cells;
    if (m == 0) fail(SCANRS_ERR_ARGUMENT, "no cells");
    // size_factors (diff_exp.rs:314-332): per-cell totals (or umi_counts, one per selected cell) over their interpolated median
    std::vector<double> counts(m);
    if (umi_counts) {
        for (uint64_t i = 0; i < m; i++) counts[i] = umi_counts[i];
    } else {
        unsigned long long *d_tot = st.scratch.get<unsigned long long>("sseq_totals", std::max<uint64_t>(1, cells));
        if (st.shard.active()) SCANRS_HIP(hipMemsetAsync(d_tot, 0, std::max<uint64_t>(1, cells) * 8, st.stream)); // the other ranks' slices
        launch_sseq_cell_totals(st, cp, gene_major, cr.n_local, d_tot + cr.begin);
        de_exchange(st).sum(d_tot, cells); // one contributor per element: the sum is a copy (m != 0 above: there are cells)
        std::vector<unsigned long long> tot(cells);
        if (cells) SCANRS_D2H(tot.data(), d_tot, cells * 8, st.stream);
        SCANRS_SYNC(st.stream);
        for (uint64_t i = 0; i < m; i++) counts[i] = (double)tot[cell_indices ? cell_indices[i] : i];
    }
    const double median = percentile(counts, 50.0);
    std::vector<double> sf(cells, 0.0);
    for (uint64_t i = 0; i < m; i++) sf[cell_indices ? cell_indices[i] : i] = counts[i] / median;
    // the moments of the size-normalized matrix (SizeNormalized: NaN factors read as 0) over the selected cells
    std::vector<int16_t> lab(cells, cell_indices ? (int16_t)-1 : (int16_t)0);
    if (cell_indices)
        for (uint64_t i = 0; i < n_sel; i++) lab[cell_indices[i]] = 0;
    std::vector<double> sf_dev(cells);
    double max_inv = 0.0, min_inv = INFINITY;
    for (uint64_t c = 0; c < cells; c++) {
        sf_dev[c] = std::isnan(sf[c]) ? 0.0 : sf[c];
        if (lab[c] == 0 && sf_dev[c] > 0.0 && std::isfinite(sf_dev[c])) { // an infinite factor (a median of 0) makes terms of exactly 0
            max_inv = std::max(max_inv, 1.0 / sf_dev[c]);
            min_inv = std::min(min_inv, 1.0 / sf_dev[c]);
        }
    }
    // One quantum for all genes, from a bound of the largest sum (m terms of the largest count over the smallest factor), when the
    // smallest term any gene can hold (a count of 1 over the largest factor) keeps its bits under it (fixed128.hpp); else a quantum per
    // gene from the class of its largest term, which costs one more walk over the nonzeros. Everything the choice reads spans ALL cells
    // (m, the factors, the all-reduced maximum count), so every rank of a sharded handle takes the same route.
    const double max_count = (double)sseq_max_count_global(st, cp);
    const double b1 = (double)m * max_count * max_inv;
    const double scale1 = fixed_scale(b1), scale2 = fixed_scale(b1 * max_count * max_inv);
    const bool per_gene = !fixed_single_quantum_keeps(min_inv, scale1, scale2);
    const int log2m = fixed_log2_ceil(m);
    st.sseq_moment_walks = per_gene ? 2 : 1;
    int16_t *d_lab = st.scratch.get<int16_t>("sseq_labels", std::max<uint64_t>(1, cr.n_local));
    double *d_sf = st.scratch.get<double>("sseq_sf", std::max<uint64_t>(1, cr.n_local));
    unsigned long long *d_sums = st.scratch.get<unsigned long long>("sseq_sums", std::max<uint64_t>(1, genes));
    unsigned long long *d_mom = st.scratch.get<unsigned long long>("sseq_mom", std::max<uint64_t>(1, genes * 4));
    uint32_t *d_bad = st.scratch.get<uint32_t>("sseq_bad", std::max<uint64_t>(1, genes));
    h2d(d_lab, lab.data() + cr.begin, cr.n_local, st.stream);
    h2d(d_sf, sf_dev.data() + cr.begin, cr.n_local, st.stream);
    std::vector<uint32_t> cls;
    uint32_t *d_cls = nullptr;
    if (per_gene) {
        d_cls = st.scratch.get<uint32_t>("sseq_cls", std::max<uint64_t>(1, genes));
        launch_sseq_term_class(st, cp, gene_major, genes, d_lab, d_sf, d_cls);
        cls.resize(genes);
        if (genes) SCANRS_D2H(cls.data(), d_cls, genes * 4, st.stream);
        SCANRS_SYNC(st.stream);
        if (st.shard.active() && genes) {
            // a gene's class over all cells is the maximum of the ranks' classes (one row of the gathered table per rank), and all
            // ranks round to the same quanta
            const std::vector<unsigned long long> mine(cls.begin(), cls.end());
            const std::vector<unsigned long long> rows = de_exchange(st).gather_host(mine.data(), genes);
            for (uint64_t g = 0; g < genes; g++) {
                unsigned long long k = 0;
                for (uint64_t r = 0; r < st.shard.world; r++) k = std::max(k, rows[r * genes + g]);
                cls[g] = (uint32_t)k;
            }
            h2d(d_cls, cls.data(), genes, st.stream);
            SCANRS_SYNC(st.stream); // `cls` is pageable
        }
    }
    launch_sseq_group_pass(st, cp, gene_major, genes, d_lab, 1, d_sums, d_sf, scale1, scale2, d_mom, d_bad, d_cls, log2m);
    if (st.shard.active() && genes) {
        // the scales come from bounds of the sums over ALL cells (m, the global maximum count, the global 1 / sf; or m and the genes'
        // classes over all ranks): every rank rounds its terms to the same quanta and the joined limbs are the 128-bit sums of the
        // unsharded pass
        unsigned long long *d_limbs = st.scratch.get<unsigned long long>("sseq_limbs", genes * SSEQ_LIMB_STRIDE);
        launch_sseq_mom_split(st, d_mom, d_bad, genes, d_limbs);
        de_exchange(st).sum(d_limbs, genes * SSEQ_LIMB_STRIDE);
        launch_sseq_mom_join(st, d_limbs, genes, d_mom, d_bad);
    }
    std::vector<unsigned long long> mom(genes * 4);
    std::vector<uint32_t> bad(genes);
    if (genes) {
        SCANRS_D2H(mom.data(), d_mom, genes * 32, st.stream);
        SCANRS_D2H(bad.data(), d_bad, genes * 4, st.stream);
    }
    SCANRS_SYNC(st.stream);
    const double md = (double)m;
    std::vector<double> mean(genes), var(genes);
    for (uint64_t g = 0; g < genes; g++) {
        // V[X] = E[X^2] - E[X]^2 (sqz/src/mat.rs:333-380)
        const double s1 = per_gene ? fixed_class_scale1(cls[g], log2m) : scale1, s2 = per_gene ? fixed_class_scale2(cls[g], log2m) : scale2;
        mean[g] = from_fixed(&mom[g * 4], s1) / md;
        var[g] = from_fixed(&mom[g * 4 + 2], s2) / md - mean[g] * mean[g];
        if (bad[g]) {
            mean[g] = INFINITY;
            var[g] = NAN;
        }
    }
    double sum_sf = 0.0;
    for (double v : sf)
        if (v != 0.0) sum_sf += 1.0 / v;
    sseq_params_from_moments(mean.data(), var.data(), genes, sum_sf, md, (double)genes, zeta_quintile, use_genes, gene_moment_phi, zeta_hat,
                             delta, gene_phi);
    memcpy(size_factors, sf.data(), cells * 8);
    memcpy(gene_means, mean.data(), genes * 8);
    memcpy(gene_variances, var.data(), genes * 8);
}

// ---- sseq_de_from_sums_with_cancellation (diff_exp.rs:190-300) ------------------------------------------------------------------
// the parameters of test j of gene g are read at [g * stride_g + j * stride_j]: (1, 0) for one SSeqParams shared by every test
void sseq_de_sums_strided(hipStream_t s, uint64_t genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                          const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t stride_g,
                          uint64_t stride_j, uint64_t big_count, const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc,
                          double *mean_in, double *mean_out, int backend, Storage *shard) {
    auto at = [&](uint64_t g, uint32_t j) { return g * stride_g + j * stride_j; };
    if (backend != SCANRS_NB_EXACT_LOGSPACE && backend != SCANRS_NB_EXACT_RATIO)
        fail(SCANRS_ERR_ARGUMENT, "backend must be SCANRS_NB_EXACT_LOGSPACE (0) or SCANRS_NB_EXACT_RATIO (1)");
    const bool ratio = backend == SCANRS_NB_EXACT_RATIO;
    const uint64_t total = genes * n_tests;
    // A sharded handle: rank r builds and launches the tests of the genes [G r / W, G (r + 1) / W) only and leaves the rest
    // of its device p array zero; one u64 all-reduce over the bit patterns then gathers them (each element is written by exactly one
    // rank: the sum is a copy). Every rank classifies every test, so the tests settled on the host stay replicated.
    const bool sharded = shard && shard->shard.active();
    const uint64_t g_lo = sharded ? genes * shard->shard.rank / shard->shard.world : 0;
    const uint64_t g_hi = sharded ? genes * (shard->shard.rank + 1) / shard->shard.world : genes;
    std::vector<uint64_t> elsewhere; // outputs of the tests that other ranks launch
    uint64_t n_mine = 0;
    std::vector<SseqExactTest> ex;
    std::vector<SseqAsymTest> as;
    std::vector<SseqRatioTest> rt;
    uint64_t n_chunks = 0, n_rchunks = 0;
    // one LogSpace test; a test's chunks and its result depend on its own inputs only, so a test that falls back from Ratio gets the bits
    // that backend = LogSpace gives it
    auto push_exact = [&](uint64_t o, uint32_t j, uint64_t g) {
        const uint64_t xa = sums_a[o], n = xa + sums_b[o];
        const double fa = sf_a[j], fb = sf_b[j], r = 1.0 / gene_phi[at(g, j)];
        ex.push_back(SseqExactTest{n, xa, fa * r, fb * r, special::nb_add_total(n, fa, fb, gene_means[at(g, j)], r), n_chunks, o});
        n_chunks += (n + SSEQ_CHUNK) / SSEQ_CHUNK; // n + 1 terms
    };
    for (uint64_t g = 0; g < genes; g++) {
        for (uint32_t j = 0; j < n_tests; j++) {
            const uint64_t o = g * n_tests + j, xa = sums_a[o], xb = sums_b[o];
            const double fa = sf_a[j], fb = sf_b[j], mu = gene_means[at(g, j)], phi = gene_phi[at(g, j)];
            const bool asym = use_genes[at(g, j)] && xa > big_count && xb > big_count;
            // nb_exact_test's early returns (dist.rs:76-86)
            if (!asym && (xa + xb == 0 || phi == 0.0 || fa == 0.0 || fb == 0.0)) {
                p[o] = 1.0;
                continue;
            }
            if (g < g_lo || g >= g_hi) {
                elsewhere.push_back(o);
                continue;
            }
            n_mine++;
            if (asym) {
                as.push_back(SseqAsymTest{xa, xb, fa, fb, mu, phi, o});
                continue;
            }
            if (!ratio) {
                push_exact(o, j, g);
                continue;
            }
            const uint64_t n = xa + xb;
            const double r = 1.0 / phi, sar = fa * r, sbr = fb * r;
            const uint64_t anchor = sseq_ratio_anchor(n, sar, sbr);
            rt.push_back(SseqRatioTest{n, xa, anchor, sar, sbr, n_rchunks, o});
            n_rchunks += (anchor + SSEQ_CHUNK - 1) / SSEQ_CHUNK + (n - anchor + SSEQ_CHUNK - 1) / SSEQ_CHUNK; // n >= 1: at least one
        }
    }
    if (ex.size() > 0xFFFFFFFFull || as.size() > 0xFFFFFFFFull || rt.size() > 0xFFFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "too many tests in one call");
    if (shard) shard->de_shard_tests = n_mine;
    // one p array for both stages: a test that falls back from Ratio is overwritten by its LogSpace result
    DevBuf<double> d_p;
    if (!rt.empty() || !ex.empty() || !as.empty() || (sharded && total)) d_p.alloc(total);
    if (sharded && total) SCANRS_HIP(hipMemsetAsync(d_p.p, 0, total * 8, s));
    if (!rt.empty()) {
        // Ratio: the tests it can partition get their p-value; the others come back as SSEQ_RATIO_FALLBACK and join the LogSpace list
        DevBuf<SseqRatioTest> d_rt(rt.size());
        DevBuf<double> d_obs(rt.size()), d_scale(n_rchunks);
        DevBuf<double2> d_part(n_rchunks);
        h2d(d_rt.p, rt.data(), rt.size(), s);
        launch_sseq_ratio(s, d_rt.p, (uint32_t)rt.size(), n_rchunks, d_obs.p, d_scale.p, d_part.p, d_p.p);
        std::vector<double> pd(total);
        SCANRS_D2H(pd.data(), d_p.p, total * 8, s);
        SCANRS_SYNC(s);
        for (const auto &t : rt) {
            if (pd[t.out] == SSEQ_RATIO_FALLBACK)
                push_exact(t.out, (uint32_t)(t.out % n_tests), t.out / n_tests);
            else
                p[t.out] = pd[t.out];
        }
    }
    if (!ex.empty() || !as.empty()) {
        DevBuf<SseqExactTest> d_ex(std::max<size_t>(1, ex.size()));
        DevBuf<SseqAsymTest> d_as(std::max<size_t>(1, as.size()));
        DevBuf<double> d_obs(std::max<size_t>(1, ex.size()));
        DevBuf<double4> d_part(std::max<uint64_t>(1, n_chunks));
        h2d(d_ex.p, ex.data(), ex.size(), s);
        h2d(d_as.p, as.data(), as.size(), s);
        launch_sseq_exact(s, d_ex.p, (uint32_t)ex.size(), n_chunks, d_obs.p, d_part.p, d_p.p);
        launch_sseq_asymptotic(s, d_as.p, (uint32_t)as.size(), d_p.p);
        std::vector<double> pd(total);
        SCANRS_D2H(pd.data(), d_p.p, total * 8, s);
        SCANRS_SYNC(s);
        for (const auto &t : ex) p[t.out] = pd[t.out];
        for (const auto &t : as) p[t.out] = pd[t.out];
    }
    if (sharded && total) {
        static_assert(sizeof(double) == sizeof(unsigned long long), "p-values travel as their bit patterns");
        de_exchange(*shard).sum(reinterpret_cast<unsigned long long *>(d_p.p), total);
        std::vector<double> pd(total);
        SCANRS_D2H(pd.data(), d_p.p, total * 8, s);
        SCANRS_SYNC(s);
        for (const uint64_t o : elsewhere) p[o] = pd[o];
    }
    snoop_poll(snoop, 0.75);
    // BH over the tested genes only
    std::vector<double> pv, q;
    for (uint32_t j = 0; j < n_tests; j++) {
        pv.clear();
        for (uint64_t g = 0; g < genes; g++) {
            p_adj[g * n_tests + j] = p[g * n_tests + j];
            if (use_genes[at(g, j)]) pv.push_back(p[g * n_tests + j]);
        }
        q.resize(pv.size());
        sseq_host_bh(pv.data(), pv.size(), q.data());
        uint64_t k = 0;
        for (uint64_t g = 0; g < genes; g++)
            if (use_genes[at(g, j)]) p_adj[g * n_tests + j] = q[k++];
    }
    snoop_poll(snoop, 0.9);
    for (uint64_t g = 0; g < genes; g++)
        for (uint32_t j = 0; j < n_tests; j++) {
            const uint64_t o = g * n_tests + j;
            log2fc[o] = std::log2((double)(1 + sums_a[o]) / (1.0 + sf_a[j])) - std::log2((double)(1 + sums_b[o]) / (1.0 + sf_b[j]));
        }
    snoop_poll(snoop, 0.95);
    for (uint64_t g = 0; g < genes; g++)
        for (uint32_t j = 0; j < n_tests; j++) {
            const uint64_t o = g * n_tests + j;
            mean_in[o] = sf_a[j] == 0.0 ? 0.0 : (double)sums_a[o] / sf_a[j];
            mean_out[o] = sf_b[j] == 0.0 ? 0.0 : (double)sums_b[o] / sf_b[j];
        }
    snoop_poll(snoop, 1.0);
}

void sseq_de_sums(hipStream_t s, uint64_t genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                  const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t big_count,
                  const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc, double *mean_in, double *mean_out, int backend) {
    sseq_de_sums_strided(s, genes, n_tests, sums_a, sums_b, sf_a, sf_b, gene_means, gene_phi, use_genes, 1, 0, big_count, snoop, p, p_adj, log2fc,
                         mean_in, mean_out, backend);
}

// ---- sseq_differential_expression (diff_exp.rs:122-175) over labels ---------------------------------------------------------------
// mode 0: every group against all other labelled cells (Cell Ranger's per-cluster DE); mode 1: group 0 against group 1;
// mode 2: every group 1 .. n_groups - 1 against group 0 (a shared control: its sums and size factor are computed once)
void sseq_de_matrix(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const int16_t *labels,
                    uint32_t n_groups, int mode, const double *size_factors, const double *gene_means, const double *gene_phi,
                    const uint8_t *use_genes, uint64_t big_count, const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p,
                    double *p_adj, double *log2fc, double *mean_in, double *mean_out, int backend) {
    if (mode != 0 && mode != 1 && mode != 2)
        fail(SCANRS_ERR_ARGUMENT, "mode must be 0 (one against the rest), 1 (group 0 against group 1) or 2 (each group against group 0)");
    if (mode != 0 && n_groups < 2) fail(SCANRS_ERR_ARGUMENT, "mode %d needs groups 0 and 1", mode);
    if (backend != SCANRS_NB_EXACT_LOGSPACE && backend != SCANRS_NB_EXACT_RATIO)
        fail(SCANRS_ERR_ARGUMENT, "backend must be SCANRS_NB_EXACT_LOGSPACE (0) or SCANRS_NB_EXACT_RATIO (1)");
    const uint64_t cells_local = cells;
    cells = cell_range(st, cells_local).global; // labels and size_factors span the whole matrix; the folds below run replicated
    check_labels(labels, cells, n_groups);
    const uint32_t n_tests = mode == 0 ? n_groups : mode == 1 ? 1 : n_groups - 1;
    snoop_poll(snoop, 0.0);
    // the size factors of each side: sums over its cells in cell order (the reference's fold over cond_a / cond_b)
    std::vector<double> fa(n_tests, 0.0), fb(n_tests, 0.0);
    if (mode == 2) {
        double control = 0.0;
        for (uint64_t c = 0; c < cells; c++) {
            const int l = labels[c];
            if (l == 0) control += size_factors[c];
            if (l > 0) fa[l - 1] += size_factors[c];
        }
        std::fill(fb.begin(), fb.end(), control);
    }
    for (uint32_t j = 0; mode != 2 && j < n_tests; j++) {
        for (uint64_t c = 0; c < cells; c++) {
            const int l = labels[c];
            if (l < 0) continue;
            if (mode == 0) {
                if (l == (int)j)
                    fa[j] += size_factors[c];
                else
                    fb[j] += size_factors[c];
            } else {
                if (l == 0) fa[j] += size_factors[c];
                if (l == 1) fb[j] += size_factors[c];
            }
        }
    }
    snoop_poll(snoop, 0.1);
    std::vector<uint64_t> sums(genes * n_groups);
    sseq_group_sums(st, cp, gene_major, genes, cells_local, labels, n_groups, sums.data(), nullptr);
    for (uint64_t g = 0; g < genes; g++) {
        const uint64_t *row = &sums[g * n_groups];
        if (mode == 0) {
            uint64_t all = 0;
            for (uint32_t j = 0; j < n_groups; j++) all += row[j];
            for (uint32_t j = 0; j < n_groups; j++) {
                sums_in[g * n_tests + j] = row[j];
                sums_out[g * n_tests + j] = all - row[j];
            }
        } else if (mode == 1) {
            sums_in[g] = row[0];
            sums_out[g] = row[1];
        } else {
            for (uint32_t j = 0; j < n_tests; j++) {
                sums_in[g * n_tests + j] = row[j + 1];
                sums_out[g * n_tests + j] = row[0];
            }
        }
    }
    snoop_poll(snoop, 0.6);
    sseq_de_sums_strided(st.stream, genes, n_tests, sums_in, sums_out, fa.data(), fb.data(), gene_means, gene_phi, use_genes, 1, 0, big_count, snoop,
                         p, p_adj, log2fc, mean_in, mean_out, backend, &st);
}

// the copy DE walks: the gene-major one when it is resident, else the cell-major one (no transposition is built for DE)
SparseCopy &sseq_resident_copy(scanrs_mat *m, bool *gene_major) {
    Storage &st = *m->st;
    if (st.shard.active() && !cols_sharded(m))
        fail(SCANRS_ERR_ARGUMENT, "differential expression of a sharded handle needs the cells (the view's columns) as the sharded dimension: this handle is sharded over the genes");
    const bool want_base_rows = !m->transposed; // genes = view rows
    const bool primary_rows = st.storage == SCANRS_CSR;
    if (primary_rows == want_base_rows) {
        *gene_major = true;
        return st.primary;
    }
    if (st.other_settled) {
        *gene_major = true;
        return st.other;
    }
    *gene_major = false;
    return st.primary;
}

void sseq_refuse_sharded(const scanrs_mat *m, const char *what) {
    if (m->st->shard.active()) fail(SCANRS_ERR_ARGUMENT, "%s of a sharded handle is not supported", what);
}

} // namespace scanrs

// ---- the extern "C" entry points. NOT under this file's contract(off): special.hpp's inline functions are compiled with the default contraction
// (included above the pragma), as in the device code
#pragma clang fp contract(fast)
using namespace scanrs;
extern "C" {
int scanrs_sseq_params(scanrs_mat *m, double zeta_quintile, const uint64_t *cell_indices, uint64_t n_sel, const double *umi_counts,
                       double *size_factors, double *gene_means, double *gene_variances, uint8_t *use_genes, double *gene_moment_phi,
                       double *zeta_hat, double *delta, double *gene_phi) {
    return guard([&] {
        if (!m || !size_factors || !gene_means || !gene_variances || !use_genes || !gene_moment_phi || !zeta_hat || !delta || !gene_phi)
            fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (!(zeta_quintile >= 0.0 && zeta_quintile <= 1.0)) fail(SCANRS_ERR_ARGUMENT, "zeta_quintile must be in [0, 1]");
        CurrentHandle cur(m->st.get());
        bool gm = false;
        SparseCopy &cp = sseq_resident_copy(m, &gm);
        m->st->de_shard_tests = m->st->de_shard_allreduces = 0;
        sseq_params(*m->st, cp, gm, m->rows(), m->cols(), zeta_quintile, cell_indices, n_sel, umi_counts, size_factors, gene_means,
                    gene_variances, use_genes, gene_moment_phi, zeta_hat, delta, gene_phi);
    });
}
int scanrs_sseq_params_from_moments(const double *mean_g, const double *var_g, uint64_t n, double sum_size_factors, double n_cells,
                                    double n_genes, double zeta_quintile, uint8_t *use_genes, double *gene_moment_phi, double *zeta_hat,
                                    double *delta, double *gene_phi) {
    return guard([&] {
        if ((n && (!mean_g || !var_g || !use_genes || !gene_moment_phi || !gene_phi)) || !zeta_hat || !delta)
            fail(SCANRS_ERR_ARGUMENT, "null argument");
        sseq_params_from_moments(mean_g, var_g, n, sum_size_factors, n_cells, n_genes, zeta_quintile, use_genes, gene_moment_phi, zeta_hat,
                                 delta, gene_phi);
    });
}
int scanrs_mat_group_sums(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, uint64_t *sums, uint64_t *cells_per_group) {
    return guard([&] {
        if (!m || !labels || !sums) fail(SCANRS_ERR_ARGUMENT, "null argument");
        CurrentHandle cur(m->st.get());
        bool gm = false;
        SparseCopy &cp = sseq_resident_copy(m, &gm);
        m->st->de_shard_tests = m->st->de_shard_allreduces = 0;
        sseq_group_sums(*m->st, cp, gm, m->rows(), m->cols(), labels, n_groups, sums, cells_per_group);
    });
}
int scanrs_sseq_de_backend(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, int mode, const double *size_factors,
                           const double *gene_means, const double *gene_phi, const uint8_t *use_genes, uint64_t big_count, int backend,
                           const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc,
                           double *mean_in, double *mean_out) {
    return guard([&] {
        if (!m || !labels || !size_factors || !gene_means || !gene_phi || !use_genes || !sums_in || !sums_out || !p || !p_adj || !log2fc ||
            !mean_in || !mean_out)
            fail(SCANRS_ERR_ARGUMENT, "null argument");
        CurrentHandle cur(m->st.get());
        bool gm = false;
        SparseCopy &cp = sseq_resident_copy(m, &gm);
        m->st->de_shard_tests = m->st->de_shard_allreduces = 0;
        sseq_de_matrix(*m->st, cp, gm, m->rows(), m->cols(), labels, n_groups, mode, size_factors, gene_means, gene_phi, use_genes, big_count,
                       snoop, sums_in, sums_out, p, p_adj, log2fc, mean_in, mean_out, backend);
    });
}
int scanrs_sseq_de(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, int mode, const double *size_factors, const double *gene_means,
                   const double *gene_phi, const uint8_t *use_genes, uint64_t big_count, const scanrs_snoop *snoop, uint64_t *sums_in,
                   uint64_t *sums_out, double *p, double *p_adj, double *log2fc, double *mean_in, double *mean_out) {
    if (mode != 0 && mode != 1)
        return guard([&] { fail(SCANRS_ERR_ARGUMENT, "mode must be 0 (one against the rest) or 1 (group 0 against group 1)"); });
    return scanrs_sseq_de_backend(m, labels, n_groups, mode, size_factors, gene_means, gene_phi, use_genes, big_count, SCANRS_NB_EXACT_LOGSPACE,
                                  snoop, sums_in, sums_out, p, p_adj, log2fc, mean_in, mean_out);
}
int scanrs_sseq_de_from_sums(uint64_t n_genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                             const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes,
                             uint64_t big_count, const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc, double *mean_in,
                             double *mean_out) {
    return scanrs_sseq_de_from_sums_backend(n_genes, n_tests, sums_a, sums_b, sf_a, sf_b, gene_means, gene_phi, use_genes, big_count,
                                            SCANRS_NB_EXACT_LOGSPACE, snoop, p, p_adj, log2fc, mean_in, mean_out);
}
int scanrs_sseq_de_from_sums_backend(uint64_t n_genes, uint32_t n_tests, const uint64_t *sums_a, const uint64_t *sums_b, const double *sf_a,
                                     const double *sf_b, const double *gene_means, const double *gene_phi, const uint8_t *use_genes,
                                     uint64_t big_count, int backend, const scanrs_snoop *snoop, double *p, double *p_adj, double *log2fc,
                                     double *mean_in, double *mean_out) {
    return guard([&] {
        if (n_genes && n_tests &&
            (!sums_a || !sums_b || !sf_a || !sf_b || !gene_means || !gene_phi || !use_genes || !p || !p_adj || !log2fc || !mean_in || !mean_out))
            fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (backend != SCANRS_NB_EXACT_LOGSPACE && backend != SCANRS_NB_EXACT_RATIO)
            fail(SCANRS_ERR_ARGUMENT, "backend must be SCANRS_NB_EXACT_LOGSPACE (0) or SCANRS_NB_EXACT_RATIO (1)");
        need_device();
        sseq_de_sums(nullptr, n_genes, n_tests, sums_a, sums_b, sf_a, sf_b, gene_means, gene_phi, use_genes, big_count, snoop, p, p_adj, log2fc,
                     mean_in, mean_out, backend);
    });
}
int scanrs_host_nb_exact_test(uint64_t x_a, uint64_t x_b, double sf_a, double sf_b, double mu, double phi, double *p) {
    return guard([&] {
        if (!p) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *p = sseq_host_exact_test(x_a, x_b, sf_a, sf_b, mu, phi);
    });
}
int scanrs_host_nb_exact_test_ratio(uint64_t x_a, uint64_t x_b, double sf_a, double sf_b, double mu, double phi, double *p) {
    return guard([&] {
        if (!p) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *p = sseq_host_exact_test_ratio(x_a, x_b, sf_a, sf_b, mu, phi);
    });
}
int scanrs_host_nb_exact_ratio_step(double k, double n, double sa_r, double sb_r, double *out) {
    return guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = ratio_step(k, n, sa_r, sb_r);
    });
}
int scanrs_host_nb_asymptotic_test(uint64_t x_a, uint64_t x_b, double sf_a, double sf_b, double mu, double phi, double *p) {
    return guard([&] {
        if (!p) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *p = special::nb_asymptotic(x_a, x_b, sf_a, sf_b, mu, phi);
    });
}
int scanrs_host_nb_log_prob_all(uint64_t n, double sf_a, double sf_b, double mu, double r, double *out) {
    return guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        sseq_host_log_prob_all(n, sf_a, sf_b, mu, r, out);
    });
}
int scanrs_host_adjusted_pvalue_bh(const double *p, uint64_t n, double *out) {
    return guard([&] {
        if (n && (!p || !out)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        sseq_host_bh(p, n, out);
    });
}
int scanrs_host_betainc(double a, double b, double x, double *out) {
    return guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = special::betainc(a, b, x);
    });
}
int scanrs_host_betaincinv(double a, double b, double p, double *out) {
    return guard([&] {
        if (!out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = special::betaincinv(a, b, p);
    });
}
} // extern "C"
