// Host logic of scanrs_sseq_de_pairs: batched pairwise sSeq DE in which test j runs with the parameters of its own union,
// compute_sseq_params(mat, zeta, Some(A ∪ B), None) (diff_exp.rs:458-490) followed by the DE of A against B (diff_exp.rs:125-161): the
// shape of merge_clusters.rs' candidates and of Cell Ranger's shared-control batched path (diff_exp.rs:361-376). Two passes over the
// nonzeros serve every pair: the per-cell totals and the fused grouped pass of merge_clusters; the accumulators stay on the device
// and the per-pair combination runs there (sseq_pairs.hip). The identity behind it: with u_c the total of cell c and m_S the
// interpolated median total of the union S, sf_c = u_c / m_S, so Σ_S x/sf_c = m_S Σ_S x/u_c and Σ_S (x/sf_c)² = m_S² Σ_S (x/u_c)², and
// the sums over S are the exact integer sums of the two groups' fixed-point accumulators.
#include "common.hpp"
#include "fixed128.hpp"
#include "shard_exchange.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

// the reference's host arithmetic is not contracted
#pragma clang fp contract(off)

namespace scanrs {

// percentile_of_sorted(.., 50) (stat.rs:140-162) of the union of two ascending lists, selecting the two ranks it reads
double sseq_union_median(const double *a, uint64_t na, const double *b, uint64_t nb) {
    const uint64_t len = na + nb;
    if (len == 0) fail(SCANRS_ERR_ARGUMENT, "percentile of an empty list");
    auto kth = [&](uint64_t k) { // k-th smallest (0-based) of the union
        uint64_t lo = k > nb ? k - nb : 0, hi = std::min<uint64_t>(k, na);
        while (lo < hi) { // the number i of elements taken from a
            const uint64_t i = (lo + hi) / 2, j = k - i;
            if (j > 0 && i < na && b[j - 1] > a[i])
                lo = i + 1;
            else
                hi = i;
        }
        const uint64_t i = lo, j = k - i;
        if (i >= na) return b[j];
        if (j >= nb) return a[i];
        return std::min(a[i], b[j]);
    };
    if (len == 1) return kth(0);
    const double length = (double)(len - 1);
    const double rank = (50.0 / 100.0) * length;
    const double l_rank = std::floor(rank);
    const double dd = rank - l_rank;
    const uint64_t n = (uint64_t)l_rank;
    const double lo = kth(n), hi = kth(n + 1);
    return lo + (hi - lo) * dd;
}

// the grouped accumulators of a sharded handle, all-reduced in tiles through a scratch of fixed size (sseq_pairs.hip)
uint64_t sseq_reduce_group_acc(Storage &st, unsigned long long *d_acc, uint64_t n_entries) {
    if (!st.shard.active() || n_entries == 0) return 0;
    unsigned long long *d_planes = st.scratch.get<unsigned long long>("sseq_acc_planes", SSEQ_ACC_PLANES * std::min<uint64_t>(SSEQ_ACC_TILE, n_entries + 1));
    uint64_t steps = 0;
    for (uint64_t e0 = 0; e0 < n_entries; e0 += SSEQ_ACC_TILE, steps++) {
        const uint64_t ne = std::min<uint64_t>(SSEQ_ACC_TILE, n_entries - e0), ne_pad = (ne + 1) & ~1ull;
        launch_pairs_acc_split(st.stream, d_acc + e0 * 5, ne, d_planes);
        ShardExchange{st, st.de_shard_allreduces}.sum(d_planes, SSEQ_ACC_PLANES * ne_pad);
        launch_pairs_acc_join(st.stream, d_planes, ne, d_acc + e0 * 5);
    }
    return steps;
}

namespace {
struct PairOut { // where the caller wants the results: genes x n_pairs each
    uint64_t *sums_in, *sums_out;
    double *p, *p_adj, *log2fc, *mean_in, *mean_out;
};
template <typename T>
void put_col(T *dst, uint64_t genes, uint32_t n_pairs, uint32_t j, const T *col) {
    if (dst)
        for (uint64_t g = 0; g < genes; g++) dst[g * n_pairs + j] = col[g];
}
struct LiteralPair { // a pair that took the literal route: its columns, scattered behind the batched tests
    uint32_t j;
    std::vector<uint64_t> si, so;
    std::vector<double> p, padj, l2, mi, mo, mean, var, phi_mm, phi;
    std::vector<uint8_t> use;
    double zh = 0.0, dl = 0.0, fa = 0.0, fb = 0.0, sum_sf = 0.0;
};
} // namespace

void sseq_de_pairs(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const int16_t *labels, uint32_t n_groups,
                   const uint32_t *pair_a, const uint32_t *pair_b, uint32_t n_pairs, double zeta_quintile, uint64_t big_count, int backend,
                   const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out, double *p, double *p_adj, double *log2fc, double *mean_in,
                   double *mean_out, scanrs_sseq_pair_params *params, bool collective) {
    // a sharded handle (collective only): the copy holds the cells [cr.begin, cr.begin + cr.n_local) and `cells` is from here on
    // the whole matrix: labels span it, the host folds run replicated, the device gets this rank's slice of the labels
    const CellRange cr = collective ? cell_range(st, cells) : CellRange{0, cells, cells};
    const uint64_t cells_local = cr.n_local;
    cells = cr.global;
    if (backend != SCANRS_NB_EXACT_LOGSPACE && backend != SCANRS_NB_EXACT_RATIO)
        fail(SCANRS_ERR_ARGUMENT, "backend must be SCANRS_NB_EXACT_LOGSPACE (0) or SCANRS_NB_EXACT_RATIO (1)");
    if (n_pairs == 0) fail(SCANRS_ERR_ARGUMENT, "n_pairs must be at least 1");
    if (n_groups == 0 || n_groups > SSEQ_MAX_GROUPS) fail(SCANRS_ERR_ARGUMENT, "n_groups must be in 1 .. %u", SSEQ_MAX_GROUPS);
    if (cells > 0xFFFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "at most 2^32 - 1 cells");
    // the labelled cells group by group, in cell order inside a group (a counting sort), and every group's segment
    std::vector<uint32_t> off(n_groups + 1, 0);
    for (uint64_t c = 0; c < cells; c++) {
        if (labels[c] < -1 || labels[c] >= (int)n_groups)
            fail(SCANRS_ERR_ARGUMENT, "label %d of cell %llu is outside -1 .. n_groups - 1", (int)labels[c], (unsigned long long)c);
        if (labels[c] >= 0) off[labels[c] + 1]++;
    }
    for (uint32_t g = 0; g < n_groups; g++) off[g + 1] += off[g];
    const uint64_t n_lab = off[n_groups];
    for (uint32_t j = 0; j < n_pairs; j++) {
        const uint32_t a = pair_a[j], b = pair_b[j];
        if (a >= n_groups || b >= n_groups) fail(SCANRS_ERR_ARGUMENT, "pair %u names group %u, outside 0 .. n_groups - 1", j, std::max(a, b));
        if (a == b) fail(SCANRS_ERR_ARGUMENT, "pair %u tests group %u against itself", j, a);
        if (off[a + 1] - off[a] + off[b + 1] - off[b] == 0) fail(SCANRS_ERR_ARGUMENT, "pair %u (groups %u and %u) has no cell", j, a, b);
    }
    std::vector<uint32_t> perm(std::max<uint64_t>(1, n_lab)), cur(off.begin(), off.end() - 1);
    for (uint64_t c = 0; c < cells; c++)
        if (labels[c] >= 0) perm[cur[labels[c]]++] = (uint32_t)c;
    const hipStream_t s = st.stream;
    st.de_pairs_passes = st.de_pairs_literal = 0;
    uint64_t passes = 0;
    snoop_poll(snoop, 0.0);

    // pass 1: per-cell totals; then every group's sorted totals and integer sums, and the pairs' headers
    // (the scale comes from the GLOBAL cell count: every rank of a sharded handle rounds every term to the same quantum)
    const double scale = fixed_scale((double)cells); // Σ x/u_c, Σ (x/u_c)², Σ 1/u_c of a group: at most one per cell
    const uint64_t total = genes * n_pairs;
    unsigned long long *d_tot = st.scratch.get<unsigned long long>("sseq_totals", cells + 1);
    if (cells_local != cells) SCANRS_HIP(hipMemsetAsync(d_tot, 0, cells * 8, s)); // the other ranks' slices
    launch_sseq_cell_totals(st, cp, gene_major, cells_local, d_tot + cr.begin);
    // one contributor per element: the sum is a copy (every pair has a cell, so there are cells)
    if (collective) ShardExchange{st, st.de_shard_allreduces}.sum(d_tot, cells);
    passes++;
    int16_t *d_lab = st.scratch.get<int16_t>("sseq_labels", std::max<uint64_t>(1, cells_local));
    h2d(d_lab, labels + cr.begin, cells_local, s);
    DevBuf<uint32_t> d_perm(perm.size()), d_off(off.size()), d_pa(n_pairs), d_pb(n_pairs);
    DevBuf<unsigned long long> d_gathered(perm.size()), d_sorted(perm.size()), d_stats((size_t)n_groups * 3);
    DevBuf<SseqPairHeader> d_hdr(n_pairs);
    DevBuf<char> sort_tmp;
    h2d(d_perm.p, perm.data(), perm.size(), s);
    h2d(d_off.p, off.data(), off.size(), s);
    h2d(d_pa.p, pair_a, n_pairs, s);
    h2d(d_pb.p, pair_b, n_pairs, s);
    launch_pairs_group_stats(s, d_tot, d_perm.p, d_off.p, n_groups, n_lab, scale, d_gathered.p, d_sorted.p, d_stats.p, sort_tmp);
    launch_pairs_headers(s, d_sorted.p, d_off.p, d_stats.p, d_pa.p, d_pb.p, n_pairs, scale, d_hdr.p);
    std::vector<SseqPairHeader> hdr(n_pairs);
    SCANRS_D2H(hdr.data(), d_hdr.p, n_pairs * sizeof(SseqPairHeader), s);
    SCANRS_SYNC(s);
    snoop_poll(snoop, 0.1);

    // pass 2: the grouped pass (one per tile of groups from the gene-major copy), then the parameters of every pair
    DevBuf<unsigned long long> d_acc(std::max<uint64_t>(1, (uint64_t)n_groups * genes * 5));
    passes += launch_merge_pass(st, cp, gene_major, genes, d_lab, n_groups, d_tot + cr.begin, scale, scale, d_acc.p);
    if (collective) sseq_reduce_group_acc(st, d_acc.p, (uint64_t)n_groups * genes); // from here on every rank holds the unsharded integers
    DevBuf<double> d_mean(std::max<uint64_t>(1, total)), d_var(std::max<uint64_t>(1, total)), d_phi_mm(std::max<uint64_t>(1, total)),
        d_phi(std::max<uint64_t>(1, total)), d_zd((size_t)n_pairs * 2);
    DevBuf<uint8_t> d_use(std::max<uint64_t>(1, total));
    DevBuf<unsigned long long> d_sa(std::max<uint64_t>(1, total)), d_sb(std::max<uint64_t>(1, total));
    launch_pairs_moments(s, d_acc.p, d_hdr.p, genes, n_pairs, scale, d_mean.p, d_var.p, d_use.p, d_phi_mm.p, d_sa.p, d_sb.p);
    launch_pairs_shrink(s, d_phi_mm.p, d_use.p, genes, n_pairs, 100.0 * zeta_quintile, d_zd.p, d_phi.p);
    std::vector<double> mean(total), phi(total), zd((size_t)n_pairs * 2);
    std::vector<uint8_t> use(total);
    if (total) {
        SCANRS_D2H(mean.data(), d_mean.p, total * 8, s);
        SCANRS_D2H(phi.data(), d_phi.p, total * 8, s);
        SCANRS_D2H(use.data(), d_use.p, total, s);
        SCANRS_D2H(sums_in, d_sa.p, total * 8, s);
        SCANRS_D2H(sums_out, d_sb.p, total * 8, s);
        if (params && params->gene_variances) SCANRS_D2H(params->gene_variances, d_var.p, total * 8, s);
        if (params && params->gene_moment_phi) SCANRS_D2H(params->gene_moment_phi, d_phi_mm.p, total * 8, s);
    }
    SCANRS_D2H(zd.data(), d_zd.p, (size_t)n_pairs * 16, s);
    SCANRS_SYNC(s);
    d_acc.release();

    // a union whose median total is 0 has no finite size factors: such a pair runs the reference's own calls (as merge_clusters does)
    std::vector<LiteralPair> lit;
    uint64_t lit_tests = 0; // tests this rank launched for the literal pairs
    {
        std::vector<int16_t> lab3;
        std::vector<uint64_t> union_idx;
        std::vector<double> sf;
        for (uint32_t j = 0; j < n_pairs; j++) {
            if (!hdr[j].literal) continue;
            lit.emplace_back();
            LiteralPair &L = lit.back();
            L.j = j;
            lab3.assign(cells, -1);
            union_idx.clear();
            for (uint64_t c = 0; c < cells; c++) {
                lab3[c] = labels[c] == (int)pair_a[j] ? 0 : labels[c] == (int)pair_b[j] ? 1 : -1;
                if (lab3[c] >= 0) union_idx.push_back(c);
            }
            sf.assign(cells, 0.0);
            for (auto *v : {&L.p, &L.padj, &L.l2, &L.mi, &L.mo, &L.mean, &L.var, &L.phi_mm, &L.phi}) v->assign(genes, 0.0);
            L.si.assign(genes, 0);
            L.so.assign(genes, 0);
            L.use.assign(genes, 0);
            sseq_params(st, cp, gene_major, genes, cells_local, zeta_quintile, union_idx.data(), union_idx.size(), nullptr, sf.data(), L.mean.data(),
                        L.var.data(), L.use.data(), L.phi_mm.data(), &L.zh, &L.dl, L.phi.data());
            sseq_de_matrix(st, cp, gene_major, genes, cells_local, lab3.data(), 2, 1, sf.data(), L.mean.data(), L.phi.data(), L.use.data(), big_count,
                           nullptr, L.si.data(), L.so.data(), L.p.data(), L.padj.data(), L.l2.data(), L.mi.data(), L.mo.data(), backend);
            for (uint64_t c = 0; c < cells; c++) { // the sides' size factors and Σ 1/sf as those two calls take them
                if (lab3[c] == 0) L.fa += sf[c];
                if (lab3[c] == 1) L.fb += sf[c];
                if (sf[c] != 0.0) L.sum_sf += 1.0 / sf[c];
            }
            passes += 3 + st.sseq_moment_walks; // totals, max count, moments (the class walk first where every gene gets its quantum), group sums
            lit_tests += st.de_shard_tests;
        }
    }
    snoop_poll(snoop, 0.6);

    std::vector<double> fa(n_pairs), fb(n_pairs);
    for (uint32_t j = 0; j < n_pairs; j++) {
        fa[j] = hdr[j].sf_a;
        fb[j] = hdr[j].sf_b;
    }
    sseq_de_sums_strided(s, genes, n_pairs, sums_in, sums_out, fa.data(), fb.data(), mean.data(), phi.data(), use.data(), n_pairs, 1, big_count, snoop,
                         p, p_adj, log2fc, mean_in, mean_out, backend, collective ? &st : nullptr);
    if (collective) st.de_shard_tests += lit_tests;

    for (const LiteralPair &L : lit) {
        const uint32_t j = L.j;
        put_col(sums_in, genes, n_pairs, j, L.si.data());
        put_col(sums_out, genes, n_pairs, j, L.so.data());
        put_col(p, genes, n_pairs, j, L.p.data());
        put_col(p_adj, genes, n_pairs, j, L.padj.data());
        put_col(log2fc, genes, n_pairs, j, L.l2.data());
        put_col(mean_in, genes, n_pairs, j, L.mi.data());
        put_col(mean_out, genes, n_pairs, j, L.mo.data());
        put_col(mean.data(), genes, n_pairs, j, L.mean.data());
        put_col(phi.data(), genes, n_pairs, j, L.phi.data());
        put_col(use.data(), genes, n_pairs, j, L.use.data());
        if (params) {
            put_col(params->gene_variances, genes, n_pairs, j, L.var.data());
            put_col(params->gene_moment_phi, genes, n_pairs, j, L.phi_mm.data());
        }
        zd[2 * (size_t)j] = L.zh;
        zd[2 * (size_t)j + 1] = L.dl;
        fa[j] = L.fa;
        fb[j] = L.fb;
        hdr[j].sum_sf = L.sum_sf;
    }
    if (params) {
        if (params->gene_means && total) memcpy(params->gene_means, mean.data(), total * 8);
        if (params->gene_phi && total) memcpy(params->gene_phi, phi.data(), total * 8);
        if (params->use_genes && total) memcpy(params->use_genes, use.data(), total);
        for (uint32_t j = 0; j < n_pairs; j++) {
            if (params->zeta_hat) params->zeta_hat[j] = zd[2 * (size_t)j];
            if (params->delta) params->delta[j] = zd[2 * (size_t)j + 1];
            if (params->sf_a) params->sf_a[j] = fa[j];
            if (params->sf_b) params->sf_b[j] = fb[j];
            if (params->median_total) params->median_total[j] = hdr[j].m_s;
            if (params->sum_size_factors) params->sum_size_factors[j] = hdr[j].sum_sf;
            if (params->n_cells_a) params->n_cells_a[j] = hdr[j].n_a;
            if (params->n_cells_b) params->n_cells_b[j] = hdr[j].n_b;
            if (params->literal) params->literal[j] = (uint8_t)hdr[j].literal;
        }
    }
    st.de_pairs_passes = passes;
    st.de_pairs_literal = lit.size();
}

} // namespace scanrs

using namespace scanrs;
extern "C" {
int scanrs_sseq_de_pairs(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, const uint32_t *pair_a, const uint32_t *pair_b, uint32_t n_pairs,
                         double zeta_quintile, uint64_t big_count, int backend, const scanrs_snoop *snoop, uint64_t *sums_in, uint64_t *sums_out,
                         double *p, double *p_adj, double *log2fc, double *mean_in, double *mean_out, scanrs_sseq_pair_params *params) {
    return guard([&] {
        if (!m || !labels || (n_pairs && (!pair_a || !pair_b)) || !sums_in || !sums_out || !p || !p_adj || !log2fc || !mean_in || !mean_out)
            fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (!(zeta_quintile >= 0.0 && zeta_quintile <= 1.0)) fail(SCANRS_ERR_ARGUMENT, "zeta_quintile must be in [0, 1]");
        CurrentHandle cur(m->st.get());
        sseq_refuse_sharded(m, "batched pairwise differential expression");
        bool gm = false;
        SparseCopy &cp = sseq_resident_copy(m, &gm);
        sseq_de_pairs(*m->st, cp, gm, m->rows(), m->cols(), labels, n_groups, pair_a, pair_b, n_pairs, zeta_quintile, big_count, backend, snoop,
                      sums_in, sums_out, p, p_adj, log2fc, mean_in, mean_out, params);
    });
}
int scanrs_sseq_de_pairs_sharded(scanrs_mat *m, const int16_t *labels, uint32_t n_groups, const uint32_t *pair_a, const uint32_t *pair_b,
                                 uint32_t n_pairs, double zeta_quintile, uint64_t big_count, int backend, const scanrs_snoop *snoop, uint64_t *sums_in,
                                 uint64_t *sums_out, double *p, double *p_adj, double *log2fc, double *mean_in, double *mean_out,
                                 scanrs_sseq_pair_params *params) {
    return guard([&] {
        if (!m || !labels || (n_pairs && (!pair_a || !pair_b)) || !sums_in || !sums_out || !p || !p_adj || !log2fc || !mean_in || !mean_out)
            fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (!(zeta_quintile >= 0.0 && zeta_quintile <= 1.0)) fail(SCANRS_ERR_ARGUMENT, "zeta_quintile must be in [0, 1]");
        CurrentHandle cur(m->st.get());
        bool gm = false;
        SparseCopy &cp = sseq_resident_copy(m, &gm); // refuses a handle sharded over the genes
        m->st->de_shard_tests = m->st->de_shard_allreduces = 0;
        sseq_de_pairs(*m->st, cp, gm, m->rows(), m->cols(), labels, n_groups, pair_a, pair_b, n_pairs, zeta_quintile, big_count, backend, snoop,
                      sums_in, sums_out, p, p_adj, log2fc, mean_in, mean_out, params, true);
    });
}
int scanrs_host_union_median(const double *a, uint64_t n_a, const double *b, uint64_t n_b, double *out) {
    return guard([&] {
        if ((n_a && !a) || (n_b && !b) || !out) fail(SCANRS_ERR_ARGUMENT, "null argument");
        *out = sseq_union_median(a, n_a, b, n_b);
    });
}
} // extern "C"
