// Host logic of merge_clusters (scan-rs/src/merge_clusters.rs, linkage.rs, stats.rs): pdist, nn_chain complete linkage,
// relabel_by_size, the medoids' launch and the merge loop with its two routes to a candidate's DE. The passes over the
// nonzeros, the medians and the tests run on the device (cluster.hip, sseq.hip).
#include "common.hpp"
#include "fixed128.hpp"
#include "shard_exchange.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <set>
#include <vector>

// the reference's host arithmetic is not contracted: fused multiply-adds here would move distances and linkage heights off its bits
#pragma clang fp contract(off)

namespace scanrs {

// ---- linkage.rs -------------------------------------------------------------------------------------------------------------------
void cluster_pdist(const double *x, uint64_t m, uint32_t d, double *out) {
    uint64_t k = 0;
    for (uint64_t i = 0; i < m; i++)
        for (uint64_t j = i + 1; j < m; j++) {
            double s = 0.0;
            for (uint32_t c = 0; c < d; c++) {
                const double t = x[i * d + c] - x[j * d + c];
                s += t * t;
            }
            out[k++] = std::sqrt(s);
        }
}

static inline uint64_t utidx(uint64_t m, uint64_t a, uint64_t b) {
    return a < b ? m * a - (a * (a + 1) / 2) + b - a - 1 : m * b - (b * (b + 1) / 2) + a - b - 1;
}

// sort_by_column(z, 2) and relabel (linkage.rs:160-216), which is also kodama's naming of a dendrogram (hclust_host.cpp): the m - 1
// merges [a, b, distance, .] in discovery order -> rows by (distance, discovery row), the cluster made by sorted row r named m + r,
// the smaller name first, sizes from the union-find
void cluster_sort_relabel(const double *z, uint64_t m, double *z_out) {
    // sort_by_column: rows by (distance, original row)
    std::vector<uint64_t> ord(m - 1);
    for (uint64_t i = 0; i + 1 < m; i++) ord[i] = i;
    std::sort(ord.begin(), ord.end(), [&](uint64_t p, uint64_t q) {
        const double u = z[p * 4 + 2], v = z[q * 4 + 2];
        return u < v || (u == v && p < q);
    });
    // relabel through the union-find
    std::vector<uint64_t> parents(2 * m - 1), usz(2 * m - 1, 1);
    for (uint64_t i = 0; i < 2 * m - 1; i++) parents[i] = i;
    uint64_t next = m;
    auto find = [&](uint64_t i) {
        uint64_t p = i;
        while (parents[i] != i) i = parents[i];
        while (parents[p] != i) {
            p = parents[p];
            parents[p] = i;
        }
        return i;
    };
    for (uint64_t r = 0; r + 1 < m; r++) {
        const double *row = &z[ord[r] * 4];
        const uint64_t pa = find((uint64_t)row[0]), pb = find((uint64_t)row[1]);
        double *o = &z_out[r * 4];
        o[0] = (double)std::min(pa, pb);
        o[1] = (double)std::max(pa, pb);
        o[2] = row[2];
        parents[pa] = next;
        parents[pb] = next;
        usz[next] = usz[pa] + usz[pb];
        o[3] = (double)usz[next];
        next++;
    }
}

// nn_chain (linkage.rs:72-158) with max, sort_by_column(z, 2) and relabel (:160-216)
void cluster_linkage_complete(const double *x, uint64_t m, uint32_t d, double *z_out) {
    if (m == 0) fail(SCANRS_ERR_ARGUMENT, "linkage of no points");
    std::vector<double> dist(m * (m - 1) / 2);
    cluster_pdist(x, m, d, dist.data());
    for (uint64_t i = 0; i < dist.size(); i++)
        if (std::isnan(dist[i])) fail(SCANRS_ERR_ARGUMENT, "a distance between the points is NaN");
    std::vector<double> z((m - 1) * 4, 0.0);
    std::vector<uint64_t> sizes(m, 1), chain(m, 0);
    uint64_t chain_length = 0, a = 0, b = 0;
    double curr_min = 0.0;
    for (uint64_t i = 0; i + 1 < m; i++) {
        if (chain_length == 0) {
            chain_length = 1;
            for (uint64_t j = 0; j < m; j++)
                if (sizes[j] > 0) {
                    chain[0] = j;
                    break;
                }
        }
        for (;;) {
            a = chain[chain_length - 1];
            if (chain_length > 1) {
                b = chain[chain_length - 2];
                curr_min = dist[utidx(m, a, b)];
            } else {
                curr_min = INFINITY;
            }
            for (uint64_t c = 0; c < m; c++) {
                if (sizes[c] == 0 || a == c) continue;
                const double acdist = dist[utidx(m, a, c)];
                if (acdist < curr_min) {
                    curr_min = acdist;
                    b = c;
                }
            }
            if (chain_length > 1 && b == chain[chain_length - 2]) break;
            chain[chain_length] = b;
            chain_length++;
        }
        chain_length -= 2;
        if (a > b) std::swap(a, b);
        const uint64_t asz = sizes[a], bsz = sizes[b];
        z[i * 4 + 0] = (double)a;
        z[i * 4 + 1] = (double)b;
        z[i * 4 + 2] = curr_min;
        z[i * 4 + 3] = (double)(asz + bsz);
        sizes[a] = 0;
        sizes[b] = asz + bsz;
        for (uint64_t j = 0; j < m; j++) {
            if (sizes[j] == 0 || j == b) continue;
            const double ja = dist[utidx(m, j, a)], jb = dist[utidx(m, j, b)];
            dist[utidx(m, j, b)] = std::max(ja, jb); // f64::max (no NaN here)
        }
    }
    cluster_sort_relabel(z.data(), m, z_out);
}

// relabel_by_size (merge_clusters.rs:43-56)
void cluster_relabel_by_size(const int16_t *labels, uint64_t n, int16_t *out) {
    std::map<int16_t, uint64_t> bins;
    for (uint64_t i = 0; i < n; i++) bins[labels[i]]++;
    std::vector<std::pair<int16_t, uint64_t>> hist(bins.begin(), bins.end());
    std::stable_sort(hist.begin(), hist.end(), [](const auto &p, const auto &q) { return p.second > q.second; });
    std::map<int16_t, int16_t> to;
    for (size_t i = 0; i < hist.size(); i++) to[hist[i].first] = (int16_t)i;
    for (uint64_t i = 0; i < n; i++) out[i] = to[labels[i]];
}

// ---- labels ------------------------------------------------------------------------------------------------------------------------
void cluster_check_labels(const int16_t *labels, uint64_t n, uint32_t k) {
    if (k == 0 || k > MERGE_MAX_CLUSTERS) fail(SCANRS_ERR_ARGUMENT, "the number of clusters must be in 1 .. %u", MERGE_MAX_CLUSTERS);
    std::vector<uint8_t> seen(k, 0);
    for (uint64_t c = 0; c < n; c++) {
        if (labels[c] < 0 || labels[c] >= (int)k)
            fail(SCANRS_ERR_ARGUMENT, "label %d of cell %llu is outside 0 .. %u", (int)labels[c], (unsigned long long)c, k - 1);
        seen[labels[c]] = 1;
    }
    for (uint32_t j = 0; j < k; j++)
        if (!seen[j]) fail(SCANRS_ERR_ARGUMENT, "label %u has no cell (labels must be 0 .. K-1, every value present)", j);
}

uint32_t cluster_count_labels(const int16_t *labels, uint64_t n) {
    int mx = -1;
    for (uint64_t c = 0; c < n; c++) {
        if (labels[c] < 0 || labels[c] >= (int)MERGE_MAX_CLUSTERS)
            fail(SCANRS_ERR_ARGUMENT, "label %d of cell %llu is outside 0 .. %u", (int)labels[c], (unsigned long long)c, MERGE_MAX_CLUSTERS - 1);
        mx = std::max(mx, (int)labels[c]);
    }
    cluster_check_labels(labels, n, (uint32_t)(mx + 1));
    return (uint32_t)(mx + 1);
}

// ---- medoids ------------------------------------------------------------------------------------------------------------------------
// key buffer of one column tile: at most 2^25 u64 (256 MB) unless one column alone is larger
static uint32_t medoid_cols_per_tile(uint64_t n, uint32_t d) {
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(d, (uint64_t(1) << 25) / std::max<uint64_t>(1, n)));
}

struct MedoidScratch {
    DevBuf<uint32_t> perm;
    DevBuf<uint64_t> off, len;
    DevBuf<unsigned long long> keys, nan_cell, state, hist;
    DevBuf<double> out;
};

static void medoids_on(hipStream_t s, MedoidScratch &ms, const double *d_scores, uint64_t n, uint32_t ld, uint32_t d, const int16_t *labels,
                       uint32_t k, double *centers) {
    if (n == 0 || d == 0) return;
    // the cells cluster by cluster (a counting sort of the labels)
    std::vector<uint64_t> off(k + 1, 0);
    for (uint64_t c = 0; c < n; c++) off[labels[c] + 1]++;
    for (uint32_t j = 0; j < k; j++) off[j + 1] += off[j];
    std::vector<uint32_t> perm(n);
    {
        std::vector<uint64_t> pos(off.begin(), off.end() - 1);
        for (uint64_t c = 0; c < n; c++) perm[pos[labels[c]]++] = (uint32_t)c;
    }
    const uint32_t cpt = medoid_cols_per_tile(n, d);
    if (ms.perm.n < n) ms.perm.alloc(n);
    if (ms.off.n < k + 1) ms.off.alloc(k + 1);
    if (ms.keys.n < n * cpt) ms.keys.alloc(n * cpt);
    if (ms.nan_cell.n < 1) ms.nan_cell.alloc(1);
    if (ms.out.n < (size_t)k * d) ms.out.alloc((size_t)k * d);
    h2d(ms.perm.p, perm.data(), n, s);
    h2d(ms.off.p, off.data(), k + 1, s);
    launch_medoids(s, d_scores, n, ld, d, ms.perm.p, ms.off.p, k, ms.keys.p, cpt, ms.nan_cell.p, ms.out.p);
    unsigned long long nan_cell = 0;
    SCANRS_D2H(&nan_cell, ms.nan_cell.p, 8, s);
    SCANRS_D2H(centers, ms.out.p, (size_t)k * d * 8, s);
    SCANRS_SYNC(s);
    if (nan_cell != ~0ull) fail(SCANRS_ERR_ARGUMENT, "the scores of cell %llu hold a NaN", nan_cell);
}

// The medoids of a sharded handle: d_scores holds the rank's own cells [cr.begin, cr.begin + cr.n_local), labels span the
// whole matrix. Every rank walks the same column tiles, pair tiles and rounds (they depend on the global sizes only), so the exchange
// steps pair up; the centers come out complete on every rank.
static void medoids_dist(Storage &st, MedoidScratch &ms, const double *d_scores, const CellRange &cr, uint32_t ld, uint32_t d,
                         const int16_t *labels, uint32_t k, double *centers) {
    if (cr.global == 0 || d == 0) return;
    const hipStream_t s = st.stream;
    const uint64_t n = cr.n_local;
    // the clusters' global sizes (the wanted ranks), and this rank's cells cluster by cluster
    std::vector<uint64_t> len(k, 0), off(k + 1, 0);
    for (uint64_t c = 0; c < cr.global; c++) len[labels[c]]++;
    const int16_t *lab = labels + cr.begin;
    for (uint64_t c = 0; c < n; c++) off[lab[c] + 1]++;
    for (uint32_t j = 0; j < k; j++) off[j + 1] += off[j];
    std::vector<uint32_t> perm(std::max<uint64_t>(1, n));
    {
        std::vector<uint64_t> pos(off.begin(), off.end() - 1);
        for (uint64_t c = 0; c < n; c++) perm[pos[lab[c]]++] = (uint32_t)c;
    }
    const uint32_t cpt = medoid_cols_per_tile(cr.global, d); // from the global count: the same tiles on every rank
    const uint32_t hist_pairs = (uint32_t)std::min<uint64_t>(MEDOID_HIST_PAIRS, (uint64_t)k * cpt);
    ShardExchange ex{st, st.de_shard_allreduces}; // (the counter of the DE calls, which the merge loop goes on to make)
    if (ms.perm.n < perm.size()) ms.perm.alloc(perm.size());
    if (ms.off.n < k + 1) ms.off.alloc(k + 1);
    if (ms.len.n < k) ms.len.alloc(k);
    if (ms.keys.n < std::max<uint64_t>(1, n * cpt)) ms.keys.alloc(std::max<uint64_t>(1, n * cpt));
    if (ms.state.n < (size_t)k * cpt * 4) ms.state.alloc((size_t)k * cpt * 4);
    if (ms.hist.n < (size_t)hist_pairs * 512) ms.hist.alloc((size_t)hist_pairs * 512);
    if (ms.nan_cell.n < 1) ms.nan_cell.alloc(1);
    if (ms.out.n < (size_t)k * d) ms.out.alloc((size_t)k * d);
    h2d(ms.perm.p, perm.data(), n, s);
    h2d(ms.off.p, off.data(), k + 1, s);
    h2d(ms.len.p, len.data(), k, s);
    SCANRS_HIP(hipMemsetAsync(ms.nan_cell.p, 0xFF, 8, s));
    for (uint32_t j0 = 0; j0 < d; j0 += cpt) {
        const uint32_t jt = std::min(cpt, d - j0), n_pairs = k * jt;
        launch_medoid_keys(s, d_scores, n, ld, j0, jt, ms.perm.p, ms.keys.p, ms.nan_cell.p);
        launch_medoid_dist_init(s, ms.len.p, k, jt, ms.state.p);
        for (int shift = 56; shift >= 0; shift -= 8)
            for (uint32_t p0 = 0; p0 < n_pairs; p0 += hist_pairs) {
                const uint32_t np = std::min(hist_pairs, n_pairs - p0);
                launch_medoid_dist_hist(s, ms.keys.p, n, ms.off.p, k, p0, np, shift, ms.state.p, ms.hist.p);
                ex.sum(ms.hist.p, (uint64_t)np * 512);
                launch_medoid_dist_pick(s, ms.hist.p, p0, np, shift, ms.state.p);
            }
        launch_medoid_dist_finish(s, ms.state.p, ms.len.p, k, j0, jt, ms.out.p, d);
    }
    // the first cell holding a NaN: every rank's own first one (+ 1; 0 = none)
    unsigned long long nan_local = 0;
    SCANRS_D2H(&nan_local, ms.nan_cell.p, 8, s);
    SCANRS_SYNC(s);
    const unsigned long long nan_mine = nan_local == ~0ull ? 0ull : cr.begin + nan_local + 1;
    const std::vector<unsigned long long> slots = ex.gather_host(&nan_mine, 1);
    SCANRS_D2H(centers, ms.out.p, (size_t)k * d * 8, s);
    SCANRS_SYNC(s);
    unsigned long long nan_cell = ~0ull;
    for (unsigned long long v : slots)
        if (v) nan_cell = std::min(nan_cell, v - 1);
    if (nan_cell != ~0ull) fail(SCANRS_ERR_ARGUMENT, "the scores of cell %llu hold a NaN", nan_cell);
}

void cluster_medoids(hipStream_t s, const double *d_scores, uint64_t n, uint32_t ld, uint32_t d, const int16_t *labels, uint32_t k, double *centers) {
    if (ld < d) fail(SCANRS_ERR_ARGUMENT, "ld must be at least d");
    if (n > 0xFFFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "at most 2^32 - 1 cells");
    if (n == 0 && k == 0) return;
    cluster_check_labels(labels, n, k);
    MedoidScratch ms;
    medoids_on(s, ms, d_scores, n, ld, d, labels, k, centers);
}

// ---- the merge loop (merge_clusters.rs:59-138) -------------------------------------------------------------------------------------
namespace {

constexpr double ADJUSTED_P_VALUE_THRESHOLD = 0.05; // merge_clusters.rs:10
constexpr double ZETA_QUINTILE = 0.995;             // compute_sseq_params(.., None) (diff_exp.rs:17)
constexpr uint64_t BIG_COUNT = 900;                 // sseq_differential_expression(.., None) (diff_exp.rs:15)

// one cluster of the fused route: its sums from the grouped pass and what its candidates need of its cells
struct FusedCluster {
    std::vector<unsigned long long> acc; // genes x 5: Σ x, Σ x/u (lo, hi), Σ (x/u)² (lo, hi)
    std::vector<double> totals;          // u_c of its cells, sorted
    unsigned long long u_sum = 0;        // Σ u_c
    U128 inv{0, 0};                      // Σ 1/u_c over u_c > 0, fixed point
};

// percentile_of_sorted(.., 50) (stat.rs:140-162) of the union of two sorted lists, selecting the two ranks it reads
double union_median(const std::vector<double> &a, const std::vector<double> &b) {
    const uint64_t len = a.size() + b.size();
    auto kth = [&](uint64_t k) { // k-th smallest (0-based) of the union
        uint64_t lo = k > b.size() ? k - b.size() : 0, hi = std::min<uint64_t>(k, a.size());
        while (lo < hi) { // the number i of elements taken from a
            const uint64_t i = (lo + hi) / 2, j = k - i;
            if (j > 0 && i < a.size() && b[j - 1] > a[i])
                lo = i + 1;
            else
                hi = i;
        }
        const uint64_t i = lo, j = k - i;
        if (i >= a.size()) return b[j];
        if (j >= b.size()) return a[i];
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

struct Candidate {
    uint64_t n_de = 0;
    double min_p = NAN;
};

void summarize(const std::vector<double> &padj, Candidate &cd) {
    for (double q : padj) {
        if (q < ADJUSTED_P_VALUE_THRESHOLD) cd.n_de++;
        if (!std::isnan(q) && !(cd.min_p <= q)) cd.min_p = q;
    }
}

} // namespace

void merge_clusters_run(Storage &st, const SparseCopy &cp, bool gene_major, uint64_t genes, uint64_t cells, const double *d_scores, uint32_t ld,
                        uint32_t d, const int16_t *labels_in, int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace,
                        bool collective) {
    if (trace) trace->n_candidates = trace->n_rounds = trace->n_merges = trace->n_passes = 0;
    // a sharded handle (collective only): the copy and d_scores hold the cells [cr.begin, cr.begin + cr.n_local); `cells` is from
    // here on the whole matrix: labels span it and the loop below runs replicated on every rank, on identical data
    const CellRange cr = collective ? cell_range(st, cells) : CellRange{0, cells, cells};
    const uint64_t cells_local = cr.n_local;
    const bool dist = collective && st.shard.active();
    cells = cr.global;
    uint64_t shard_tests = 0;
    if (cells == 0) return;
    if (ld < d) fail(SCANRS_ERR_ARGUMENT, "ld must be at least d");
    if (cells > 0xFFFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "at most 2^32 - 1 cells");
    std::vector<int16_t> labels(labels_in, labels_in + cells);
    uint32_t k = cluster_count_labels(labels.data(), cells);
    const hipStream_t s = st.stream;
    uint64_t passes = 0;

    // the fused route's one pass: per-cell totals, then per (cluster, gene) sums of the original clustering
    const bool fused = st.opt.merge_fused != 0;
    std::vector<FusedCluster> fc;
    std::vector<double> cell_tot;
    const double scale = fixed_scale((double)cells); // Σ x/u_c, Σ (x/u_c)², Σ 1/u_c of a cluster: at most one per cell
    if (fused) {
        unsigned long long *d_tot = st.scratch.get<unsigned long long>("merge_totals", cells + 1);
        if (dist) SCANRS_HIP(hipMemsetAsync(d_tot, 0, cells * 8, s)); // the other ranks' slices
        launch_sseq_cell_totals(st, cp, gene_major, cells_local, d_tot + cr.begin);
        if (dist) ShardExchange{st, st.de_shard_allreduces}.sum(d_tot, cells); // one contributor per element: the sum is a copy
        passes++;
        int16_t *d_lab = st.scratch.get<int16_t>("merge_labels", std::max<uint64_t>(1, cells_local));
        h2d(d_lab, labels.data() + cr.begin, cells_local, s);
        DevBuf<unsigned long long> d_acc(std::max<uint64_t>(1, (uint64_t)k * genes * 5));
        passes += launch_merge_pass(st, cp, gene_major, genes, d_lab, k, d_tot + cr.begin, scale, scale, d_acc.p);
        if (dist) sseq_reduce_group_acc(st, d_acc.p, (uint64_t)k * genes); // every rank now holds the unsharded integers
        std::vector<unsigned long long> tot(cells), acc((uint64_t)k * genes * 5);
        SCANRS_D2H(tot.data(), d_tot, cells * 8, s);
        if (genes) SCANRS_D2H(acc.data(), d_acc.p, acc.size() * 8, s);
        SCANRS_SYNC(s);
        fc.resize(k);
        cell_tot.resize(cells);
        for (uint32_t j = 0; j < k; j++) fc[j].acc.assign(acc.begin() + (uint64_t)j * genes * 5, acc.begin() + (uint64_t)(j + 1) * genes * 5);
        for (uint64_t c = 0; c < cells; c++) {
            FusedCluster &f = fc[labels[c]];
            cell_tot[c] = (double)tot[c];
            f.totals.push_back((double)tot[c]);
            f.u_sum += tot[c];
            if (tot[c]) add128(f.inv, to_fixed(1.0 / (double)tot[c], scale));
        }
        for (auto &f : fc) std::sort(f.totals.begin(), f.totals.end());
    }

    // each current cluster as its set of original clusters (the cells' partition): the key of seen_pairs
    std::vector<std::vector<uint16_t>> members(k);
    for (uint32_t j = 0; j < k; j++) members[j] = {(uint16_t)j};
    std::set<std::pair<std::vector<uint16_t>, std::vector<uint16_t>>> seen_pairs;
    std::vector<uint64_t> n_cells(k, 0);
    for (uint64_t c = 0; c < cells; c++) n_cells[labels[c]]++;

    MedoidScratch ms;
    std::vector<double> centers, z, mean(genes), var(genes), phi_mm(genes), phi(genes), sf(cells);
    std::vector<uint8_t> use(genes);
    std::vector<uint64_t> sa(genes), sb(genes), union_idx;
    std::vector<double> p(genes), padj(genes), l2(genes), mi(genes), mo(genes);
    std::vector<int16_t> lab3(cells);
    uint64_t n_cand = 0, n_rounds = 0, n_merges = 0;

    // the literal route: compute_sseq_params on the union, then sseq_differential_expression(group0, group1), as the reference calls them
    auto literal = [&](uint32_t l0, uint32_t l1, Candidate &cd) {
        union_idx.clear();
        for (uint64_t c = 0; c < cells; c++) {
            lab3[c] = labels[c] == (int)l0 ? 0 : labels[c] == (int)l1 ? 1 : -1;
            if (lab3[c] >= 0) union_idx.push_back(c);
        }
        double zh = 0.0, dl = 0.0;
        sseq_params(st, cp, gene_major, genes, cells_local, ZETA_QUINTILE, union_idx.data(), union_idx.size(), nullptr, sf.data(), mean.data(), var.data(),
                    use.data(), phi_mm.data(), &zh, &dl, phi.data());
        std::vector<uint64_t> si(genes * 1), so(genes * 1);
        sseq_de_matrix(st, cp, gene_major, genes, cells_local, lab3.data(), 2, 1, sf.data(), mean.data(), phi.data(), use.data(), BIG_COUNT, nullptr,
                       si.data(), so.data(), p.data(), padj.data(), l2.data(), mi.data(), mo.data());
        passes += 3 + st.sseq_moment_walks; // totals, max count, moments (the class walk first where every gene gets its quantum), group sums
        shard_tests += st.de_shard_tests;
        summarize(padj, cd);
    };
    // the fused route: the union's params and both sides' sums from the clusters' accumulators (O(genes)), then the tests
    auto from_sums = [&](uint32_t l0, uint32_t l1, Candidate &cd) {
        const FusedCluster &A = fc[l0], &B = fc[l1];
        const double m_s = union_median(A.totals, B.totals);
        if (m_s == 0.0) return literal(l0, l1, cd); // size factors are not finite: the literal route keeps that case's handling
        // a cell total so large that a count of 1 in that cell would not keep its bits under the pass's quantum (fixed128.hpp): the
        // literal route's moments choose a quantum per gene
        const double top = std::max(A.totals.empty() ? 0.0 : A.totals.back(), B.totals.empty() ? 0.0 : B.totals.back());
        if (!fixed_totals_quantum_keeps((unsigned long long)top, scale)) return literal(l0, l1, cd);
        const double n_s = (double)(n_cells[l0] + n_cells[l1]);
        U128 inv = A.inv;
        add128(inv, B.inv);
        const double sum_sf = m_s * from_fixed(&inv.lo, scale); // Σ 1/sf_c = m_S Σ 1/u_c
        for (uint64_t g = 0; g < genes; g++) {
            const unsigned long long *a = &A.acc[g * 5], *b = &B.acc[g * 5];
            U128 s1{a[1], a[2]}, s2{a[3], a[4]};
            add128(s1, U128{b[1], b[2]});
            add128(s2, U128{b[3], b[4]});
            // Σ x/sf = m_S Σ x/u_c, Σ (x/sf)² = m_S² Σ (x/u_c)²; V[X] = E[X²] - E[X]² (sqz/src/mat.rs:333-380)
            mean[g] = m_s * from_fixed(&s1.lo, scale) / n_s;
            var[g] = m_s * m_s * from_fixed(&s2.lo, scale) / n_s - mean[g] * mean[g];
            sa[g] = a[0];
            sb[g] = b[0];
        }
        double zh = 0.0, dl = 0.0;
        sseq_params_from_moments(mean.data(), var.data(), genes, sum_sf, n_s, (double)genes, ZETA_QUINTILE, use.data(), phi_mm.data(), &zh, &dl,
                                 phi.data());
        const double fa = (double)A.u_sum / m_s, fb = (double)B.u_sum / m_s;
        if (dist) { // the tests split over the ranks by gene, gathered by one exchange (§7g)
            sseq_de_sums_strided(s, genes, 1, sa.data(), sb.data(), &fa, &fb, mean.data(), phi.data(), use.data(), 1, 0, BIG_COUNT, nullptr, p.data(),
                                 padj.data(), l2.data(), mi.data(), mo.data(), SCANRS_NB_EXACT_LOGSPACE, &st);
            shard_tests += st.de_shard_tests;
        } else {
            sseq_de_sums(s, genes, 1, sa.data(), sb.data(), &fa, &fb, mean.data(), phi.data(), use.data(), BIG_COUNT, nullptr, p.data(), padj.data(),
                         l2.data(), mi.data(), mo.data());
        }
        summarize(padj, cd);
    };

    for (;;) {
        n_rounds++;
        // bins are the labels 0 .. k-1 in order; centers row i belongs to label i
        centers.assign((size_t)k * d, 0.0);
        if (dist)
            medoids_dist(st, ms, d_scores, cr, ld, d, labels.data(), k, centers.data());
        else
            medoids_on(s, ms, d_scores, cells, ld, d, labels.data(), k, centers.data());
        z.assign((size_t)(k - 1) * 4, 0.0);
        cluster_linkage_complete(centers.data(), k, d, z.data());
        const double max_label = (double)(k - 1);
        bool any_merged = false;
        for (uint32_t i = 0; i + 1 < k; i++) {
            if (!(z[i * 4] <= max_label && z[i * 4 + 1] <= max_label)) continue;
            const uint32_t leaf0 = (uint32_t)z[i * 4], leaf1 = (uint32_t)z[i * 4 + 1];
            if (!seen_pairs.insert({members[leaf0], members[leaf1]}).second) continue;
            // CancelProgress::check (snoop/src/lib.rs:37-58) before every candidate
            snoop_check(snoop);
            Candidate cd;
            if (fused)
                from_sums(leaf0, leaf1, cd);
            else
                literal(leaf0, leaf1, cd);
            if (trace && n_cand < trace->capacity) {
                trace->leaf0[n_cand] = (int16_t)leaf0;
                trace->leaf1[n_cand] = (int16_t)leaf1;
                trace->n_de[n_cand] = cd.n_de;
                trace->min_p_adj[n_cand] = cd.min_p;
            }
            n_cand++;
            if (cd.n_de == 0) {
                // cells of leaf1 take leaf0, labels above leaf1 move down by one
                for (auto &l : labels) {
                    if (l == (int)leaf1)
                        l = (int16_t)leaf0;
                    else if (l > (int)leaf1)
                        l--;
                }
                std::vector<uint16_t> mm;
                std::merge(members[leaf0].begin(), members[leaf0].end(), members[leaf1].begin(), members[leaf1].end(), std::back_inserter(mm));
                members[leaf0] = std::move(mm);
                members.erase(members.begin() + leaf1);
                n_cells[leaf0] += n_cells[leaf1];
                n_cells.erase(n_cells.begin() + leaf1);
                if (fused) {
                    FusedCluster &A = fc[leaf0], &B = fc[leaf1];
                    for (uint64_t g = 0; g < genes; g++) {
                        unsigned long long *a = &A.acc[g * 5];
                        const unsigned long long *b = &B.acc[g * 5];
                        a[0] += b[0];
                        U128 s1{a[1], a[2]}, s2{a[3], a[4]};
                        add128(s1, U128{b[1], b[2]});
                        add128(s2, U128{b[3], b[4]});
                        a[1] = s1.lo, a[2] = s1.hi, a[3] = s2.lo, a[4] = s2.hi;
                    }
                    std::vector<double> t;
                    t.reserve(A.totals.size() + B.totals.size());
                    std::merge(A.totals.begin(), A.totals.end(), B.totals.begin(), B.totals.end(), std::back_inserter(t));
                    A.totals = std::move(t);
                    A.u_sum += B.u_sum;
                    add128(A.inv, B.inv);
                    fc.erase(fc.begin() + leaf1);
                }
                k--;
                n_merges++;
                any_merged = true;
                break;
            }
        }
        if (!any_merged) break;
    }
    cluster_relabel_by_size(labels.data(), cells, labels_out);
    if (trace) {
        trace->n_candidates = n_cand;
        trace->n_rounds = n_rounds;
        trace->n_merges = n_merges;
        trace->n_passes = passes;
    }
    if (dist) st.de_shard_tests = shard_tests;
}

} // namespace scanrs

// ---- the extern "C" entry points ------------------------------------------------------------------------------------------------------
using namespace scanrs;
extern "C" {
int scanrs_host_pdist(const double *x, uint64_t m, uint32_t d, double *out) {
    return guard([&] {
        if (m > 1 && (!out || (!x && d))) fail(SCANRS_ERR_ARGUMENT, "null argument");
        cluster_pdist(x, m, d, out);
    });
}
int scanrs_host_linkage_complete(const double *x, uint64_t m, uint32_t d, double *z) {
    return guard([&] {
        if ((!x && d) || (!z && m > 1)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        cluster_linkage_complete(x, m, d, z);
    });
}
int scanrs_host_relabel_by_size(const int16_t *labels, uint64_t n, int16_t *out) {
    return guard([&] {
        if (n && (!labels || !out)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        cluster_relabel_by_size(labels, n, out);
    });
}
int scanrs_cluster_medoids(const double *pca, uint64_t n, uint32_t ld, uint32_t d, const int16_t *labels, uint32_t k, double *centers) {
    return guard([&] {
        if (n && (!pca || !labels || (!centers && d))) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (ld < d) fail(SCANRS_ERR_ARGUMENT, "ld must be at least d");
        need_device();
        DevBuf<double> d_pca(std::max<uint64_t>(1, n * ld));
        if (n) SCANRS_HIP(hipMemcpyAsync(d_pca.p, pca, n * ld * 8, hipMemcpyHostToDevice, nullptr));
        cluster_medoids(nullptr, d_pca.p, n, ld, d, labels, k, centers);
    });
}
int scanrs_cluster_medoids_device(const double *d_pca, uint64_t n, uint32_t ld, uint32_t d, const int16_t *labels, uint32_t k, double *centers) {
    return guard([&] {
        if (n && (!d_pca || !labels || (!centers && d))) fail(SCANRS_ERR_ARGUMENT, "null argument");
        need_device();
        cluster_medoids(nullptr, d_pca, n, ld, d, labels, k, centers);
    });
}
int scanrs_merge_clusters(scanrs_mat *m, const double *pca, int pca_is_device, uint32_t ld, uint32_t d, const int16_t *labels,
                          int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        const uint64_t cells = m->cols();
        if (cells && (!pca || !labels || !labels_out)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (trace && trace->capacity && (!trace->leaf0 || !trace->leaf1 || !trace->n_de || !trace->min_p_adj))
            fail(SCANRS_ERR_ARGUMENT, "trace arrays are null");
        if (ld < d) fail(SCANRS_ERR_ARGUMENT, "ld must be at least d");
        CurrentHandle cur(m->st.get());
        sseq_refuse_sharded(m, "merge_clusters");
        bool gm = false;
        SparseCopy &cp = sseq_resident_copy(m, &gm);
        Storage &st = *m->st;
        DevBuf<double> d_pca;
        const double *scores = pca;
        if (!pca_is_device && cells) {
            d_pca.alloc(cells * ld);
            SCANRS_HIP(hipMemcpyAsync(d_pca.p, pca, cells * ld * 8, hipMemcpyHostToDevice, st.stream));
            scores = d_pca.p;
        }
        merge_clusters_run(st, cp, gm, m->rows(), cells, scores, ld, d, labels, labels_out, snoop, trace);
    });
}
int scanrs_merge_clusters_sharded(scanrs_mat *m, const double *pca, int pca_is_device, uint32_t ld, uint32_t d, const int16_t *labels,
                                  int16_t *labels_out, const scanrs_snoop *snoop, scanrs_merge_trace *trace) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        CurrentHandle cur(m->st.get());
        bool gm = false;
        SparseCopy &cp = sseq_resident_copy(m, &gm); // refuses a handle sharded over the genes
        Storage &st = *m->st;
        const CellRange cr = cell_range(st, m->cols());
        if (cr.global && (!pca || !labels || !labels_out)) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (trace && trace->capacity && (!trace->leaf0 || !trace->leaf1 || !trace->n_de || !trace->min_p_adj))
            fail(SCANRS_ERR_ARGUMENT, "trace arrays are null");
        if (ld < d) fail(SCANRS_ERR_ARGUMENT, "ld must be at least d");
        st.de_shard_tests = st.de_shard_allreduces = 0;
        // host scores span the whole matrix and only this rank's rows go to the device; device scores are the rank's own rows already
        DevBuf<double> d_pca;
        const double *scores = pca;
        if (!pca_is_device && cr.global) {
            d_pca.alloc(std::max<uint64_t>(1, cr.n_local * ld));
            if (cr.n_local) SCANRS_HIP(hipMemcpyAsync(d_pca.p, pca + cr.begin * ld, cr.n_local * ld * 8, hipMemcpyHostToDevice, st.stream));
            scores = d_pca.p;
        }
        merge_clusters_run(st, cp, gm, m->rows(), cr.n_local, scores, ld, d, labels, labels_out, snoop, trace, true);
    });
}
int scanrs_cluster_medoids_sharded(scanrs_mat *m, const double *pca, int pca_is_device, uint32_t ld, uint32_t d, const int16_t *labels,
                                   uint32_t k, double *centers) {
    return guard([&] {
        if (!m) fail(SCANRS_ERR_ARGUMENT, "null handle");
        CurrentHandle cur(m->st.get());
        bool gm = false;
        (void)sseq_resident_copy(m, &gm); // refuses a handle sharded over the genes
        Storage &st = *m->st;
        const CellRange cr = cell_range(st, m->cols());
        if (cr.global && (!pca || !labels || (!centers && d))) fail(SCANRS_ERR_ARGUMENT, "null argument");
        if (ld < d) fail(SCANRS_ERR_ARGUMENT, "ld must be at least d");
        if (cr.global > 0xFFFFFFFFull) fail(SCANRS_ERR_ARGUMENT, "at most 2^32 - 1 cells");
        if (cr.global == 0 && k == 0) return;
        cluster_check_labels(labels, cr.global, k);
        st.de_shard_tests = st.de_shard_allreduces = 0;
        DevBuf<double> d_pca;
        const double *scores = pca;
        if (!pca_is_device && cr.global) {
            d_pca.alloc(std::max<uint64_t>(1, cr.n_local * ld));
            if (cr.n_local) SCANRS_HIP(hipMemcpyAsync(d_pca.p, pca + cr.begin * ld, cr.n_local * ld * 8, hipMemcpyHostToDevice, st.stream));
            scores = d_pca.p;
        }
        MedoidScratch ms;
        if (st.shard.active())
            medoids_dist(st, ms, scores, cr, ld, d, labels, k, centers);
        else
            medoids_on(st.stream, ms, scores, cr.global, ld, d, labels, k, centers);
    });
}
} // extern "C"
