"""CPU restatements of batched pairwise DE with per-pair sSeq parameters (scanrs_sseq_de_pairs), no device.

Test j of a call is, in the reference, `compute_sseq_params(mat, zeta, Some(A ∪ B), None)` (diff_exp.rs:458-490) followed by the DE of
A against B (diff_exp.rs:125-161), the shape of merge_clusters.rs' candidates. Two restatements of it:

  literal_pair   those two calls through tests/sseq_ref.py
  fused_pair     the library's route: per (group, gene) Σ x and Σ x/u_c, Σ (x/u_c)² as exact Python integers in the library's
                 fixed-point quantum (u_c the cell's total), combined per pair through sf_c = u_c / m_S, m_S the interpolated
                 median total of the union

and the seeded case generator both test files share."""
from __future__ import annotations

import math

import numpy as np
from scipy import sparse

import sseq_ratio_ref as rref
import sseq_ref as ref

LOGSPACE, RATIO = 0, 1
ZETA = 0.995
# (seed, genes, cells, conditions besides the control): the gene counts straddle the wave (63, 65) and the workgroup (257) of the
# per-pair kernels; 1 and 2 genes are the degenerate ends of the (G - 1), (G - 2) denominators of delta
CASES = [(11, 1, 600, 5), (12, 2, 700, 6), (13, 63, 900, 6), (14, 65, 1200, 7), (15, 257, 1500, 8)]


def make_case(seed, genes, cells, n_cond):
    """genes x cells counts (scipy CSR, uint32), labels and pairs. Gamma-rated genes with geometric counts; five hot Poisson(40)
    genes (both sums of a large pair pass big_count = 900: the asymptotic branch) and an all-zero gene where the gene count allows;
    5 % of the cells labelled -1; group 0 (the control) holds half the cells; the last two groups are a singleton and a 3-cell
    condition. Pairs: every condition against the control, the control against condition 1, and the singleton against the 3 cells.
    No union of a pair has a median total of 0 (that route has its own tests)."""
    rng = np.random.default_rng(seed)
    rate = rng.gamma(0.6, 2.0, genes) + (4.0 if genes < 16 else 0.02)  # few genes: high rates keep the totals off 0
    depth = rng.uniform(0.5, 2.0, cells)
    mean = rate[:, None] * depth[None, :]
    m = rng.geometric(1.0 / (1.0 + mean)) - 1
    if genes >= 16:
        m[:5] = rng.poisson(40.0, (5, cells))
        m[5] = 0
    n_groups = n_cond + 1
    labels = np.full(cells, -1, dtype=np.int16)
    order = rng.permutation(cells)
    n_out = cells // 20
    rest = order[n_out:]
    half = cells // 2
    labels[rest[:half]] = 0
    labels[rest[half]] = n_groups - 2
    labels[rest[half + 1:half + 4]] = n_groups - 1
    tail = rest[half + 4:]
    labels[tail] = 1 + rng.integers(0, n_cond - 2, len(tail))
    pairs = [(g, 0) for g in range(1, n_groups)] + [(0, 1), (n_groups - 2, n_groups - 1)]
    mat = sparse.csr_matrix(m.astype(np.uint32))
    tot = np.asarray(mat.sum(axis=0)).ravel()
    for a, b in pairs:
        assert ref.median(tot[(labels == a) | (labels == b)].astype(np.float64)) > 0.0, "a union with a median total of 0: pick another seed"
    return dict(mat=mat, labels=labels, n_groups=n_groups, pairs=pairs, genes=genes, cells=cells)


# ---- the tests of one pair ----------------------------------------------------------------------------------------------------------
def exact_test(x_a, x_b, sf_a, sf_b, mu, phi, backend):
    """The exact branch as the library runs it: LogSpace (dist.rs:74-118), or Ratio (dist.rs:155-215) where the device
    partitions the test and LogSpace elsewhere (include/scanrs_amd.h, scanrs_sseq_de_backend). A NaN dispersion gives NaN."""
    if x_a + x_b != 0 and math.isnan(phi):
        return math.nan
    if backend == RATIO and not rref.degenerate(x_a, x_b, sf_a, sf_b, phi) and rref.in_ratio_partition(x_a, x_b, sf_a, sf_b, mu, phi):
        return rref.nb_exact_test_ratio(x_a, x_b, sf_a, sf_b, mu, phi)
    return ref.nb_exact_test(x_a, x_b, sf_a, sf_b, mu, phi)


def de_from_sums(sums_a, sums_b, sf_a, sf_b, params, big_count=ref.BIG_COUNT_DEFAULT, backend=LOGSPACE):
    """diff_exp.rs:177-300 with the exact test's backend."""
    sums_a, sums_b = np.asarray(sums_a, dtype=np.uint64), np.asarray(sums_b, dtype=np.uint64)
    mu, phi, use = params["gene_means"], params["gene_phi"], params["use_genes"]
    p = np.zeros(len(sums_a))
    exact = np.zeros(len(sums_a), dtype=bool)
    for g in range(len(sums_a)):
        a, b = int(sums_a[g]), int(sums_b[g])
        if use[g] and a > big_count and b > big_count:
            p[g] = ref.nb_asymptotic_test(a, b, sf_a, sf_b, mu[g], phi[g])
        else:
            p[g] = exact_test(a, b, sf_a, sf_b, float(mu[g]), float(phi[g]), backend)
            exact[g] = True
    padj = p.copy()
    idx = np.flatnonzero(use)
    padj[idx] = ref.adjusted_pvalue_bh(p[idx])
    with np.errstate(divide="ignore", invalid="ignore"):
        l2 = np.log2((1 + sums_a).astype(np.float64) / (1.0 + sf_a)) - np.log2((1 + sums_b).astype(np.float64) / (1.0 + sf_b))
        mi = np.zeros(len(p)) if sf_a == 0 else sums_a.astype(np.float64) / sf_a
        mo = np.zeros(len(p)) if sf_b == 0 else sums_b.astype(np.float64) / sf_b
    return dict(sums_in=sums_a, sums_out=sums_b, p_values=p, adjusted_p_values=padj, log2_fold_change=l2, normalized_mean_in=mi,
                normalized_mean_out=mo, exact=exact, size_factor_a=sf_a, size_factor_b=sf_b)


def literal_pair(mat, labels, a, b, zeta=ZETA, big_count=ref.BIG_COUNT_DEFAULT, backend=LOGSPACE):
    """compute_sseq_params on the sorted union, then A against B: (params, result)."""
    labels = np.asarray(labels)
    ca, cb = np.flatnonzero(labels == a), np.flatnonzero(labels == b)
    union = np.sort(np.concatenate([ca, cb]))
    with np.errstate(divide="ignore", invalid="ignore"):
        prm = ref.compute_sseq_params(mat, zeta, cell_indices=union)
    csc = sparse.csc_matrix(mat)
    sf = prm["size_factors"]
    fa = 0.0
    for i in ca:
        fa += sf[i]
    fb = 0.0
    for i in cb:
        fb += sf[i]
    sa = np.asarray(csc[:, ca].sum(axis=1), dtype=np.uint64).ravel()
    sb = np.asarray(csc[:, cb].sum(axis=1), dtype=np.uint64).ravel()
    return prm, de_from_sums(sa, sb, fa, fb, prm, big_count, backend)


# ---- the fused route ----------------------------------------------------------------------------------------------------------------
def fixed_scale_exp(bound):
    """fixed128.hpp's fixed_scale: the exponent E of the quantum 2^-E, bound * 2^E < 2^124."""
    return 124 - (math.frexp(float(bound))[1] - 1) - 1


def _to_fixed(t, e):
    """to_fixed: t (float64 array) in quanta of 2^-e, rounded once, half to even, as exact Python integers."""
    y = np.ldexp(t, e)
    return [int(v) for v in np.rint(y)]


def _from_fixed(s, e):
    """from_fixed: the two u64 words to f64, added, over the scale."""
    return math.ldexp(float(s >> 64) * 18446744073709551616.0 + float(s & 0xFFFFFFFFFFFFFFFF), -e)


class GroupSums:
    """What the two passes leave per group: sorted totals, Σ u, Σ 1/u, and per gene Σ x, Σ x/u, Σ (x/u)² (integers)."""

    def __init__(self, mat, labels, n_groups):
        coo = sparse.coo_matrix(mat)
        self.genes, self.cells = mat.shape
        labels = np.asarray(labels)
        self.e = fixed_scale_exp(self.cells)
        tot = np.asarray(sparse.csc_matrix(mat).sum(axis=0)).ravel().astype(np.int64)
        keep = (labels[coo.col] >= 0) & (coo.data > 0)
        row, col, x = coo.row[keep], coo.col[keep], coo.data[keep].astype(np.float64)
        t = x / tot[col].astype(np.float64)
        flat = labels[col].astype(np.int64) * self.genes + row
        n = n_groups * self.genes
        self.x = np.zeros(n, dtype=object)
        self.s1 = np.zeros(n, dtype=object)
        self.s2 = np.zeros(n, dtype=object)
        np.add.at(self.x, flat, np.array([int(v) for v in coo.data[keep]], dtype=object))
        np.add.at(self.s1, flat, np.array(_to_fixed(t, self.e), dtype=object))
        np.add.at(self.s2, flat, np.array(_to_fixed(t * t, self.e), dtype=object))
        self.totals, self.u_sum, self.inv = [], [], []
        for g in range(n_groups):
            u = np.sort(tot[labels == g])
            self.totals.append(u)
            self.u_sum.append(int(u.sum()))
            pos = u[u > 0].astype(np.float64)
            self.inv.append(sum(_to_fixed(1.0 / pos, self.e)))

    def col(self, arr, g):
        return arr[g * self.genes:(g + 1) * self.genes]


def fused_pair(gs, a, b, zeta=ZETA, big_count=ref.BIG_COUNT_DEFAULT, backend=LOGSPACE):
    """The pair's parameters from the two groups' sums (cluster_host.cpp's from_sums), then the tests: (params, result).
    None when the union's median total is 0 (the library takes the literal route)."""
    ua, ub = gs.totals[a], gs.totals[b]
    m_s = ref.median(np.concatenate([ua, ub]).astype(np.float64))
    if m_s == 0.0:
        return None
    n_s = float(len(ua) + len(ub))
    sum_sf = m_s * _from_fixed(gs.inv[a] + gs.inv[b], gs.e)
    s1, s2 = gs.col(gs.s1, a) + gs.col(gs.s1, b), gs.col(gs.s2, a) + gs.col(gs.s2, b)
    mean = np.array([m_s * _from_fixed(int(v), gs.e) / n_s for v in s1])
    var = np.array([m_s * m_s * _from_fixed(int(v), gs.e) / n_s for v in s2]) - mean * mean
    with np.errstate(divide="ignore", invalid="ignore"):
        prm = ref.params_from_moments(mean, var, sum_sf, n_s, float(gs.genes), zeta)
    prm.update(median_total=m_s, sum_size_factors=sum_sf, n_cells_a=len(ua), n_cells_b=len(ub))
    fa, fb = float(gs.u_sum[a]) / m_s, float(gs.u_sum[b]) / m_s
    sa = np.array([int(v) for v in gs.col(gs.x, a)], dtype=np.uint64)
    sb = np.array([int(v) for v in gs.col(gs.x, b)], dtype=np.uint64)
    return prm, de_from_sums(sa, sb, fa, fb, prm, big_count, backend)


_CACHE = {}


def case_results(idx, backend=LOGSPACE):
    """(case, [literal (params, result) per pair], [fused (params, result) per pair]) of CASES[idx], computed once per process."""
    key = (idx, backend)
    if key not in _CACHE:
        case = make_case(*CASES[idx])
        gs = GroupSums(case["mat"], case["labels"], case["n_groups"])
        lit = [literal_pair(case["mat"], case["labels"], a, b, backend=backend) for a, b in case["pairs"]]
        fus = [fused_pair(gs, a, b, backend=backend) for a, b in case["pairs"]]
        _CACHE[key] = (case, lit, fus)
    return _CACHE[key]
