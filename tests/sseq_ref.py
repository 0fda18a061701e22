"""CPU restatement of the reference's sSeq differential expression (diff-exp/src/{dist,stat,diff_exp,utils}.rs) with
numpy and scipy, the checker of the library's DE. Matrices are scipy.sparse, genes x cells. The exact test is evaluated
term by term (the reference's running recurrence written directly), its ln Γ differences without the cancellation of two large gammaln
values (gammaln_rise); `direct=True` gives the formula with gammaln of every argument."""
from __future__ import annotations

import numpy as np
from scipy import sparse
from scipy.special import betainc, betaincinv, gammaln

BIG_COUNT_DEFAULT = 900


# ---- dist.rs ----------------------------------------------------------------------------------------------------------------
def adjusted_pvalue_bh(p):
    """dist.rs:22-50: descending with NaNs first (stable), running minimum of p n/(n - rank), capped at 1."""
    p = np.asarray(p, dtype=np.float64)
    n = len(p)
    keyed = sorted(range(n), key=lambda i: (0, 0.0) if np.isnan(p[i]) else (1, -p[i]))
    out = np.zeros(n)
    mn = np.finfo(np.float64).max
    for idx, i in enumerate(keyed):
        v = p[i] * (n / (n - idx))
        if v < mn:
            mn = v
        out[i] = min(mn, 1.0)
    return out


def _stirling_tail(z):
    """ln Γ(z) - [(z - 1/2) ln z - z + 1/2 ln 2π] for z >= 15: the series B_2m / (2m (2m-1) z^(2m-1)), 8 terms"""
    t = 1.0 / (z * z)
    s = np.zeros_like(t)
    for c in (-3617.0 / 122400.0, 1.0 / 156.0, -691.0 / 360360.0, 1.0 / 1188.0, -1.0 / 1680.0, 1.0 / 1260.0, -1.0 / 360.0, 1.0 / 12.0):
        s = s * t + c
    return s / z


def gammaln_rise(y, k):
    """ln Γ(y + k) - ln Γ(y) for a scalar y > 0 and an array k >= 0 as one quantity. From y = 15 on Stirling's series gives the difference itself;
    gammaln(y + k) - gammaln(y) would carry an ulp of ln Γ(y) ~ y ln y, 5e-7 at y = 2e8, where the difference is of size k ln y. Below 15
    ln Γ(y) is small and the plain difference loses nothing."""
    k = np.asarray(k, dtype=np.float64)
    if y < 15.0:
        return gammaln(y + k) - gammaln(y)
    z = y + k
    return (y - 0.5) * np.log1p(k / y) + k * np.log(z) - k + _stirling_tail(z) - _stirling_tail(np.float64(y))


def log_prob_all(count, sa, sb, mu, r, direct=False):
    """dist.rs:259-310, term by term (k = 0 .. count). direct: with gammaln of every argument, as the reference writes the constant; otherwise
    (what the tests check the library with) the two ln Γ differences are taken as such, see gammaln_rise. tests/test_sseq_exact_cpu.py holds
    this form to the high-precision reference."""
    k = np.arange(count + 1, dtype=np.float64)
    j = count - k
    const = count * np.log(mu / (r + mu)) + (sa + sb) * np.log(r / (r + mu))
    if direct:
        add_total = const - gammaln(sa * r) - gammaln(sb * r)
        return gammaln(sa * r + k) + gammaln(sb * r + j) - gammaln(k + 1.0) - gammaln(j + 1.0) + add_total
    return (gammaln_rise(sa * r, k) - gammaln(k + 1.0)) + (gammaln_rise(sb * r, j) - gammaln(j + 1.0)) + const


def nb_exact_test(x_a, x_b, sf_a, sf_b, mu, phi, direct=False):
    """dist.rs:74-118."""
    if x_a + x_b == 0 or phi == 0.0 or sf_a == 0.0 or sf_b == 0.0:
        return 1.0
    lp = log_prob_all(int(x_a + x_b), sf_a, sf_b, mu, 1.0 / phi, direct)
    return _p_from_terms(lp, lp <= lp[int(x_a)])


def nb_exact_test_tie_bounds(x_a, x_b, sf_a, sf_b, mu, phi, rtol=1e-12):
    """(p without, p with) the terms at k != x_a that tie with the observed one to rtol: their side of `<=` is decided
    by rounding, in the reference too."""
    lp = log_prob_all(int(x_a + x_b), sf_a, sf_b, mu, 1.0 / phi)
    obs = lp[int(x_a)]
    tie = np.abs(lp - obs) <= rtol * abs(obs)
    lo = (lp <= obs) & ~tie
    lo[int(x_a)] = True
    return _p_from_terms(lp, lo), _p_from_terms(lp, (lp <= obs) | tie)


def _p_from_terms(lp, ext):
    max_all = lp.max()
    max_ext = lp[ext].max()
    s_all = np.log(np.sum(np.exp(lp - max_all))) + max_all
    s_ext = np.log(np.sum(np.exp(lp[ext] - max_ext))) + max_ext
    return float(np.exp(s_ext - s_all))


def nb_asymptotic_test(count_a, count_b, sf_a, sf_b, mu, phi):
    """dist.rs:226-257."""
    alpha = sf_a * mu / (1.0 + phi * mu)
    beta = (sf_b / sf_a) * alpha
    xa, xb = float(count_a), float(count_b)
    median = betaincinv(alpha, beta, 0.5)

    def cdf(a, b, x):
        return 0.0 if x < 0 else 1.0 if x > 1 else betainc(a, b, x)

    if (xa + 0.5) / (xa + xb) < median:
        return 2.0 * cdf(alpha, beta, (xa + 0.5) / (xa + xb))
    return 2.0 * cdf(beta, alpha, (xb + 0.5) / (xa + xb))


# ---- stat.rs ----------------------------------------------------------------------------------------------------------------
def exact_sum(v):
    """stat.rs:49-80: Shewchuk partials, added up in order."""
    partials = []
    for x in v:
        x = float(x)
        j = 0
        for i in range(len(partials)):
            y = partials[i]
            if abs(x) < abs(y):
                x, y = y, x
            hi = x + y
            lo = y - (hi - x)
            if lo != 0.0:
                partials[j] = lo
                j += 1
            x = hi
        if j >= len(partials):
            partials.append(x)
        else:
            partials[j] = x
            del partials[j + 1:]
    s = 0.0
    for p in partials:
        s += p
    return s


def mean(v):
    return exact_sum(v) / len(v)


def var(v, ddof):
    if len(v) < ddof:
        return 0.0
    m = mean(v)
    s = 0.0
    for x in v:
        s += (float(x) - m) * (float(x) - m)
    return s / (len(v) - ddof)


def percentile(v, pct):
    """stat.rs:116-162."""
    s = sorted(float(x) for x in v)
    if len(s) == 1:
        return s[0]
    if pct == 100.0:
        return s[-1]
    rank = (pct / 100.0) * (len(s) - 1)
    lr = np.floor(rank)
    d = rank - lr
    n = int(lr)
    return s[n] + (s[n + 1] - s[n]) * d


def median(v):
    return percentile(v, 50.0)


# ---- diff_exp.rs ------------------------------------------------------------------------------------------------------------
def size_factors(mat, cell_indices=None, umi_counts=None):
    """diff_exp.rs:314-332. mat: scipy.sparse genes x cells."""
    cells = mat.shape[1]
    col = np.asarray(mat.sum(axis=0), dtype=np.float64).ravel()
    if umi_counts is not None:
        counts = np.asarray(umi_counts, dtype=np.float64)
    else:
        counts = col if cell_indices is None else col[np.asarray(cell_indices)]
    med = median(counts)
    if cell_indices is None:
        return counts / med
    sf = np.zeros(cells)
    sf[np.asarray(cell_indices)] = counts / med
    return sf


def params_from_moments(mean_g, var_g, sum_size_factors, n_cells, n_genes, zeta_quintile):
    """diff_exp.rs:377-456."""
    mean_g, var_g = np.asarray(mean_g, dtype=np.float64), np.asarray(var_g, dtype=np.float64)
    use = var_g > 0
    phi_mm = np.zeros(len(var_g))
    used = []
    for i in range(len(var_g)):
        if use[i]:
            phi_mm[i] = max(0.0, (n_cells * var_g[i] - mean_g[i] * sum_size_factors) / (mean_g[i] * mean_g[i] * sum_size_factors))
            used.append(phi_mm[i])
    if used:
        zeta_hat = percentile(used, 100.0 * zeta_quintile)
        m = mean(used)
        a = 0.0
        for x in used:
            a += (x - m) * (x - m)
        b = 0.0
        for x in used:
            b += (x - zeta_hat) * (x - zeta_hat)
        delta = (a / (n_genes - 1.0)) / (b / (n_genes - 2.0))
    else:
        zeta_hat, delta = 0.0, 0.0
    cond = any(x > 0 for x in used)
    phi = np.where(cond & use, (1.0 - delta) * phi_mm + delta * zeta_hat, 0.0)
    return dict(gene_means=mean_g, gene_variances=var_g, use_genes=use, gene_moment_phi=phi_mm, zeta_hat=zeta_hat, delta=delta, gene_phi=phi)


def compute_sseq_params(mat, zeta_quintile=0.995, cell_indices=None, umi_counts=None):
    """diff_exp.rs:458-500 (moments: sqz mean_var_rows / mean_var_axis, E[x^2] - E[x]^2)."""
    mat = sparse.csc_matrix(mat)
    genes, cells = mat.shape
    sf = size_factors(mat, cell_indices, umi_counts)
    sel = np.arange(cells) if cell_indices is None else np.asarray(cell_indices)
    sub = mat[:, sel].tocoo()
    safe = np.where(np.isnan(sf), 0.0, sf)[sel]
    v = sub.data.astype(np.float64) / safe[sub.col]
    s1 = np.bincount(sub.row, weights=v, minlength=genes)
    s2 = np.bincount(sub.row, weights=v * v, minlength=genes)
    m = float(len(sel))
    mean_g = s1 / m
    var_g = s2 / m - mean_g ** 2
    sum_sf = float(np.sum(1.0 / sf[sf != 0]))
    out = params_from_moments(mean_g, var_g, sum_sf, m, float(genes), zeta_quintile)
    out["size_factors"] = sf
    return out


def de_from_sums(sums_a, sums_b, sf_a, sf_b, params, big_count=BIG_COUNT_DEFAULT):
    """diff_exp.rs:177-300."""
    sums_a, sums_b = np.asarray(sums_a, dtype=np.uint64), np.asarray(sums_b, dtype=np.uint64)
    mu, phi, use = params["gene_means"], params["gene_phi"], params["use_genes"]
    p = np.zeros(len(sums_a))
    for g in range(len(sums_a)):
        a, b = int(sums_a[g]), int(sums_b[g])
        if use[g] and a > big_count and b > big_count:
            p[g] = nb_asymptotic_test(a, b, sf_a, sf_b, mu[g], phi[g])
        else:
            p[g] = nb_exact_test(a, b, sf_a, sf_b, mu[g], phi[g])
    padj = p.copy()
    idx = np.flatnonzero(use)
    padj[idx] = adjusted_pvalue_bh(p[idx])
    l2 = np.log2((1 + sums_a).astype(np.float64) / (1.0 + sf_a)) - np.log2((1 + sums_b).astype(np.float64) / (1.0 + sf_b))
    mi = np.zeros(len(p)) if sf_a == 0 else sums_a.astype(np.float64) / sf_a
    mo = np.zeros(len(p)) if sf_b == 0 else sums_b.astype(np.float64) / sf_b
    return dict(sums_in=sums_a, sums_out=sums_b, p_values=p, adjusted_p_values=padj, log2_fold_change=l2, normalized_mean_in=mi,
                normalized_mean_out=mo)


def differential_expression(mat, cond_a, cond_b, params, big_count=BIG_COUNT_DEFAULT):
    """diff_exp.rs:122-175."""
    mat = sparse.csc_matrix(mat)
    sf = params["size_factors"]
    fa = 0.0
    for i in cond_a:
        fa += sf[i]
    fb = 0.0
    for i in cond_b:
        fb += sf[i]
    sa = np.asarray(mat[:, list(cond_a)].sum(axis=1), dtype=np.uint64).ravel()
    sb = np.asarray(mat[:, list(cond_b)].sum(axis=1), dtype=np.uint64).ravel()
    return de_from_sums(sa, sb, fa, fb, params, big_count)


def one_vs_rest(mat, labels, params, big_count=BIG_COUNT_DEFAULT, n_groups=None):
    """Each group against all other labelled cells (utils.rs:77-117 with -1 = in no group)."""
    labels = np.asarray(labels)
    n_groups = int(labels.max()) + 1 if n_groups is None else n_groups
    out = []
    for j in range(n_groups):
        a = np.flatnonzero(labels == j)
        b = np.flatnonzero((labels >= 0) & (labels != j))
        out.append(differential_expression(mat, a, b, params, big_count))
    return out
