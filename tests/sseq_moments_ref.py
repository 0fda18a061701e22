"""Reference side of the sSeq moment tests (tests/test_sseq_moments_cpu.py, tests/test_gpu_sseq_moments.py). No GPU, no library.

`compute_sseq_params` (diff_exp.rs:458-500) turns the counts into per-gene moments of x / sf_c and those into the dispersions. Its
only floating-point sums are the two moments; tests/sseq_ref.py forms them in f64 and cannot say which of two f64 answers is right.
Here they are exact:

  exact_moments       the size factors as sseq_ref.size_factors gives them (f64 by definition), the f64 terms t = fl(x / sf_c) and
                      fl(t t) that the reference and the kernels both form, S1 = Σ t and S2 = Σ fl(t t) as exact rationals
                      (fractions.Fraction), mean = S1 / m and var = S2 / m - mean² in mpmath at 400 bits
  exact_params        sseq_params_from_moments (diff_exp.rs:377-456) evaluated at 400 bits from those moments
  emulate             the library's accumulation restated with Python integers: the scale rule, to_fixed, the exact integer sum,
                      from_fixed and the f64 expressions of sseq_host.cpp behind it. rule="single": one quantum for all genes from
                      the global bound m max_count max(1/sf), always (what the tests prove their grid adversarial with); rule="library": that
                      quantum only where the smallest possible term keeps 40 / 33 bits under it, else a quantum per gene from the
                      class of its largest term (fixed128.hpp)
  pairs_exact / pairs_emulate   the same for sseq_de_pairs: terms fl(x / u_c) under fixed_scale(cells), combined per pair as
                      pairs_moments_kernel does (mean = m_S S1 / n_S, var = m_S² S2 / n_S - mean²)
  contract_ratios     error / bound per gene for the moment contract; downstream_bounds carries it through the formulas

The contract (the project's numbers: the column moments' rule, tests/test_gpu_subset.py, tests/test_gpu_sseq_pairs.py):
  |S1 - exact| <= TOL_SUM S1, |mean - exact| <= TOL_SUM mean, |var - exact| <= TOL_VAR S2 / m,
use_genes (var > 0) equal wherever the exact var >= USE_POSED S2 / m."""
import math
from fractions import Fraction

import mpmath
import numpy as np
from scipy import sparse

import sseq_ref as ref

MP = mpmath.mp.clone()
MP.prec = 400  # 120 digits

TOL_SUM = 1e-12
TOL_VAR = 1e-10
USE_POSED = 1e-9
U = 2.0 ** -53  # unit roundoff of f64

KEEP_BITS_1, KEEP_BITS_2 = 40, 33  # fixed128.hpp: FX_KEEP_BITS_*
CLASS_CLAMP = 440  # FX_CLASS_CLAMP


def _mpf(fr):
    return MP.mpf(fr.numerator) / MP.mpf(fr.denominator)


def labelled_terms(mat, cell_indices=None, umi_counts=None):
    """(sf, m, genes, gene index, f64 term t = fl(x / sf_c)) of every nonzero in a selected cell; NaN factors read as 0."""
    mat = sparse.csc_matrix(mat)
    genes, cells = mat.shape
    with np.errstate(divide="ignore", invalid="ignore"):
        sf = ref.size_factors(mat, cell_indices, umi_counts)
    sel = np.arange(cells) if cell_indices is None else np.asarray(cell_indices)
    sub = mat[:, sel].tocoo()
    safe = np.where(np.isnan(sf), 0.0, sf)[sel]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = sub.data.astype(np.float64) / safe[sub.col]
    return sf, len(sel), genes, sub.row.astype(np.int64), t


def _exact_from_terms(genes, g_idx, t):
    s1, s2, bad, n = [Fraction(0)] * genes, [Fraction(0)] * genes, [False] * genes, [0] * genes
    with np.errstate(over="ignore"):
        tt = t * t
    for g, a, b in zip(g_idx.tolist(), t.tolist(), tt.tolist()):
        if not math.isfinite(a):
            bad[g] = True
            continue
        s1[g] += Fraction(a)
        s2[g] += Fraction(b)
        n[g] += 1
    return s1, s2, bad, n


def _moments(s1, s2, bad, m, w1=1, w2=1):
    """mean = w1 S1 / m, var = w2 S2 / m - mean² (mpf); a gene with a non-finite term: mean = inf, var = nan, as the reference's f64 gives"""
    mm = MP.mpf(m)
    mean, var, q = [], [], []
    for a, b, x in zip(s1, s2, bad):
        if x:
            mean.append(MP.inf)
            var.append(MP.nan)
            q.append(MP.nan)
            continue
        mu = w1 * _mpf(a) / mm
        ex2 = w2 * _mpf(b) / mm
        mean.append(mu)
        var.append(ex2 - mu * mu)
        q.append(ex2)
    return mean, var, q


def exact_moments(mat, cell_indices=None, umi_counts=None):
    """dict: sf (f64), m, S1, S2 (Fraction per gene), bad, n_terms, mean, var, ex2 = S2 / m (mpf), sum_sf = Σ 1 / sf over sf != 0 (mpf)."""
    sf, m, genes, g_idx, t = labelled_terms(mat, cell_indices, umi_counts)
    s1, s2, bad, n = _exact_from_terms(genes, g_idx, t)
    mean, var, q = _moments(s1, s2, bad, m)
    sum_sf = MP.mpf(0)
    for v in sf.tolist():
        if v != 0.0 and not math.isnan(v):
            sum_sf += 1 / MP.mpf(v)
    return dict(sf=sf, m=m, genes=genes, S1=s1, S2=s2, bad=bad, n_terms=n, mean=mean, var=var, ex2=q, sum_sf=sum_sf)


def _percentile(vals, pct):
    """stat.rs:140-162 in mpf"""
    s = sorted(vals)
    if len(s) == 1:
        return s[0]
    if pct == 100.0:
        return s[-1]
    rank = MP.mpf(pct) / 100 * (len(s) - 1)
    lr = MP.floor(rank)
    n = int(lr)
    return s[n] + (s[n + 1] - s[n]) * (rank - lr)


def exact_params(mom, zeta_quintile=0.995, n_genes=None):
    """diff_exp.rs:377-456 at 400 bits. dict: use (list of bool), gene_moment_phi, gene_phi (mpf lists), zeta_hat, delta, a, b, mean_phi."""
    mean, var, f, n = mom["mean"], mom["var"], mom["sum_sf"], MP.mpf(mom["m"])
    big_g = MP.mpf(len(var) if n_genes is None else n_genes)
    use = [bool(v > 0) for v in var]  # nan > 0 is False
    phi = [max(MP.mpf(0), (n * v - mu * f) / (mu * mu * f)) if u else MP.mpf(0) for mu, v, u in zip(mean, var, use)]
    used = [p for p, u in zip(phi, use) if u]
    zh = dl = a = b = mphi = MP.mpf(0)
    if used:
        zh = _percentile(used, 100.0 * zeta_quintile)
        mphi = sum(used) / len(used)
        a = sum((x - mphi) ** 2 for x in used)
        b = sum((x - zh) ** 2 for x in used)
        dl = (a / (big_g - 1)) / (b / (big_g - 2)) if b != 0 else MP.nan
    cond = any(x > 0 for x in used)
    gphi = [(1 - dl) * p + dl * zh if (cond and u) else MP.mpf(0) for p, u in zip(phi, use)]
    return dict(use=use, gene_moment_phi=phi, gene_phi=gphi, zeta_hat=zh, delta=dl, a=a, b=b, mean_phi=mphi, n_used=len(used), n_genes=big_g)


_EXACT = {}


def exact_variant(name, vname):
    """(moments, params, bounds) of a variant of tests/sseq_moments_cases.py, computed once and shared by the tests"""
    import sseq_moments_cases as mc

    if (name, vname) not in _EXACT:
        v = mc.variant(name, vname)
        mom = exact_moments(mc.case(name)["mat"], v["cell_indices"], v["umi_counts"])
        par = exact_params(mom)
        _EXACT[(name, vname)] = (mom, par, downstream_bounds(mom, par))
    return _EXACT[(name, vname)]


def worst_ratios(mom, par, bounds, got):
    """(the largest error / bound per quantity, the genes whose use flag counts and differs) of a result: a dict as
    sseq_ref.params_from_moments returns it, or the library's SSeqParams"""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))
    s1 = got.get("S1") if isinstance(got, dict) else None
    r = contract_ratios(mom, get("gene_means"), get("gene_variances"), s1)
    worst = dict(mean=max(r["mean"]), var=max(r["var"]), S1=max(r["S1"], default=0.0))
    worst.update(downstream_ratios(par, bounds, got))
    return worst, use_mismatches(mom, par, get("use_genes"))


# ---- the bounds ----------------------------------------------------------------------------------------------------------------------
def use_posed(mom):
    """per gene: the sign of var is well posed (exact var >= USE_POSED S2 / m, or the gene has no finite variance at all: bad, or no term)"""
    out = []
    for v, q, bad, n in zip(mom["var"], mom["ex2"], mom["bad"], mom["n_terms"]):
        out.append(True if (bad or n == 0) else bool(v >= USE_POSED * q))
    return out


def downstream_bounds(mom, par, zeta_quintile=0.995):
    """The moment contract carried to first order through sseq_params_from_moments, plus the rounding of an f64 evaluation (U = 2^-53).
    With em = TOL_SUM mean_g and ev = TOL_VAR S2_g / m the errors allowed in a gene's moments, F = Σ 1/sf, n = m, G = the gene count:

      phi_g = max(0, n var / (mean² F) - 1 / mean):  d phi = n ev / (mean² F) + em (2 n |var| / (mean³ F) + 1 / mean²)
            = n TOL_VAR (S2/m) / (mean² F) + TOL_SUM (2 n |var| / (mean² F) + 1 / mean)                       (max(0, .) is 1-Lipschitz)
        rounding: six f64 operations on the two parts and F itself, a plain f64 sum of m rounded quotients (relative (m + 1) U):
            (8 + m) U n |var| / (mean² F) + 8 U / mean
      zeta_hat: an interpolation between two order statistics of the used phi, each 1-Lipschitz in the largest change of any phi:
            d zeta = max over the used genes of d phi, + 4 U |zeta_hat| for the interpolation
      mean_phi: d = the mean of d phi
      a = Σ (phi - mean_phi)²:  da = 2 Σ |phi - mean_phi| (d phi + d mean_phi);  b = Σ (phi - zeta)²:  db = 2 Σ |phi - zeta| (d phi + d zeta)
      delta = (a / (G - 1)) / (b / (G - 2)):  d delta = (da / (G - 1)) / (b / (G - 2)) + delta db / b, + 2 (n_used + 6) U delta for the
            two f64 sums of n_used non-negative terms and the divisions
      gene_phi = (1 - delta) phi + delta zeta:  d = |1 - delta| d phi + (|phi| + |zeta|) d delta + |delta| d zeta + 4 U (|(1 - delta) phi| + |delta zeta|)

    zeta_hat, delta and gene_phi are defined only through the SET of used genes, so they are compared only where every gene's use flag
    is well posed (use_posed), and where b is not within 1e-6 of zero relative to Σ phi² (the issue's condition): `compare_shrink`."""
    mean, var, q, f, n = mom["mean"], mom["var"], mom["ex2"], mom["sum_sf"], MP.mpf(mom["m"])
    m = mom["m"]
    use, phi = par["use"], par["gene_moment_phi"]
    dphi = []
    for mu, v, ex2, u in zip(mean, var, q, use):
        if not u:
            dphi.append(MP.mpf(0))
            continue
        lead = n * abs(v) / (mu * mu * f)
        dphi.append(n * TOL_VAR * ex2 / (mu * mu * f) + TOL_SUM * (2 * lead + 1 / mu) + (8 + m) * U * lead + 8 * U / mu)
    used = [i for i, u in enumerate(use) if u]
    out = dict(gene_moment_phi=dphi, zeta_hat=MP.mpf(0), delta=MP.mpf(0), gene_phi=[MP.mpf(0)] * len(use), compare_shrink=False)
    if not used:  # no gene with variance: zeta_hat = delta = 0 exactly (the zero bounds ask for equality), if that much is posed
        out["compare_shrink"] = bool(all(use_posed(mom)))
        return out
    zh, dl, a, b, mphi, big_g = par["zeta_hat"], par["delta"], par["a"], par["b"], par["mean_phi"], par["n_genes"]
    dz = max(dphi[i] for i in used) + 4 * U * abs(zh)
    dmphi = sum(dphi[i] for i in used) / len(used)
    sum_sq = sum(phi[i] ** 2 for i in used)
    out["zeta_hat"] = dz
    out["compare_shrink"] = bool(all(use_posed(mom)) and sum_sq > 0 and b > 1e-6 * sum_sq)
    if not out["compare_shrink"]:
        return out
    da = 2 * sum(abs(phi[i] - mphi) * (dphi[i] + dmphi) for i in used)
    db = 2 * sum(abs(phi[i] - zh) * (dphi[i] + dz) for i in used)
    dd = (da / (big_g - 1)) / (b / (big_g - 2)) + abs(dl) * db / b + 2 * (len(used) + 6) * U * abs(dl)
    out["delta"] = dd
    out["gene_phi"] = [abs(1 - dl) * dphi[i] + (abs(phi[i]) + abs(zh)) * dd + abs(dl) * dz + 4 * U * (abs((1 - dl) * phi[i]) + abs(dl * zh)) if use[i]
                       else MP.mpf(0) for i in range(len(use))]
    return out


def contract_ratios(mom, mean, var, s1=None):
    """error / bound per gene for a result's mean and var (f64 arrays), and for its S1 where given: dict of lists; a gene with a
    non-finite term must come back as (inf, nan) exactly and reads 0.0 if so, inf otherwise. A bound of 0 (no term) asks for equality."""
    def ratio(err, bound):
        if bound == 0:
            return 0.0 if err == 0 else math.inf
        return float(err / bound)

    out = dict(mean=[], var=[], S1=[])
    for g in range(mom["genes"]):
        if mom["bad"][g]:
            ok = math.isinf(float(mean[g])) and float(mean[g]) > 0 and math.isnan(float(var[g]))
            out["mean"].append(0.0 if ok else math.inf)
            out["var"].append(0.0 if ok else math.inf)
            out["S1"].append(0.0)
            continue
        if not (math.isfinite(float(mean[g])) and math.isfinite(float(var[g]))):
            out["mean"].append(math.inf)
            out["var"].append(math.inf)
            out["S1"].append(math.inf)
            continue
        out["mean"].append(ratio(abs(MP.mpf(float(mean[g])) - mom["mean"][g]), TOL_SUM * mom["mean"][g]))
        out["var"].append(ratio(abs(MP.mpf(float(var[g])) - mom["var"][g]), TOL_VAR * mom["ex2"][g]))
        if s1 is not None:
            e = _mpf(mom["S1"][g])
            out["S1"].append(ratio(abs(MP.mpf(float(s1[g])) - e), TOL_SUM * e))
    return out


def use_mismatches(mom, par, use_got):
    """the genes whose use flag counts (use_posed) and differs"""
    return [g for g, (p, e) in enumerate(zip(use_posed(mom), par["use"])) if p and bool(use_got[g]) != e]


def downstream_ratios(par, bounds, got):
    """error / bound for gene_moment_phi, gene_phi (worst gene), zeta_hat, delta; `got`: anything with those attributes or keys (f64)."""
    get = (lambda k: got[k]) if isinstance(got, dict) else (lambda k: getattr(got, k))

    def ratio(err, bound):
        if not MP.isfinite(err):
            return math.inf
        if bound == 0:
            return 0.0 if err == 0 else math.inf
        return float(err / bound)

    out = {}
    # a gene out of use_genes has a dispersion of exactly 0, wherever its flag is posed (a zero bound asks for equality)
    out["unused_zero"] = max((ratio(abs(MP.mpf(float(get(f)[g]))), 0) for f in ("gene_moment_phi", "gene_phi")
                              for g in range(len(par["use"])) if not par["use"][g] and not bool(get("use_genes")[g])), default=0.0)
    out["gene_moment_phi"] = max((ratio(abs(MP.mpf(float(get("gene_moment_phi")[g])) - par["gene_moment_phi"][g]), bounds["gene_moment_phi"][g])
                                  for g in range(len(par["use"])) if par["use"][g]), default=0.0)
    if bounds["compare_shrink"]:
        out["zeta_hat"] = ratio(abs(MP.mpf(float(get("zeta_hat"))) - par["zeta_hat"]), bounds["zeta_hat"])
        out["delta"] = ratio(abs(MP.mpf(float(get("delta"))) - par["delta"]), bounds["delta"])
        out["gene_phi"] = max((ratio(abs(MP.mpf(float(get("gene_phi")[g])) - par["gene_phi"][g]), bounds["gene_phi"][g])
                               for g in range(len(par["use"])) if par["use"][g]), default=0.0)
    return out


# ---- the library's accumulation in Python integers ---------------------------------------------------------------------------------
def fixed_scale_exp(bound):
    """fixed128.hpp fixed_scale: E with scale = 2^E, bound 2^E < 2^124 (0 for a bound that is not positive and finite)"""
    if not (bound > 0.0) or not math.isfinite(bound):
        return 0
    return 124 - (math.frexp(bound)[1] - 1) - 1


def _ldexp(x, e):
    try:
        return math.ldexp(x, e)
    except OverflowError:
        return math.inf


def to_fixed(t, e):
    """to_fixed(t, 2^e) as an integer: t 2^e is exact in f64 (short of under- and overflow), then rounded half to even"""
    y = _ldexp(t, e)
    return round(Fraction(y))


def from_fixed(n, e):
    """from_fixed: ((double)hi 2^64 + (double)lo) / 2^e in f64"""
    hi, lo = n >> 64, n & 0xFFFFFFFFFFFFFFFF
    return _ldexp(float(hi) * 18446744073709551616.0 + float(lo), -e)


def term_class(t):
    if not (t > 0.0):
        return 0
    e = math.frexp(t)[1] - 1
    if t < 2.0 ** -1022:
        e = -1023
    return min(max(e, -CLASS_CLAMP), CLASS_CLAMP) + CLASS_CLAMP + 1


def log2_ceil(m):
    l = 0
    while (1 << l) < m:
        l += 1
    return l


def single_quantum_keeps(tmin, e1, e2):
    """fixed128.hpp fixed_single_quantum_keeps, in its f64 arithmetic"""
    with np.errstate(over="ignore", under="ignore"):
        return bool(np.float64(tmin) * np.float64(_ldexp(1.0, e1)) >= 2.0 ** KEEP_BITS_1 and
                    np.float64(tmin) * np.float64(tmin) * np.float64(_ldexp(1.0, e2)) >= 2.0 ** KEEP_BITS_2)


def emulate(mat, cell_indices=None, umi_counts=None, rule="library", zeta_quintile=0.995):
    """sseq_params (sseq_host.cpp) without a device: dict with mean, var, S1 (f64 arrays), route ("single" / "per_gene"), e1, e2 (the
    single quantum's exponents) and the parameters sseq_ref.params_from_moments makes of them."""
    mat = sparse.csc_matrix(mat)
    sf, m, genes, g_idx, t = labelled_terms(mat, cell_indices, umi_counts)
    sel = np.arange(mat.shape[1]) if cell_indices is None else np.asarray(cell_indices)
    safe = np.where(np.isnan(sf), 0.0, sf)[sel]
    pos = safe[(safe > 0.0) & np.isfinite(safe)]  # an infinite factor makes terms of exactly 0
    with np.errstate(over="ignore"):
        max_inv = float(np.max(1.0 / pos)) if pos.size else 0.0
        min_inv = float(np.min(1.0 / pos)) if pos.size else math.inf
        max_count = float(mat.data.max()) if mat.nnz else 0.0
        b1 = float(np.float64(m) * np.float64(max_count) * np.float64(max_inv))
        b2 = float(np.float64(b1) * np.float64(max_count) * np.float64(max_inv))
    e1, e2 = fixed_scale_exp(b1), fixed_scale_exp(b2)
    per_gene = rule == "library" and not single_quantum_keeps(min_inv, e1, e2)
    with np.errstate(over="ignore"):
        tt = t * t
    lm = log2_ceil(m)
    cls = [0] * genes
    if per_gene:
        for g, a in zip(g_idx.tolist(), t.tolist()):
            if math.isfinite(a):
                cls[g] = max(cls[g], term_class(a))
    ex1 = [(122 - lm - (k - CLASS_CLAMP - 1)) if (per_gene and k) else (0 if per_gene else e1) for k in cls]
    ex2 = [(121 - lm - 2 * (k - CLASS_CLAMP - 1)) if (per_gene and k) else (0 if per_gene else e2) for k in cls]
    a1, a2, bad = [0] * genes, [0] * genes, [False] * genes
    for g, a, b in zip(g_idx.tolist(), t.tolist(), tt.tolist()):
        if not math.isfinite(a):
            bad[g] = True
            continue
        a1[g] += to_fixed(a, ex1[g])
        a2[g] += to_fixed(b, ex2[g])
    assert max(a1 + a2 + [0]) < 1 << 128, "a sum left the 128-bit accumulator"
    md = np.float64(m)
    s1 = np.array([from_fixed(a, e) for a, e in zip(a1, ex1)], dtype=np.float64)
    s2 = np.array([from_fixed(a, e) for a, e in zip(a2, ex2)], dtype=np.float64)
    mean = s1 / md
    var = s2 / md - mean * mean
    mean[bad], var[bad] = np.inf, np.nan
    sum_sf = 0.0
    for v in sf.tolist():  # the host's fold, in cell order
        if v != 0.0:
            sum_sf += 1.0 / v
    par = ref.params_from_moments(mean, var, sum_sf, float(m), float(genes), zeta_quintile)
    par.update(S1=s1, route="per_gene" if per_gene else "single", e1=e1, e2=e2, size_factors=sf)
    return par


# ---- the pairs form (sseq_pairs_host.cpp, pairs_moments_kernel) ---------------------------------------------------------------------
def _pair_setup(mat, labels, pair):
    mat = sparse.csc_matrix(mat)
    labels = np.asarray(labels)
    tot = np.asarray(mat.sum(axis=0), dtype=np.uint64).ravel()
    sel = np.flatnonzero((labels == pair[0]) | (labels == pair[1]))
    m_s = ref.median(tot[sel].astype(np.float64))  # the interpolated median of the union's totals, in f64 as the header kernel takes it
    sub = mat[:, sel].tocoo()
    u = tot[sel].astype(np.float64)[sub.col]
    t = sub.data.astype(np.float64) / u  # a nonzero's cell has a positive total
    return mat, len(sel), float(m_s), sub.row.astype(np.int64), t


def pairs_exact(mat, labels, pair):
    """the exact moments of one pair's union S: mean = m_S S1 / n_S, var = m_S² S2 / n_S - mean², S1 = Σ fl(x / u_c), S2 = Σ fl(t t); the
    dict of exact_moments with ex2 = m_S² S2 / n_S and sum_sf = m_S Σ 1 / u_c (exact)"""
    mat, n_s, m_s, g_idx, t = _pair_setup(mat, labels, pair)
    genes = mat.shape[0]
    s1, s2, bad, n = _exact_from_terms(genes, g_idx, t)
    w = MP.mpf(m_s)
    mean, var, q = _moments(s1, s2, bad, n_s, w, w * w)
    labels = np.asarray(labels)
    tot = np.asarray(mat.sum(axis=0), dtype=np.uint64).ravel()
    inv = sum((1 / MP.mpf(int(v)) for v, l in zip(tot.tolist(), labels.tolist()) if l in (pair[0], pair[1]) and v), MP.mpf(0))
    return dict(m=n_s, genes=genes, S1=s1, S2=s2, bad=bad, n_terms=n, mean=mean, var=var, ex2=q, sum_sf=w * inv, m_s=m_s)


def pairs_route(mat, labels, pair):
    """"batched" or "literal" (pairs_header_kernel): literal when the union's largest cell total does not keep a count of 1's bits under
    fixed_scale(cells) (fixed_totals_quantum_keeps), or its median total is 0"""
    mat = sparse.csc_matrix(mat)
    labels = np.asarray(labels)
    tot = np.asarray(mat.sum(axis=0), dtype=np.uint64).ravel()
    sel = np.flatnonzero((labels == pair[0]) | (labels == pair[1]))
    top = int(tot[sel].max())
    e = fixed_scale_exp(float(mat.shape[1]))
    if ref.median(tot[sel].astype(np.float64)) == 0.0 or (top and not single_quantum_keeps(1.0 / float(top), e, e)):
        return "literal"
    return "batched"


def pairs_emulate(mat, labels, pair, rule="library"):
    """mean, var (f64 arrays) of one pair as the library accumulates them: both sums under fixed_scale(cells) (rule="single": always;
    rule="library": a literal pair is compute_sseq_params over the union's cells, see `emulate`)"""
    if rule == "library" and pairs_route(mat, labels, pair) == "literal":
        labels = np.asarray(labels)
        em = emulate(mat, np.flatnonzero((labels == pair[0]) | (labels == pair[1])), None, "library")
        return dict(mean=em["gene_means"], var=em["gene_variances"], e=None, route="literal")
    mat, n_s, m_s, g_idx, t = _pair_setup(mat, labels, pair)
    genes, cells = mat.shape
    e = fixed_scale_exp(float(cells))
    a1, a2 = [0] * genes, [0] * genes
    for g, a, b in zip(g_idx.tolist(), t.tolist(), (t * t).tolist()):
        a1[g] += to_fixed(a, e)
        a2[g] += to_fixed(b, e)
    ms, ns = np.float64(m_s), np.float64(n_s)
    mean = np.array([ms * np.float64(from_fixed(a, e)) / ns for a in a1], dtype=np.float64)
    var = np.array([ms * ms * np.float64(from_fixed(a, e)) / ns for a in a2], dtype=np.float64) - mean * mean
    return dict(mean=mean, var=var, e=e, route="batched")
