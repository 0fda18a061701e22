"""The cases of the sSeq moment tests, shared by tests/test_sseq_moments_cpu.py and tests/test_gpu_sseq_moments.py.

A case is a small genes x cells count matrix (uint32, scipy CSR) with a list of variants, each the arguments of one
compute_sseq_params call: `cell_indices` (a selection: the other cells are skipped) and `umi_counts`. What goes wrong in a
fixed-point sum depends on the exponents of its terms, not on its length, so the shapes are tiny: genes <= 128 and cells <= 4096,
but for pairs_total_2^40, whose cell total of 2^40 takes 257 counts of u32 size (265 genes).

  benign                  tests/test_gpu_sseq.py::test_params_synthetic's distribution: geometric counts, umi_counts in U(50, 400)
  one_huge_count          one count of 4e9 in cell 0, a gene with a single count of 1 in that cell, genes with counts in ordinary cells only
  raw_like                most cells of total 1 - 3, six of total ~1e5 with a count ~6e4; genes seen once, only in the large cells
  umi_spread_1e3/1e6/1e12 umi_counts in two clusters that ratio apart, the median in the small or in the large cluster; genes expressed only
                          in the large-factor cells, only in the small-factor cells, and in both
  huge_count_and_spread   one_huge_count's matrix under umi_counts spread over 1e3
  single_nonzero_genes    one nonzero per gene, counts 1 and 2^32 - 1
  constant_gene           power-of-two size factors and a gene with x / sf equal in every selected cell: its exact variance is 0, so the
                          sign of its variance is not posed; its contract is |var| <= bound only
  zero_factor             a selected cell with umi_counts 0 and nonzeros in it: the non-finite path (mean = inf, var = NaN)
  wave_edges              gene lengths 0, 1, 63, 64, 65, 129 in turn over 128 genes: the edges of a 64-lane wave's loop over a gene. A
                          launch covers 65536 genes before a wave takes a second one, so the GPU file also runs it (and two cases of the
                          per-gene route) under the handle option "sseq_grid_cap" = 2: eight outer vectors per sweep of the grid
  pairs_total_2^34 / 2^40 for sseq_de_pairs: cell 0's total reaches that power through counts of 2^32 - 1, a gene has its only count, 1, in
                          that cell; three groups and all three pairs

`de`: the case also runs one one-vs-rest call (its counts are small enough for the exact test's term-by-term reference)."""
import functools

import numpy as np
from scipy import sparse

U32_MAX = 2 ** 32 - 1


def _geometric(genes, cells, density, seed):
    rng = np.random.default_rng(seed)
    m = sparse.random(genes, cells, density=density, format="csr", random_state=seed, data_rvs=lambda n: rng.geometric(0.3, n))
    return m.astype(np.uint32)


def _coo(genes, cells, rows, cols, vals):
    m = sparse.coo_matrix((np.asarray(vals, dtype=np.uint64), (np.asarray(rows), np.asarray(cols))), shape=(genes, cells)).tocsr()
    assert m.data.max() <= U32_MAX
    return m.astype(np.uint32)


def _variant(name, cells=None, umi=None):
    return dict(name=name, cell_indices=None if cells is None else np.asarray(cells, dtype=np.uint64),
                umi_counts=None if umi is None else np.asarray(umi, dtype=np.float64))


def _benign():
    m = _geometric(96, 700, 0.04, 5)
    rng = np.random.default_rng(9)
    sel = np.sort(rng.choice(700, 450, replace=False))
    return dict(mat=m, de=True, variants=[_variant("natural"), _variant("cells", sel), _variant("umi", None, rng.uniform(50, 400, 700)),
                                          _variant("cells+umi", sel, rng.uniform(50, 400, 450))])


def _huge_matrix():
    genes, cells = 40, 512
    base = _geometric(genes, cells, 0.1, 31).tolil()
    base[:, 0] = 0  # cell 0 holds the two special counts only
    base[0, :] = 0
    base[1, :] = 0
    base[0, 0] = 4_000_000_000
    base[1, 0] = 1
    m = base.tocsr().astype(np.uint32)
    m.eliminate_zeros()
    return m


def _one_huge_count():
    m = _huge_matrix()
    sel = np.concatenate([[0], np.arange(5, 512, 2)])
    return dict(mat=m, de=False, variants=[_variant("natural"), _variant("cells", sel)])


def _raw_like():
    genes, cells, n_big = 64, 2048, 6
    rng = np.random.default_rng(41)
    rows, cols, vals = [], [], []
    for c in range(n_big, cells):  # totals 1 - 3, single counts over the genes 0 .. 47
        k = int(rng.integers(1, 4))
        for g in rng.choice(48, k, replace=False):
            rows.append(g), cols.append(c), vals.append(1)
    for c in range(n_big):  # total ~1e5: one count ~6e4 in a gene 48 .. 55, the rest over the genes 0 .. 47
        rows.append(48 + c), cols.append(c), vals.append(int(rng.integers(55_000, 65_000)))
        for g in range(48):
            rows.append(g), cols.append(c), vals.append(int(rng.integers(500, 1200)))
    for g in range(56, 64):  # seen once, in a large cell
        rows.append(g), cols.append((g - 56) % n_big), vals.append(1)
    m = _coo(genes, cells, rows, cols, vals)
    sel = np.concatenate([np.arange(n_big), np.arange(n_big + 1, cells, 3)])
    # no one-vs-rest call: the p-values of the genes with a count ~6e4 in one cell underflow to 0, which no relative tolerance compares
    return dict(mat=m, de=False, variants=[_variant("natural"), _variant("cells", sel)])


def _umi_spread(ratio, seed):
    genes, cells = 48, 500
    a_end, m_end = 200, 300  # cells [0, 200): always the small cluster; [200, 300): either; [300, 500): always the large one
    rng = np.random.default_rng(seed)
    m = _geometric(genes, cells, 0.15, seed).tolil()
    m[0:16, 0:m_end] = 0  # genes 0 .. 15: only in the large-factor cells
    m[16:32, a_end:cells] = 0  # genes 16 .. 31: only in the small-factor cells
    m = m.tocsr().astype(np.uint32)
    m.eliminate_zeros()
    small = 100.0 * rng.uniform(1.0, 2.0, cells)
    lo = small.copy()
    lo[m_end:] *= ratio  # 300 small, 200 large: the median lies in the small cluster
    hi = small.copy()
    hi[a_end:] *= ratio  # 200 small, 300 large: in the large one
    sel = np.sort(rng.choice(cells, 330, replace=False))
    return dict(mat=m, de=True, variants=[_variant("natural"), _variant("median_small", None, lo), _variant("median_large", None, hi),
                                                 _variant("cells+median_large", sel, hi[sel])])


def _huge_count_and_spread():
    m = _huge_matrix()
    rng = np.random.default_rng(53)
    umi = 100.0 * rng.uniform(1.0, 2.0, 512)
    a, b = umi.copy(), umi.copy()
    a[:200] *= 1e3  # cell 0 among the large factors
    b[300:] *= 1e3  # cell 0 among the small ones
    return dict(mat=m, de=False, variants=[_variant("huge_in_large", None, a), _variant("huge_in_small", None, b)])


def _single_nonzero_genes():
    genes, cells = 64, 256
    rows = np.arange(genes)
    cols = 4 * (rows // 2) + 1  # two genes per occupied cell: a count of 1 and one of 2^32 - 1; the other cells are empty
    vals = np.where(rows % 2 == 0, 1, U32_MAX)
    m = _coo(genes, cells, rows, cols, vals)
    sel = np.unique(cols)
    rng = np.random.default_rng(61)
    # over all cells the median total is 0: every factor is infinite or NaN, every term exactly 0, whatever the quantum
    return dict(mat=m, de=False, variants=[_variant("cells", sel), _variant("cells+umi", sel, rng.uniform(50, 400, len(sel))), _variant("median_0")])


def _constant_gene():
    genes, cells = 48, 300
    m = _geometric(genes, cells, 0.1, 71).tolil()
    rng = np.random.default_rng(72)
    umi = np.full(cells, 2.0)
    umi[rng.choice(cells, 60, replace=False)] = 1.0
    umi[rng.choice(np.flatnonzero(umi == 2.0), 60, replace=False)] = 8.0  # 60 x 1, 180 x 2, 60 x 8: the median is 2, every factor a power of two
    m[0, :] = 0
    m = m.tocsr().astype(np.uint32)
    m.eliminate_zeros()
    m = m.tolil()
    for c in range(cells):
        m[0, c] = int(3 * umi[c])  # x / sf = 3 * 2 in every cell
    m = m.tocsr().astype(np.uint32)
    sel = np.flatnonzero(umi != 8.0)  # 60 x 1, 180 x 2: the median stays 2
    return dict(mat=m, de=True, variants=[_variant("umi", None, umi), _variant("cells+umi", sel, umi[sel])])


def _zero_factor():
    m = _geometric(64, 400, 0.08, 81)
    rng = np.random.default_rng(82)
    umi = rng.uniform(50, 400, 400)
    c0 = int(np.argmax(np.diff(sparse.csc_matrix(m).indptr)))  # a cell with nonzeros in several genes
    umi[c0] = 0.0
    sel = np.sort(np.unique(np.concatenate([[c0], rng.choice(400, 250, replace=False)])))
    return dict(mat=m, de=False, zero_cell=c0, variants=[_variant("umi", None, umi), _variant("cells+umi", sel, umi[sel])])


def _wave_edges():
    genes, cells = 128, 256
    rng = np.random.default_rng(91)
    lengths = [0, 1, 63, 64, 65, 129]
    rows, cols, vals = [], [], []
    for g in range(genes):
        n = lengths[g % len(lengths)]
        cc = rng.choice(cells, n, replace=False)
        rows += [g] * n
        cols += cc.tolist()
        vals += rng.geometric(0.3, n).tolist()
    m = _coo(genes, cells, rows, cols, vals)
    sel = np.sort(rng.choice(cells, 170, replace=False))
    return dict(mat=m, de=False, variants=[_variant("natural"), _variant("cells+umi", sel, rng.uniform(50, 400, 170))])


def _pairs_total(power, cells):
    n_top = -(-(2 ** power) // U32_MAX)  # counts of 2^32 - 1 that reach 2^power
    genes = max(40, n_top + 8)
    base = _geometric(genes, cells, 0.1, 100 + power).tolil()
    base[:, 0] = 0
    base[0, :] = 0
    for g in range(n_top):
        base[1 + g, 0] = U32_MAX
    base[0, 0] = 1  # gene 0: its only count, in the cell of the huge total
    m = base.tocsr().astype(np.uint32)
    m.eliminate_zeros()
    rng = np.random.default_rng(200 + power)
    labels = rng.integers(-1, 3, cells).astype(np.int16)
    labels[0] = 0
    assert int(m[:, 0].sum()) >= 2 ** power
    # the genes with a count of 2^32 - 1 have counts in every group: with big_count = 0 each of their tests takes the asymptotic branch
    # (an exact test would sum 2^32 terms)
    for j in range(3):
        assert (np.asarray(m[1:1 + n_top][:, labels == j].sum(axis=1)).ravel() > 0).all()
    return dict(mat=m, labels=labels, pairs=[(0, 1), (0, 2), (1, 2)], n_groups=3)


CASES = {
    "benign": _benign,
    "one_huge_count": _one_huge_count,
    "raw_like": _raw_like,
    "umi_spread_1e3": lambda: _umi_spread(1e3, 101),
    "umi_spread_1e6": lambda: _umi_spread(1e6, 102),
    "umi_spread_1e12": lambda: _umi_spread(1e12, 103),
    "huge_count_and_spread": _huge_count_and_spread,
    "single_nonzero_genes": _single_nonzero_genes,
    "constant_gene": _constant_gene,
    "zero_factor": _zero_factor,
    "wave_edges": _wave_edges,
}
PAIRS_CELLS = 4096  # fixed_scale(cells) = 2^111: a count of 1 over a total of 2^34 keeps 43 bits of its square, over 2^40 it keeps 31
def merge_total_case():
    """for merge_clusters' fused pass: cell 0 (in cluster 0) holds 257 counts of 2^32 - 1, a total above 2^40, and gene 0's only count;
    every other gene has a count in every cell, so that each cluster's sum is above merge_clusters' big_count of 900 and the genes
    with the huge counts take the asymptotic test (an exact one would sum 2^32 terms). Clusters 0 and 1 lie close in the scores."""
    rng = np.random.default_rng(311)
    n_top, sizes = 257, [700, 700, 648]
    genes, cells = n_top + 9, sum(sizes)
    counts = (rng.poisson(3.0, (genes, cells)) + 1).astype(np.uint64)
    counts[0, :] = 0
    counts[:, 0] = 0
    counts[0, 0] = 1
    counts[1:1 + n_top, 0] = U32_MAX
    labels = np.repeat(np.arange(3), sizes).astype(np.int16)
    for j in range(3):
        assert (counts[1:, labels == j].sum(axis=1) > 900).all()
    assert int(counts[:, 0].sum()) >= 2 ** 40
    x = np.concatenate([rng.standard_normal((700, 2)), rng.standard_normal((700, 2)) + 0.5, rng.standard_normal((648, 2)) + 30.0])
    return dict(mat=sparse.csr_matrix(counts.astype(np.uint32)), labels=labels, scores=x)


PAIRS_CASES = {
    "pairs_total_2^34": lambda: _pairs_total(34, PAIRS_CELLS),
    "pairs_total_2^40": lambda: _pairs_total(40, PAIRS_CELLS),
}
# constant_gene's constant gene; every other case decides use_genes for all of its genes
USE_LEFT_OUT_CAP = 0.10


@functools.lru_cache(maxsize=None)
def case(name):
    return (CASES.get(name) or PAIRS_CASES[name])()


def variant_ids():
    return [(name, v["name"]) for name in CASES for v in case(name)["variants"]]


def variant(name, vname):
    return next(v for v in case(name)["variants"] if v["name"] == vname)


def de_labels(name):
    """three groups and some cells in none, for the one-vs-rest call of a case"""
    cells = case(name)["mat"].shape[1]
    return np.random.default_rng(len(name)).integers(-1, 3, cells).astype(np.int16)
